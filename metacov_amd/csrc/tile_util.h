// What the tile modules (runs.hip, windows.hip, bases.hip) share: the HIP
// error macro (also engine.hip's, ecor.hip's, exp_gpu.hip's and
// bam_gpu.hip's) and the grow-only device array; the skeleton of a tile stage
// on the host (the handle base, the segment checks, the cut of a segment into
// tiles); on the device the one-workgroup prefix scan over per-tile counts, a
// tile's count of flagged positions and its ordered compaction offsets.  Only
// scan.hip keeps a copy of the macro of its own.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/metacov_amd.h"
#include "common.h"

#define HIP_TRY(expr)                                                          \
    do {                                                                       \
        hipError_t e_ = (expr);                                                \
        if (e_ != hipSuccess) {                                                \
            mc::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                          __FILE__, __LINE__);                                 \
            return MC_E_HIP;                                                   \
        }                                                                      \
    } while (0)

namespace mc {

// grow-only device array, kPadBytes of room behind the n elements asked for
template <typename T, size_t kPadBytes = 0>
struct Buf {
    T* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = std::max(n, (size_t)256);
        hipError_t e = hipMalloc(&p, want * sizeof(T) + kPadBytes);
        if (e == hipSuccess) cap = want;
        return e;
    }
    ~Buf() {
        if (p) (void)hipFree(p);
    }
};

// ---- the host side of a tile stage ------------------------------------------

constexpr int64_t kMaxPos = int64_t(1) << 40;       // a segment's end at most: mc_set_contigs' length bound

// What mc_runs, mc_windows and mc_bases are built on: the device, the stream
// every launch and copy of the handle goes to, kEvents timing events (a span
// of a *_timing call lies between two of them) and kPin pinned 8-byte words
// for the few words a call reads back.
template <int kEvents, int kPin>
struct StageHandle {
    static constexpr int kPinWords = kPin;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[kEvents] = {};
    unsigned long long* pin = nullptr;
    int mark(int e) {
        HIP_TRY(hipEventRecord(ev[e], stream));
        return MC_OK;
    }
    int elapsed(int from, int to, float* ms) {
        HIP_TRY(hipEventElapsedTime(ms, ev[from], ev[to]));
        return MC_OK;
    }
    // The last element of a scan (8 bytes at d_src) through pin[slot], behind what is on the stream.
    int read_total(const int64_t* d_src, int slot, int64_t* total) {
        HIP_TRY(hipMemcpyAsync(pin + slot, d_src, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        std::memcpy(total, pin + slot, 8);
        return MC_OK;
    }
    ~StageHandle() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        if (pin) (void)hipHostFree(pin);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// A new handle H (a StageHandle) on `device`, which becomes the current device.
template <typename H>
int stage_create(int device, H** out) {
    *out = nullptr;
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    MC_REQUIRE(device >= 0 && device < n_dev, MC_E_HIP, "no HIP device %d (%d present)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    H* h = new H();
    h->device = device;
    bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
              (H::kPinWords == 0 || hipHostMalloc((void**)&h->pin, H::kPinWords * sizeof(unsigned long long),
                                                  hipHostMallocDefault) == hipSuccess);
    for (auto& e : h->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    if (!ok) {
        delete h;
        mc::set_error("HIP stream / event creation failed");
        return MC_E_HIP;
    }
    *out = h;
    return MC_OK;
}

template <typename H>
int stage_destroy(H* h) {
    if (h) {
        (void)hipSetDevice(h->device);
        delete h;
    }
    return MC_OK;
}

inline int bad_segment_tid(int64_t s, int32_t tid) {
    mc::set_error("segment %lld: tid %d out of range", (long long)s, tid);
    return MC_E_INVALID;
}

inline int check_segment_range(int64_t s, const int64_t* start, const int64_t* end) {
    MC_REQUIRE(start[s] >= 0 && end[s] >= start[s] && end[s] <= kMaxPos, MC_E_INVALID,
               "segment %lld: bad range [%lld, %lld)", (long long)s, (long long)start[s], (long long)end[s]);
    return MC_OK;
}

// The depth vector of a ctx as a stage reads it: open() once per call, then
// segment() for each segment in turn, which leaves the segment's contig in
// off and ext (the contig looked up last is kept).
struct DepthSource {
    mc_ctx* ctx = nullptr;
    const int32_t* d = nullptr;
    int64_t total_len = 0;
    int32_t tid = 0;
    int64_t off = 0, ext = 0;
    bool have = false;
    // handle: the stage's name for mc_last_error; MC_E_STATE where the depth is not computed
    int open(mc_ctx* c, int device, const char* handle) {
        int dev = -1;
        if (int rc = mc_ctx_device(c, &dev)) return rc;
        MC_REQUIRE(dev == device, MC_E_INVALID, "ctx is on device %d, the %s handle on device %d", dev, handle,
                   device);
        ctx = c;
        return mc_depth_device(c, &d, &total_len);
    }
    int segment(int64_t s, const int32_t* tids, const int64_t* start, const int64_t* end) {
        if (!have || tids[s] != tid) {
            int64_t o = 0, e = 0;
            const int rc = mc_contig_offset(ctx, tids[s], &o, &e);
            if (rc == MC_E_INVALID) return bad_segment_tid(s, tids[s]);
            if (rc) return rc;
            MC_REQUIRE(o >= 0 && e >= 0 && o + e <= total_len, MC_E_STATE, "contig %d lies outside the depth vector",
                       tids[s]);
            tid = tids[s], off = o, ext = e, have = true;
        }
        return check_segment_range(s, start, end);
    }
    // elements of the 16-byte aligned window in front of depth-vector index `first`
    int lead(int64_t first) const { return (int)((reinterpret_cast<uintptr_t>(d + first) >> 2) & 3); }
    // the depth vector is complete (the stage's stream is another one)
    int ready() const { return mc_synchronize(ctx); }
};

// Cuts [a, end) into the pieces that become tiles and appends them to tiles:
// one entry piece(a, n) for each piece, in order, n at most tile - lead(a)
// positions and, but for the last piece, a multiple of unit (1: any length; a
// small window's length: whole windows).  unit is at most tile - 3, so that a
// piece is never empty; the table stays below 2^31 entries.
template <typename Tile, typename Lead, typename Piece>
int cut_tiles(std::vector<Tile>& tiles, int tile, int64_t a, int64_t end, int64_t unit, Lead lead, Piece piece) {
    MC_REQUIRE(unit >= 1 && unit <= tile - 3, MC_E_STATE, "cut unit %lld outside 1..%d", (long long)unit, tile - 3);
    while (a < end) {
        const int64_t n = std::min<int64_t>((tile - lead(a)) / unit * unit, end - a);
        tiles.push_back(piece(a, n));
        a += n;
        MC_REQUIRE(tiles.size() < (size_t)INT32_MAX, MC_E_RANGE, "more than 2^31 tiles of %d positions", tile);
    }
    return MC_OK;
}

// seg_tile[s] is the table's size when segment s was cut; seg_tile[S] = n_tiles.  An empty segment then
// takes the next non-empty one's first tile, so that a scan's base at seg_tile[s] is the segment's first output.
inline void close_seg_tile(std::vector<int64_t>& seg_tile, int64_t n_tiles, const int64_t* start,
                           const int64_t* end) {
    const int64_t S = (int64_t)seg_tile.size() - 1;
    seg_tile[S] = n_tiles;
    for (int64_t s = S - 1; s >= 0; --s)
        if (end[s] == start[s]) seg_tile[s] = seg_tile[s + 1];
}

// ---- the device side ----------------------------------------------------------

constexpr int kScanThreads = 1024;
constexpr int kScanWidth = kScanThreads * 4;        // entries per iteration of the scan

// dst[i] = sum of src[0, i) for i <= n, by ONE workgroup of kScanThreads
// threads, all of which call; the calls of a kernel follow one another.  An
// iteration sums kScanWidth = 2^12 entries in 32 bits, the carry across
// iterations is 64-bit.  The iteration's sum for each user:
//   runs.hip     run starts of a tile of 2^13 positions:            <= 2^25
//   bases.hip    sites, or a consensus column, of a tile of 2^11:   <= 2^23
//                inserted bases (at most 32 behind a position):     <= 2^28
//                insertion events, rows and calls: the events of a begin are
//                held to 2^31 - 1 in all (a batch's own, before that check,
//                to one per CIGAR word of the batch):                < 2^31
__device__ __forceinline__ void tile_scan(const int32_t* src, int64_t n, int64_t* dst) {
    __shared__ int32_t wsum[kScanThreads / 64];
    __shared__ int64_t carry_s;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int64_t i0 = 0; i0 < n; i0 += kScanWidth) {
        const int64_t i = i0 + 4 * (int64_t)t;
        const int64_t carry = carry_s;                      // (read here: its latency hides behind the loads)
        int32_t c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = i + k < n ? src[i + k] : 0;
        const int32_t mine = c[0] + c[1] + c[2] + c[3];
        int32_t inc = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t o = __shfl_up(inc, off, 64);
            if (lane >= off) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int32_t wbase = 0, total = 0;
        for (int w = 0; w < kScanThreads / 64; ++w) {
            if (w < wave) wbase += wsum[w];
            total += wsum[w];
        }
        int64_t b = carry + wbase + (inc - mine);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i + k < n) dst[i + k] = b;
            b += c[k];
        }
        __syncthreads();                                    // every thread has read carry_s and wsum
        if (t == 0) carry_s += total;
        __syncthreads();
    }
    if (t == 0) dst[n] = carry_s;
    __syncthreads();                // dst[] is visible to this workgroup; carry_s is free for the next call
}

// counts[blockIdx.x] = the bits set in the fm words of the workgroup's kWaves waves, all of whose threads call.
template <int kWaves>
__device__ __forceinline__ void tile_count(uint32_t fm, int32_t* __restrict__ counts) {
    __shared__ int32_t wsum[kWaves];
    int32_t c = __popc(fm);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t sum = 0;
        for (int i = 0; i < kWaves; ++i) sum += wsum[i];
        counts[blockIdx.x] = sum;
    }
}

// Ordered compaction of a tile whose thread t holds, in round r, the element
// r * 64 * kWaves + t: bit r of fm flags it.  out[r] = the tile's flagged
// elements before it, in (round, wave, lane) order, by ballot ranks per round
// and wave; meaningful where the bit is set.  All threads call.
template <int kWaves, int kRounds>
__device__ __forceinline__ void tile_offsets(uint32_t fm, int32_t (&out)[kRounds]) {
    __shared__ int32_t wcnt[kRounds][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t rank[kRounds];                                  // flagged elements of this round in lower lanes of the wave
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const unsigned long long m = __ballot((fm >> r) & 1);
        rank[r] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
        if (lane == 0) wcnt[r][wave] = __popcll(m);
    }
    __syncthreads();
    int32_t run = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        int32_t mine = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w == wave) mine = run;
            run += wcnt[r][w];
        }
        out[r] = mine + rank[r];
    }
}

}  // namespace mc
