// Per-base depth as runs: run-length compaction of the depth vector K2 left
// in HBM (the form bedtools genomecov -bg/-bga, mosdepth and samtools depth
// write; nothing in the reference, which reports region statistics only).
//
// For every segment (tid, start, end) of a call, in input order, the maximal
// runs of equal q(depth): q(d) = d, or with n_edges > 0 the number of edges
// <= d (mosdepth --quantize).  Positions past a contig's extent have depth 0
// and take part like any value.  A run never crosses a segment boundary.
//
// The host cuts every segment into tiles of at most kTile positions (a tile
// never spans two segments) and uploads the tile table.  Three launches, none
// of which waits on another workgroup:
//   A  runs_count_kernel  one workgroup per tile: run starts in the tile
//   B  runs_scan_kernel   ONE workgroup looping over kScanWidth tiles per
//                         iteration: exclusive int64 tile bases, then
//                         seg_first[s] = base of segment s's first tile
//   C  runs_emit_kernel   flags again, ranks from ballots per wave and the
//                         waves' totals through LDS, (start, value) scattered
//                         to base + rank
// The host reads the grand total (8 bytes) between B and C to size the output.
//
// Tile layout: 256 threads = 4 waves; wave w owns positions [2048 w, 2048 w +
// 2048) of the tile's 16-byte aligned window, in 8 rounds of 64 lanes x 4
// positions, so every wave load is 1 KiB contiguous (global_load_dwordx4) and
// run starts are ordered by (wave, round, lane, element).  A tile whose first
// position is not 16-byte aligned (sub-range segments, contig offsets) starts
// `lead` (1..3) elements into its window and holds at most kTile - lead
// positions; those and the elements around the extent are loaded one by one,
// guarded, so no load leaves [first, first + valid) of the tile, except the
// one predecessor element a non-first tile reads at first - 1.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/metacov_amd.h"
#include "common.h"
#include "tile_util.h"

namespace {

using mc::Buf;
using mc::kScanThreads;
using mc::kScanWidth;                               // tiles per iteration of pass B

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRounds = 8;                          // int4 loads per lane
constexpr int kTile = kThreads * 4 * kRounds;       // 8192 positions
constexpr int kWavePos = kTile / kWaves;            // 2048
constexpr int kMaxEdges = 16;

struct Tile {
    int64_t first;     // depth-vector index of the tile's first position
    int64_t rel;       // contig-relative position of it
    int32_t n;         // positions (lead + n <= kTile)
    int32_t valid;     // of them inside the contig's extent (a prefix)
    int32_t seg;
    int32_t flags;     // 1: first tile of its segment; 2: position rel - 1 is inside the extent
};
static_assert(sizeof(Tile) == 32, "tile table entry");

struct Edges {
    int32_t n;
    int32_t e[kMaxEdges];
};

template <bool Q>
__device__ __forceinline__ int32_t quant(int32_t d, const Edges& E) {
    if (!Q) return d;
    int32_t c = 0;
    for (int i = 0; i < E.n; ++i) c += E.e[i] <= d;
    return c;
}

// The calling lane's 32 values (q applied) and run-start flags (bit 4 r + k:
// element k of round r) of tile t.  lead: elements of the aligned window in
// front of the tile's first position.
template <bool Q>
__device__ __forceinline__ uint32_t tile_flags(const int32_t* __restrict__ d, const Tile& t,
                                               const Edges& E, int lead, int wave, int lane,
                                               int32_t (&qv)[kRounds][4]) {
    const int32_t* w = d + (t.first - lead);            // the window: 16-byte aligned
    int32_t edge = 0;                                   // lane 0: the value before the wave's first element
    // loads first (independent), then the flags
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int e0 = wave * kWavePos + (r * 64 + lane) * 4;   // window element of qv[r][0]
        const int p0 = e0 - lead;                               // tile position of it
        if (p0 >= 0 && p0 + 4 <= t.valid) {
            const int4 v = *reinterpret_cast<const int4*>(w + e0);
            qv[r][0] = v.x; qv[r][1] = v.y; qv[r][2] = v.z; qv[r][3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) qv[r][k] = (p0 + k >= 0 && p0 + k < t.valid) ? w[e0 + k] : 0;
        }
        if (r == 0 && lane == 0 && p0 - 1 >= 0 && p0 - 1 < t.valid) edge = w[e0 - 1];
    }
    int32_t prev = 0;                                   // the value at tile position -1
    if ((t.flags & 3) == 2) prev = d[t.first - 1];
    prev = quant<Q>(prev, E);
    const bool seg_first = t.flags & 1;
    uint32_t fm = 0;
    int32_t carry = quant<Q>(edge, E);                  // lane 0's predecessor of this round
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) qv[r][k] = quant<Q>(qv[r][k], E);
        const int p0 = wave * kWavePos + (r * 64 + lane) * 4 - lead;
        int32_t before = __shfl_up(qv[r][3], 1, 64);
        if (lane == 0) before = carry;
        carry = __shfl(qv[r][3], 63, 64);               // lane 0 of the next round follows lane 63 of this one
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = p0 + k;
            int32_t b = k ? qv[r][k - 1] : before;
            if (p == 0) b = prev;
            const bool f = p >= 0 && p < t.n && (qv[r][k] != b || (p == 0 && seg_first));
            fm |= (uint32_t)f << (4 * r + k);
        }
    }
    return fm;
}

__device__ __forceinline__ int lead_of(const int32_t* d, const Tile& t) {
    return (int)((reinterpret_cast<uintptr_t>(d + t.first) >> 2) & 3);
}

template <bool Q>
__global__ __launch_bounds__(kThreads) void runs_count_kernel(const int32_t* __restrict__ d,
                                                             const Tile* __restrict__ tiles, Edges E,
                                                             int32_t* __restrict__ counts) {
    const Tile t = tiles[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t qv[kRounds][4];
    mc::tile_count<kWaves>(tile_flags<Q>(d, t, E, lead_of(d, t), wave, lane, qv), counts);
}

// One workgroup.  base[i] = sum of counts[0, i) for i <= n_tiles, then
// seg_first[s] = base[seg_tile[s]] for s <= S (seg_tile[s]: the first tile of
// the first non-empty segment at or after s; n_tiles when there is none).
__global__ __launch_bounds__(kScanThreads) void runs_scan_kernel(const int32_t* __restrict__ counts,
                                                                int64_t n_tiles, int64_t* __restrict__ base,
                                                                const int64_t* __restrict__ seg_tile, int64_t S,
                                                                int64_t* __restrict__ seg_first) {
    mc::tile_scan(counts, n_tiles, base);
    for (int64_t s = threadIdx.x; s <= S; s += kScanThreads) seg_first[s] = base[seg_tile[s]];
}

template <bool Q>
__global__ __launch_bounds__(kThreads) void runs_emit_kernel(const int32_t* __restrict__ d,
                                                            const Tile* __restrict__ tiles, Edges E,
                                                            const int64_t* __restrict__ base,
                                                            int64_t* __restrict__ run_start,
                                                            int32_t* __restrict__ run_value) {
    __shared__ int32_t wsum[kWaves];
    const Tile t = tiles[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lead = lead_of(d, t);
    int32_t qv[kRounds][4];
    const uint32_t fm = tile_flags<Q>(d, t, E, lead, wave, lane, qv);
    // rank of each flagged element inside the wave, in (round, lane, element) order
    int32_t rank[kRounds];
    int32_t run = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        int32_t before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned long long m = __ballot((fm >> (4 * r + k)) & 1);
            before += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
            all += __popcll(m);
        }
        rank[r] = run + before;
        run += all;
    }
    if (lane == 0) wsum[wave] = run;
    __syncthreads();
    int64_t out = base[blockIdx.x];
    for (int w = 0; w < wave; ++w) out += wsum[w];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int p0 = wave * kWavePos + (r * 64 + lane) * 4 - lead;
        int64_t o = out + rank[r];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if ((fm >> (4 * r + k)) & 1) {
                run_start[o] = t.rel + p0 + k;
                run_value[o] = qv[r][k];
                ++o;
            }
        }
    }
}

}  // namespace

namespace {
enum { kEvCount, kEvScan, kEvScanEnd, kEvEmit, kEvEmitEnd, kEvents };   // the count pass ends where the scan begins
}

// pin[0]: the grand total, read between B and C
struct mc_runs : mc::StageHandle<kEvents, 1> {
    Buf<Tile> tiles;
    Buf<int32_t> counts;
    Buf<int64_t> base, seg_tile, seg_first, run_start;
    Buf<int32_t> run_value;
    bool computed = false;
    int64_t S = 0, n_runs = 0, n_tiles = 0;
    float ms[3] = {0, 0, 0};
};

extern "C" int mc_runs_create(int device, mc_runs** out) {
    MC_REQUIRE(out, MC_E_INVALID, "null argument");
    return mc::stage_create(device, out);
}

extern "C" int mc_runs_destroy(mc_runs* r) { return mc::stage_destroy(r); }

extern "C" int mc_runs_dims(int32_t* tile, int32_t* scan_width) {
    MC_REQUIRE(tile && scan_width, MC_E_INVALID, "null argument");
    *tile = kTile;
    *scan_width = kScanWidth;
    return MC_OK;
}

extern "C" int mc_runs_compute(mc_runs* r, mc_ctx* ctx, int64_t S, const int32_t* tid, const int64_t* start,
                               const int64_t* end, int32_t n_edges, const int32_t* edges, int64_t* n_runs) {
    MC_REQUIRE(r && ctx && n_runs, MC_E_INVALID, "null argument");
    MC_REQUIRE(S >= 0 && (S == 0 || (tid && start && end)), MC_E_INVALID, "bad segment arrays");
    MC_REQUIRE(n_edges >= 0 && n_edges <= kMaxEdges && (n_edges == 0 || edges), MC_E_INVALID,
               "%d quantisation edges outside 0..%d", n_edges, kMaxEdges);
    Edges E{};
    E.n = n_edges;
    for (int i = 0; i < n_edges; ++i) {
        MC_REQUIRE(edges[i] >= 0 && (i == 0 || edges[i] > edges[i - 1]), MC_E_INVALID,
                   "quantisation edges must be non-negative and strictly increasing (edge %d = %d)", i, edges[i]);
        E.e[i] = edges[i];
    }
    mc::DepthSource src;
    if (int rc = src.open(ctx, r->device, "runs")) return rc;
    const int32_t* d_depth = src.d;
    r->computed = false;

    // ---- tile table (host), every segment checked against the contig table
    std::vector<Tile> tiles;
    std::vector<int64_t> seg_tile((size_t)S + 1);
    for (int64_t s = 0; s < S; ++s) {
        if (int rc = src.segment(s, tid, start, end)) return rc;
        seg_tile[s] = (int64_t)tiles.size();
        const int rc = mc::cut_tiles(
            tiles, kTile, start[s], end[s], 1, [&](int64_t a) { return src.lead(src.off + a); },
            [&](int64_t a, int64_t n) {
                Tile t;
                t.first = src.off + a;
                t.rel = a;
                t.n = (int32_t)n;
                t.valid = (int32_t)std::max<int64_t>(0, std::min<int64_t>(n, src.ext - a));
                t.seg = (int32_t)std::min<int64_t>(s, INT32_MAX);
                t.flags = (a == start[s] ? 1 : 0) | (a >= 1 && a - 1 < src.ext ? 2 : 0);
                return t;
            });
        if (rc) return rc;
    }
    const int64_t T = (int64_t)tiles.size();
    mc::close_seg_tile(seg_tile, T, start, end);

    if (int rc = src.ready()) return rc;
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(r->tiles.reserve((size_t)T));
    HIP_TRY(r->counts.reserve((size_t)T));
    HIP_TRY(r->base.reserve((size_t)T + 1));
    HIP_TRY(r->seg_tile.reserve((size_t)S + 1));
    HIP_TRY(r->seg_first.reserve((size_t)S + 1));
    hipStream_t st = r->stream;
    if (T) HIP_TRY(hipMemcpyAsync(r->tiles.p, tiles.data(), (size_t)T * sizeof(Tile), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(r->seg_tile.p, seg_tile.data(), ((size_t)S + 1) * 8, hipMemcpyHostToDevice, st));
    if (int rc = r->mark(kEvCount)) return rc;
    if (T) {
        if (n_edges)
            hipLaunchKernelGGL(runs_count_kernel<true>, dim3((unsigned)T), dim3(kThreads), 0, st, d_depth,
                               r->tiles.p, E, r->counts.p);
        else
            hipLaunchKernelGGL(runs_count_kernel<false>, dim3((unsigned)T), dim3(kThreads), 0, st, d_depth,
                               r->tiles.p, E, r->counts.p);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = r->mark(kEvScan)) return rc;
    hipLaunchKernelGGL(runs_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, r->counts.p, T, r->base.p,
                       r->seg_tile.p, S, r->seg_first.p);
    HIP_TRY(hipGetLastError());
    if (int rc = r->mark(kEvScanEnd)) return rc;
    int64_t total = 0;
    if (int rc = r->read_total(r->base.p + T, 0, &total)) return rc;
    MC_REQUIRE(total >= 0 && total <= T * (int64_t)kTile, MC_E_STATE, "run count %lld out of range",
               (long long)total);
    HIP_TRY(r->run_start.reserve((size_t)total));
    HIP_TRY(r->run_value.reserve((size_t)total));
    if (int rc = r->mark(kEvEmit)) return rc;
    if (T) {
        if (n_edges)
            hipLaunchKernelGGL(runs_emit_kernel<true>, dim3((unsigned)T), dim3(kThreads), 0, st, d_depth,
                               r->tiles.p, E, r->base.p, r->run_start.p, r->run_value.p);
        else
            hipLaunchKernelGGL(runs_emit_kernel<false>, dim3((unsigned)T), dim3(kThreads), 0, st, d_depth,
                               r->tiles.p, E, r->base.p, r->run_start.p, r->run_value.p);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = r->mark(kEvEmitEnd)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    if (int rc = r->elapsed(kEvCount, kEvScan, &r->ms[0])) return rc;
    if (int rc = r->elapsed(kEvScan, kEvScanEnd, &r->ms[1])) return rc;
    if (int rc = r->elapsed(kEvEmit, kEvEmitEnd, &r->ms[2])) return rc;
    r->S = S;
    r->n_runs = total;
    r->n_tiles = T;
    r->computed = true;
    *n_runs = total;
    return MC_OK;
}

extern "C" int mc_runs_seg_first(const mc_runs* r, int64_t* seg_first) {
    MC_REQUIRE(r && seg_first, MC_E_INVALID, "null argument");
    MC_REQUIRE(r->computed, MC_E_STATE, "no runs computed (call mc_runs_compute)");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipMemcpyAsync(seg_first, r->seg_first.p, ((size_t)r->S + 1) * 8, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return MC_OK;
}

extern "C" int mc_runs_get(const mc_runs* r, int64_t first, int64_t count, int64_t* run_start,
                           int32_t* run_value) {
    MC_REQUIRE(r, MC_E_INVALID, "null argument");
    MC_REQUIRE(r->computed, MC_E_STATE, "no runs computed (call mc_runs_compute)");
    MC_REQUIRE(first >= 0 && count >= 0 && first <= r->n_runs && count <= r->n_runs - first, MC_E_INVALID,
               "runs [%lld, %lld + %lld) outside [0, %lld]", (long long)first, (long long)first,
               (long long)count, (long long)r->n_runs);
    MC_REQUIRE(count == 0 || (run_start && run_value), MC_E_INVALID, "null out");
    if (count == 0) return MC_OK;
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipMemcpyAsync(run_start, r->run_start.p + first, (size_t)count * 8, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipMemcpyAsync(run_value, r->run_value.p + first, (size_t)count * 4, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return MC_OK;
}

extern "C" int mc_runs_device(const mc_runs* r, const int64_t** d_start, const int32_t** d_value,
                              const int64_t** d_seg_first, int64_t* n_runs) {
    MC_REQUIRE(r && d_start && d_value && d_seg_first && n_runs, MC_E_INVALID, "null argument");
    MC_REQUIRE(r->computed, MC_E_STATE, "no runs computed (call mc_runs_compute)");
    *d_start = r->run_start.p;
    *d_value = r->run_value.p;
    *d_seg_first = r->seg_first.p;
    *n_runs = r->n_runs;
    return MC_OK;
}

extern "C" int mc_runs_timing(const mc_runs* r, float* count_ms, float* scan_ms, float* emit_ms, int64_t* tiles) {
    MC_REQUIRE(r && count_ms && scan_ms && emit_ms && tiles, MC_E_INVALID, "null argument");
    MC_REQUIRE(r->computed, MC_E_STATE, "no runs computed (call mc_runs_compute)");
    *count_ms = r->ms[0];
    *scan_ms = r->ms[1];
    *emit_ms = r->ms[2];
    *tiles = r->n_tiles;
    return MC_OK;
}
