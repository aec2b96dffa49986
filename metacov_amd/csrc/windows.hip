// Windowed coverage: per-window depth sums and threshold counts, and the depth
// histogram per segment, from the depth vector K2 left in HBM (mosdepth --by /
// --thresholds / *.dist.txt, deepTools bins, CoverM's covered fraction; nothing
// in the reference, which reports region statistics only).
//
// Segments (tid, start, end) follow mc_runs_compute's rules.  Segment s is cut
// into windows of `window` positions (the last one short; window == 0: the
// whole segment), windows [seg_first[s], seg_first[s + 1]).  Per window: the
// int64 sum of depths and, per threshold, the positions with depth >= it.
//
// The host cuts every segment into tiles of at most kTile - lead positions and
// uploads the tile table.  A window of at most kSmall = kTile - 3 positions
// lies in exactly one tile (a tile holds whole windows only, bar a segment's
// short last window); a longer window is cut into pieces of one tile each.
//   A  windows_tile_kernel     one workgroup per tile.
//        one window (or piece) in the tile: per-lane sums over its 32 values,
//          wave reduction (DPP), the four waves through LDS, one row written:
//          the window's own row, or the piece's partial row
//        several windows: accumulators in LDS (int64 sum + int32 counts per
//          window).  A lane's 4 consecutive values lie in at most 2 windows
//          (window >= 16), and with window >= 256 so do the 256 consecutive
//          positions of a wave round: then the lanes keep partials of the
//          wave's current window and the next over the rounds, and the wave
//          reduces and adds them once per window it touches; else every lane
//          adds its own non-zero partials (integer LDS adds, order-independent).
//          The tile's windows are then stored as contiguous rows.
//   B  windows_combine_kernel  one wave per window of several pieces: its
//        partial rows are contiguous in piece order; lanes stride over them,
//        wave reduction, lane 0 writes.  No atomics in A or B.
//   H  windows_hist_kernel     kHistGroups persistent workgroups, each over a
//        contiguous range of the histogram's tile table, an n_bins histogram
//        in LDS (LDS atomic adds, depth clamped to the last bin) kept while
//        consecutive tiles belong to one segment; on a segment change and at
//        the end of the range the non-zero bins go to the segment's global row
//        with 64-bit integer atomicAdd (rows zeroed on the stream before).
// No workgroup waits on another.  Loads are runs.hip's: wave w owns positions
// [2048 w, 2048 w + 2048) of the tile's 16-byte aligned window in 8 rounds of
// 64 lanes x 4 positions (global_load_dwordx4, 1 KiB contiguous per wave load);
// the elements at an unaligned `lead` and around the extent are loaded one by
// one, guarded, so no load leaves [first, first + valid) of the tile.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/metacov_amd.h"
#include "common.h"
#include "tile_util.h"

namespace {

using mc::Buf;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRounds = 8;                          // int4 loads per lane
constexpr int kTile = kThreads * 4 * kRounds;       // 8192 positions
constexpr int kWavePos = kTile / kWaves;            // 2048
constexpr int kRoundPos = 64 * 4;                   // positions of one wave round
constexpr int kSmall = kTile - 3;                   // windows up to this lie in one tile whatever its lead
constexpr int kMaxThr = 16;
constexpr int kMaxBins = 8192;                      // 32 KiB of LDS bins
constexpr int kHistGroups = 1024;
constexpr int kHistFlushTiles = 1 << 17;            // an LDS bin stays below 2^31
constexpr int64_t kMaxHistCells = int64_t(1) << 27;

struct Tile {
    int64_t first;     // depth-vector index of the tile's first position
    int64_t out;       // first window row, or the partial row (flags & 1); histogram: the segment
    int32_t n;         // positions (lead + n <= kTile)
    int32_t valid;     // of them inside the contig's extent (a prefix)
    int32_t win;       // window length in the tile (>= n: one window or piece)
    int32_t flags;     // 1: the row is a partial row of a window of several pieces
};
static_assert(sizeof(Tile) == 32, "tile table entry");

struct Multi {         // a window of several pieces
    int64_t window, first_piece, n_pieces;
};

struct Thr {
    int32_t n;
    int32_t t[kMaxThr];
};

__device__ __forceinline__ int lead_of(const int32_t* d, const Tile& t) {
    return (int)((reinterpret_cast<uintptr_t>(d + t.first) >> 2) & 3);
}

// The calling lane's 32 values of tile t; 0 outside [0, valid).  lead: elements
// of the aligned window in front of the tile's first position.
__device__ __forceinline__ void tile_load(const int32_t* __restrict__ d, const Tile& t, int lead, int wave,
                                          int lane, int32_t (&v)[kRounds][4]) {
    const int32_t* w = d + (t.first - lead);            // the window: 16-byte aligned
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int e0 = wave * kWavePos + (r * 64 + lane) * 4;   // window element of v[r][0]
        const int p0 = e0 - lead;                               // tile position of it
        if (p0 >= 0 && p0 + 4 <= t.valid) {
            const int4 x = *reinterpret_cast<const int4*>(w + e0);
            v[r][0] = x.x; v[r][1] = x.y; v[r][2] = x.z; v[r][3] = x.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[r][k] = (p0 + k >= 0 && p0 + k < t.valid) ? w[e0 + k] : 0;
        }
    }
}

// Row and wave totals, the same value in every lane of the row / wave.  All 64
// lanes must be active.  Inside a row of 16 lanes a DPP butterfly (lane ^ 1, lane ^ 2 as quad
// permutations, then the half-row and the row mirrored: after each step the
// lanes that hold equal partial sums double); the four rows' totals are read
// with v_readlane and added as scalars.  No LDS traffic, unlike __shfl_xor.
template <int CTRL>
__device__ __forceinline__ int32_t dpp(int32_t x) {
    return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, false);
}
constexpr int kDppXor1 = 0xB1;          // quad_perm:[1,0,3,2]
constexpr int kDppXor2 = 0x4E;          // quad_perm:[2,3,0,1]
constexpr int kDppHalfMirror = 0x141;   // row_half_mirror: lane i <-> 7 - i of each 8
constexpr int kDppMirror = 0x140;       // row_mirror: lane i <-> 15 - i of each 16

__device__ __forceinline__ int32_t row_sum(int32_t x) {     // the total of the lane's row of 16
    x += dpp<kDppXor1>(x);
    x += dpp<kDppXor2>(x);
    x += dpp<kDppHalfMirror>(x);
    x += dpp<kDppMirror>(x);
    return x;
}

__device__ __forceinline__ int32_t wave_sum(int32_t x) {
    x = row_sum(x);
    return __builtin_amdgcn_readlane(x, 0) + __builtin_amdgcn_readlane(x, 16) +
           __builtin_amdgcn_readlane(x, 32) + __builtin_amdgcn_readlane(x, 48);
}

template <int CTRL>
__device__ __forceinline__ int64_t dpp64(int64_t x) {
    const uint32_t lo = (uint32_t)dpp<CTRL>((int32_t)(uint32_t)x);
    const uint32_t hi = (uint32_t)dpp<CTRL>((int32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ int64_t row_sum(int64_t x) {
    x += dpp64<kDppXor1>(x);
    x += dpp64<kDppXor2>(x);
    x += dpp64<kDppHalfMirror>(x);
    x += dpp64<kDppMirror>(x);
    return x;
}

__device__ __forceinline__ int64_t wave_sum(int64_t x) {
    x = row_sum(x);
    int64_t total = 0;
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)x, 16 * row);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)((uint64_t)x >> 32), 16 * row);
        total += (int64_t)(((uint64_t)hi << 32) | lo);
    }
    return total;
}

// NT: the compiled threshold slots (0, 4 or 16 >= thr.n), so the per-threshold
// arrays stay in registers.  Dynamic LDS: (max windows per tile) x (8 + 4 n_thr)
// bytes, the int64 sums first.
template <int NT>
__global__ __launch_bounds__(kThreads) void windows_tile_kernel(
    const int32_t* __restrict__ d, const Tile* __restrict__ tiles, Thr thr, uint32_t inv_win /* ceil(2^32 / window) */,
    int64_t* __restrict__ sum, int64_t* __restrict__ ge, int64_t* __restrict__ psum, int64_t* __restrict__ pge) {
    extern __shared__ int64_t lds[];
    __shared__ int64_t wpart[kWaves][1 + kMaxThr];
    const Tile t = tiles[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lead = lead_of(d, t);
    const int nt = thr.n;
    int32_t v[kRounds][4];
    tile_load(d, t, lead, wave, lane, v);

    if (t.n <= t.win) {
        // ---- one window (or one piece of a window): per-lane sums, one row
        int64_t s = 0;
        int32_t c[NT > 0 ? NT : 1] = {};
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int p0 = wave * kWavePos + (r * 64 + lane) * 4 - lead;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = p0 + k >= 0 && p0 + k < t.n;
                s += in ? v[r][k] : 0;
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    if (j < nt) c[j] += in && v[r][k] >= thr.t[j];
            }
        }
        s = wave_sum(s);
#pragma unroll
        for (int j = 0; j < NT; ++j)
            if (j < nt) c[j] = wave_sum(c[j]);
        if (lane == 0) {
            wpart[wave][0] = s;
#pragma unroll
            for (int j = 0; j < NT; ++j)
                if (j < nt) wpart[wave][1 + j] = c[j];
        }
        __syncthreads();
        if ((int)threadIdx.x <= nt) {
            int64_t a = 0;
            for (int w = 0; w < kWaves; ++w) a += wpart[w][threadIdx.x];
            int64_t* o_sum = (t.flags & 1) ? psum : sum;
            int64_t* o_ge = (t.flags & 1) ? pge : ge;
            if (threadIdx.x == 0)
                o_sum[t.out] = a;
            else
                o_ge[t.out * nt + (threadIdx.x - 1)] = a;
        }
        return;
    }

    // ---- several whole windows: accumulators in LDS
    const int win = t.win;
    const int nw = (t.n + win - 1) / win;
    int64_t* wsum = lds;
    int32_t* wcnt = reinterpret_cast<int32_t*>(lds + nw);
    for (int i = threadIdx.x; i < nw; i += kThreads) wsum[i] = 0;
    for (int i = threadIdx.x; i < nw * nt; i += kThreads) wcnt[i] = 0;
    __syncthreads();
    if (win >= kRoundPos) {
        // A round (256 consecutive positions) lies in at most 2 windows: the
        // lanes keep partials of window cur (A; the counts' low halves) and
        // cur + 1 (B; high halves) over the rounds, and the wave adds A's
        // totals to LDS whenever a round starts past cur's end.  A lane adds at
        // most 32 per half, a row of lanes 512.  All of this is wave-uniform.
        int cur = (int)__umulhi((uint32_t)max(0, wave * kWavePos - lead), inv_win);
        int nb = (cur + 1) * win;                       // cur's end
        int64_t s_a = 0, s_b = 0;
        int32_t c[NT > 0 ? NT : 1] = {};
        bool any_b = false;
        auto flush = [&]() {                            // A's totals to window cur, row by row of 16 lanes
            const int64_t s = row_sum(s_a);
            int32_t cw[NT > 0 ? NT : 1] = {};
#pragma unroll
            for (int j = 0; j < NT; ++j)
                if (j < nt) cw[j] = row_sum(c[j]) & 0xffff;
            if ((lane & 15) == 0 && cur < nw) {
                if (s) atomicAdd(reinterpret_cast<unsigned long long*>(wsum + cur), (unsigned long long)s);
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    if (j < nt && cw[j]) atomicAdd(wcnt + cur * nt + j, cw[j]);
            }
        };
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int p0 = wave * kWavePos + (r * 64 + lane) * 4 - lead;
            const int pf = max(0, wave * kWavePos + r * kRoundPos - lead);             // the round's tile positions
            const int pl = min(t.n - 1, wave * kWavePos + r * kRoundPos + kRoundPos - 1 - lead);
            if (pl < pf) break;                         // past the tile's end, as are the rounds after it
            if (pf >= nb) {                             // the round starts in window cur + 1: B becomes A
                flush();
                s_a = s_b, s_b = 0;
#pragma unroll
                for (int j = 0; j < NT; ++j) c[j] = (int32_t)((uint32_t)c[j] >> 16);
                ++cur, nb += win;
            }
            any_b = pl >= nb;
            if (NT <= 4 && !any_b) {                    // the whole round lies in window cur (a second copy of
                                                        // the loop: with 16 slots it costs too many registers)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool in = p0 + k >= 0 && p0 + k < t.n;
                    s_a += in ? v[r][k] : 0;
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        if (j < nt) c[j] += in && v[r][k] >= thr.t[j];
                }
                continue;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = p0 + k;
                const bool in = p >= 0 && p < t.n;
                const bool hi = p >= nb;
                const int32_t x = in ? v[r][k] : 0;
                s_a += hi ? 0 : x;
                s_b += hi ? x : 0;
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    if (j < nt) c[j] += (int32_t)(in && v[r][k] >= thr.t[j]) << (hi ? 16 : 0);
            }
        }
        flush();
        if (any_b) {
            s_a = s_b;
#pragma unroll
            for (int j = 0; j < NT; ++j) c[j] = (int32_t)((uint32_t)c[j] >> 16);
            ++cur;
            flush();
        }
    } else {
        // A lane's 4 consecutive values lie in at most 2 windows (window >= 16):
        // every lane adds its own non-zero partials.
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int p0 = wave * kWavePos + (r * 64 + lane) * 4 - lead;
            if (p0 + 3 < 0 || p0 >= t.n) continue;
            const int lo = (int)__umulhi((uint32_t)max(p0, 0), inv_win);
            const int b = (lo + 1) * win;               // positions < b: window lo; the others: lo + 1
            int64_t s_lo = 0, s_hi = 0;
            int32_t c[NT > 0 ? NT : 1] = {};            // low half: window lo, high half: lo + 1
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = p0 + k;
                const bool in = p >= 0 && p < t.n;
                const bool hi = p >= b;
                const int32_t x = in ? v[r][k] : 0;
                s_lo += hi ? 0 : x;
                s_hi += hi ? x : 0;
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    if (j < nt) c[j] += (int32_t)(in && v[r][k] >= thr.t[j]) << (hi ? 16 : 0);
            }
            if (s_lo && lo < nw) atomicAdd(reinterpret_cast<unsigned long long*>(wsum + lo), (unsigned long long)s_lo);
            if (s_hi && lo + 1 < nw)
                atomicAdd(reinterpret_cast<unsigned long long*>(wsum + lo + 1), (unsigned long long)s_hi);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                if (j < nt) {
                    const int32_t c_lo = c[j] & 0xffff, c_hi = c[j] >> 16;
                    if (c_lo && lo < nw) atomicAdd(wcnt + lo * nt + j, c_lo);
                    if (c_hi && lo + 1 < nw) atomicAdd(wcnt + (lo + 1) * nt + j, c_hi);
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nw; i += kThreads) sum[t.out + i] = wsum[i];
    for (int i = threadIdx.x; i < nw * nt; i += kThreads) ge[t.out * nt + i] = wcnt[i];
}

// One wave per window of several pieces.
template <int NT>
__global__ __launch_bounds__(kThreads) void windows_combine_kernel(
    const Multi* __restrict__ multi, int64_t n_multi, int32_t nt, const int64_t* __restrict__ psum,
    const int64_t* __restrict__ pge, int64_t* __restrict__ sum, int64_t* __restrict__ ge) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (m >= n_multi) return;                           // wave-uniform
    const Multi w = multi[m];
    int64_t s = 0;
    int64_t c[NT > 0 ? NT : 1] = {};
    for (int64_t i = lane; i < w.n_pieces; i += 64) {
        const int64_t p = w.first_piece + i;
        s += psum[p];
#pragma unroll
        for (int j = 0; j < NT; ++j)
            if (j < nt) c[j] += pge[p * nt + j];
    }
    s = wave_sum(s);
#pragma unroll
    for (int j = 0; j < NT; ++j)
        if (j < nt) c[j] = wave_sum(c[j]);
    if (lane == 0) {
        sum[w.window] = s;
#pragma unroll
        for (int j = 0; j < NT; ++j)
            if (j < nt) ge[w.window * nt + j] = c[j];
    }
}

// kHistGroups workgroups; workgroup g takes tiles [g per, (g + 1) per).
// Dynamic LDS: n_bins x 4 bytes.
__global__ __launch_bounds__(kThreads) void windows_hist_kernel(const int32_t* __restrict__ d,
                                                               const Tile* __restrict__ tiles, int64_t n_tiles,
                                                               int64_t per, int32_t n_bins,
                                                               unsigned long long* __restrict__ hist) {
    extern __shared__ int32_t bins[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t a = (int64_t)blockIdx.x * per, b = min(n_tiles, a + per);
    if (a >= b) return;
    for (int i = threadIdx.x; i < n_bins; i += kThreads) bins[i] = 0;
    __syncthreads();
    const int32_t top = n_bins - 1;
    int64_t seg = -1;
    int since = 0;                                      // tiles since the last flush
    for (int64_t i = a; i < b; ++i) {
        const Tile t = tiles[i];
        if (seg >= 0 && (t.out != seg || since >= kHistFlushTiles)) {
            __syncthreads();
            for (int k = threadIdx.x; k < n_bins; k += kThreads) {
                const int32_t c = bins[k];
                if (c) {
                    atomicAdd(hist + seg * n_bins + k, (unsigned long long)c);
                    bins[k] = 0;
                }
            }
            __syncthreads();
            since = 0;
        }
        seg = t.out;
        ++since;
        if (t.valid == 0) {                             // entirely past the extent: depth 0
            if (threadIdx.x == 0) atomicAdd(bins, t.n);
            continue;
        }
        const int lead = lead_of(d, t);
        int32_t v[kRounds][4];
        tile_load(d, t, lead, wave, lane, v);
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int p0 = wave * kWavePos + (r * 64 + lane) * 4 - lead;
            int32_t q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = min(v[r][k], top);
            const bool full = p0 >= 0 && p0 + 4 <= t.n;
            const bool same = full && q[0] == q[1] && q[1] == q[2] && q[2] == q[3] &&
                              q[0] == __builtin_amdgcn_readfirstlane(q[0]);
            if (__all(same)) {                          // one value over the round: one add
                if (lane == 0) atomicAdd(bins + q[0], kRoundPos);
                continue;
            }
            // equal neighbours of the lane's 4 values go together
            int32_t run = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = p0 + k >= 0 && p0 + k < t.n;
                run += in;
                const bool last = k == 3 || q[k + (k < 3)] != q[k];
                if (last && run) {
                    atomicAdd(bins + q[k], run);
                    run = 0;
                }
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n_bins; k += kThreads) {
        const int32_t c = bins[k];
        if (c) atomicAdd(hist + seg * n_bins + k, (unsigned long long)c);
    }
}

}  // namespace

namespace {
enum { kEvTile, kEvCombine, kEvCombineEnd, kEvHist, kEvHistEnd, kEvents };   // the tile pass ends where the combine begins
}

struct mc_windows : mc::StageHandle<kEvents, 0> {
    Buf<Tile> tiles, htiles;
    Buf<Multi> multi;
    Buf<int64_t> seg_first, sum, ge, psum, pge;
    Buf<unsigned long long> hist;
    bool computed = false, hist_done = false;
    int64_t S = 0, n_windows = 0, n_tiles = 0;
    int32_t n_thr = 0;
    float ms[3] = {0, 0, 0};
};

extern "C" int mc_windows_create(int device, mc_windows** out) {
    MC_REQUIRE(out, MC_E_INVALID, "null argument");
    return mc::stage_create(device, out);
}

extern "C" int mc_windows_destroy(mc_windows* w) { return mc::stage_destroy(w); }

extern "C" int mc_windows_dims(int32_t* tile, int32_t* min_window, int32_t* max_bins, int32_t* hist_groups) {
    MC_REQUIRE(tile && min_window && max_bins && hist_groups, MC_E_INVALID, "null argument");
    *tile = kTile;
    *min_window = MC_WINDOWS_MIN;
    *max_bins = kMaxBins;
    *hist_groups = kHistGroups;
    return MC_OK;
}

extern "C" int mc_windows_compute(mc_windows* w, mc_ctx* ctx, int64_t S, const int32_t* tid, const int64_t* start,
                                  const int64_t* end, int64_t window, int32_t n_thr, const int32_t* thr,
                                  int64_t* n_windows) {
    MC_REQUIRE(w && ctx && n_windows, MC_E_INVALID, "null argument");
    MC_REQUIRE(S >= 0 && (S == 0 || (tid && start && end)), MC_E_INVALID, "bad segment arrays");
    MC_REQUIRE(window == 0 || window >= MC_WINDOWS_MIN, MC_E_INVALID,
               "window %lld: must be 0 (the whole segment) or at least %d", (long long)window, MC_WINDOWS_MIN);
    MC_REQUIRE(n_thr >= 0 && n_thr <= kMaxThr && (n_thr == 0 || thr), MC_E_INVALID,
               "%d thresholds outside 0..%d", n_thr, kMaxThr);
    Thr H{};
    H.n = n_thr;
    for (int i = 0; i < n_thr; ++i) {
        MC_REQUIRE(thr[i] >= 0 && (i == 0 || thr[i] > thr[i - 1]), MC_E_INVALID,
                   "thresholds must be non-negative and strictly increasing (threshold %d = %d)", i, thr[i]);
        H.t[i] = thr[i];
    }
    mc::DepthSource src;
    if (int rc = src.open(ctx, w->device, "windows")) return rc;
    const int32_t* d_depth = src.d;
    w->computed = false;

    // ---- seg_first (arithmetic), every segment checked against the contig table
    std::vector<int64_t> seg_first((size_t)S + 1);
    std::vector<int64_t> c_off((size_t)S), c_ext((size_t)S);
    seg_first[0] = 0;
    for (int64_t s = 0; s < S; ++s) {
        if (int rc = src.segment(s, tid, start, end)) return rc;
        c_off[s] = src.off, c_ext[s] = src.ext;
        const int64_t len = end[s] - start[s];
        const int64_t k = len == 0 ? 0 : window == 0 ? 1 : 1 + (len - 1) / window;
        seg_first[s + 1] = seg_first[s] + k;
        MC_REQUIRE(seg_first[s + 1] <= (int64_t(1) << 31), MC_E_RANGE, "more than 2^31 windows in one call");
    }
    const int64_t W = seg_first[S];

    // ---- tile table: whole windows per tile, or one piece of a long window
    std::vector<Tile> tiles;
    std::vector<Multi> multi;
    int64_t n_pieces = 0;                         // partial rows
    int max_nw = 1;                               // windows of the fullest tile
    for (int64_t s = 0; s < S; ++s) {
        const int64_t len = end[s] - start[s];
        if (len == 0) continue;
        const int64_t win = window == 0 || window > len ? len : window;
        int64_t row = seg_first[s];
        auto push = [&](int64_t a, int64_t n, int64_t out, int32_t twin, int32_t flags) {
            Tile t;
            t.first = c_off[s] + a;
            t.out = out;
            t.n = (int32_t)n;
            t.valid = (int32_t)std::max<int64_t>(0, std::min<int64_t>(n, c_ext[s] - a));
            t.win = twin;
            t.flags = flags;
            return t;
        };
        const auto lead = [&](int64_t a) { return src.lead(c_off[s] + a); };
        if (win <= kSmall) {                      // a tile holds whole windows (at least one: kSmall <= kTile - 3)
            const int rc = mc::cut_tiles(tiles, kTile, start[s], end[s], win, lead, [&](int64_t a, int64_t n) {
                const int64_t nw = (n + win - 1) / win, row0 = row;
                max_nw = (int)std::max<int64_t>(max_nw, nw);
                row += nw;
                return push(a, n, row0, (int32_t)win, 0);
            });
            if (rc) return rc;
        } else {
            for (int64_t wa = start[s]; wa < end[s]; wa += win, ++row) {
                const int64_t we = std::min(wa + win, end[s]);
                const int64_t piece0 = n_pieces;
                const size_t tile0 = tiles.size();
                const int rc = mc::cut_tiles(tiles, kTile, wa, we, 1, lead,
                                             [&](int64_t a, int64_t n) { return push(a, n, n_pieces++, kTile, 1); });
                if (rc) return rc;
                if (n_pieces - piece0 == 1) {     // a short last window: its row directly
                    tiles[tile0].out = row;
                    tiles[tile0].flags = 0;
                    n_pieces = piece0;
                } else {
                    multi.push_back(Multi{row, piece0, n_pieces - piece0});
                }
            }
        }
    }
    const int64_t T = (int64_t)tiles.size();
    const int64_t M = (int64_t)multi.size();

    if (int rc = src.ready()) return rc;
    HIP_TRY(hipSetDevice(w->device));
    HIP_TRY(w->tiles.reserve((size_t)T));
    HIP_TRY(w->multi.reserve((size_t)M));
    HIP_TRY(w->seg_first.reserve((size_t)S + 1));
    HIP_TRY(w->sum.reserve((size_t)W));
    HIP_TRY(w->ge.reserve((size_t)W * n_thr));
    HIP_TRY(w->psum.reserve((size_t)n_pieces));
    HIP_TRY(w->pge.reserve((size_t)n_pieces * n_thr));
    hipStream_t st = w->stream;
    if (T) HIP_TRY(hipMemcpyAsync(w->tiles.p, tiles.data(), (size_t)T * sizeof(Tile), hipMemcpyHostToDevice, st));
    if (M) HIP_TRY(hipMemcpyAsync(w->multi.p, multi.data(), (size_t)M * sizeof(Multi), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(w->seg_first.p, seg_first.data(), ((size_t)S + 1) * 8, hipMemcpyHostToDevice, st));
    const int NT = n_thr == 0 ? 0 : n_thr <= 4 ? 4 : 16;
    const uint32_t inv_win =                      // only tiles of several windows divide: 16 <= window <= kSmall
        window >= MC_WINDOWS_MIN && window <= kSmall ? (uint32_t)(((uint64_t(1) << 32) + window - 1) / window) : 0;
    const size_t lds = (size_t)max_nw * (8 + 4 * (size_t)n_thr);
    if (int rc = w->mark(kEvTile)) return rc;
    if (T) {
        const dim3 g((unsigned)T), b(kThreads);
        if (NT == 0)
            hipLaunchKernelGGL(windows_tile_kernel<0>, g, b, lds, st, d_depth, w->tiles.p, H, inv_win, w->sum.p,
                               w->ge.p, w->psum.p, w->pge.p);
        else if (NT == 4)
            hipLaunchKernelGGL(windows_tile_kernel<4>, g, b, lds, st, d_depth, w->tiles.p, H, inv_win, w->sum.p,
                               w->ge.p, w->psum.p, w->pge.p);
        else
            hipLaunchKernelGGL(windows_tile_kernel<16>, g, b, lds, st, d_depth, w->tiles.p, H, inv_win, w->sum.p,
                               w->ge.p, w->psum.p, w->pge.p);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = w->mark(kEvCombine)) return rc;
    if (M) {
        const dim3 g((unsigned)((M + kWaves - 1) / kWaves)), b(kThreads);
        if (NT == 0)
            hipLaunchKernelGGL(windows_combine_kernel<0>, g, b, 0, st, w->multi.p, M, n_thr, w->psum.p, w->pge.p,
                               w->sum.p, w->ge.p);
        else if (NT == 4)
            hipLaunchKernelGGL(windows_combine_kernel<4>, g, b, 0, st, w->multi.p, M, n_thr, w->psum.p, w->pge.p,
                               w->sum.p, w->ge.p);
        else
            hipLaunchKernelGGL(windows_combine_kernel<16>, g, b, 0, st, w->multi.p, M, n_thr, w->psum.p, w->pge.p,
                               w->sum.p, w->ge.p);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = w->mark(kEvCombineEnd)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    if (int rc = w->elapsed(kEvTile, kEvCombine, &w->ms[0])) return rc;
    if (int rc = w->elapsed(kEvCombine, kEvCombineEnd, &w->ms[1])) return rc;
    w->S = S;
    w->n_windows = W;
    w->n_tiles = T;
    w->n_thr = n_thr;
    w->computed = true;
    *n_windows = W;
    return MC_OK;
}

extern "C" int mc_windows_seg_first(const mc_windows* w, int64_t* seg_first) {
    MC_REQUIRE(w && seg_first, MC_E_INVALID, "null argument");
    MC_REQUIRE(w->computed, MC_E_STATE, "no windows computed (call mc_windows_compute)");
    HIP_TRY(hipSetDevice(w->device));
    HIP_TRY(hipMemcpyAsync(seg_first, w->seg_first.p, ((size_t)w->S + 1) * 8, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return MC_OK;
}

extern "C" int mc_windows_get(const mc_windows* w, int64_t first, int64_t count, int64_t* sum, int64_t* ge) {
    MC_REQUIRE(w, MC_E_INVALID, "null argument");
    MC_REQUIRE(w->computed, MC_E_STATE, "no windows computed (call mc_windows_compute)");
    MC_REQUIRE(first >= 0 && count >= 0 && first <= w->n_windows && count <= w->n_windows - first, MC_E_INVALID,
               "windows [%lld, %lld + %lld) outside [0, %lld]", (long long)first, (long long)first,
               (long long)count, (long long)w->n_windows);
    MC_REQUIRE(count == 0 || (sum && (ge || w->n_thr == 0)), MC_E_INVALID, "null out");
    if (count == 0) return MC_OK;
    HIP_TRY(hipSetDevice(w->device));
    HIP_TRY(hipMemcpyAsync(sum, w->sum.p + first, (size_t)count * 8, hipMemcpyDeviceToHost, w->stream));
    if (w->n_thr)
        HIP_TRY(hipMemcpyAsync(ge, w->ge.p + first * w->n_thr, (size_t)count * w->n_thr * 8, hipMemcpyDeviceToHost,
                               w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return MC_OK;
}

extern "C" int mc_windows_device(const mc_windows* w, const int64_t** d_sum, const int64_t** d_ge,
                                 const int64_t** d_seg_first, int64_t* n_windows, int32_t* n_thr) {
    MC_REQUIRE(w && d_sum && d_ge && d_seg_first && n_windows && n_thr, MC_E_INVALID, "null argument");
    MC_REQUIRE(w->computed, MC_E_STATE, "no windows computed (call mc_windows_compute)");
    *d_sum = w->sum.p;
    *d_ge = w->ge.p;
    *d_seg_first = w->seg_first.p;
    *n_windows = w->n_windows;
    *n_thr = w->n_thr;
    return MC_OK;
}

extern "C" int mc_windows_hist(mc_windows* w, mc_ctx* ctx, int64_t S, const int32_t* tid, const int64_t* start,
                               const int64_t* end, int32_t n_bins, int64_t* hist) {
    MC_REQUIRE(w && ctx, MC_E_INVALID, "null argument");
    MC_REQUIRE(S >= 0 && (S == 0 || (tid && start && end && hist)), MC_E_INVALID, "bad segment arrays");
    MC_REQUIRE(n_bins >= 1 && n_bins <= kMaxBins, MC_E_INVALID, "%d bins outside 1..%d", n_bins, kMaxBins);
    mc::DepthSource src;
    if (int rc = src.open(ctx, w->device, "windows")) return rc;
    const int32_t* d_depth = src.d;
    MC_REQUIRE(S * (int64_t)n_bins <= kMaxHistCells, MC_E_RANGE, "%lld segments x %d bins exceed 2^27 cells",
               (long long)S, n_bins);
    std::vector<Tile> tiles;
    for (int64_t s = 0; s < S; ++s) {
        if (int rc = src.segment(s, tid, start, end)) return rc;
        const int rc = mc::cut_tiles(
            tiles, kTile, start[s], end[s], 1, [&](int64_t a) { return src.lead(src.off + a); },
            [&](int64_t a, int64_t n) {
                Tile t;
                t.first = src.off + a;
                t.out = s;
                t.n = (int32_t)n;
                t.valid = (int32_t)std::max<int64_t>(0, std::min<int64_t>(n, src.ext - a));
                t.win = kTile;
                t.flags = 0;
                return t;
            });
        if (rc) return rc;
    }
    const int64_t T = (int64_t)tiles.size();
    const size_t cells = (size_t)S * n_bins;
    if (int rc = src.ready()) return rc;
    HIP_TRY(hipSetDevice(w->device));
    HIP_TRY(w->htiles.reserve((size_t)T));
    HIP_TRY(w->hist.reserve(cells));
    hipStream_t st = w->stream;
    if (T) HIP_TRY(hipMemcpyAsync(w->htiles.p, tiles.data(), (size_t)T * sizeof(Tile), hipMemcpyHostToDevice, st));
    if (cells) HIP_TRY(hipMemsetAsync(w->hist.p, 0, cells * 8, st));
    if (int rc = w->mark(kEvHist)) return rc;
    if (T) {
        const int64_t per = (T + kHistGroups - 1) / kHistGroups;
        hipLaunchKernelGGL(windows_hist_kernel, dim3(kHistGroups), dim3(kThreads), (size_t)n_bins * 4, st, d_depth,
                           w->htiles.p, T, per, n_bins, w->hist.p);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = w->mark(kEvHistEnd)) return rc;
    if (cells) HIP_TRY(hipMemcpyAsync(hist, w->hist.p, cells * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (int rc = w->elapsed(kEvHist, kEvHistEnd, &w->ms[2])) return rc;
    w->hist_done = true;
    return MC_OK;
}

extern "C" int mc_windows_timing(const mc_windows* w, float* window_ms, float* combine_ms, float* hist_ms,
                                 int64_t* tiles) {
    MC_REQUIRE(w && window_ms && combine_ms && hist_ms && tiles, MC_E_INVALID, "null argument");
    MC_REQUIRE(w->computed || w->hist_done, MC_E_STATE,
               "nothing computed (call mc_windows_compute or mc_windows_hist)");
    *window_ms = w->computed ? w->ms[0] : 0;
    *combine_ms = w->computed ? w->ms[1] : 0;
    *hist_ms = w->hist_done ? w->ms[2] : 0;
    *tiles = w->computed ? w->n_tiles : 0;
    return MC_OK;
}
