// Windowed diversity: the kernels of mc_bases_diversity (the contract is the
// header's, "Diversity").  Included by bases.hip inside its anonymous
// namespace, behind Tile and the tile constants.
//
// Launches, both on the handle's stream, neither waiting on another workgroup:
//   div_zero_kernel   one thread per column of the first and the last row a
//                     tile touches: the only rows that tiles share.
//   div_tile_kernel   one workgroup per tile.  A thread reads 4 consecutive
//                     elements of the tile's 16-byte aligned window with one
//                     16-byte load per plane (A, C, G, T) and one 4-byte load of
//                     the reference; elements outside the tile are masked.  A
//                     wave so covers 256 consecutive positions.  The eight
//                     columns are summed per window in LDS rows: a wave whose
//                     positions lie in one or two windows reduces by lane
//                     shuffles and adds once per window, any other wave's lanes
//                     add their own (a lane's 4 positions lie in at most two
//                     windows, a window being at least 16 long).  All integer.
//                     The rows of the windows inside the tile are stored; the
//                     first and the last go to global memory by 64-bit integer
//                     atomicAdd, exact in any order.
// Every loop is bounded by the tile size or by the windows of a tile.

constexpr int kDivCols = MC_DIV_COLS;               // positions covered bases snv pi_fix compared con_diff pop_diff
constexpr int kDivRows = kTile / MC_DIV_MIN_WINDOW + 2;   // windows a tile can touch (129), and one of room
constexpr unsigned long long kDivMaxN = 1ull << 26;  // a covered position's A + C + G + T stays below this

struct DivTile {
    int64_t win;       // global index of the first window the tile touches
    int64_t off;       // the tile's first position, counted from that window's start
};
static_assert(sizeof(DivTile) == 16, "diversity tile entry");

struct DivArgs {
    unsigned long long min_depth, min_count, min_ppm;   // min_depth already raised to 2, min_count to 1
    int64_t window;                                      // the window length; for whole segments, above every length
};

// One window's sums of the lanes that call it: bases and pi_fix in 64 bits, the
// five counts in 10-bit fields (at most 4 per lane, 256 per wave): c0 holds
// covered, snv, compared at bits 0, 10, 20; c1 holds con_diff, pop_diff.
struct DivAcc {
    unsigned long long bases, pi;
    uint32_t c0, c1;
};

__device__ __forceinline__ bool div_qualifies(uint32_t x, unsigned long long n, const DivArgs& d) {
    return x >= d.min_count && (unsigned long long)x * 1000000ull >= d.min_ppm * n;
}

// The window, counted from the tile's first one, of the position p places behind that window's start
// (p < window + kTile).
__device__ __forceinline__ int div_window_of(int64_t p, int64_t window) {
    return window >= kTile ? (int)(p >= window) : (int)((uint32_t)p / (uint32_t)window);
}

__device__ __forceinline__ void div_position(const uint32_t (&a)[4], uint32_t r, const DivArgs& d, int64_t i,
                                             DivAcc& acc, unsigned long long* __restrict__ bad) {
    const unsigned long long n = (unsigned long long)a[0] + a[1] + a[2] + a[3];
    acc.bases += n;
    if (n < d.min_depth) return;
    if (n >= kDivMaxN) {
        atomicMin(bad, (unsigned long long)i);
        return;
    }
    int top = 0;
    uint32_t most = a[0];               // (kept beside top: a[top] would index the array by a variable)
#pragma unroll
    for (int c = 1; c < 4; ++c)
        if (a[c] > most) {
            most = a[c];
            top = c;
        }
    uint32_t minor = 0;
    unsigned long long sq = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c != top && a[c] > minor) minor = a[c];
        sq += (unsigned long long)a[c] * a[c];
    }
    acc.c0 += 1u;
    if (div_qualifies(minor, n, d)) acc.c0 += 1u << 10;
    const unsigned long long num = n * n - sq;
    if (num != 0) acc.pi += (unsigned long long)__double2ll_rn((double)num / (double)(n * (n - 1)) * 4294967296.0);
    if (r < 4) {
        acc.c0 += 1u << 20;
        if ((uint32_t)top != r) {
            uint32_t ar = a[0];
#pragma unroll
            for (int c = 1; c < 4; ++c)
                if (r == (uint32_t)c) ar = a[c];
            acc.c1 += 1u;
            if (!div_qualifies(ar, n, d)) acc.c1 += 1u << 10;
        }
    }
}

// Adds acc to LDS row w (w < nw): the fields that are not zero.
__device__ __forceinline__ void div_add(const DivAcc& acc, int w, int nw, unsigned long long (*s64)[2],
                                        uint32_t (*s32)[5]) {
    if (w >= nw) return;
    if (acc.bases) atomicAdd(&s64[w][0], acc.bases);
    if (acc.pi) atomicAdd(&s64[w][1], acc.pi);
#pragma unroll
    for (int f = 0; f < 5; ++f) {
        const uint32_t v = ((f < 3 ? acc.c0 : acc.c1) >> (10 * (f % 3))) & 0x3FFu;
        if (v) atomicAdd(&s32[w][f], v);
    }
}

__device__ __forceinline__ void div_wave_sum(DivAcc& acc) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        acc.bases += __shfl_xor(acc.bases, off, 64);
        acc.pi += __shfl_xor(acc.pi, off, 64);
        acc.c0 += __shfl_xor(acc.c0, off, 64);
        acc.c1 += __shfl_xor(acc.c1, off, 64);
    }
}

__global__ __launch_bounds__(256) void div_zero_kernel(const Tile* __restrict__ tiles,
                                                       const DivTile* __restrict__ dt, int64_t n_tiles,
                                                       int64_t window, int64_t* __restrict__ rows) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t ti = j >> 4;
    if (ti >= n_tiles) return;
    const DivTile d = dt[ti];
    const int last = div_window_of(d.off + tiles[ti].n - 1, window);
    rows[(d.win + ((j & 8) ? last : 0)) * kDivCols + (j & 7)] = 0;
}

__global__ __launch_bounds__(kThreads) void div_tile_kernel(const uint32_t* __restrict__ planes, int64_t stride,
                                                           const uint8_t* __restrict__ ref,
                                                           const Tile* __restrict__ tiles,
                                                           const DivTile* __restrict__ dt, DivArgs da,
                                                           int64_t* __restrict__ rows,
                                                           unsigned long long* __restrict__ bad) {
    __shared__ unsigned long long s64[kDivRows][2];   // bases, pi_fix
    __shared__ uint32_t s32[kDivRows][5];             // covered, snv, compared, con_diff, pop_diff
    const Tile t = tiles[blockIdx.x];
    const DivTile d = dt[blockIdx.x];
    const int nw = div_window_of(d.off + t.n - 1, da.window) + 1;    // at most kDivRows - 1
    for (int j = threadIdx.x; j < nw * 2; j += kThreads) s64[j >> 1][j & 1] = 0;
    for (int j = threadIdx.x; j < nw * 5; j += kThreads) s32[j / 5][j % 5] = 0;
    __syncthreads();

    // elements [4 * thread, 4 * thread + 4) of the aligned window; position k = element - lead
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int e0 = 4 * (int)threadIdx.x;
    const int k_lo = max(256 * wave - t.lead, 0), k_hi = min(256 * wave + 255 - t.lead, t.n - 1);   // the wave's
    if (k_lo <= k_hi) {
        const int w_lo = div_window_of(d.off + k_lo, da.window), w_hi = div_window_of(d.off + k_hi, da.window);
        const bool together = w_hi - w_lo <= 1;                      // wave-uniform
        DivAcc acc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        int w_base = w_lo;
        if (e0 + 3 >= t.lead && e0 < t.lead + t.n) {
            const int64_t g = t.out - t.lead + e0;                   // 16-byte aligned, inside the plane's stride
            const uint4 pa = *reinterpret_cast<const uint4*>(planes + g);
            const uint4 pc = *reinterpret_cast<const uint4*>(planes + stride + g);
            const uint4 pg = *reinterpret_cast<const uint4*>(planes + 2 * stride + g);
            const uint4 pt = *reinterpret_cast<const uint4*>(planes + 3 * stride + g);
            const uint32_t rw = ref ? *reinterpret_cast<const uint32_t*>(ref + g) : 0x04040404u;
            const uint32_t va[4] = {pa.x, pa.y, pa.z, pa.w}, vc[4] = {pc.x, pc.y, pc.z, pc.w};
            const uint32_t vg[4] = {pg.x, pg.y, pg.z, pg.w}, vt[4] = {pt.x, pt.y, pt.z, pt.w};
            const int k_first = max(e0 - t.lead, 0);                 // the lane's first position
            if (!together) w_base = div_window_of(d.off + k_first, da.window);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = e0 + j - t.lead;
                if (k >= 0 && k < t.n) {
                    const uint32_t a[4] = {va[j], vc[j], vg[j], vt[j]};
                    const int w = div_window_of(d.off + k, da.window);
                    if (w == w_base)
                        div_position(a, (rw >> (8 * j)) & 0xFFu, da, t.out + k, acc[0], bad);
                    else
                        div_position(a, (rw >> (8 * j)) & 0xFFu, da, t.out + k, acc[1], bad);
                }
            }
        }
        if (together) {
            div_wave_sum(acc[0]);
            if (w_hi != w_lo) div_wave_sum(acc[1]);
            if ((threadIdx.x & 63) == 0) {
                div_add(acc[0], w_lo, nw, s64, s32);
                if (w_hi != w_lo) div_add(acc[1], w_hi, nw, s64, s32);
            }
        } else {
            div_add(acc[0], w_base, nw, s64, s32);
            div_add(acc[1], w_base + 1, nw, s64, s32);
        }
    }
    __syncthreads();

    for (int j = threadIdx.x; j < nw * kDivCols; j += kThreads) {
        const int w = j >> 3, c = j & 7;
        int64_t v;
        if (c == 0) {                                                // the window's positions inside the tile
            const int64_t a = (int64_t)w * da.window - d.off, z = a + da.window;
            v = (z < t.n ? z : (int64_t)t.n) - (a > 0 ? a : 0);
        } else if (c == 2 || c == 4) {
            v = (int64_t)s64[w][c == 4];
        } else {
            v = (int64_t)s32[w][c == 1 ? 0 : c == 3 ? 1 : c - 3];
        }
        int64_t* dst = rows + (d.win + w) * kDivCols + c;
        if (w == 0 || w == nw - 1) {                                 // perhaps shared with a neighbour: zeroed before
            if (v) atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)v);
        } else {
            *dst = v;
        }
    }
}
