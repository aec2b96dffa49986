// Sample comparison: the tile kernel of mc_bases_compare (the contract is the
// header's, "Comparison").  Included by bases.hip inside its anonymous
// namespace, behind bases_div.h: the windows, DivTile, div_window_of and the
// zero launch (div_zero_kernel) are diversity's, the rows having as many
// columns.
//
//   cmp_tile_kernel   one workgroup per tile of a's tile table (b's is the
//                     same: the cut depends on the segments only).  A thread
//                     reads 4 consecutive elements of the tile's 16-byte
//                     aligned window with eight 16-byte loads: A, C, G, T of
//                     each handle through its own planes pointer and stride;
//                     elements outside the tile are masked.  The seven sums
//                     are kept per window in LDS rows, by the wave path of
//                     div_tile_kernel: a wave whose positions lie in one or
//                     two windows reduces by lane shuffles and adds once per
//                     window, any other wave's lanes add their own.  All
//                     integer.  The rows of the windows inside the tile are
//                     stored; the first and the last go to global memory by
//                     64-bit integer atomicAdd, exact in any order.
// Every loop is bounded by the tile size or by the windows of a tile.

constexpr int kCmpCols = MC_CMP_COLS;   // positions covered_a covered_b compared con_diff pop_diff snv dist_fix
static_assert(MC_CMP_COLS == MC_DIV_COLS, "div_zero_kernel and the row indexing serve both stages");

// One window's sums of the lanes that call it: dist_fix in 64 bits, the six
// counts in 10-bit fields (at most 4 per lane, 256 per wave) in column order:
// c0 holds covered_a, covered_b, compared at bits 0, 10, 20; c1 holds
// con_diff, pop_diff, snv.
struct CmpAcc {
    unsigned long long dist;
    uint32_t c0, c1;
};

// The first maximum of x in channel order and the largest of the other three
// (both kept beside the index: x[top] would index the array by a variable).
__device__ __forceinline__ void cmp_major(const uint32_t (&x)[4], int& top, uint32_t& minor) {
    top = 0;
    uint32_t most = x[0];
#pragma unroll
    for (int c = 1; c < 4; ++c)
        if (x[c] > most) {
            most = x[c];
            top = c;
        }
    minor = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c != top && x[c] > minor) minor = x[c];
}

__device__ __forceinline__ void cmp_position(const uint32_t (&a)[4], const uint32_t (&b)[4], const DivArgs& d,
                                             int64_t i, CmpAcc& acc, unsigned long long* __restrict__ bad) {
    const unsigned long long na = (unsigned long long)a[0] + a[1] + a[2] + a[3];
    const unsigned long long nb = (unsigned long long)b[0] + b[1] + b[2] + b[3];
    const bool ca = na >= d.min_depth, cb = nb >= d.min_depth;
    acc.c0 += (uint32_t)ca + ((uint32_t)cb << 10);
    if (!(ca && cb)) return;
    if (na >= kDivMaxN || nb >= kDivMaxN) {
        atomicMin(bad, (unsigned long long)i);
        return;
    }
    int top_a, top_b;
    uint32_t minor_a, minor_b;
    cmp_major(a, top_a, minor_a);
    cmp_major(b, top_b, minor_b);
    bool shared = false;                 // an allele present in both samples
    unsigned long long num = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        shared |= (c == top_a || div_qualifies(a[c], na, d)) && (c == top_b || div_qualifies(b[c], nb, d));
        const unsigned long long u = a[c] * nb, v = b[c] * na;       // below 2^52 each
        num += u > v ? u - v : v - u;
    }
    acc.c0 += 1u << 20;
    if (top_a != top_b) acc.c1 += 1u;
    if (!shared) acc.c1 += 1u << 10;
    if (div_qualifies(minor_a, na, d) || div_qualifies(minor_b, nb, d)) acc.c1 += 1u << 20;
    if (num != 0)
        acc.dist += (unsigned long long)__double2ll_rn((double)num / (double)(2 * na * nb) * 4294967296.0);
}

// Adds acc to LDS row w (w < nw): the fields that are not zero.
__device__ __forceinline__ void cmp_add(const CmpAcc& acc, int w, int nw, unsigned long long* s64,
                                        uint32_t (*s32)[6]) {
    if (w >= nw) return;
    if (acc.dist) atomicAdd(&s64[w], acc.dist);
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const uint32_t v = ((f < 3 ? acc.c0 : acc.c1) >> (10 * (f % 3))) & 0x3FFu;
        if (v) atomicAdd(&s32[w][f], v);
    }
}

__device__ __forceinline__ void cmp_wave_sum(CmpAcc& acc) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        acc.dist += __shfl_xor(acc.dist, off, 64);
        acc.c0 += __shfl_xor(acc.c0, off, 64);
        acc.c1 += __shfl_xor(acc.c1, off, 64);
    }
}

__global__ __launch_bounds__(kThreads) void cmp_tile_kernel(const uint32_t* __restrict__ planes_a, int64_t stride_a,
                                                           const uint32_t* __restrict__ planes_b, int64_t stride_b,
                                                           const Tile* __restrict__ tiles,
                                                           const DivTile* __restrict__ dt, DivArgs da,
                                                           int64_t* __restrict__ rows,
                                                           unsigned long long* __restrict__ bad) {
    __shared__ unsigned long long s64[kDivRows];      // dist_fix
    __shared__ uint32_t s32[kDivRows][6];             // covered_a, covered_b, compared, con_diff, pop_diff, snv
    const Tile t = tiles[blockIdx.x];
    const DivTile d = dt[blockIdx.x];
    const int nw = div_window_of(d.off + t.n - 1, da.window) + 1;    // at most kDivRows - 1
    for (int j = threadIdx.x; j < nw; j += kThreads) s64[j] = 0;
    for (int j = threadIdx.x; j < nw * 6; j += kThreads) s32[j / 6][j % 6] = 0;
    __syncthreads();

    // elements [4 * thread, 4 * thread + 4) of the aligned window; position k = element - lead
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int e0 = 4 * (int)threadIdx.x;
    const int k_lo = max(256 * wave - t.lead, 0), k_hi = min(256 * wave + 255 - t.lead, t.n - 1);   // the wave's
    if (k_lo <= k_hi) {
        const int w_lo = div_window_of(d.off + k_lo, da.window), w_hi = div_window_of(d.off + k_hi, da.window);
        const bool together = w_hi - w_lo <= 1;                      // wave-uniform
        CmpAcc acc[2] = {{0, 0, 0}, {0, 0, 0}};
        int w_base = w_lo;
        if (e0 + 3 >= t.lead && e0 < t.lead + t.n) {
            const int64_t g = t.out - t.lead + e0;                   // 16-byte aligned, inside either plane's stride
            const uint4 aa = *reinterpret_cast<const uint4*>(planes_a + g);
            const uint4 ac = *reinterpret_cast<const uint4*>(planes_a + stride_a + g);
            const uint4 ag = *reinterpret_cast<const uint4*>(planes_a + 2 * stride_a + g);
            const uint4 at = *reinterpret_cast<const uint4*>(planes_a + 3 * stride_a + g);
            const uint4 ba = *reinterpret_cast<const uint4*>(planes_b + g);
            const uint4 bc = *reinterpret_cast<const uint4*>(planes_b + stride_b + g);
            const uint4 bg = *reinterpret_cast<const uint4*>(planes_b + 2 * stride_b + g);
            const uint4 bt = *reinterpret_cast<const uint4*>(planes_b + 3 * stride_b + g);
            const uint32_t xa[4] = {aa.x, aa.y, aa.z, aa.w}, xc[4] = {ac.x, ac.y, ac.z, ac.w};
            const uint32_t xg[4] = {ag.x, ag.y, ag.z, ag.w}, xt[4] = {at.x, at.y, at.z, at.w};
            const uint32_t ya[4] = {ba.x, ba.y, ba.z, ba.w}, yc[4] = {bc.x, bc.y, bc.z, bc.w};
            const uint32_t yg[4] = {bg.x, bg.y, bg.z, bg.w}, yt[4] = {bt.x, bt.y, bt.z, bt.w};
            const int k_first = max(e0 - t.lead, 0);                 // the lane's first position
            if (!together) w_base = div_window_of(d.off + k_first, da.window);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = e0 + j - t.lead;
                if (k >= 0 && k < t.n) {
                    const uint32_t a[4] = {xa[j], xc[j], xg[j], xt[j]};
                    const uint32_t b[4] = {ya[j], yc[j], yg[j], yt[j]};
                    const int w = div_window_of(d.off + k, da.window);
                    if (w == w_base)
                        cmp_position(a, b, da, t.out + k, acc[0], bad);
                    else
                        cmp_position(a, b, da, t.out + k, acc[1], bad);
                }
            }
        }
        if (together) {
            cmp_wave_sum(acc[0]);
            if (w_hi != w_lo) cmp_wave_sum(acc[1]);
            if ((threadIdx.x & 63) == 0) {
                cmp_add(acc[0], w_lo, nw, s64, s32);
                if (w_hi != w_lo) cmp_add(acc[1], w_hi, nw, s64, s32);
            }
        } else {
            cmp_add(acc[0], w_base, nw, s64, s32);
            cmp_add(acc[1], w_base + 1, nw, s64, s32);
        }
    }
    __syncthreads();

    for (int j = threadIdx.x; j < nw * kCmpCols; j += kThreads) {
        const int w = j >> 3, c = j & 7;
        int64_t v;
        if (c == 0) {                                                // the window's positions inside the tile
            const int64_t a = (int64_t)w * da.window - d.off, z = a + da.window;
            v = (z < t.n ? z : (int64_t)t.n) - (a > 0 ? a : 0);
        } else if (c == 7) {
            v = (int64_t)s64[w];
        } else {
            v = (int64_t)s32[w][c - 1];
        }
        int64_t* dst = rows + (d.win + w) * kCmpCols + c;
        if (w == 0 || w == nw - 1) {                                 // perhaps shared with a neighbour: zeroed before
            if (v) atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)v);
        } else {
            *dst = v;
        }
    }
}
