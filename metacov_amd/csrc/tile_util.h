// What the tile modules (runs.hip, windows.hip, bases.hip) share: the HIP
// error macro (also engine.hip's, ecor.hip's, exp_gpu.hip's and
// bam_gpu.hip's), the grow-only device array and the one-workgroup prefix
// scan over per-tile counts.  Only scan.hip keeps a copy of the macro of its
// own.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

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

}  // namespace mc
