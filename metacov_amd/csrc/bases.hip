// Per-position base counts: what the reads say at each position (A, C, G, T,
// N, deletion), the form pysam's AlignmentFile.count_coverage(), samtools
// mpileup, pysamstats and bam-readcount report (nothing in the reference,
// whose pileup only reads PileupColumn.n), and the variant sites among them.
//
// The contract (include/metacov_amd.h, "per-position base counts") in short:
// every read walks its CIGAR from pos with qpos = 0; M/=/X count the base at
// (qpos, rpos) into its channel, D counts DEL, N advances the reference, I/S
// the query, H/P nothing.  nt16 codes 1/2/4/8 are A/C/G/T, every other code
// is N.  A base below min_baseq counts nothing unless the read's qualities
// are absent (first byte 0xFF); DEL takes no quality test.  The planes are
// counts[6][N] over the concatenated segments of mc_bases_begin.
//
// Launches, all on the handle's stream, none waiting on another workgroup:
//   bases_prepass_kernel  one thread per read of a batch: reference span and
//                         query length of its CIGAR, the validity checks
//                         (order against the predecessor as one 64-bit
//                         compare), the lowest bad index through an atomic
//                         min and the batch's largest span through an atomic
//                         max per wave.  The host reads those two words.
//   bases_pileup_kernel   one 512-thread workgroup per tile of at most kTile
//                         positions of one segment; only the tiles between
//                         the batch's first and last read in (tid, position)
//                         order are launched.  Two binary searches in the
//                         sorted batch give the reads of the tile's
//                         contig with pos in [tile start - max span, tile
//                         end); a tile with none returns before touching LDS
//                         or HBM.  Waves take the reads 64 at a time: lane i
//                         loads read i's words, then the reads that reach
//                         the tile are walked in turn with those words
//                         broadcast; the CIGAR op loop is wave-uniform
//                         (scalar loads of further ops); lanes stride over
//                         the op's positions clipped to the tile; one
//                         LDS integer add per counted base into 6 planes x
//                         kTile x 4 B = 48 KiB.  The flush adds the LDS
//                         planes into the global ones, 16 bytes per lane,
//                         with plain load-add-store: a tile has one owner in
//                         a launch and the launches of successive batches
//                         are ordered on the stream.  No global atomics.
//   bases_pileup_kernel<kModeStrand>   the same walk on a handle that tracks strand
//                         (pileup_tile<true>): the reads' flags beside their
//                         other words, forward and reverse counts in the two
//                         16-bit halves of the same LDS words (two 32-bit
//                         walks for a tile with more than 65535 reads), the
//                         flush into the totals and the reverse planes.
//   bases_pileup_kernel<kModeQuality>  the same walk on a handle that tracks quality
//                         (pileup_tile<kModeQuality>): the reads' MAPQ bytes
//                         beside their other words, one 64-bit LDS add per
//                         counted base (count, quality byte, MAPQ in 16 + 24 +
//                         24 bits), kQSub workgroups per tile with kQTile
//                         8-byte cells each (the same 48 KiB), the reads in
//                         groups of at most kQGroup with a flush after each
//                         into the count, bq and mq planes.
//   bases_ends_kernel     mc_bases_add_batch_device only (the batch is in
//                         device memory, e.g. the GPU decoder's bases-mode
//                         table): one thread writes the first and last read's
//                         (tid, pos) behind the pre-pass flags, so the words
//                         the host needs come back in the same small copy.
//   sites_count / scan / emit   the count - scan - emit pattern of runs.hip
//                         over the planes with the site predicate; the host
//                         reads the total (8 bytes) between scan and emit.
//   cons_call / scan / emit     the consensus letters (see the kernels): the
//                         same pattern, the emit over the 1-byte letters.
//   ins_* / cons_ins_*    the opt-in insertion stage (bases_ins.h): events per
//                         batch behind the pileup launch, grouped into the
//                         allele table, called into the compact consensus.
//
// A tile whose first plane index is not 16-byte aligned starts `lead` (1..3)
// elements into its LDS window and holds at most kTile - lead positions, so
// LDS element k always pairs with plane element out - lead + k and the
// 16-byte flush is aligned; window elements outside the tile are never
// counted into and never written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/metacov_amd.h"
#include "common.h"
#include "tile_util.h"

namespace {

using mc::kScanThreads;

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 2048;                         // positions per tile: 6 x 4 B x 2048 = 48 KiB of LDS
constexpr int kPlanes = 6;                          // A, C, G, T, N, DEL
constexpr int kRounds = kTile / kThreads;           // positions per thread of the sites kernels
using mc::kMaxPos;
constexpr unsigned long long kNoBad = ~0ull;
constexpr uint32_t kQueryOps = 0x193u;              // M I S = X advance the query
constexpr uint32_t kRefOps = 0x18Du;                // M D N = X advance the reference
constexpr int kModePlain = 0, kModeStrand = 1, kModeQuality = 2;   // what a kernel keeps beside the counts
constexpr int kQTile = 1024;                        // positions per workgroup of the quality pileup: 48 KiB of cells
constexpr int kQSub = kTile / kQTile;               // its workgroups per tile, one per kQTile elements of the window
constexpr int64_t kQGroup = 65535;                  // reads per walk of it: 16-bit count, 24-bit sums, no carry

struct Tile {
    int64_t out;       // plane index of the tile's first position
    int64_t rel;       // contig-relative position of it
    int32_t n;         // positions (lead + n <= kTile)
    int32_t tid;
    int32_t seg;
    int32_t lead;      // out & 3: elements of the aligned window in front of it
};
static_assert(sizeof(Tile) == 32, "tile table entry");

// One batch of reads in device memory (the layout of mc_bases_add_batch).
struct Batch {
    const int32_t* tid;
    const int32_t* pos;
    const int32_t* l_seq;
    const int64_t* cig_off;
    const uint32_t* cigar;
    const int64_t* seq_off;
    const uint8_t* seq;
    const int64_t* qual_off;
    const uint8_t* qual;
    int64_t n, n_words, seq_bytes, qual_bytes;
};

struct SiteArgs {
    unsigned long long min_depth, min_count, min_ppm;
};

__device__ __forceinline__ long long read_key(int32_t tid, int32_t pos) {
    return (long long)(((unsigned long long)(uint32_t)tid << 32) | (uint32_t)pos);
}

__global__ __launch_bounds__(kThreads) void bases_prepass_kernel(Batch b, int32_t n_ref,
                                                                int32_t* __restrict__ span,
                                                                unsigned long long* __restrict__ bad,
                                                                int32_t* __restrict__ max_span) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int32_t sp = 0;
    if (i < b.n) {
        const int32_t tid = b.tid[i], pos = b.pos[i], l = b.l_seq[i];
        const int64_t c0 = b.cig_off[i], c1 = b.cig_off[i + 1];
        const int64_t so = b.seq_off[i], qo = b.qual_off[i];
        bool ok = tid >= 0 && tid < n_ref && pos >= 0 && l >= 0 && c0 >= 0 && c1 >= c0 && c1 <= b.n_words;
        ok = ok && so >= 0 && so + ((int64_t)l + 1) / 2 <= b.seq_bytes && qo >= 0 && qo + l <= b.qual_bytes;
        if (ok && i > 0) ok = read_key(b.tid[i - 1], b.pos[i - 1]) <= read_key(tid, pos);
        if (ok) {
            int64_t q = 0, r = 0;
            for (int64_t k = c0; k < c1; ++k) {
                const uint32_t cw = b.cigar[k];
                const uint32_t op = cw & 15u;
                if ((kQueryOps >> op) & 1u) q += cw >> 4;
                if ((kRefOps >> op) & 1u) r += cw >> 4;
            }
            ok = q == l && r <= INT32_MAX;
            if (ok) sp = (int32_t)r;
        }
        span[i] = sp;
        if (!ok) atomicMin(bad, (unsigned long long)i);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sp = max(sp, __shfl_xor(sp, off, 64));
    // (the plain look first: after the first waves nearly every wave's maximum is already there, and
    // same-address atomics serialise)
    if ((threadIdx.x & 63) == 0 && sp > __atomic_load_n(max_span, __ATOMIC_RELAXED)) atomicMax(max_span, sp);
}

// Lane i's value, wave-uniform (i is wave-uniform).
__device__ __forceinline__ int32_t bcast(int32_t v, int i) { return __builtin_amdgcn_readlane(v, i); }
__device__ __forceinline__ int64_t bcast64(int64_t v, int i) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)v, i);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)((uint64_t)v >> 32), i);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// First read at or after (tid, pos) in the sorted batch; at most 64 steps.
__device__ __forceinline__ int64_t lower_bound(const Batch& b, int32_t tid, int64_t pos) {
    int64_t a = 0, z = b.n;
    while (a < z) {
        const int64_t m = a + ((z - a) >> 1);
        const int32_t mt = b.tid[m];
        if (mt < tid || (mt == tid && (int64_t)b.pos[m] < pos))
            a = m + 1;
        else
            z = m;
    }
    return a;
}

// One tile of a batch (the launch comment above).  kStrand: the reads' flags
// are read too and the counts of the reverse-strand reads (flag & 0x10) also
// go into the rev planes, in the same 48 KiB of LDS.  A tile that looks at no
// more than 65535 reads counts both strands in one walk, forward in the low
// and reverse in the high 16 bits of each LDS word (a read covers a position
// at most once, so neither half can carry); a tile with more reads walks them
// twice with full 32-bit words, the forward reads first, then the reverse
// ones.  Both conditions are uniform over the workgroup.
// kQuality: the reads' mapq bytes are read too and every counted base adds
// one 64-bit LDS word that carries three fields, the count in bits 0..15, the
// quality byte in bits 16..39 and the read's MAPQ in bits 40..63 (DEL: no
// quality).  Cells of 8 bytes: a workgroup owns kQTile elements of the tile's
// window, so the LDS stays 48 KiB and a tile is kQSub workgroups, each with
// its own binary searches and its own part of the planes.  The reads are
// walked in groups of at most kQGroup with a flush after each: a read covers a
// position at most once, so within a group the count stays below 2^16 and both
// sums below 2^24 and no field carries into the next.  The flush unpacks the
// fields and adds them into the count, bq and mq planes.
template <int kMode>
__device__ __forceinline__ void pileup_tile(const Batch& b, const int32_t* __restrict__ span,
                                            const Tile* __restrict__ tiles, const int32_t* __restrict__ order,
                                            int32_t max_span, int32_t min_baseq, uint32_t* __restrict__ planes,
                                            int64_t stride, const uint16_t* __restrict__ flag,
                                            uint32_t* __restrict__ rev, const uint8_t* __restrict__ mapq,
                                            uint32_t* __restrict__ bq, uint32_t* __restrict__ mq) {
    constexpr bool kStrand = kMode == kModeStrand, kQual = kMode == kModeQuality;
    constexpr int kW = kQual ? kQTile : kTile;              // elements of the LDS window
    using Cell = typename std::conditional<kQual, unsigned long long, uint32_t>::type;
    __shared__ __attribute__((aligned(16))) Cell acc[kPlanes * kW];
    Tile t = tiles[order[kQual ? blockIdx.x / kQSub : blockIdx.x]];
    if (kQual) {                                            // this workgroup's part of the tile's window
        const int w0 = (int)(blockIdx.x % kQSub) * kW;
        const int a = t.lead > w0 ? t.lead : w0, z = t.lead + t.n < w0 + kW ? t.lead + t.n : w0 + kW;
        if (a >= z) return;
        t.out += a - t.lead;
        t.rel += a - t.lead;
        t.n = z - a;
        t.lead = a - w0;                                    // (out - lead stays 16-byte aligned: w0 is a multiple of 4)
    }
    const int64_t t0 = t.rel, t1 = t.rel + t.n;
    const int64_t lo = lower_bound(b, t.tid, t0 > max_span ? t0 - max_span : 0);
    const int64_t hi = lower_bound(b, t.tid, t1);
    if (lo >= hi) return;
    const bool packed = kStrand && hi - lo <= 65535;
    const int passes = kQual ? (int)((hi - lo + kQGroup - 1) / kQGroup) : kStrand && !packed ? 2 : 1;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (int pass = 0; pass < passes; ++pass) {
        if ((kStrand || kQual) && pass) __syncthreads();    // the pass before has flushed the window
        if constexpr (kQual) {
            for (int k = threadIdx.x * 2; k < kPlanes * kW; k += kThreads * 2)
                *reinterpret_cast<uint4*>(&acc[k]) = make_uint4(0, 0, 0, 0);
        } else {
            for (int k = threadIdx.x * 4; k < kPlanes * kTile; k += kThreads * 4)
                *reinterpret_cast<uint4*>(&acc[k]) = make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
        const int64_t glo = kQual ? lo + pass * kQGroup : lo;                          // this pass's reads
        const int64_t ghi = kQual && glo + kQGroup < hi ? glo + kQGroup : hi;
        // A wave takes 64 consecutive reads at a time: lane i loads read i's words (coalesced, independent
        // loads), then the reads that reach the tile are walked one by one with those words broadcast.
        for (int64_t g = glo + 64 * (int64_t)wave; g < ghi; g += 64 * kWaves) {
            const int64_t mine = g + lane;
            const bool have = mine < ghi;
            const int32_t m_pos = have ? b.pos[mine] : 0;
            const int32_t m_span = have ? span[mine] : 0;
            const int32_t m_l = have ? b.l_seq[mine] : 0;
            const int64_t m_c0 = have ? b.cig_off[mine] : 0, m_c1 = have ? b.cig_off[mine + 1] : 0;
            const int64_t m_so = have ? b.seq_off[mine] : 0, m_qo = have ? b.qual_off[mine] : 0;
            const uint32_t m_cw = m_c1 > m_c0 ? b.cigar[m_c0] : 0u;        // the first op: the only one of most reads
            const int32_t m_q0 = m_l > 0 ? (int32_t)b.qual[m_qo] : 0;
            int32_t m_rev = 0;
            if (kStrand) m_rev = have ? (int32_t)((flag[mine] >> 4) & 1u) : 0;
            int32_t m_mq = 0;
            if (kQual) m_mq = have ? (int32_t)mapq[mine] : 0;
            unsigned long long todo = __ballot(have && (int64_t)m_pos + m_span > t0 &&
                                               (!kStrand || packed || m_rev == pass));
            while (todo) {
                const int i = __ffsll(todo) - 1;
                todo &= todo - 1;
                const int64_t pos = bcast(m_pos, i), l = bcast(m_l, i);
                const int64_t c0 = bcast64(m_c0, i), c1 = bcast64(m_c1, i);
                const int64_t so = bcast64(m_so, i), qo = bcast64(m_qo, i);
                const bool test_q = min_baseq > 0 && !(l > 0 && bcast(m_q0, i) == 0xFF);
                bool absent = false;
                if (kQual) absent = l > 0 && bcast(m_q0, i) == 0xFF;
                Cell one = 1u;
                if (kStrand) one = packed && bcast(m_rev, i) ? 0x10000u : 1u;
                if (kQual) one = (Cell)1u | ((unsigned long long)(uint32_t)bcast(m_mq, i) << 40);
                int64_t rp = pos, q = 0;
                for (int64_t k = c0; k < c1 && rp < t1; ++k) {
                    const uint32_t cw = k == c0 ? (uint32_t)bcast((int32_t)m_cw, i) : b.cigar[k];
                    const uint32_t op = cw & 15u;
                    const int64_t len = cw >> 4;
                    if (op == 0 || op == 7 || op == 8) {
                        const int64_t e = rp + len < t1 ? rp + len : t1;
                        for (int64_t j = (rp > t0 ? rp : t0) + lane; j < e; j += 64) {
                            const int64_t qq = q + (j - rp);
                            if (qq < l) {
                                const uint32_t byte = b.seq[so + (qq >> 1)];
                                const uint32_t code = (qq & 1) ? (byte & 15u) : (byte >> 4);
                                if (kQual) {                // the byte is summed too: absent qualities add 0
                                    const uint32_t qv = absent ? 0u : (uint32_t)b.qual[qo + qq];
                                    if (!test_q || (int32_t)qv >= min_baseq) {
                                        const int ch =
                                            code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 8 ? 3 : 4;
                                        atomicAdd(&acc[ch * kW + t.lead + (int)(j - t0)],
                                                  (Cell)(one + ((unsigned long long)qv << 16)));
                                    }
                                } else if (!test_q || (int32_t)b.qual[qo + qq] >= min_baseq) {
                                    const int ch = code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 8 ? 3 : 4;
                                    atomicAdd(&acc[ch * kW + t.lead + (int)(j - t0)], one);
                                }
                            }
                        }
                        rp += len;
                        q += len;
                    } else if (op == 2) {
                        const int64_t e = rp + len < t1 ? rp + len : t1;
                        for (int64_t j = (rp > t0 ? rp : t0) + lane; j < e; j += 64)
                            atomicAdd(&acc[5 * kW + t.lead + (int)(j - t0)], one);
                        rp += len;
                    } else if (op == 3) {
                        rp += len;
                    } else if (op == 1 || op == 4) {
                        q += len;
                    }
                }
            }
        }
        __syncthreads();
        const int first = t.lead, last = t.lead + t.n;          // the tile's part of the window
        if constexpr (kQual) {
            // four cells per thread, the three fields of each into their plane sets (bq of DEL is never added to)
            for (int e = threadIdx.x * 4; e < kPlanes * kW; e += kThreads * 4) {
                const int c = e / kW, k = e % kW;
                const uint4 lo2 = *reinterpret_cast<const uint4*>(&acc[e]);
                const uint4 hi2 = *reinterpret_cast<const uint4*>(&acc[e + 2]);
                if (!(lo2.x | lo2.z | hi2.x | hi2.z)) continue;    // (a cell's count is in its low word)
                const unsigned long long w[4] = {lo2.x | ((unsigned long long)lo2.y << 32),
                                                 lo2.z | ((unsigned long long)lo2.w << 32),
                                                 hi2.x | ((unsigned long long)hi2.y << 32),
                                                 hi2.z | ((unsigned long long)hi2.w << 32)};
                uint32_t vc[4], vb[4], vm[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    vc[i] = (uint32_t)(w[i] & 0xFFFFu);
                    vb[i] = (uint32_t)(w[i] >> 16) & 0xFFFFFFu;
                    vm[i] = (uint32_t)(w[i] >> 40);
                }
                const int64_t o = c * stride + (t.out - t.lead) + k;   // 16-byte aligned
                if (k >= first && k + 4 <= last) {
                    uint32_t* const dst[3] = {planes + o, bq + o, mq + o};
                    const uint32_t* const src[3] = {vc, vb, vm};
#pragma unroll
                    for (int f = 0; f < 3; ++f) {
                        if (!(src[f][0] | src[f][1] | src[f][2] | src[f][3])) continue;
                        uint4 x = *reinterpret_cast<const uint4*>(dst[f]);
                        x.x += src[f][0]; x.y += src[f][1]; x.z += src[f][2]; x.w += src[f][3];
                        *reinterpret_cast<uint4*>(dst[f]) = x;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (vc[i] && k + i >= first && k + i < last) {
                            planes[o + i] += vc[i];
                            if (vb[i]) bq[o + i] += vb[i];
                            if (vm[i]) mq[o + i] += vm[i];
                        }
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < kPlanes; ++c) {
                uint32_t* g = planes + c * stride + (t.out - t.lead);   // 16-byte aligned
                uint32_t* gr = kStrand ? rev + c * stride + (t.out - t.lead) : nullptr;
                for (int k = threadIdx.x * 4; k < kTile; k += kThreads * 4) {
                    uint4 v = *reinterpret_cast<const uint4*>(&acc[c * kTile + k]);
                    if (!(v.x | v.y | v.z | v.w)) continue;
                    uint4 r = make_uint4(0, 0, 0, 0);               // the reverse strand's share of v
                    if (kStrand) {
                        if (packed) {
                            r = make_uint4(v.x >> 16, v.y >> 16, v.z >> 16, v.w >> 16);
                            v = make_uint4((v.x & 0xFFFFu) + r.x, (v.y & 0xFFFFu) + r.y, (v.z & 0xFFFFu) + r.z,
                                           (v.w & 0xFFFFu) + r.w);
                        } else if (pass) {
                            r = v;
                        }
                    }
                    if (k >= first && k + 4 <= last) {
                        uint4 o = *reinterpret_cast<const uint4*>(g + k);
                        o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
                        *reinterpret_cast<uint4*>(g + k) = o;
                        if (kStrand && (r.x | r.y | r.z | r.w)) {
                            uint4 p = *reinterpret_cast<const uint4*>(gr + k);
                            p.x += r.x; p.y += r.y; p.z += r.z; p.w += r.w;
                            *reinterpret_cast<uint4*>(gr + k) = p;
                        }
                    } else {
                        const uint32_t e[4] = {v.x, v.y, v.z, v.w};
                        const uint32_t er[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (e[i] && k + i >= first && k + i < last) {
                                g[k + i] += e[i];
                                if (kStrand && er[i]) gr[k + i] += er[i];
                            }
                    }
                }
            }
        }
    }
}

// What a mode's pileup kernel takes beside the plain arguments: nothing, flag[n] beside the batch's per-read
// columns and the reverse planes, or mapq[n] and the two sum plane sets (all indexed like planes).  A plain
// handle's kernel so carries no strand or quality argument.
template <int kMode>
struct PileupMode {};
template <>
struct PileupMode<kModeStrand> {
    const uint16_t* flag;
    uint32_t* rev;
};
template <>
struct PileupMode<kModeQuality> {
    const uint8_t* mapq;
    uint32_t *bq, *mq;
};

// One workgroup per tile (kQSub per tile in the quality mode).
template <int kMode>
__global__ __launch_bounds__(kThreads) void bases_pileup_kernel(Batch b, const int32_t* __restrict__ span,
                                                               const Tile* __restrict__ tiles,
                                                               const int32_t* __restrict__ order, int32_t max_span,
                                                               int32_t min_baseq, uint32_t* __restrict__ planes,
                                                               int64_t stride, PileupMode<kMode> m) {
    if constexpr (kMode == kModeStrand)
        pileup_tile<kMode>(b, span, tiles, order, max_span, min_baseq, planes, stride, m.flag, m.rev, nullptr, nullptr,
                           nullptr);
    else if constexpr (kMode == kModeQuality)
        pileup_tile<kMode>(b, span, tiles, order, max_span, min_baseq, planes, stride, nullptr, nullptr, m.mapq, m.bq,
                           m.mq);
    else
        pileup_tile<kMode>(b, span, tiles, order, max_span, min_baseq, planes, stride, nullptr, nullptr, nullptr,
                           nullptr, nullptr);
}

// depth = A + C + G + T + DEL; the base allele is ref (0..3) where given,
// else the allele with the highest count (ties: the lowest channel).  64-bit
// integers only.  The plain predicate (kStrand false; r and min_alt unused): alt,
// the highest count among the other four, passes min_count and min_ppm.  The
// strand predicate (mc_bases_sites_strand): a site needs one allele besides the
// base allele that passes min_count and min_ppm and is seen min_alt times on
// each strand (r: the reverse counts; forward = total - reverse).  With
// min_alt == 0 this is the plain predicate: both count tests are monotone in
// the count, so some allele passes them iff the strongest does.  The quality
// predicate (mc_bases_sites_quality; r: the bq sums, m: the mq sums, min_alt:
// min_alt_baseq, min_mq: min_alt_mapq): the allele's sums also reach the
// thresholds times its count, DEL (index 4) with no baseq test; with both 0
// it is the plain predicate for the same reason.
template <int kMode>
__device__ __forceinline__ bool is_site(const uint32_t (&a)[5], const uint32_t (&r)[5], const uint32_t (&m)[5], int ref,
                                        const SiteArgs& s, uint32_t min_alt, uint32_t min_mq) {
    constexpr bool kStrand = kMode != kModePlain;
    const unsigned long long depth = (unsigned long long)a[0] + a[1] + a[2] + a[3] + a[4];
    int base = 0;
    if (ref >= 0 && ref < 4) {
        base = ref;
    } else {
#pragma unroll
        for (int i = 1; i < 5; ++i)
            if (a[i] > a[base]) base = i;
    }
    if (!kStrand) {
        unsigned long long alt = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i)
            if (i != base && a[i] > alt) alt = a[i];
        return depth >= s.min_depth && alt >= s.min_count && alt * 1000000ull >= s.min_ppm * depth;
    }
    bool any = false;
    if (kMode == kModeQuality) {
#pragma unroll
        for (int i = 0; i < 5; ++i)
            any = any || (i != base && a[i] >= s.min_count && a[i] * 1000000ull >= s.min_ppm * depth &&
                          m[i] >= (unsigned long long)min_mq * a[i] &&
                          (i == 4 || r[i] >= (unsigned long long)min_alt * a[i]));
        return depth >= s.min_depth && any;
    }
#pragma unroll
    for (int i = 0; i < 5; ++i)
        any = any || (i != base && a[i] >= s.min_count && a[i] * 1000000ull >= s.min_ppm * depth &&
                      r[i] >= min_alt && a[i] - r[i] >= min_alt);
    return depth >= s.min_depth && any;
}

// Bit r of the result: position r * kThreads + threadIdx.x of tile t is a site.
// rev (the reverse planes, or the bq planes) is read only when kMode is not
// kModePlain, mqp (the mq planes) only when it is kModeQuality.
template <int kMode>
__device__ __forceinline__ uint32_t site_flags(const uint32_t* __restrict__ planes, const uint32_t* __restrict__ rev,
                                               const uint32_t* __restrict__ mqp, int64_t stride,
                                               const uint8_t* __restrict__ ref, const Tile& t, const SiteArgs& s,
                                               uint32_t min_alt, uint32_t min_mq) {
    constexpr bool kStrand = kMode != kModePlain;
    uint32_t fm = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int k = r * kThreads + (int)threadIdx.x;
        if (k < t.n) {
            const int64_t i = t.out + k;
            const uint32_t a[5] = {planes[i], planes[stride + i], planes[2 * stride + i], planes[3 * stride + i],
                                   planes[5 * stride + i]};
            uint32_t b[5] = {0, 0, 0, 0, 0};
            if (kStrand) {
                b[0] = rev[i], b[1] = rev[stride + i], b[2] = rev[2 * stride + i], b[3] = rev[3 * stride + i];
                b[4] = rev[5 * stride + i];
            }
            uint32_t m[5] = {0, 0, 0, 0, 0};
            if (kMode == kModeQuality) {
                m[0] = mqp[i], m[1] = mqp[stride + i], m[2] = mqp[2 * stride + i], m[3] = mqp[3 * stride + i];
                m[4] = mqp[5 * stride + i];
            }
            fm |= (uint32_t)is_site<kMode>(a, b, m, ref ? (int)ref[i] : 4, s, min_alt, min_mq) << r;
        }
    }
    return fm;
}

// The tile's sites from its threads' flag words: positions and counts in
// position order (mc::tile_offsets' order with a 64-bit running offset of its
// own: through the helper the three emit kernels held 10 to 16 more VGPRs and
// the strand one measured slower); site_rev (or null): the reverse counts (or the bq sums)
// beside them; site_mq (or null): the mq sums.
__device__ __forceinline__ void sites_emit_tile(uint32_t fm, const Tile& t, const uint32_t* __restrict__ planes,
                                                const uint32_t* __restrict__ rev, int64_t stride,
                                                const int64_t* __restrict__ base, int64_t* __restrict__ site_pos,
                                                uint32_t* __restrict__ site_counts,
                                                uint32_t* __restrict__ site_rev,
                                                const uint32_t* __restrict__ mqp = nullptr,
                                                uint32_t* __restrict__ site_mq = nullptr) {
    __shared__ int32_t wcnt[kRounds][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t rank[kRounds];                                  // sites of this round in lower lanes of the wave
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const unsigned long long m = __ballot((fm >> r) & 1);
        rank[r] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
        if (lane == 0) wcnt[r][wave] = __popcll(m);
    }
    __syncthreads();
    int64_t run = base[blockIdx.x];                         // positions ascend with (round, wave, lane)
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        int64_t mine = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w == wave) mine = run;
            run += wcnt[r][w];
        }
        if ((fm >> r) & 1) {
            const int k = r * kThreads + (int)threadIdx.x;
            const int64_t o = mine + rank[r], i = t.out + k;
            site_pos[o] = t.rel + k;
#pragma unroll
            for (int c = 0; c < kPlanes; ++c) site_counts[o * kPlanes + c] = planes[c * stride + i];
            if (site_rev) {
#pragma unroll
                for (int c = 0; c < kPlanes; ++c) site_rev[o * kPlanes + c] = rev[c * stride + i];
            }
            if (site_mq) {
#pragma unroll
                for (int c = 0; c < kPlanes; ++c) site_mq[o * kPlanes + c] = mqp[c * stride + i];
            }
        }
    }
}

// What a mode's sites kernels take beside the plain arguments: nothing, the
// reverse planes with min_alt and the sites' reverse counts, or the bq and mq
// planes with both thresholds and the sites' sums.  The count kernel leaves the
// output pointers alone.  A plain handle's kernels so carry no strand or
// quality argument.
template <int kMode>
struct SitesMode {};
template <>
struct SitesMode<kModeStrand> {
    const uint32_t* rev;
    uint32_t min_alt;
    uint32_t* site_rev;
};
template <>
struct SitesMode<kModeQuality> {
    const uint32_t *bq, *mq;
    uint32_t min_bq, min_mq;
    uint32_t *site_bq, *site_mq;
};

template <int kMode>
__device__ __forceinline__ uint32_t mode_site_flags(const uint32_t* __restrict__ planes, int64_t stride,
                                                    const uint8_t* __restrict__ ref, const Tile& t, const SiteArgs& s,
                                                    const SitesMode<kMode>& m) {
    if constexpr (kMode == kModeStrand)
        return site_flags<kMode>(planes, m.rev, nullptr, stride, ref, t, s, m.min_alt, 0);
    else if constexpr (kMode == kModeQuality)
        return site_flags<kMode>(planes, m.bq, m.mq, stride, ref, t, s, m.min_bq, m.min_mq);
    else
        return site_flags<kMode>(planes, nullptr, nullptr, stride, ref, t, s, 0, 0);
}

template <int kMode>
__global__ __launch_bounds__(kThreads) void sites_count_kernel(const uint32_t* __restrict__ planes, int64_t stride,
                                                              const uint8_t* __restrict__ ref,
                                                              const Tile* __restrict__ tiles, SiteArgs s,
                                                              SitesMode<kMode> m, int32_t* __restrict__ counts) {
    const Tile t = tiles[blockIdx.x];
    mc::tile_count<kWaves>(mode_site_flags<kMode>(planes, stride, ref, t, s, m), counts);
}

// One workgroup.  base[i] = sum of counts[0, i) for i <= n_tiles, then
// seg_first[s] = base[seg_tile[s]] for s <= S (runs.hip's scan kernel).  The
// scan of the sites, of the insertion rows and of the consensus' two insertion
// columns; with S = -1 and null segment arrays the scan alone, for the
// insertion events' counts per tile.
__global__ __launch_bounds__(kScanThreads) void tile_scan_kernel(const int32_t* __restrict__ counts, int64_t n_tiles,
                                                                int64_t* __restrict__ base,
                                                                const int64_t* __restrict__ seg_tile, int64_t S,
                                                                int64_t* __restrict__ seg_first) {
    mc::tile_scan(counts, n_tiles, base);
    for (int64_t s = threadIdx.x; s <= S; s += kScanThreads) seg_first[s] = base[seg_tile[s]];
}

template <int kMode>
__global__ __launch_bounds__(kThreads) void sites_emit_kernel(const uint32_t* __restrict__ planes, int64_t stride,
                                                             const uint8_t* __restrict__ ref,
                                                             const Tile* __restrict__ tiles, SiteArgs s,
                                                             SitesMode<kMode> m, const int64_t* __restrict__ base,
                                                             int64_t* __restrict__ site_pos,
                                                             uint32_t* __restrict__ site_counts) {
    const Tile t = tiles[blockIdx.x];
    const uint32_t fm = mode_site_flags<kMode>(planes, stride, ref, t, s, m);
    if constexpr (kMode == kModeStrand)
        sites_emit_tile(fm, t, planes, m.rev, stride, base, site_pos, site_counts, m.site_rev);
    else if constexpr (kMode == kModeQuality)
        sites_emit_tile(fm, t, planes, m.bq, stride, base, site_pos, site_counts, m.site_bq, m.mq, m.site_mq);
    else
        sites_emit_tile(fm, t, planes, nullptr, stride, base, site_pos, site_counts, nullptr);
}

// ---- consensus (the rule is the header's, "Consensus") ----------------------
// cons_call_kernel   one workgroup per tile, the sites kernels' position-to-
//                    thread mapping: five planes and the optional ref read
//                    once, one letter per position into the aligned buffer
//                    (a wave stores 64 consecutive bytes), the tile's eight
//                    summary columns through wave reductions and one LDS step.
// cons_scan_kernel   one workgroup: exclusive prefix sums over the tiles of
//                    each of the eight columns; out_first and the summary rows
//                    are differences of them at the segments' tile ranges.
// cons_emit_kernel   one workgroup per tile: reads the aligned letters (1 B per
//                    position) and writes those that are not '-' in position
//                    order, by ballot ranks per round and wave.
// No global atomics; every loop is bounded by the tile size or the tile count.

constexpr int kConsCols = MC_CONS_COLS;             // positions called ambiguous nocall low deleted differs length

struct ConsArgs {
    unsigned long long min_depth, min_count, call_ppm;   // min_depth and min_count already raised to 1
    uint32_t flags;
};

__device__ __forceinline__ bool cons_qualifies(uint32_t x, unsigned long long depth, const ConsArgs& c) {
    return x >= c.min_count && (unsigned long long)x * 1000000ull >= c.call_ppm * depth;
}

// The letter of a position with counts a[0..4] (A C G T DEL) and reference
// code r.  Its class is counted into packed 10-bit counters: w0 holds called,
// ambiguous, no call at bits 0, 10, 20; w1 holds low, deleted, differs.
__device__ __forceinline__ uint32_t cons_letter(const uint32_t (&a)[5], uint32_t r, const ConsArgs& c,
                                                uint32_t& w0, uint32_t& w1) {
    const unsigned long long depth = (unsigned long long)a[0] + a[1] + a[2] + a[3] + a[4];
    const bool known = r < 4;
    if (depth < c.min_depth) {
        w1 += 1u;
        return ((c.flags & MC_CONS_FILL_REF) && known) ? ((0x74676361u >> (8 * r)) & 0xFFu) : (uint32_t)'N';
    }
    int top = 0;
#pragma unroll
    for (int i = 1; i < 5; ++i)
        if (a[i] > a[top]) top = i;
    if (top == 4) {
        if (!cons_qualifies(a[4], depth, c)) {
            w0 += 1u << 20;
            return 'N';
        }
        w1 += (1u << 10) + (known ? 1u << 20 : 0u);
        return '-';
    }
    uint32_t mask = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) mask |= (uint32_t)cons_qualifies(a[i], depth, c) << i;
    if (!(c.flags & MC_CONS_IUPAC)) mask &= 1u << top;
    if (mask == 0) {
        w0 += 1u << 20;
        return 'N';
    }
    // ".ACMGRSV" and "TWYHKDBN", eight letters per 64-bit word, the first in the low byte
    const unsigned long long tab = mask < 8 ? 0x565352474D43412Eull : 0x4E42444B48595754ull;
    const uint32_t letter = (uint32_t)(tab >> (8 * (mask & 7u))) & 0xFFu;
    if (mask & (mask - 1)) {
        w0 += 1u << 10;
    } else {
        w0 += 1u;
        if (known && (uint32_t)top != r) w1 += 1u << 20;
    }
    return letter;
}

__global__ __launch_bounds__(kThreads) void cons_call_kernel(const uint32_t* __restrict__ planes, int64_t stride,
                                                            const uint8_t* __restrict__ ref,
                                                            const Tile* __restrict__ tiles, int64_t n_tiles,
                                                            ConsArgs ca, uint8_t* __restrict__ aligned,
                                                            int32_t* __restrict__ cols) {
    __shared__ uint32_t wsum[kWaves][2];
    const Tile t = tiles[blockIdx.x];
    uint32_t w0 = 0, w1 = 0;            // three 10-bit counters each: at most 4 per thread, 256 per wave
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int k = r * kThreads + (int)threadIdx.x;
        if (k < t.n) {
            const int64_t i = t.out + k;
            const uint32_t a[5] = {planes[i], planes[stride + i], planes[2 * stride + i], planes[3 * stride + i],
                                   planes[5 * stride + i]};
            aligned[i] = (uint8_t)cons_letter(a, ref ? (uint32_t)ref[i] : 4u, ca, w0, w1);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        w0 += __shfl_xor(w0, off, 64);
        w1 += __shfl_xor(w1, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        wsum[threadIdx.x >> 6][0] = w0;
        wsum[threadIdx.x >> 6][1] = w1;
    }
    __syncthreads();
    if (threadIdx.x < 6) {              // thread c sums counter c of the eight waves
        const int word = threadIdx.x / 3, shift = 10 * (threadIdx.x % 3);
        int32_t sum = 0;
        for (int w = 0; w < kWaves; ++w) sum += (int32_t)((wsum[w][word] >> shift) & 0x3FFu);
        cols[(1 + (int64_t)threadIdx.x) * n_tiles + blockIdx.x] = sum;
        if (threadIdx.x == 4) {         // deleted: the kept count beside it
            cols[blockIdx.x] = t.n;
            cols[7 * n_tiles + blockIdx.x] = t.n - sum;
        }
    }
}

// One workgroup.  For each column c: pre[c][i] = sum of cols[c][0, i) for
// i <= n_tiles (a tile's entry is at most kTile).  Then out_first[s] =
// pre[7][seg_tile[s]] and rows[s][c] = pre[c][seg_tile[s + 1]] -
// pre[c][seg_tile[s]]: a segment's tiles are contiguous, an empty segment has
// none.
__global__ __launch_bounds__(kScanThreads) void cons_scan_kernel(const int32_t* __restrict__ cols, int64_t n_tiles,
                                                                int64_t* __restrict__ pre,
                                                                const int64_t* __restrict__ seg_tile, int64_t S,
                                                                int64_t* __restrict__ out_first,
                                                                int64_t* __restrict__ rows) {
    const int t = threadIdx.x;
    for (int col = 0; col < kConsCols; ++col) mc::tile_scan(cols + col * n_tiles, n_tiles, pre + col * (n_tiles + 1));
    for (int64_t s = t; s <= S; s += kScanThreads) out_first[s] = pre[7 * (n_tiles + 1) + seg_tile[s]];
    for (int64_t j = t; j < S * kConsCols; j += kScanThreads) {
        const int64_t s = j / kConsCols, col = j % kConsCols;
        const int64_t* p = pre + col * (n_tiles + 1);
        rows[j] = p[seg_tile[s + 1]] - p[seg_tile[s]];
    }
}

__global__ __launch_bounds__(kThreads) void cons_emit_kernel(const uint8_t* __restrict__ aligned,
                                                            const Tile* __restrict__ tiles,
                                                            const int64_t* __restrict__ base,
                                                            uint8_t* __restrict__ compact) {
    const Tile t = tiles[blockIdx.x];
    uint32_t letter[kRounds];
    uint32_t fm = 0;                                        // bit r: the letter of round r is kept
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int k = r * kThreads + (int)threadIdx.x;
        letter[r] = k < t.n ? (uint32_t)aligned[t.out + k] : (uint32_t)'-';
        fm |= (uint32_t)(letter[r] != (uint32_t)'-') << r;
    }
    int32_t rank[kRounds];                                  // positions ascend with (round, wave, lane)
    mc::tile_offsets<kWaves>(fm, rank);
    const int64_t first = base[blockIdx.x];
#pragma unroll
    for (int r = 0; r < kRounds; ++r)
        if ((fm >> r) & 1) compact[first + rank[r]] = (uint8_t)letter[r];
}

#include "bases_ins.h"   // the insertion stage's kernels
#include "bases_div.h"   // the diversity stage's kernels
#include "bases_cmp.h"   // the comparison stage's tile kernel

constexpr size_t kArenaPad = 64;   // bytes behind every uploaded array

// grow-only device array, kArenaPad bytes of room behind the n elements asked for
template <typename T>
using Buf = mc::Buf<T, kArenaPad>;

// a grouped allele table in device memory (rows sorted by (i, other, len, code))
struct InsTable {
    Buf<int64_t> i;
    Buf<int32_t> len;
    Buf<uint64_t> code;
    Buf<uint8_t> other;
    Buf<uint32_t> cnt;
    Buf<int32_t> rowcount;               // [T]
    Buf<int64_t> rowbase, first;         // [T + 1], [S + 1]
    int64_t n = 0;
    bool valid = false;
};

// The handle's timing events: a span of a *_timing call lies between two of
// them (the consensus' call ends where its scan begins, the diversity's and
// the comparison's zero pass where its tile pass begins); kEvCmpWait is
// recorded on the other handle's stream, for this one to wait on.
enum {
    kEvPrepass, kEvPrepassEnd, kEvPileup, kEvPileupEnd, kEvSites, kEvSitesEnd,
    kEvConsCall, kEvConsScan, kEvConsScanEnd, kEvConsEmit, kEvConsEmitEnd,
    kEvDivZero, kEvDivTile, kEvDivEnd,
    kEvCmpWait, kEvCmpZero, kEvCmpTile, kEvCmpEnd,
    kEvInsExtract, kEvInsExtractEnd, kEvInsGroup, kEvInsGroupEnd, kEvInsCons, kEvInsConsEnd,
    kEvents
};

// The per-window rows of one stage (mc_bases_diversity, mc_bases_compare) and what tells the two apart: the pin
// slot of the bad word, the three timing events, the names in the state error and the tail of the range error.
struct WindowRows {
    int slot, ev_zero, ev_tile, ev_end;
    const char *noun, *call, *bad_what;
    bool have = false;
    int64_t n = 0;                       // windows in all
    std::vector<int64_t> first;          // [S + 1]
    Buf<DivTile> tiles;                  // [T]
    Buf<int64_t> rows;                   // [n][8]
    Buf<unsigned long long> bad;         // the lowest plane index with 2^26 bases or more (pin[slot] on the host)
    float ms_tile = 0, ms_zero = 0;
    void drop() {
        have = false;
        ms_tile = ms_zero = 0;
    }
};

#define MC_REQUIRE_ROWS(r) MC_REQUIRE((r).have, MC_E_STATE, "no %s computed (call %s)", (r).noun, (r).call)

}  // namespace

// pin: [0] lowest bad read, [1] max span (int32), [2] site total, [3] consensus total, [4] insertion totals,
// [7] the diversity's bad index, [8] the comparison's
struct mc_bases : mc::StageHandle<kEvents, 9> {
    int32_t n_ref = 0;
    // segments and planes (mc_bases_begin)
    bool begun = false;
    int32_t min_baseq = 0;
    int64_t S = 0, N = 0, stride = 4, n_tiles = 0;
    std::vector<int64_t> seg_off;
    std::vector<int32_t> seg_tid;        // the segments as begun, on the host (mc_bases_compare's check)
    std::vector<int64_t> seg_start, seg_end;
    std::vector<int64_t> tile_out;       // the tiles' first plane indices, on the host (diversity, mc_bases_ins_set)
    Buf<Tile> tiles;
    Buf<int32_t> order;                  // the tiles sorted by (tid, rel)
    std::vector<std::pair<int32_t, int64_t>> tile_key;   // (tid, rel) of order[i], on the host
    Buf<int64_t> seg_tile;
    Buf<uint32_t> planes;
    // the batch in flight
    Buf<int32_t> tid, pos, l_seq, span;
    Buf<int64_t> cig_off, seq_off, qual_off;
    Buf<uint32_t> cigar;
    Buf<uint8_t> seq, qual;
    Buf<unsigned long long> flags;       // [0] lowest bad read, [1] max span
    bool have_last = false;
    int32_t last_tid = 0, last_pos = 0;
    int64_t n_reads = 0;
    Buf<uint8_t> ref;                    // the reference plane of the call in flight (upload_ref)
    // sites
    bool have_sites = false;
    int64_t n_sites = 0;
    Buf<int32_t> counts;
    Buf<int64_t> base, site_first, site_pos;
    Buf<uint32_t> site_counts;
    float ms_prepass = 0, ms_pileup = 0, ms_sites = 0;
    // consensus: buffers of its own, so sites and a consensus live side by side
    bool have_cons = false;
    int64_t n_cons = 0;                  // compact letters in all
    Buf<uint8_t> cons_aligned, cons_compact;
    Buf<int32_t> cons_cols;              // [8][T]
    Buf<int64_t> cons_pre, cons_first, cons_rows;   // [8][T + 1], [S + 1], [S][8]
    float ms_cons_call = 0, ms_cons_scan = 0, ms_cons_emit = 0;
    // diversity, and the comparison with another handle: buffers of their own again, so their rows live beside
    // sites and a consensus and beside each other
    WindowRows div{7, kEvDivZero, kEvDivTile, kEvDivEnd, "diversity", "mc_bases_diversity",
                   "a covered position is 2^26 or more (pi_fix is exact below that)"};
    WindowRows cmp{8, kEvCmpZero, kEvCmpTile, kEvCmpEnd, "comparison", "mc_bases_compare",
                   "a compared position is 2^26 or more in one of the samples (dist_fix is exact below that)"};
    // insertions (opt-in, mc_bases_track_insertions): events, their sorted buckets, two row tables
    bool track_next = false, tracking = false;
    bool ins_from_set = false;           // mc_bases_ins_set installed the sorted buckets
    int64_t n_events = 0;
    InsEvent* events = nullptr;          // grows with its contents kept
    size_t events_cap = 0;
    Buf<int32_t> ins_counts, tile_total, ins_cursor;
    Buf<int64_t> ins_base, ins_bbase;
    bool sorted_valid = false, have_weight = false;
    Buf<InsEvent> ins_sorted;
    Buf<uint32_t> ins_weight;
    InsTable tab_user, tab_cons;
    Buf<uint8_t> cons_called;
    Buf<int32_t> cons_ins_cols;          // [2][T]: bases inserted, insertions called
    Buf<int64_t> cons_ins_pre, cons_ins_first, cons_ins_rows;   // [2][T + 1], [2][S + 1], [S][2]
    bool have_cons_ins = false;
    float ms_ins_extract = 0, ms_ins_group = 0, ms_ins_cons = 0;
    // strand (opt-in, mc_bases_track_strand): the reverse-strand reads' planes beside the totals
    bool strand_next = false, strand = false;
    Buf<uint32_t> rev;                   // [6][stride], indexed like planes
    Buf<uint16_t> rflag;                 // the flags of the host batch in flight
    bool have_sites_rev = false;         // the sites are mc_bases_sites_strand's: site_rev is filled
    Buf<uint32_t> site_rev;
    // quality (opt-in, mc_bases_track_quality): the sums of the counted bases' quality bytes and of their reads' MAPQ
    bool quality_next = false, quality = false;
    Buf<uint32_t> bq, mq;                // [6][stride] each, indexed like planes
    Buf<uint8_t> rmapq;                  // the mapq column of the host batch in flight
    bool have_sites_q = false;           // the sites are mc_bases_sites_quality's: site_bq and site_mq are filled
    Buf<uint32_t> site_bq, site_mq;
    ~mc_bases() {
        if (events) (void)hipFree(events);
    }
};

namespace {

// [first, first + count) lies inside [0, n]; what: the elements' name for mc_last_error.
int check_range(int64_t first, int64_t count, int64_t n, const char* what) {
    MC_REQUIRE(first >= 0 && count >= 0 && first <= n && count <= n - first, MC_E_INVALID,
               "%s [%lld, %lld + %lld) outside [0, %lld]", what, (long long)first, (long long)first, (long long)count,
               (long long)n);
    return MC_OK;
}

// count elements of each of the six planes, plane c from src + c * src_stride to
// dst + c * dst_stride (the host's side is [6][count]), and the synchronisation.
int copy_planes(const mc_bases* h, uint32_t* dst, int64_t dst_stride, const uint32_t* src, int64_t src_stride,
                int64_t count, hipMemcpyKind kind) {
    for (int c = 0; c < kPlanes; ++c)
        HIP_TRY(hipMemcpyAsync(dst + c * dst_stride, src + c * src_stride, (size_t)count * 4, kind, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MC_OK;
}

// The caller's reference plane (N codes, or null) in device memory for the call in flight: *d_ref, or null.
int upload_ref(mc_bases* h, const uint8_t* ref, const uint8_t** d_ref) {
    *d_ref = nullptr;
    if (!ref || !h->N) return MC_OK;
    HIP_TRY(h->ref.reserve((size_t)h->N));
    HIP_TRY(hipMemcpyAsync(h->ref.p, ref, (size_t)h->N, hipMemcpyHostToDevice, h->stream));
    *d_ref = h->ref.p;
    return MC_OK;
}

// The events or the planes changed: the row tables and the consensus' insertions are stale.
void invalidate_ins(mc_bases* h) {
    h->tab_user.valid = h->tab_cons.valid = false;
    h->have_cons_ins = false;
}

// The planes or the installed insertions changed: the window rows of both stages and their timings are gone.
void drop_window_rows(mc_bases* h) {
    h->div.drop();
    h->cmp.drop();
}

// The planes changed: so are the sites, the consensus and the row tables (their rows were kept by depth).
void invalidate_results(mc_bases* h) {
    h->have_sites = false;
    h->have_cons = false;
    drop_window_rows(h);
    invalidate_ins(h);
}

}  // namespace

extern "C" int mc_bases_create(int device, int32_t n_ref, mc_bases** out) {
    MC_REQUIRE(out, MC_E_INVALID, "null argument");
    *out = nullptr;
    MC_REQUIRE(n_ref >= 0, MC_E_INVALID, "n_ref %d is negative", n_ref);
    if (int rc = mc::stage_create(device, out)) return rc;
    (*out)->n_ref = n_ref;
    if ((*out)->flags.reserve(2) != hipSuccess) {
        delete *out;
        *out = nullptr;
        mc::set_error("HIP stream / event creation failed");
        return MC_E_HIP;
    }
    return MC_OK;
}

extern "C" int mc_bases_destroy(mc_bases* h) { return mc::stage_destroy(h); }

extern "C" int mc_bases_dims(int32_t* tile) {
    MC_REQUIRE(tile, MC_E_INVALID, "null argument");
    *tile = kTile;
    return MC_OK;
}

extern "C" int mc_bases_begin(mc_bases* h, int64_t S, const int32_t* tid, const int64_t* start, const int64_t* end,
                              int32_t min_baseq) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(S >= 0 && (S == 0 || (tid && start && end)), MC_E_INVALID, "bad segment arrays");
    MC_REQUIRE(min_baseq >= 0, MC_E_INVALID, "min_baseq %d is negative", min_baseq);
    MC_REQUIRE(!(h->strand_next && h->quality_next), MC_E_STATE,
               "strand tracking (mc_bases_track_strand) and quality tracking (mc_bases_track_quality) are both on: "
               "one handle keeps one of them");
    h->begun = false;
    h->have_sites = false;
    h->have_cons = false;
    h->have_cons_ins = false;
    drop_window_rows(h);
    h->tracking = false;
    h->strand = false;
    h->have_sites_rev = false;
    h->quality = false;
    h->have_sites_q = false;

    // ---- tile table (host): a tile never spans two segments
    std::vector<Tile> tiles;
    std::vector<int64_t> seg_tile((size_t)S + 1), seg_off((size_t)S + 1);
    int64_t N = 0;
    for (int64_t s = 0; s < S; ++s) {
        if (tid[s] < 0 || tid[s] >= h->n_ref) return mc::bad_segment_tid(s, tid[s]);
        if (int rc = mc::check_segment_range(s, start, end)) return rc;
        seg_tile[s] = (int64_t)tiles.size();
        seg_off[s] = N;
        const int rc = mc::cut_tiles(
            tiles, kTile, start[s], end[s], 1, [&](int64_t) { return (int)(N & 3); },
            [&](int64_t a, int64_t n) {
                Tile t;
                t.out = N;
                t.rel = a;
                t.lead = (int32_t)(N & 3);
                t.n = (int32_t)n;
                t.tid = tid[s];
                t.seg = (int32_t)std::min<int64_t>(s, INT32_MAX);
                N += n;
                return t;
            });
        if (rc) return rc;
    }
    const int64_t T = (int64_t)tiles.size();
    seg_off[S] = N;
    mc::close_seg_tile(seg_tile, T, start, end);
    const int64_t stride = std::max<int64_t>(4, (N + 3) & ~int64_t(3));   // every plane 16-byte aligned
    // the tiles in (tid, rel) order: a batch launches only the range of them its reads can reach
    std::vector<int32_t> order((size_t)T);
    for (int64_t i = 0; i < T; ++i) order[(size_t)i] = (int32_t)i;
    std::sort(order.begin(), order.end(), [&tiles](int32_t a, int32_t b) {
        return tiles[a].tid != tiles[b].tid ? tiles[a].tid < tiles[b].tid : tiles[a].rel < tiles[b].rel;
    });
    std::vector<std::pair<int32_t, int64_t>> tile_key((size_t)T);
    for (int64_t i = 0; i < T; ++i) tile_key[(size_t)i] = {tiles[order[(size_t)i]].tid, tiles[order[(size_t)i]].rel};

    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->tiles.reserve((size_t)T));
    HIP_TRY(h->order.reserve((size_t)T));
    HIP_TRY(h->seg_tile.reserve((size_t)S + 1));
    HIP_TRY(h->planes.reserve((size_t)(kPlanes * stride)));
    hipStream_t st = h->stream;
    if (T) HIP_TRY(hipMemcpyAsync(h->tiles.p, tiles.data(), (size_t)T * sizeof(Tile), hipMemcpyHostToDevice, st));
    if (T) HIP_TRY(hipMemcpyAsync(h->order.p, order.data(), (size_t)T * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->seg_tile.p, seg_tile.data(), ((size_t)S + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(h->planes.p, 0, (size_t)(kPlanes * stride) * sizeof(uint32_t), st));
    if (h->strand_next) {
        HIP_TRY(h->rev.reserve((size_t)(kPlanes * stride)));
        HIP_TRY(hipMemsetAsync(h->rev.p, 0, (size_t)(kPlanes * stride) * sizeof(uint32_t), st));
    }
    if (h->quality_next) {
        HIP_TRY(h->bq.reserve((size_t)(kPlanes * stride)));
        HIP_TRY(h->mq.reserve((size_t)(kPlanes * stride)));
        HIP_TRY(hipMemsetAsync(h->bq.p, 0, (size_t)(kPlanes * stride) * sizeof(uint32_t), st));
        HIP_TRY(hipMemsetAsync(h->mq.p, 0, (size_t)(kPlanes * stride) * sizeof(uint32_t), st));
    }
    if (h->track_next) {                          // the events of an earlier begin are gone
        HIP_TRY(h->tile_total.reserve((size_t)T));
        if (T) HIP_TRY(hipMemsetAsync(h->tile_total.p, 0, (size_t)T * 4, st));
    }
    HIP_TRY(hipStreamSynchronize(st));            // the host vectors are released
    h->tracking = h->track_next;
    h->strand = h->strand_next;
    h->quality = h->quality_next;
    h->n_events = 0;
    h->ins_from_set = false;
    h->sorted_valid = h->have_weight = false;
    h->tab_user.valid = h->tab_cons.valid = false;
    h->ms_ins_extract = h->ms_ins_group = h->ms_ins_cons = 0;
    h->tile_out.resize((size_t)T);
    for (int64_t i = 0; i < T; ++i) h->tile_out[(size_t)i] = tiles[(size_t)i].out;
    h->S = S;
    h->N = N;
    h->stride = stride;
    h->n_tiles = T;
    h->seg_off = std::move(seg_off);
    h->seg_tid.assign(tid, tid + S);
    h->seg_start.assign(start, start + S);
    h->seg_end.assign(end, end + S);
    h->tile_key = std::move(tile_key);
    h->min_baseq = min_baseq;
    h->have_last = false;
    h->n_reads = 0;
    h->ms_prepass = h->ms_pileup = h->ms_sites = 0;
    h->ms_cons_call = h->ms_cons_scan = h->ms_cons_emit = 0;
    h->begun = true;
    return MC_OK;
}

namespace {

// Why read i of the batch is invalid, for mc_last_error (the pre-pass found i).
// label (>= 0): the read's index in the caller's batch, where the arrays are
// an excerpt of it (mc_bases_add_batch_device copies back two reads).
void name_bad_read(const mc_bases* h, int64_t i, const int32_t* tid, const int32_t* pos, const int64_t* cig_off,
                   const uint32_t* cigar, const int32_t* l_seq, const int64_t* seq_off, const int64_t* qual_off,
                   int64_t n_words, int64_t seq_bytes, int64_t qual_bytes, int64_t label = -1) {
    const long long r = (long long)(label >= 0 ? label : i);
    if (tid[i] < 0 || tid[i] >= h->n_ref) return mc::set_error("read %lld: tid %d out of range", r, tid[i]);
    if (pos[i] < 0) return mc::set_error("read %lld: negative pos %d", r, pos[i]);
    if (l_seq[i] < 0) return mc::set_error("read %lld: negative l_seq %d", r, l_seq[i]);
    if (cig_off[i] < 0 || cig_off[i + 1] < cig_off[i] || cig_off[i + 1] > n_words)
        return mc::set_error("read %lld: CIGAR offsets outside the batch", r);
    if (seq_off[i] < 0 || seq_off[i] + ((int64_t)l_seq[i] + 1) / 2 > seq_bytes || qual_off[i] < 0 ||
        qual_off[i] + l_seq[i] > qual_bytes)
        return mc::set_error("read %lld: bases or qualities outside the batch", r);
    if (i > 0 && (tid[i - 1] > tid[i] || (tid[i - 1] == tid[i] && pos[i - 1] > pos[i])))
        return mc::set_error("read %lld: reads are not sorted by (tid, pos)", r);
    int64_t q = 0, ref = 0;
    for (int64_t k = cig_off[i]; k < cig_off[i + 1]; ++k) {
        const uint32_t op = cigar[k] & 15u;
        if ((kQueryOps >> op) & 1u) q += cigar[k] >> 4;
        if ((kRefOps >> op) & 1u) ref += cigar[k] >> 4;
    }
    if (q != l_seq[i])
        return mc::set_error("read %lld: CIGAR query length %lld differs from l_seq %d", r, (long long)q, l_seq[i]);
    mc::set_error("read %lld: reference span %lld exceeds 2^31 - 1", r, (long long)ref);
}

constexpr int64_t kMaxEvents = INT32_MAX;   // per begin: every count and prefix of the stage fits 31 bits

// The events table with room for `need` events, the first n_events kept.
int ins_reserve_events(mc_bases* h, size_t need) {
    if (need <= h->events_cap) return MC_OK;
    const size_t want = std::max({need, h->events_cap * 2, (size_t)4096});
    InsEvent* p = nullptr;
    HIP_TRY(hipMalloc(&p, want * sizeof(InsEvent) + kArenaPad));
    if (h->events && h->n_events) {
        const hipError_t e = hipMemcpyAsync(p, h->events, (size_t)h->n_events * sizeof(InsEvent),
                                            hipMemcpyDeviceToDevice, h->stream);
        if (e != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) {
            (void)hipFree(p);
            mc::set_error("copying the insertion events failed");
            return MC_E_HIP;
        }
    }
    if (h->events) (void)hipFree(h->events);
    h->events = p;
    h->events_cap = want;
    return MC_OK;
}

// The insertion events of the batch in flight, behind its pileup launch: the
// same tiles (nt of them from index first of the sorted order).  The batch
// total comes back on the synchronisation that ends the batch anyway; a batch
// with events costs one more for its fill pass.
int ins_extract(mc_bases* h, const Batch& b, int64_t first, int64_t nt, int32_t max_span) {
    hipStream_t st = h->stream;
    invalidate_ins(h);
    HIP_TRY(h->ins_counts.reserve((size_t)nt));
    HIP_TRY(h->ins_base.reserve((size_t)nt + 1));
    if (int rc = h->mark(kEvInsExtract)) return rc;
    hipLaunchKernelGGL(ins_extract_kernel<false>, dim3((unsigned)nt), dim3(kThreads), 0, st, b, h->span.p, h->tiles.p,
                       h->order.p + first, max_span, h->ins_counts.p, (const int64_t*)nullptr, (InsEvent*)nullptr,
                       (int64_t)0, (int32_t*)nullptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, h->ins_counts.p, nt, h->ins_base.p,
                       (const int64_t*)nullptr, (int64_t)-1, (int64_t*)nullptr);
    HIP_TRY(hipGetLastError());
    int64_t total = 0;
    if (int rc = h->read_total(h->ins_base.p + nt, 4, &total)) return rc;
    MC_REQUIRE(total >= 0, MC_E_STATE, "insertion event count %lld out of range", (long long)total);
    MC_REQUIRE(h->n_events + total <= kMaxEvents, MC_E_RANGE, "more than 2^31 - 1 insertion events");
    if (total) {
        const int rc = ins_reserve_events(h, (size_t)(h->n_events + total));
        if (rc != MC_OK) return rc;
        hipLaunchKernelGGL(ins_extract_kernel<true>, dim3((unsigned)nt), dim3(kThreads), 0, st, b, h->span.p,
                           h->tiles.p, h->order.p + first, max_span, h->ins_counts.p, h->ins_base.p,
                           h->events + h->n_events, total, h->tile_total.p);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = h->mark(kEvInsExtractEnd)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    if (int rc = h->elapsed(kEvInsExtract, kEvInsExtractEnd, &ms)) return rc;
    h->ms_ins_extract += ms;
    h->n_events += total;
    h->sorted_valid = false;
    return MC_OK;
}

// The events in per-tile buckets, each sorted by (i, other, len, code); kept
// until the events change.
int ins_sort(mc_bases* h) {
    if (h->sorted_valid) return MC_OK;
    const int64_t T = h->n_tiles, E = h->n_events;
    hipStream_t st = h->stream;
    HIP_TRY(h->ins_bbase.reserve((size_t)T + 1));
    HIP_TRY(h->ins_cursor.reserve((size_t)T));
    HIP_TRY(h->ins_sorted.reserve((size_t)E));
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, h->tile_total.p, T, h->ins_bbase.p,
                       (const int64_t*)nullptr, (int64_t)-1, (int64_t*)nullptr);
    HIP_TRY(hipGetLastError());
    if (E && T) {
        HIP_TRY(hipMemsetAsync(h->ins_cursor.p, 0, (size_t)T * 4, st));
        hipLaunchKernelGGL(ins_scatter_kernel, dim3((unsigned)((E + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                           h->events, E, T, h->ins_bbase.p, h->ins_cursor.p, h->ins_sorted.p);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ins_sort_kernel, dim3((unsigned)T), dim3(kThreads), 0, st, h->ins_sorted.p, h->ins_bbase.p,
                           h->tiles.p);
        HIP_TRY(hipGetLastError());
    }
    h->have_weight = false;
    h->sorted_valid = true;
    return MC_OK;
}

// The rows of the sorted buckets that pass the thresholds, into tab.
int ins_encode(mc_bases* h, const SiteArgs& sa, InsTable& tab) {
    const int64_t T = h->n_tiles, S = h->S;
    hipStream_t st = h->stream;
    tab.valid = false;
    HIP_TRY(tab.rowcount.reserve((size_t)T));
    HIP_TRY(tab.rowbase.reserve((size_t)T + 1));
    HIP_TRY(tab.first.reserve((size_t)S + 1));
    const uint32_t* w = h->have_weight ? h->ins_weight.p : nullptr;
    if (T) {
        hipLaunchKernelGGL(ins_encode_kernel<false>, dim3((unsigned)T), dim3(kThreads), 0, st, h->ins_sorted.p, w,
                           h->ins_bbase.p, h->planes.p, h->stride, sa, tab.rowcount.p, (const int64_t*)nullptr,
                           (int64_t*)nullptr, (int32_t*)nullptr, (uint64_t*)nullptr, (uint8_t*)nullptr,
                           (uint32_t*)nullptr);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, tab.rowcount.p, T, tab.rowbase.p,
                       h->seg_tile.p, S, tab.first.p);
    HIP_TRY(hipGetLastError());
    int64_t total = 0;
    if (int rc = h->read_total(tab.rowbase.p + T, 4, &total)) return rc;
    MC_REQUIRE(total >= 0 && total <= h->n_events, MC_E_STATE, "insertion row count %lld out of range",
               (long long)total);
    HIP_TRY(tab.i.reserve((size_t)total));
    HIP_TRY(tab.len.reserve((size_t)total));
    HIP_TRY(tab.code.reserve((size_t)total));
    HIP_TRY(tab.other.reserve((size_t)total));
    HIP_TRY(tab.cnt.reserve((size_t)total));
    if (T && total) {
        hipLaunchKernelGGL(ins_encode_kernel<true>, dim3((unsigned)T), dim3(kThreads), 0, st, h->ins_sorted.p, w,
                           h->ins_bbase.p, h->planes.p, h->stride, sa, (int32_t*)nullptr, tab.rowbase.p, tab.i.p,
                           tab.len.p, tab.code.p, tab.other.p, tab.cnt.p);
        HIP_TRY(hipGetLastError());
    }
    tab.n = total;
    tab.valid = true;
    return MC_OK;
}

}  // namespace

namespace {

// ends[0..3] = the first and the last read's (tid, pos): the few words of a
// device batch the host needs (tile range, order across batches).
__global__ void bases_ends_kernel(Batch b, int32_t* __restrict__ ends) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        ends[0] = b.tid[0];
        ends[1] = b.pos[0];
        ends[2] = b.tid[b.n - 1];
        ends[3] = b.pos[b.n - 1];
    }
}

// f(std::integral_constant<int, mode>()): the one place where the host picks a mode's kernels.
template <typename F>
void for_mode(int mode, F f) {
    if (mode == kModeQuality)
        f(std::integral_constant<int, kModeQuality>());
    else if (mode == kModeStrand)
        f(std::integral_constant<int, kModeStrand>());
    else
        f(std::integral_constant<int, kModePlain>());
}

PileupMode<kModePlain> pileup_mode(const mc_bases*, const uint16_t*, const uint8_t*,
                                   std::integral_constant<int, kModePlain>) {
    return {};
}
PileupMode<kModeStrand> pileup_mode(const mc_bases* h, const uint16_t* flag, const uint8_t*,
                                    std::integral_constant<int, kModeStrand>) {
    return {flag, h->rev.p};
}
PileupMode<kModeQuality> pileup_mode(const mc_bases* h, const uint16_t*, const uint8_t* mapq,
                                     std::integral_constant<int, kModeQuality>) {
    return {mapq, h->bq.p, h->mq.p};
}

SitesMode<kModePlain> sites_mode(const mc_bases*, uint32_t, uint32_t, std::integral_constant<int, kModePlain>) {
    return {};
}
SitesMode<kModeStrand> sites_mode(const mc_bases* h, uint32_t min_alt, uint32_t,
                                  std::integral_constant<int, kModeStrand>) {
    return {h->rev.p, min_alt, h->site_rev.p};
}
SitesMode<kModeQuality> sites_mode(const mc_bases* h, uint32_t min_bq, uint32_t min_mq,
                                   std::integral_constant<int, kModeQuality>) {
    return {h->bq.p, h->mq.p, min_bq, min_mq, h->site_bq.p, h->site_mq.p};
}

// The pileup launch of a batch over tiles [first, first + nt) of the sorted
// order; flag: the reads' flags in device memory on a handle that tracks
// strand; mapq: their MAPQ bytes there on one that tracks quality.
void launch_pileup(mc_bases* h, const Batch& b, int64_t first, int64_t nt, int32_t max_span, const uint16_t* flag,
                   const uint8_t* mapq) {
    for_mode(h->quality ? kModeQuality : h->strand ? kModeStrand : kModePlain, [&](auto mode) {
        constexpr int kMode = decltype(mode)::value;
        hipLaunchKernelGGL(bases_pileup_kernel<kMode>, dim3((unsigned)(nt * (kMode == kModeQuality ? kQSub : 1))),
                           dim3(kThreads), 0, h->stream, b, h->span.p, h->tiles.p, h->order.p + first, max_span,
                           h->min_baseq, h->planes.p, h->stride, pileup_mode(h, flag, mapq, mode));
    });
}

// The per-read column a batch entry point takes beside the nine arrays: none,
// the flag words (the _flags calls) or the MAPQ bytes (the _mapq calls).
struct Column {
    const uint16_t* flag = nullptr;
    const uint8_t* mapq = nullptr;
    bool flagged = false, with_mapq = false;
};

// What every batch entry point checks before it looks at the reads.  device:
// the device entry points are to be named to a strand or quality handle's
// caller who gave no flags or no mapq; arrays: the nine per-read arrays are
// there.
int check_batch(const mc_bases* h, int64_t n, bool arrays, const Column& col, bool device) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    MC_REQUIRE(!h->ins_from_set, MC_E_STATE, "insertions were installed by mc_bases_ins_set (call mc_bases_begin)");
    MC_REQUIRE(col.flagged || !h->strand, MC_E_STATE, "the handle tracks strand: the reads' flags are needed (%s)",
               device ? "mc_bases_add_batch_device_flags" : "mc_bases_add_batch_flags");
    MC_REQUIRE(col.with_mapq || !h->quality, MC_E_STATE, "the handle tracks quality: the reads' mapq is needed (%s)",
               device ? "mc_bases_add_batch_device_mapq" : "mc_bases_add_batch_mapq");
    MC_REQUIRE(n >= 0, MC_E_INVALID, "negative read count");
    MC_REQUIRE(n == 0 || (arrays && (col.flag || !h->strand) && (col.mapq || !h->quality)), MC_E_INVALID,
               "null read arrays");
    return MC_OK;
}

int check_arenas(int64_t n_words, const uint32_t* cigar, int64_t seq_bytes, const uint8_t* seq, int64_t qual_bytes,
                 const uint8_t* qual) {
    MC_REQUIRE(n_words >= 0 && seq_bytes >= 0 && qual_bytes >= 0, MC_E_INVALID, "negative arena size");
    MC_REQUIRE((n_words == 0 || cigar) && (seq_bytes == 0 || seq) && (qual_bytes == 0 || qual), MC_E_INVALID,
               "null arena");
    return MC_OK;
}

// The batch's first read does not sort before the previous batch's last one (a
// first read the pre-pass will reject is left to it).
int check_order(const mc_bases* h, int32_t tid0, int32_t pos0) {
    if (h->have_last && tid0 >= 0 && pos0 >= 0)
        MC_REQUIRE(h->last_tid < tid0 || (h->last_tid == tid0 && h->last_pos <= pos0), MC_E_INVALID,
                   "read 0: reads are not sorted by (tid, pos) against the previous batch");
    return MC_OK;
}

// A batch from the pre-pass on; b: its arrays in device memory (span has room
// for its reads), flag: its flags there on a handle that tracks strand, mapq:
// its MAPQ bytes there on one that tracks quality.
// host_ends: the first and the last read's (tid, pos) where the host has them,
// else null and bases_ends_kernel fetches them into flags[2..3] (the handle's
// flags buffer has room for 256 words), one copy back with the pre-pass' words.
// The order against the previous batch is checked before the pre-pass' verdict.
// A read the pre-pass rejected: MC_E_INVALID with its index in *bad_read (else
// -1) and the message left to the caller, who knows where the arrays are.
int finish_batch(mc_bases* h, const Batch& b, const int32_t* host_ends, const uint16_t* flag, const uint8_t* mapq,
                 int64_t* bad_read) {
    *bad_read = -1;
    hipStream_t st = h->stream;
    h->pin[0] = kNoBad;
    h->pin[1] = 0;
    HIP_TRY(hipMemcpyAsync(h->flags.p, h->pin, 16, hipMemcpyHostToDevice, st));
    const int64_t groups = (b.n + kThreads - 1) / kThreads;
    MC_REQUIRE(groups < (int64_t)INT32_MAX, MC_E_RANGE, "more than 2^39 reads in one batch");
    if (int rc = h->mark(kEvPrepass)) return rc;
    hipLaunchKernelGGL(bases_prepass_kernel, dim3((unsigned)groups), dim3(kThreads), 0, st, b, h->n_ref, h->span.p,
                       h->flags.p, reinterpret_cast<int32_t*>(h->flags.p + 1));
    HIP_TRY(hipGetLastError());
    if (int rc = h->mark(kEvPrepassEnd)) return rc;
    if (!host_ends) {
        hipLaunchKernelGGL(bases_ends_kernel, dim3(1), dim3(64), 0, st, b, reinterpret_cast<int32_t*>(h->flags.p + 2));
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(h->pin, h->flags.p, host_ends ? 16 : 32, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int32_t ends[4];
    std::memcpy(ends, host_ends ? (const void*)host_ends : (const void*)&h->pin[2], 16);
    if (int rc = check_order(h, ends[0], ends[1])) return rc;
    const unsigned long long bad = h->pin[0];
    if (bad != kNoBad) {
        if (bad < (unsigned long long)b.n)
            *bad_read = (int64_t)bad;
        else
            mc::set_error("read index %llu out of range", bad);
        return MC_E_INVALID;
    }
    int32_t max_span = 0;
    std::memcpy(&max_span, &h->pin[1], 4);
    MC_REQUIRE(max_span >= 0, MC_E_STATE, "maximum span %d out of range", max_span);
    if (int rc = h->mark(kEvPileup)) return rc;
    // A tile the batch can reach starts after (first read's pos - kTile) and before (last read's pos +
    // max span), in (tid, rel) order: only that range of the sorted tiles is launched.
    const auto t_lo = std::lower_bound(h->tile_key.begin(), h->tile_key.end(),
                                       std::make_pair(ends[0], (int64_t)ends[1] - kTile));
    const auto t_hi = std::lower_bound(h->tile_key.begin(), h->tile_key.end(),
                                       std::make_pair(ends[2], (int64_t)ends[3] + max_span));
    if (max_span > 0 && t_lo < t_hi) {
        launch_pileup(h, b, t_lo - h->tile_key.begin(), t_hi - t_lo, max_span, flag, mapq);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = h->mark(kEvPileupEnd)) return rc;
    if (h->tracking && max_span > 0 && t_lo < t_hi) {
        const int rc = ins_extract(h, b, t_lo - h->tile_key.begin(), t_hi - t_lo, max_span);
        if (rc != MC_OK) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));            // the caller's arrays and the handle's batch buffers are free again
    float a = 0, c = 0;
    if (int rc = h->elapsed(kEvPrepass, kEvPrepassEnd, &a)) return rc;
    if (int rc = h->elapsed(kEvPileup, kEvPileupEnd, &c)) return rc;
    h->ms_prepass += a;
    h->ms_pileup += c;
    h->have_last = true;
    h->last_tid = ends[2];
    h->last_pos = ends[3];
    h->n_reads += b.n;
    invalidate_results(h);
    return MC_OK;
}

// mc_bases_add_batch, mc_bases_add_batch_flags and mc_bases_add_batch_mapq (col: what they take).
int add_batch(mc_bases* h, int64_t n, const int32_t* tid, const int32_t* pos, const int64_t* cig_off,
              const uint32_t* cigar, const int32_t* l_seq, const int64_t* seq_off, const uint8_t* seq,
              const int64_t* qual_off, const uint8_t* qual, const Column& col) {
    if (int rc = check_batch(h, n, tid && pos && cig_off && l_seq && seq_off && qual_off, col, false)) return rc;
    if (n == 0) return MC_OK;
    const int64_t n_words = cig_off[n], seq_bytes = seq_off[n], qual_bytes = qual_off[n];
    if (int rc = check_arenas(n_words, cigar, seq_bytes, seq, qual_bytes, qual)) return rc;
    if (int rc = check_order(h, tid[0], pos[0])) return rc;     // (before the upload)
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->tid.reserve((size_t)n));
    HIP_TRY(h->pos.reserve((size_t)n));
    HIP_TRY(h->l_seq.reserve((size_t)n));
    HIP_TRY(h->span.reserve((size_t)n));
    HIP_TRY(h->cig_off.reserve((size_t)n + 1));
    HIP_TRY(h->seq_off.reserve((size_t)n + 1));
    HIP_TRY(h->qual_off.reserve((size_t)n + 1));
    HIP_TRY(h->cigar.reserve((size_t)n_words));
    HIP_TRY(h->seq.reserve((size_t)seq_bytes));
    HIP_TRY(h->qual.reserve((size_t)qual_bytes));
    if (h->strand) HIP_TRY(h->rflag.reserve((size_t)n));
    if (h->quality) HIP_TRY(h->rmapq.reserve((size_t)n));
    hipStream_t st = h->stream;
    const auto up = [st](void* d, const void* s, size_t bytes) {
        return bytes ? hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    HIP_TRY(up(h->tid.p, tid, (size_t)n * 4));
    HIP_TRY(up(h->pos.p, pos, (size_t)n * 4));
    HIP_TRY(up(h->l_seq.p, l_seq, (size_t)n * 4));
    HIP_TRY(up(h->cig_off.p, cig_off, ((size_t)n + 1) * 8));
    HIP_TRY(up(h->seq_off.p, seq_off, ((size_t)n + 1) * 8));
    HIP_TRY(up(h->qual_off.p, qual_off, ((size_t)n + 1) * 8));
    HIP_TRY(up(h->cigar.p, cigar, (size_t)n_words * 4));
    HIP_TRY(up(h->seq.p, seq, (size_t)seq_bytes));
    HIP_TRY(up(h->qual.p, qual, (size_t)qual_bytes));
    if (h->strand) HIP_TRY(up(h->rflag.p, col.flag, (size_t)n * 2));
    if (h->quality) HIP_TRY(up(h->rmapq.p, col.mapq, (size_t)n));
    const Batch b{h->tid.p, h->pos.p, h->l_seq.p, h->cig_off.p, h->cigar.p, h->seq_off.p, h->seq.p,
                  h->qual_off.p, h->qual.p, n, n_words, seq_bytes, qual_bytes};
    const int32_t ends[4] = {tid[0], pos[0], tid[n - 1], pos[n - 1]};
    int64_t bad = -1;
    const int rc = finish_batch(h, b, ends, h->rflag.p, h->rmapq.p, &bad);
    if (bad >= 0)
        name_bad_read(h, bad, tid, pos, cig_off, cigar, l_seq, seq_off, qual_off, n_words, seq_bytes, qual_bytes);
    return rc;
}

}  // namespace

extern "C" int mc_bases_add_batch(mc_bases* h, int64_t n, const int32_t* tid, const int32_t* pos,
                                  const int64_t* cig_off, const uint32_t* cigar, const int32_t* l_seq,
                                  const int64_t* seq_off, const uint8_t* seq, const int64_t* qual_off,
                                  const uint8_t* qual) {
    return add_batch(h, n, tid, pos, cig_off, cigar, l_seq, seq_off, seq, qual_off, qual, Column{});
}

extern "C" int mc_bases_add_batch_flags(mc_bases* h, int64_t n, const int32_t* tid, const int32_t* pos,
                                        const int64_t* cig_off, const uint32_t* cigar, const int32_t* l_seq,
                                        const int64_t* seq_off, const uint8_t* seq, const int64_t* qual_off,
                                        const uint8_t* qual, const uint16_t* flag) {
    return add_batch(h, n, tid, pos, cig_off, cigar, l_seq, seq_off, seq, qual_off, qual,
                     Column{flag, nullptr, true, false});
}

extern "C" int mc_bases_add_batch_mapq(mc_bases* h, int64_t n, const int32_t* tid, const int32_t* pos,
                                       const int64_t* cig_off, const uint32_t* cigar, const int32_t* l_seq,
                                       const int64_t* seq_off, const uint8_t* seq, const int64_t* qual_off,
                                       const uint8_t* qual, const uint8_t* mapq) {
    return add_batch(h, n, tid, pos, cig_off, cigar, l_seq, seq_off, seq, qual_off, qual,
                     Column{nullptr, mapq, false, true});
}

namespace {

// mc_bases_add_batch_device, mc_bases_add_batch_device_flags and mc_bases_add_batch_device_mapq.
int add_batch_device(mc_bases* h, int64_t n, const int32_t* d_tid, const int32_t* d_pos, const int64_t* d_cig_off,
                     const uint32_t* d_cigar, int64_t n_words, const int32_t* d_l_seq, const int64_t* d_seq_off,
                     const uint8_t* d_seq, int64_t seq_bytes, const int64_t* d_qual_off, const uint8_t* d_qual,
                     int64_t qual_bytes, const Column& col) {
    if (int rc = check_batch(h, n, d_tid && d_pos && d_cig_off && d_l_seq && d_seq_off && d_qual_off, col, true))
        return rc;
    if (n == 0) return MC_OK;
    if (int rc = check_arenas(n_words, d_cigar, seq_bytes, d_seq, qual_bytes, d_qual)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->span.reserve((size_t)n));
    const Batch b{d_tid, d_pos, d_l_seq, d_cig_off, d_cigar, d_seq_off, d_seq, d_qual_off, d_qual,
                  n, n_words, seq_bytes, qual_bytes};
    int64_t bad = -1;
    const int rc = finish_batch(h, b, nullptr, col.flag, col.mapq, &bad);
    if (bad < 0) return rc;
    // the bad read's fields behind its predecessor's key (two-entry arrays: name_bad_read's i - 1 and i)
    hipStream_t st = h->stream;
    const int64_t i = bad, j = i > 0 ? 1 : 0;
    int32_t t2[2] = {0, 0}, p2[2] = {0, 0}, l2[2] = {0, 0};
    int64_t c3[3] = {0, 0, 0}, s2[2] = {0, 0}, q2[2] = {0, 0};
    const auto down = [st](void* d, const void* s, size_t bytes) {
        return hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToHost, st);
    };
    HIP_TRY(down(t2, d_tid + i - j, (size_t)(j + 1) * 4));
    HIP_TRY(down(p2, d_pos + i - j, (size_t)(j + 1) * 4));
    HIP_TRY(down(l2 + j, d_l_seq + i, 4));
    HIP_TRY(down(c3 + j, d_cig_off + i, 16));
    HIP_TRY(down(s2 + j, d_seq_off + i, 8));
    HIP_TRY(down(q2 + j, d_qual_off + i, 8));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<uint32_t> words;
    int64_t local_words = n_words;
    if (c3[j] >= 0 && c3[j + 1] >= c3[j] && c3[j + 1] <= n_words) {   // the words, rebased to offset 0
        words.resize((size_t)(c3[j + 1] - c3[j]));
        if (!words.empty()) {
            HIP_TRY(down(words.data(), d_cigar + c3[j], words.size() * 4));
            HIP_TRY(hipStreamSynchronize(st));
        }
        // (the bases' and qualities' offsets stay absolute: name_bad_read only compares them)
        c3[j + 1] -= c3[j];
        c3[j] = 0;
        local_words = c3[j + 1];
    }
    name_bad_read(h, j, t2, p2, c3, words.data(), l2, s2, q2, local_words, seq_bytes, qual_bytes, i);
    return MC_E_INVALID;
}

}  // namespace

extern "C" int mc_bases_add_batch_device(mc_bases* h, int64_t n, const int32_t* d_tid, const int32_t* d_pos,
                                         const int64_t* d_cig_off, const uint32_t* d_cigar, int64_t n_words,
                                         const int32_t* d_l_seq, const int64_t* d_seq_off, const uint8_t* d_seq,
                                         int64_t seq_bytes, const int64_t* d_qual_off, const uint8_t* d_qual,
                                         int64_t qual_bytes) {
    return add_batch_device(h, n, d_tid, d_pos, d_cig_off, d_cigar, n_words, d_l_seq, d_seq_off, d_seq, seq_bytes,
                            d_qual_off, d_qual, qual_bytes, Column{});
}

extern "C" int mc_bases_add_batch_device_flags(mc_bases* h, int64_t n, const int32_t* d_tid, const int32_t* d_pos,
                                               const int64_t* d_cig_off, const uint32_t* d_cigar, int64_t n_words,
                                               const int32_t* d_l_seq, const int64_t* d_seq_off,
                                               const uint8_t* d_seq, int64_t seq_bytes, const int64_t* d_qual_off,
                                               const uint8_t* d_qual, int64_t qual_bytes, const uint16_t* d_flag) {
    return add_batch_device(h, n, d_tid, d_pos, d_cig_off, d_cigar, n_words, d_l_seq, d_seq_off, d_seq, seq_bytes,
                            d_qual_off, d_qual, qual_bytes, Column{d_flag, nullptr, true, false});
}

extern "C" int mc_bases_add_batch_device_mapq(mc_bases* h, int64_t n, const int32_t* d_tid, const int32_t* d_pos,
                                              const int64_t* d_cig_off, const uint32_t* d_cigar, int64_t n_words,
                                              const int32_t* d_l_seq, const int64_t* d_seq_off, const uint8_t* d_seq,
                                              int64_t seq_bytes, const int64_t* d_qual_off, const uint8_t* d_qual,
                                              int64_t qual_bytes, const uint8_t* d_mapq) {
    return add_batch_device(h, n, d_tid, d_pos, d_cig_off, d_cigar, n_words, d_l_seq, d_seq_off, d_seq, seq_bytes,
                            d_qual_off, d_qual, qual_bytes, Column{nullptr, d_mapq, false, true});
}

extern "C" int mc_bases_seg_off(const mc_bases* h, int64_t* seg_off) {
    MC_REQUIRE(h && seg_off, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    std::memcpy(seg_off, h->seg_off.data(), ((size_t)h->S + 1) * 8);
    return MC_OK;
}

extern "C" int mc_bases_get(const mc_bases* h, int64_t first, int64_t count, uint32_t* out) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    if (int rc = check_range(first, count, h->N, "positions")) return rc;
    MC_REQUIRE(count == 0 || out, MC_E_INVALID, "null out");
    if (count == 0) return MC_OK;
    HIP_TRY(hipSetDevice(h->device));
    return copy_planes(h, out, count, h->planes.p + first, h->stride, count, hipMemcpyDeviceToHost);
}

extern "C" int mc_bases_device(const mc_bases* h, const uint32_t** d_planes, int64_t* stride, int64_t* n) {
    MC_REQUIRE(h && d_planes && stride && n, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    *d_planes = h->planes.p;
    *stride = h->stride;
    *n = h->N;
    return MC_OK;
}

namespace {

// mc_bases_sites (mode kModePlain: the plain predicate and kernels; min_alt
// and min_mq unused), mc_bases_sites_strand (kModeStrand, min_alt its
// threshold) and mc_bases_sites_quality (kModeQuality, min_alt the baseq and
// min_mq the mapq threshold) share everything but the count and emit launches.
int sites(mc_bases* h, int64_t min_depth, int64_t min_count, int64_t min_ppm, int mode, int64_t min_alt,
          int64_t min_mq, const uint8_t* ref, int64_t* n_sites) {
    const bool strand = mode == kModeStrand, quality = mode == kModeQuality;
    MC_REQUIRE(min_depth >= 0 && min_count >= 0 && min_ppm >= 0 && min_ppm <= 1000000, MC_E_INVALID,
               "site thresholds out of range (min_depth %lld, min_count %lld, min_ppm %lld of 10^6)",
               (long long)min_depth, (long long)min_count, (long long)min_ppm);
    h->have_sites = false;
    h->have_sites_rev = false;
    h->have_sites_q = false;
    const int64_t T = h->n_tiles, S = h->S;
    const uint32_t k_mq = (uint32_t)min_mq;
    const uint32_t k_alt = (uint32_t)std::min<int64_t>(std::max<int64_t>(min_alt, 0), UINT32_MAX);
    const SiteArgs sa{(unsigned long long)min_depth, (unsigned long long)min_count, (unsigned long long)min_ppm};
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->counts.reserve((size_t)T));
    HIP_TRY(h->base.reserve((size_t)T + 1));
    HIP_TRY(h->site_first.reserve((size_t)S + 1));
    hipStream_t st = h->stream;
    const uint8_t* d_ref = nullptr;
    if (int rc = upload_ref(h, ref, &d_ref)) return rc;
    if (int rc = h->mark(kEvSites)) return rc;
    if (T) {
        for_mode(mode, [&](auto m) {
            hipLaunchKernelGGL(sites_count_kernel<decltype(m)::value>, dim3((unsigned)T), dim3(kThreads), 0, st,
                               h->planes.p, h->stride, d_ref, h->tiles.p, sa, sites_mode(h, k_alt, k_mq, m),
                               h->counts.p);
        });
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, h->counts.p, T, h->base.p,
                       h->seg_tile.p, S, h->site_first.p);
    HIP_TRY(hipGetLastError());
    int64_t total = 0;
    if (int rc = h->read_total(h->base.p + T, 2, &total)) return rc;
    MC_REQUIRE(total >= 0 && total <= h->N, MC_E_STATE, "site count %lld out of range", (long long)total);
    HIP_TRY(h->site_pos.reserve((size_t)total));
    HIP_TRY(h->site_counts.reserve((size_t)total * kPlanes));
    if (strand) HIP_TRY(h->site_rev.reserve((size_t)total * kPlanes));
    if (quality) {
        HIP_TRY(h->site_bq.reserve((size_t)total * kPlanes));
        HIP_TRY(h->site_mq.reserve((size_t)total * kPlanes));
    }
    if (T) {
        for_mode(mode, [&](auto m) {      // (after the reserves: the mode's output pointers are final)
            hipLaunchKernelGGL(sites_emit_kernel<decltype(m)::value>, dim3((unsigned)T), dim3(kThreads), 0, st,
                               h->planes.p, h->stride, d_ref, h->tiles.p, sa, sites_mode(h, k_alt, k_mq, m),
                               h->base.p, h->site_pos.p, h->site_counts.p);
        });
        HIP_TRY(hipGetLastError());
    }
    if (int rc = h->mark(kEvSitesEnd)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    if (int rc = h->elapsed(kEvSites, kEvSitesEnd, &h->ms_sites)) return rc;   // (the 8-byte read-back included)
    h->n_sites = total;
    h->have_sites = true;
    h->have_sites_rev = strand;
    h->have_sites_q = quality;
    *n_sites = total;
    return MC_OK;
}

}  // namespace

extern "C" int mc_bases_sites(mc_bases* h, int64_t min_depth, int64_t min_count, int64_t min_ppm,
                              const uint8_t* ref, int64_t* n_sites) {
    MC_REQUIRE(h && n_sites, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    return sites(h, min_depth, min_count, min_ppm, kModePlain, 0, 0, ref, n_sites);
}

extern "C" int mc_bases_sites_strand(mc_bases* h, int64_t min_depth, int64_t min_count, int64_t min_ppm,
                                     int64_t min_alt_strand, const uint8_t* ref, int64_t* n_sites) {
    MC_REQUIRE(h && n_sites, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    MC_REQUIRE(h->strand, MC_E_STATE, "the handle does not track strand (mc_bases_track_strand before begin)");
    MC_REQUIRE(min_alt_strand >= 0, MC_E_INVALID, "min_alt_strand %lld is negative", (long long)min_alt_strand);
    return sites(h, min_depth, min_count, min_ppm, kModeStrand, min_alt_strand, 0, ref, n_sites);
}

extern "C" int mc_bases_sites_get_reverse(const mc_bases* h, int64_t first, int64_t count, uint32_t* rev_counts) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->have_sites && h->have_sites_rev, MC_E_STATE,
               "no strand sites computed (call mc_bases_sites_strand)");
    if (int rc = check_range(first, count, h->n_sites, "sites")) return rc;
    MC_REQUIRE(count == 0 || rev_counts, MC_E_INVALID, "null out");
    if (count == 0) return MC_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(rev_counts, h->site_rev.p + first * kPlanes, (size_t)count * kPlanes * 4,
                           hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MC_OK;
}

extern "C" int mc_bases_track_strand(mc_bases* h, int on) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(on == 0 || on == 1, MC_E_INVALID, "on must be 0 or 1, not %d", on);
    h->strand_next = on != 0;
    return MC_OK;
}

extern "C" int mc_bases_get_reverse(const mc_bases* h, int64_t first, int64_t count, uint32_t* out) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    MC_REQUIRE(h->strand, MC_E_STATE, "the handle does not track strand (mc_bases_track_strand before begin)");
    if (int rc = check_range(first, count, h->N, "positions")) return rc;
    MC_REQUIRE(count == 0 || out, MC_E_INVALID, "null out");
    if (count == 0) return MC_OK;
    HIP_TRY(hipSetDevice(h->device));
    return copy_planes(h, out, count, h->rev.p + first, h->stride, count, hipMemcpyDeviceToHost);
}

extern "C" int mc_bases_reverse_device(const mc_bases* h, const uint32_t** d_rev, int64_t* stride, int64_t* n) {
    MC_REQUIRE(h && d_rev && stride && n, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    MC_REQUIRE(h->strand, MC_E_STATE, "the handle does not track strand (mc_bases_track_strand before begin)");
    *d_rev = h->rev.p;
    *stride = h->stride;
    *n = h->N;
    return MC_OK;
}

extern "C" int mc_bases_set_strand(mc_bases* h, int64_t first, int64_t count, const uint32_t* total,
                                   const uint32_t* rev) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    MC_REQUIRE(h->strand, MC_E_STATE, "the handle does not track strand (mc_bases_track_strand before begin)");
    if (int rc = check_range(first, count, h->N, "positions")) return rc;
    MC_REQUIRE(count == 0 || (total && rev), MC_E_INVALID, "null in");
    for (int64_t k = 0; k < kPlanes * count; ++k)
        MC_REQUIRE(rev[k] <= total[k], MC_E_INVALID, "channel %lld, position %lld: reverse count %u exceeds total %u",
                   (long long)(k / count), (long long)(first + k % count), rev[k], total[k]);
    const int rc = mc_bases_set(h, first, count, total);
    if (rc != MC_OK || count == 0) return rc;
    return copy_planes(h, h->rev.p + first, h->stride, rev, count, count, hipMemcpyHostToDevice);
}

// ---- quality (the header's "Quality sums") -----------------------------------

#define MC_REQUIRE_QUALITY(h) \
    MC_REQUIRE((h)->quality, MC_E_STATE, "the handle does not track quality (mc_bases_track_quality before begin)")

extern "C" int mc_bases_track_quality(mc_bases* h, int on) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(on == 0 || on == 1, MC_E_INVALID, "on must be 0 or 1, not %d", on);
    h->quality_next = on != 0;
    return MC_OK;
}

extern "C" int mc_bases_get_quality(const mc_bases* h, int64_t first, int64_t count, uint32_t* bq, uint32_t* mq) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    MC_REQUIRE_QUALITY(h);
    if (int rc = check_range(first, count, h->N, "positions")) return rc;
    MC_REQUIRE(count == 0 || (bq && mq), MC_E_INVALID, "null out");
    if (count == 0) return MC_OK;
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = copy_planes(h, bq, count, h->bq.p + first, h->stride, count, hipMemcpyDeviceToHost)) return rc;
    return copy_planes(h, mq, count, h->mq.p + first, h->stride, count, hipMemcpyDeviceToHost);
}

extern "C" int mc_bases_quality_device(const mc_bases* h, const uint32_t** d_bq, const uint32_t** d_mq,
                                       int64_t* stride, int64_t* n) {
    MC_REQUIRE(h && d_bq && d_mq && stride && n, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    MC_REQUIRE_QUALITY(h);
    *d_bq = h->bq.p;
    *d_mq = h->mq.p;
    *stride = h->stride;
    *n = h->N;
    return MC_OK;
}

extern "C" int mc_bases_set_quality(mc_bases* h, int64_t first, int64_t count, const uint32_t* total,
                                    const uint32_t* bq, const uint32_t* mq) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    MC_REQUIRE_QUALITY(h);
    if (int rc = check_range(first, count, h->N, "positions")) return rc;
    MC_REQUIRE(count == 0 || (total && bq && mq), MC_E_INVALID, "null in");
    for (int64_t k = 0; k < kPlanes * count; ++k) {
        const long long c = (long long)(k / count), p = (long long)(first + k % count);
        MC_REQUIRE(bq[k] <= 255ull * total[k], MC_E_INVALID,
                   "channel %lld, position %lld: baseq sum %u exceeds 255 x count %u", c, p, bq[k], total[k]);
        MC_REQUIRE(mq[k] <= 255ull * total[k], MC_E_INVALID,
                   "channel %lld, position %lld: mapq sum %u exceeds 255 x count %u", c, p, mq[k], total[k]);
        MC_REQUIRE(c != MC_BASES_DEL || bq[k] == 0, MC_E_INVALID,
                   "position %lld: baseq sum %u of DEL is not 0", p, bq[k]);
    }
    const int rc = mc_bases_set(h, first, count, total);
    if (rc != MC_OK || count == 0) return rc;
    if (int rc2 = copy_planes(h, h->bq.p + first, h->stride, bq, count, count, hipMemcpyHostToDevice)) return rc2;
    return copy_planes(h, h->mq.p + first, h->stride, mq, count, count, hipMemcpyHostToDevice);
}

extern "C" int mc_bases_sites_quality(mc_bases* h, int64_t min_depth, int64_t min_count, int64_t min_ppm,
                                      int64_t min_alt_baseq, int64_t min_alt_mapq, const uint8_t* ref,
                                      int64_t* n_sites) {
    MC_REQUIRE(h && n_sites, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    MC_REQUIRE_QUALITY(h);
    MC_REQUIRE(min_alt_baseq >= 0 && min_alt_baseq <= 255 && min_alt_mapq >= 0 && min_alt_mapq <= 255, MC_E_INVALID,
               "quality thresholds outside 0..255 (min_alt_baseq %lld, min_alt_mapq %lld)", (long long)min_alt_baseq,
               (long long)min_alt_mapq);
    return sites(h, min_depth, min_count, min_ppm, kModeQuality, min_alt_baseq, min_alt_mapq, ref, n_sites);
}

extern "C" int mc_bases_sites_get_quality(const mc_bases* h, int64_t first, int64_t count, uint32_t* bq,
                                          uint32_t* mq) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->have_sites && h->have_sites_q, MC_E_STATE,
               "no quality sites computed (call mc_bases_sites_quality)");
    if (int rc = check_range(first, count, h->n_sites, "sites")) return rc;
    MC_REQUIRE(count == 0 || (bq && mq), MC_E_INVALID, "null out");
    if (count == 0) return MC_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(bq, h->site_bq.p + first * kPlanes, (size_t)count * kPlanes * 4, hipMemcpyDeviceToHost,
                           h->stream));
    HIP_TRY(hipMemcpyAsync(mq, h->site_mq.p + first * kPlanes, (size_t)count * kPlanes * 4, hipMemcpyDeviceToHost,
                           h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MC_OK;
}

extern "C" int mc_bases_quality_dims(int32_t* tile, int32_t* group) {
    MC_REQUIRE(tile && group, MC_E_INVALID, "null argument");
    *tile = kQTile;
    *group = (int32_t)kQGroup;
    return MC_OK;
}

extern "C" int mc_bases_sites_first(const mc_bases* h, int64_t* site_first) {
    MC_REQUIRE(h && site_first, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->have_sites, MC_E_STATE, "no sites computed (call mc_bases_sites)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(site_first, h->site_first.p, ((size_t)h->S + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MC_OK;
}

extern "C" int mc_bases_sites_get(const mc_bases* h, int64_t first, int64_t count, int64_t* site_pos,
                                  uint32_t* site_counts) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->have_sites, MC_E_STATE, "no sites computed (call mc_bases_sites)");
    if (int rc = check_range(first, count, h->n_sites, "sites")) return rc;
    MC_REQUIRE(count == 0 || (site_pos && site_counts), MC_E_INVALID, "null out");
    if (count == 0) return MC_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(site_pos, h->site_pos.p + first, (size_t)count * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(site_counts, h->site_counts.p + first * kPlanes, (size_t)count * kPlanes * 4,
                           hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MC_OK;
}

extern "C" int mc_bases_timing(const mc_bases* h, float* prepass_ms, float* pileup_ms, float* sites_ms,
                               int64_t* tiles, int64_t* reads) {
    MC_REQUIRE(h && prepass_ms && pileup_ms && sites_ms && tiles && reads, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    *prepass_ms = h->ms_prepass;
    *pileup_ms = h->ms_pileup;
    *sites_ms = h->ms_sites;
    *tiles = h->n_tiles;
    *reads = h->n_reads;
    return MC_OK;
}

extern "C" int mc_bases_set(mc_bases* h, int64_t first, int64_t count, const uint32_t* in) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    if (int rc = check_range(first, count, h->N, "positions")) return rc;
    MC_REQUIRE(count == 0 || in, MC_E_INVALID, "null in");
    invalidate_results(h);
    if (count == 0) return MC_OK;
    HIP_TRY(hipSetDevice(h->device));
    return copy_planes(h, h->planes.p + first, h->stride, in, count, count, hipMemcpyHostToDevice);
}

extern "C" int mc_bases_consensus(mc_bases* h, int64_t min_depth, int64_t min_count, int64_t call_ppm,
                                  uint32_t flags, const uint8_t* ref, int64_t* n_out) {
    MC_REQUIRE(h && n_out, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    MC_REQUIRE(min_depth >= 0 && min_count >= 0 && call_ppm >= 0 && call_ppm <= 1000000, MC_E_INVALID,
               "consensus thresholds out of range (min_depth %lld, min_count %lld, call_ppm %lld of 10^6)",
               (long long)min_depth, (long long)min_count, (long long)call_ppm);
    // (a handle that does not track knows no MC_CONS_INS: the bit is as unknown there as it always was)
    MC_REQUIRE((flags & ~(MC_CONS_IUPAC | MC_CONS_FILL_REF | (h->tracking ? MC_CONS_INS : 0u))) == 0, MC_E_INVALID,
               "unknown consensus flags 0x%x%s", flags,
               (flags & MC_CONS_INS) ? " (MC_CONS_INS needs mc_bases_track_insertions before begin)" : "");
    MC_REQUIRE(!(flags & MC_CONS_FILL_REF) || ref, MC_E_INVALID, "MC_CONS_FILL_REF needs a reference plane");
    const bool with_ins = (flags & MC_CONS_INS) != 0;
    h->have_cons = false;
    h->have_cons_ins = false;
    const int64_t T = h->n_tiles, S = h->S;
    const ConsArgs ca{(unsigned long long)std::max<int64_t>(min_depth, 1),
                      (unsigned long long)std::max<int64_t>(min_count, 1), (unsigned long long)call_ppm, flags};
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->cons_aligned.reserve((size_t)h->N));
    HIP_TRY(h->cons_cols.reserve((size_t)(kConsCols * T)));
    HIP_TRY(h->cons_pre.reserve((size_t)(kConsCols * (T + 1))));
    HIP_TRY(h->cons_first.reserve((size_t)S + 1));
    HIP_TRY(h->cons_rows.reserve((size_t)(S * kConsCols)));
    hipStream_t st = h->stream;
    const uint8_t* d_ref = nullptr;
    if (int rc = upload_ref(h, ref, &d_ref)) return rc;
    if (int rc = h->mark(kEvConsCall)) return rc;
    if (T) {
        hipLaunchKernelGGL(cons_call_kernel, dim3((unsigned)T), dim3(kThreads), 0, st, h->planes.p, h->stride, d_ref,
                           h->tiles.p, T, ca, h->cons_aligned.p, h->cons_cols.p);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = h->mark(kEvConsScan)) return rc;
    hipLaunchKernelGGL(cons_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, h->cons_cols.p, T, h->cons_pre.p,
                       h->seg_tile.p, S, h->cons_first.p, h->cons_rows.p);
    HIP_TRY(hipGetLastError());
    if (int rc = h->mark(kEvConsScanEnd)) return rc;
    int64_t total = 0;
    if (int rc = h->read_total(h->cons_pre.p + 7 * (T + 1) + T, 3, &total)) return rc;
    MC_REQUIRE(total >= 0 && total <= h->N, MC_E_STATE, "consensus length %lld out of range", (long long)total);
    int64_t inserted = 0;
    if (with_ins) {
        // the rows that qualify at a position that is not LOW, the top allele of each position, the two
        // per-tile columns (bases inserted, insertions called) and their prefixes
        if (int rc = h->mark(kEvInsCons)) return rc;
        int rc = ins_sort(h);
        if (rc != MC_OK) return rc;
        rc = ins_encode(h, SiteArgs{ca.min_depth, ca.min_count, ca.call_ppm}, h->tab_cons);
        if (rc != MC_OK) return rc;
        InsTable& tb = h->tab_cons;
        HIP_TRY(h->cons_called.reserve((size_t)tb.n));
        HIP_TRY(h->cons_ins_cols.reserve((size_t)(2 * T)));
        HIP_TRY(h->cons_ins_pre.reserve((size_t)(2 * (T + 1))));
        HIP_TRY(h->cons_ins_first.reserve((size_t)(2 * (S + 1))));
        HIP_TRY(h->cons_ins_rows.reserve((size_t)(2 * S)));
        if (tb.n) HIP_TRY(hipMemsetAsync(h->cons_called.p, 0, (size_t)tb.n, st));
        if (T) {
            hipLaunchKernelGGL(cons_ins_pick_kernel, dim3((unsigned)T), dim3(kThreads), 0, st, tb.rowbase.p, tb.i.p,
                               tb.len.p, tb.other.p, tb.cnt.p, h->cons_called.p, h->cons_ins_cols.p,
                               h->cons_ins_cols.p + T);
            HIP_TRY(hipGetLastError());
        }
        for (int c = 0; c < 2; ++c) {
            hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, h->cons_ins_cols.p + c * T, T,
                               h->cons_ins_pre.p + c * (T + 1), h->seg_tile.p, S, h->cons_ins_first.p + c * (S + 1));
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(cons_ins_fix_kernel, dim3((unsigned)(S / 256 + 1)), dim3(256), 0, st, S,
                           h->cons_ins_first.p, h->cons_ins_first.p + (S + 1), h->cons_first.p, h->cons_rows.p,
                           h->cons_ins_rows.p);
        HIP_TRY(hipGetLastError());
        if (int rc = h->mark(kEvInsConsEnd)) return rc;
        rc = h->read_total(h->cons_ins_pre.p + T, 4, &inserted);
        if (rc != MC_OK) return rc;
        MC_REQUIRE(inserted >= 0 && inserted <= kMaxInsLen * tb.n, MC_E_STATE, "inserted bases %lld out of range",
                   (long long)inserted);
        if (int rc = h->elapsed(kEvInsCons, kEvInsConsEnd, &h->ms_ins_cons)) return rc;
    }
    HIP_TRY(h->cons_compact.reserve((size_t)(total + inserted)));
    if (int rc = h->mark(kEvConsEmit)) return rc;
    if (T) {
        if (with_ins) {
            const InsTable& tb = h->tab_cons;
            hipLaunchKernelGGL(cons_emit_ins_kernel, dim3((unsigned)T), dim3(kThreads), 0, st, h->cons_aligned.p,
                               h->tiles.p, h->cons_pre.p + 7 * (T + 1), h->cons_ins_pre.p, tb.rowbase.p, tb.i.p,
                               tb.len.p, tb.code.p, h->cons_called.p, h->cons_compact.p, total + inserted);
        } else {
            hipLaunchKernelGGL(cons_emit_kernel, dim3((unsigned)T), dim3(kThreads), 0, st, h->cons_aligned.p,
                               h->tiles.p, h->cons_pre.p + 7 * (T + 1), h->cons_compact.p);
        }
        HIP_TRY(hipGetLastError());
    }
    if (int rc = h->mark(kEvConsEmitEnd)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    if (int rc = h->elapsed(kEvConsCall, kEvConsScan, &h->ms_cons_call)) return rc;
    if (int rc = h->elapsed(kEvConsScan, kEvConsScanEnd, &h->ms_cons_scan)) return rc;
    if (int rc = h->elapsed(kEvConsEmit, kEvConsEmitEnd, &h->ms_cons_emit)) return rc;
    h->n_cons = total + inserted;
    h->have_cons = true;
    h->have_cons_ins = with_ins;
    *n_out = h->n_cons;
    return MC_OK;
}

extern "C" int mc_bases_consensus_first(const mc_bases* h, int64_t* out_first) {
    MC_REQUIRE(h && out_first, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->have_cons, MC_E_STATE, "no consensus computed (call mc_bases_consensus)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(out_first, h->cons_first.p, ((size_t)h->S + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MC_OK;
}

extern "C" int mc_bases_consensus_summary(const mc_bases* h, int64_t* rows) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->have_cons, MC_E_STATE, "no consensus computed (call mc_bases_consensus)");
    MC_REQUIRE(h->S == 0 || rows, MC_E_INVALID, "null rows");
    if (h->S == 0) return MC_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(rows, h->cons_rows.p, (size_t)h->S * kConsCols * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MC_OK;
}

extern "C" int mc_bases_consensus_get(const mc_bases* h, int compact, int64_t first, int64_t count,
                                      uint8_t* letters) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->have_cons, MC_E_STATE, "no consensus computed (call mc_bases_consensus)");
    const int64_t n = compact ? h->n_cons : h->N;
    if (int rc = check_range(first, count, n, compact ? "compact letters" : "aligned letters")) return rc;
    MC_REQUIRE(count == 0 || letters, MC_E_INVALID, "null out");
    if (count == 0) return MC_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(letters, (compact ? h->cons_compact.p : h->cons_aligned.p) + first, (size_t)count,
                           hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MC_OK;
}

extern "C" int mc_bases_consensus_device(const mc_bases* h, const uint8_t** d_aligned, const uint8_t** d_compact) {
    MC_REQUIRE(h && d_aligned && d_compact, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->have_cons, MC_E_STATE, "no consensus computed (call mc_bases_consensus)");
    *d_aligned = h->cons_aligned.p;
    *d_compact = h->cons_compact.p;
    return MC_OK;
}

extern "C" int mc_bases_consensus_timing(const mc_bases* h, float* call_ms, float* scan_ms, float* emit_ms) {
    MC_REQUIRE(h && call_ms && scan_ms && emit_ms, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    *call_ms = h->ms_cons_call;
    *scan_ms = h->ms_cons_scan;
    *emit_ms = h->ms_cons_emit;
    return MC_OK;
}

// ---- diversity (the contract is the header's, "Diversity") --------------------

namespace {

// The windows of `window` positions over h's segments (arithmetic: first[S + 1], *n_windows) and, per tile of
// mc_bases_begin's cut, its first window and where in it the tile starts: tile_out against seg_off is the
// tile's offset inside its segment.  For mc_bases_diversity and mc_bases_compare.
int div_windows(const mc_bases* h, int64_t window, std::vector<int64_t>& first, std::vector<DivTile>& dt,
                int64_t* n_windows) {
    const int64_t T = h->n_tiles, S = h->S;
    first.assign((size_t)S + 1, 0);
    int64_t nw = 0;
    for (int64_t s = 0; s < S; ++s) {
        first[(size_t)s] = nw;
        const int64_t len = h->seg_off[(size_t)s + 1] - h->seg_off[(size_t)s];
        nw += window ? (len + window - 1) / window : (len > 0);
        MC_REQUIRE(nw <= (int64_t(1) << 31), MC_E_RANGE, "more than 2^31 windows of %lld positions",
                   (long long)window);
    }
    first[(size_t)S] = nw;
    dt.resize((size_t)T);
    for (int64_t i = 0, s = 0; i < T; ++i) {
        const int64_t out = h->tile_out[(size_t)i];
        while (h->seg_off[(size_t)s + 1] <= out) ++s;       // tiles and segments ascend together; out < N
        const int64_t p = out - h->seg_off[(size_t)s];
        dt[(size_t)i] = window ? DivTile{first[(size_t)s] + p / window, p % window} : DivTile{first[(size_t)s], p};
    }
    *n_windows = nw;
    return MC_OK;
}

// The thresholds and the window as the tile kernels take them.
DivArgs div_args(int64_t window, int64_t min_depth, int64_t min_count, int64_t min_ppm) {
    return DivArgs{(unsigned long long)std::max<int64_t>(min_depth, 2),
                   (unsigned long long)std::max<int64_t>(min_count, 1), (unsigned long long)min_ppm,
                   window ? window : 2 * kMaxPos};
}

// One window-row result from h's planes, on h's stream: the windows, the bad word seeded, the DivTiles uploaded,
// the rows tiles share zeroed, then the stage's tile kernel (`launch(stream)`, called only with tiles to run:
// the one step that differs), the bad word back, the two times.  cols: the stage's columns per row.  The caller
// has made h's device current and put what its kernel reads besides h's planes in front on the stream.
template <typename Launch>
int window_rows(mc_bases* h, WindowRows& r, int64_t window, const DivArgs& da, int cols, int64_t* n_windows,
                Launch launch) {
    r.have = false;
    const int64_t T = h->n_tiles;
    std::vector<int64_t> first;
    std::vector<DivTile> dt;
    int64_t nw = 0;
    if (int rc = div_windows(h, window, first, dt, &nw)) return rc;
    HIP_TRY(r.tiles.reserve((size_t)T));
    HIP_TRY(r.rows.reserve((size_t)(nw * cols)));
    HIP_TRY(r.bad.reserve(1));
    hipStream_t st = h->stream;
    h->pin[r.slot] = kNoBad;
    HIP_TRY(hipMemcpyAsync(r.bad.p, h->pin + r.slot, 8, hipMemcpyHostToDevice, st));
    if (T) HIP_TRY(hipMemcpyAsync(r.tiles.p, dt.data(), (size_t)T * sizeof(DivTile), hipMemcpyHostToDevice, st));
    if (int rc = h->mark(r.ev_zero)) return rc;
    if (T) {
        hipLaunchKernelGGL(div_zero_kernel, dim3((unsigned)((T * 16 + 255) / 256)), dim3(256), 0, st, h->tiles.p,
                           r.tiles.p, T, da.window, r.rows.p);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = h->mark(r.ev_tile)) return rc;
    if (T) {
        launch(st);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = h->mark(r.ev_end)) return rc;
    HIP_TRY(hipMemcpyAsync(h->pin + r.slot, r.bad.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));            // (dt is released)
    const unsigned long long bad = h->pin[r.slot];
    MC_REQUIRE(bad == kNoBad, MC_E_RANGE, "plane index %llu: A + C + G + T of %s", bad, r.bad_what);
    if (int rc = h->elapsed(r.ev_zero, r.ev_tile, &r.ms_zero)) return rc;
    if (int rc = h->elapsed(r.ev_tile, r.ev_end, &r.ms_tile)) return rc;
    r.first = std::move(first);
    r.n = nw;
    r.have = true;
    *n_windows = nw;
    return MC_OK;
}

// The four accessors of a window-row result (mc_bases_diversity_* and mc_bases_compare_*), behind the callers'
// null checks.
int rows_first(const WindowRows& r, int64_t* win_first) {
    MC_REQUIRE_ROWS(r);
    std::memcpy(win_first, r.first.data(), r.first.size() * 8);
    return MC_OK;
}

int rows_get(const mc_bases* h, const WindowRows& r, int cols, int64_t first, int64_t count, int64_t* rows) {
    MC_REQUIRE_ROWS(r);
    if (int rc = check_range(first, count, r.n, "windows")) return rc;
    MC_REQUIRE(count == 0 || rows, MC_E_INVALID, "null out");
    if (count == 0) return MC_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(rows, r.rows.p + first * cols, (size_t)count * cols * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MC_OK;
}

int rows_device(const WindowRows& r, const int64_t** d_rows, int64_t* n_windows) {
    MC_REQUIRE_ROWS(r);
    *d_rows = r.rows.p;
    *n_windows = r.n;
    return MC_OK;
}

int rows_timing(const WindowRows& r, float* tile_ms, float* zero_ms) {
    MC_REQUIRE_ROWS(r);
    *tile_ms = r.ms_tile;
    *zero_ms = r.ms_zero;
    return MC_OK;
}

}  // namespace

extern "C" int mc_bases_diversity(mc_bases* h, int64_t window, int64_t min_depth, int64_t min_count, int64_t min_ppm,
                                  const uint8_t* ref, int64_t* n_windows) {
    MC_REQUIRE(h && n_windows, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    MC_REQUIRE(min_depth >= 0 && min_count >= 0 && min_ppm >= 0 && min_ppm <= 1000000, MC_E_INVALID,
               "diversity thresholds out of range (min_depth %lld, min_count %lld, min_ppm %lld of 10^6)",
               (long long)min_depth, (long long)min_count, (long long)min_ppm);
    MC_REQUIRE(window == 0 || window >= MC_DIV_MIN_WINDOW, MC_E_INVALID, "window %lld: must be 0 or at least %d",
               (long long)window, MC_DIV_MIN_WINDOW);
    h->div.have = false;
    HIP_TRY(hipSetDevice(h->device));
    const uint8_t* d_ref = nullptr;
    if (int rc = upload_ref(h, ref, &d_ref)) return rc;
    const DivArgs da = div_args(window, min_depth, min_count, min_ppm);
    return window_rows(h, h->div, window, da, kDivCols, n_windows, [&](hipStream_t st) {
        hipLaunchKernelGGL(div_tile_kernel, dim3((unsigned)h->n_tiles), dim3(kThreads), 0, st, h->planes.p, h->stride,
                           d_ref, h->tiles.p, h->div.tiles.p, da, h->div.rows.p, h->div.bad.p);
    });
}

extern "C" int mc_bases_diversity_first(const mc_bases* h, int64_t* win_first) {
    MC_REQUIRE(h && win_first, MC_E_INVALID, "null argument");
    return rows_first(h->div, win_first);
}

extern "C" int mc_bases_diversity_get(const mc_bases* h, int64_t first, int64_t count, int64_t* rows) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    return rows_get(h, h->div, kDivCols, first, count, rows);
}

extern "C" int mc_bases_diversity_device(const mc_bases* h, const int64_t** d_rows, int64_t* n_windows) {
    MC_REQUIRE(h && d_rows && n_windows, MC_E_INVALID, "null argument");
    return rows_device(h->div, d_rows, n_windows);
}

extern "C" int mc_bases_diversity_timing(const mc_bases* h, float* tile_ms, float* combine_ms) {
    MC_REQUIRE(h && tile_ms && combine_ms, MC_E_INVALID, "null argument");
    return rows_timing(h->div, tile_ms, combine_ms);
}

// ---- comparison (the contract is the header's, "Comparison") ------------------

extern "C" int mc_bases_compare(mc_bases* a, const mc_bases* b, int64_t window, int64_t min_depth, int64_t min_count,
                                int64_t min_ppm, int64_t* n_windows) {
    MC_REQUIRE(a && b && n_windows, MC_E_INVALID, "null argument");
    MC_REQUIRE(a->begun && b->begun, MC_E_STATE, "no segments on %s (call mc_bases_begin)",
               a->begun ? "the second handle" : "the first handle");
    MC_REQUIRE(a->device == b->device, MC_E_INVALID, "the handles are on devices %d and %d", a->device, b->device);
    MC_REQUIRE(a->S == b->S, MC_E_INVALID, "segment %lld: the handles have %lld and %lld segments",
               (long long)std::min(a->S, b->S), (long long)a->S, (long long)b->S);
    for (int64_t s = 0; s < a->S; ++s) {
        const size_t k = (size_t)s;
        MC_REQUIRE(a->seg_tid[k] == b->seg_tid[k] && a->seg_start[k] == b->seg_start[k] &&
                       a->seg_end[k] == b->seg_end[k],
                   MC_E_INVALID, "segment %lld differs: tid %d [%lld, %lld) against tid %d [%lld, %lld)", (long long)s,
                   a->seg_tid[k], (long long)a->seg_start[k], (long long)a->seg_end[k], b->seg_tid[k],
                   (long long)b->seg_start[k], (long long)b->seg_end[k]);
    }
    MC_REQUIRE(min_depth >= 0 && min_count >= 0 && min_ppm >= 0 && min_ppm <= 1000000, MC_E_INVALID,
               "comparison thresholds out of range (min_depth %lld, min_count %lld, min_ppm %lld of 10^6)",
               (long long)min_depth, (long long)min_count, (long long)min_ppm);
    MC_REQUIRE(window == 0 || window >= MC_DIV_MIN_WINDOW, MC_E_INVALID, "window %lld: must be 0 or at least %d",
               (long long)window, MC_DIV_MIN_WINDOW);
    a->cmp.have = false;
    HIP_TRY(hipSetDevice(a->device));
    if (a != b) {                                 // b's planes may still be in flight on its stream
        HIP_TRY(hipEventRecord(a->ev[kEvCmpWait], b->stream));
        HIP_TRY(hipStreamWaitEvent(a->stream, a->ev[kEvCmpWait], 0));
    }
    const DivArgs da = div_args(window, min_depth, min_count, min_ppm);
    return window_rows(a, a->cmp, window, da, kCmpCols, n_windows, [&](hipStream_t st) {
        hipLaunchKernelGGL(cmp_tile_kernel, dim3((unsigned)a->n_tiles), dim3(kThreads), 0, st, a->planes.p, a->stride,
                           b->planes.p, b->stride, a->tiles.p, a->cmp.tiles.p, da, a->cmp.rows.p, a->cmp.bad.p);
    });
}

extern "C" int mc_bases_compare_first(const mc_bases* a, int64_t* win_first) {
    MC_REQUIRE(a && win_first, MC_E_INVALID, "null argument");
    return rows_first(a->cmp, win_first);
}

extern "C" int mc_bases_compare_get(const mc_bases* a, int64_t first, int64_t count, int64_t* rows) {
    MC_REQUIRE(a, MC_E_INVALID, "null argument");
    return rows_get(a, a->cmp, kCmpCols, first, count, rows);
}

extern "C" int mc_bases_compare_device(const mc_bases* a, const int64_t** d_rows, int64_t* n_windows) {
    MC_REQUIRE(a && d_rows && n_windows, MC_E_INVALID, "null argument");
    return rows_device(a->cmp, d_rows, n_windows);
}

extern "C" int mc_bases_compare_timing(const mc_bases* a, float* tile_ms, float* zero_ms) {
    MC_REQUIRE(a && tile_ms && zero_ms, MC_E_INVALID, "null argument");
    return rows_timing(a->cmp, tile_ms, zero_ms);
}

// ---- insertion alleles (the contract is the header's, "Insertion alleles") ----

extern "C" int mc_bases_track_insertions(mc_bases* h, int on) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(on == 0 || on == 1, MC_E_INVALID, "on must be 0 or 1, not %d", on);
    h->track_next = on != 0;
    return MC_OK;
}

extern "C" int mc_bases_insertions(mc_bases* h, int64_t min_depth, int64_t min_count, int64_t min_ppm,
                                   int64_t* n_rows) {
    MC_REQUIRE(h && n_rows, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    MC_REQUIRE(h->tracking, MC_E_STATE, "insertions are not tracked (call mc_bases_track_insertions before begin)");
    MC_REQUIRE(min_depth >= 0 && min_count >= 0 && min_ppm >= 0 && min_ppm <= 1000000, MC_E_INVALID,
               "insertion thresholds out of range (min_depth %lld, min_count %lld, min_ppm %lld of 10^6)",
               (long long)min_depth, (long long)min_count, (long long)min_ppm);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const SiteArgs sa{(unsigned long long)min_depth, (unsigned long long)min_count, (unsigned long long)min_ppm};
    if (int rc = h->mark(kEvInsGroup)) return rc;
    int rc = ins_sort(h);
    if (rc != MC_OK) return rc;
    rc = ins_encode(h, sa, h->tab_user);
    if (rc != MC_OK) return rc;
    if (int rc = h->mark(kEvInsGroupEnd)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    if (int rc = h->elapsed(kEvInsGroup, kEvInsGroupEnd, &h->ms_ins_group)) return rc;   // (the 8-byte read-back included)
    *n_rows = h->tab_user.n;
    return MC_OK;
}

extern "C" int mc_bases_insertions_first(const mc_bases* h, int64_t* first) {
    MC_REQUIRE(h && first, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->tracking && h->tab_user.valid, MC_E_STATE, "no insertions computed (call mc_bases_insertions)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(first, h->tab_user.first.p, ((size_t)h->S + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MC_OK;
}

extern "C" int mc_bases_insertions_get(const mc_bases* h, int64_t first, int64_t count, int64_t* i, int32_t* len,
                                       uint64_t* code, uint8_t* other, uint32_t* cnt) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->tracking && h->tab_user.valid, MC_E_STATE, "no insertions computed (call mc_bases_insertions)");
    const InsTable& t = h->tab_user;
    if (int rc = check_range(first, count, t.n, "rows")) return rc;
    MC_REQUIRE(count == 0 || (i && len && code && other && cnt), MC_E_INVALID, "null out");
    if (count == 0) return MC_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    HIP_TRY(hipMemcpyAsync(i, t.i.p + first, (size_t)count * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(len, t.len.p + first, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(code, t.code.p + first, (size_t)count * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(other, t.other.p + first, (size_t)count, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cnt, t.cnt.p + first, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MC_OK;
}

extern "C" int mc_bases_insertions_timing(const mc_bases* h, float* extract_ms, float* group_ms, float* cons_ms,
                                          int64_t* events) {
    MC_REQUIRE(h && extract_ms && group_ms && cons_ms && events, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    MC_REQUIRE(h->tracking, MC_E_STATE, "insertions are not tracked (call mc_bases_track_insertions before begin)");
    *extract_ms = h->ms_ins_extract;
    *group_ms = h->ms_ins_group;
    *cons_ms = h->ms_ins_cons;
    *events = h->n_events;
    return MC_OK;
}

extern "C" int mc_bases_ins_set(mc_bases* h, int64_t n, const int64_t* i, const int32_t* len, const uint64_t* code,
                                const uint8_t* other, const uint32_t* cnt) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->begun, MC_E_STATE, "no segments (call mc_bases_begin)");
    MC_REQUIRE(h->tracking, MC_E_STATE, "insertions are not tracked (call mc_bases_track_insertions before begin)");
    MC_REQUIRE(n >= 0 && n <= kMaxEvents, MC_E_INVALID, "row count %lld out of range", (long long)n);
    MC_REQUIRE(n == 0 || (i && len && code && other && cnt), MC_E_INVALID, "null row arrays");
    const int64_t T = h->n_tiles;
    std::vector<InsEvent> ev((size_t)n);
    std::vector<int32_t> total((size_t)T, 0);
    for (int64_t r = 0; r < n; ++r) {
        MC_REQUIRE(i[r] >= 0 && i[r] < h->N, MC_E_INVALID, "row %lld: index %lld outside [0, %lld)", (long long)r,
                   (long long)i[r], (long long)h->N);
        MC_REQUIRE(other[r] <= 1, MC_E_INVALID, "row %lld: other is %d", (long long)r, (int)other[r]);
        if (other[r])
            MC_REQUIRE(len[r] == 0 && code[r] == 0, MC_E_INVALID, "row %lld: an OTHER row has len 0 and code 0",
                       (long long)r);
        else
            MC_REQUIRE(len[r] >= 1 && len[r] <= kMaxInsLen && (len[r] == 32 || (code[r] >> (2 * len[r])) == 0),
                       MC_E_INVALID, "row %lld: len %d or code out of range", (long long)r, len[r]);
        MC_REQUIRE(cnt[r] >= 1, MC_E_INVALID, "row %lld: count 0", (long long)r);
        InsEvent e;
        e.i = i[r];
        e.lo = other[r] ? kInsOther : (uint32_t)len[r];
        e.code = code[r];
        const int64_t t = std::upper_bound(h->tile_out.begin(), h->tile_out.end(), i[r]) - h->tile_out.begin() - 1;
        MC_REQUIRE(t >= 0 && t < T, MC_E_STATE, "row %lld: no tile", (long long)r);
        e.tile = (uint32_t)t;
        if (r > 0) {
            const InsEvent& p = ev[(size_t)r - 1];
            MC_REQUIRE(p.i < e.i || (p.i == e.i && (p.lo < e.lo || (p.lo == e.lo && p.code < e.code))), MC_E_INVALID,
                       "row %lld: rows are not sorted by (i, other, len, code) and unique", (long long)r);
        }
        ev[(size_t)r] = e;
        ++total[(size_t)t];
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    h->sorted_valid = false;
    invalidate_ins(h);
    h->have_cons = false;
    drop_window_rows(h);
    HIP_TRY(h->ins_sorted.reserve((size_t)n));
    HIP_TRY(h->ins_weight.reserve((size_t)n));
    HIP_TRY(h->ins_bbase.reserve((size_t)T + 1));
    if (n) {
        HIP_TRY(hipMemcpyAsync(h->ins_sorted.p, ev.data(), (size_t)n * sizeof(InsEvent), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(h->ins_weight.p, cnt, (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    if (T) HIP_TRY(hipMemcpyAsync(h->tile_total.p, total.data(), (size_t)T * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, h->tile_total.p, T, h->ins_bbase.p,
                       (const int64_t*)nullptr, (int64_t)-1, (int64_t*)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    h->n_events = n;
    h->ins_from_set = true;
    h->have_weight = true;
    h->sorted_valid = true;
    return MC_OK;
}

extern "C" int mc_bases_consensus_ins(const mc_bases* h, int64_t* rows) {
    MC_REQUIRE(h, MC_E_INVALID, "null argument");
    MC_REQUIRE(h->have_cons && h->have_cons_ins, MC_E_STATE,
               "no consensus with MC_CONS_INS computed (call mc_bases_consensus)");
    MC_REQUIRE(h->S == 0 || rows, MC_E_INVALID, "null rows");
    if (h->S == 0) return MC_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(rows, h->cons_ins_rows.p, (size_t)h->S * 2 * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MC_OK;
}

extern "C" int mc_bases_ins_dims(int32_t* sort_chunk, int32_t* max_len) {
    MC_REQUIRE(sort_chunk && max_len, MC_E_INVALID, "null argument");
    *sort_chunk = kSortChunk;
    *max_len = kMaxInsLen;
    return MC_OK;
}
