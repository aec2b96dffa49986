// Insertion alleles: the kernels of the opt-in insertion stage of mc_bases
// (the contract is the header's, "Insertion alleles").  Included by bases.hip
// inside its anonymous namespace, behind Tile, Batch, lower_bound and
// tile_scan_kernel, the one-workgroup scan every stage here reuses.
//
// Launches, all on the handle's stream, none waiting on another workgroup:
//   ins_extract_kernel<false / true>   per batch, one workgroup per tile of the
//                         pileup launch's tile range, the same two binary
//                         searches; one THREAD per read (the walk reads CIGAR
//                         words only, a few per read, so a wave per read would
//                         idle 63 lanes).  The count pass writes the tile's
//                         number of events, tile_scan_kernel prefixes them,
//                         the fill pass appends 24-byte events to the handle's
//                         table inside the range its count pass sized (slot
//                         by an LDS counter, checked before every store) and
//                         loads query bases only inside I ops of at most 32.
//   ins_scatter_kernel    at group time: events into per-tile buckets (bases
//                         from a scan of the per-tile totals the fill passes
//                         kept), one global atomic per event for the slot.
//   ins_sort_kernel       one workgroup per tile with two or more events: a
//                         bitonic network with every comparator ascending
//                         (the first step of a merge mirrors, i ^ (k - 1)), so
//                         indices past the bucket's end act as +infinity and
//                         are skipped: no padding.  A bucket of at most
//                         kSortChunk events is sorted in LDS as 12-byte keys;
//                         a larger one runs the same network over global
//                         memory, strides below kSortChunk in LDS chunk by
//                         chunk.
//   ins_encode_kernel<false / true>    one workgroup per tile: run heads of the
//                         sorted bucket (run length by a binary search for the
//                         run's end), the threshold predicate with the depth
//                         from the planes, ballot ranks; count pass, scan,
//                         emit pass into the row arrays.
//   cons_ins_pick_kernel, cons_ins_fix_kernel, cons_emit_ins_kernel
//                         the consensus with MC_CONS_INS (see each).
// Every loop is bounded by an op count, a bucket size or the tile size.

struct InsEvent {
    int64_t i;         // plane index of the anchor
    uint32_t lo;       // other << 31 | len (0 for OTHER): (other, len) in numeric order
    uint32_t tile;     // the tile of i
    uint64_t code;
};
static_assert(sizeof(InsEvent) == 24, "insertion event");

constexpr int kSortChunk = 4096;                    // events sorted in LDS: 12 B x 4096 = 48 KiB, the pileup's footprint
constexpr int kMaxInsLen = 32;                      // a longer insertion is OTHER
constexpr uint32_t kInsOther = 0x80000000u;

template <bool kFill>
__global__ __launch_bounds__(kThreads) void ins_extract_kernel(Batch b, const int32_t* __restrict__ span,
                                                              const Tile* __restrict__ tiles,
                                                              const int32_t* __restrict__ order, int32_t max_span,
                                                              int32_t* __restrict__ counts,
                                                              const int64_t* __restrict__ base,
                                                              InsEvent* __restrict__ events, int64_t cap,
                                                              int32_t* __restrict__ tile_total) {
    __shared__ int32_t n_s;
    const int32_t ti = order[blockIdx.x];
    const Tile t = tiles[ti];
    const int64_t t0 = t.rel, t1 = t.rel + t.n;
    const int64_t lo = lower_bound(b, t.tid, t0 > max_span ? t0 - max_span : 0);
    const int64_t hi = lower_bound(b, t.tid, t1);
    const int32_t limit = kFill ? counts[blockIdx.x] : 0;
    const int64_t out = kFill ? base[blockIdx.x] : 0;
    if (kFill && limit == 0) return;
    if (threadIdx.x == 0) n_s = 0;
    __syncthreads();
    int32_t mine = 0;
    for (int64_t r = lo + threadIdx.x; r < hi; r += kThreads) {
        const int64_t pos = b.pos[r];
        if (pos + span[r] <= t0) continue;
        const int64_t c0 = b.cig_off[r], c1 = b.cig_off[r + 1];
        int64_t rp = pos, q = 0;
        // an anchor is rp - 1: past the tile once rp > t1
        for (int64_t k = c0; k < c1 && rp <= t1; ++k) {
            const uint32_t cw = b.cigar[k];
            const uint32_t op = cw & 15u;
            const int64_t len = cw >> 4;
            if (op == 1) {
                if (len >= 1 && rp > pos && rp - 1 >= t0 && rp - 1 < t1) {
                    if (!kFill) {
                        ++mine;
                    } else {
                        const int32_t slot = atomicAdd(&n_s, 1);
                        if (slot < limit && out + slot < cap) {
                            const int64_t so = b.seq_off[r], l = b.l_seq[r];
                            bool other = len > kMaxInsLen;
                            uint64_t code = 0;
                            if (!other) {
                                for (int j = 0; j < (int)len; ++j) {
                                    const int64_t qq = q + j;
                                    uint32_t nt = 0;
                                    if (qq < l) {
                                        const uint32_t byte = b.seq[so + (qq >> 1)];
                                        nt = (qq & 1) ? (byte & 15u) : (byte >> 4);
                                    }
                                    const uint32_t v = nt == 1 ? 0u : nt == 2 ? 1u : nt == 4 ? 2u : nt == 8 ? 3u : 4u;
                                    other = other || v == 4u;
                                    code = (code << 2) | (v & 3u);
                                }
                            }
                            InsEvent e;
                            e.i = t.out + (rp - 1 - t0);
                            e.lo = other ? kInsOther : (uint32_t)len;
                            e.tile = (uint32_t)ti;
                            e.code = other ? 0ull : code;
                            events[out + slot] = e;
                        }
                    }
                }
                q += len;
            } else if (op == 4) {
                q += len;
            } else if (op == 0 || op == 7 || op == 8) {
                rp += len;
                q += len;
            } else if (op == 2 || op == 3) {
                rp += len;
            }
        }
    }
    if (!kFill) {
        if (mine) atomicAdd(&n_s, mine);
        __syncthreads();
        if (threadIdx.x == 0) counts[blockIdx.x] = n_s;
    } else {
        // (one owner per tile in a launch, the launches ordered on the stream: plain load-add-store)
        if (threadIdx.x == 0) tile_total[ti] += limit;
    }
}

__global__ __launch_bounds__(kThreads) void ins_scatter_kernel(const InsEvent* __restrict__ events, int64_t n,
                                                              int64_t n_tiles, const int64_t* __restrict__ bbase,
                                                              int32_t* __restrict__ cursor,
                                                              InsEvent* __restrict__ sorted) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const InsEvent v = events[e];
    if ((int64_t)v.tile >= n_tiles) return;
    const int64_t a = bbase[v.tile], room = bbase[v.tile + 1] - a;
    const int32_t slot = atomicAdd(&cursor[v.tile], 1);
    if (slot < room) sorted[a + slot] = v;
}

__device__ __forceinline__ bool ins_less(const InsEvent& x, const InsEvent& y) {
    if (x.i != y.i) return x.i < y.i;
    if (x.lo != y.lo) return x.lo < y.lo;
    return x.code < y.code;
}
__device__ __forceinline__ bool ins_same(const InsEvent& x, const InsEvent& y) {
    return x.i == y.i && x.lo == y.lo && x.code == y.code;
}

// One step of the network on the m keys in LDS.  Pair p of a mirror step of
// block size k is (block * k + off, block * k + k - 1 - off); of a stride
// step j it is (i, i + j) with bit j of i clear.  The upper index past m: skip.
__device__ __forceinline__ void lds_step(uint32_t* khi, uint64_t* kcode, int m, int pairs, int k, int j) {
    for (int p = threadIdx.x; p < pairs; p += kThreads) {
        int i, l;
        if (k) {
            const int half = k >> 1, blk = p / half, off = p - blk * half;
            i = blk * k + off;
            l = blk * k + k - 1 - off;
        } else {
            i = 2 * j * (p / j) + (p % j);
            l = i + j;
        }
        if (l < m) {
            const uint32_t hi = khi[i], hl = khi[l];
            const uint64_t ci = kcode[i], cl = kcode[l];
            if (hl < hi || (hl == hi && cl < ci)) {
                khi[i] = hl;
                khi[l] = hi;
                kcode[i] = cl;
                kcode[l] = ci;
            }
        }
    }
    __syncthreads();
}

// Bucket elements [c0, c0 + m) to LDS keys and back.  The key's high word is
// (i - tile's first index) << 7 | other << 6 | len: 11 + 1 + 6 bits.
__device__ __forceinline__ void lds_load(const InsEvent* g, int64_t c0, int m, int64_t out0, uint32_t* khi,
                                         uint64_t* kcode) {
    for (int e = threadIdx.x; e < m; e += kThreads) {
        const InsEvent v = g[c0 + e];
        khi[e] = ((uint32_t)(v.i - out0) << 7) | ((v.lo >> 31) << 6) | (v.lo & 63u);
        kcode[e] = v.code;
    }
    __syncthreads();
}
__device__ __forceinline__ void lds_store(InsEvent* g, int64_t c0, int m, int64_t out0, uint32_t tile,
                                          const uint32_t* khi, const uint64_t* kcode) {
    for (int e = threadIdx.x; e < m; e += kThreads) {
        const uint32_t h = khi[e];
        InsEvent v;
        v.i = out0 + (h >> 7);
        v.lo = ((h >> 6) & 1u) ? kInsOther : (h & 63u);
        v.tile = tile;
        v.code = kcode[e];
        g[c0 + e] = v;
    }
    __syncthreads();
}

__device__ __forceinline__ int pow2_ceil(int m) {
    int p = 1;
    while (p < m) p <<= 1;
    return p;
}

__global__ __launch_bounds__(kThreads) void ins_sort_kernel(InsEvent* __restrict__ sorted,
                                                           const int64_t* __restrict__ bbase,
                                                           const Tile* __restrict__ tiles) {
    __shared__ uint32_t khi[kSortChunk];
    __shared__ uint64_t kcode[kSortChunk];
    const int64_t a = bbase[blockIdx.x], n = bbase[blockIdx.x + 1] - a;
    if (n < 2) return;
    const int64_t out0 = tiles[blockIdx.x].out;
    InsEvent* g = sorted + a;
    // every chunk sorted in LDS: the stages k = 2 .. kSortChunk of the network
    for (int64_t c0 = 0; c0 < n; c0 += kSortChunk) {
        const int m = (int)(n - c0 < kSortChunk ? n - c0 : kSortChunk);
        const int m2 = pow2_ceil(m);
        lds_load(g, c0, m, out0, khi, kcode);
        for (int k = 2; k <= m2; k <<= 1) {
            lds_step(khi, kcode, m, m2 >> 1, k, 0);
            for (int j = k >> 2; j >= 1; j >>= 1) lds_step(khi, kcode, m, m2 >> 1, 0, j);
        }
        lds_store(g, c0, m, out0, blockIdx.x, khi, kcode);
    }
    if (n <= kSortChunk) return;
    // the stages above: strides of kSortChunk and more over global memory, the rest per chunk in LDS
    for (int64_t k = 2 * kSortChunk; (k >> 1) < n; k <<= 1) {
        const int64_t half = k >> 1, blocks = (n + k - 1) / k;
        for (int64_t p = threadIdx.x; p < blocks * half; p += kThreads) {
            const int64_t blk = p / half, off = p - blk * half;
            const int64_t i = blk * k + off, l = blk * k + k - 1 - off;
            if (l < n) {
                const InsEvent x = g[i], y = g[l];
                if (ins_less(y, x)) {
                    g[i] = y;
                    g[l] = x;
                }
            }
        }
        __syncthreads();
        for (int64_t j = k >> 2; j >= kSortChunk; j >>= 1) {
            const int64_t pairs = ((n + 2 * j - 1) / (2 * j)) * j;
            for (int64_t p = threadIdx.x; p < pairs; p += kThreads) {
                const int64_t i = 2 * j * (p / j) + (p % j), l = i + j;
                if (l < n) {
                    const InsEvent x = g[i], y = g[l];
                    if (ins_less(y, x)) {
                        g[i] = y;
                        g[l] = x;
                    }
                }
            }
            __syncthreads();
        }
        for (int64_t c0 = 0; c0 < n; c0 += kSortChunk) {
            const int m = (int)(n - c0 < kSortChunk ? n - c0 : kSortChunk);
            lds_load(g, c0, m, out0, khi, kcode);
            for (int j = kSortChunk >> 1; j >= 1; j >>= 1) lds_step(khi, kcode, m, kSortChunk >> 1, 0, j);
            lds_store(g, c0, m, out0, blockIdx.x, khi, kcode);
        }
    }
}

// The rows of one tile's sorted bucket: a run of equal events is one row, its
// count the run's length (or, for a table installed by mc_bases_ins_set, the
// weight of its single event).  A row is kept iff depth >= min_depth, count >=
// min_count and count * 10^6 >= min_ppm * depth, depth = A + C + G + T + DEL at i.
template <bool kEmit>
__global__ __launch_bounds__(kThreads) void ins_encode_kernel(const InsEvent* __restrict__ sorted,
                                                             const uint32_t* __restrict__ weight,
                                                             const int64_t* __restrict__ bbase,
                                                             const uint32_t* __restrict__ planes, int64_t stride,
                                                             SiteArgs s, int32_t* __restrict__ rowcount,
                                                             const int64_t* __restrict__ rowbase,
                                                             int64_t* __restrict__ o_i, int32_t* __restrict__ o_len,
                                                             uint64_t* __restrict__ o_code,
                                                             uint8_t* __restrict__ o_other,
                                                             uint32_t* __restrict__ o_cnt) {
    __shared__ int32_t wcnt[kWaves];
    const int64_t a = bbase[blockIdx.x], n = bbase[blockIdx.x + 1] - a;
    if (n == 0) {
        if (!kEmit && threadIdx.x == 0) rowcount[blockIdx.x] = 0;
        return;
    }
    const InsEvent* g = sorted + a;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t run = kEmit ? rowbase[blockIdx.x] : 0;
    const int64_t end = kEmit ? rowbase[blockIdx.x + 1] : 0;
    for (int64_t e0 = 0; e0 < n; e0 += kThreads) {
        const int64_t e = e0 + threadIdx.x;
        bool keep = false;
        InsEvent me;
        unsigned long long cnt = 0;
        if (e < n) {
            me = g[e];
            if (e == 0 || !ins_same(g[e - 1], me)) {
                if (weight) {
                    cnt = weight[a + e];
                } else {
                    int64_t x = e + 1, z = n;              // the first event past the run
                    while (x < z) {
                        const int64_t mid = x + ((z - x) >> 1);
                        if (ins_same(g[mid], me))
                            x = mid + 1;
                        else
                            z = mid;
                    }
                    cnt = (unsigned long long)(x - e);
                }
                const unsigned long long depth = (unsigned long long)planes[me.i] + planes[stride + me.i] +
                                                 planes[2 * stride + me.i] + planes[3 * stride + me.i] +
                                                 planes[5 * stride + me.i];
                keep = depth >= s.min_depth && cnt >= s.min_count && cnt * 1000000ull >= s.min_ppm * depth;
            }
        }
        const unsigned long long m = __ballot(keep);
        const int32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int64_t mine = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w == wave) mine = run;
            run += wcnt[w];
        }
        if (kEmit && keep) {
            const int64_t o = mine + rank;
            if (o < end) {
                o_i[o] = me.i;
                o_len[o] = (int32_t)(me.lo & 63u);
                o_code[o] = me.code;
                o_other[o] = (uint8_t)(me.lo >> 31);
                o_cnt[o] = (uint32_t)cnt;
            }
        }
        __syncthreads();                                    // wcnt is free for the next round
    }
    if (!kEmit && threadIdx.x == 0) rowcount[blockIdx.x] = (int32_t)run;
}

// ---- consensus with MC_CONS_INS ---------------------------------------------
// The table these kernels read was encoded with the consensus thresholds
// (depth >= max(min_depth, 1): the position is not LOW; count >= max(min_count,
// 1) and count * 10^6 >= call_ppm * depth: qualifies), so every row in it
// qualifies; qualifies is monotone in the count, so the top allele qualifies
// iff any row of its position is in the table.

// One workgroup per tile, one thread per row of it: the first row of a
// position's group that is not OTHER walks the group's non-OTHER rows (they
// sort before OTHER, by len, then code) and marks the first maximum of the
// count: ties go to the shorter len, then the smaller code.  called[] is
// zeroed before the launch.  The tile's called insertions and their bases go
// into two per-tile columns.
__global__ __launch_bounds__(kThreads) void cons_ins_pick_kernel(const int64_t* __restrict__ rowbase,
                                                                const int64_t* __restrict__ o_i,
                                                                const int32_t* __restrict__ o_len,
                                                                const uint8_t* __restrict__ o_other,
                                                                const uint32_t* __restrict__ o_cnt,
                                                                uint8_t* __restrict__ called,
                                                                int32_t* __restrict__ col_bases,
                                                                int32_t* __restrict__ col_calls) {
    __shared__ int32_t nb, nc;
    const int64_t r0 = rowbase[blockIdx.x], r1 = rowbase[blockIdx.x + 1];
    if (r0 == r1) {
        if (threadIdx.x == 0) {
            col_bases[blockIdx.x] = 0;
            col_calls[blockIdx.x] = 0;
        }
        return;
    }
    if (threadIdx.x == 0) nb = nc = 0;
    __syncthreads();
    for (int64_t r = r0 + threadIdx.x; r < r1; r += kThreads) {
        const int64_t i = o_i[r];
        if ((r == r0 || o_i[r - 1] != i) && !o_other[r]) {
            int64_t best = r;
            for (int64_t j = r + 1; j < r1 && o_i[j] == i && !o_other[j]; ++j)
                if (o_cnt[j] > o_cnt[best]) best = j;
            called[best] = 1;
            atomicAdd(&nb, o_len[best]);
            atomicAdd(&nc, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        col_bases[blockIdx.x] = nb;
        col_calls[blockIdx.x] = nc;
    }
}

// One thread per segment: out_first and the summary's length take the
// inserted bases in; rows2[s] = (insertions called, bases inserted).
__global__ void cons_ins_fix_kernel(int64_t S, const int64_t* __restrict__ first_bases,
                                    const int64_t* __restrict__ first_calls, int64_t* __restrict__ out_first,
                                    int64_t* __restrict__ rows, int64_t* __restrict__ rows2) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > S) return;
    out_first[s] += first_bases[s];
    if (s < S) {
        const int64_t nb = first_bases[s + 1] - first_bases[s];
        rows[s * kConsCols + 7] += nb;
        rows2[2 * s] = first_calls[s + 1] - first_calls[s];
        rows2[2 * s + 1] = nb;
    }
}

// cons_emit_kernel with the called insertions of the tile: their rows go into
// an LDS map position -> row, a kept letter's offset counts the kept letters
// and the inserted bases before it, and the position's thread writes its
// insertion's letters behind its own letter (or, where the position was called
// DEL, where that letter would have been).
__global__ __launch_bounds__(kThreads) void cons_emit_ins_kernel(const uint8_t* __restrict__ aligned,
                                                                const Tile* __restrict__ tiles,
                                                                const int64_t* __restrict__ base,
                                                                const int64_t* __restrict__ ins_base,
                                                                const int64_t* __restrict__ rowbase,
                                                                const int64_t* __restrict__ o_i,
                                                                const int32_t* __restrict__ o_len,
                                                                const uint64_t* __restrict__ o_code,
                                                                const uint8_t* __restrict__ called,
                                                                uint8_t* __restrict__ compact, int64_t cap) {
    __shared__ int32_t wcnt[kRounds][kWaves];
    __shared__ int32_t row_of[kTile];
    const Tile t = tiles[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = rowbase[blockIdx.x], r1 = rowbase[blockIdx.x + 1];
    const bool any = r1 > r0;                               // (uniform)
    if (any) {
        for (int k = threadIdx.x; k < kTile; k += kThreads) row_of[k] = -1;
        __syncthreads();
        for (int64_t r = r0 + threadIdx.x; r < r1; r += kThreads) {
            const int64_t k = o_i[r] - t.out;
            if (called[r] && k >= 0 && k < t.n) row_of[k] = (int32_t)(r - r0);
        }
        __syncthreads();
    }
    uint32_t letter[kRounds];
    int32_t before[kRounds], row[kRounds], ilen[kRounds];   // kept letters and inserted bases in lower lanes
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int k = r * kThreads + (int)threadIdx.x;
        letter[r] = k < t.n ? (uint32_t)aligned[t.out + k] : (uint32_t)'-';
        row[r] = any && k < t.n ? row_of[k] : -1;
        ilen[r] = row[r] >= 0 ? o_len[r0 + row[r]] : 0;
        const int32_t mine = (letter[r] != (uint32_t)'-' ? 1 : 0) + ilen[r];
        int32_t inc = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t o = __shfl_up(inc, off, 64);
            if (lane >= off) inc += o;
        }
        before[r] = inc - mine;
        if (lane == 63) wcnt[r][wave] = inc;
    }
    __syncthreads();
    int64_t run = base[blockIdx.x] + ins_base[blockIdx.x];  // positions ascend with (round, wave, lane)
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        int64_t mine = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w == wave) mine = run;
            run += wcnt[r][w];
        }
        int64_t o = mine + before[r];
        if (letter[r] != (uint32_t)'-') {
            if (o < cap) compact[o] = (uint8_t)letter[r];
            ++o;
        }
        if (ilen[r] > 0) {
            const uint64_t code = o_code[r0 + row[r]];
            for (int j = 0; j < ilen[r] && j < kMaxInsLen; ++j)
                if (o + j < cap) compact[o + j] = (uint8_t)((0x54474341u >> (8 * ((code >> (2 * (ilen[r] - 1 - j))) & 3u))) & 0xFFu);
        }
    }
}
