/*
 * metacov_amd — MI355X (gfx950) per-base coverage engine, C ABI.
 *
 * Drop-in replacement for the arithmetic under the reference's pileup path:
 *
 *   metacov pileup (metacov/cli.py:49-108)
 *     -> pileup.classic(bam, ref, start, end)      (metacov/pileup.py:9-26)
 *        -> pysam AlignmentFile.pileup()  ->  htslib bam_plp / PileupColumn.n
 *           (called at metacov/pileup.py:13; third-party, unpinned)
 *        -> numpy min/max/median/std/mean/sorted()/sum  (pileup.py:18-26)
 *
 * and of the reference's only hand-written BAM read iterator
 * (scan.AlignmentFileIterator, metacov/scan.pyx:188-294; decl scan.pxd:6-27),
 * whose per-record callback protocol (ReadProcessor.process_read,
 * scan.pxd:30-36) is replaced by a batched struct-of-arrays interface.
 *
 * Conventions
 *  - every function returns int: 0 = ok, < 0 = error (MC_E_*); the message
 *    of the last error on the calling thread is mc_last_error().
 *  - callers own all host buffers; they are copied during the call.
 *  - the library owns device buffers, inside an opaque mc_ctx (one per GPU).
 *    A ctx is not thread-safe; distinct ctxs may be driven from distinct
 *    host threads.  There is no CPU fallback: a ctx needs a HIP device.
 *  - positions are 0-based; regions are half-open [start, end).
 */
#ifndef METACOV_AMD_H
#define METACOV_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MC_OK            0
#define MC_E_INVALID    -1   /* bad argument (null pointer, range, unsorted reads, ...) */
#define MC_E_HIP        -2   /* HIP runtime error (no device, OOM, launch failure) */
#define MC_E_IO         -3   /* file / BGZF / BAM format error */
#define MC_E_STATE      -4   /* call out of order (e.g. stats before depth) */
#define MC_E_RANGE      -5   /* value outside what the engine represents exactly */

/* Per-region statistics, exact integers.  Everything classic() reports
 * (pileup.py:18-26) follows from it:
 *   min = min, max = max, sum = sum,
 *   avg = round(sum / n, 2), std = round(sqrt((n*sumsq - sum^2) / n^2), 2),
 *   med = (med_lo + med_hi) / 2 truncated (np.median then int()),
 *   q23 = round(q23_sum / q23_cnt, 2)
 * with med_lo = sorted[(n-1)/2], med_hi = sorted[n/2] and q23_sum the sum of
 * sorted[n/4 .. n - n/4)  (pileup.py:24).  n == 0 marks an empty region
 * (classic raises ValueError there). */
typedef struct mc_region_stat {
    int64_t  n;
    int64_t  sum;
    uint64_t sumsq;
    int64_t  min;
    int64_t  max;
    int64_t  med_lo;
    int64_t  med_hi;
    int64_t  q23_sum;
    int64_t  q23_cnt;
} mc_region_stat;

/* Kernel timings of the last mc_compute_depth / mc_region_stats calls, in
 * milliseconds, from HIP events recorded on the ctx stream. */
typedef struct mc_timings {
    float cigar_ms;      /* K1: CIGAR -> span (0 when spans were given) */
    float depth_ms;      /* K2: tile depth kernel */
    float stats_ms;      /* K3: region histogram + reduction (+ finalize) */
    float prepare_ms;    /* ingest: sortedness check, extents, tile index */
    int64_t depth_launches;
    int64_t stats_launches;
    /* Sums over every mc_compute_depth_stats[_device] call of this ctx (each
     * read once its stream has drained inside the call), so a caller can
     * average many calls without a timing query between them. */
    double fused_depth_ms_total;   /* K2 */
    double fused_stats_ms_total;   /* K3b (+ fallback K3) */
    int64_t fused_calls;
    /* Batches prepared by the direct path and accepted by K2's checks, and
     * full mc_prepare passes (explicit, or a direct batch handed over). */
    int64_t direct_batches;
    int64_t full_prepares;
    double prepare_ms_total;       /* every prepare's prepare_ms (direct: the probe) */
    /* Direct batches redone with a wider halo (their spans outgrew the one
     * the previous batch set), and the halo (positions) of the last one. */
    int64_t halo_redos;
    int64_t direct_halo;
} mc_timings;

typedef struct mc_ctx mc_ctx;

const char* mc_last_error(void);
const char* mc_version(void);
/* "mc-source-sha256:<hex>": the sources and flags this library was built from
 * (metacov_amd/build.py rebuilds when the tree's hash differs). */
const char* mc_build_id(void);

/* The HIP runtime and device `device`'s context, initialised ahead of the
 * first mc_ctx_create (which does it anyway): the CLI calls it on a thread
 * while Python imports its modules, so the two start-up costs overlap
 * (nothing in the reference; pysam has no device to initialise).  A device
 * out of range initialises the runtime only. */
int mc_runtime_init(int device);

/* ---- context ------------------------------------------------------------ */
int mc_ctx_create(int device, mc_ctx** out);
int mc_ctx_destroy(mc_ctx* ctx);
/* Use an external hipStream_t (e.g. torch's current stream); NULL = own stream. */
int mc_ctx_set_stream(mc_ctx* ctx, void* hip_stream);
int mc_ctx_device(const mc_ctx* ctx, int* device);

/* ---- inputs ------------------------------------------------------------- */
/* Contig table: the BAM header's @SQ lengths (pysam bam.lengths,
 * used at util.py:64-69).  Resets reads and depth. */
int mc_set_contigs(mc_ctx* ctx, int32_t n, const int64_t* lengths);

/* Append coordinate-sorted pileup intervals (host pointers): read i covers
 * [pos[i], pos[i] + span[i]) on contig tid[i].  These are the records the
 * pileup "all" stepper keeps (flag & 0x704 == 0), span = reference length
 * of the CIGAR (ops M/D/N/=/X), 0 for a mapped read with none (1 under
 * MC_LEGACY_ENDPOS); a span-0 read adds no depth.
 * Replaces: per-record AlignmentFileIterator.cnext()/get_tid()/get_pos()
 * (scan.pyx:213-283) feeding ReadProcessor.process_read (scan.pxd:35). */
int mc_add_reads(mc_ctx* ctx, int64_t n, const int32_t* tid,
                 const int32_t* pos, const int32_t* span);

/* Same, but the copy is only enqueued on the ctx stream: with pinned host
 * buffers (hipHostMalloc / torch pin_memory) the DMA overlaps the caller's
 * next decode.  The buffers must stay unchanged until mc_synchronize(ctx)
 * (double-buffered streaming ingest: fill B, mc_synchronize, add A's
 * successor ...). */
int mc_add_reads_async(mc_ctx* ctx, int64_t n, const int32_t* tid,
                       const int32_t* pos, const int32_t* span);

/* Page-locked host buffers for mc_add_reads_async (hipHostMalloc). */
int mc_pinned_alloc(int64_t bytes, void** out);
int mc_pinned_free(void* p);

/* Same, but the three arrays are already in this ctx's device memory
 * (e.g. torch tensors); they are copied into the ctx. */
int mc_add_reads_device(mc_ctx* ctx, int64_t n, const int32_t* d_tid,
                        const int32_t* d_pos, const int32_t* d_span);

/* Long-read / raw-CIGAR mode: spans are computed on the GPU (K1) from the
 * BAM-packed CIGAR words (op in low 4 bits, length << 4) of each read,
 * read i owning cigar[cig_off[i] .. cig_off[i+1]).  Host pointers. */
int mc_add_reads_cigar(mc_ctx* ctx, int64_t n, const int32_t* tid,
                       const int32_t* pos, const int64_t* cig_off,
                       const uint32_t* cigar);

/* Same with device pointers (a batch already in HBM, e.g. torch tensors).
 * tid / pos are copied into the ctx before the call returns (the caller may
 * free or overwrite them afterwards); cig_off and cigar are BORROWED: they
 * must stay valid until the next mc_prepare (K1 reads them there), so a
 * 40 GB CIGAR batch is never duplicated.  cig_off[0] must be 0. */
int mc_add_reads_cigar_device(mc_ctx* ctx, int64_t n, const int32_t* d_tid,
                              const int32_t* d_pos, const int64_t* d_cig_off,
                              const uint32_t* d_cigar);

/* K1's span of a read whose CIGAR has no reference-consuming op: 0 (current
 * htslib bam_plp_push, the default) or 1 (legacy = 1: htslib <= 1.9
 * bam_endpos; see MC_LEGACY_ENDPOS).  Applies to later mc_add_reads_cigar*. */
int mc_set_legacy_endpos(mc_ctx* ctx, int legacy);

/* Drops the ctx's reads (the contigs stay): the next batch starts empty. */
int mc_clear_reads(mc_ctx* ctx);

/* The full prepare: validates order, computes contig extents (max of length
 * and furthest read end), the chunk index, K2's packed read words and the
 * long-read buckets.  Compute calls run it when the direct path (see
 * mc_set_direct_prepare) cannot take the batch; an explicit call builds an
 * index that later compute calls reuse. */
int mc_prepare(mc_ctx* ctx);

/* Drops the prepared index and depth (the reads stay): the next compute call
 * prepares the same device reads again, as for a fresh batch (what the
 * benchmark's per-batch step times). */
int mc_invalidate(mc_ctx* ctx);

/* Per-batch prepare of the compute calls (default on).  A compute call on a
 * batch that mc_prepare has not seen takes the DIRECT path: a sparse sample
 * of the reads (every 256th) locates each chunk's reads, K2 loads the raw
 * (tid, pos, span) and checks every read itself (range, order, end within
 * its contig, span <= 4096), so no separate pass over the batch runs before
 * K2.  A batch the direct path cannot take (unsorted / invalid reads: the
 * full prepare raises its exact error; long reads or reads past their
 * contig's end: handled by the full prepare, and later batches of the same
 * contig set go there directly) is re-run through mc_prepare inside the same
 * call, so results never depend on the path.  enable = 0: always mc_prepare. */
int mc_set_direct_prepare(mc_ctx* ctx, int enable);

/* ---- compute ------------------------------------------------------------ */
/* Per-position depth of every contig (K1 if needed, then K2). */
int mc_compute_depth(mc_ctx* ctx);

/* Copy depth[start, end) of contig tid to host (zeros past the extent). */
int mc_get_depth(mc_ctx* ctx, int32_t tid, int64_t start, int64_t end, int32_t* out);

/* Device pointer to the concatenated depth vector and each contig's offset
 * into it (for zero-copy consumers, e.g. torch). */
int mc_depth_device(mc_ctx* ctx, const int32_t** d_depth, int64_t* total_len);
int mc_contig_offset(mc_ctx* ctx, int32_t tid, int64_t* offset, int64_t* extent);

/* Region statistics (K3) for R regions; rows in input order.  Regions may
 * overlap and may run past the contig end (those positions count as 0,
 * as in pileup.py:11-16). */
int mc_region_stats(mc_ctx* ctx, int64_t R, const int32_t* tid,
                    const int64_t* start, const int64_t* end,
                    mc_region_stat* out);

/* Same, writing the R rows into device memory (for an RCCL all-gather). */
int mc_region_stats_device(mc_ctx* ctx, int64_t R, const int32_t* tid,
                           const int64_t* start, const int64_t* end,
                           mc_region_stat* d_out);

/* numpy's float64 sum of squared deviations of each region's column vector,
 * in numpy's own order, from the depth vector in HBM: with m = mean[r]
 * (= fl(sum / n), what np.mean returns), out[r] = the sum np.std forms over
 * fl(fl(v - m)^2): pairwise_sum within each 8192-element reduction buffer,
 * the buffers added in turn.  sqrt(fl(out[r] / n)) is then np.std(columns)
 * bit for bit (pileup.py:22).  classic() rounds it to two decimals; the
 * exact variance rounds the same way except within numpy's rounding noise of
 * a .xx5 boundary, and only such regions need this (metacov_amd.engine).
 * Regions must be non-empty; positions past the extent count as 0. */
int mc_region_np_sqdev(mc_ctx* ctx, int64_t R, const int32_t* tid,
                       const int64_t* start, const int64_t* end,
                       const double* mean, double* out);

/* Depth AND region statistics in one pass: K2 folds every tile into the
 * regions covering it while the depth values are still in registers, so the
 * depth vector is written once and never re-read.  Regions must not overlap
 * each other for the fused path (whole contigs, a tiling of a contig, most
 * BLAST hit lists); otherwise this runs K2 then K3.  Same rows as
 * mc_region_stats.  Each region's histogram window holds 864 values (1728 for
 * long reads) around its contig's estimated depth; a region whose median /
 * q23 ranks fall outside it is recomputed exactly from the depth vector
 * (mc_fused_recomputes / mc_fused_fallbacks). */
int mc_compute_depth_stats(mc_ctx* ctx, int64_t R, const int32_t* tid,
                           const int64_t* start, const int64_t* end,
                           mc_region_stat* out);
int mc_compute_depth_stats_device(mc_ctx* ctx, int64_t R, const int32_t* tid,
                                  const int64_t* start, const int64_t* end,
                                  mc_region_stat* d_out);
int mc_fused_fallbacks(mc_ctx* ctx, int64_t* out);
/* Regions of the last fused call whose median / q23 ranks left their LDS
 * window and were recomputed exactly ON THE DEVICE within the call (long-read
 * batches, or after a call that had such regions: the depth vector is
 * re-read for those regions only, no host round trip); mc_fused_fallbacks
 * counts the ones the host's K3 recomputed instead. */
int mc_fused_recomputes(mc_ctx* ctx, int64_t* out);

/* Aligned bases (sum of spans) of the reads added so far. */
int mc_aligned_bases(mc_ctx* ctx, int64_t* out);
int mc_max_depth(mc_ctx* ctx, int32_t* out);
int mc_get_timings(mc_ctx* ctx, mc_timings* out);
int mc_synchronize(mc_ctx* ctx);

/* ---- per-base depth as runs (csrc/runs.hip) --------------------------------
 * The depth vector run-length encoded on the device: what bedtools genomecov
 * -bg/-bga, mosdepth and samtools depth write as (contig, start, end, depth)
 * lines (nothing in the reference, whose pileup reports the nine statistics
 * only).  Depths are exact: the pileup read cap (below) is a per-query
 * artefact and is not applied.
 *
 * mc_runs_compute: for each of S segments [start, end) of contig tid, in
 * input order, the maximal runs of equal q(depth).  Segments may be unsorted,
 * overlapping, duplicated or empty and may run past the contig's extent
 * (those positions have depth 0, as in mc_get_depth, and take part like any
 * value: zero runs are kept).  q(d) = d with n_edges = 0; else the number of
 * edges <= d (n_edges <= 16 strictly increasing non-negative edges; 1, 4, 100
 * are mosdepth's --quantize 0:1:4:100:).  Run i starts at run_start[i]
 * (relative to the contig) with value run_value[i] and ends where the next
 * run of its segment starts, or at the segment's end; segment s owns runs
 * [seg_first[s], seg_first[s + 1]) (none when it is empty).  A run never
 * crosses a segment boundary.  *n_runs = seg_first[S].
 *
 * The ctx's depth must be computed (MC_E_STATE) on the handle's device
 * (MC_E_INVALID, as for a bad tid, range or edge list).  The call waits for
 * the ctx (mc_synchronize), then runs on the handle's own stream: one count
 * pass and one emit pass over the segments' depth (two reads of 4 B per
 * position), an exclusive scan of the per-tile counts between them.  Results
 * stay in device memory owned by the handle (12 B per run; buffers only grow
 * and are reused) until the next mc_runs_compute or mc_runs_destroy.
 * mc_runs_get copies runs [first, first + count) to the host
 * (MC_E_INVALID outside [0, n_runs]); mc_runs_device exposes the arrays to
 * zero-copy consumers.  mc_runs_timing: HIP-event times of the three launches
 * of the last compute and its tile count.  mc_runs_dims (test hook): the tile
 * size and the tiles the scan takes per iteration. */
typedef struct mc_runs mc_runs;
int mc_runs_create(int device, mc_runs** out);
int mc_runs_destroy(mc_runs* r);
int mc_runs_compute(mc_runs* r, mc_ctx* ctx, int64_t S, const int32_t* tid, const int64_t* start,
                    const int64_t* end, int32_t n_edges, const int32_t* edges, int64_t* n_runs);
int mc_runs_seg_first(const mc_runs* r, int64_t* seg_first /* S + 1 */);
int mc_runs_get(const mc_runs* r, int64_t first, int64_t count, int64_t* run_start, int32_t* run_value);
int mc_runs_device(const mc_runs* r, const int64_t** d_start, const int32_t** d_value,
                   const int64_t** d_seg_first, int64_t* n_runs);
int mc_runs_timing(const mc_runs* r, float* count_ms, float* scan_ms, float* emit_ms, int64_t* tiles);
int mc_runs_dims(int32_t* tile, int32_t* scan_width);

/* ---- windowed coverage (csrc/windows.hip) ----------------------------------
 * The form between the nine statistics per region and the per-base runs: the
 * depth sum and threshold counts of fixed windows (mosdepth --by / --thresholds,
 * deepTools bins, CoverM's covered fraction) and the depth histogram per
 * segment (mosdepth's *.dist.txt).  One streaming read of the depth vector
 * each; integer only, exact and identical from call to call.  Nothing in the
 * reference.  Depths are exact (no pileup read cap).
 *
 * Segments are mc_runs_compute's: unsorted, overlapping, duplicated or empty
 * ones are fine, positions past the contig's extent have depth 0 and count
 * like any value; a bad tid, start < 0, end < start or end > 2^40 is
 * MC_E_INVALID (the message names the segment), as is a ctx on another
 * device; MC_E_STATE before the ctx's depth is computed.
 *
 * mc_windows_compute: segment s is cut into the windows
 * [start + k window, min(start + (k + 1) window, end)), k = 0 .. ceil(len /
 * window) - 1; window == 0: one window per non-empty segment, the whole of
 * it.  An empty segment owns no window.  Segment s owns windows [seg_first[s],
 * seg_first[s + 1]) (arithmetic, computed on the host, kept on the device for
 * mc_windows_device); *n_windows = seg_first[S] (more than 2^31: MC_E_RANGE).
 * Per window: sum, the exact int64 sum of its depths, and ge[j], the number of
 * its positions with depth >= thr[j] (0 <= n_thr <= 16 non-negative, strictly
 * increasing thresholds, else MC_E_INVALID; with n_thr == 0 ge may be NULL).
 * window is 0 or at least MC_WINDOWS_MIN (else MC_E_INVALID): below 16
 * positions a window's record is larger than the depth values it summarises,
 * and the runs above are the right output.  The call waits for the ctx
 * (mc_synchronize), then runs on the handle's own stream: one pass over the
 * segments' depth (4 B per position read once; a window inside one tile is
 * finished there, a longer one leaves a partial row per tile) and a combine
 * pass over the partial rows.  Results stay in device memory owned by the
 * handle (8 (1 + n_thr) B per window; buffers only grow and are reused) until
 * the next mc_windows_compute or mc_windows_destroy.  mc_windows_get copies
 * windows [first, first + count) to the host (MC_E_INVALID outside [0,
 * n_windows]); mc_windows_device exposes the arrays to zero-copy consumers.
 *
 * mc_windows_hist: hist[s][b], b < n_bins - 1, is the number of positions of
 * segment s with depth == b; the last bin counts depth >= n_bins - 1; every row
 * sums to end - start.  1 <= n_bins <= max_bins (mc_windows_dims; else
 * MC_E_INVALID); S n_bins above 2^27 is MC_E_RANGE.  Independent of
 * mc_windows_compute, whose results it leaves in place.
 *
 * mc_windows_timing: HIP-event times of the last compute's two launches and
 * of the last histogram launch, and the last compute's tile count (MC_E_STATE
 * before either ran).  mc_windows_dims (test hook): the tile size,
 * MC_WINDOWS_MIN, the bins the LDS layout affords, and the histogram's fixed
 * workgroup count. */
#define MC_WINDOWS_MIN 16
typedef struct mc_windows mc_windows;
int mc_windows_create(int device, mc_windows** out);
int mc_windows_destroy(mc_windows* w);
int mc_windows_compute(mc_windows* w, mc_ctx* ctx, int64_t S, const int32_t* tid, const int64_t* start,
                       const int64_t* end, int64_t window, int32_t n_thr, const int32_t* thr,
                       int64_t* n_windows);
int mc_windows_seg_first(const mc_windows* w, int64_t* seg_first /* S + 1 */);
int mc_windows_get(const mc_windows* w, int64_t first, int64_t count, int64_t* sum /* count */,
                   int64_t* ge /* count x n_thr, row-major */);
int mc_windows_device(const mc_windows* w, const int64_t** d_sum, const int64_t** d_ge,
                      const int64_t** d_seg_first, int64_t* n_windows, int32_t* n_thr);
int mc_windows_hist(mc_windows* w, mc_ctx* ctx, int64_t S, const int32_t* tid, const int64_t* start,
                    const int64_t* end, int32_t n_bins, int64_t* hist /* host, S x n_bins */);
int mc_windows_timing(const mc_windows* w, float* window_ms, float* combine_ms, float* hist_ms,
                      int64_t* tiles);
int mc_windows_dims(int32_t* tile, int32_t* min_window, int32_t* max_bins, int32_t* hist_groups);

/* ---- per-position base counts (csrc/bases.hip, csrc/bases_src.cpp) ----------
 * What the reads say at each position: counts of A, C, G, T, N and deletions
 * (channels MC_BASES_A .. MC_BASES_DEL), the numbers pysam's
 * AlignmentFile.count_coverage(), samtools mpileup, pysamstats and
 * bam-readcount report, and the variant sites among them.  Nothing in the
 * reference (metacov/pileup.py only reads PileupColumn.n); the contract is
 * this library's own, modelled on count_coverage.  Integer only: results are
 * exact, identical from call to call and independent of how the reads were
 * split into batches.  The handle is independent of any mc_ctx; it is not
 * thread-safe.
 *
 * Reads (mc_bases_add_batch; host pointers, copied during the call): n reads
 * sorted by (tid, pos), the order mc_add_reads demands, also across the
 * batches of one mc_bases_begin.  Read i has
 *   tid[i], pos[i]                      0 <= tid < n_ref, pos >= 0
 *   cigar[cig_off[i] .. cig_off[i+1])   BAM-packed words (len << 4 | op), as
 *                                       mc_add_reads_cigar
 *   l_seq[i]                            bases in the read
 *   seq[seq_off[i] ..]                  nt16 codes, two per byte, high nibble
 *                                       first ((l_seq + 1) / 2 bytes; any
 *                                       byte offset), as mc_scan_src_batch
 *   qual[qual_off[i] ..]                one quality byte per base (l_seq bytes)
 * cig_off, seq_off and qual_off have n + 1 entries; the last one is the size
 * of its arena.  Walking a read: from rpos = pos, qpos = 0, per CIGAR op
 *   M, =, X   each (qpos, rpos) pair counts one into the channel of the base;
 *             both advance
 *   D         counts one into DEL at each rpos (no quality test); rpos advances
 *   N         rpos advances
 *   I, S      qpos advances
 *   H, P      (and the unassigned op codes) nothing
 * nt16 codes 1, 2, 4, 8 are A, C, G, T; every other code, 0 ('=') included,
 * is N.  With min_baseq > 0 a base whose quality is below it counts nothing,
 * unless the read's first quality byte is 0xFF (qualities absent), which
 * passes any threshold.  A batch with an unsorted read, a tid outside
 * [0, n_ref), a negative pos or l_seq, a CIGAR whose query length (sum of
 * M/I/S/=/X) differs from l_seq, a reference span above 2^31 - 1 or offsets
 * outside the arenas is MC_E_INVALID; mc_last_error names the first such
 * read ("read <i>: ...") and the batch adds nothing.
 *
 * Segments (mc_bases_begin) are mc_runs_compute's (tid, start, end): unsorted,
 * overlapping, duplicated or empty ones are fine, and a segment may run past
 * the contig's end (the handle knows no contig lengths); a tid outside
 * [0, n_ref), start < 0, end < start or end > 2^40 is MC_E_INVALID (the
 * message names the segment).  begin allocates and zeroes counts[6][N],
 * N = sum of (end - start): plane c, index seg_off[s] + (p - start[s]), is the
 * count of channel c at position p of segment s (mc_bases_seg_off: S + 1
 * offsets).  A read counts into every segment that holds the position;
 * positions no read reaches stay 0.  A second begin starts from zero;
 * mc_bases_add_batch, _seg_off, _get, _device, _sites and _timing before the
 * first are MC_E_STATE.  mc_bases_get copies positions [first, first + count)
 * of the six planes to out[6][count] (MC_E_INVALID outside [0, N]);
 * mc_bases_device exposes the planes (plane c starts at d_planes + c * stride).
 *
 * Device side: a pre-pass kernel per batch (reference span and query length
 * per read, the checks above, the lowest bad index and the largest span), then
 * one 512-thread workgroup per tile of at most *tile positions of one segment:
 * the tile's reads by two binary searches, one LDS integer add per counted
 * base, and a flush of the LDS planes into the global ones by plain
 * load-add-store (one owner per tile; batches are ordered on the handle's
 * stream).  No global atomics.  Counts are uint32.
 *
 * Sites (mc_bases_sites), a second stage over the planes on the device: with
 * depth = A + C + G + T + DEL (N is never an allele), the base allele is the
 * reference allele where ref (optional, uint8 [N], indexed like a plane:
 * 0..3 = A/C/G/T, anything else = unknown) gives one, otherwise the allele
 * with the highest count (ties: the lowest channel); alt is the highest count
 * among the other four alleles.  Position p is a site iff depth >= min_depth,
 * alt >= min_count and alt * 10^6 >= min_ppm * depth (64-bit integers;
 * thresholds >= 0, min_ppm <= 10^6, else MC_E_INVALID).  Segment s owns sites
 * [site_first[s], site_first[s + 1]); site i is at site_pos[i] (relative to
 * the contig, ascending within a segment) with the six counts
 * site_counts[i][0..5].  Results stay in device memory owned by the handle
 * (buffers only grow) until the next mc_bases_sites, _add_batch, _set or _begin.
 * mc_bases_timing: HIP-event times since begin of the pre-pass and pileup
 * kernels (summed over the batches) and of the last sites call, the tile
 * count and the reads added.  mc_bases_dims (test hook): the tile size.
 *
 * mc_bases_src_*: the host record source that stands in for the read loop of
 * count_coverage (htslib sam_itr_next, bam_get_cigar / bam_get_seq /
 * bam_get_qual): the kept records of a coordinate-sorted BAM in the layout
 * above (each read's bases start on a 4-byte boundary).  Kept: tid >= 0,
 * (flag & flag_filter) == 0 (0x704: pysam's read_callback='all' and this
 * library's pileup filter) and mapq >= min_mapq.  Kept records without SEQ and
 * kept records whose CIGAR query length (CG:B,I resolved as htslib's
 * bam_read1 does) differs from l_seq are skipped and counted
 * (mc_bases_src_counts).  An unsorted file is MC_E_INVALID.  mc_bases_src_next
 * hands out up to max_reads reads (it stops once max_bases bases are in);
 * *n == 0 at the end of the file.  mc_bases_src_batch: the arrays of the last
 * batch, valid until the next call on the source.
 *
 * Strand (opt-in, as the insertion alleles are).  A read is on the reverse
 * strand iff flag & 0x10; no other flag bit matters.  Every count a read makes
 * (A, C, G, T, N, DEL) belongs to its strand; a deletion takes the strand of
 * the read it is in.  mc_bases_track_strand(h, on): on = 1 / 0 makes the NEXT
 * mc_bases_begin also allocate and zero rev[6][N] (or not); another value is
 * MC_E_INVALID.  rev is indexed exactly like the planes and holds the counts
 * of the reverse-strand reads; the six planes stay the totals, so
 * mc_bases_get, _sites, _consensus and _insertions give the same results with
 * tracking on as off, and forward = total - rev.  Integer only, exact,
 * independent of the batch split, repeatable.
 *   Reads: mc_bases_add_batch_flags / _add_batch_device_flags take the nine
 * arrays plus flag[n] (uint16, the BAM flag words; a device pointer for the
 * device call; a sub-range of a resident table is d_flag + a); checks and
 * error messages are mc_bases_add_batch's.  On a handle that tracks strand the
 * flag-less calls are MC_E_STATE (the message says the flags are needed); on
 * one that does not, the new calls ignore the flags and are the old ones.
 *   Fetch: mc_bases_get_reverse copies positions [first, first + count) of the
 * reverse planes to out[6][count]; mc_bases_reverse_device exposes them (plane
 * c at d_rev + c * stride).  mc_bases_set_strand (test hook): sets both plane
 * sets from total[6][count] and rev[6][count]; rev > total anywhere is
 * MC_E_INVALID (checked on the host, nothing is written); sites and consensus
 * results are gone as after mc_bases_set.  (mc_bases_set itself leaves the
 * reverse planes alone.)  All three are MC_E_STATE without tracking.
 *   Sites: mc_bases_sites_strand.  Alleles are A, C, G, T, DEL; depth and the
 * base allele are exactly mc_bases_sites'.  Position p is a site iff
 * depth >= min_depth and some allele i != base has a[i] >= min_count,
 * a[i] * 10^6 >= min_ppm * depth, fwd[i] >= min_alt_strand and
 * rev[i] >= min_alt_strand.  With min_alt_strand == 0 that is mc_bases_sites'
 * predicate and the site list is identical.  A negative min_alt_strand is
 * MC_E_INVALID, a handle without tracking MC_E_STATE.  The result lands in
 * mc_bases_sites' buffers (mc_bases_sites_first and _sites_get read it);
 * mc_bases_sites_get_reverse copies the sites' reverse counts
 * rev_counts[count][6] (MC_E_STATE after a plain mc_bases_sites).
 *   Device side: a second instantiation of the pileup kernel, same 48 KiB of
 * LDS, no global atomics, one owner per tile.  A tile that looks at no more
 * than 65535 reads counts forward in the low and reverse in the high 16 bits
 * of each LDS word (a read covers a position at most once, so neither half
 * can carry) and its flush adds low + high to the total plane and high to the
 * reverse plane; a tile with more reads walks them twice with 32-bit words,
 * the forward reads, a flush, then the reverse reads.
 *   Sources: mc_bases_src_flags gives the flags of the last batch (valid as
 * long as mc_bases_src_batch's arrays); the GPU decoder's bases mode always
 * fills a flag column (mc_bam_gpu_bases_flags, _bases_copy_flags).
 *   Not covered: the strand of insertion alleles, strand in the consensus
 * rule, strand-bias statistics (floating point: host work over these counts).
 *
 * Quality sums (opt-in, as strand is): how good the evidence behind a count
 * is, the sums behind bam-readcount's avg_basequality / avg_mapping_quality and
 * pysamstats' baseq / mapq.  mc_bases_track_quality(h, on): on = 1 / 0 makes
 * the NEXT mc_bases_begin also allocate and zero two plane sets (or not);
 * another value is MC_E_INVALID.  Both are uint32 and indexed exactly like the
 * count planes:
 *   bq[6][N]  the sum of the quality bytes of the bases counted into channel c
 *             at a position.  Only counted bases contribute (those that pass
 *             min_baseq); a read whose qualities are absent (first QUAL byte
 *             0xFF) is counted as without tracking and adds 0; plane
 *             MC_BASES_DEL stays 0 (a deletion has no base).
 *   mq[6][N]  the sum of the MAPQ bytes of the reads counted into channel c,
 *             DEL included.  The byte is summed as it is: 255 is not special.
 * The sums are exact while a channel's count x 255 < 2^32 and wrap modulo 2^32
 * beyond; they are independent of the batch split and repeatable.  The count
 * planes are unchanged by tracking: mc_bases_get, _sites, _consensus and
 * _insertions give the same results with it on as off.  Quality and strand
 * tracking in one pass are out of scope: a begin with both on is MC_E_STATE
 * (the message names both).
 *   Reads: mc_bases_add_batch_mapq / _add_batch_device_mapq take the nine
 * arrays plus mapq[n] (uint8; a device pointer for the device call; a
 * sub-range of a resident table is d_mapq + a); checks and error messages are
 * mc_bases_add_batch's.  On a handle that tracks quality the calls without
 * mapq are MC_E_STATE; on one that does not, the new calls ignore the column.
 *   Fetch: mc_bases_get_quality copies positions [first, first + count) of
 * both sets to bq[6][count] and mq[6][count]; mc_bases_quality_device exposes
 * them (plane c at d_bq + c * stride, d_mq + c * stride).
 * mc_bases_set_quality (test hook): sets the counts and both sum sets from
 * total, bq, mq [6][count]; bq[c] > 255 * total[c], mq[c] > 255 * total[c] or
 * bq[DEL] != 0 anywhere is MC_E_INVALID (checked on the host, nothing is
 * written); results are gone as after mc_bases_set (which leaves the sums
 * alone).  All three are MC_E_STATE without tracking.
 *   Sites: mc_bases_sites_quality.  Depth and the base allele are exactly
 * mc_bases_sites'.  Position p is a site iff depth >= min_depth and some
 * allele i != base has a[i] >= min_count, a[i] * 10^6 >= min_ppm * depth,
 * mq[i] >= min_alt_mapq * a[i] and, for i != DEL, bq[i] >= min_alt_baseq *
 * a[i]; all in 64-bit integers (the mean reaches the threshold, without a
 * division).  Thresholds outside 0..255 are MC_E_INVALID, a handle without
 * tracking MC_E_STATE.  With both thresholds 0 the site list is
 * mc_bases_sites' exactly.  The result lands in mc_bases_sites' buffers;
 * mc_bases_sites_get_quality copies the sites' sums bq[count][6] and
 * mq[count][6] (MC_E_STATE after a plain or a strand sites call).
 *   Device side: a third instantiation of the pileup kernel, no global
 * atomics, one owner per plane element.  One 64-bit LDS add per counted base
 * carries the count (bits 0..15), the quality byte (16..39) and the MAPQ
 * (40..63).  With 8-byte cells a workgroup holds 1024 positions in the same
 * 48 KiB, so a 2048-position tile is two workgroups, each with its half of
 * the tile's aligned window.  A read covers a position at most once, so over
 * at most 65535 reads no field carries (65535 x 255 < 2^24): a workgroup walks
 * its reads in groups of that size and flushes the three fields into the
 * three plane sets after each (mc_bases_quality_dims: 1024, 65535).
 *   Sources: mc_bases_src_mapq gives the MAPQ column of the last batch (valid
 * as long as mc_bases_src_batch's arrays); the GPU decoder's bases mode always
 * fills a mapq column beside its flag column (mc_bam_gpu_bases_mapq,
 * _bases_copy_mapq).
 *   Not covered: quality with strand in one pass, quality in the consensus
 * rule or the insertion table, means or medians (the reader's division),
 * bam-readcount's read-position and mismatch columns. */
#define MC_BASES_A   0
#define MC_BASES_C   1
#define MC_BASES_G   2
#define MC_BASES_T   3
#define MC_BASES_N   4
#define MC_BASES_DEL 5
typedef struct mc_bases mc_bases;
int mc_bases_create(int device, int32_t n_ref, mc_bases** out);
int mc_bases_destroy(mc_bases* h);
int mc_bases_begin(mc_bases* h, int64_t S, const int32_t* tid, const int64_t* start, const int64_t* end,
                   int32_t min_baseq);
int mc_bases_add_batch(mc_bases* h, int64_t n, const int32_t* tid, const int32_t* pos,
                       const int64_t* cig_off /* n + 1 */, const uint32_t* cigar, const int32_t* l_seq,
                       const int64_t* seq_off /* n + 1 */, const uint8_t* seq,
                       const int64_t* qual_off /* n + 1 */, const uint8_t* qual);
/* mc_bases_add_batch with the nine arrays in device memory on the handle's
 * device (e.g. mc_bam_gpu_bases_device's): same reads, same checks, same
 * error classes and messages, same kernels, no copies of the arrays.  The
 * offsets are absolute into the arenas and the arena sizes are explicit
 * (n_words, seq_bytes, qual_bytes), so a sub-range [a, a + n) of a resident
 * read table is d_tid + a, d_pos + a, d_cig_off + a, d_l_seq + a, d_seq_off + a
 * and d_qual_off + a with the arena pointers and sizes unchanged.  The first
 * and last read's (tid, pos) (the tile range, the order check across batches)
 * come back with the pre-pass flags in one 32-byte copy; only for an invalid
 * batch are the bad read's fields and CIGAR words copied back to name it.
 * Returns after its kernels, so the memory may be freed afterwards. */
int mc_bases_add_batch_device(mc_bases* h, int64_t n, const int32_t* d_tid, const int32_t* d_pos,
                              const int64_t* d_cig_off /* n + 1 */, const uint32_t* d_cigar, int64_t n_words,
                              const int32_t* d_l_seq, const int64_t* d_seq_off /* n + 1 */, const uint8_t* d_seq,
                              int64_t seq_bytes, const int64_t* d_qual_off /* n + 1 */, const uint8_t* d_qual,
                              int64_t qual_bytes);
int mc_bases_seg_off(const mc_bases* h, int64_t* seg_off /* S + 1 */);
int mc_bases_get(const mc_bases* h, int64_t first, int64_t count, uint32_t* out /* 6 x count */);
int mc_bases_device(const mc_bases* h, const uint32_t** d_planes, int64_t* stride, int64_t* n);
int mc_bases_sites(mc_bases* h, int64_t min_depth, int64_t min_count, int64_t min_ppm,
                   const uint8_t* ref /* N, or NULL */, int64_t* n_sites);
int mc_bases_sites_first(const mc_bases* h, int64_t* site_first /* S + 1 */);
int mc_bases_sites_get(const mc_bases* h, int64_t first, int64_t count, int64_t* site_pos /* count */,
                       uint32_t* site_counts /* count x 6 */);
int mc_bases_timing(const mc_bases* h, float* prepass_ms, float* pileup_ms, float* sites_ms, int64_t* tiles,
                    int64_t* reads);
int mc_bases_dims(int32_t* tile);
int mc_bases_track_strand(mc_bases* h, int on);
int mc_bases_add_batch_flags(mc_bases* h, int64_t n, const int32_t* tid, const int32_t* pos,
                             const int64_t* cig_off /* n + 1 */, const uint32_t* cigar, const int32_t* l_seq,
                             const int64_t* seq_off /* n + 1 */, const uint8_t* seq,
                             const int64_t* qual_off /* n + 1 */, const uint8_t* qual, const uint16_t* flag /* n */);
int mc_bases_add_batch_device_flags(mc_bases* h, int64_t n, const int32_t* d_tid, const int32_t* d_pos,
                                    const int64_t* d_cig_off /* n + 1 */, const uint32_t* d_cigar, int64_t n_words,
                                    const int32_t* d_l_seq, const int64_t* d_seq_off /* n + 1 */,
                                    const uint8_t* d_seq, int64_t seq_bytes, const int64_t* d_qual_off /* n + 1 */,
                                    const uint8_t* d_qual, int64_t qual_bytes, const uint16_t* d_flag /* n */);
int mc_bases_get_reverse(const mc_bases* h, int64_t first, int64_t count, uint32_t* out /* 6 x count */);
int mc_bases_reverse_device(const mc_bases* h, const uint32_t** d_rev, int64_t* stride, int64_t* n);
int mc_bases_set_strand(mc_bases* h, int64_t first, int64_t count, const uint32_t* total /* 6 x count */,
                        const uint32_t* rev /* 6 x count */);
int mc_bases_sites_strand(mc_bases* h, int64_t min_depth, int64_t min_count, int64_t min_ppm,
                          int64_t min_alt_strand, const uint8_t* ref /* N, or NULL */, int64_t* n_sites);
int mc_bases_sites_get_reverse(const mc_bases* h, int64_t first, int64_t count,
                               uint32_t* rev_counts /* count x 6 */);
int mc_bases_track_quality(mc_bases* h, int on);
int mc_bases_add_batch_mapq(mc_bases* h, int64_t n, const int32_t* tid, const int32_t* pos,
                            const int64_t* cig_off /* n + 1 */, const uint32_t* cigar, const int32_t* l_seq,
                            const int64_t* seq_off /* n + 1 */, const uint8_t* seq,
                            const int64_t* qual_off /* n + 1 */, const uint8_t* qual, const uint8_t* mapq /* n */);
int mc_bases_add_batch_device_mapq(mc_bases* h, int64_t n, const int32_t* d_tid, const int32_t* d_pos,
                                   const int64_t* d_cig_off /* n + 1 */, const uint32_t* d_cigar, int64_t n_words,
                                   const int32_t* d_l_seq, const int64_t* d_seq_off /* n + 1 */,
                                   const uint8_t* d_seq, int64_t seq_bytes, const int64_t* d_qual_off /* n + 1 */,
                                   const uint8_t* d_qual, int64_t qual_bytes, const uint8_t* d_mapq /* n */);
int mc_bases_get_quality(const mc_bases* h, int64_t first, int64_t count, uint32_t* bq /* 6 x count */,
                         uint32_t* mq /* 6 x count */);
int mc_bases_quality_device(const mc_bases* h, const uint32_t** d_bq, const uint32_t** d_mq, int64_t* stride,
                            int64_t* n);
int mc_bases_set_quality(mc_bases* h, int64_t first, int64_t count, const uint32_t* total /* 6 x count */,
                         const uint32_t* bq /* 6 x count */, const uint32_t* mq /* 6 x count */);
int mc_bases_sites_quality(mc_bases* h, int64_t min_depth, int64_t min_count, int64_t min_ppm,
                           int64_t min_alt_baseq, int64_t min_alt_mapq, const uint8_t* ref /* N, or NULL */,
                           int64_t* n_sites);
int mc_bases_sites_get_quality(const mc_bases* h, int64_t first, int64_t count, uint32_t* bq /* count x 6 */,
                               uint32_t* mq /* count x 6 */);
int mc_bases_quality_dims(int32_t* tile /* positions per workgroup */, int32_t* group /* reads per flush */);

/* Consensus (mc_bases_consensus), a third stage over the planes on the device:
 * one letter per position, called from the counts alone.  Without
 * MC_CONS_INS a consensus never contains inserted bases (the planes hold
 * none); with it, see "Insertion alleles" below.  Integer only, exact and
 * deterministic.
 *
 * At plane index i let a[0..3] be the A, C, G, T counts, d the DEL count (the
 * N plane is ignored, as in sites), depth = a0 + a1 + a2 + a3 + d in 64 bits
 * and r the reference code where ref is given (uint8 [N], exactly as
 * mc_bases_sites takes it: 0..3 = A/C/G/T, anything else = unknown).
 * qualifies(x) means x >= max(min_count, 1) and x * 10^6 >= call_ppm * depth,
 * in 64-bit integers.  Every position falls into exactly one class:
 *   LOW     depth < max(min_depth, 1).  Letter N; with MC_CONS_FILL_REF and r
 *           known, the reference base in lower case (acgt).
 *   otherwise top is the first maximum of (A, C, G, T, DEL) in channel order:
 *           a base wins a tie against DEL, a lower channel a tie between bases.
 *   DEL     top is DEL and qualifies(d).  Letter '-' in the aligned output,
 *           nothing in the compact one.  top is DEL and does not qualify:
 *           NOCALL, letter N.
 *   top is a base, without MC_CONS_IUPAC: CALLED with top's letter if it
 *           qualifies, else NOCALL (N).
 *   top is a base, with MC_CONS_IUPAC: Q = the bases b with qualifies(a[b]).
 *           Empty: NOCALL.  One element (it is top, qualifies being monotone in
 *           the count): CALLED.  Two to four: AMBIG with the IUPAC letter of the
 *           set, ".ACMGRSVTWYHKDBN"[mask] with bit A = 1, C = 2, G = 4, T = 8.
 * Two outputs: the aligned sequence has one letter per position (indices are
 * plane indices, segment s owns [seg_off[s], seg_off[s + 1])); the compact
 * sequence is the aligned one without its '-', segment s owning
 * [out_first[s], out_first[s + 1]), *n_out letters in all.  The summary has
 * MC_CONS_COLS int64 per segment: positions, called, ambiguous, nocall, low,
 * deleted, differs, length; differs counts the positions with r known that
 * are DEL, or CALLED with a letter other than the reference's;
 * length = positions - deleted.
 *
 * Errors: before begin, and _first / _summary / _get / _device without a
 * current consensus, MC_E_STATE; negative thresholds, call_ppm > 10^6, unknown
 * flag bits, MC_CONS_FILL_REF with ref == NULL, and a _get range outside the
 * aligned buffer [0, N] (compact == 0) or the compact one [0, n_out],
 * MC_E_INVALID.  Results stay in device memory owned by the handle (buffers
 * only grow; mc_bases_consensus_device exposes both letter buffers) until the
 * next mc_bases_consensus, _add_batch, _set or _begin; they share nothing with
 * the sites buffers, so sites survive a consensus call and the other way
 * round.  mc_bases_consensus_timing: HIP-event times of the last call's three
 * launches.  Device side: a call kernel (one workgroup per tile: planes and
 * ref read once, the letter stored, eight counts per tile by wave reductions
 * and one LDS step), a one-workgroup scan (prefix sums of the eight columns
 * over the tiles; out_first and the summary rows are their differences at the
 * segments' tile ranges) and an emit kernel that compacts the aligned letters
 * (1 B read per position) by ballot ranks.  No global atomics.
 *
 * mc_bases_set (test hook): overwrites plane positions [first, first + count)
 * from in[6][count] (host memory; any counts up to 2^32 - 1, MC_E_INVALID
 * outside [0, N]) and invalidates sites and consensus results. */
#define MC_CONS_IUPAC    1u
#define MC_CONS_FILL_REF 2u
#define MC_CONS_COLS     8
int mc_bases_consensus(mc_bases* h, int64_t min_depth, int64_t min_count, int64_t call_ppm, uint32_t flags,
                       const uint8_t* ref /* N, or NULL */, int64_t* n_out /* compact letters in all */);
int mc_bases_consensus_first(const mc_bases* h, int64_t* out_first /* S + 1 */);
int mc_bases_consensus_summary(const mc_bases* h, int64_t* rows /* S x 8 */);
int mc_bases_consensus_get(const mc_bases* h, int compact, int64_t first, int64_t count, uint8_t* letters);
int mc_bases_consensus_device(const mc_bases* h, const uint8_t** d_aligned, const uint8_t** d_compact);
int mc_bases_consensus_timing(const mc_bases* h, float* call_ms, float* scan_ms, float* emit_ms);
int mc_bases_set(mc_bases* h, int64_t first, int64_t count, const uint32_t* in /* 6 x count */);

/* Diversity (mc_bases_diversity), a further stage over the planes on the
 * device: per window the sums a metagenome user derives breadth, mean base
 * depth, SNV density, nucleotide diversity and the identity to the reference
 * from (inStrain's conANI and popANI).  MC_DIV_COLS int64 per window, all
 * integer, exact and independent of order.
 *
 * Windows are mc_windows_compute's, over the handle's segments: segment s of
 * length L = seg_off[s + 1] - seg_off[s] is cut into the windows [k * window,
 * min((k + 1) * window, L)) of its plane indices; window == 0 is one window
 * per non-empty segment; an empty segment owns none.  Segment s owns rows
 * [win_first[s], win_first[s + 1]) (mc_bases_diversity_first, arithmetic);
 * *n_windows = win_first[S] (more than 2^31: MC_E_RANGE).  window is 0 or at
 * least MC_DIV_MIN_WINDOW, else MC_E_INVALID.
 *
 * At plane index i let a[0..3] be the A, C, G, T counts and n = a0 + a1 + a2 +
 * a3 in 64 bits (DEL and N are ignored: a deletion is not a base), r = ref[i]
 * as mc_bases_sites takes it (0..3 = A/C/G/T; anything else, or ref == NULL,
 * unknown), md = max(min_depth, 2), mc = max(min_count, 1), qualifies(x) =
 * x >= mc and x * 10^6 >= min_ppm * n in 64-bit integers, major the first
 * maximum of a in channel order, minor the largest of the other three counts.
 * A position is covered iff n >= md.  The columns:
 *   0 positions  the window's length
 *   1 covered    covered positions
 *   2 bases      sum of n over ALL the window's positions
 *   3 snv        covered positions with qualifies(minor)
 *   4 pi_fix     sum over the covered positions of q, below
 *   5 compared   covered positions with r known
 *   6 con_diff   of those, major != r
 *   7 pop_diff   of those, major != r and not qualifies(a[r])
 * so that pi = pi_fix / 2^32 / covered, conANI = 1 - con_diff / compared and
 * popANI = 1 - pop_diff / compared.  q is the unbiased pairwise estimator (Nei
 * and Li) in 32.32 fixed point: num = n^2 - sum a_c^2, den = n (n - 1), both
 * exact in uint64, q = llrint((double)num / (double)den * 2^32): one IEEE
 * double division, round half to even; q = 0 where num == 0.  Both
 * conversions are exact while n < 2^26, and q <= 2^32.  A covered position
 * with n >= 2^26 fails the call with MC_E_RANGE (mc_last_error names the
 * lowest such plane index) and no result becomes current.
 *
 * Errors: before begin, and _first / _get / _device / _timing without a
 * current result, MC_E_STATE; negative thresholds, min_ppm > 10^6, window in
 * 1..15 and a _get range outside [0, n_windows], MC_E_INVALID.  The rows stay
 * in device memory owned by the handle (buffers only grow;
 * mc_bases_diversity_device exposes them) until the next mc_bases_diversity,
 * _add_batch, _set, _ins_set or _begin; they share nothing with the sites,
 * consensus or insertion buffers, so those results survive a diversity call
 * and the other way round.  Strand, quality and insertion tracking do not
 * change a row.  Device side (csrc/bases_div.h): one workgroup per tile sums
 * the columns per window in LDS (wave reductions where a wave's positions lie
 * in one or two windows, LDS adds otherwise); the rows of windows inside a
 * tile are stored, the first and the last window of a tile, which neighbours
 * may share, are zeroed by a launch in front (combine_ms of
 * mc_bases_diversity_timing; tile_ms is the tile kernel's) and added with
 * 64-bit integer atomics.  No floating-point atomics. */
#define MC_DIV_COLS 8
#define MC_DIV_MIN_WINDOW 16
int mc_bases_diversity(mc_bases* h, int64_t window, int64_t min_depth, int64_t min_count, int64_t min_ppm,
                       const uint8_t* ref /* N, or NULL */, int64_t* n_windows);
int mc_bases_diversity_first(const mc_bases* h, int64_t* win_first /* S + 1 */);
int mc_bases_diversity_get(const mc_bases* h, int64_t first, int64_t count, int64_t* rows /* count x 8 */);
int mc_bases_diversity_device(const mc_bases* h, const int64_t** d_rows, int64_t* n_windows);
int mc_bases_diversity_timing(const mc_bases* h, float* tile_ms, float* combine_ms);

/* Comparison (mc_bases_compare), a further stage over the planes of TWO
 * handles on the device: per window the sums a metagenome user derives the
 * identity of two samples' populations from (inStrain compare's conANI and
 * popANI between samples) and the mean distance of their allele frequencies.
 * MC_CMP_COLS int64 per window, all integer, exact and independent of order.
 *
 * Handles: a and b, on one device, both begun on the same segments: the same
 * S and per segment the same tid, start and end, else MC_E_INVALID
 * (mc_last_error names the first differing segment).  Their tile tables and
 * plane layouts are then the same, mc_bases_begin's cut depending on the
 * segments only.  a == b is allowed: con_diff = pop_diff = dist_fix = 0 and
 * compared = covered_a = covered_b.
 *
 * Windows are Diversity's: window == 0 or at least MC_DIV_MIN_WINDOW, segment
 * s owns rows [win_first[s], win_first[s + 1]) (mc_bases_compare_first),
 * *n_windows = win_first[S] (more than 2^31: MC_E_RANGE).
 *
 * At plane index i, for sample x in {a, b}, let x[0..3] be its A, C, G, T
 * counts and n_x their sum in 64 bits (DEL and N are ignored, as in
 * Diversity), md = max(min_depth, 2), mc = max(min_count, 1),
 * qualifies_x(v) = v >= mc and v * 10^6 >= min_ppm * n_x (each sample against
 * its own depth), major_x the first maximum of x in channel order, minor_x
 * the largest of the other three counts, covered_x = n_x >= md, present_x(c)
 * = c == major_x or qualifies_x(x[c]).  The columns:
 *   0 positions  the window's length
 *   1 covered_a  positions with covered_a
 *   2 covered_b  positions with covered_b
 *   3 compared   positions covered in both
 *   4 con_diff   compared and major_a != major_b
 *   5 pop_diff   compared and no channel c has present_a(c) and present_b(c):
 *                the samples share no allele (this implies con_diff)
 *   6 snv        compared and (qualifies_a(minor_a) or qualifies_b(minor_b))
 *   7 dist_fix   sum over the compared positions of q, below
 * so that conANI = 1 - con_diff / compared, popANI = 1 - pop_diff / compared
 * and the mean allele-frequency distance = dist_fix / 2^32 / compared.  q is
 * the total-variation distance of the two allele-frequency vectors in 32.32
 * fixed point: num = sum over c of |a[c] * n_b - b[c] * n_a|, den = 2 * n_a *
 * n_b, q = llrint((double)num / (double)den * 2^32): one IEEE double
 * division, round half to even; q = 0 where num == 0.  With n_a, n_b < 2^26
 * every product is below 2^52 and num <= den < 2^53, so both conversions are
 * exact, and q <= 2^32.  A compared position with n_a or n_b of 2^26 or more
 * fails the call with MC_E_RANGE (mc_last_error names the lowest such plane
 * index) and no result becomes current; a position that is not compared never
 * raises it.  Swapping the handles swaps columns 1 and 2 and changes nothing
 * else.
 *
 * The result belongs to a: its rows stay in device memory owned by a (buffers
 * of its own that only grow; mc_bases_compare_device exposes them), on a's
 * stream, until the next mc_bases_compare on a, or a's _add_batch, _set,
 * _ins_set or _begin.  b is only read; the call waits for b's stream before
 * it launches.  The sites, consensus, insertion and diversity results of
 * either handle survive a compare, and the other way round; strand, quality
 * and insertion tracking on either handle do not change a row.
 *
 * Errors: either handle before begin, and _first / _get / _device / _timing
 * without a current result, MC_E_STATE; a null handle, handles on different
 * devices, differing segments, negative thresholds, min_ppm > 10^6, window in
 * 1..15 and a _get range outside [0, n_windows], MC_E_INVALID.  Device side
 * (csrc/bases_cmp.h): Diversity's shape, one workgroup per tile reading both
 * handles' A, C, G, T planes; zero_ms of mc_bases_compare_timing is the launch
 * that zeroes the rows tiles share, tile_ms the tile kernel's.  No
 * floating-point atomics. */
#define MC_CMP_COLS 8
int mc_bases_compare(mc_bases* a, const mc_bases* b, int64_t window, int64_t min_depth, int64_t min_count,
                     int64_t min_ppm, int64_t* n_windows);
int mc_bases_compare_first(const mc_bases* a, int64_t* win_first /* S + 1 */);
int mc_bases_compare_get(const mc_bases* a, int64_t first, int64_t count, int64_t* rows /* count x 8 */);
int mc_bases_compare_device(const mc_bases* a, const int64_t** d_rows, int64_t* n_windows);
int mc_bases_compare_timing(const mc_bases* a, float* tile_ms, float* zero_ms);

/* Insertion alleles (csrc/bases_ins.h), an opt-in stage of mc_bases, off by
 * default: with it off no launch, byte or error of the calls above changes.
 * The reference has nothing here; the contract is this library's own.
 *
 * The walk is the one above: from rpos = pos, qpos = 0.  An I op of length
 * L >= 1 met at reference cursor rpos > pos (M, =, X, D or N ops of at least
 * one reference position in all precede it in the read) is an EVENT at anchor
 * p = rpos - 1, the reference base before the inserted bases (the mpileup and
 * VCF convention).  A leading insertion (rpos == pos: only S, H, P or I before
 * it) is ignored, as mpileup ignores it, so every anchor lies in
 * [pos, pos + span) and the pileup's tile search finds every contributing
 * read.  A trailing I counts; two I ops of one read at one anchor are two
 * events; no quality test applies (as for DEL: min_baseq does not touch
 * insertions).  The event's allele is (len, code): if L <= 32 and all L query
 * bases qpos .. qpos + L have nt16 codes 1, 2, 4 or 8, len = L and code =
 * sum of b_j * 4^(L - 1 - j) with A, C, G, T = 0..3 (numeric order of equal
 * lengths is lexicographic order).  Otherwise (longer, or an ambiguity code
 * inside) the event is OTHER: len = 0, code = 0, other = 1; OTHER events are
 * counted and never called.  An event belongs to every plane index i whose
 * segment holds p (overlapping and duplicated segments each get it, as the
 * planes do); an anchor outside every segment adds nothing.
 *
 * The allele table is the multiset of events, grouped: rows (i int64, len
 * int32, code uint64, other uint8, count uint32), sorted by (i, other, len,
 * code) and unique, so a segment's rows are contiguous and a position's OTHER
 * row is its last.  It is a function of the set of reads alone: the same
 * reads in any split into batches give identical bytes.  At most 2^31 - 1
 * events per begin (MC_E_RANGE).
 *
 * mc_bases_track_insertions(h, on): on = 1 / 0 makes the NEXT mc_bases_begin
 * (and those after it) track or not; NULL handle or another value of on is
 * MC_E_INVALID.  mc_bases_begin clears the events.  On a handle whose current
 * begin does not track, every call below is MC_E_STATE (before the first begin
 * too); mc_bases_consensus with MC_CONS_INS is MC_E_INVALID there, the answer
 * to that flag bit since before it had a meaning.
 * mc_bases_insertions groups the events and keeps the rows with
 * depth(i) = A + C + G + T + DEL at i (64 bits), depth >= min_depth, count >=
 * min_count and count * 10^6 >= min_ppm * depth, the sites predicate:
 * (0, 1, 0) keeps every row.  Negative thresholds or min_ppm > 10^6:
 * MC_E_INVALID.  Segment s owns rows [first[s], first[s + 1])
 * (mc_bases_insertions_first); mc_bases_insertions_get copies rows [first,
 * first + count) (MC_E_INVALID outside [0, *n_rows] or with a NULL array for
 * count > 0; both MC_E_STATE without a current table: it is gone after the
 * next mc_bases_add_batch, _set, _ins_set or _begin).
 * mc_bases_insertions_timing: HIP-event times of the extract launches since
 * begin, of the last mc_bases_insertions and of the insertion part of the
 * last consensus, and the events held.
 * mc_bases_ins_set (test hook, as mc_bases_set): installs a grouped table of n
 * rows in place of the events; MC_E_INVALID unless the rows are sorted by
 * (i, other, len, code) and unique, 0 <= i < N, other is 0 (1 <= len <= 32,
 * code < 4^len) or 1 (len = 0, code = 0) and count >= 1.  Until the next
 * begin mc_bases_add_batch and _add_batch_device are then MC_E_STATE.
 *
 * MC_CONS_INS for mc_bases_consensus: at each plane index i whose class is not
 * LOW the TOP allele is the row that is not OTHER with the highest count
 * (ties: the shorter len, then the smaller code).  If it qualifies
 * (qualifies(count) of "Consensus", with depth(i)), its len letters, upper
 * case, follow position i's letter in the COMPACT output; where i was called
 * DEL they stand where that letter would have been.  One insertion per anchor
 * at most.  The aligned buffer is unchanged (one letter per position).  With
 * the flag, out_first, *n_out and the summary's length become positions -
 * deleted + inserted, and mc_bases_consensus_ins returns per segment the
 * insertions called and the bases inserted (MC_E_STATE unless the current
 * consensus was made with the flag).  Without the flag every output is byte
 * for byte what it was, on tracking handles too.
 *
 * Device side: per batch an extract (one workgroup per tile of the pileup
 * launch's range, one thread per read, CIGAR words only; count pass, scan,
 * fill pass appending 24-byte events, query bases loaded only inside I ops);
 * at mc_bases_insertions a scatter into per-tile buckets, one workgroup per
 * bucket sorting it (bitonic, in LDS up to 4096 events, else over global
 * memory with LDS for the short strides) and a run-length encode with the
 * threshold predicate (count pass, scan, emit pass). */
#define MC_CONS_INS      4u
int mc_bases_track_insertions(mc_bases* h, int on);
int mc_bases_insertions(mc_bases* h, int64_t min_depth, int64_t min_count, int64_t min_ppm, int64_t* n_rows);
int mc_bases_insertions_first(const mc_bases* h, int64_t* first /* S + 1 */);
int mc_bases_insertions_get(const mc_bases* h, int64_t first, int64_t count, int64_t* i, int32_t* len,
                            uint64_t* code, uint8_t* other, uint32_t* cnt);
int mc_bases_insertions_timing(const mc_bases* h, float* extract_ms, float* group_ms, float* cons_ms,
                               int64_t* events);
int mc_bases_ins_set(mc_bases* h, int64_t n, const int64_t* i, const int32_t* len, const uint64_t* code,
                     const uint8_t* other, const uint32_t* cnt);
int mc_bases_consensus_ins(const mc_bases* h, int64_t* rows /* S x 2 */);
/* (test hook) the events one workgroup sorts in LDS, and the longest callable insertion */
int mc_bases_ins_dims(int32_t* sort_chunk, int32_t* max_len);

typedef struct mc_bases_src mc_bases_src;
int mc_bases_src_open(const char* path, int n_threads, uint32_t flag_filter, int min_mapq, mc_bases_src** out);
int mc_bases_src_close(mc_bases_src* s);
int mc_bases_src_n_targets(const mc_bases_src* s, int32_t* n);
int mc_bases_src_target(const mc_bases_src* s, int32_t i, const char** name, int64_t* length);
int mc_bases_src_next(mc_bases_src* s, int64_t max_reads, int64_t max_bases, int64_t* n);
int mc_bases_src_batch(const mc_bases_src* s, const int32_t** tid, const int32_t** pos, const int64_t** cig_off,
                       const uint32_t** cigar, const int32_t** l_seq, const int64_t** seq_off,
                       const uint8_t** seq, const int64_t** qual_off, const uint8_t** qual);
int mc_bases_src_flags(const mc_bases_src* s, const uint16_t** flag /* n of the last batch */);
int mc_bases_src_mapq(const mc_bases_src* s, const uint8_t** mapq /* n of the last batch */);
int mc_bases_src_counts(const mc_bases_src* s, int64_t* records, int64_t* kept, int64_t* no_seq,
                        int64_t* bad_cigar);

/* ---- htslib's pileup read cap (opt-in) -----------------------------------
 * pysam's AlignmentFile.pileup(ref, start, end) (pileup.py:13) runs htslib's
 * pileup with max_depth = 8000: bam_plp_push drops a read that starts where
 * its predecessor started while the pileup's read pool holds more than
 * max_depth nodes.  keep[i] = 0 for the reads it would drop, given the
 * coordinate-sorted reads one pileup call sees (for classic(): the region's
 * overlapping records).  Host C++ (contigs on n_threads threads); the depth
 * of the kept reads is then computed as usual.  Version-dependent htslib
 * behaviour: parity unpinned (no htslib in this image); the closed form is
 * pinned by a literal restatement of the push/next loop (oracle/htslib_plp.py). */
int mc_depth_cap_mask(int64_t n, const int32_t* tid, const int32_t* pos, const int32_t* span,
                      int32_t max_depth, int n_threads, uint8_t* keep, int64_t* n_dropped);

/* The same mask on the device (csrc/capmask.h: one wave per query walks its
 * start groups in order; a chunk of 64 reads that cannot reach the cap is
 * applied in bulk).  d_*: device arrays; each distinct tid is one query.
 * MC_E_INVALID for unsorted reads, MC_E_RANGE for a span >= 32704 (the
 * wave's LDS ring of read ends; mc_depth_cap_mask takes those). */
int mc_depth_cap_mask_device(int device, int64_t n, const int32_t* d_tid, const int32_t* d_pos,
                             const int32_t* d_span, int32_t max_depth, uint8_t* d_keep,
                             int64_t* n_dropped);

/* The capped recompute's batch, built on the device (metacov_amd.depthcap):
 * from coordinate-sorted device intervals (e.g. mc_bam_gpu_intervals_device),
 * region r's query — the reads of contig qtid[r] overlapping [qstart[r],
 * qend[r]) by bam_endpos, what pysam's pileup(ref, start, end) hands htslib
 * (pileup.py:13) — with the cap applied, becomes contig r of the ctx's
 * batch.  The ctx must hold R contigs (mc_set_contigs: the regions' contig
 * lengths) and no reads.  Dropped reads (and reads of the gathered range
 * outside the query) stay in the batch with span 0, so they add no depth.
 * n_dropped: reads the cap dropped.  MC_E_RANGE for a span >= 32704. */
int mc_add_reads_capped(mc_ctx* ctx, int64_t n, const int32_t* d_tid, const int32_t* d_pos,
                        const int32_t* d_span, int64_t R, const int32_t* qtid, const int64_t* qstart,
                        const int64_t* qend, int32_t max_depth, int64_t* n_dropped);

/* ---- host BAM decoder (C++, multi-threaded BGZF inflate) ----------------
 * Replaces the pysam/htslib read path the reference uses: AlignmentFile
 * header (bam.references / bam.lengths, cli.py:80, util.py:64-69),
 * IteratorRowAll over records (scan.pyx:204), and bam_plp_push's pileup
 * interval [pos, pos + bam_cigar2rlen) (MC_LEGACY_ENDPOS: bam_endpos). */
typedef struct mc_bam mc_bam;

/* OR'd into any decoder's flag_filter (bits 0-15 are BAM flags): the pileup
 * interval of a mapped read with no reference-consuming CIGAR op is
 * [pos, pos + 1), as htslib <= 1.9 bam_plp_push set it (tail->end =
 * bam_endpos(b)).  Default (bit clear): current htslib, whose bam_plp_push
 * sets tail->end = pos + bam_cigar2rlen(...) ("raw rlen rather than
 * bam_endpos() which adjusts rlen=0 to rlen=1"), so such a read has span 0
 * and adds nothing to PileupColumn.n.  Version-dependent; parity unpinned. */
#define MC_LEGACY_ENDPOS 0x10000u

int mc_bam_open(const char* path, int n_threads, uint32_t flag_filter,
                int keep_cigar, mc_bam** out);
int mc_bam_close(mc_bam* bam);
int mc_bam_n_targets(const mc_bam* bam, int32_t* n);
int mc_bam_target(const mc_bam* bam, int32_t i, const char** name, int64_t* length);
/* records in the file / records kept by the flag filter (and tid >= 0) */
int mc_bam_counts(const mc_bam* bam, int64_t* n_records, int64_t* n_kept,
                  int64_t* n_mapped, int64_t* n_unmapped);
int mc_bam_intervals(const mc_bam* bam, int32_t* tid, int32_t* pos, int32_t* span);
/* keep_cigar only: total CIGAR words, then offsets (n_kept + 1) and words */
int mc_bam_n_cigar_words(const mc_bam* bam, int64_t* n);
int mc_bam_cigars(const mc_bam* bam, int64_t* cig_off, uint32_t* cigar);

/* ---- streaming decode -----------------------------------------------------
 * Bounded-memory variant of mc_bam_open for BAMs larger than host memory:
 * BGZF blocks are inflated a window (window_bytes inflated, 0 = 256 MiB) at
 * a time on n_threads threads and the kept records' intervals come out in
 * order, up to `cap` per mc_bam_stream_next call (*n_out = 0 at the end).
 * mc_bam_stream_header exposes the header and the running record counts
 * through the mc_bam accessors (mc_bam_n_targets, mc_bam_target,
 * mc_bam_counts); the handle stays owned by the stream. */
typedef struct mc_bam_stream mc_bam_stream;
int mc_bam_stream_open(const char* path, int n_threads, uint32_t flag_filter,
                       int64_t window_bytes, mc_bam_stream** out);
int mc_bam_stream_next(mc_bam_stream* s, int64_t cap, int32_t* tid, int32_t* pos,
                       int32_t* span, int64_t* n_out);
int mc_bam_stream_header(const mc_bam_stream* s, const mc_bam** header);
int mc_bam_stream_close(mc_bam_stream* s);

/* ---- BAI index ------------------------------------------------------------
 * The reference opens an indexed BAM (`metacov pileup` needs `samtools
 * index`: pysam AlignmentFile.pileup(ref, start, end) at pileup.py:13 is an
 * indexed query; AlignmentFile.mapped / .unmapped at cli.py:58-66 read the
 * index pseudo-bins).  mc_bam_index_build writes <bam>.bai (bai_path NULL)
 * the way htslib's hts_idx_push / hts_idx_finish do.  mc_bam_open_contigs
 * decodes only the records of the chosen contigs (one rank's shard) through
 * the index: same intervals as mc_bam_open restricted to those tids (global
 * tid values), whole-file mapped / unmapped counts from the index.
 * mc_bam_index_stats: per-reference mapped / unmapped counts and the records
 * without coordinates (sharding costs without a decode). */
int mc_bam_index_build(const char* bam_path, const char* bai_path, int n_threads);
int mc_bam_index_stats(const char* bai_path, int32_t n_ref, int64_t* n_mapped,
                       int64_t* n_unmapped, int64_t* n_no_coor);
int mc_bam_open_contigs(const char* path, const char* bai_path, int n_threads,
                        uint32_t flag_filter, int keep_cigar, int32_t n_sel,
                        const int32_t* sel, mc_bam** out);
/* Where each contig's records lie in a coordinate-sorted BAM: what a BAI's
 * per-reference pseudo-bin holds (htslib hts_idx_finish, bin 37450).
 * beg_voff / end_voff are the virtual offsets (bgzf_tell: compressed block
 * offset << 16 | offset inside the inflated block) of the contig's first
 * record and of the end of its last one; equal when it has no records.
 * n_kept: records kept under a decode's flag filter (mc_bam_gpu_extents;
 * 0 when read from an index). */
typedef struct mc_contig_extent {
    int64_t beg_voff;
    int64_t end_voff;
    int64_t n_mapped;     /* records of this tid without flag 0x4 */
    int64_t n_unmapped;   /* records of this tid with flag 0x4 */
    int64_t n_kept;
} mc_contig_extent;
/* The extents table of an index (the role of pysam's indexed
 * AlignmentFile.fetch(ref) at metacov/pileup.py:13 / :90: which bytes hold a
 * contig's reads); *n_no_coor: records without coordinates. */
int mc_bam_index_extents(const char* bai_path, int32_t n_ref, mc_contig_extent* ext,
                         int64_t* n_no_coor);

/* ---- GPU BAM decode ------------------------------------------------------
 * The records mc_bam_open keeps (same intervals in file order, same record /
 * mapped / unmapped counts, same error classes), decoded on `device`: the
 * host reads the file (n_threads pread threads into pinned staging, 0 = 16)
 * and scans the BGZF block headers; one GPU lane inflates each BGZF block,
 * and the BAM records are found and parsed per 64 KiB segment of the
 * inflated stream (csrc/bam_gpu.hip).  window_bytes: inflated bytes per
 * window (0 = 4 GiB); a record cut by a window is carried to the next.
 * The kept intervals stay in device memory owned by the handle
 * (mc_bam_gpu_intervals_device: valid until mc_bam_gpu_close; hand them to
 * mc_add_reads_device); so do the decode's window buffers (about 2.5 x the
 * window size) until mc_bam_gpu_close.  Replaces, like mc_bam_open, the record walk under
 * pysam's pileup (IteratorRowAll, scan.pyx:204-216). */
typedef struct mc_bam_gpu mc_bam_gpu;
typedef struct mc_bam_gpu_timings {
    double read_ms;      /* host: file read + upload of the compressed windows */
    double inflate_ms;   /* gz_inflate_kernel (HIP events) */
    double parse_ms;     /* record sync / walk / fill, with their host checks */
    double total_ms;     /* the whole mc_bam_gpu_open */
    int64_t windows;
    int64_t blocks;
    int64_t resyncs;     /* segment starts corrected after a walk (sync false positives) */
    int64_t compressed_bytes;
    int64_t inflated_bytes;
    double scan_ms;      /* host: BGZF block header scan */
    double upload_ms;    /* host: every file read + upload, overlapped or not */
    double kernel_ms;    /* gz_inflate_kernel launches (HIP events), summed over launches */
    double open_ms;      /* the decode inside mc_bam_gpu_open, teardown of its file mapping included */
    int64_t parse_rounds;   /* most walk / check rounds of any parsed window (1: no false sync) */
    int64_t resync_passes;  /* re-syncs with the long chain after repeated false syncs */
} mc_bam_gpu_timings;
int mc_bam_gpu_open(const char* path, int device, int n_threads, uint32_t flag_filter,
                    int64_t window_bytes, mc_bam_gpu** out);
int mc_bam_gpu_header(const mc_bam_gpu* g, const mc_bam** header);
int mc_bam_gpu_intervals_device(const mc_bam_gpu* g, int64_t* n, const int32_t** d_tid,
                                const int32_t** d_pos, const int32_t** d_span);
int mc_bam_gpu_intervals(const mc_bam_gpu* g, int32_t* tid, int32_t* pos, int32_t* span);
int mc_bam_gpu_stats(const mc_bam_gpu* g, mc_bam_gpu_timings* t);
int mc_bam_gpu_close(mc_bam_gpu* g);
/* Releases the decode's staging buffers (compressed bytes, inflated stream,
 * block and segment tables) of an open handle; its results (intervals, read
 * table or scan columns, the per-contig extents) stay valid.  For handles
 * kept between calls (metacov_amd.pileup's path cache).  freed (optional):
 * device bytes released. */
int mc_bam_gpu_trim(mc_bam_gpu* g, int64_t* freed);
/* `metacov scan` input decoded on the GPU (the BAM half of scan.pyx:188-216,
 * IteratorRowAll: every record in file order; replaces mc_scan_src_open_bam's
 * host walk): the whole file as the SoA batch mc_scan_add_batch_device takes
 * (rlen = l_seq, flag, gpos = pos [+ l_seq on the reverse strand], gisize =
 * tlen when properly paired else 0, tid, packed nt16 bases at 4-byte aligned
 * offsets seq_off[0..n]), left in device memory owned by the handle. */
int mc_bam_gpu_open_scan(const char* path, int device, int n_threads, int64_t window_bytes, mc_bam_gpu** out);
int mc_bam_gpu_scan_device(const mc_bam_gpu* g, int64_t* n, const int32_t** d_rlen, const int32_t** d_flag,
                           const int32_t** d_gpos, const int32_t** d_gisize, const int32_t** d_tid,
                           const int64_t** d_seq_off, const uint8_t** d_seq, int64_t* seq_bytes);
/* pileup.experimental's read table decoded on the GPU (the device form of
 * mc_reads_open's walk, exp_reads.cpp; replaces bam.fetch at
 * metacov/pileup.py:101): every placed record (tid >= 0) in file order, with
 * tid, pos, end (pos + reference length; pos + 1 when unmapped or 0), flag,
 * bits (1 no SEQ, 2 no reference length), the 2-bit code of the first k_len
 * bases of query_alignment_sequence (0xFFFFFFFF: none) and the query name
 * (name_len bytes at name_off in the names arena), left in device memory owned
 * by the handle.  mc_bam_gpu_reads_copy copies them to caller buffers of
 * n entries (names: name_bytes). */
int mc_bam_gpu_open_reads(const char* path, int device, int n_threads, int k_len, int64_t window_bytes,
                          mc_bam_gpu** out);
int mc_bam_gpu_reads_device(const mc_bam_gpu* g, int64_t* n, const int32_t** d_tid, const int32_t** d_pos,
                            const int64_t** d_end, const int32_t** d_flag, const uint8_t** d_bits,
                            const uint32_t** d_kmer, const uint8_t** d_name_len, const int64_t** d_name_off,
                            const uint8_t** d_names, int64_t* name_bytes);
int mc_bam_gpu_reads_copy(const mc_bam_gpu* g, int32_t* tid, int32_t* pos, int64_t* end, int32_t* flag,
                          uint8_t* bits, uint32_t* kmer, uint8_t* name_len, int64_t* name_off, uint8_t* names);
/* The base counter's input decoded on the GPU (the device form of
 * mc_bases_src_*: same kept set, same skips, same counts, same layout).  The
 * whole file is decoded, windowed as the other modes; the records
 * mc_bases_src_next would hand out stay in device memory owned by the handle,
 * in file order, as one read table in mc_bases_add_batch's layout: tid, pos
 * and l_seq [n], cig_off, seq_off and qual_off [n + 1] (absolute offsets, the
 * last one the arena's size), and three arenas: CIGAR words (the CG:B,I words
 * where the record carries the tag), nt16 bytes (every read starts on a 4-byte
 * boundary, zero fill) and quality bytes (packed).  mc_bam_gpu_bases_device
 * gives the device pointers, n and the arena sizes (valid until
 * mc_bam_gpu_close; hand them, or a sub-range of the reads, to
 * mc_bases_add_batch_device); mc_bam_gpu_bases_copy copies the table to host
 * buffers of those sizes (tests, debugging); mc_bam_gpu_bases_counts gives
 * mc_bases_src_counts' four numbers.  The sort order is not checked here (the
 * base counter's pre-pass checks it); a record that is malformed for
 * mc_bases_src_next is MC_E_IO.  Device work: a count and a fill walk with one
 * lane per 64 KiB segment (the fill writes the columns, the offsets and each
 * read's source offsets), then a gather kernel that copies CIGAR, SEQ and QUAL
 * with 16 lanes per read.  If the table outgrows device memory the open fails
 * with MC_E_HIP and says so.  mc_bam_gpu_header, _stats, _trim and _close work
 * as for the other modes; the other modes' accessors (intervals, scan, reads,
 * extents, restrict) are MC_E_STATE on such a handle, and these three are
 * MC_E_STATE on any other.  Whole files only (no contig subset, no extents). */
int mc_bam_gpu_open_bases(const char* path, int device, int n_threads, uint32_t flag_filter, int min_mapq,
                          int64_t window_bytes, mc_bam_gpu** out);
int mc_bam_gpu_bases_device(const mc_bam_gpu* g, int64_t* n, const int32_t** d_tid, const int32_t** d_pos,
                            const int64_t** d_cig_off, const uint32_t** d_cigar, int64_t* n_words,
                            const int32_t** d_l_seq, const int64_t** d_seq_off, const uint8_t** d_seq,
                            int64_t* seq_bytes, const int64_t** d_qual_off, const uint8_t** d_qual,
                            int64_t* qual_bytes);
int mc_bam_gpu_bases_copy(const mc_bam_gpu* g, int32_t* tid, int32_t* pos, int64_t* cig_off /* n + 1 */,
                          uint32_t* cigar, int32_t* l_seq, int64_t* seq_off /* n + 1 */, uint8_t* seq,
                          int64_t* qual_off /* n + 1 */, uint8_t* qual);
/* The flag column of the bases-mode read table (2 bytes per read, written by
 * the fill walk beside tid / pos / l_seq): the device pointer (a sub-range
 * [a, a + n) is *d_flag + a), or a copy to flag[n] on the host. */
int mc_bam_gpu_bases_flags(const mc_bam_gpu* g, const uint16_t** d_flag);
int mc_bam_gpu_bases_copy_flags(const mc_bam_gpu* g, uint16_t* flag /* n */);
/* The mapq column beside it (1 byte per read, record byte 9 as it is). */
int mc_bam_gpu_bases_mapq(const mc_bam_gpu* g, const uint8_t** d_mapq);
int mc_bam_gpu_bases_copy_mapq(const mc_bam_gpu* g, uint8_t* mapq /* n */);
int mc_bam_gpu_bases_counts(const mc_bam_gpu* g, int64_t* records, int64_t* kept, int64_t* no_seq,
                            int64_t* bad_cigar);
/* The same for one rank's contigs (mc_bam_gpu_open_extents' blocks and
 * extents table: only the selected contigs' BGZF blocks are read and
 * inflated); tids stay the header's.  The header counts are the table's. */
int mc_bam_gpu_open_reads_extents(const char* path, int device, int n_threads, int k_len, int32_t n_ref,
                                  const mc_contig_extent* ext, int64_t n_no_coor, int32_t n_sel, const int32_t* sel,
                                  mc_bam_gpu** out);
/* One rank's contig shard decoded on the GPU ("each rank
 * decodes only its contigs' BGZF chunks, located via BAI virtual offsets";
 * replaces the per-contig indexed query under pysam's pileup(ref, start,
 * end), metacov/pileup.py:13).  Only the BGZF blocks holding the selected
 * contigs' records are read, uploaded and inflated; the kept records are
 * those mc_bam_open keeps of those contigs, in file order.  Their device
 * tids are LOCAL ids (the rank of the header tid in the sorted, de-duplicated
 * selection: the contig ids of a ctx holding just those contigs), in
 * mc_bam_gpu_intervals_device as in mc_bam_gpu_intervals[_range].  The
 * header counts are the whole file's, from the extents (as an index reports
 * them).  mc_bam_gpu_open_contigs reads the extents from the BAI (bai_path
 * NULL: <path>.bai); mc_bam_gpu_open_extents takes them from the caller
 * (e.g. mc_bam_gpu_extents of a whole-file decode on another rank, for a BAM
 * without an index). */
int mc_bam_gpu_open_contigs(const char* path, const char* bai_path, int device, int n_threads,
                            uint32_t flag_filter, int32_t n_sel, const int32_t* sel,
                            mc_bam_gpu** out);
int mc_bam_gpu_open_extents(const char* path, int device, int n_threads, uint32_t flag_filter,
                            int32_t n_ref, const mc_contig_extent* ext, int64_t n_no_coor,
                            int32_t n_sel, const int32_t* sel, mc_bam_gpu** out);
/* The extents table of a decoded file, computed on the device during the
 * record walk (per contig: first record, end of the last record, mapped /
 * unmapped / kept counts).  For a whole-file handle it is the BAI's
 * pseudo-bin data; MC_E_INVALID if the records of a contig are not
 * contiguous (the file is not coordinate-sorted).  A contig-subset handle
 * returns the table it was opened with, with n_kept filled in for its
 * contigs. */
int mc_bam_gpu_extents(const mc_bam_gpu* g, int32_t n_ref, mc_contig_extent* ext,
                       int64_t* n_no_coor);
/* A whole-file handle turned into a contig-subset one in place: only the
 * kept intervals of the selected contigs remain, in file order, with local
 * tids (as mc_bam_gpu_open_contigs gives them); the header counts stay the
 * whole file's.  (Rank 0 of a multi-GPU run without an index decodes the
 * whole file for the extents table and keeps its own shard this way.)
 * MC_E_INVALID if the file is not coordinate-sorted. */
int mc_bam_gpu_restrict(mc_bam_gpu* g, int32_t n_sel, const int32_t* sel);
/* Kept intervals [first, first + count) of the handle, copied to the host
 * (the records of chosen contigs: offsets from the extents' n_kept). */
int mc_bam_gpu_intervals_range(const mc_bam_gpu* g, int64_t first, int64_t count, int32_t* tid,
                               int32_t* pos, int32_t* span);
/* Test hooks (no GPU): the lane decoder of the inflate kernel and the record
 * parse of the walk kernels, run on the host.  mc_gz_inflate_host: one raw
 * deflate stream into exactly isize bytes (MC_E_IO otherwise).
 * mc_bam_rec_parse_host: record body r[0, len) after block_size -> 0
 * dropped, 1 kept (out3 = tid, pos, span), 2 tid beyond n_ref, 3 CIGAR
 * overruns, 4 span exceeds int32. */
int mc_gz_inflate_host(const uint8_t* src, int64_t clen, uint8_t* dst, int64_t isize);
int mc_bam_rec_parse_host(const uint8_t* r, int64_t len, int32_t n_ref, uint32_t flag_filter,
                          int32_t* out3);
/* mc_bam_rec_bases_host: the bases-mode record rule for the record body
 * r[0, len) -> 0 dropped by the filters, 1 taken (out7 = tid, pos, l_seq, the
 * CIGAR word count, and the offsets in r of the CIGAR words, of SEQ and of
 * QUAL), 2 kept without SEQ, 3 kept with a CIGAR query length other than
 * l_seq, 4 malformed (l_seq < 0; CIGAR, SEQ or QUAL past len; tid outside
 * [-1, n_ref); len < 32).  Reads nothing outside r[0, len). */
int mc_bam_rec_bases_host(const uint8_t* r, int64_t len, int32_t n_ref, uint32_t flag_filter, int32_t min_mapq,
                          int64_t* out7);
/* mc_bam_rec_chain_host: 1 if offset q of the inflated stream d[0, n) starts
 * `chain` structurally valid records in sort order (mapped records' bin
 * fields equal to reg2bin of their span), or a shorter such chain ending
 * exactly at n — the GPU record sync's rule; else 0. */
int mc_bam_rec_chain_host(const uint8_t* d, int64_t n, int64_t q, int32_t n_ref, int chain);
/* mc_bgzf_scan_host: the GPU decode's BGZF block scan (pread, n_threads
 * ranges) -> block count, inflated total, the first cap block offsets. */
int mc_bgzf_scan_host(const char* path, int n_threads, int64_t* n_blocks, int64_t* inflated,
                      int64_t* offsets, int64_t cap);
/* Test hook (needs the GPU): the inflate kernel itself, launched as the
 * resident decode launches it, over n_blocks raw deflate payloads
 * comp[cdata[i], cdata[i] + clen[i]), block i inflating to
 * out[out_off[i], out_off[i] + isize[i]).  The device output is filled with
 * 0xAA before the launch and `out` (a host buffer of out_bytes) receives all
 * of it, so bytes written outside a block's range are visible.  status[i]:
 * the kernel's per-block result (0 ok, 1 block type, 2 stored length, 3 code
 * lengths, 4 code, 5 distance, 6 more output than isize, 7 payload overrun,
 * 8 fewer bytes than isize; -1: no lane visited the block); a non-zero status
 * is data, not an error return.  max_lanes: 0 for the decode's own grid, else
 * the lanes the grid is capped at (fewer lanes than blocks: each lane takes
 * several blocks in turn), a positive multiple of the kernel's lanes per wave;
 * the lanes per wave always divide 64, so every multiple of 64 is accepted.
 * MC_E_INVALID (nothing launched): a payload outside comp, an output range
 * outside out, overlapping output ranges, a bad max_lanes. */
int mc_gz_inflate_device(int device, int64_t n_blocks, const uint8_t* comp, int64_t comp_bytes,
                         const int64_t* cdata, const int32_t* clen, const int64_t* out_off,
                         const int32_t* isize, uint8_t* out, int64_t out_bytes, int32_t max_lanes,
                         int32_t* status);

/* ---- synthetic BAM writer ------------------------------------------------
 * Writes coordinate-sorted records from SoA arrays as BGZF-compressed BAM
 * (blocks deflated on n_threads threads; level = zlib level).  The role of
 * the reference's `metacov simulate` (cli.py:288-414) for the benchmarks and
 * end-to-end tests, without ART.  Bases 'A', qualities 30, names "r<i>". */
int mc_bam_write(const char* path, int32_t n_ref, const char* const* names,
                 const int64_t* lengths, int64_t n, const int32_t* tid,
                 const int32_t* pos, const uint16_t* flag, const int64_t* cig_off,
                 const uint32_t* cigar, int32_t l_seq, int level, int n_threads);

/* ---- pileup.experimental (metacov/pileup.py:38-173, SURVEY.md §8 f) --------
 * The reference's experimental estimator, called by `metacov pileup -k`
 * (cli.py:81, :93-95) after classic() for every region.
 *
 * Read side (host C++): mc_reads_open decodes every placed record of a
 * coordinate-sorted BAM into the fields experimental() reads from pysam
 * (flags, query_name, reference_start, reference_length, the first K bases
 * of query_alignment_sequence as a 2-bit A/C/G/T code).  It replaces
 * bam.fetch(ref, start, end) at pileup.py:101.  mc_experimental_reads runs
 * the per-read loop (pileup.py:101-151) for R regions on n_threads threads:
 *   counts[8*q + 0..7] = status (0 ok, 1 read without SEQ, 2 read without
 *       reference_length, 3 k_cor None with a mate pair -- the reference
 *       raises TypeError for 1-3), secondary, improper, nreads,
 *       sum(cov), #distinct starts, sum(cov2), #"RCOR is ZERO" events
 *   sums[4*q + 0..3] = sum(cov_cor) (summation order differs from the
 *       reference), builtin sum(cor) and np.add.reduce(cor) (both exact),
 *       wnf (exact, pairing order)
 * K-mer tables: val/has [4^K] per read number (k_cor[0], k_cor[1]); pass
 * NULL tables for k_cor = None.  Events of region q (readno << 32 | code):
 * mc_experimental_events. */
typedef struct mc_reads mc_reads;
int mc_reads_open(const char* path, int n_threads, int k_len, mc_reads** out);
/* The same table with the BAM decoded on GPU `device` (mc_bam_gpu_open_reads)
 * and copied to the host; the same checks and errors. */
int mc_reads_open_gpu(const char* path, int device, int n_threads, int k_len, mc_reads** out);
/* One rank's read table: the placed records of contigs sel[0..n_sel) only,
 * decoded from their BGZF blocks (extents: a BAI's, mc_bam_index_extents, or
 * a whole-file decode's, mc_bam_gpu_extents). */
int mc_reads_open_gpu_extents(const char* path, int device, int n_threads, int k_len, int32_t n_ref,
                              const mc_contig_extent* ext, int64_t n_no_coor, int32_t n_sel, const int32_t* sel,
                              mc_reads** out);
int mc_reads_close(mc_reads* r);
int mc_reads_header(const mc_reads* r, int32_t* n_ref, int64_t* n_records, int64_t* n_placed);
int mc_reads_target(const mc_reads* r, int32_t i, const char** name, int64_t* length);
/* The table itself (views into the handle, n_placed entries; first: n_ref + 1
 * per-contig record offsets, max_span: n_ref) -- for tests and bindings that
 * read the placed records directly. */
int mc_reads_fields(const mc_reads* r, const int32_t** pos, const int64_t** end, const uint16_t** flag,
                    const uint8_t** bits, const uint32_t** kmer, const uint64_t** name_off,
                    const uint8_t** name_len, const char** names, int64_t* name_bytes,
                    const int64_t** first, const int64_t** max_span);
int mc_experimental_reads(mc_reads* r, int k_len, const double* val1, const uint8_t* has1,
                          const double* val2, const uint8_t* has2, int64_t R,
                          const int32_t* tid, const int64_t* start, const int64_t* end,
                          int n_threads, int64_t* counts, double* sums);
int mc_experimental_events(const mc_reads* r, int64_t region, int64_t cap, uint64_t* events,
                           int64_t* n);

/* Sequence side (GPU, fp64): the k-mer correction correlation of
 * pileup.py:63-88 -- fwd / rev k-mer weights over the region's bases, the
 * 900-tap normal-pdf correlation of rev and inner(fwd, revsum) -- plus the
 * G+C / A+T counts of pileup.py:64-66.  seq = all contigs' bases back to
 * back (as in the FASTA, any case); a region is (base offset of its first
 * base, bases available n <= length, length = end - start).  fwd / rev:
 * dense [4^K] tables, 0 for missing keys; taps = norm[0 .. n_taps).
 * inner[q] is ecor * length.  kernel_ms: HIP-event time of the kernel. */
typedef struct mc_ecor mc_ecor;
int mc_ecor_create(int device, mc_ecor** out);
int mc_ecor_destroy(mc_ecor* e);
int mc_ecor_set_sequence(mc_ecor* e, int64_t n_bytes, const uint8_t* seq);
int mc_ecor_set_tables(mc_ecor* e, int k_len, const double* fwd, const double* rev,
                       int n_taps, const double* taps);
int mc_ecor_run(mc_ecor* e, int64_t R, const int64_t* base, const int64_t* n_avail,
                const int64_t* length, double* inner, int64_t* gc, int64_t* at,
                float* kernel_ms);

/* ---- metacov scan: read histograms (SURVEY.md §8 f ranks 3-4) --------------
 * Replaces scan.scan_reads + the ReadProcessor plugins (metacov/scan.pyx:
 * 345-376 ReadProcessor / ReadProcessorList, 380-419 ByFlag, 422-476
 * BaseHist, 479-511 KmerHist, 514-552 MirrorHist, 555-588 IsizeHist,
 * 623-672 scan_reads) and the read iterators they are fed by
 * (AlignmentFileIterator scan.pyx:188-294, FastQFileIterator :297-340 over
 * pyfq.FastQFile / FastQFilePair, pyfq.pyx:60-270).
 *
 * Sources (host C++): every record of a BAM (file order, placed and unplaced)
 * or of one FASTQ / a FASTQ pair (plain or gzip), handed out in SoA batches
 * of the ReadIterator accessors: rlen = get_len, flag = get_flags, gpos =
 * get_pos, gisize = get_isize, tid = get_tid (int32 each), packed nt16 bases
 * (2 per byte, high nibble first; seq_off[n + 1] byte offsets).  Batch
 * arrays are borrowed until the next mc_scan_src_next. */
typedef struct mc_scan_src mc_scan_src;
int mc_scan_src_open_bam(const char* path, int n_threads, mc_scan_src** out);
int mc_scan_src_open_fastq(const char* path1, const char* path2, mc_scan_src** out);
/* SAM text (plain, gzip or BGZF), the records as htslib's sam_parse1 stores
 * them (pysam opens a .sam for `metacov scan x.sam`: cli.py:171-173,
 * scan.pyx:188-216): @SQ order for the tids, POS - 1, nt16 bases. */
int mc_scan_src_open_sam(const char* path, mc_scan_src** out);
int mc_scan_src_close(mc_scan_src* s);
int mc_scan_src_n_targets(const mc_scan_src* s, int32_t* n);
int mc_scan_src_target(const mc_scan_src* s, int32_t i, const char** name, int64_t* length);
int mc_scan_src_next(mc_scan_src* s, int64_t max_reads, int64_t max_seq_bytes, int64_t* n_out);
int mc_scan_src_batch(const mc_scan_src* s, const int32_t** rlen, const int32_t** flag,
                      const int32_t** gpos, const int32_t** gisize, const int32_t** tid,
                      const int64_t** seq_off, const uint8_t** seq, int64_t* seq_bytes);
int mc_scan_src_records(const mc_scan_src* s, int64_t* n_records);

/* Histograms (GPU).  The processor tree the CLI builds (cli.py:247-257):
 * ByFlag over any of BaseHist(base_start), KmerHist(k, nk, step, offset),
 * MirrorHist(offset, n), IsizeHist, grouped by the flag masks in order
 * (2^n_flags groups, the first flag the most significant group bit).
 * mc_scan_set_reference: FASTA sequences (ASCII) for BaseHist / MirrorHist;
 * a batch's ref_id selects one per read (-1: none; reads as N).
 * mc_scan_run drives a source through the kernel (max_reads 0 = all), with
 * tid_to_ref mapping source tids to reference sequences.  Results come back
 * group-major in the reference's layouts: base [G][rows][5] with rows =
 * max(50, longest read) + base_start, kmer [G][4^K+1][NK], mirror
 * [G][N+1][2], isize [G][isize_cap] and isize_max [G]. */
typedef struct mc_scan_config {
    int32_t n_flags;
    uint32_t flags[16];
    int32_t base_on, base_start;
    int32_t kmer_on, kmer_k, kmer_nk, kmer_step, kmer_offset;
    int32_t mirror_on, mirror_offset, mirror_n;
    int32_t isize_on;
} mc_scan_config;
typedef struct mc_scan mc_scan;
int mc_scan_create(int device, const mc_scan_config* cfg, mc_scan** out);
int mc_scan_destroy(mc_scan* s);
int mc_scan_set_reference(mc_scan* s, int32_t n_seq, const int64_t* off, const int64_t* len,
                          int64_t n_bytes, const uint8_t* ascii);
int mc_scan_add_batch(mc_scan* s, int64_t n, const int32_t* rlen, const int32_t* flag,
                      const int32_t* gpos, const int32_t* gisize, const int32_t* ref_id,
                      const int64_t* seq_off, const uint8_t* seq);
int mc_scan_add_batch_device(mc_scan* s, int64_t n, const int32_t* rlen, const int32_t* flag,
                             const int32_t* gpos, const int32_t* gisize, const int32_t* ref_id,
                             const int64_t* seq_off, const uint8_t* seq, int32_t max_rlen,
                             int64_t max_abs_isize, float* kernel_ms);
int mc_scan_run(mc_scan* s, mc_scan_src* src, int32_t n_map, const int32_t* tid_to_ref,
                int64_t max_reads, int64_t batch_reads, int64_t* n_done);
/* mc_scan_run over a BAM decoded on the GPU (mc_bam_gpu_open_scan): the same
 * reads and reference-id rule, the whole file as one device batch. */
int mc_scan_run_gpu(mc_scan* s, const mc_bam_gpu* g, int32_t n_map, const int32_t* tid_to_ref,
                    int64_t max_reads, int64_t* n_done);
int mc_scan_dims(mc_scan* s, int32_t* groups, int64_t* base_rows, int64_t* isize_cap,
                 int32_t* max_rlen, int64_t* n_reads);
int mc_scan_results(mc_scan* s, uint32_t* base, uint32_t* kmer, uint32_t* mirror,
                    uint32_t* isize, int32_t* isize_max);
int mc_scan_timing(mc_scan* s, float* last_kernel_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* METACOV_AMD_H */
