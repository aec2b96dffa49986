"""Benchmark of the comparison stage (csrc/bases_cmp.h: div_zero / cmp_tile).

    python scripts/bench_compare.py [--reads N] [--contigs C] [--length L] [--batch B]
                                    [--out profiles/compare_bench.json]

Workload: bench_diversity.py's (C contigs of L positions, N reads of 150 bases
with 1 % mismatches, 2 % with a 2-base deletion and 2 % with a 2-base
insertion, segments = whole contigs) for each of two samples: one reference,
two read sets from two seeds, piled up once into two counters; generation and
pileup are not timed here.  On those planes, in one process, the calls
alternating round by round (2 warm-up rounds, then 9 measured; medians of
HIP-event times, the spread beside them):

  compare     min_depth 5, min_count 2, min_frac 0.05 at window 0 (whole
              contigs), 500 and 16 (the LDS-add path): tile_ms and zero_ms of
              mc_bases_compare_timing
  diversity   the same thresholds and windows on sample a's planes, with the
              reference plane: tile_ms of mc_bases_diversity_timing.
              div_tile_kernel reads 17 B per position where cmp_tile_kernel
              reads 32: the yardstick
  host route  both samples' six planes copied to the host (48 B per position)
              and the contract in numpy (tests/compare_model.py), contig by
              contig; its rows are compared with the GPU's at all three windows

No test gates on any of these times.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

ARGS = dict(min_depth=5, min_count=2, min_ppm=50000)
WINDOWS = (0, 500, 16)
HBM_PEAK = 8.0e12                   # bytes/s
BYTES_PER_POSITION = 32             # four planes of each of the two samples
DIV_BYTES_PER_POSITION = 17         # four planes and the reference byte


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000, help="per sample")
    ap.add_argument("--contigs", type=int, default=100)
    ap.add_argument("--length", type=int, default=500_000)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    return ap.parse_args(argv)


def median(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def spread(xs):
    """(max - min) / median of the measured runs."""
    xs = np.asarray(xs, np.float64)
    return float((xs.max() - xs.min()) / np.median(xs))


def main(argv=None):
    args = parse(argv)
    import torch
    torch.zeros(1, device="cuda")          # torch's HIP runtime first (tests/conftest.py)
    import bench_bases
    from metacov_amd import bases as mb
    from tests import compare_model as cm
    from tests import diversity_model as dm
    rng = np.random.default_rng(args.seed)
    nc, L = args.contigs, args.length
    per = args.reads // nc
    n_reads = per * nc
    ref = (1 << rng.integers(0, 4, size=(nc, L + 8), dtype=np.uint8)).astype(np.uint8)
    all_tid = np.repeat(np.arange(nc, dtype=np.int32), per)
    tids = np.arange(nc, dtype=np.int32)
    positions = nc * L
    code_of = np.full(16, 4, np.uint8)
    code_of[[1, 2, 4, 8]] = [0, 1, 2, 3]
    ref_codes = code_of[ref[:, :L]].reshape(-1)

    counters = []
    t0 = time.perf_counter()
    for k in range(2):                     # the two samples: one reference, a read set per seed
        srng = np.random.default_rng(args.seed + 1 + k)
        all_pos = np.sort(srng.integers(0, L - 152, size=(nc, per), dtype=np.int32), axis=1).reshape(-1)
        bc = mb.BaseCounter(nc, 0)
        bc.begin(tids, np.zeros(nc, np.int64), np.full(nc, L, np.int64), min_baseq=0)
        for a in range(0, n_reads, args.batch):
            z = min(n_reads, a + args.batch)
            b = bench_bases.make_batch(srng, ref, all_tid[a:z], all_pos[a:z])[0]
            bc.add_reads(b["tid"], b["pos"], b["cig_off"], b["cigar"], b["l_seq"], b["seq_off"], b["seq"],
                         b["qual_off"], b["qual"])
        counters.append(bc)
    build_s = time.perf_counter() - t0
    sa, sb = counters

    tile = {w: [] for w in WINDOWS}
    zero = {w: [] for w in WINDOWS}
    wall = {w: [] for w in WINDOWS}
    div_tile = {w: [] for w in WINDOWS}
    got = {}
    for k in range(11):
        for w in WINDOWS:
            t0 = time.perf_counter()
            got[w] = sa.compare(sb, w, **ARGS)
            dt = time.perf_counter() - t0
            sa.diversity(w, ref=ref_codes, **ARGS)
            if k >= 2:
                t = sa.compare_timing()
                tile[w].append(t["tile_ms"])
                zero[w].append(t["zero_ms"])
                wall[w].append(dt * 1e3)
                div_tile[w].append(sa.diversity_timing()["tile_ms"])

    # the host route: both samples' planes to the host, the contract in numpy, contig by contig
    copy_s = model_s = 0.0
    agrees = True
    bounds = {w: dm.windows([0, L], w) for w in WINDOWS}
    for c in range(nc):
        t0 = time.perf_counter()
        pa, pb = sa.counts(c * L, L), sb.counts(c * L, L)
        copy_s += time.perf_counter() - t0
        t0 = time.perf_counter()
        per_pos = cm.per_position(pa, pb, **ARGS)
        pre = np.concatenate([np.zeros((cm.COLS, 1), np.int64), np.cumsum(per_pos, axis=1)], axis=1)
        for w in WINDOWS:
            _, _, lo, hi = bounds[w]
            rows = (pre[:, hi] - pre[:, lo]).T
            a = int(got[w].win_first[c])
            agrees = agrees and bool(np.array_equal(rows, got[w].rows[a:a + len(rows)]))
        model_s += time.perf_counter() - t0
    sa.close()
    sb.close()

    floor_ms = BYTES_PER_POSITION * positions / HBM_PEAK * 1e3
    by_window = {}
    for w in WINDOWS:
        t_ms, z_ms, d_ms = median(tile[w]), median(zero[w]), median(div_tile[w])
        by_window[str(w)] = {
            "windows": len(got[w]), "tile_ms": t_ms, "zero_ms": z_ms, "total_ms": t_ms + z_ms,
            "tile_ms_spread": spread(tile[w]), "call_wall_ms": median(wall[w]),
            "div_tile_ms": d_ms, "div_tile_ms_spread": spread(div_tile[w]), "tile_over_div_tile": t_ms / d_ms,
            "fraction_of_hbm_floor": floor_ms / (t_ms + z_ms),
            "achieved_GBps": BYTES_PER_POSITION * positions / (t_ms * 1e-3) / 1e9,
            "div_achieved_GBps": DIV_BYTES_PER_POSITION * positions / (d_ms * 1e-3) / 1e9,
            "tile_ms_all_runs": tile[w], "zero_ms_all_runs": zero[w], "div_tile_ms_all_runs": div_tile[w]}
    whole = got[0].rows.sum(axis=0)
    line = {
        "metric": "compare: positions/sec through div_zero + cmp_tile at window 0 (csrc/bases_cmp.h), 1 MI355X",
        "value": positions / (by_window["0"]["total_ms"] * 1e-3), "unit": "positions/s", "n_gpus": 1,
        "higher_is_better": True, "dtype": "uint32 planes, int64 rows",
        "data": "synthetic (host-generated, C3-shaped)",
        "config": {"workload": "%d contigs x %d positions, two samples of %d x 150-base reads (1 %% mismatches, "
                               "2 %% 2D, 2 %% 2I) on one reference, segments = whole contigs" % (nc, L, n_reads),
                   "compare": ARGS, "diversity": ARGS,
                   "runs": "median of 9 after 2 warm-ups, HIP events, the calls alternating in one process; "
                           "spread = (max - min) / median",
                   "pileup_build_s": round(build_s, 2)},
        "positions": positions, "reads_per_sample": n_reads,
        "by_window": by_window,
        "hbm_floor_ms": floor_ms,
        "bytes_ratio_to_diversity": BYTES_PER_POSITION / DIV_BYTES_PER_POSITION,
        "totals_window_0": dict(zip(mb.CMP_COLUMNS, (int(v) for v in whole))),
        "roofline": {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK / 1e9,
                     "algorithmic_bytes": BYTES_PER_POSITION * positions,
                     "note": "four planes (16 B) of each sample read per position, 64 B written per window"},
        "host_route": {"what": "both samples' planes copied to the host (48 B per position) and the contract in "
                               "numpy (tests/compare_model.py), contig by contig, the three windows from one "
                               "prefix sum",
                       "copy_s": copy_s, "numpy_s": model_s, "agrees": agrees},
    }
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    if not agrees:
        raise SystemExit("the GPU comparison rows differ from the host route")


if __name__ == "__main__":
    main()
