"""Benchmark of the diversity stage (csrc/bases_div.h: div_zero / div_tile).

    python scripts/bench_diversity.py [--reads N] [--contigs C] [--length L] [--batch B]
                                      [--out profiles/diversity_bench.json]

Workload: bench_consensus.py's (C contigs of L positions, N reads of 150 bases
with 1 % mismatches, 2 % with a 2-base deletion and 2 % with a 2-base
insertion, segments = whole contigs), piled up once; generation and pileup are
not timed here.  On those planes, in one process, the calls alternating round
by round (2 warm-up rounds, then 9 measured; medians of HIP-event times):

  diversity   min_depth 5, min_count 2, min_frac 0.05, with the reference
              plane, at window 0 (whole contigs), 500 and 16 (the LDS-add
              path): tile_ms and combine_ms of mc_bases_diversity_timing
  consensus   bench_consensus.py's call: call_ms of mc_bases_consensus_timing.
              cons_call_kernel reads five planes and ref and writes 1 B per
              position: the closest byte mix, the yardstick
  host route  the six planes copied to the host (24 B per position) and the
              contract in numpy (tests/diversity_model.py), contig by contig;
              its rows are compared with the GPU's at all three windows

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
CONS = dict(min_depth=10, min_count=2, call_ppm=500000)
WINDOWS = (0, 500, 16)
HBM_PEAK = 8.0e12                   # bytes/s
BYTES_PER_POSITION = 17             # four planes and the reference byte


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--contigs", type=int, default=100)
    ap.add_argument("--length", type=int, default=500_000)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    return ap.parse_args(argv)


def median(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def main(argv=None):
    args = parse(argv)
    import torch
    torch.zeros(1, device="cuda")          # torch's HIP runtime first (tests/conftest.py)
    import bench_bases
    from metacov_amd import bases as mb
    from tests import diversity_model as dm
    rng = np.random.default_rng(args.seed)
    nc, L = args.contigs, args.length
    per = args.reads // nc
    n_reads = per * nc
    ref = (1 << rng.integers(0, 4, size=(nc, L + 8), dtype=np.uint8)).astype(np.uint8)
    all_tid = np.repeat(np.arange(nc, dtype=np.int32), per)
    all_pos = np.sort(rng.integers(0, L - 152, size=(nc, per), dtype=np.int32), axis=1).reshape(-1)
    tids = np.arange(nc, dtype=np.int32)
    positions = nc * L
    code_of = np.full(16, 4, np.uint8)
    code_of[[1, 2, 4, 8]] = [0, 1, 2, 3]
    ref_codes = code_of[ref[:, :L]].reshape(-1)

    bc = mb.BaseCounter(nc, 0)
    bc.begin(tids, np.zeros(nc, np.int64), np.full(nc, L, np.int64), min_baseq=0)
    t0 = time.perf_counter()
    for a in range(0, n_reads, args.batch):
        z = min(n_reads, a + args.batch)
        b = bench_bases.make_batch(rng, ref, all_tid[a:z], all_pos[a:z])[0]
        bc.add_reads(b["tid"], b["pos"], b["cig_off"], b["cigar"], b["l_seq"], b["seq_off"], b["seq"],
                     b["qual_off"], b["qual"])
    build_s = time.perf_counter() - t0

    tile = {w: [] for w in WINDOWS}
    zero = {w: [] for w in WINDOWS}
    wall = {w: [] for w in WINDOWS}
    cons_call = []
    got = {}
    for k in range(11):
        for w in WINDOWS:
            t0 = time.perf_counter()
            got[w] = bc.diversity(w, ref=ref_codes, **ARGS)
            dt = time.perf_counter() - t0
            if k >= 2:
                t = bc.diversity_timing()
                tile[w].append(t["tile_ms"])
                zero[w].append(t["combine_ms"])
                wall[w].append(dt * 1e3)
        bc.consensus(ref=ref_codes, **CONS)
        if k >= 2:
            cons_call.append(bc.consensus_timing()["call_ms"])

    # the host route: planes to the host, the contract in numpy, contig by contig
    copy_s = model_s = 0.0
    agrees = True
    bounds = {w: dm.windows([0, L], w) for w in WINDOWS}
    for c in range(nc):
        t0 = time.perf_counter()
        planes = bc.counts(c * L, L)
        copy_s += time.perf_counter() - t0
        t0 = time.perf_counter()
        per_pos = dm.per_position(planes, ref=ref_codes[c * L:(c + 1) * L], **ARGS)
        pre = np.concatenate([np.zeros((dm.COLS, 1), np.int64), np.cumsum(per_pos, axis=1)], axis=1)
        for w in WINDOWS:
            _, _, lo, hi = bounds[w]
            rows = (pre[:, hi] - pre[:, lo]).T
            a = int(got[w].win_first[c])
            agrees = agrees and bool(np.array_equal(rows, got[w].rows[a:a + len(rows)]))
        model_s += time.perf_counter() - t0
    bc.close()

    floor_ms = BYTES_PER_POSITION * positions / HBM_PEAK * 1e3
    c_ms = median(cons_call)
    by_window = {}
    for w in WINDOWS:
        t_ms, z_ms = median(tile[w]), median(zero[w])
        by_window[str(w)] = {
            "windows": len(got[w]), "tile_ms": t_ms, "zero_ms": z_ms, "total_ms": t_ms + z_ms,
            "call_wall_ms": median(wall[w]), "tile_over_cons_call": t_ms / c_ms,
            "fraction_of_hbm_floor": floor_ms / (t_ms + z_ms),
            "achieved_GBps": BYTES_PER_POSITION * positions / (t_ms * 1e-3) / 1e9,
            "tile_ms_all_runs": tile[w], "zero_ms_all_runs": zero[w]}
    whole = got[0].rows.sum(axis=0)
    line = {
        "metric": "diversity: positions/sec through div_zero + div_tile at window 0 (csrc/bases_div.h), 1 MI355X",
        "value": positions / (by_window["0"]["total_ms"] * 1e-3), "unit": "positions/s", "n_gpus": 1,
        "higher_is_better": True, "dtype": "uint32 planes, int64 rows",
        "data": "synthetic (host-generated, C3-shaped)",
        "config": {"workload": "%d contigs x %d positions, %d x 150-base reads (1 %% mismatches, 2 %% 2D, 2 %% 2I), "
                               "segments = whole contigs" % (nc, L, n_reads),
                   "diversity": ARGS, "consensus": CONS,
                   "runs": "median of 9 after 2 warm-ups, HIP events, the calls alternating in one process",
                   "pileup_build_s": round(build_s, 2)},
        "positions": positions, "reads": n_reads,
        "by_window": by_window,
        "cons_call_ms": c_ms, "cons_call_ms_all_runs": cons_call,
        "hbm_floor_ms": floor_ms,
        "totals_window_0": dict(zip(mb.DIV_COLUMNS, (int(v) for v in whole))),
        "roofline": {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK / 1e9,
                     "algorithmic_bytes": BYTES_PER_POSITION * positions,
                     "note": "four planes (16 B) and ref (1 B) read per position, 64 B written per window"},
        "host_route": {"what": "planes copied to the host (24 B per position) and the contract in numpy "
                               "(tests/diversity_model.py), contig by contig, the three windows from one prefix sum",
                       "copy_s": copy_s, "numpy_s": model_s, "agrees": agrees},
    }
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    if not agrees:
        raise SystemExit("the GPU diversity rows differ from the host route")


if __name__ == "__main__":
    main()
