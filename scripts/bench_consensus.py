"""Benchmark of the consensus kernels (csrc/bases.hip: cons_call / scan / emit).

    python scripts/bench_consensus.py [--reads N] [--contigs C] [--length L] [--batch B]
                                      [--out profiles/consensus_bench.json]

Workload: bench_bases.py's (C contigs of L positions, N reads of 150 bases
with 1 % mismatches, 2 % with a 2-base deletion and 2 % with a 2-base
insertion, segments = whole contigs), piled up once; generation and pileup are
not timed here.  On those planes, in one process:

  consensus   min_depth 10, min_count 2, call_frac 0.5, with the reference
              plane: HIP-event times of the call, scan and emit launches
              (mc_bases_consensus_timing), median of 9 calls after 2 warm-ups
  sites       min_depth 10, min_count 2, min_ppm 20000 (bench_bases.py's
              call): sites_ms of mc_bases_timing, median of 9 after 2.  Its
              count pass reads the same five planes: the yardstick
  host route  the six planes copied to the host (24 B per position) and the
              same rule in numpy, contig by contig; its letters are compared
              with the GPU's

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

ARGS = dict(min_depth=10, min_count=2, call_ppm=500000)
SITES = (10, 2, 20000)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--contigs", type=int, default=100)
    ap.add_argument("--length", type=int, default=500_000)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    return ap.parse_args(argv)


def host_call(planes, ref, min_depth, min_count, call_ppm):
    """The rule without IUPAC and fill_ref in numpy: (aligned letters, differs
    count) of planes [6, n] with reference codes ref [n]."""
    five = planes[[0, 1, 2, 3, 5]].astype(np.int64)
    depth = five.sum(axis=0)
    top = np.argmax(five, axis=0)
    x = five[top, np.arange(five.shape[1])]
    ok = (x >= max(min_count, 1)) & (x * 1000000 >= call_ppm * depth) & (depth >= max(min_depth, 1))
    letters = np.where(ok, np.frombuffer(b"ACGT-", np.uint8)[top], np.uint8(ord("N")))
    differs = ok & (ref < 4) & (top != ref)
    return letters, int(differs.sum())


def median(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def main(argv=None):
    args = parse(argv)
    import torch
    torch.zeros(1, device="cuda")          # torch's HIP runtime first (tests/conftest.py)
    import bench_bases
    from metacov_amd import bases as mb
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

    times = {"call_ms": [], "scan_ms": [], "emit_ms": []}
    wall = []
    for k in range(11):
        t0 = time.perf_counter()
        cons = bc.consensus(ref=ref_codes, **ARGS)
        w = time.perf_counter() - t0
        if k >= 2:
            wall.append(w * 1e3)
            for key, v in bc.consensus_timing().items():
                times[key].append(v)
    sites_ms = []
    for k in range(11):
        sites = bc.sites(*SITES)
        if k >= 2:
            sites_ms.append(bc.timing()["sites_ms"])
    summary = cons.summary.sum(axis=0)

    # the host route: planes to the host, the rule in numpy, contig by contig
    copy_s = call_s = 0.0
    agrees, host_differs = True, 0
    for c in range(nc):
        t0 = time.perf_counter()
        planes = bc.counts(c * L, L)
        copy_s += time.perf_counter() - t0
        t0 = time.perf_counter()
        letters, d = host_call(planes, ref_codes[c * L:(c + 1) * L], **ARGS)
        call_s += time.perf_counter() - t0
        host_differs += d
        agrees = agrees and bool(np.array_equal(letters, cons.aligned(c)))
    agrees = agrees and host_differs == int(summary[mb.DIFFERS])
    bc.close()

    med = {k: median(v) for k, v in times.items()}
    total = med["call_ms"] + med["scan_ms"] + med["emit_ms"]
    s_ms = median(sites_ms)
    line = {
        "metric": "consensus: positions/sec through call + scan + emit (csrc/bases.hip), 1 MI355X",
        "value": positions / (total * 1e-3), "unit": "positions/s", "n_gpus": 1, "higher_is_better": True,
        "dtype": "uint32 planes, uint8 letters", "data": "synthetic (host-generated, C3-shaped)",
        "config": {"workload": "%d contigs x %d positions, %d x 150-base reads (1 %% mismatches, 2 %% 2D, 2 %% 2I), "
                               "segments = whole contigs" % (nc, L, n_reads),
                   "consensus": ARGS, "sites": dict(zip(("min_depth", "min_count", "min_ppm"), SITES)),
                   "runs": "median of 9 after 2 warm-ups, HIP events", "pileup_build_s": round(build_s, 2)},
        "positions": positions, "reads": n_reads,
        "kernels_ms": {"call": med["call_ms"], "scan": med["scan_ms"], "emit": med["emit_ms"], "total": total,
                       "all_runs": times},
        "consensus_call_wall_ms": median(wall),
        "sites_ms": s_ms, "sites_ms_all_runs": sites_ms, "n_sites": len(sites),
        "call_over_sites": med["call_ms"] / s_ms, "total_over_sites": total / s_ms,
        "summary": dict(zip(mb.SUMMARY_COLUMNS, (int(v) for v in summary))),
        "roofline": {"bound": "hbm", "unit": "GB/s", "peak": 8000.0,
                     "algorithmic_bytes_call": 22 * positions,
                     "achieved_call": 22 * positions / (med["call_ms"] * 1e-3) / 1e9,
                     "note": "call: five planes (20 B) + ref (1 B) read, 1 B written per position; emit: 1 B read "
                             "and at most 1 B written"},
        "host_route": {"what": "planes copied to the host (24 B per position) and the same rule in numpy, contig by "
                               "contig", "copy_s": copy_s, "numpy_s": call_s, "agrees": agrees},
    }
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    if not agrees:
        raise SystemExit("the GPU consensus differs from the host route")


if __name__ == "__main__":
    main()
