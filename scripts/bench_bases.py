"""Benchmark of the base-count kernels (csrc/bases.hip).

    python scripts/bench_bases.py [--reads N] [--contigs C] [--length L] [--batch B]
                                  [--host-batches K] [--out profiles/bases_bench.json]

Workload (synthetic, C3-shaped, sized to fit memory): C contigs of L positions,
N reads of 150 bases spread evenly, drawn from a random reference with 1 %
mismatches; 2 % of the reads carry a 2-base deletion (70M2D80M) and 2 % a
2-base insertion (70M2I78M).  Segments = whole contigs.  The reads are
generated on the host batch by batch (B reads each, in mc_bases_add_batch's
layout, every read's bases on a 4-byte boundary as the BAM source lays them
out) and added one batch at a time; generation is not timed.

Recorded: HIP-event times of the pre-pass and the pileup kernel summed over
the batches (mc_bases_timing), of one sites call, counted bases per second,
and the achieved bytes against the algorithmic ones: bases + qualities + CIGAR
words + 12 B per read (tid, pos, l_seq) read once, 24 B per position written.
The pileup launch of every batch flushes only the tiles its reads touch, so
with sorted batches the planes are written about once.  For context: the same
counts through numpy on the host (bincount per channel; the first K batches,
compared with the GPU's planes), and K2's time on the same intervals.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RL = 150
CIGARS = [((RL << 4) | 0,), ((70 << 4) | 0, (2 << 4) | 2, (80 << 4) | 0), ((70 << 4) | 0, (2 << 4) | 1, (78 << 4) | 0)]
SPANS = [150, 152, 148]


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--contigs", type=int, default=100)
    ap.add_argument("--length", type=int, default=500_000)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--host-batches", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    return ap.parse_args(argv)


def make_batch(rng, ref, tid, pos):
    """The reads at (tid, pos) (sorted) as an add_batch batch plus their kind
    (0: 150M, 1: 70M2D80M, 2: 70M2I78M) and nt16 codes [n, 150]."""
    n = len(tid)
    kind = rng.choice(3, size=n, p=[0.96, 0.02, 0.02]).astype(np.int8)
    # the reference bases under each query base: D shifts the tail by +2, I repeats two bases
    qi = np.arange(RL, dtype=np.int64)
    off = np.stack([qi, qi + 2 * (qi >= 70), np.where(qi < 70, qi, np.maximum(qi - 2, 70))])
    codes = ref[tid.astype(np.int64)[:, None], pos.astype(np.int64)[:, None] + off[kind]]
    miss = rng.random(codes.shape, dtype=np.float32) < 0.01
    codes[miss] = (1 << rng.integers(0, 4, size=int(miss.sum()))).astype(np.uint8)
    seq = np.zeros((n, 76), np.uint8)
    seq[:, :75] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    qual = rng.integers(20, 41, size=(n, RL), dtype=np.uint8)
    n_ops = np.where(kind == 0, 1, 3)
    cig_off = np.zeros(n + 1, np.int64)
    cig_off[1:] = np.cumsum(n_ops)
    cigar = np.zeros(int(cig_off[-1]), np.uint32)
    for k, words in enumerate(CIGARS):
        at = cig_off[:-1][kind == k]
        for j, w in enumerate(words):
            cigar[at + j] = w
    b = {"tid": tid, "pos": pos, "cig_off": cig_off, "cigar": cigar, "l_seq": np.full(n, RL, np.int32),
         "seq_off": np.arange(n + 1, dtype=np.int64) * 76, "seq": seq.reshape(-1),
         "qual_off": np.arange(n + 1, dtype=np.int64) * RL, "qual": qual.reshape(-1)}
    return b, kind, codes


def host_counts(planes, length, tid, pos, kind, codes):
    """The batch's counts added to planes [6, contigs * length] with numpy."""
    chan = np.full(16, 4, np.int64)
    chan[[1, 2, 4, 8]] = [0, 1, 2, 3]
    base = tid.astype(np.int64) * length + pos
    qi = np.arange(RL, dtype=np.int64)
    size = planes.shape[1]
    for k in range(3):
        m = kind == k
        if not m.any():
            continue
        if k == 0:
            q, r = qi, qi
        elif k == 1:
            q, r = qi, qi + 2 * (qi >= 70)
        else:
            q = np.concatenate([qi[:70], qi[72:]])
            r = np.arange(RL - 2, dtype=np.int64)
        idx = (chan[codes[m][:, q]] * size + base[m][:, None] + r).reshape(-1)
        planes += np.bincount(idx, minlength=6 * size).reshape(6, size)
        if k == 1:
            d = (5 * size + base[m][:, None] + np.array([70, 71])).reshape(-1)
            planes += np.bincount(d, minlength=6 * size).reshape(6, size)


def main(argv=None):
    args = parse(argv)
    import torch
    torch.zeros(1, device="cuda")          # torch's HIP runtime first (tests/conftest.py)
    from metacov_amd import bases as mb
    from metacov_amd.engine import CoverageEngine
    rng = np.random.default_rng(args.seed)
    nc, L = args.contigs, args.length
    per = args.reads // nc
    n_reads = per * nc
    ref = (1 << rng.integers(0, 4, size=(nc, L + 8), dtype=np.uint8)).astype(np.uint8)
    all_tid = np.repeat(np.arange(nc, dtype=np.int32), per)
    all_pos = np.sort(rng.integers(0, L - 152, size=(nc, per), dtype=np.int32), axis=1).reshape(-1)
    tids = np.arange(nc, dtype=np.int32)
    starts = np.zeros(nc, np.int64)
    ends = np.full(nc, L, np.int64)
    positions = nc * L

    bc = mb.BaseCounter(nc, 0)
    # warm-up: every kernel once on a small batch (code objects load at the first launch)
    bc.begin(tids[:1], starts[:1], ends[:1], min_baseq=0)
    w = make_batch(np.random.default_rng(0), ref, all_tid[:1000], all_pos[:1000])[0]
    bc.add_reads(w["tid"], w["pos"], w["cig_off"], w["cigar"], w["l_seq"], w["seq_off"], w["seq"], w["qual_off"],
                 w["qual"])
    bc.sites(10, 2, 20000)
    bc.begin(tids, starts, ends, min_baseq=0)
    host_contigs = 0
    host_planes = None
    host_s = gen_s = add_s = 0.0
    bytes_in = counted = 0
    all_span = np.zeros(n_reads, np.int32)
    for k, a in enumerate(range(0, n_reads, args.batch)):
        z = min(n_reads, a + args.batch)
        t0 = time.perf_counter()
        b, kind, codes = make_batch(rng, ref, all_tid[a:z], all_pos[a:z])
        gen_s += time.perf_counter() - t0
        all_span[a:z] = np.array(SPANS, np.int32)[kind]
        t0 = time.perf_counter()
        bc.add_reads(b["tid"], b["pos"], b["cig_off"], b["cigar"], b["l_seq"], b["seq_off"], b["seq"],
                     b["qual_off"], b["qual"])
        add_s += time.perf_counter() - t0
        n = z - a
        bytes_in += n * 75 + n * RL + 4 * len(b["cigar"]) + 12 * n
        counted += int(np.where(kind == 0, 150, np.where(kind == 1, 152, 148)).sum())
        if k < args.host_batches:
            hc = int(all_tid[z - 1]) + 1
            if host_planes is None:
                host_planes = np.zeros((6, hc * L), np.int64)
            elif hc * L > host_planes.shape[1]:
                grown = np.zeros((6, hc * L), np.int64)
                grown[:, :host_planes.shape[1]] = host_planes
                host_planes = grown
            t0 = time.perf_counter()
            host_counts(host_planes, L, all_tid[a:z], all_pos[a:z].astype(np.int64), kind, codes)
            host_s += time.perf_counter() - t0
            host_contigs, host_reads = hc, z
    t = bc.timing()
    sites = bc.sites(10, 2, 20000)
    t_sites = bc.timing()["sites_ms"]
    agrees = None
    if host_planes is not None:
        # only contigs whose reads are all in the host batches compare
        full = int(all_tid[host_reads]) if host_reads < n_reads else nc
        got = bc.counts(0, full * L).astype(np.int64)
        agrees = bool(full > 0 and np.array_equal(got, host_planes[:, :full * L]))
        host_contigs = full
    total = sum(int(bc.counts(c * L, min(10, nc - c) * L).astype(np.int64).sum()) for c in range(0, nc, 10))
    bc.close()

    eng = CoverageEngine(0)
    eng.set_contigs(np.full(nc, L, np.int64))
    eng.add_reads(all_tid, all_pos, all_span)
    eng.compute_depth()
    eng.synchronize()
    eng.compute_depth()
    eng.synchronize()
    k2_ms = eng.timings()["depth_ms"]
    eng.close()

    alg = bytes_in + 24 * positions
    line = {
        "metric": "base counts: counted bases/sec through the pileup kernel (csrc/bases.hip), 1 MI355X",
        "value": counted / (t["pileup_ms"] * 1e-3), "unit": "bases/s", "n_gpus": 1, "higher_is_better": True,
        "dtype": "uint32", "data": "synthetic (host-generated, C3-shaped)",
        "config": {"workload": "%d contigs x %d positions, %d x 150-base reads (1 %% mismatches, 2 %% 2D, 2 %% 2I), "
                               "%d reads per batch, segments = whole contigs" % (nc, L, n_reads, args.batch),
                   "generate_s": round(gen_s, 2)},
        "positions": positions, "reads": n_reads, "counted_bases": counted, "tiles": t["tiles"],
        "kernels_ms": {"prepass": t["prepass_ms"], "pileup": t["pileup_ms"], "sites": t_sites},
        "add_reads_wall_s": add_s,
        "sites": {"min_depth": 10, "min_count": 2, "min_ppm": 20000, "n": len(sites)},
        "roofline": {"bound": "hbm", "achieved": alg / (t["pileup_ms"] * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s",
                     "frac": alg / (t["pileup_ms"] * 1e-3) / 8e12, "algorithmic_bytes": alg,
                     "note": "bases + qualities + CIGAR + 12 B per read read once, 24 B per position written, "
                             "over the pileup kernel's time"},
        "host_route": {"what": "numpy bincount per channel over the first %d batches" % args.host_batches,
                       "seconds": host_s, "reads": int(min(args.host_batches * args.batch, n_reads)),
                       "contigs_compared": host_contigs, "agrees": agrees},
        "k2_depth_ms_same_intervals": k2_ms,
        "planes_sum_equals_counted_bases": bool(total == counted),
    }
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    if agrees is False:
        raise SystemExit("the GPU planes differ from the host route")


if __name__ == "__main__":
    main()
