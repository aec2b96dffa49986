"""Benchmark of the insertion stage (csrc/bases_ins.h): extract, group, consensus.

    python scripts/bench_insertions.py [--reads N] [--contigs C] [--length L] [--batch B]
                                       [--out profiles/insertions_bench.json]

Workload: bench_bases.py's (C contigs of L positions, N reads of 150 bases
with 1 % mismatches, 2 % with a 2-base deletion and 2 % with a 2-base
insertion, segments = whole contigs).  The batches are generated once and kept
on the host; generation is not timed.  In one process, alternating:

  off         a counter that does not track: the pileup kernel's time over the
              batches (mc_bases_timing), the yardstick of the extract
  on          a tracking counter over the same batches: its pileup time, the
              extract's (count pass, scan, read-back, fill pass; summed over
              the batches, mc_bases_insertions_timing) and the first
              mc_bases_insertions (scatter, sort, encode).  3 rounds of off /
              on after one warm-up round; medians
  encode      further mc_bases_insertions calls on the sorted buckets (the
              encode alone), median of 9
  consensus   min_depth 10, min_count 2, call_frac 0.5 with the reference
              plane, without and with insertions: the three launches'
              HIP-event times and the insertion part's (encode with the
              consensus thresholds, pick, two scans, fix), median of 9 after 2
  host route  the same table from the first batch's reads in numpy (the I op
              found per read kind, np.unique over (anchor, code)), against a
              tracking counter fed that batch alone; the rows are compared

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


def add(bc, b):
    bc.add_reads(b["tid"], b["pos"], b["cig_off"], b["cigar"], b["l_seq"], b["seq_off"], b["seq"], b["qual_off"],
                 b["qual"])


def host_table(batch, kind, codes, length):
    """(index, code, count) of the batch's insertion alleles in numpy: kind 2
    is 70M2I78M, so the anchor is pos + 69 and the allele bases 70 and 71."""
    m = kind == 2
    digit = np.full(16, 0, np.int64)
    digit[[1, 2, 4, 8]] = [0, 1, 2, 3]
    index = batch["tid"][m].astype(np.int64) * length + batch["pos"][m] + 69
    code = digit[codes[m][:, 70]] * 4 + digit[codes[m][:, 71]]
    key, count = np.unique(index * 16 + code, return_counts=True)
    return key // 16, key % 16, count


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
    starts, ends = np.zeros(nc, np.int64), np.full(nc, L, np.int64)
    positions = nc * L
    code_of = np.full(16, 4, np.uint8)
    code_of[[1, 2, 4, 8]] = [0, 1, 2, 3]
    ref_codes = code_of[ref[:, :L]].reshape(-1)
    batches, first_extra = [], None
    for a in range(0, n_reads, args.batch):
        z = min(n_reads, a + args.batch)
        b, kind, codes = bench_bases.make_batch(rng, ref, all_tid[a:z], all_pos[a:z])
        batches.append(b)
        if first_extra is None:
            first_extra = (kind, codes)

    off, on = mb.BaseCounter(nc, 0), mb.BaseCounter(nc, 0)
    rounds = {"pileup_off_ms": [], "pileup_on_ms": [], "prepass_on_ms": [], "extract_ms": [], "group_first_ms": [],
              "add_wall_off_s": [], "add_wall_on_s": []}
    for k in range(4):                      # round 0 warms both up
        off.begin(tids, starts, ends)
        t0 = time.perf_counter()
        for b in batches:
            add(off, b)
        w_off = time.perf_counter() - t0
        on.begin(tids, starts, ends, insertions=True)
        t0 = time.perf_counter()
        for b in batches:
            add(on, b)
        w_on = time.perf_counter() - t0
        ins = on.insertions(1, 1, 0)
        if k:
            t = on.insertions_timing()
            rounds["pileup_off_ms"].append(off.timing()["pileup_ms"])
            rounds["pileup_on_ms"].append(on.timing()["pileup_ms"])
            rounds["prepass_on_ms"].append(on.timing()["prepass_ms"])
            rounds["extract_ms"].append(t["extract_ms"])
            rounds["group_first_ms"].append(t["group_ms"])
            rounds["add_wall_off_s"].append(w_off)
            rounds["add_wall_on_s"].append(w_on)
    events = on.insertions_timing()["events"]
    same_planes = bool(np.array_equal(off.counts(0, min(positions, 1 << 22)), on.counts(0, min(positions, 1 << 22))))
    encode_ms = []
    for k in range(11):
        on.insertions(10, 2, 20000)
        if k >= 2:
            encode_ms.append(on.insertions_timing()["group_ms"])

    plain = {"call_ms": [], "scan_ms": [], "emit_ms": []}
    with_ins = {"call_ms": [], "scan_ms": [], "emit_ms": [], "insertion_part_ms": []}
    for k in range(11):
        on.consensus(ref=ref_codes, **ARGS)
        tp = on.consensus_timing()
        cons = on.consensus(ref=ref_codes, insertions=True, **ARGS)
        tw = on.consensus_timing()
        if k >= 2:
            for key in plain:
                plain[key].append(tp[key])
                with_ins[key].append(tw[key])
            with_ins["insertion_part_ms"].append(on.insertions_timing()["consensus_ms"])
    inserted = cons.inserted.sum(axis=0)

    # the host route on the first batch
    kind, codes = first_extra
    t0 = time.perf_counter()
    h_index, h_code, h_count = host_table(batches[0], kind, codes, L)
    host_s = time.perf_counter() - t0
    on.begin(tids, starts, ends, insertions=True)
    t0 = time.perf_counter()
    add(on, batches[0])
    small = on.insertions(0, 1, 0)
    gpu_slice_wall_s = time.perf_counter() - t0
    ts = on.insertions_timing()
    agrees = bool(np.array_equal(small.index, h_index) and np.array_equal(small.code.astype(np.int64), h_code) and
                  np.array_equal(small.count.astype(np.int64), h_count) and (small.length == 2).all() and
                  not small.other.any())
    off.close()
    on.close()

    med = {k: median(v) for k, v in rounds.items()}
    mp, mw = {k: median(v) for k, v in plain.items()}, {k: median(v) for k, v in with_ins.items()}
    plain_total = mp["call_ms"] + mp["scan_ms"] + mp["emit_ms"]
    with_total = mw["call_ms"] + mw["scan_ms"] + mw["emit_ms"] + mw["insertion_part_ms"]
    words = sum(len(b["cigar"]) for b in batches)
    line = {
        "metric": "insertions: extract time over the pileup kernel's on the same batches (csrc/bases_ins.h), 1 MI355X",
        "value": med["extract_ms"] / med["pileup_off_ms"], "unit": "ratio", "n_gpus": 1, "higher_is_better": False,
        "dtype": "24-byte events, uint32 counts", "data": "synthetic (host-generated, C3-shaped)",
        "config": {"workload": "%d contigs x %d positions, %d x 150-base reads (1 %% mismatches, 2 %% 2D, 2 %% 2I), "
                               "segments = whole contigs, batches of %d" % (nc, L, n_reads, args.batch),
                   "runs": "3 rounds off / on after 1 warm-up, medians; encode and consensus: median of 9 after 2; "
                           "HIP events"},
        "positions": positions, "reads": n_reads, "cigar_words": words, "events": events, "rows": len(ins),
        "batches": len(batches),
        "ms": {"pileup_off": med["pileup_off_ms"], "pileup_on": med["pileup_on_ms"], "prepass_on": med["prepass_on_ms"],
               "extract": med["extract_ms"], "group_first": med["group_first_ms"], "encode": median(encode_ms),
               "all_rounds": rounds, "encode_all_runs": encode_ms},
        "add_wall_s": {"off": med["add_wall_off_s"], "on": med["add_wall_on_s"]},
        "extract_over_pileup": med["extract_ms"] / med["pileup_off_ms"],
        "group_over_pileup": med["group_first_ms"] / med["pileup_off_ms"],
        "planes_equal_off_on": same_planes,
        "consensus_ms": {"plain": dict(mp, total=plain_total), "with_insertions": dict(mw, total=with_total),
                         "with_over_plain": with_total / plain_total,
                         "insertions_called": int(inserted[0]), "bases_inserted": int(inserted[1])},
        "host_route": {"what": "the first batch's reads: numpy from the generator's read kinds and codes, np.unique "
                               "over (anchor, code); the GPU side is add_reads + insertions of that batch alone",
                       "reads": int(len(batches[0]["tid"])), "rows": int(len(h_index)), "numpy_s": host_s,
                       "gpu_wall_s": gpu_slice_wall_s, "gpu_extract_ms": ts["extract_ms"],
                       "gpu_group_ms": ts["group_ms"], "agrees": agrees},
    }
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    if not agrees or not same_planes:
        raise SystemExit("the GPU table differs from the host route, or tracking changed the planes")


if __name__ == "__main__":
    main()
