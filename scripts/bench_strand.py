"""Benchmark of the strand-resolved base counts (csrc/bases.hip).

    python scripts/bench_strand.py [--reads N] [--contigs C] [--length L] [--batch B] [--rounds R]
                                   [--parent-lib metacov_amd/variants/lib_parent.so]
                                   [--out profiles/strand_bench.json]

Workload: scripts/bench_bases.py's (C contigs of L positions, N reads of 150
bases, 1 % mismatches, 2 % 2-base deletions, 2 % 2-base insertions, B reads
per batch, segments = whole contigs), every read reverse with probability
1/2, seeded.  The batches are generated once and kept on the host.

One process.  After one untimed pass of every variant, R rounds alternate
  plain     begin(), add_reads() of every batch: the unstranded pileup kernel
  strand    begin(strand=True), add_reads(..., flag=...): the strand kernel
  parent    `plain` through another build of the library (--parent-lib, e.g.
            the parent commit's; left out when the file is absent)
and record, per pass, the HIP-event times of the pre-pass and the pileup
kernels summed over the batches (mc_bases_timing) and of one sites call
(plain: mc_bases_sites; strand: mc_bases_sites_strand with min_alt_strand 0
and 2).  Reported: every pass, the medians, the spread (max - min) between the
repeats of one variant, strand / plain, and the gate: the strand pileup must
take less than two plain pileups, which is what two unstranded passes filtered
on 0x10 would cost.  The strand pass's totals must equal the plain pass's
planes and its reverse planes the counts of the reverse reads alone (a plain
pass over those reads).

Then scripts/bench_bases_decode.py's synthetic BAM: add_bam(decode="gpu") with
and without strand, alternating, wall clock; and the decoder's parse step
(mc_bam_gpu_stats' parse_ms, which holds the fill walk that writes the flag
column) of this build against --parent-lib's.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CHUNK = 1 << 24


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--contigs", type=int, default=100)
    ap.add_argument("--length", type=int, default=500_000)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "metacov_amd", "variants", "lib_parent.so"))
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--out", default=None, help="also write the result to this file")
    return ap.parse_args(argv)


def stats(xs):
    return {"runs": [round(x, 4) for x in xs], "median": statistics.median(xs), "spread": max(xs) - min(xs)}


def feed(bc, batches, flags=None):
    for k, b in enumerate(batches):
        bc.add_reads(b["tid"], b["pos"], b["cig_off"], b["cigar"], b["l_seq"], b["seq_off"], b["seq"], b["qual_off"],
                     b["qual"], **({} if flags is None else {"flag": flags[k]}))


def planes_equal(get_a, get_b, n):
    return all(np.array_equal(get_a(o, min(CHUNK, n - o)), get_b(o, min(CHUNK, n - o))) for o in range(0, n, CHUNK))


def reverse_only(b, f):
    """The reverse reads of a batch as a batch (150-base reads: fixed strides)."""
    m = (f & 0x10) != 0
    n = int(m.sum())
    words = np.diff(b["cig_off"])
    cig_off = np.zeros(n + 1, np.int64)
    cig_off[1:] = np.cumsum(words[m])
    return {"tid": b["tid"][m], "pos": b["pos"][m], "cig_off": cig_off, "cigar": b["cigar"][np.repeat(m, words)],
            "l_seq": b["l_seq"][m], "seq_off": np.arange(n + 1, dtype=np.int64) * 76,
            "seq": b["seq"].reshape(-1, 76)[m].reshape(-1), "qual_off": np.arange(n + 1, dtype=np.int64) * 150,
            "qual": b["qual"].reshape(-1, 150)[m].reshape(-1)}


def main(argv=None):
    args = parse(argv)
    import torch
    torch.zeros(1, device="cuda")          # torch's HIP runtime first (tests/conftest.py)
    from bench_bases import make_batch
    from metacov_amd import _lib
    from metacov_amd import bases as mb
    parent = _lib.load(args.parent_lib) if os.path.exists(args.parent_lib) else None
    rng = np.random.default_rng(args.seed)
    nc, L = args.contigs, args.length
    per = args.reads // nc
    n_reads = per * nc
    ref = (1 << rng.integers(0, 4, size=(nc, L + 8), dtype=np.uint8)).astype(np.uint8)
    all_tid = np.repeat(np.arange(nc, dtype=np.int32), per)
    all_pos = np.sort(rng.integers(0, L - 152, size=(nc, per), dtype=np.int32), axis=1).reshape(-1)
    tids, starts, ends = np.arange(nc, dtype=np.int32), np.zeros(nc, np.int64), np.full(nc, L, np.int64)
    n_pos = nc * L
    t0 = time.perf_counter()
    batches = [make_batch(rng, ref, all_tid[a:a + args.batch], all_pos[a:a + args.batch])[0]
               for a in range(0, n_reads, args.batch)]
    flags = [(rng.integers(0, 2, size=len(b["tid"])) * 0x10).astype(np.uint16) for b in batches]
    gen_s = time.perf_counter() - t0

    counters = {"plain": mb.BaseCounter(nc, 0), "strand": mb.BaseCounter(nc, 0)}
    if parent is not None:
        counters["parent"] = mb.BaseCounter(nc, 0, lib=parent)
    order = [v for v in ("plain", "parent", "strand") if v in counters]
    pile = {v: [] for v in order}
    pre = {v: [] for v in order}
    sites_ms = {"plain": [], "strand_k0": [], "strand_k2": []}
    if parent is not None:
        sites_ms["parent"] = []
    n_sites = {}
    for rnd in range(args.rounds + 1):          # round 0 warms up
        for v in order:
            bc = counters[v]
            bc.begin(tids, starts, ends, **({"strand": True} if v == "strand" else {}))
            feed(bc, batches, flags if v == "strand" else None)
            t = bc.timing()
            if v == "strand":
                s0 = bc.sites(10, 2, 20000, min_alt_strand=0)
                k0 = bc.timing()["sites_ms"]
                s2 = bc.sites(10, 2, 20000, min_alt_strand=2)
                k2 = bc.timing()["sites_ms"]
                n_sites["strand_k0"], n_sites["strand_k2"] = len(s0), len(s2)
            else:
                n_sites[v] = len(bc.sites(10, 2, 20000))
                k0 = bc.timing()["sites_ms"]
            if rnd:
                pile[v].append(t["pileup_ms"])
                pre[v].append(t["prepass_ms"])
                if v == "strand":
                    sites_ms["strand_k0"].append(k0)
                    sites_ms["strand_k2"].append(k2)
                else:
                    sites_ms[v].append(k0)
    plain, strand = counters["plain"], counters["strand"]
    totals_equal = planes_equal(plain.counts, strand.counts, n_pos)
    parent_equal = None if parent is None else planes_equal(plain.counts, counters["parent"].counts, n_pos)
    rev_sum = sum(int(strand.counts_reverse(o, min(CHUNK, n_pos - o)).astype(np.int64).sum())
                  for o in range(0, n_pos, CHUNK))
    tot_sum = sum(int(strand.counts(o, min(CHUNK, n_pos - o)).astype(np.int64).sum()) for o in range(0, n_pos, CHUNK))
    plain.begin(tids, starts, ends)             # the reverse reads alone through the unstranded kernel
    feed(plain, [reverse_only(b, f) for b, f in zip(batches, flags)])
    reverse_equal = planes_equal(plain.counts, strand.counts_reverse, n_pos)
    for bc in counters.values():
        bc.close()

    med = statistics.median
    ratio = med(pile["strand"]) / med(pile["plain"])
    result = {
        "metric": "strand-resolved base counts: strand pileup time over unstranded pileup time (csrc/bases.hip), "
                  "1 MI355X",
        "value": ratio, "unit": "x (medians of HIP-event times summed over the batches)", "n_gpus": 1,
        "higher_is_better": False, "date": time.strftime("%Y-%m-%d"),
        "data": "synthetic (host-generated, scripts/bench_bases.py's workload, half the reads reverse)",
        "config": {"workload": "%d contigs x %d positions, %d x 150-base reads, %d reads per batch, segments = whole "
                               "contigs" % (nc, L, n_reads, args.batch),
                   "rounds": args.rounds, "warmup_rounds": 1, "order_in_a_round": order, "generate_s": round(gen_s, 2)},
        "pileup_ms": {v: stats(pile[v]) for v in order},
        "prepass_ms": {v: stats(pre[v]) for v in order},
        "sites_ms": {v: stats(x) for v, x in sites_ms.items()},
        "n_sites": n_sites,
        "strand_over_plain": {"pileup": ratio, "sites_k0": med(sites_ms["strand_k0"]) / med(sites_ms["plain"]),
                              "sites_k2": med(sites_ms["strand_k2"]) / med(sites_ms["plain"])},
        "gate_strand_below_two_plain_passes": {"strand_pileup_ms": med(pile["strand"]),
                                               "two_plain_pileups_ms": 2 * med(pile["plain"]),
                                               "passed": bool(ratio < 2.0)},
        "checks": {"totals_equal_plain": bool(totals_equal), "reverse_equals_plain_over_reverse_reads":
                   bool(reverse_equal), "reverse_sum": rev_sum, "total_sum": tot_sum,
                   "sites_k0_equal_plain": n_sites["strand_k0"] == n_sites["plain"],
                   "parent_planes_equal": parent_equal},
    }
    if parent is not None:
        d = med(pile["plain"]) - med(pile["parent"])
        result["unstranded_against_parent"] = {
            "pileup_ms_difference_of_medians": d, "spread_plain": stats(pile["plain"])["spread"],
            "spread_parent": stats(pile["parent"])["spread"],
            "within_spread": bool(abs(d) <= max(stats(pile["plain"])["spread"], stats(pile["parent"])["spread"])),
            "sites_ms_difference_of_medians": med(sites_ms["plain"]) - med(sites_ms["parent"])}
    if not args.skip_decode:
        result["decode"] = bench_decode(args, mb, parent)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    bad = [k for k in ("totals_equal_plain", "reverse_equals_plain_over_reverse_reads", "sites_k0_equal_plain")
           if not result["checks"][k]]
    if bad or parent_equal is False:
        raise SystemExit("results differ: %s" % (bad or "parent planes"))
    if ratio >= 2.0:
        raise SystemExit("the strand pileup is not faster than two unstranded passes (%.2fx)" % ratio)


def bench_decode(args, mb, parent):
    from metacov_amd import synth
    nc, L = args.contigs, args.length
    lengths = [L] * nc
    names = ["contig_%d" % (i + 1) for i in range(nc)]
    tids, starts, ends = np.arange(nc, dtype=np.int32), np.zeros(nc, np.int64), np.full(nc, L, np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "strand_bench.bam")
        synth.write_bam_fast(path, names, lengths, *synth.edge_mix_arrays(lengths, args.reads, seed=args.seed), level=1,
                             n_threads=args.threads)
        wall = {"plain": [], "strand": []}
        kern = {"plain": [], "strand": []}
        parse_ms = {"this": [], "parent": []}
        rev_sum = tot_sum = 0
        with mb.BaseCounter(nc, 0) as bc:
            for rnd in range(args.rounds + 1):  # round 0 warms up
                for v in ("plain", "strand"):
                    bc.begin(tids, starts, ends, strand=v == "strand")
                    t0 = time.perf_counter()
                    bc.add_bam(path, n_threads=args.threads, decode="gpu")
                    w = time.perf_counter() - t0
                    if rnd:
                        wall[v].append(w)
                        kern[v].append(bc.timing()["pileup_ms"])
                for who, lib in (("this", None), ("parent", parent)):
                    if who == "parent" and parent is None:
                        continue
                    with mb.GpuBaseSource(path, 0, args.threads, lib=lib) as src:
                        if rnd:
                            parse_ms[who].append(src.timings()["parse_ms"])
            n_pos = nc * L
            rev_sum = sum(int(bc.counts_reverse(o, min(CHUNK, n_pos - o)).astype(np.int64).sum())
                          for o in range(0, n_pos, CHUNK))
            tot_sum = sum(int(bc.counts(o, min(CHUNK, n_pos - o)).astype(np.int64).sum())
                          for o in range(0, n_pos, CHUNK))
        size = os.path.getsize(path)
    out = {"data": "synthetic BAM (synth.write_bam_fast, edge mix, BGZF level 1; scripts/bench_bases_decode.py's)",
           "bam_bytes": size, "add_bam_gpu_s": {v: stats(wall[v]) for v in wall},
           "pileup_ms": {v: stats(kern[v]) for v in kern},
           "strand_over_plain_wall": statistics.median(wall["strand"]) / statistics.median(wall["plain"]),
           "decode_parse_ms": {k: stats(v) for k, v in parse_ms.items() if v},
           "reverse_sum": rev_sum, "total_sum": tot_sum}
    return out


if __name__ == "__main__":
    main()
