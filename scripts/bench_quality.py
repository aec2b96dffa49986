"""Benchmark of the per-allele quality sums (csrc/bases.hip).

    python scripts/bench_quality.py [--reads N] [--contigs C] [--length L] [--batch B] [--rounds R]
                                    [--parent-lib metacov_amd/variants/lib_parent.so]
                                    [--layout-lib metacov_amd/variants/lib_q2048.so]
                                    [--out profiles/quality_bench.json]

Workload: scripts/bench_bases.py's (C contigs of L positions, N reads of 150
bases, 1 % mismatches, 2 % 2-base deletions, 2 % 2-base insertions, qualities
20..40, B reads per batch, segments = whole contigs), every read with a MAPQ
drawn from 0..60, seeded.  The batches are generated once and kept on the host.

One process.  After one untimed pass of every variant, R rounds alternate
  plain     begin(), add_reads() of every batch: the plain pileup kernel
  parent    `plain` through another build of the library (--parent-lib: the
            parent commit's sources built by `python -m metacov_amd.build` in
            an export of that commit; left out when the file is absent)
  quality   begin(quality=True), add_reads(..., mapq=...): the quality kernel
  layout    `quality` through a build of this tree with another LDS layout of
            the quality kernel (--layout-lib: kQTile of csrc/bases.hip set to
            2048, one 96 KiB workgroup per tile, or to 512, four of 24 KiB;
            left out when the file is absent); its planes and sums must equal
            `quality`'s
and record, per pass, the HIP-event times of the pre-pass and the pileup
kernels summed over the batches (mc_bases_timing) and of one sites call
(plain: mc_bases_sites; quality: mc_bases_sites_quality with thresholds 0 / 0
and 30 / 30).  Reported: every pass, the medians, the spread (max - min)
between the repeats of one variant, quality / plain (recorded, no bar: nothing
computed these sums before), and the condition on the plain kernel: this
build's median within the spread of the parent's.  The quality pass's count
planes must equal the plain pass's, and the totals of its two sum sets what
the host adds up from the batches.

Then scripts/bench_bases_decode.py's synthetic BAM: add_bam(decode="gpu") with
and without quality, alternating, wall clock; and the decoder's parse step
(mc_bam_gpu_stats' parse_ms, which holds the fill walk that writes the mapq
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
EVENTS = np.array([150, 152, 148], np.int64)        # counts a read of bench_bases' kind 0 / 1 / 2 makes


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
    ap.add_argument("--layout-lib", default=os.path.join(ROOT, "metacov_amd", "variants", "lib_q2048.so"))
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--out", default=None, help="also write the result to this file")
    return ap.parse_args(argv)


def stats(xs):
    return {"runs": [round(x, 4) for x in xs], "median": statistics.median(xs), "spread": max(xs) - min(xs)}


def feed(bc, batches, mapqs=None):
    for k, b in enumerate(batches):
        bc.add_reads(b["tid"], b["pos"], b["cig_off"], b["cigar"], b["l_seq"], b["seq_off"], b["seq"], b["qual_off"],
                     b["qual"], **({} if mapqs is None else {"mapq": mapqs[k]}))


def planes_equal(get_a, get_b, n):
    return all(np.array_equal(get_a(o, min(CHUNK, n - o)), get_b(o, min(CHUNK, n - o))) for o in range(0, n, CHUNK))


def quality_sums(bc, n):
    """(sum of bq, sum of mq, sum of bq[DEL]) over all positions."""
    sb = sm = sd = 0
    for o in range(0, n, CHUNK):
        bq, mq = bc.quality(o, min(CHUNK, n - o))
        sb += int(bq.astype(np.int64).sum())
        sm += int(mq.astype(np.int64).sum())
        sd += int(bq[5].astype(np.int64).sum())
    return sb, sm, sd


def main(argv=None):
    args = parse(argv)
    import torch
    torch.zeros(1, device="cuda")          # torch's HIP runtime first (tests/conftest.py)
    from bench_bases import make_batch
    from metacov_amd import _lib
    from metacov_amd import bases as mb
    parent = _lib.load(args.parent_lib) if os.path.exists(args.parent_lib) else None
    layout = _lib.load(args.layout_lib) if os.path.exists(args.layout_lib) else None
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
    made = [make_batch(rng, ref, all_tid[a:a + args.batch], all_pos[a:a + args.batch])
            for a in range(0, n_reads, args.batch)]
    batches = [m[0] for m in made]
    mapqs = [rng.integers(0, 61, size=len(b["tid"]), dtype=np.uint8) for b in batches]
    # what the sums must add up to: every aligned base is counted (min_baseq 0, the reads lie inside the contigs),
    # the two inserted bases of kind 2 (query 70 and 71) are not
    want_bq = want_mq = 0
    for (b, kind, _), m in zip(made, mapqs):
        q = b["qual"].reshape(-1, 150)
        want_bq += int(q.sum(dtype=np.int64)) - int(q[kind == 2, 70:72].sum(dtype=np.int64))
        want_mq += int((m.astype(np.int64) * EVENTS[kind]).sum())
    del made
    gen_s = time.perf_counter() - t0

    counters = {"plain": mb.BaseCounter(nc, 0), "quality": mb.BaseCounter(nc, 0)}
    if parent is not None:
        counters["parent"] = mb.BaseCounter(nc, 0, lib=parent)
    if layout is not None:
        counters["layout"] = mb.BaseCounter(nc, 0, lib=layout)
    order = [v for v in ("plain", "parent", "quality", "layout") if v in counters]
    pile = {v: [] for v in order}
    pre = {v: [] for v in order}
    sites_ms = {"plain": [], "quality_0_0": [], "quality_30_30": []}
    if parent is not None:
        sites_ms["parent"] = []
    n_sites = {}
    layout_error = None
    for rnd in range(args.rounds + 1):          # round 0 warms up
        for v in order:
            if v == "layout" and layout_error:
                continue
            bc = counters[v]
            with_q = v in ("quality", "layout")
            bc.begin(tids, starts, ends, **({"quality": True} if with_q else {}))
            try:
                feed(bc, batches, mapqs if with_q else None)
            except _lib.MetacovError as e:
                if v != "layout":
                    raise
                layout_error = str(e)           # (a 96 KiB workgroup the device will not launch)
                continue
            t = bc.timing()
            if v == "quality":
                s0 = bc.sites(10, 2, 20000)
                k0 = bc.timing()["sites_ms"]
                s2 = bc.sites(10, 2, 20000, min_alt_baseq=30, min_alt_mapq=30)
                k2 = bc.timing()["sites_ms"]
                n_sites["quality_0_0"], n_sites["quality_30_30"] = len(s0), len(s2)
            elif v != "layout":
                n_sites[v] = len(bc.sites(10, 2, 20000))
                k0 = bc.timing()["sites_ms"]
            if rnd:
                pile[v].append(t["pileup_ms"])
                pre[v].append(t["prepass_ms"])
                if v == "layout":
                    pass
                elif v == "quality":
                    sites_ms["quality_0_0"].append(k0)
                    sites_ms["quality_30_30"].append(k2)
                else:
                    sites_ms[v].append(k0)
    plain, quality = counters["plain"], counters["quality"]
    counts_equal = planes_equal(plain.counts, quality.counts, n_pos)
    parent_equal = None if parent is None else planes_equal(plain.counts, counters["parent"].counts, n_pos)
    got_bq, got_mq, got_del = quality_sums(quality, n_pos)
    layout_equal = None
    if layout_error:
        layout = None
    if layout is not None:
        alt = counters["layout"]
        layout_equal = planes_equal(quality.counts, alt.counts, n_pos) and all(
            np.array_equal(x, y) for o in range(0, n_pos, CHUNK)
            for x, y in zip(quality.quality(o, min(CHUNK, n_pos - o)), alt.quality(o, min(CHUNK, n_pos - o))))
    for bc in counters.values():
        bc.close()

    med = statistics.median
    ratio = med(pile["quality"]) / med(pile["plain"])
    result = {
        "metric": "per-allele quality sums: quality pileup time over plain pileup time (csrc/bases.hip), 1 MI355X",
        "value": ratio, "unit": "x (medians of HIP-event times summed over the batches); recorded, no bar",
        "n_gpus": 1, "higher_is_better": False, "date": time.strftime("%Y-%m-%d"),
        "data": "synthetic (host-generated, scripts/bench_bases.py's workload, qualities 20..40, MAPQ 0..60)",
        "config": {"workload": "%d contigs x %d positions, %d x 150-base reads, %d reads per batch, segments = whole "
                               "contigs" % (nc, L, n_reads, args.batch),
                   "rounds": args.rounds, "warmup_rounds": 1, "order_in_a_round": order, "generate_s": round(gen_s, 2),
                   "quality_kernel": dict(zip(("positions_per_workgroup", "reads_per_flush"), mb.quality_dims()))},
        "pileup_ms": {v: stats(pile[v]) for v in order if pile[v]},
        "prepass_ms": {v: stats(pre[v]) for v in order if pre[v]},
        "sites_ms": {v: stats(x) for v, x in sites_ms.items()},
        "n_sites": n_sites,
        "quality_over_plain": {"pileup": ratio, "sites_0_0": med(sites_ms["quality_0_0"]) / med(sites_ms["plain"]),
                               "sites_30_30": med(sites_ms["quality_30_30"]) / med(sites_ms["plain"])},
        "checks": {"counts_equal_plain": bool(counts_equal), "bq_sum": got_bq, "bq_sum_expected": want_bq,
                   "mq_sum": got_mq, "mq_sum_expected": want_mq, "bq_del_sum": got_del,
                   "sums_as_expected": got_bq == want_bq and got_mq == want_mq and got_del == 0,
                   "sites_0_0_equal_plain": n_sites["quality_0_0"] == n_sites["plain"],
                   "parent_planes_equal": parent_equal, "layout_planes_and_sums_equal": layout_equal},
    }
    if layout_error:
        result["lds_layouts"] = {"other_failed": layout_error}
        result["pileup_ms"].pop("layout", None)
        result["prepass_ms"].pop("layout", None)
    if layout is not None:
        result["lds_layouts"] = {
            "kept": "1024 positions per workgroup, 48 KiB, two workgroups per tile",
            "other": "%d positions per workgroup, %d KiB (--layout-lib)" % (mb.quality_dims(layout)[0],
                                                                            mb.quality_dims(layout)[0] * 48 // 1024),
            "other_dims": dict(zip(("positions_per_workgroup", "reads_per_flush"), mb.quality_dims(layout))),
            "pileup_ms_kept": med(pile["quality"]), "pileup_ms_other": med(pile["layout"]),
            "other_over_kept": med(pile["layout"]) / med(pile["quality"])}
    if parent is not None:
        d = med(pile["plain"]) - med(pile["parent"])
        result["plain_against_parent"] = {
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
    bad = [k for k in ("counts_equal_plain", "sums_as_expected", "sites_0_0_equal_plain") if not result["checks"][k]]
    if bad or parent_equal is False or layout_equal is False:
        raise SystemExit("results differ: %s" % (bad or "parent or layout planes"))


def bench_decode(args, mb, parent):
    from metacov_amd import synth
    nc, L = args.contigs, args.length
    lengths = [L] * nc
    names = ["contig_%d" % (i + 1) for i in range(nc)]
    tids, starts, ends = np.arange(nc, dtype=np.int32), np.zeros(nc, np.int64), np.full(nc, L, np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "quality_bench.bam")
        synth.write_bam_fast(path, names, lengths, *synth.edge_mix_arrays(lengths, args.reads, seed=args.seed), level=1,
                             n_threads=args.threads)
        wall = {"plain": [], "quality": []}
        kern = {"plain": [], "quality": []}
        parse_ms = {"this": [], "parent": []}
        with mb.BaseCounter(nc, 0) as bc:
            for rnd in range(args.rounds + 1):  # round 0 warms up
                for v in ("plain", "quality"):
                    bc.begin(tids, starts, ends, quality=v == "quality")
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
            bq_sum, mq_sum, _ = quality_sums(bc, nc * L)
        size = os.path.getsize(path)
    return {"data": "synthetic BAM (synth.write_bam_fast, edge mix, BGZF level 1; scripts/bench_bases_decode.py's)",
            "bam_bytes": size, "add_bam_gpu_s": {v: stats(wall[v]) for v in wall},
            "pileup_ms": {v: stats(kern[v]) for v in kern},
            "quality_over_plain_wall": statistics.median(wall["quality"]) / statistics.median(wall["plain"]),
            "decode_parse_ms": {k: stats(v) for k, v in parse_ms.items() if v},
            "bq_sum": bq_sum, "mq_sum": mq_sum}


if __name__ == "__main__":
    main()
