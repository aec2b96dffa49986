"""Benchmark of the depth-runs kernels (csrc/runs.hip) against the only other
route to the same arrays: copy the depth vector to the host and run-length
encode it in numpy.

    python scripts/bench_runs.py [--reads N] [--steps K] [--warmup W] [--quantize SPEC]
                                 [--out profiles/runs_bench.json]

Workload: bench.py's C3 batch (1000 contigs, ~1.0 Gbp, 100M x ~150 bp reads
generated on the GPU); its depth is computed once (K2).  One step = one
mc_runs_compute over every contig's [0, length): the count, scan and emit
launches, timed by HIP events on the handle's stream (mc_runs_timing).
Algorithmic bytes per step = 2 reads of the depth vector (4 B per position
each) + 12 B per run written.

Host route (what a caller had before): eng.depth(t) for every contig (a
device-to-host copy of 4 B per position), then np.flatnonzero(np.diff(v)) per
contig; wall clock, one pass.  The two results are compared: seg_first, start
and value must be equal.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000_000)
    ap.add_argument("--contigs", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--quantize", default=None, help="mosdepth spec, e.g. 0:1:4:100: (default: none)")
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    return ap.parse_args(argv)


def host_route(eng, lengths, edges):
    """(seg_first, start, value, copy_s, encode_s): depth to the host contig
    by contig, run-length encoded with numpy."""
    seg_first = np.zeros(len(lengths) + 1, np.int64)
    starts, values = [], []
    copy_s = encode_s = 0.0
    for t, n in enumerate(lengths):
        t0 = time.perf_counter()
        v = eng.depth(t, 0, int(n))
        t1 = time.perf_counter()
        if len(edges):
            v = np.searchsorted(edges, v, side="right").astype(np.int32)
        first = np.concatenate([[0], np.flatnonzero(np.diff(v) != 0) + 1]) if n else np.zeros(0, np.int64)
        starts.append(first)
        values.append(v[first])
        seg_first[t + 1] = seg_first[t] + len(first)
        copy_s += t1 - t0
        encode_s += time.perf_counter() - t1
    return (seg_first, np.concatenate(starts).astype(np.int64), np.concatenate(values).astype(np.int32),
            copy_s, encode_s)


def main(argv=None):
    args = parse(argv)
    import torch
    torch.zeros(1, device="cuda")          # torch's HIP runtime first (tests/conftest.py)
    from bench import config_contigs, device_workload
    from metacov_amd import runs as mruns
    from metacov_amd.engine import CoverageEngine
    dev = torch.device("cuda", 0)
    lengths, weights = config_contigs("c3", args.reads, args.contigs)
    t0 = time.time()
    tid, pos, span, _ = device_workload(torch, lengths, weights, args.reads, 1, dev)
    torch.cuda.synchronize()
    gen_s = time.time() - t0
    eng = CoverageEngine(0)
    eng.set_contigs(lengths)
    eng.add_reads(tid, pos, span)
    eng.compute_depth()
    eng.synchronize()
    del tid, pos, span
    edges = mruns._edges(args.quantize)
    nc = len(lengths)
    tids = np.arange(nc, dtype=np.int32)
    starts = np.zeros(nc, np.int64)
    ends = np.ascontiguousarray(lengths, np.int64)
    positions = int(ends.sum())
    h = mruns.RunsHandle(0)
    for _ in range(args.warmup):
        h.compute(eng._h, tids, starts, ends, edges)
    rows = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        n_runs, seg_first = h.compute(eng._h, tids, starts, ends, edges)
        rows.append(h.timing())
    wall = (time.perf_counter() - t0) / max(1, args.steps)
    ms = {k: float(np.mean([r[k] for r in rows])) for k in ("count_ms", "scan_ms", "emit_ms")}
    kern_ms = sum(ms.values())
    alg = 2 * 4 * positions + 12 * n_runs
    t0 = time.perf_counter()
    start, value = h.get(0, n_runs)
    fetch_s = time.perf_counter() - t0
    line = {
        "metric": "depth runs: positions/sec through count + scan + emit (csrc/runs.hip), 1 MI355X",
        "value": positions / (kern_ms * 1e-3), "unit": "positions/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "higher_is_better": True, "dtype": "int32",
        "data": "synthetic (bench.py's GPU-generated C3 batch)",
        "config": {"workload": "C3: %d contigs (%.3f Gbp), %d x ~150 bp reads, every contig over "
                               "[0, length), quantize %s" % (nc, positions / 1e9, args.reads, args.quantize),
                   "generate_s": round(gen_s, 2)},
        "positions": positions, "runs": int(n_runs), "tiles": rows[-1]["tiles"],
        "kernels_ms": dict(ms, total=kern_ms),
        "call_ms": wall * 1e3,
        "fetch_runs_to_host_s": fetch_s,
        "roofline": {"bound": "hbm", "achieved": alg / (kern_ms * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s",
                     "frac": alg / (kern_ms * 1e-3) / 8e12, "algorithmic_bytes_per_step": alg,
                     "note": "2 x 4 B per position read + 12 B per run written, over the three kernels' time"},
    }
    if not args.no_host_route:
        t0 = time.perf_counter()
        sf, s, v, copy_s, encode_s = host_route(eng, lengths, edges)
        total_s = time.perf_counter() - t0
        same = (np.array_equal(sf, seg_first) and np.array_equal(s, start) and np.array_equal(v, value))
        line["host_route"] = {"total_s": total_s, "depth_copy_s": copy_s, "numpy_encode_s": encode_s,
                              "what": "eng.depth(t) per contig + np.flatnonzero(np.diff(v))", "agrees": bool(same)}
        line["vs_host_route"] = {"kernels": total_s / (kern_ms * 1e-3),
                                 "call_plus_fetch": total_s / (wall + fetch_s)}
        if not same:
            print(json.dumps(line))
            raise SystemExit("the GPU runs differ from the host route")
    h.close()
    eng.close()
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
