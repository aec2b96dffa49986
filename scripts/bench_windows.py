"""Benchmark of the windowed-coverage kernels (csrc/windows.hip) against the
depth-runs count pass (the same single 4 B/position read of the depth vector)
and against the only other route to the same arrays: copy the depth vector to
the host and reduce it in numpy.

    python scripts/bench_windows.py [--reads N] [--steps K] [--warmup W]
                                    [--out profiles/windows_bench.json]

Workload: bench.py's C3 batch (1000 contigs, ~1.0 Gbp, 100M x ~150 bp reads
generated on the GPU); its depth is computed once (K2).  Every contig over
[0, length).  Three configurations, each the median of --steps HIP-event
timings after --warmup calls (mc_windows_timing):
    window=500 with thresholds 1, 10, 30        (tile kernel; windows inside a tile)
    window=0 over whole contigs                 (tile kernel writing partial rows + combine kernel)
    hist with 1024 bins                         (histogram kernel)
and, in the same process, runs_count_kernel's time from mc_runs_timing.
Algorithmic bytes: 4 B per position read + the rows written (8 (1 + n_thr) B
per window, partial rows written and read again, 8 B per histogram cell).

Host route (what a caller had before): eng.depth(t) for every contig (a
device-to-host copy of 4 B per position), then np.add.reduceat per threshold
and np.bincount; wall clock, one pass.  The results must equal the GPU's.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12      # HBM bytes/s


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000_000)
    ap.add_argument("--contigs", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=int, default=500)
    ap.add_argument("--thresholds", default="1,10,30")
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    return ap.parse_args(argv)


def host_route(eng, lengths, window, thr, n_bins):
    """(sum_w, ge_w, sum_0, ge_0, hist, copy_s, reduce_s): depth to the host
    contig by contig, reduced with numpy."""
    sum_w, ge_w, sum_0, ge_0, hist = [], [], [], [], []
    copy_s = reduce_s = 0.0
    for t, n in enumerate(lengths):
        t0 = time.perf_counter()
        v = eng.depth(t, 0, int(n))
        t1 = time.perf_counter()
        if n:
            at = np.arange(0, n, window)
            flags = [(v >= x).astype(np.int64) for x in thr]
            sum_w.append(np.add.reduceat(v.astype(np.int64), at))
            ge_w.append(np.stack([np.add.reduceat(f, at) for f in flags], axis=1))
            sum_0.append(int(v.sum(dtype=np.int64)))
            ge_0.append([int(f.sum()) for f in flags])
        hist.append(np.bincount(np.minimum(v, n_bins - 1), minlength=n_bins))
        copy_s += t1 - t0
        reduce_s += time.perf_counter() - t1
    return (np.concatenate(sum_w), np.concatenate(ge_w), np.array(sum_0, np.int64),
            np.array(ge_0, np.int64).reshape(len(sum_0), len(thr)), np.array(hist, np.int64), copy_s, reduce_s)


def main(argv=None):
    args = parse(argv)
    import torch
    torch.zeros(1, device="cuda")          # torch's HIP runtime first (tests/conftest.py)
    from bench import config_contigs, device_workload
    from metacov_amd import runs as mruns
    from metacov_amd import windows as mwin
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
    thr = mwin._thresholds(args.thresholds)
    nc = len(lengths)
    tids = np.arange(nc, dtype=np.int32)
    starts = np.zeros(nc, np.int64)
    ends = np.ascontiguousarray(lengths, np.int64)
    positions = int(ends.sum())
    h = mwin.WindowsHandle(0)
    r = mruns.RunsHandle(0)
    no_edges = np.zeros(0, np.int32)

    def timed(call, keys):
        for _ in range(args.warmup):
            call()
        rows = []
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = call()
            rows.append(keys())
        wall = (time.perf_counter() - t0) / max(1, args.steps)
        return out, {k: float(np.median([x[k] for x in rows])) for k in rows[0]}, wall, rows[-1]

    _, runs_ms, _, _ = timed(lambda: r.compute(eng._h, tids, starts, ends, no_edges), r.timing)
    count_ms = runs_ms["count_ms"]
    (n_w, _), w_ms, w_wall, w_last = timed(lambda: h.compute(eng._h, tids, starts, ends, args.window, thr),
                                           h.timing)
    sum_w, ge_w = h.get(0, n_w)
    (n_0, _), z_ms, z_wall, z_last = timed(lambda: h.compute(eng._h, tids, starts, ends, 0, thr), h.timing)
    sum_0, ge_0 = h.get(0, n_0)
    hist, h_ms, h_wall, _ = timed(lambda: h.hist(eng._h, tids, starts, ends, args.bins), h.timing)
    row = 8 * (1 + len(thr))

    def entry(what, kernel_ms, wall, alg, extra):
        return dict({"what": what, "kernels_ms": kernel_ms, "total_ms": sum(kernel_ms.values()),
                     "vs_runs_count_pass": sum(kernel_ms.values()) / count_ms, "call_ms": wall * 1e3,
                     "algorithmic_bytes": alg, "achieved_GBps": alg / (sum(kernel_ms.values()) * 1e-3) / 1e9,
                     "frac_of_hbm_peak": alg / (sum(kernel_ms.values()) * 1e-3) / PEAK}, **extra)

    pieces_0 = z_last["tiles"]
    configs = {
        "window": entry("window=%d, thresholds %s" % (args.window, args.thresholds),
                        {"window_ms": w_ms["window_ms"], "combine_ms": w_ms["combine_ms"]}, w_wall,
                        4 * positions + row * n_w, {"windows": int(n_w), "tiles": w_last["tiles"]}),
        "whole_contigs": entry("window=0 over whole contigs, thresholds %s" % args.thresholds,
                               {"window_ms": z_ms["window_ms"], "combine_ms": z_ms["combine_ms"]}, z_wall,
                               4 * positions + 2 * row * pieces_0 + row * n_0,
                               {"windows": int(n_0), "tiles": pieces_0}),
        "hist": entry("hist, %d bins" % args.bins, {"hist_ms": h_ms["hist_ms"]}, h_wall,
                      4 * positions + 8 * nc * args.bins, {"cells": nc * args.bins}),
    }
    line = {
        "metric": "windowed coverage: positions/sec through the window kernel (csrc/windows.hip), 1 MI355X",
        "value": positions / (configs["window"]["total_ms"] * 1e-3), "unit": "positions/s", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "higher_is_better": True, "dtype": "int32",
        "data": "synthetic (bench.py's GPU-generated C3 batch)",
        "config": {"workload": "C3: %d contigs (%.3f Gbp), %d x ~150 bp reads, every contig over [0, length)"
                               % (nc, positions / 1e9, args.reads), "generate_s": round(gen_s, 2),
                   "timing": "median of %d HIP-event timings after %d warm-up calls" % (args.steps, args.warmup)},
        "positions": positions,
        "runs_count_pass_ms": count_ms,
        "runs_count_pass_frac_of_hbm_peak": 4 * positions / (count_ms * 1e-3) / PEAK,
        "configs": configs,
    }
    if not args.no_host_route:
        t0 = time.perf_counter()
        hs_w, hg_w, hs_0, hg_0, hh, copy_s, reduce_s = host_route(eng, lengths, args.window, thr, args.bins)
        total_s = time.perf_counter() - t0
        same = {"window": bool(np.array_equal(hs_w, sum_w) and np.array_equal(hg_w, ge_w)),
                "whole_contigs": bool(np.array_equal(hs_0, sum_0) and np.array_equal(hg_0, ge_0)),
                "hist": bool(np.array_equal(hh, hist))}
        gpu_s = sum(c["total_ms"] for c in configs.values()) * 1e-3
        line["host_route"] = {"total_s": total_s, "depth_copy_s": copy_s, "numpy_reduce_s": reduce_s,
                              "what": "eng.depth(t) per contig + np.add.reduceat / np.bincount", "agrees": same}
        line["vs_host_route"] = {"kernels": total_s / gpu_s}
        if not all(same.values()):
            print(json.dumps(line))
            raise SystemExit("the GPU results differ from the host route")
    h.close()
    r.close()
    eng.close()
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
