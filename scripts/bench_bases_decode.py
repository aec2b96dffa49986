"""Benchmark of the two record sources of the base counter.

    python scripts/bench_bases_decode.py [--reads N] [--contigs C] [--length L] [--runs R] [--threads T]
                                         [--bam X.bam] [--out profiles/bases_decode_bench.json]

Workload: a synthetic coordinate-sorted BAM written with synth.write_bam_fast
(edge-mix CIGARs and flags, 150-base reads, bases 'A', qualities 30, BGZF
level 1; scripts/bench_bases.py's shape: 100 contigs x 500 kbp, 10 M reads),
segments = whole contigs.  The file is written once and stays in the page
cache, so neither path waits for a disk.  Its payload is uniform, so it
deflates far better than real reads: the inflate times are those of this
file, not of a sequencer's.

Timed, after one untimed warm-up run of each path (code objects load at the
first launch), over R runs each (every run listed, the median reported):
BaseCounter.add_bam end to end (wall clock around the call, which returns
after its kernels) with decode="host" (the unchanged host source: the
baseline) and decode="gpu"; of the GPU path also the decode alone
(GpuBaseSource: wall clock, and the decoder's own read / inflate / parse
times, mc_bam_gpu_stats: host clocks around synchronised steps; for a
resident decode inflate_ms spans the pieces' uploads and inflate launches,
"windows" counts those pieces, and parse_ms holds the walks, the arena
allocations and the gather), add_device alone, and the pre-pass and pileup kernels by
HIP events (mc_bases_timing).  For what the gather costs over a walk that
copies nothing: parse_ms of an interval-mode decode (mc_bam_gpu_open) of the
same file.  The planes of the two paths must be equal.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 1 << 24


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--contigs", type=int, default=100)
    ap.add_argument("--length", type=int, default=500_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16, help="host threads of both paths and of the BAM writer")
    ap.add_argument("--bam", default=None, help="keep the BAM here (default: a temporary file)")
    ap.add_argument("--out", default=None, help="also write the result to this file")
    return ap.parse_args(argv)


def planes_equal(a, b, n):
    return all(np.array_equal(a.counts(o, min(CHUNK, n - o)), b.counts(o, min(CHUNK, n - o)))
               for o in range(0, n, CHUNK))


def interval_decode(lib, path):
    from metacov_amd import _lib
    g = ctypes.c_void_p()
    t0 = time.perf_counter()
    _lib.check(lib.mc_bam_gpu_open(path.encode(), 0, 0, 0x704, 0, ctypes.byref(g)), lib)
    wall = time.perf_counter() - t0
    t = _lib.GpuDecodeTimings()
    _lib.check(lib.mc_bam_gpu_stats(g, ctypes.byref(t)), lib)
    lib.mc_bam_gpu_close(g)
    return {"open_wall_ms": wall * 1e3, "read_ms": t.read_ms, "inflate_ms": t.inflate_ms, "parse_ms": t.parse_ms}


def main(argv=None):
    args = parse(argv)
    import torch
    torch.zeros(1, device="cuda")          # torch's HIP runtime first (tests/conftest.py)
    from metacov_amd import _lib, synth
    from metacov_amd import bases as mb
    lib = _lib.load()
    nc, L = args.contigs, args.length
    lengths = [L] * nc
    names = ["contig_%d" % (i + 1) for i in range(nc)]
    tmp = None
    path = args.bam
    if path is None:
        tmp = tempfile.TemporaryDirectory()
        path = os.path.join(tmp.name, "bases_decode_bench.bam")
    t0 = time.perf_counter()
    synth.write_bam_fast(path, names, lengths, *synth.edge_mix_arrays(lengths, args.reads, seed=args.seed), level=1,
                         n_threads=args.threads)
    write_s = time.perf_counter() - t0
    tids = np.arange(nc, dtype=np.int32)
    starts = np.zeros(nc, np.int64)
    ends = np.full(nc, L, np.int64)
    n_pos = nc * L

    host_bc, gpu_bc = mb.BaseCounter(nc, 0), mb.BaseCounter(nc, 0)
    host_s, gpu_s, decode_s, add_s, decode_t, kernels = [], [], [], [], [], []
    counts = {}
    for run in range(args.runs + 1):            # run 0 warms up
        host_bc.begin(tids, starts, ends)
        t0 = time.perf_counter()
        counts["host"] = host_bc.add_bam(path, n_threads=args.threads)
        h = time.perf_counter() - t0
        gpu_bc.begin(tids, starts, ends)
        t0 = time.perf_counter()
        counts["gpu"] = gpu_bc.add_bam(path, n_threads=args.threads, decode="gpu")
        g = time.perf_counter() - t0
        # the same again in its two halves
        gpu_bc.begin(tids, starts, ends)
        t0 = time.perf_counter()
        src = mb.GpuBaseSource(path, 0, args.threads)
        d = time.perf_counter() - t0
        t0 = time.perf_counter()
        gpu_bc.add_device(src)
        a = time.perf_counter() - t0
        dt = src.timings()
        table = {"reads": len(src), "cigar_words": src.n_words, "seq_bytes": src.seq_bytes,
                 "qual_bytes": src.qual_bytes}
        src.close()
        if run:
            host_s.append(h)
            gpu_s.append(g)
            decode_s.append(d)
            add_s.append(a)
            decode_t.append({k: dt[k] for k in ("read_ms", "inflate_ms", "parse_ms", "total_ms", "windows",
                                                "resyncs", "parse_rounds")})
            kt = gpu_bc.timing()
            kernels.append({"prepass_ms": kt["prepass_ms"], "pileup_ms": kt["pileup_ms"]})
    equal = planes_equal(host_bc, gpu_bc, n_pos)
    host_kt = host_bc.timing()
    host_bc.close()
    gpu_bc.close()
    interval = [interval_decode(lib, path) for _ in range(args.runs + 1)][1:]
    size = os.path.getsize(path)
    if tmp is not None:
        tmp.cleanup()

    med = statistics.median
    line = {
        "metric": "base counts end to end from a BAM: add_bam(decode='gpu') against add_bam(decode='host'), 1 MI355X",
        "value": med(host_s) / med(gpu_s), "unit": "x (host seconds / gpu seconds, medians)", "n_gpus": 1,
        "higher_is_better": True, "date": time.strftime("%Y-%m-%d"),
        "data": "synthetic (synth.write_bam_fast: bases 'A', qualities 30, BGZF level 1; in the page cache)",
        "config": {"workload": "%d contigs x %d positions, %d x 150-base reads (edge mix), segments = whole contigs"
                               % (nc, L, args.reads),
                   "bam_bytes": size, "inflated_bytes": dt["inflated_bytes"], "write_s": round(write_s, 2),
                   "runs": args.runs, "warmup_runs": 1, "host_threads": args.threads},
        "records": counts["gpu"], "table": table,
        "host": {"add_bam_s": host_s, "median_s": med(host_s),
                 "kernels_ms_last_run": {"prepass": host_kt["prepass_ms"], "pileup": host_kt["pileup_ms"]}},
        "gpu": {"add_bam_s": gpu_s, "median_s": med(gpu_s), "decode_open_s": decode_s, "add_device_s": add_s,
                "decode": decode_t, "kernels_ms": kernels},
        "interval_mode_decode_same_file": interval,
        "gather_cost": {"bases_parse_ms_median": med(t["parse_ms"] for t in decode_t),
                        "interval_parse_ms_median": med(t["parse_ms"] for t in interval)},
        "counts_equal": counts["host"] == counts["gpu"], "planes_equal": bool(equal),
    }
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    if not equal or counts["host"] != counts["gpu"]:
        raise SystemExit("the GPU-decoded planes or counts differ from the host path's")


if __name__ == "__main__":
    main()
