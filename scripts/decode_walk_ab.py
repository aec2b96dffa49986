"""A/B of the GPU decode's record walks: parse_ms of two builds, all four modes.

    python scripts/decode_walk_ab.py --make X.bam
    METACOV_AMD_LIB=<other build> python scripts/decode_walk_ab.py --bam X.bam --out DIR/parent_1.json [--hash]
    python scripts/decode_walk_ab.py --bam X.bam --out DIR/head_1.json [--hash]
    ... (alternately, one process per run, rounds 1..R)
    python scripts/decode_walk_ab.py --merge DIR --rounds R --out profiles/decode_walk_refactor_ab.json

--make writes the workload of scripts/bench_bases_decode.py (10 M reads, 100
contigs, BGZF level 1).  A run decodes it resident in each mode (intervals,
scan, reads, bases): one untimed warm-up decode (with --hash: SHA-256 of
every column of its tables, copied from the device), then --runs timed
decodes, and records parse_ms (the walks, their host checks and the fill) and
the round counters of mc_bam_gpu_stats.  --merge applies the rule of
profiles/bases_refactor_ab.json: per mode, head's median inside the parent's
run-to-run spread (max - min of its per-process medians), or faster; and the
hashed tables of round 1 equal.
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("intervals", "scan", "reads", "bases")


def hip_runtime():
    """The HIP runtime the library brought into the process (for the copies of device columns)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise SystemExit("no HIP runtime loaded")


def open_mode(lib, L, mode, path):
    p, g = path.encode(), ctypes.c_void_p()
    rc = {"intervals": lambda: lib.mc_bam_gpu_open(p, 0, 16, 0x704, 0, ctypes.byref(g)),
          "scan": lambda: lib.mc_bam_gpu_open_scan(p, 0, 16, 0, ctypes.byref(g)),
          "reads": lambda: lib.mc_bam_gpu_open_reads(p, 0, 16, 5, 0, ctypes.byref(g)),
          "bases": lambda: lib.mc_bam_gpu_open_bases(p, 0, 16, 0x704, 0, 0, ctypes.byref(g))}[mode]()
    L.check(rc, lib)
    return g


def columns(lib, L, mode, g):
    """([(name, device pointer, bytes)], sizes) of the mode's tables."""
    P, I, b = ctypes.c_void_p, ctypes.c_int64, ctypes.byref
    n = I()
    if mode == "intervals":
        c = [P() for _ in range(3)]
        L.check(lib.mc_bam_gpu_intervals_device(g, b(n), *map(b, c)), lib)
        return list(zip(("tid", "pos", "span"), c, [n.value * 4] * 3)), {"n": n.value}
    if mode == "scan":
        c, sb = [P() for _ in range(7)], I()
        L.check(lib.mc_bam_gpu_scan_device(g, b(n), *map(b, c), b(sb)), lib)
        names = ("rlen", "flag", "gpos", "gisize", "tid", "seq_off", "seq")
        return list(zip(names, c, [n.value * 4] * 5 + [(n.value + 1) * 8, sb.value])), \
            {"n": n.value, "seq_bytes": sb.value}
    if mode == "reads":
        c, nb = [P() for _ in range(9)], I()
        L.check(lib.mc_bam_gpu_reads_device(g, b(n), *map(b, c), b(nb)), lib)
        names = ("tid", "pos", "end", "flag", "bits", "kmer", "name_len", "name_off", "names")
        k = n.value
        return list(zip(names, c, [k * 4, k * 4, k * 8, k * 4, k, k * 4, k, k * 8, nb.value])), \
            {"n": k, "name_bytes": nb.value}
    tid, pos, co, cg, ls, so, sq, qo, ql, fl, mq = (P() for _ in range(11))
    nw, sb, qb = I(), I(), I()
    L.check(lib.mc_bam_gpu_bases_device(g, b(n), b(tid), b(pos), b(co), b(cg), b(nw), b(ls), b(so), b(sq), b(sb), b(qo),
                                        b(ql), b(qb)), lib)
    L.check(lib.mc_bam_gpu_bases_flags(g, b(fl)), lib)
    L.check(lib.mc_bam_gpu_bases_mapq(g, b(mq)), lib)
    cnt = [I() for _ in range(4)]
    L.check(lib.mc_bam_gpu_bases_counts(g, *map(b, cnt)), lib)
    k = n.value
    cols = [("tid", tid, k * 4), ("pos", pos, k * 4), ("cig_off", co, (k + 1) * 8), ("cigar", cg, nw.value * 4),
            ("l_seq", ls, k * 4), ("seq_off", so, (k + 1) * 8), ("seq", sq, sb.value), ("qual_off", qo, (k + 1) * 8),
            ("qual", ql, qb.value), ("flag", fl, k * 2), ("mapq", mq, k)]
    return cols, {"n": k, "n_words": nw.value, "seq_bytes": sb.value, "qual_bytes": qb.value,
                  "counts": [c.value for c in cnt]}


def hashes(lib, L, mode, g, hip):
    cols, out = columns(lib, L, mode, g)
    for name, ptr, nbytes in cols:
        buf = np.empty(max(nbytes, 1), np.uint8)
        if nbytes:
            rc = hip.hipMemcpy(ctypes.c_void_p(buf.ctypes.data), ptr, ctypes.c_size_t(nbytes), 2)   # device to host
            if rc:
                raise SystemExit("hipMemcpy failed: %d" % rc)
        out[name] = hashlib.sha256(buf[:nbytes]).hexdigest()
    return out


def stats(lib, L, g):
    t = L.GpuDecodeTimings()
    L.check(lib.mc_bam_gpu_stats(g, ctypes.byref(t)), lib)
    return {k: getattr(t, k) for k in ("parse_ms", "inflate_ms", "total_ms", "windows", "resyncs", "parse_rounds",
                                       "resync_passes", "inflated_bytes")}


def make(path):
    from metacov_amd import synth
    lengths = [500_000] * 100
    names = ["contig_%d" % (i + 1) for i in range(100)]
    t0 = time.perf_counter()
    synth.write_bam_fast(path, names, lengths, *synth.edge_mix_arrays(lengths, 10_000_000, seed=1), level=1,
                         n_threads=16)
    print("wrote %s: %d bytes in %.1f s" % (path, os.path.getsize(path), time.perf_counter() - t0), flush=True)


def run(a):
    from metacov_amd import _lib as L
    lib = L.load()
    res = {"lib": os.environ.get("METACOV_AMD_LIB", "the tree's"), "build_id": lib.mc_build_id().decode(),
           "modes": {}}
    hip = None
    for mode in MODES:
        g = open_mode(lib, L, mode, a.bam)            # warm-up, untimed
        m = {"warmup": stats(lib, L, g)}
        if a.hash:
            hip = hip or hip_runtime()
            m["sha256"] = hashes(lib, L, mode, g, hip)
        lib.mc_bam_gpu_close(g)
        m["runs"] = []
        for _ in range(a.runs):
            g = open_mode(lib, L, mode, a.bam)
            m["runs"].append(stats(lib, L, g))
            lib.mc_bam_gpu_close(g)
        res["modes"][mode] = m
        print(mode, [round(r["parse_ms"], 3) for r in m["runs"]], flush=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


def merge(a):
    runs = {s: [json.load(open("%s/%s_%d.json" % (a.merge, s, r))) for r in range(1, a.rounds + 1)]
            for s in ("parent", "head")}
    res = {
        "what": "parse_ms (mc_bam_gpu_stats: the walks, their host checks and the fill) of the one-frame walk_kernel "
                "against the commit before (its build loaded through METACOV_AMD_LIB), alternately, one process per "
                "run, one MI355X; resident decode of scripts/bench_bases_decode.py's file (10 M reads, 100 contigs, "
                "level 1), every mode",
        "commands": ["python scripts/decode_walk_ab.py --make X.bam",
                     "METACOV_AMD_LIB=<parent build> python scripts/decode_walk_ab.py --bam X.bam --out DIR/parent_<r>.json"
                     "   (round 1 of each side with --hash; per mode 1 untimed decode, then %d timed)" % a.runs,
                     "python scripts/decode_walk_ab.py --bam X.bam --out DIR/head_<r>.json",
                     "python scripts/decode_walk_ab.py --merge DIR --rounds %d --out <this file>" % a.rounds],
        "order": "round 1: parent, head; round 2: parent, head; ...",
        "unit": "ms",
        "rule": "head's median of medians within the parent's spread (max - min of its per-process medians), or faster",
        "builds": {side: runs[side][0]["build_id"] for side in runs},
        "series": {},
    }
    ok = True
    for m in MODES:
        s = {}
        for side in ("parent", "head"):
            samples = [[r["parse_ms"] for r in p["modes"][m]["runs"]] for p in runs[side]]
            med = [statistics.median(x) for x in samples]
            s[side] = {"samples": samples, "medians": med, "median": statistics.median(med),
                       "spread": max(med) - min(med)}
        s["head_minus_parent"] = s["head"]["median"] - s["parent"]["median"]
        s["pass"] = s["head_minus_parent"] <= s["parent"]["spread"]
        c = [{k: r[k] for k in ("resyncs", "parse_rounds", "resync_passes", "windows")}
             for side in ("parent", "head") for p in runs[side] for r in p["modes"][m]["runs"]]
        s["round_counters"] = c[0]
        s["round_counters_equal_in_every_run"] = all(x == c[0] for x in c)
        hp, hh = (runs[side][0]["modes"][m].get("sha256") for side in ("parent", "head"))
        s["tables_sha256"] = {"parent": hp, "head": hh, "equal": hp is not None and hp == hh}
        ok &= s["tables_sha256"]["equal"]
        res["series"][m] = s
        print(m, "parent %.3f (spread %.3f) head %.3f  pass %s  tables equal %s" %
              (s["parent"]["median"], s["parent"]["spread"], s["head"]["median"], s["pass"],
               s["tables_sha256"]["equal"]))
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    if not ok:
        raise SystemExit("the tables of the two builds differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make", help="write the workload BAM here and exit")
    ap.add_argument("--bam")
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=5, help="timed decodes per mode")
    ap.add_argument("--hash", action="store_true", help="SHA-256 of every column of the warm-up decode's tables")
    ap.add_argument("--merge", help="folder of parent_<r>.json / head_<r>.json to merge into --out")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.make:
        make(a.make)
    elif a.merge:
        merge(a)
    else:
        run(a)


if __name__ == "__main__":
    main()
