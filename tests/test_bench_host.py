"""bench.py's host-side pieces that need no GPU: the all-cores CPU
baseline's thread choice (cgroup quota, not the oversubscribed affinity set)
and its sweep record, and what --dump-outputs writes."""
import numpy as np

import bench
from oracle.coracle import STAT_DTYPE


def test_cpu_thread_counts_follow_the_quota(monkeypatch):
    monkeypatch.setattr(bench, "affinity_cpus", lambda: 256)
    monkeypatch.setattr(bench, "cpu_quota", lambda: 16.0)
    assert bench.cpu_thread_counts() == [16, 32, 256]
    monkeypatch.setattr(bench, "cpu_quota", lambda: None)
    monkeypatch.setenv("OMP_NUM_THREADS", "16")
    assert bench.cpu_thread_counts() == [16, 32, 256]
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert bench.cpu_thread_counts() == [256]
    assert bench.cpu_thread_counts(explicit=7) == [7]
    monkeypatch.setattr(bench, "affinity_cpus", lambda: 8)
    monkeypatch.setattr(bench, "cpu_quota", lambda: 2.5)
    assert bench.cpu_thread_counts() == [2, 4, 8]


def test_cpu_baseline_parallel_reports_the_sweep(lib_built):
    rng = np.random.default_rng(0)
    lengths = np.array([5_000, 3_000, 7_000], np.int64)
    tid = np.repeat(np.arange(3, dtype=np.int32), 400)
    pos = np.concatenate([np.sort(rng.integers(0, L - 100, 400)) for L in lengths]).astype(np.int32)
    span = np.full(len(tid), 100, np.int32)
    r = bench.cpu_baseline_parallel(lengths, tid, pos, span, [1, 2], min_s=0.01)
    assert [x["threads"] for x in r["sweep"]] == [1, 2]
    assert r["cores"] in (1, 2) and r["value"] == max(x["value"] for x in r["sweep"])
    assert "cpu_quota" in r and r["unit"] == "aligned bases/s"


def test_depth_sample_windows_whole_or_seeded():
    small = np.array([1000, 1, 70_000], np.int64)
    assert bench.depth_sample_windows(small) == [(0, 0, 1000), (1, 0, 1), (2, 0, 70_000)]
    big = np.array([5_000_000, 3, 100, 9_000_000], np.int64)   # more than the budget: a sample
    w = bench.depth_sample_windows(big)
    assert w == bench.depth_sample_windows(big.copy())          # fixed seed: the same windows every run
    assert len(w) == 256 and sum(e - s for _, s, e in w) <= bench.DUMP_DEPTH_POSITIONS
    for t, s, e in w:
        assert 0 <= s < e <= big[t] and e - s == min(bench.DUMP_DEPTH_POSITIONS // 256, big[t])
    w2 = bench.depth_sample_windows(big, budget=512)             # contigs shorter than a window: whole
    assert all(e - s == min(2, big[t]) for t, s, e in w2)


def test_dump_outputs_writes_float64_npy(tmp_path):
    rows = np.zeros(3, dtype=STAT_DTYPE)
    rows["n"] = [5, 6, 7]
    rows["sumsq"] = [1, 2, 2 ** 40]
    rows["min"] = [-1, 0, 3]
    depth = np.arange(10, dtype=np.int32)
    out = tmp_path / "a" / "b"                                   # created on demand
    bench.dump_outputs(str(out), rows, depth)
    t = np.load(out / "region_stats.npy")
    d = np.load(out / "depth.npy")
    assert t.dtype == np.float64 and t.shape == (3, 9)
    assert t[:, 0].tolist() == [5, 6, 7] and t[2, 2] == 2.0 ** 40 and t[0, 3] == -1
    assert d.dtype == np.float64 and np.array_equal(d, np.arange(10))
