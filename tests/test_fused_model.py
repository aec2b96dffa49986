"""CPU checks of the fused statistics window's model (tests/fused_model.py):
the model's rows against the oracle on every case set the GPU tests run
(tests/test_gpu_fused_window.py), the preconditions of those cases, and the
mutants the case sets must tell from the real rules."""
import numpy as np
import pytest

from oracle import coracle
from tests import fused_model as fm

SETS = sorted(fm.CASE_SETS)
W = fm.K_HIST_BINS


def oracle_rows(b):
    d, ext, coff = coracle.depth(b.lengths, b.tid, b.pos, b.span)
    return d, ext, coff, coracle.region_stats(d, ext, coff, b.rtid, b.rs, b.re)


_ORACLE = {}


def oracle_of(name, variant):
    if (name, variant) not in _ORACLE:
        _ORACLE[(name, variant)] = oracle_rows(fm.built(name, variant))
    return _ORACLE[(name, variant)]


def row_equal(row, want):
    return all(int(row[f]) == int(want[f]) for f in fm.ROW_FIELDS)


def test_constants_match_source():
    for k, v in fm.source_constants().items():
        assert getattr(fm, k) == v, k


def test_reads_for_profile():
    """Big jumps, a long plateau (reads restarted at max_span), zeros inside."""
    rng = np.random.default_rng(5)
    d = np.concatenate([rng.integers(0, 3000, size=200), np.full(700, 2500), np.zeros(3, np.int64),
                        rng.integers(0, 50, size=97), [7]])
    for max_span in (1, 64, 4096):
        pos, span = fm.reads_for_profile(d, max_span)
        assert (np.diff(pos) >= 0).all() and span.min() >= 1 and span.max() <= max_span
        assert (pos.astype(np.int64) + span).max() <= len(d)
        got, ext, coff = coracle.depth([len(d)], np.zeros(len(pos), np.int32), pos, span)
        assert ext[0] == len(d) and np.array_equal(got, d)
    assert fm.reads_for_profile(d, 64)[1].max() == 64


def test_rounding():
    assert [fm.llround(x) for x in (0.0, 0.49, 0.5, 1.5, 2.5, 2648.5)] == [0, 0, 1, 2, 3, 2649]
    assert [fm.llrint(x) for x in (0.0, 0.49, 0.5, 1.5, 2.5, 2648.5)] == [0, 0, 0, 2, 2, 2648]


def test_redundant_flag_terms():
    """For n >= 1, q_lo <= r_lo and q_hi - 1 >= r_hi: whenever a median term of
    K3b's flag holds, the quartile term of the same side holds too.  (The
    kernel keeps all four.)"""
    for n in range(1, 65):
        r_lo, r_hi, q_lo, q_hi = (n - 1) // 2, n // 2, n // 4, n - n // 4
        assert q_lo <= r_lo and q_hi - 1 >= r_hi
        for win_lo in range(n + 1):
            for win_hi in range(win_lo, n + 1):
                two = q_lo < win_lo or q_hi - 1 >= win_hi
                four = r_lo < win_lo or r_hi >= win_hi or two
                assert two == four


@pytest.mark.parametrize("variant", fm.VARIANTS)
@pytest.mark.parametrize("name", SETS)
def test_model_rows_vs_oracle(name, variant):
    """The batch gives exactly the prescribed depth; every unflagged region's
    model row is the oracle's; every flagged region's row is not (in med_lo,
    med_hi or q23_sum), so its flag is needed."""
    b = fm.built(name, variant)
    d, ext, coff, want = oracle_of(name, variant)
    assert np.array_equal(ext, b.extent)
    for t in range(len(b.lengths)):
        assert np.array_equal(d[coff[t]:coff[t] + ext[t]], b.profiles[t]), t
    assert int(b.span.max()) <= fm.K_SHORT_MAX or b.long_read
    base, info = fm.model_rows(b)
    assert np.array_equal(base, b.base)
    n_flag = 0
    for r, c in enumerate(info):
        tag = (r, b.items[r].tag if b.items[r] else None)
        if c["flag"]:
            n_flag += 1
            # (the one flag that is only cautious: the ranks that leave the window
            # are all zeros past the extent, which the unrecomputed row has as 0)
            zeros_only = not c["terms"][1] and not c["terms"][3] and c["low"] == c["zx"]
            differs = any(int(c["row"][f]) != int(want[r][f]) for f in ("med_lo", "med_hi", "q23_sum"))
            assert differs != zeros_only, tag
        else:
            assert row_equal(c["row"], want[r]), (tag, c["row"], want[r])
    assert 0 < n_flag < len(info)


@pytest.mark.parametrize("variant", fm.VARIANTS)
@pytest.mark.parametrize("name", SETS)
def test_fixed_point_and_edge_values(name, variant):
    """The cells' values were placed from the bases the model computes from
    the final reads; base - 1, base, base + 863 and base + 864 all occur in
    regions of a contig whose base is above 0; base 0 occurs too."""
    b = fm.built(name, variant)
    base = fm._bases(b.base_variant, b.extent, b.tid, b.span)
    assert np.array_equal(base, b.base)
    for t, c in enumerate(b.contigs):
        prof, pos, span = c.assemble(int(base[t]), b.floor[t], b.counts[t])
        assert np.array_equal(prof, b.profiles[t])
        assert np.array_equal(pos, b.pos[b.tid == t]) and np.array_equal(span, b.span[b.tid == t])
    if name in ("rank_edges", "value_edges", "compose", "slot"):
        assert (base[:len(b.contigs)] == 0).any()
    t = 0
    assert base[t] > 0
    seen = set()
    for r in np.nonzero(b.rtid == t)[0]:
        seen.update((b.profiles[t][b.rs[r]:min(b.re[r], b.lengths[t])] - base[t]).tolist())
    need = {W - 1, W} if name == "slot" else {-1, 0, W - 1, W}
    assert need <= seen, (need - seen)


@pytest.mark.parametrize("variant", fm.VARIANTS)
def test_rank_edge_preconditions(variant):
    """Each rank cell has q_lo - win_lo and (q_hi - 1) - win_hi where its
    builder meant them; every distance occurs, from values below the window,
    from zeros past the extent alone (base > 0) and, on the high side, on a
    contig of base 0; the flag follows from the two distances."""
    b = fm.built("rank_edges", variant)
    base, info = fm.model_rows(b)
    seen = {"real": set(), "zx": set(), "base0": set()}
    ns = set()
    for r, (i, c) in enumerate(zip(b.items, info)):
        w = i.want
        dl, dh = c["q_lo"] - c["win_lo"], c["q_hi"] - 1 - c["win_hi"]
        kind = "base0" if base[b.rtid[r]] == 0 else "zx" if i.zx else "real"
        if kind == "base0":
            assert c["low"] == 0 and w["dl"] is None
        else:
            assert dl == w["dl"], i.tag
            assert base[b.rtid[r]] > 0
        if kind == "zx":
            assert c["low"] == i.zx and c["n"] == i.n + i.zx     # nothing real below the window
        if w["dh"] is not None:
            assert dh == w["dh"], i.tag
        assert c["flag"] == (dl < 0 or dh >= 0), i.tag
        seen[kind].add((dl if kind != "base0" else None, dh if w["dh"] is not None else None))
        ns.add(c["n"])
    assert {(dl, dh) for dl in (-1, 0, 1) for dh in (-2, -1, 0)} <= seen["real"]
    assert {dl for dl, _ in seen["zx"]} == {-1, 0, 1} and (0, 0) in seen["zx"]
    assert {dh for _, dh in seen["base0"]} == {-2, -1, 0}
    assert {1, 2, 3, 4, 5, 12, 13, 14, 15} <= ns


@pytest.mark.parametrize("variant", fm.VARIANTS)
def test_value_edge_preconditions(variant):
    """Runs of 1 .. 4 across each edge at each alignment, flagged and not;
    cell lengths no multiple of 4; cells with nothing inside the window."""
    b = fm.built("value_edges", variant)
    base, info = fm.model_rows(b)
    off = fm.contig_offsets(b.extent)
    seen = set()
    for r, (i, c) in enumerate(zip(b.items, info)):
        if i.tag.split()[0] in ("high", "low") and base[b.rtid[r]] > 0:
            pair, rr, aa, kind = i.tag.split()
            assert (off[b.rtid[r]] + b.rs[r]) % 4 == int(aa[2:]) and c["n"] % 4 != 0
            v = b.profiles[0][b.rs[r]:b.re[r]] - base[0]
            edge = (W - 1, W) if pair == "high" else (-1, 0)
            k = np.nonzero(np.isin(v, edge))[0]
            runs = np.diff(np.nonzero(np.diff(v[k[0]:k[-1] + 1]) != 0)[0])
            assert len(runs) and (runs == int(rr[2:])).all(), i.tag
            assert kind == "dense" or not c["flag"], i.tag
            seen.add((pair, int(rr[2:]), int(aa[2:]), c["flag"]))
    for pair in ("high", "low"):
        for rr in (1, 2, 3, 4):
            for aa in (0, 1, 2, 3):
                assert (pair, rr, aa, False) in seen
            assert any((pair, rr, aa, True) in seen for aa in (0, 1, 2, 3))
    by_tag = {i.tag: c for i, c in zip(b.items, info)}
    assert by_tag["all above"]["high"] == 7 and by_tag["all above"]["in_hist"] == 0
    assert by_tag["all below"]["low"] == 7 and by_tag["all below"]["in_hist"] == 0
    c = by_tag["below and above, none inside"]
    assert c["low"] == 3 and c["high"] == 3 and c["in_hist"] == 0


@pytest.mark.parametrize("variant", fm.VARIANTS)
def test_compose_preconditions(variant):
    b = fm.built("compose", variant)
    base, info = fm.model_rows(b)
    c = {i.tag: x for i, x in zip(b.items, info) if i}
    z = c["zx only below, unflagged"]
    assert z["low"] == 3 and z["high"] == 0 and not z["flag"] and z["row"]["min"] == 0
    z = c["zx below, high above"]
    assert z["low"] == 3 and z["high"] == 2 and not z["flag"] and z["row"]["min"] == 0
    z = c["zx and real below"]
    assert z["low"] == 3 and not z["flag"] and z["row"]["min"] == 0
    z = c["low real, unflagged"]
    assert z["low"] == 2 and z["high"] == 0 and not z["flag"] and z["row"]["min"] == base[0] - 7
    z = c["high only, unflagged"]
    assert z["low"] == 0 and z["high"] == 2 and not z["flag"] and z["row"]["max"] == base[0] + W + 29
    z = c["low and high, unflagged"]
    assert z["low"] == 2 and z["high"] == 2 and not z["flag"]
    assert c["low real, flagged"]["flag"] and c["high, flagged"]["flag"] and c["zx below, flagged"]["flag"]
    z = c["base0 zx in bin 0"]
    assert z["low"] == 0 and z["in_hist"] == 11 and not z["flag"] and z["row"]["min"] == 0
    z = c["base0 zx and high"]
    assert z["low"] == 0 and z["high"] == 2 and not z["flag"]
    # the extra regions: past the extent (base > 0: all below the window, flagged; base 0: bin 0) and empty
    ex = [x for i, x in zip(b.items, info) if i is None]
    assert [x["n"] for x in ex] == [5, 1, 7, 0, 0, 0]
    assert ex[0]["flag"] and ex[0]["low"] == 5 and ex[1]["flag"] and not ex[2]["flag"] and ex[2]["in_hist"] == 7
    assert not any(x["flag"] for x in ex[3:])
    # the tiny contig: both branches of the body rule occur, and its estimate is an exact half on the full prepare
    if b.base_variant == "full":
        mean = float(b.span.astype(np.int64).sum()) / len(b.span)
        t = len(b.contigs) - 2
        assert b.contigs[t].plain and b.lengths[t] <= 2 * mean < b.lengths[0]
        est = float(b.span[b.tid == t].astype(np.int64).sum()) / float(b.lengths[t])
        assert est == base[t] + fm.K_WIN_BELOW + 0.5 and base[t] % 2 == 0
        assert not c["tie base"]["flag"] and c["tie base"]["in_hist"] == 1
        # the contig whose reads run past its length: the extent gives the base, and the length would not
        t += 1
        assert b.extent[t] == b.lengths[t] + 4 and (np.delete(b.extent, t) == np.delete(b.lengths, t)).all()
        assert fm.window_base_full(b.lengths, b.tid, b.span)[t] != base[t]
        assert not c["overhang base"]["flag"] and not c["overhang base+863"]["flag"] and not c["overhang zx"]["flag"]
        assert c["overhang zx"]["zx"] == 3


@pytest.mark.parametrize("variant", fm.VARIANTS)
def test_tiny_chunk_slot_preconditions(variant):
    b = fm.built("tiny", variant)
    off = fm.contig_offsets(b.extent)
    n1 = np.nonzero(b.re - b.rs == 1)[0][:fm.K_TILE_W]
    assert np.array_equal(off[0] + b.rs[n1], fm.K_TILE_W + np.arange(fm.K_TILE_W))   # one tile, exactly
    base, info = fm.model_rows(b)
    small = [r for r, i in enumerate(b.items) if i.tag]
    shared = sum(1 for r in small if b.rs[r] // 4 == (b.re[r] - 1) // 4 and b.re[r] - b.rs[r] < 4)
    assert shared > 20 and any(info[r]["flag"] for r in small) and not all(info[r]["flag"] for r in small)
    assert sum(c["flag"] for c in info) <= fm.K_FB_SLOTS

    b = fm.built("chunk", variant)
    off = fm.contig_offsets(b.extent)
    w = fm.chunk_width(b.extent)
    assert w == 2 * fm.K_TILE_W == fm.chunk_width(b.extent, long_hint=True)
    base, info = fm.model_rows(b)
    for r, edge, flag in ((0, fm.K_TILE_W, False), (1, w, False), (2, 2 * w, True)):
        t = b.rtid[r]
        gs, ge = off[t] + b.rs[r], off[t] + b.re[r]
        assert gs < edge < ge and info[r]["flag"] == flag
        v = b.profiles[t][b.rs[r]:b.re[r]] - base[t]
        for side in (v[:edge - gs], v[edge - gs:]):
            assert (side < 0).any() and (side >= W).any()

    b = fm.built("slot", variant)
    base, info = fm.model_rows(b)
    flags = np.array([c["flag"] for c in info])
    assert flags.sum() == fm.K_FB_SLOTS + 1 and flags[:fm.K_FB_SLOTS + 1].all()
    assert (b.re - b.rs == 8).all() and len(flags) > fm.K_FB_SLOTS + 8


MUTANTS = {
    "q_lo_le": dict(q_lo_le=True),
    "q_hi_gt": dict(q_hi_gt=True),
    "kwin_plus": dict(kwin=W + 1),
    "kwin_minus": dict(kwin=W - 1),
    "win_below_plus": dict(win_below=fm.K_WIN_BELOW + 1),
    "win_below_minus": dict(win_below=fm.K_WIN_BELOW - 1),
    "rounding_llround": dict(rounding="llround"),
    "no_min_rule": dict(min_rule=False),
    "max_high_ge": dict(max_high_ge=True),
    "zx_bin_always": dict(zx_bin_always=True),
}


def mutant_kills(name, variant, params):
    """Regions on which the mutated model predicts another flag than the real
    one, or leaves a region unflagged with a row that is not the oracle's."""
    b = fm.built(name, variant)
    want = oracle_of(name, variant)[3]
    _, real = fm.model_rows(b)
    _, mut = fm.model_rows(b, params)
    kills = []
    for r, (c, m) in enumerate(zip(real, mut)):
        if c["flag"] != m["flag"] or (not m["flag"] and not row_equal(m["row"], want[r])):
            kills.append(r)
    return kills


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_killed(mutant):
    """Every mutant is told from the real rules by a case set the GPU tests
    run, in the prepared variant; all but the rounding mutant (which needs an
    exact half) in the direct variant too."""
    params = fm.Params(**MUTANTS[mutant])
    sets = [n for n in SETS if n != "slot"]
    killed = {v: [n for n in sets if mutant_kills(n, v, params)] for v in ("full", "direct")}
    assert killed["full"], mutant
    if mutant != "rounding_llround":
        assert killed["direct"], mutant
    else:
        assert killed["full"] == ["compose"]


def test_real_model_kills_nothing():
    for name in SETS:
        assert mutant_kills(name, "full", fm.Params()) == []


def test_recompute_path():
    assert fm.recompute_path(3, False) == (3, 0)
    assert fm.recompute_path(3, True) == (0, 3)
    assert fm.recompute_path(fm.K_FB_SLOTS, True) == (0, fm.K_FB_SLOTS)
    assert fm.recompute_path(fm.K_FB_SLOTS + 1, True) == (fm.K_FB_SLOTS + 1, 0)
    assert fm.recompute_path(3, True, max_depth=fm.K_LDS_BINS) == (3, 0)
    assert fm.recompute_path(0, True) == (0, 0)
