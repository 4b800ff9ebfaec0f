"""CPU side of tests/test_gpu_fast_chain.py: the long-double references, the float64 restatement of the fast path's transfer-matrix
chain and the list builder's rule (tests/fast_chain_model.py).  The restatement must pass the gates the device's matrices and vectors
are put through, with a wide margin, and three deliberate faults must each miss a gate by at least 100 x its bound -- otherwise the
gates could not tell a correct chain from a wrong one.  chain_rule is held to figures worked out by hand from the rule's text."""
import os
import subprocess
import numpy as np
import pytest
import fast_chain_model as fc
from fast_chain_model import LD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hostlib_built():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "host"), "libpsmc_host.so"], check=True)


def test_positions():
    """kc_ranges on hand-made tiles: every lo % 4, the last tile of a segment, ranges of zero steps"""
    down = lambda hi, lo: list(range(hi, lo - 1, -1))
    assert fc.kc_ranges(65, 128, 1000, False, 1) == ([list(range(65, 129))], [])
    assert fc.kc_ranges(65, 128, 1000, True, 1) == ([down(128, 69)], [68, 67, 66, 65])     # p* = 68
    assert fc.kc_ranges(66, 129, 1000, True, 1) == ([down(129, 69)], [68, 67, 66])
    assert fc.kc_ranges(67, 130, 1000, True, 1) == ([down(130, 69)], [68, 67])
    assert fc.kc_ranges(68, 131, 1000, True, 1) == ([down(131, 69)], [68])                 # lo itself is rescaled
    assert fc.kc_ranges(937, 1000, 1000, True, 1) == ([down(999, 941)], [940, 939, 938, 937])   # top = L - 1
    assert fc.kc_ranges(997, 1000, 1000, True, 1) == ([[]], [999, 998, 997])               # nothing above p* = 1000 > top
    r, tail = fc.kc_ranges(9, 16, 1000, True, 16)                                          # 16 .. 13 in 16 ranges, tail 12 .. 9
    assert [len(x) for x in r].count(0) == 12 and sum(r, []) == [16, 15, 14, 13] and tail == [12, 11, 10, 9]
    r, tail = fc.kc_ranges(9, 16, 1000, False, 3)
    assert r == [[9, 10], [11, 12, 13], [14, 15, 16]] and tail == []
    assert fc.kc_ranges(65, 128, 1000, True, 1, "split_shift") == ([down(128, 70)], [68, 67, 66, 65])


def test_references_agree(golden):
    """boundary_refs against range_matrix_ref: the forward vector at a tile's end is its start vector through the product of the tile's
    steps, the backward vector under a tile is the one above it through the tile's ranges and tail -- at tiles of 37 bins, every lo % 4"""
    a, e, a0 = fc.model(golden, "n23_curve")
    seg = fc.gaps_input(golden.segs_mid[3], 37, n_tiles=12, rest=5, runs=((5, 6),))[1]
    L, T = len(seg), 37
    entry, bentry = fc.boundary_refs(a, e, a0, seg, T)
    tl = fc.tiles_of(L, T)
    assert np.isnan(entry[0]).all() and not np.isnan(entry[1:]).any() and not np.isnan(bentry).any()
    assert np.array_equal(bentry[-1], fc.emissions(e, LD)[seg[-1]] / fc.emissions(e, LD)[seg[-1]].sum())
    for t in range(1, len(tl) - 1):
        M = fc.range_matrix_ref(a, e, seg, list(range(tl[t][0], tl[t][1] + 1)))
        assert fc.vector_error(entry[t] @ M, entry[t + 1]) < 1e-16
    for t in range(len(tl) - 1, 0, -1):
        r, tail = fc.kc_ranges(tl[t][0], tl[t][1], L, True, 2)
        M = fc.range_matrix_ref(a, e, seg, r[0] + r[1] + tail, backward=True)
        assert fc.vector_error(bentry[t] @ M, bentry[t - 1]) < 1e-16
    # the power shortcut of range_matrix_ref is the plain product
    pos = list(range(tl[5][0], tl[6][1] + 1))
    plain = np.eye(23, dtype=LD)
    for p in pos:
        plain = (plain @ np.asarray(a, dtype=LD)) * fc.emissions(e, LD)[seg[p - 1]]
    assert float(np.abs(fc.range_matrix_ref(a, e, seg, pos) - plain).max() / plain.max()) < 1e-17


def run_chain(golden, name, T, sub, backward, fault=None, n_tiles=14, runs=((5, 8),), first=3, count=9, second=False):
    """The restatement over one chain of a small "gaps" segment (data tiles with het bins, a run of gap tiles, data tiles again), started
    from the long-double boundary vector; the worst error / bound ratio of the gates (a), (b), (c)."""
    a, e, a0 = fc.model(golden, name, second)
    n = a.shape[0]
    seg = fc.gaps_input(golden.segs_mid[3], T, n_tiles=n_tiles, rest=5, runs=runs)[1]
    L = len(seg)
    tl = fc.tiles_of(L, T)
    entry, bentry = fc.boundary_refs(a, e, a0, seg, T)
    order = list(range(first, first + count - 1)) if not backward else list(range(first + count - 1, first, -1))
    head = first if not backward else first + count - 1
    x = np.asarray((bentry if backward else entry)[head], dtype=np.float64)
    worst = dict(a=0.0, b=0.0, c=0.0)
    spread = 0
    for t in order:
        lo, hi = tl[t]
        y, mats = fc.chain_tile(a, e, seg, lo, hi, backward, sub, x, fault)
        ranges, tail = fc.kc_ranges(lo, hi, L, backward, sub)          # (the correct ranges)
        for (K, E), r in zip(mats, ranges):
            ref = fc.range_matrix_ref(a, e, seg, r, backward)
            worst["a"] = max(worst["a"], fc.matrix_error(K, E, ref, n) / fc.matrix_bound(len(r), n))
            spread = max(spread, int(E.max() - E.min()))
        want = fc.chain_tile_ref(a, e, seg, lo, hi, backward, mats, x, n)
        worst["b"] = max(worst["b"], fc.vector_error(y, want) / fc.apply_bound(sub, n, backward))
        nxt = t - 1 if backward else t + 1
        d = (L - min(tl[nxt][1], L - 1) - 1) if backward else tl[nxt][0] - 1
        worst["c"] = max(worst["c"], fc.vector_error(y, (bentry if backward else entry)[nxt]) / fc.vector_bound(d, n))
        x = y
    return worst, spread


CASES = [("n64_curve", 64, 1), ("n64_flat", 64, 3), ("rho_1e-6", 64, 1), ("tmax_60", 64, 1), ("n23_curve", 37, 1), ("psmc3", 37, 2), ("psmc63", 8, 16),
         ("n64_curve", 256, 4), ("psmc100", 64, 1)]


@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("name, T, sub", CASES, ids=lambda v: str(v))
def test_restatement_inside_the_bounds(golden, hostlib_built, name, T, sub, backward):
    """(a) every matrix against the long-double product of its steps, (b) every tile of the chain against the long-double product of its
    own matrices, (c) every vector against the long-double sweep from the segment's end: all within a fifth of their bounds"""
    big = T == 256 or name == "psmc100"
    worst, _ = run_chain(golden, name, T, sub, backward, **(dict(n_tiles=9, runs=((4, 5),), first=2, count=6) if big else {}))
    print("CHAINMODEL %s T %d sub %d %s: error / bound (a) %.3f (b) %.3f (c) %.3f" % (name, T, sub, "backward" if backward else "forward", worst["a"], worst["b"], worst["c"]))
    assert max(worst.values()) <= 0.2, worst


@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("fault, gate", [("drop_row", "b"), ("no_exp", "b"), ("split_shift", "c")])
def test_faults_miss_the_gates(golden, fault, gate, backward):
    """A source row dropped from one product, the exponents ignored, the backward range split moved by one position: each at least
    100 x outside a gate's bound (the split concerns the backward direction only; forward it changes nothing and passes)."""
    worst, spread = run_chain(golden, "n64_curve", 64, 1, backward, fault)
    print("CHAINMODEL fault %s %s: error / bound (a) %.3g (b) %.3g (c) %.3g; exponents spread over %d" % (fault, "backward" if backward else "forward", worst["a"], worst["b"], worst["c"], spread))
    if fault == "split_shift" and not backward:
        assert max(worst.values()) <= 0.2, worst
        return
    if fault == "no_exp":
        assert spread >= 2          # (a condition on the input: the columns' exponents differ)
    assert worst[gate] >= 100, worst
    if fault == "split_shift":      # the matrices themselves are then products of other positions than the reference's
        assert worst["a"] >= 100, worst


# ------------------------------------------------------------------ chain_rule
def rule_of(segs, T, W, n, **kw):
    cls, glue = fc.gap_plan(segs, T)
    return fc.chain_rule(segs, T, W, glue, cls, n, **kw)


def test_chain_rule_gaps(golden):
    """ "gaps" at tiles of 64 bins, warm-ups of 4096: the runs (4, 10), (29, 6), (39, 4) of the long segment in both directions, forward
    the one that ends last first, backward the one that starts first; at 128 states only (4, 10) unless kc_min = 2; one shared slot per
    direction; at tiles of 37 bins a matrix per tile"""
    src = golden.segs_mid[3]
    segs, F = fc.gaps_input(src, 64), fc.front_tiles(64)
    r = rule_of(segs, 64, 4096, 64)
    assert r["runs"] == ([(F + 39, 4), (F + 29, 6), (F + 4, 10)], [(F + 4, 10), (F + 29, 6), (F + 39, 4)])
    assert r["sub"] == 1 and len(r["kc"]) == 2 * (3 + 5 + 9)
    assert r["kc"][:3] == [(F + 39, 0), (F + 40, 0), (F + 41, 0)] and r["kslot"][:3] == [0, 1, 1]
    assert r["kc"][17:26] == [(F + t, 1) for t in range(13, 4, -1)] and r["kslot"][17:26] == [4] + [5] * 8
    assert len(r["kuniq"]) == 8 and r["kuniq"] == [0, 1, 3, 8, 17, 18, 26, 31]
    assert rule_of(segs, 64, 4096, 128)["runs"] == ([(F + 4, 10)], [(F + 4, 10)])
    assert rule_of(segs, 64, 4096, 100, kc_min=2)["runs"] == r["runs"]
    assert rule_of(segs, 64, 4096, 64, kc_min=0)["runs"] == ([], [])
    assert rule_of(segs, 64, 4096, 64, kc_sub=3)["sub"] == 3 and rule_of(segs, 64, 4096, 128, kc_sub=3)["sub"] == 1
    assert rule_of(segs, 64, 256, 64)["sub"] == 2 and rule_of(segs, 256, 3072, 64)["sub"] == 1 and rule_of(segs, 3712, 3072, 64)["sub"] == 4
    s37, F37 = fc.gaps_input(src, 37), fc.front_tiles(37)
    r = rule_of(s37, 37, 4096, 64)
    assert sorted(r["runs"][0]) == sorted(r["runs"][1]) == [(F37 + 4, 10), (F37 + 29, 6), (F37 + 39, 4)]
    assert r["kslot"] == list(range(34)) and r["kuniq"] == list(range(34))


def test_chain_rule_first_tile_and_cap(golden):
    """A forward run on the segment's first tile is chained from its second tile; group_cap cuts runs by their data bins (gap tiles are
    free); a budget of 64 admits what fits, longest first"""
    src = golden.segs_mid[3]
    segs, F = fc.head_input(src, 64), fc.front_tiles(64)
    r = rule_of(segs, 64, 4096, 64)
    assert r["runs"] == ([(F + 1, 7)], [(F + 0, 8)])
    assert r["kc"][:6] == [(F + t, 0) for t in range(1, 7)] and r["kslot"][:6] == [0] * 6
    assert rule_of(fc.gaps_input(src, 64, runs=((1, 1),)), 64, 4096, 64, kc_min=2)["runs"] == ([(F + 1, 2)], [(F + 0, 3)])
    assert rule_of(fc.gaps_input(src, 64, runs=((1, 2),)), 64, 4096, 64, kc_min=2)["runs"] == ([(F + 1, 3)], [(F + 0, 4)])
    # everything glued: 150 tiles of 8 bins and a ragged one, runs of 20 tiles under group_cap = 160, each costs 19 of the budget of 64
    T, nt = 8, 151
    segs = [np.zeros(150 * 8 + 5, np.uint8)]
    segs[0][::3] = 1
    glue = np.array([2] + [3] * (nt - 2) + [1]); cls = np.zeros(nt, np.int32)
    r = fc.chain_rule(segs, T, 4096, glue, cls, 64, group_cap=160)
    # forward the runs that end last come first: (140, 11) costs 10, (120, 20), (100, 20) 19 each, (80, 20) no longer fits, nor any other
    assert r["runs"][0] == [(140, 11), (120, 20), (100, 20)]
    # backward the runs that start first: (0, 20) -> 19, (20, 20), (40, 20); then 7 are left: nothing fits but ... (140, 11) costs 10: no
    assert r["runs"][1] == [(0, 20), (20, 20), (40, 20)]
    assert len(r["kc"]) == 10 + 19 + 19 + 3 * 19 and r["kslot"] == list(range(len(r["kc"])))


def test_chain_rule_hom(golden):
    """ "hom" under hom_tiles = 1, hom_min = 2 T, group_cap = 1024 (classes and glue bits by the plan rule of tests/test_gpu_hom_tiles.py): several
    runs per direction, all chained; tile 22 (a het-free mix) keeps a slot of its own, the all-homozygous tiles around it share one"""
    from test_gpu_hom_tiles import rule
    T, W = 64, 4096
    segs, F = fc.hom_input(golden.segs_mid[3], T), fc.front_tiles(T)
    cls, glue = rule(segs, T, W, 2 * T)
    assert list(cls[F + 20:F + 25]) == [3, 3, 3, 3, 3]
    r = fc.chain_rule(segs, T, W, glue, cls, 64, group_cap=1024)
    for d in (0, 1):
        assert len(r["runs"][d]) >= 2
    slot = {kt: r["kslot"][j] for j, kt in enumerate(r["kc"])}
    for d in (0, 1):
        assert slot[(F + 20 + d, d)] == slot[(F + 23, d)] == slot[(F + 21, d)] != slot[(F + 22, d)]
        assert sum(1 for j, kt in enumerate(r["kc"]) if r["kslot"][j] == slot[(F + 22, d)]) == 1
