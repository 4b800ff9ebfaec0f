"""CPU side of "wide_gap_tiles" (tests/test_gpu_wide_gap.py holds the GPU side): the numpy restatement of the plan rule
(tests/wide_gap_model.py plan_rule) against expectations written by hand, the chains (chain_rule) against the figures a port of the
planner gave, the transfer-matrix chain against the sweep on the 200-state golden model, and the long-double matrix references and
the per-application gate that tests/test_gpu_wide_gap_chain.py uses."""
import os
import numpy as np
import pytest
from conftest import GOLD
from wide_gap_model import (plan_rule, chain_rule, chain_errors, chain_vs_sweep, matrix_ref, matrix_rows_ref, twin, triple, head_run, tail_run,
                            tiles_missing, MISSING)


def seg(L, *gaps):
    s = np.zeros(L, dtype=np.uint8)
    s[::7] = 1
    for lo, hi in gaps:   # positions lo .. hi (1-based, inclusive) are missing
        s[lo - 1:hi] = MISSING
    return s


def expect(n, cls=(), fwd=(), bwd=()):
    c, g = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for v, tiles in cls:
        c[list(tiles)] = v
    g[list(fwd)] |= 1
    g[list(bwd)] |= 2
    return c, g


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_rule_run_shorter_than_the_minimum():
    """T = 10, W = 20, minimum 40 bins: three gap tiles (30 bins) are class 1 and glue nothing; with a minimum of 30 they qualify."""
    s = seg(200, (101, 130))   # tiles 10, 11, 12 of 20
    assert same(plan_rule([s], 10, 20, 40), expect(20, cls=[(1, (10, 11, 12))]))
    # qualifying: the run's tiles both ways; forward the tiles whose window lo - 20 .. lo - 1 reaches a run tile: 13 (111..130) and 14
    # (121..140; tile 12 is 121..130); backward the mirror: 9 (window 101..120) and 8 (91..110; tile 10 is 101..110)
    assert same(plan_rule([s], 10, 20, 30), expect(20, cls=[(2, (10, 11, 12))], fwd=(10, 11, 12, 13, 14), bwd=(8, 9, 10, 11, 12)))
    # auto: a quarter of the warm-up = 5 bins
    assert same(plan_rule([s], 10, 20), plan_rule([s], 10, 20, 30))
    # a gap that is not tile-aligned leaves only its full tiles: 103 .. 132 holds tiles 11 and 12
    assert same(plan_rule([seg(200, (103, 132))], 10, 20, 20), expect(20, cls=[(2, (11, 12))], fwd=(11, 12, 13, 14), bwd=(9, 10, 11, 12)))


def test_rule_run_touching_an_anchored_tile():
    """T = 10, W = 20: tiles 0, 1, 2 are anchored forward (lo - 20 <= 1), tiles 17, 18, 19 backward (hi + 21 >= 200).  A run over
    tiles 1 .. 4 is class 2 throughout, but the anchored ones are not glued forward."""
    s = seg(200, (11, 50))
    assert same(plan_rule([s], 10, 20, 10), expect(20, cls=[(2, (1, 2, 3, 4))], fwd=(3, 4, 5, 6), bwd=(0, 1, 2, 3, 4)))
    # the mirror at the other end: tiles 15 .. 18
    s = seg(200, (151, 190))
    assert same(plan_rule([s], 10, 20, 10), expect(20, cls=[(2, (15, 16, 17, 18))], fwd=(15, 16, 17, 18, 19), bwd=(13, 14, 15, 16)))


def test_rule_run_ending_in_the_last_tile():
    """Missing data to the segment's end: the last tile is never a gap tile (position L is special), nor is a ragged one; the first
    tile is not one either."""
    s = seg(195, (151, 195))   # tiles 15 .. 18 full, tile 19 holds 191 .. 195
    c, g = plan_rule([s], 10, 20, 10)
    assert same((c, g), expect(20, cls=[(2, (15, 16, 17, 18))], fwd=(15, 16, 17, 18, 19), bwd=(13, 14, 15, 16)))
    s = seg(200, (1, 40))
    assert same(plan_rule([s], 10, 20, 10), expect(20, cls=[(2, (1, 2, 3))], fwd=(3, 4, 5), bwd=(0, 1, 2, 3)))
    # a segment of missing data only, and one too short to have an inner tile
    c, g = plan_rule([seg(100, (1, 100)), seg(20, (1, 20))], 10, 0, 10)
    assert list(c) == [0] + [2] * 8 + [0] + [0, 0] and not g[10:].any()


def test_rule_two_runs_500_bins_apart():
    """The shape of stress segment 2: two runs 500 bins apart, T = 100, W = 1000 -- the tiles between the runs hang on both."""
    s = seg(6000, (2001, 3000), (3501, 4500))   # tiles 20 .. 29 and 35 .. 44 of 60
    c, g = plan_rule([s], 100, 1000)
    want = expect(60, cls=[(2, list(range(20, 30)) + list(range(35, 45)))], fwd=range(20, 55), bwd=range(10, 45))
    assert same((c, g), want)
    # two segments: nothing crosses from one into the next
    c2, g2 = plan_rule([s, seg(6000)], 100, 1000)
    assert same((c2[:60], g2[:60]), want) and not c2[60:].any() and not g2[60:].any()


@pytest.mark.parametrize("T", [576, 7360])
def test_chain_matches_the_sweep(T):
    """n200.a, 40 tiles (T = 576; 2 at T = 7360, the benchmark genome's tile), forward and backward: one application of M against T
    single steps from the same vector, in tile_mismatch's metric, is within 5e-13 -- half the default warm_tol.  Measured here:
    8.2e-15 forward and 3.9e-14 backward at T = 576; 1.8e-14 and 7.7e-14 at T = 7360."""
    w = dict(np.load(os.path.join(GOLD, "estep_wide.npz")))
    a, e, a0 = w["n200.a"], w["n200.e"], w["n200.a0"]
    tiles = 40 if T == 576 else 2
    x0 = a0 * e[0] * (1.0 + 0.5 * np.sin(np.arange(len(a0))))   # not the stationary vector
    f = chain_vs_sweep(a, x0, T, tiles)
    b = chain_vs_sweep(a, e[1] * (1.0 + 0.5 * np.cos(np.arange(len(a0)))), T, tiles, backward=True)
    print("chain against sweep, T = %d: forward %.2e backward %.2e" % (T, f, b))
    assert f <= 5e-13 and b <= 5e-13, (f, b)


# ------------------------------------------------------------------ the chains (chain_rule) and the long-double matrix
def test_chain_rule_twin(golden):
    """Two runs of 1024 missing bins 128 bins apart, warm-up 512, auto minimum: in all three tilings two chains per direction, the second
    one level later, and no unanchored tile left to speculate -- the figures a port of the planner gave."""
    s = twin(golden.segs_mid[3])
    assert len(s) == 2776
    want = {64: ([(9, 11, 20, 0), (23, 15, 38, 1)], [(34, 12, 22, 0), (19, 15, 4, 1)]),
            37: ([(14, 21, 35, 0), (40, 26, 66, 1)], [(60, 21, 39, 0), (34, 26, 8, 1)]),
            8: ([(65, 100, 165, 0), (182, 127, 309, 1)], [(281, 100, 181, 0), (164, 127, 37, 1)])}
    for T, w in want.items():
        assert chain_rule([s], T, 512) == w, T
        nt = (len(s) + T - 1) // T
        cls, glue = plan_rule([s], T, 512)
        for b in range(nt):   # every tile is anchored or glued, in both directions
            lo, hi = 1 + T * b, min(len(s), T * (b + 1))
            assert lo - 512 <= 1 or glue[b] & 1, (T, b)
            assert hi + 513 >= len(s) or glue[b] & 2, (T, b)


@pytest.mark.parametrize("tiles, runs, fwd, bwd", [
    (60, (3, 8), [(5, 4, 9, 0)], [(8, 6, 2, 0)]),        # the forward chain starts inside the run: tiles 3 and 4 are anchored
    (60, (2, 4), [(5, 0, 5, 0)], [(4, 3, 1, 0)]),        # anchored throughout forward: count 0, the walk alone
    (60, (55, 57), [(55, 3, 58, 0)], [(54, 0, 54, 0)]),  # its mirror
    (40, (0, 39), [(5, 34, 39, 0)], [(34, 34, 0, 0)]),   # a segment of missing data only: the walks stand on its first and last tile
])
def test_chain_rule_branches(tiles, runs, fwd, bwd):
    """Tiles of 64 bins, warm-up 256 (tiles 0 .. 4 anchored forward, the last five backward), minimum 128 bins."""
    assert chain_rule([tiles_missing(None, tiles, 64, runs)], 64, 256, 128) == (fwd, bwd)


def test_chain_rule_levels_and_segments(golden):
    """triple: three runs two tiles apart, levels 0, 1, 2 both ways.  head_run / tail_run: the count-0 branch and a chain that starts
    inside its run, at a warm-up of 512.  Two segments: tile numbers run on, a run anchored through to its segment's end adds nothing,
    and the launch order is by level first."""
    src = golden.segs_mid[3]
    t = triple(src)
    assert chain_rule([t], 64, 256, 128) == ([(20, 4, 24, 0), (26, 4, 30, 1), (32, 4, 36, 2)], [(35, 4, 31, 0), (29, 4, 25, 1), (23, 4, 19, 2)])
    # without a warm-up nothing but the runs is glued: every chain is level 0
    assert [c[3] for d in chain_rule([t], 64, 0, 128) for c in d] == [0] * 6
    assert chain_rule([head_run(src)], 64, 512, 128) == ([(9, 0, 9, 0)], [(5, 1, 4, 0)])
    assert chain_rule([tail_run(src)], 64, 512, 128) == ([(9, 1, 10, 0)], [(5, 0, 5, 0)])
    # five tiles with the run on tiles 1 .. 3, warm-up 256: every tile is anchored both ways, so behind the run everything to the
    # segment's end is exact in either direction -- no chain
    short = tiles_missing(src, 5, 64, (1, 3))
    assert (plan_rule([short], 64, 256, 128)[0] == 2).sum() == 3
    assert chain_rule([short], 64, 256, 128) == ([], [])
    f2, b2 = chain_rule([short, t], 64, 256, 128)
    assert f2 == [(25, 4, 29, 0), (31, 4, 35, 1), (37, 4, 41, 2)]
    assert b2 == [(40, 4, 36, 0), (34, 4, 30, 1), (28, 4, 24, 2)]
    f3, b3 = chain_rule([t, t], 64, 256, 128)   # by level, then in sweep order over the whole plan
    assert [c[0] for c in f3] == [20, 90, 26, 96, 32, 102] and [c[0] for c in b3] == [105, 35, 99, 29, 93, 23]


def test_matrix_ref():
    """The binary power, the stepped rows and 64 plain float64 products agree at 200 states and T = 64: rows sum to 1, the float64
    restatement is within 4 T n 2^-53 per row by a wide margin (the bound of tests/test_gpu_wide_gap_chain.py is no measurement)."""
    w = dict(np.load(os.path.join(GOLD, "estep_wide.npz")))
    a = w["n200.a"]
    M = matrix_ref(a, 64)
    assert M.dtype == np.longdouble and float(np.abs(M.sum(1) - 1).max()) < 64 * 200 * 2.0 ** -53   # (the rows of the golden a sum to 1 within an ulp or two)
    rows = [0, 1, 100, 198, 199]
    R = matrix_rows_ref(a, 64, rows)
    assert float(np.abs(R - M[rows]).max()) < 1e-16
    assert float(np.abs(matrix_ref(a, 7) - matrix_rows_ref(a, 7, range(200))).max()) < 1e-16
    P = np.eye(200)
    for _ in range(64):
        P = P @ a
    err = float((np.abs(P - M).max(1) / M.max(1)).max())
    print("float64 power against long double, n = 200, T = 64: %.2e (bound %.2e)" % (err, 4 * 64 * 200 * 2.0 ** -53))
    assert err <= 4 * 64 * 200 * 2.0 ** -53 / 50


def test_chain_gate_notices_a_dropped_row():
    """chain_errors, the per-application gate of tests/test_gpu_wide_gap_chain.py, on a float64 restatement of k_wf_gapchain at the
    149-state golden model (padded to 192: five ranges of rows forward): the faithful one is within 2 n 2^-53 both ways; one whose
    ranges are floor(n / 5) rows long -- states 145 .. 148 never contribute -- or whose backward sweep leaves the last row out is far
    outside it."""
    w = dict(np.load(os.path.join(GOLD, "estep_wide.npz")))
    a, e, a0 = w["n149.a"], w["n149.e"], w["n149.a0"]
    n, S, KS, T, tiles = 149, 192, 5, 64, 6
    M = np.zeros((n, S)); P = np.eye(n)
    for _ in range(T):
        P = P @ a
    M[:, :n] = P
    x0 = np.zeros(S); x0[:n] = a0 * e[0] * (1.0 + 0.5 * np.sin(np.arange(n)))

    def chain(backward, kc=None, rows=n):
        v, out = x0.copy(), [x0.copy()]
        for _ in range(tiles):
            y = np.zeros(S)
            if backward:
                y[:rows] = M[:rows] @ v
            else:
                for g in range(KS):   # partial sums of the row ranges, lowest first
                    y += v[g * kc:min(n, (g + 1) * kc)] @ M[g * kc:min(n, (g + 1) * kc)]
            v = y / y.sum()
            out.append(v)
        return np.array(out)

    bound = 2 * n * 2.0 ** -53
    fwd = [(0, tiles, tiles, 0)]
    bwd = [(tiles, tiles, 0, 0)]
    good_f, seen = chain_errors(n, M, chain(False, kc=(n + KS - 1) // KS), fwd, False)
    good_b, _ = chain_errors(n, M, chain(True)[::-1], bwd, True)
    bad_f, _ = chain_errors(n, M, chain(False, kc=n // KS), fwd, False)
    bad_b, _ = chain_errors(n, M, chain(True, rows=n - 1)[::-1], bwd, True)
    print("chain gate: faithful %.1e / %.1e, a dropped row %.1e / %.1e, bound %.1e" % (good_f, good_b, bad_f, bad_b, bound))
    assert seen == tiles and good_f <= bound and good_b <= bound
    assert bad_f > 100 * bound and bad_b > 100 * bound
