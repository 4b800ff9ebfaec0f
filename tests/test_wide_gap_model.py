"""CPU side of "wide_gap_tiles" (tests/test_gpu_wide_gap.py holds the GPU side): the numpy restatement of the plan rule
(tests/wide_gap_model.py plan_rule) against expectations written by hand, and the transfer-matrix chain against the sweep on the
200-state golden model."""
import os
import numpy as np
import pytest
from conftest import GOLD
from wide_gap_model import plan_rule, chain_vs_sweep, MISSING


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
