"""CPU side of "wide_hom_tiles" (tests/test_gpu_wide_hom.py and tests/test_gpu_wide_hom_chain.py hold the GPU side): the generalised
plan rule of tests/wide_hom_model.py against a toy worked out by hand and against plan_rule of tests/wide_gap_model.py whenever hom
is off, and the pilot-scaled matrix of a homozygous tile against the bin-by-bin sweep on the 149-state golden model."""
import os
import numpy as np
import pytest
from conftest import GOLD
import wide_gap_model as gm
from wide_gap_model import MISSING
from wide_hom_model import plan_rule, chain_rule, hom_pilot, hom_matrix, hom_chain_vs_sweep, hom_matrix_ref, chain_errors, hom_sandwich, hom_mixed


def toy():
    """12 tiles of 10 bins, hets at every seventh bin; tile 4 missing, tiles 5 and 6 homozygous, tile 7 half homozygous half missing,
    tile 8 homozygous.  With a warm-up of 20 tiles 0 .. 2 are anchored forward and tiles 9 .. 11 backward."""
    s = np.zeros(120, dtype=np.uint8)
    s[::7] = 1
    s[40:50] = MISSING
    s[50:70] = 0
    s[70:75] = 0; s[75:80] = MISSING
    s[80:90] = 0
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


def test_rule_by_hand():
    """The toy, worked out from the rule's text.  Both options on, minima 10 (gap) and 20 (hom): tiles 4 .. 6 are ONE run that qualifies
    through both; the mix tile 7 is data and ends it; tile 8 alone is 10 bins of hom, class 3.  Forward the run's tiles and the tiles
    whose window lo - 20 .. lo - 1 reaches positions 41 .. 70: 7 (51 .. 70) and 8 (61 .. 80); backward tiles 3 (41 .. 60) and 2 (31 .. 50)."""
    s = toy()
    both = plan_rule([s], 10, 20, gap_min=10, hom_min=20, gap=True, hom=True)
    assert same(both, expect(12, cls=[(2, (4,)), (4, (5, 6)), (3, (8,))], fwd=(4, 5, 6, 7, 8), bwd=(2, 3, 4, 5, 6)))
    # through the gap threshold alone (hom minimum out of reach), and through the hom threshold alone: the same run, whole
    assert same(plan_rule([s], 10, 20, gap_min=10, hom_min=500, gap=True, hom=True), both)
    assert same(plan_rule([s], 10, 20, gap_min=500, hom_min=20, gap=True, hom=True), both)
    # neither: classes 1 and 3, nothing glued
    assert same(plan_rule([s], 10, 20, gap_min=500, hom_min=500, gap=True, hom=True), expect(12, cls=[(1, (4,)), (3, (5, 6, 8))]))
    # hom alone: the missing tile is data; the run is tiles 5, 6
    assert same(plan_rule([s], 10, 20, hom_min=20), expect(12, cls=[(4, (5, 6)), (3, (8,))], fwd=(5, 6, 7, 8), bwd=(3, 4, 5, 6)))
    # ... and with a minimum of 10 tile 8 is a run of its own BEHIND the mix tile: glued tiles 9 (window 71 .. 90) and 10 forward, 7 backward
    assert same(plan_rule([s], 10, 20, hom_min=10), expect(12, cls=[(4, (5, 6, 8))], fwd=(5, 6, 7, 8, 9, 10), bwd=(3, 4, 5, 6, 7, 8)))
    # the chains: the walk behind tiles 5, 6 goes through the mix tile; the run that resumes behind it is one level later, both ways
    assert chain_rule([s], 10, 20, hom_min=10) == ([(5, 2, 7, 0), (8, 1, 9, 1)], [(8, 1, 7, 0), (6, 2, 4, 1)])
    assert chain_rule([s], 10, 20, gap_min=10, hom_min=20, gap=True, hom=True) == ([(4, 3, 7, 0)], [(6, 3, 3, 0)])
    # auto: a quarter of the warm-up = 5 bins
    assert same(plan_rule([s], 10, 20), plan_rule([s], 10, 20, hom_min=10))


def test_rule_reduces_to_the_gap_rule(golden):
    """hom off: classes, glue bits and chains are plan_rule's and chain_rule's of tests/wide_gap_model.py, on the toy, on the inputs of
    both GPU test files and on the gap tests' own -- whatever hom_min says; both off: nothing."""
    src = golden.segs_mid[3]
    inputs = [([toy()], 10, 20, 10), (hom_mixed(src, golden.segs_mid[4]), 100, 30, 1000), (hom_mixed(src, golden.segs_mid[4]), 37, 5, 1000),
              ([hom_sandwich(src)], 64, 512, 0), ([gm.twin(src)], 64, 512, 0), ([gm.triple(src)], 64, 256, 128),
              (gm.mixed(src, golden.segs_mid[4]), 100, 30, 1000)]
    for segs, T, W, m in inputs:
        for hom_min in (0, 1, 1000):
            got = plan_rule(segs, T, W, gap_min=m, hom_min=hom_min, gap=True, hom=False)
            assert same(got, gm.plan_rule(segs, T, W, m)), (T, W, m)
            assert chain_rule(segs, T, W, gap_min=m, hom_min=hom_min, gap=True, hom=False) == gm.chain_rule(segs, T, W, m)
        none = plan_rule(segs, T, W, gap_min=m, gap=False, hom=False)
        assert not none[0].any() and not none[1].any()


def test_inputs_of_the_gpu_tests(golden):
    """hom_sandwich at tiles of 64 bins and a warm-up of 512: 63 tiles of class 4, at least 59 glued each way, one chain per direction.
    hom_mixed at tiles of 100 bins, minima 1000: hom alone -- the 3000-bin run, the 1200 bins behind the mix stretch (one level later at a warm-up of 400), the
    1000 bins behind the missing data, and the 200-bin run class 3; with the gap option the missing data and the hom bins behind it are
    ONE run of both classes; a mix tile is class 0 and ends the run in front of it."""
    segs = [hom_sandwich(golden.segs_mid[3])]
    assert len(segs[0]) == 4696
    cls, glue = plan_rule(segs, 64, 512)
    assert (cls == 4).sum() == 63 and list(np.flatnonzero(cls == 4)) == list(range(5, 68))
    assert list(np.flatnonzero(cls == 3)) == [1, 70]   # het-free tiles of the called pieces themselves: too short to qualify
    assert (glue & 1).sum() >= 59 and (glue & 2).sum() >= 59
    f, b = chain_rule(segs, 64, 512)
    assert len(f) == 1 and len(b) == 1 and f[0][3] == 0 and b[0][3] == 0
    segs = hom_mixed(golden.segs_mid[3], golden.segs_mid[4])
    cls, glue = plan_rule(segs, 100, 30, hom_min=1000)
    assert set(np.flatnonzero(cls == 4)) >= set(range(15, 45)) | set(range(48, 60)) | set(range(95, 105))
    assert cls[45] == 0 and cls[46] == 0 and cls[47] == 0 and cls[70] == 3 and cls[71] == 3 and not cls[85:95].any()
    f, b = chain_rule(segs, 100, 30, hom_min=1000)
    lev = {c[0]: c[3] for c in f}
    assert lev[15] == 0 and lev[48] == 0 and lev[95] == 0, f   # (a warm-up of 30 glues tile 45 only: tile 47 speculates)
    f4, b4 = chain_rule(segs, 100, 400, hom_min=1000)            # a warm-up of 400: the walk behind tile 44 goes through the mix tiles 45 .. 47
    assert (48, 12, 60, 1) in f4 and (44, 30, 14, 1) in b4, (f4, b4)
    cls2, _ = plan_rule(segs, 100, 30, gap_min=1000, hom_min=1000, gap=True, hom=True)
    assert (cls2[85:95] == 2).all() and (cls2[95:105] == 4).all()
    assert (95, 10, 105, 0) in f and (85, 20, 105, 0) in chain_rule(segs, 100, 30, gap_min=1000, hom_min=1000, gap=True, hom=True)[0]
    # through either threshold: 1000 missing bins alone, or 1000 hom bins alone, qualify the whole run
    for gmin, hmin in ((1000, 5000), (5000, 1000)):
        c3, _ = plan_rule(segs, 100, 30, gap_min=gmin, hom_min=hmin, gap=True, hom=True)
        assert (c3[85:95] == 2).all() and (c3[95:105] == 4).all(), (gmin, hmin)
    c4, _ = plan_rule(segs, 100, 30, gap_min=5000, hom_min=5000, gap=True, hom=True)
    assert (c4[85:95] == 1).all() and (c4[95:105] == 3).all()


@pytest.mark.parametrize("T", [64, 7360])
def test_hom_matrix_matches_the_sweep(T):
    """n149.a / e, forward and backward: one application of the pilot-scaled M_h (backward: D M_h D^-1) against T single steps from the
    same vector, up to a positive factor (tile_mismatch's metric), within 1e-12, over 40 tiles (2 at T = 7360); and the pilot's
    power-of-two factors alone hold the pilot's sum within [2^-4, 2^4] at every bin -- so no row of M_h, at most n times the pilot
    elementwise, can overflow, and M_h itself is finite and non-negative with no row of zeros."""
    w = dict(np.load(os.path.join(GOLD, "estep_wide.npz")))
    a, e, a0 = w["n149.a"], w["n149.e"], w["n149.a0"]
    e0 = e[0]
    tiles = 40 if T == 64 else 2
    fac, lo, hi = hom_pilot(a, e0, T)
    assert len(fac) == (T + 3) // 4 and (np.frexp(fac)[0] == 0.5).all()   # powers of two
    assert 2.0 ** -4 <= lo and hi <= 2.0 ** 4, (lo, hi)
    M = hom_matrix(a, e0, T, fac)
    assert np.isfinite(M).all() and (M >= 0).all() and (M.max(1) > 0).all()
    pilot = M.sum(0) / len(a0)
    assert (M <= len(a0) * pilot[None, :] * (1 + 1e-9)).all()
    x0 = a0 * e0 * (1.0 + 0.5 * np.sin(np.arange(len(a0))))
    f = hom_chain_vs_sweep(a, e0, x0, T, tiles)
    b = hom_chain_vs_sweep(a, e0, e[1] * (1.0 + 0.5 * np.cos(np.arange(len(a0)))), T, tiles, backward=True)
    print("hom chain against sweep, T = %d: forward %.2e backward %.2e; pilot sum in [%.3g, %.3g], product of the factors 2^%d" % (
        T, f, b, lo, hi, int(np.log2(fac).sum())))
    assert f <= 1e-12 and b <= 1e-12, (f, b)


def test_hom_references():
    """The unscaled M_h in long double: the binary power and the stepped rows agree, and the float64 pilot-scaled matrix with its
    factors undone is within T (4 n + 1) 2^-53 per row of it by a wide margin (the bound of tests/test_gpu_wide_hom_chain.py is no
    measurement).  The per-application gate on a float64 restatement of the chain: the faithful one passes (2 n + 2) 2^-53 both
    ways, one that forgets D^-1 backward is far outside."""
    w = dict(np.load(os.path.join(GOLD, "estep_wide.npz")))
    a, e = w["n149.a"], w["n149.e"]
    e0, n, T, S = e[0], 149, 64, 192
    ref = hom_matrix_ref(a, e0, T)
    rows = [0, 1, 100, 147, 148]
    assert float(np.abs(hom_matrix_ref(a, e0, T, rows) - ref[rows]).max() / ref.max()) < 1e-17
    fac, _, _ = hom_pilot(a, e0, T)
    M = hom_matrix(a, e0, T, fac)
    err = float((np.abs(M.astype(np.longdouble) / np.prod(fac.astype(np.longdouble)) - ref).max(1) / ref.max(1)).max())
    bound = T * (4 * n + 1) * 2.0 ** -53
    print("float64 M_h against long double, n = 149, T = 64: %.2e (bound %.2e)" % (err, bound))
    assert err <= bound / 50
    Mp = np.zeros((n, S)); Mp[:, :n] = M
    x0 = np.zeros(S); x0[:n] = w["n149.a0"] * e0 * (1.0 + 0.5 * np.sin(np.arange(n)))
    tiles = 6

    def chain(backward, dinv=True):
        v, out = x0.copy(), [x0.copy()]
        for _ in range(tiles):
            y = np.zeros(S)
            if backward:
                y[:n] = e0 * (Mp @ np.concatenate([v[:n] / e0 if dinv else v[:n], v[n:]]))
            else:
                y = v[:n] @ Mp
            v = y / y.sum()
            out.append(v)
        return np.array(out)

    cls = np.full(tiles + 1, 4)
    gate = (2 * n + 2) * 2.0 ** -53
    good_f, seen = chain_errors(n, None, Mp, e0, cls, chain(False), [(0, tiles, tiles, 0)], False)
    good_b, _ = chain_errors(n, None, Mp, e0, cls, chain(True)[::-1], [(tiles, tiles, 0, 0)], True)
    bad_b, _ = chain_errors(n, None, Mp, e0, cls, chain(True, dinv=False)[::-1], [(tiles, tiles, 0, 0)], True)
    print("hom chain gate: faithful %.1e / %.1e, without D^-1 %.1e, bound %.1e" % (good_f, good_b, bad_b, gate))
    assert seen == [0, tiles] and good_f <= gate and good_b <= gate and bad_b > 100 * gate
