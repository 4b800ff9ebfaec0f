"""CPU side of "wide_mix_tiles" (tests/test_gpu_wide_mix.py and tests/test_gpu_wide_mix_chain.py hold the GPU side): (1) the plan rule
of tests/wide_mix_model.py against plan_rule of tests/wide_hom_model.py whenever no mix tile is in play, on hom_mixed and under the
cap; (2) the two matrices of a mix tile, built row by row from the shifted sequence as the kernels build them, against T single
steps of the sweeps and against long double, and their reduction on a pure hom tile; (3) the pilots' factors; and the arrangement of
the input mix_sandwich."""
import os
import numpy as np
import pytest
from conftest import GOLD
import wide_gap_model as gm
import wide_hom_model as hm
from wide_gap_model import MISSING, mismatch
from wide_hom_model import hom_mixed, hom_sandwich, hom_pilot, hom_matrix
from wide_mix_model import (plan_rule, chain_rule, cap_tiles, sequence, mix_pilot, mix_matrix, mix_matrix_ref, PairRef, sweep, chain_errors,
                            mix_sandwich, tile_symbols, HOM_PAIR, GAP_PAIR, N_FIRST, N_LAST)

U = 2.0 ** -53


@pytest.fixture(scope="module")
def wide():
    return dict(np.load(os.path.join(GOLD, "estep_wide.npz")))


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def tile_class(t):
    """k_tile_class: 0 het, 1 all missing, 2 all homozygous, 3 het-free with both"""
    t = np.asarray(t)
    return 0 if (t == 1).any() else (1 if (t == MISSING).all() else (2 if (t == 0).all() else 3))


# ------------------------------------------------------------------ (1) the plan rule
def test_rule_reduces_to_the_hom_rule(golden):
    """Without a mix tile in play -- `mix` off, a cap of no tile, or an input without a class-3 chain tile -- classes, glue bits and
    chains are those of tests/wide_hom_model.py, whatever the other options say."""
    src = golden.segs_mid[3]
    busy = gm._called(golden.segs_mid[4][:2500]).copy()
    busy[31::60] = 1
    inputs = [(hom_mixed(src, golden.segs_mid[4]), 100, 30, 1000), (hom_mixed(src, golden.segs_mid[4]), 37, 5, 1000),
              ([mix_sandwich(src)], 64, 512, 0), ([hom_sandwich(src)], 64, 512, 0), ([gm.triple(src)], 64, 256, 128)]
    for segs, T, W, m in inputs:
        for gap in (False, True):
            for hom in (False, True):
                r = dict(gap_min=m, hom_min=m, gap=gap, hom=hom)
                want = hm.plan_rule(segs, T, W, **r)
                for off in (dict(mix=False), dict(mix=True, mix_tiles=0)):
                    got = plan_rule(segs, T, W, **r, **off)
                    if hom and off["mix"]:   # refused tiles are class 5 in the report, and nothing else differs
                        assert set(got[0][got[0] != want[0]]) <= {5} and not want[0][got[0] == 5].any()
                        assert np.array_equal(got[1], want[1])
                    else:
                        assert same(got, want), (T, W, m, gap, hom, off)
                    if gap or hom:
                        assert chain_rule(segs, T, W, **r, **off) == hm.chain_rule(segs, T, W, **r)
                if not hom:                  # the option has an effect only with "wide_hom_tiles"
                    assert same(plan_rule(segs, T, W, **r, mix=True), want)
    for segs, T, W in (([busy], 64, 256), ([hom_sandwich(src)[300:4396]], 64, 512)):   # no class-3 tile at all
        assert same(plan_rule(segs, T, W), hm.plan_rule(segs, T, W))
        assert not (plan_rule(segs, T, W)[0] >= 5).any()


def test_rule_on_hom_mixed(golden):
    """hom_mixed at tiles of 100 bins, "wide_hom_min" = 1000: the 300 alternating bins (tiles 45 .. 47) join the 3000-bin run in front of
    them and the 1200 bins behind them into ONE run, tiles 15 .. 59; the chains of that stretch collapse from two per direction (the
    second one level later at a warm-up of 400) to one.  With a cap of two tiles tile 47 is refused: class 5, and it ends the run as
    before.  The tile across the border of the 1000 missing and the 1000 hom bins does not exist at tiles of 100 -- at tiles of 37 it
    does, and joins both with the gap option when its 37 bins are what the hom tiles behind it lack of "wide_hom_min"."""
    segs = hom_mixed(golden.segs_mid[3], golden.segs_mid[4])
    cls, glue = plan_rule(segs, 100, 400, hom_min=1000)
    old, _ = hm.plan_rule(segs, 100, 400, hom_min=1000)
    assert list(old[45:48]) == [0, 0, 0] and list(cls[45:48]) == [6, 6, 6]
    assert (cls[15:45] == 4).all() and (cls[48:60] == 4).all() and cls[14] == 0 and cls[60] == 0
    f, b = chain_rule(segs, 100, 400, hom_min=1000)
    f0, b0 = hm.chain_rule(segs, 100, 400, hom_min=1000)
    assert (48, 12, 60, 1) in f0 and (44, 30, 14, 1) in b0
    assert (15, 45, 60, 0) in f and (59, 45, 14, 0) in b and len(f) == len(f0) - 1 and len(b) == len(b0) - 1, (f, b)
    capped, _ = plan_rule(segs, 100, 400, hom_min=1000, mix_tiles=2)
    assert list(capped[45:48]) == [6, 6, 5] and (capped[48:60] == 4).all()
    assert chain_rule(segs, 100, 400, hom_min=1000, mix_tiles=2)[0].count((48, 12, 60, 1)) == 1
    # mix bins count towards "wide_hom_min": tiles 45 .. 47 alone are 300 bins; with the 200-bin hom run at 7000 nothing changes
    assert (cls[70:72] == 3).all()
    lone = [np.concatenate([gm._called(golden.segs_mid[3][:1000]), segs[0][4500:4800], gm._called(golden.segs_mid[3][1000:2000])])]
    assert (plan_rule(lone, 100, 30, hom_min=300)[0][10:13] == 6).all() and (plan_rule(lone, 100, 30, hom_min=301)[0][10:13] == 5).all()
    c37, _ = plan_rule(segs, 37, 5, gap_min=1000, hom_min=999, gap=True)   # (26 full hom tiles and the mix tile: 999 bins)
    assert plan_rule(segs, 37, 5, gap_min=1000, hom_min=1000, gap=True)[0][9500 // 37] == 5
    t = 9500 // 37
    assert tile_class(tile_symbols(segs[0], 37, t)) == 3 and c37[t] == 6 and c37[t - 1] == 2 and c37[t + 1] == 4


def test_cap_figures():
    """the figures of the header: 16.8 MB per tile at 1024 states, about 120 tiles under the default; 0.8 MB at 200 states, about 2500;
    "wide_mix_mb" = 1 admits no tile at 1024 states"""
    assert 16 * 1024 * 1024 == 16777216 and cap_tiles(1024, 2048) == 122
    assert 16 * 200 * 256 == 819200 and cap_tiles(200, 2048) == 2500
    assert cap_tiles(1024, 1) == 0 and cap_tiles(200, 1) == 1


def test_mix_sandwich_arrangement(golden):
    """The input of the GPU tests, at tiles of 64 bins and a warm-up of 512.  Every tile that lies inside the het-free stretch (5 .. 67)
    is class 3 of k_tile_class, except the stretch of two pure hom tiles (20, 21) and the stretch of two pure gap tiles (40, 41) that
    the same run must hold; at least one class-3 tile has N first, at least one has N last; the N positions are irregular (the tiles'
    patterns are pairwise different) and the same at every call.  With all three options tiles 5 .. 67 are ONE run of all three kinds."""
    s = mix_sandwich(golden.segs_mid[3])
    assert len(s) == 4696 and np.array_equal(s, mix_sandwich(golden.segs_mid[3]))
    assert np.array_equal(s[:300], hom_sandwich(golden.segs_mid[3])[:300]) and np.array_equal(s[4396:], hom_sandwich(golden.segs_mid[3])[4396:])
    kinds = [tile_class(tile_symbols(s, 64, b)) for b in range(5, 68)]
    for b, k in zip(range(5, 68), kinds):
        assert k == (2 if b in HOM_PAIR else (1 if b in GAP_PAIR else 3)), (b, k)
    mixes = [b for b in range(5, 68) if b not in HOM_PAIR + GAP_PAIR]
    assert any(tile_symbols(s, 64, b)[0] == MISSING for b in mixes) and tile_symbols(s, 64, N_FIRST)[0] == MISSING and tile_symbols(s, 64, N_FIRST)[-1] == 0
    assert any(tile_symbols(s, 64, b)[-1] == MISSING for b in mixes) and tile_symbols(s, 64, N_LAST)[-1] == MISSING and tile_symbols(s, 64, N_LAST)[0] == 0
    assert len({tile_symbols(s, 64, b).tobytes() for b in mixes}) == len(mixes)
    rule = dict(gap=True, hom=True)
    cls, glue = plan_rule([s], 64, 512, **rule)
    want = [4 if b in HOM_PAIR else (2 if b in GAP_PAIR else 6) for b in range(5, 68)]
    assert list(cls[5:68]) == want and cls[4] == 0 and cls[68] == 0
    f, b = chain_rule([s], 64, 512, **rule)
    assert len(f) == 1 and len(b) == 1 and f[0][3] == 0 and b[0][3] == 0 and f[0][1] >= 55 and b[0][1] >= 55
    # without the option the two pure stretches are lone runs of two tiles (128 bins: just "wide_hom_min" / "wide_gap_min" auto) between
    # data tiles -- what the scattered N bins of real data leave of a run of homozygosity
    old, _ = hm.plan_rule([s], 64, 512, **rule)
    assert sorted(5 + np.flatnonzero(old[5:68])) == sorted(HOM_PAIR + GAP_PAIR) and list(old[[20, 21, 40, 41]]) == [4, 4, 2, 2]
    # without "wide_gap_tiles" the two gap tiles are data: two runs
    c2, _ = plan_rule([s], 64, 512)
    assert not c2[40:42].any() and (c2[5:40] >= 4).all() and (c2[42:68] == 6).all()


# ------------------------------------------------------------------ (2) identities
def tiles_for(T, seed):
    """a tile whose first bin is N, one whose last bin is N, one that starts and ends homozygous -- N at irregular positions inside"""
    rng = np.random.default_rng(seed)
    out = {}
    for name in ("N first", "N last", "hom ends"):
        t = np.where(rng.random(T) < 0.2, MISSING, 0).astype(np.uint8)
        t[0], t[-1] = 0, 0
        if name == "N first":
            t[0] = MISSING
        if name == "N last":
            t[-1] = MISSING
        out[name] = t
    return out


@pytest.mark.parametrize("n", [149, 200])
def test_mix_matrices_match_the_sweeps(wide, n):
    """T = 64.  F and B are built row by row from the (shifted) sequence with their pilots' factors, as the kernels build them.  T single
    forward steps from a random positive vector equal x F up to scale, T single backward steps equal B y up to scale (tile_mismatch's
    metric, within 1e-12 in float64); against the long-double product of the single steps both matrices, factors undone, are within
    T (4 n + 1) u per row (on twelve rows across the lanes) -- the bound of the GPU test, met here by a wide margin.  A B built from the UNshifted sequence is far off."""
    a, e = wide["n%d.a" % n], wide["n%d.e" % n]
    e0, T = e[0], 64
    rng = np.random.default_rng(n)
    for name, sym in tiles_for(T, 7).items():
        x0, y0 = rng.random(n) + 0.05, rng.random(n) + 0.05
        mats = []
        for dr in (0, 1):
            fac, lo, hi = mix_pilot(a, e0, sym, dr)
            assert len(fac) == (T + 3) // 4 and (np.frexp(fac)[0] == 0.5).all()
            M = mix_matrix(a, e0, sym, dr, fac)
            assert np.isfinite(M).all() and (M >= 0).all() and (M.max(1) > 0).all()
            rows = sorted({0, 1, 2, 63, 64, 65, 127, 128, n // 2, n - 3, n - 2, n - 1})   # (every row would take 2 s per matrix)
            ref = mix_matrix_ref(a, e0, sym, dr, rows)
            err = float((np.abs(M[rows].astype(np.longdouble) / np.prod(fac.astype(np.longdouble)) - ref).max(1) / ref.max(1)).max())
            assert err <= T * (4 * n + 1) * U / 50, (name, dr, err)
            mats.append(M)
        F, B = mats
        f = mismatch(x0 @ F, sweep(a, e0, sym, x0, False))
        b = mismatch(B @ y0, sweep(a, e0, sym, y0, True))
        print("mix tile (%s) n %d: x F against the sweep %.2e, B y against the sweep %.2e" % (name, n, f, b))
        assert f <= 1e-12 and b <= 1e-12, (name, f, b)
        # F and B are genuinely different maps: B is NOT D F D^-1 on a mix tile
        dfd = e0[:, None] * F / e0[None, :]
        assert mismatch(dfd @ y0, sweep(a, e0, sym, y0, True)) > 1e-6, name


@pytest.mark.parametrize("n", [149, 200])
def test_mix_matrices_on_a_pure_hom_tile(wide, n):
    """On a pure hom tile F reduces to hom_matrix of tests/wide_hom_model.py -- the same bits, pilot and rows -- and B to D M_h D^-1 up
    to scale: row k of B is e0_k e_k (a D)^(T-1) a."""
    a, e = wide["n%d.a" % n], wide["n%d.e" % n]
    e0, T = e[0], 64
    sym = np.zeros(T, np.uint8)
    fac, _, _ = mix_pilot(a, e0, sym, 0)
    hfac, _, _ = hom_pilot(a, e0, T)
    assert np.array_equal(fac, hfac)
    F = mix_matrix(a, e0, sym, 0, fac)
    Mh = hom_matrix(a, e0, T, hfac)
    assert np.array_equal(F, Mh)
    fb, _, _ = mix_pilot(a, e0, sym, 1)
    B = mix_matrix(a, e0, sym, 1, fb)
    want = e0[:, None] * Mh / e0[None, :]
    scale = B.sum() / want.sum()
    rel = np.abs(B - scale * want).max(1) / (scale * want).max(1)
    assert float(rel.max()) <= T * (4 * n + 1) * U, float(rel.max())
    # and on a pure gap tile both are a to the power T
    gap = np.full(T, MISSING, np.uint8)
    P = np.linalg.matrix_power(a, T)
    for dr in (0, 1):
        M = mix_matrix(a, e0, gap, dr, mix_pilot(a, e0, gap, dr)[0])
        M = M / M.sum() * P.sum()
        assert float((np.abs(M - P).max(1) / P.max(1)).max()) <= 4 * T * n * U


def test_pair_reference_is_the_stepped_product(wide):
    """PairRef -- the long-double product of the T single-step matrices associated through the shared core and the powers of a D, what
    tests/test_gpu_wide_mix_chain.py compares whole matrices with -- against mix_matrix_ref, which steps the rows one bin at a time:
    both matrices of the three kinds of tile, of a pure hom tile and of a pure gap tile agree within 2 T n 2^-64 of the
    row's largest (each is T products of at most n non-negative terms rounded to 64 bits)."""
    n, T = 149, 64
    a, e = wide["n149.a"], wide["n149.e"]
    ref = PairRef(a, e[0])
    tiles = dict(tiles_for(T, 7), hom=np.zeros(T, np.uint8), gap=np.full(T, MISSING, np.uint8))
    for name, sym in tiles.items():
        F, B = ref.pair(sym)
        for dr, M in ((0, F), (1, B)):
            rows = list(range(0, n, 7)) + [n - 1]   # (the stepped side costs T products per row set: every seventh row and the last)
            want = mix_matrix_ref(a, e[0], sym, dr, rows)
            err = float((np.abs(M[rows] - want).max(1) / want.max(1)).max())
            assert err <= 2 * T * n * 2.0 ** -64, (name, dr, err)


# ------------------------------------------------------------------ (3) the pilots
def test_pilot_factors_at_the_genome_tile(wide):
    """T = 7360, the benchmark genome's tile, N at three short stretches per tile as the simulated genome has them, n = 149: the
    ceil(T / 4) factors of either direction are powers of two, and they alone hold the pilot's sum within [2^-4, 2^4] at every bin -- so
    no row of either matrix, at most n times its pilot elementwise (checked on five rows), can overflow."""
    a, e = wide["n149.a"], wide["n149.e"]
    e0, T, n = e[0], 7360, 149
    rng = np.random.default_rng(3)
    sym = np.zeros(T, np.uint8)
    for at in rng.integers(0, T - 40, 3):
        sym[at:at + int(rng.integers(5, 40))] = MISSING
    sym[0] = MISSING
    for dr in (0, 1):
        fac, lo, hi = mix_pilot(a, e0, sym, dr)
        assert len(fac) == T // 4 and (np.frexp(fac)[0] == 0.5).all()
        assert 2.0 ** -4 <= lo and hi <= 2.0 ** 4, (dr, lo, hi)
        rows = [0, 1, 74, 147, 148]
        x = np.zeros((len(rows), n)); x[np.arange(len(rows)), rows] = 1.0
        u = np.full(n, 1.0 / n)
        if dr == 1 and sym[0] == 0:
            x = x * e0[None, :]
        for p, o in enumerate(sequence(sym, dr)):
            if p % 4 == 0:
                x, u = x * fac[p // 4], u * fac[p // 4]
            ev = e0 if o == 0 else np.ones(n)
            x, u = (x @ a) * ev[None, :], (u @ a) * ev
            assert np.isfinite(x).all()
        assert (x <= n * u[None, :] * (1 + 1e-9)).all() and (x.max(1) > 0).all()
        print("mix pilot T %d dir %d: sum in [%.3g, %.3g], product of the factors 2^%d" % (T, dr, lo, hi, int(np.log2(fac).sum())))


def test_chain_gate(wide):
    """The per-application gate of tests/test_gpu_wide_mix_chain.py on a float64 restatement of the chain across three mix tiles: the
    faithful chain passes (2 n + 2) u both ways; one that applies D F D^-1 backward instead of B is far outside."""
    n, T, S = 149, 64, 192
    a, e = wide["n149.a"], wide["n149.e"]
    e0 = e[0]
    tiles = list(tiles_for(T, 11).values())
    FB = []
    for sym in tiles:
        FB.append([np.pad(mix_matrix(a, e0, sym, dr, mix_pilot(a, e0, sym, dr)[0]), ((0, 0), (0, S - n))) for dr in (0, 1)])
    x0 = np.zeros(S); x0[:n] = wide["n149.a0"] * e0 * (1.0 + 0.5 * np.sin(np.arange(n)))
    cls = np.array([6, 6, 6, 0])

    def chain(backward, wrong=False):
        v, out = x0.copy(), [x0.copy()]
        for i in range(3):
            t = 2 - i if backward else i
            y = np.zeros(S)
            if backward:
                A = e0[:, None] * FB[t][0][:, :n] / e0[None, :] if wrong else FB[t][1][:, :n]
                y[:n] = A @ v[:n]
            else:
                y = v[:n] @ FB[t][0]
            v = y / y.sum()
            out.append(v)
        return np.array(out)

    gate = (2 * n + 2) * U
    good_f, seen = chain_errors(n, None, None, {t: FB[t][0] for t in range(3)}, e0, cls, chain(False), [(0, 3, 3, 0)], False)
    mb = {t: FB[t][1] for t in range(3)}
    vb = np.zeros((4, S)); vb[[2, 1, 0]] = chain(True)[:3]
    # backward: the chain starts at tile 2 (first) with vec[2] and writes tiles 1, 0 -- crossing tiles 2, 1
    good_b, _ = chain_errors(n, None, None, mb, e0, cls, vb, [(2, 2, 0, 0)], True)
    wb = np.zeros((4, S)); wb[[2, 1, 0]] = chain(True, wrong=True)[:3]
    bad_b, _ = chain_errors(n, None, None, mb, e0, cls, wb, [(2, 2, 0, 0)], True)
    print("mix chain gate: faithful %.1e / %.1e, D F D^-1 backward %.1e, bound %.1e" % (good_f, good_b, bad_b, gate))
    assert seen == [0, 0, 3] and good_f <= gate and good_b <= gate and bad_b > 100 * gate
