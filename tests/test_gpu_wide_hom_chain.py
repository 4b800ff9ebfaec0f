"""The transfer-matrix chain of "wide_hom_tiles" looked at directly (psmc_amd/csrc/estep_wide_gap.hip k_wf_hompilot / k_wf_hommat /
k_wf_gapchain HOM), in the manner of tests/test_gpu_wide_gap_chain.py: tests/test_gpu_wide_hom.py judges the E-step's statistics,
where a wrong matrix or chain is invisible (k_wf_verify catches the vector and a repair walks the run).  Here
  (a) M_h from psmc_hip_wide_hom_matrix, the pilot's powers of two undone, against the long-double product of T single steps,
  (b) every application of the chain (psmc_hip_wide_tile_vectors) against the long-double product of the DEVICE's matrix of the
      crossed tile's class and the DEVICE's previous vector -- hom tiles alone, and runs that hold gap tiles and hom tiles,
  (c) the matrix of the benchmark genome's tile length, 7360 bins: finite, and no row lost against the pilot,
  (d) the two harsh models of tests/test_gpu_wide_gap_chain.py.
Lines that start with HOMTEST (shown with -s) are the figures profiles/wide_hom_tests.txt records.

Bounds, u = 2^-53.  (a) per row max_j |M - Mref| / max_j Mref <= T (4 n + 1) u, and the same per cell on the cells of at least
1e-6 x the row's largest (the project's cell rule).  4 T n u is the bound of tests/test_gpu_wide_gap_chain.py for the same sweep
under the missing symbol: each of the T steps forms an entry from at most n non-negative products and a fixed number of scan levels.
Under symbol 0 every step multiplies the entry by e0 once more -- one rounding, a factor within 1 +- u per step, T u in all: the term
the emission adds.  The pilot's factors are powers of two and add nothing; the reference is (a D)^T in long double from the same
float64 a and e0.  (b) per cell (2 n + 2) u on the cells of at least 1e-6 x the vector's largest: 2 n u as in that file (one sum of n
non-negative products, one sum of n terms for the norm, one reciprocal, one product); backward across a hom tile the product is
e0_k sum_j M_h[k][j] (v_j / e0_j) -- the division adds one rounding to every term of a sum of non-negative terms, u on the sum, and
the product by e0_k one more.  Forward, and across gap tiles, the bound of that file holds and the larger one is not needed; one bound
is asserted for all.  Neither bound was taken from what the kernels give."""
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal, GOLD
from test_gpu_wide_fast import check
from test_gpu_wide_gap import reference, run, work, level
from test_gpu_wide_gap_chain import params, width, boundary_rows, HARSH, U
from wide_gap_model import tiles_missing, MISSING
from wide_hom_model import plan_rule, chain_rule, chain_errors, hom_matrix_ref, hom_sandwich, hom_mixed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAND = dict(chunk=64, warmup=512)


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module")
def wide():
    return dict(np.load(os.path.join(GOLD, "estep_wide.npz")))


def unscaled(M, fac):
    """the device's M_h with the pilot's powers of two undone, in long double (exact: the product of the factors is a power of two)"""
    return M.astype(np.longdouble) / np.prod(fac.astype(np.longdouble))


# ------------------------------------------------------------------ (a) + (b): matrix and chain on the sandwich
CASES = [(n, "mild") for n in (149, 192, 193, 256, 257, 1024)] + [(n, m) for m in HARSH for n in (200, 1024)]


@pytest.mark.parametrize("n, model", CASES, ids=lambda v: str(v))
def test_hommat_and_chain(hip, golden, wide, n, model):
    """hom_sandwich at tiles of 64 bins, warm-up 512 -- on and just past every padded width, and the two harsh models.  The matrix: the
    whole of it up to 257 states, beyond them the rows on the lane, wave and padding boundaries, per row and per cell within
    T (4 n + 1) u of (a D)^T in long double; padded columns exactly 0; the factors are the ceil(T / 4) powers of two; a second E-step
    builds the same bits.  The chain: on the mild models no repair round runs, so entry / bentry of the chained tiles are the chain's
    own vectors, and every one is the normalised product of the device's matrix and the vector before it within (2 n + 2) u per cell.
    (On the harsh models repair rounds may run and rewrite vectors: there the matrix is judged, and the chain by the statistics.)"""
    par = params(n, wide, model)
    T = 64
    segs = [hom_sandwich(golden.segs_mid[3])]
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), wide_hom_tiles=1, **SAND)
    es.load_segments(segs)
    try:
        es.estep_factored(par[0], par[1][:2], par[2])
        M, fac = es.wide_hom_matrix()
        es.estep_factored(par[0], par[1][:2], par[2])
        M2, fac2 = es.wide_hom_matrix()
        d = es.fast_diag()
        chains = es.wide_gap_chains()
        cls = es.wide_plan_tiles()["cls"]
        vec = [es.wide_tile_vectors(0), es.wide_tile_vectors(1)]
        again = es.wide_gap_rechained()
    finally:
        es.close()
    S = width(n)
    assert M.shape == (n, S) and np.isfinite(M).all() and (M >= 0).all()
    assert bits_equal(M, M2) and bits_equal(fac, fac2)
    assert not M[:, n:].any()
    assert fac.shape == ((T + 3) // 4,) and (np.frexp(fac)[0] == 0.5).all()
    rows = list(range(n)) if n <= 257 else boundary_rows(n)
    e0 = par[1][0]
    ref = hom_matrix_ref(par[0], e0, T, None if n <= 257 else rows)
    got = unscaled(M, fac)[rows, :n]
    bound = T * (4 * n + 1) * U
    top = ref.max(1)
    dd = np.abs(got - ref)
    row_err = dd.max(1) / top
    big = ref >= 1e-6 * top[:, None]
    cell_err = np.where(big, dd / np.where(big, ref, 1), 0).max(1)
    print("HOMTEST hommat n %d T %d %s: worst row %.2e (row %d) worst cell %.2e (row %d) bound %.2e -- shares %.3f / %.3f; product of the factors 2^%d; smallest row maximum %.1e" % (
        n, T, model, float(row_err.max()), rows[int(row_err.argmax())], float(cell_err.max()), rows[int(cell_err.argmax())], bound,
        float(row_err.max()) / bound, float(cell_err.max()) / bound, int(np.log2(fac).sum()), float(top.min())))
    assert float(row_err.max()) <= bound, (n, model, float(row_err.max()), bound)
    assert float(cell_err.max()) <= bound, (n, model, float(cell_err.max()), bound)
    assert chains == list(chain_rule(segs, 64, 512)), chains
    if model != "mild":
        print("HOMTEST harsh %s n %d: %s rechained %s" % (model, n, work(d), again))
        return
    assert d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0 and again == [0, 0], (d, again)
    gate = (2 * n + 2) * U
    out = []
    for dr in (0, 1):
        worst, seen = chain_errors(n, None, M, e0, cls, vec[dr], chains[dr], dr == 1)
        assert seen == [0, sum(c[1] for c in chains[dr])] and seen[1] > 0
        out.append(worst)
    print("HOMTEST homchain n %d: worst cell per application forward %.2e backward %.2e bound %.2e -- shares %.3f / %.3f (%d + %d applications)" % (
        n, out[0], out[1], gate, out[0] / gate, out[1] / gate, sum(c[1] for c in chains[0]), sum(c[1] for c in chains[1])))
    assert out[0] <= gate and out[1] <= gate, (n, out, gate)


@pytest.mark.parametrize("model", list(HARSH))
def test_hom_sandwich_harsh_models(hip, golden, oracle, wide, model):
    """rho0 = 1e-6 and t_max = 60 at 200 states on the sandwich: right against the oracle, and never ECONVERGE; repair rounds may happen
    and are printed."""
    par = params(200, wide, model)
    segs = [hom_sandwich(golden.segs_mid[3])]
    want = reference(hip, oracle, ("hom sandwich", 200, model), 200, par, segs)
    r, d, es = run(hip, 200, segs, par, wide_hom_tiles=1, **SAND)    # (ECONVERGE would raise)
    again = es.wide_gap_rechained()
    es.close()
    print("HOMTEST harsh %s n 200 statistics: on %s rechained %s" % (model, work(d), again))
    check(r, want[0], want[1], want[2], ("hom sandwich", model, work(d)), (par[0], par[1]), segs)


# ------------------------------------------------------------------ (b) runs of both kinds, and levels
def both_kinds(T=64):
    """40 tiles of T bins, all symbol 0 but for hets at every fifth bin of tiles 0 .. 3 and 36 .. 39; tiles 10 .. 13 and 20 .. 23 missing:
    with both options tiles 4 .. 35 are ONE run -- hom, gap, hom, gap, hom -- that the chain crosses with two matrices in turn"""
    d = tiles_missing(None, 40, T, (10, 13), (20, 23))
    for b in list(range(4)) + list(range(36, 40)):
        d[b * T:(b + 1) * T:5] = 1
    return d


@pytest.mark.parametrize("n", [200, 300])
def test_chain_of_both_kinds(hip, golden, oracle, wide, n):
    """One run that alternates hom and gap tiles, warm-up 256 (tiles 0 .. 4 anchored forward, 35 .. 39 backward, so both chains start
    inside the run from an anchored tile's exact exit vector): one chain per direction, no repair round, every application within
    (2 n + 2) u of the product with the crossed tile's own matrix -- 8 across gap tiles and 23 across hom tiles in either direction --
    and the statistics pass every gate."""
    segs = [both_kinds()]
    par = params(n, wide)
    o = dict(chunk=64, warmup=256, wide_gap_tiles=1, wide_hom_tiles=1, wide_gap_min=128, wide_hom_min=128)
    want = reference(hip, oracle, ("both kinds", n), n, par, segs)
    r, d, es = run(hip, n, segs, par, **o)
    try:
        chains = es.wide_gap_chains()
        pt = es.wide_plan_tiles()
        M = es.wide_gap_matrix()
        Mh, fac = es.wide_hom_matrix()
        vec = [es.wide_tile_vectors(0), es.wide_tile_vectors(1)]
        again = es.wide_gap_rechained()
    finally:
        es.close()
    rule = dict(gap_min=128, hom_min=128, gap=True, hom=True)
    cls, glue = plan_rule(segs, 64, 256, **rule)
    assert list(cls[4:36]) == [4] * 6 + [2] * 4 + [4] * 6 + [2] * 4 + [4] * 12 and not cls[:4].any() and not cls[36:].any()
    assert np.array_equal(pt["cls"], cls) and np.array_equal(pt["glue"], glue)
    assert chains == list(chain_rule(segs, 64, 256, **rule)) == [[(5, 31, 36, 0)], [(34, 31, 3, 0)]], chains
    assert d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0 and again == [0, 0], (d, again)
    gate = (2 * n + 2) * U
    out = []
    for dr in (0, 1):
        worst, seen = chain_errors(n, M, Mh, par[1][0], cls, vec[dr], chains[dr], dr == 1)
        assert seen == [8, 23], seen
        out.append(worst)
    print("HOMTEST bothkinds n %d: worst cell per application forward %.2e backward %.2e bound %.2e -- shares %.3f / %.3f; %s" % (
        n, out[0], out[1], gate, out[0] / gate, out[1] / gate, work(d)))
    assert out[0] <= gate and out[1] <= gate, (n, out, gate)
    check(r, want[0], want[1], want[2], ("both kinds", n, work(d)), (par[0], par[1]), segs)


def test_levels_behind_a_mix_tile(hip, golden, oracle, wide):
    """hom_mixed at tiles of 100 bins and a warm-up of 400: the walk behind the 3000-bin run goes through the three tiles that hold both
    symbols, and the run that resumes behind them is chained one level later, in both directions; the plan is the numpy rule's, the
    result is right and reproducible (two fresh contexts, and from checkpoints)."""
    n = 200
    segs = hom_mixed(golden.segs_mid[3], golden.segs_mid[4])
    par = params(n, wide)
    want = reference(hip, oracle, ("hom mixed", n), n, par, segs)
    o = dict(chunk=100, warmup=400, wide_hom_tiles=1, wide_hom_min=1000)
    got = []
    for extra in (dict(), dict(), dict(wide_ckpt=1)):
        r, d, es = run(hip, n, segs, par, **o, **extra)
        got.append((r, d, es.wide_gap_chains(), es.wide_gap_rechained(), es.wide_plan_tiles()))
        es.close()
    (r1, d1, c1, a1, p1), (r2, d2, c2, a2, p2), (rc, dc, cc, ac, pc) = got
    cls, glue = plan_rule(segs, 100, 400, hom_min=1000)
    assert np.array_equal(p1["cls"], cls) and np.array_equal(p1["glue"], glue)
    assert c1 == list(chain_rule(segs, 100, 400, hom_min=1000)) and (48, 12, 60, 1) in c1[0] and (44, 30, 14, 1) in c1[1], c1
    print("HOMTEST levels n %d: forward %s backward %s; %s; rechained %s" % (n, c1[0], c1[1], work(d1), a1))
    check(r1, want[0], want[1], want[2], ("levels", work(d1)), (par[0], par[1]), segs)
    from test_gpu_wide_gap import same_bits
    assert same_bits(r1, r2) and d1 == d2 and a1 == a2
    assert same_bits(rc, r1) and ac == a1


# ------------------------------------------------------------------ (c) the benchmark genome's tile
def test_hommat_long_tile(hip, wide):
    """T = 7360, 200 states: six tiles of symbol 0, the inner four one run.  No entry of M_h is inf or NaN, every row's maximum divided
    by the pilot row's maximum (the pilot row: the mean of the rows, the uniform vector's image) is finite and > 0, no entry exceeds n
    times the pilot's, and the product of the 1840 factors -- what an unscaled matrix would have lost -- is printed."""
    n, T = 200, 7360
    par = params(n, wide)
    segs = [np.zeros(6 * T, np.uint8)]
    r, d, es = run(hip, n, segs, par, chunk=T, warmup=512, wide_hom_tiles=1)
    try:
        M, fac = es.wide_hom_matrix()
        cls = es.wide_plan_tiles()["cls"]
    finally:
        es.close()
    assert list(cls) == [0, 4, 4, 4, 4, 0]
    assert fac.shape == (T // 4,) and (np.frexp(fac)[0] == 0.5).all()
    assert np.isfinite(M).all() and (M >= 0).all() and not M[:, n:].any()
    pilot = M[:, :n].sum(0) / n
    ratio = M[:, :n].max(1) / pilot.max()
    print("HOMTEST longtile n %d T %d: row maximum / pilot maximum in [%.3g, %.3g]; pilot sum %.3g; product of the factors 2^%d; %s" % (
        n, T, float(ratio.min()), float(ratio.max()), float(pilot.sum()), int(np.log2(fac).sum()), work(d)))
    assert np.isfinite(ratio).all() and (ratio > 0).all()
    assert (M[:, :n] <= n * pilot[None, :] * (1 + 1e-9)).all()
    assert 2.0 ** -8 <= pilot.sum() <= 2.0
