"""The transfer-matrix chain of "wide_mix_tiles" looked at directly (psmc_amd/csrc/estep_wide_gap.hip k_wf_mixpilot / k_wf_mixmat /
k_wf_gapchain MIX), in the manner of tests/test_gpu_wide_hom_chain.py: tests/test_gpu_wide_mix.py judges the E-step's statistics, where a
wrong matrix or chain is invisible (k_wf_verify catches the vector and a repair walks the run).  Here, on mix_sandwich of
tests/wide_mix_model.py with all three options on -- ONE run of gap, hom and mix tiles --
  (a) the two matrices of the class-6 tiles from psmc_hip_wide_mix_matrix, their pilots' powers of two undone, against the long-double
      product of the T single steps (F = a D_lo ... a D_hi, B = D_lo a ... D_hi a),
  (b) every application of the chain (psmc_hip_wide_tile_vectors) against the long-double product of the DEVICE's matrix of the crossed
      tile and the DEVICE's previous vector,
  (c) one matrix pair of the benchmark genome's tile length, 7360 bins: finite, and no row lost against its pilot,
  (d) the two harsh models of tests/test_gpu_wide_gap_chain.py.
Lines that start with MIXTEST (shown with -s) are the figures profiles/wide_mix_tests.txt records.

Bounds, u = 2^-53, derived in tests/test_gpu_wide_hom_chain.py and not taken from what the kernels give.  (a) per row
max_j |M - Mref| / max_j Mref <= T (4 n + 1) u, and the same per cell on the cells of at least 1e-6 x the row's largest: every one of
the T steps is one sum of at most n non-negative products plus at most one emission rounding (none at a missing bin; the row's start
value e0_k of B is a float64 both sides start from).  (b) per cell (2 n + 2) u on the cells of at least 1e-6 x the vector's largest: no
division occurs across a mix tile, so the 2 n u of one sum of n non-negative products, the norm, its reciprocal and the product cover
it, and the larger bound of that file is asserted for all three kinds.

WHAT (a) COVERS.  A matrix exists where a chain crosses the tile in its direction: F of the tiles 9 .. 67 and B of the tiles 5 .. 64 here
(the others are anchored in that direction, and the diagnostic answers "invalid state" for them): 111 matrices of the 59 class-6 tiles.
Every one of them is checked at every size for: finite, non-negative, padded columns
exactly 0, ceil(T / 4) power-of-two factors, the bits of a second E-step, and -- through (b) -- consistency with the chain.  Against
long double, per row and per cell:
  149, 192, 193 states   EVERY row of EVERY matrix of EVERY class-6 tile (111 matrices);
  200 (harsh), 256, 257  every row of both matrices of three tiles -- the one with N first, the one with N last, and tile 15, which
                         starts and ends homozygous -- and of every other matrix the row (37 slot + 101 dir) mod n, which walks
                         over lanes, waves and the padding edge as the slot moves;
  1024                   the rows on the lane, wave and padding boundaries (boundary_rows) of B of the tile with N first and of F of
                         the tile with N last.
The reference of a whole matrix is PairRef of tests/wide_mix_model.py: the long-double product of the same T single-step matrices,
associated through the core that F and B share and the powers of a D between the missing bins (tests/test_wide_mix_model.py holds
it to the row-by-row stepping) -- about a dozen products of n x n matrices per tile, 14 ms each at 149 states and 74 ms at 257.  That
is what decides the split above: all tiles cost 12 s at 149 states, 27 s at 192 / 193 and would cost over a minute at 256 / 257 and
minutes at 1024, where single rows are stepped instead (mix_matrix_ref)."""
import hashlib
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal, GOLD
from test_gpu_wide_fast import check
from test_gpu_wide_gap import reference, run, work, level
from test_gpu_wide_gap_chain import params, width, boundary_rows, HARSH, U
from wide_gap_model import MISSING
from wide_mix_model import plan_rule, chain_rule, chain_errors, crossed, mix_matrix_ref, PairRef, mix_sandwich, tile_symbols, N_FIRST, N_LAST

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAND = dict(chunk=64, warmup=512)
ALL3 = dict(wide_gap_tiles=1, wide_hom_tiles=1, wide_mix_tiles=1)
RULE = dict(gap=True, hom=True)


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
    """the device's matrix with its pilot's powers of two undone, in long double (exact: the product of the factors is a power of two)"""
    return M.astype(np.longdouble) / np.prod(fac.astype(np.longdouble))


def digest(pair):
    return tuple(hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() for x in pair)


def rows_checked(n, tiles, built):
    """{(tile, dir): rows, or None for every row} -- what the long-double reference is formed for (the module's docstring)"""
    out = {}
    if n <= 257:
        full = tiles if n <= 193 else (N_FIRST, N_LAST, 15)
        for slot, t in enumerate(tiles):
            for dr in (0, 1):
                if (t, dr) in built:
                    out[(t, dr)] = None if t in full else [(37 * slot + 101 * dr) % n]
    else:
        out[(N_FIRST, 1)] = boundary_rows(n)
        out[(N_LAST, 0)] = boundary_rows(n)
    return out


CASES = [(n, "mild") for n in (149, 192, 193, 256, 257, 1024)] + [(n, m) for m in HARSH for n in (200, 1024)]


@pytest.mark.parametrize("n, model", CASES, ids=lambda v: str(v))
def test_mixmat_and_chain(hip, golden, wide, n, model):
    """mix_sandwich at tiles of 64 bins, warm-up 512, all three options: tiles 5 .. 67 are one run of 59 mix tiles, two hom tiles and two
    gap tiles.  (a) as the module's docstring says.  (b) on the mild models no repair round runs, so entry / bentry of the chained tiles
    are the chain's own vectors, and every one is the normalised product of the device's own matrix of the crossed tile and the
    device's previous vector within (2 n + 2) u per cell.  (On the harsh models repair rounds may run and rewrite vectors: there the
    matrices are judged, and the chain by the statistics of tests/test_gpu_wide_mix.py.)"""
    par = params(n, wide, model)
    T = 64
    segs = [mix_sandwich(golden.segs_mid[3])]
    cls_want, glue_want = plan_rule(segs, 64, 512, **RULE)
    tiles = [int(t) for t in np.flatnonzero(cls_want == 6)]
    assert len(tiles) == 59 and N_FIRST in tiles and N_LAST in tiles
    on_path = crossed(chain_rule(segs, 64, 512, **RULE))
    built = [(t, dr) for t in tiles for dr in (0, 1) if t in on_path[dr]]
    assert len(built) == 111 and all((t, dr) in built for t in (N_FIRST, N_LAST, 15) for dr in (0, 1))
    want_rows = rows_checked(n, tiles, built)
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), **ALL3, **SAND)
    es.load_segments(segs)
    S = width(n)
    nf = (T + 3) // 4
    try:
        es.estep_factored(par[0], par[1][:2], par[2])
        pt = es.wide_plan_tiles()
        assert np.array_equal(pt["cls"], cls_want) and np.array_equal(pt["glue"], glue_want)
        first = {k: es.wide_mix_matrix(*k) for k in built} if n <= 257 else None
        if first is None:   # (111 matrices of 8 MB: their bits as one SHA-256 digest each)
            first = {k: digest(es.wide_mix_matrix(*k)) for k in built}
        es.estep_factored(par[0], par[1][:2], par[2])
        d = es.fast_diag()
        chains = es.wide_gap_chains()
        vec = [es.wide_tile_vectors(0), es.wide_tile_vectors(1)]
        again = es.wide_gap_rechained()
        M_gap, (M_hom, _) = es.wide_gap_matrix(), es.wide_hom_matrix()
        worst = dict(row=0.0, cell=0.0, at=None, top=np.inf, lg=[], rows=0)
        pair = PairRef(par[0], par[1][0])
        bound = T * (4 * n + 1) * U
        e0 = par[1][0]
        for t in tiles:
            sym = tile_symbols(segs[0], T, t)
            whole = pair.pair(sym) if None in (want_rows.get((t, 0), 0), want_rows.get((t, 1), 0)) else None
            for dr in (0, 1):
                if (t, dr) not in built:   # anchored in this direction: no chain crosses it, no matrix
                    with pytest.raises(hip.HipError, match="no chain of the plan crosses"):
                        es.wide_mix_matrix(t, dr)
                    continue
                M, fac = es.wide_mix_matrix(t, dr)
                assert M.shape == (n, S) and np.isfinite(M).all() and (M >= 0).all() and not M[:, n:].any(), (t, dr)
                assert fac.shape == (nf,) and (np.frexp(fac)[0] == 0.5).all(), (t, dr)
                if n <= 257:
                    assert bits_equal(M, first[(t, dr)][0]) and bits_equal(fac, first[(t, dr)][1]), (t, dr)
                else:
                    assert digest((M, fac)) == first[(t, dr)], (t, dr)
                if (t, dr) not in want_rows:
                    continue
                rows = want_rows[(t, dr)]
                if rows is None:
                    rows, ref = list(range(n)), whole[dr]
                else:
                    ref = mix_matrix_ref(par[0], e0, sym, dr, rows)
                worst["rows"] += len(rows)
                got = unscaled(M, fac)[rows, :n]
                top = ref.max(1)
                dd = np.abs(got - ref)
                row_err = float((dd.max(1) / top).max())
                big = ref >= 1e-6 * top[:, None]
                cell_err = float(np.where(big, dd / np.where(big, ref, 1), 0).max())
                if cell_err > worst["cell"]:
                    worst["at"] = (t, dr)
                worst["row"], worst["cell"], worst["top"] = max(worst["row"], row_err), max(worst["cell"], cell_err), min(worst["top"], float(top.min()))
                worst["lg"].append(int(np.log2(fac).sum()))
                assert row_err <= bound, (n, model, t, dr, row_err, bound)
                assert cell_err <= bound, (n, model, t, dr, cell_err, bound)
        print("MIXTEST mixmat n %d T %d %s: %d matrices, %d rows against long double: worst row %.2e worst cell %.2e (tile %s) bound %.2e -- shares %.3f / %.3f; products of the factors 2^%d .. 2^%d; smallest row maximum %.1e" % (
            n, T, model, len(want_rows), worst["rows"], worst["row"], worst["cell"], worst["at"], bound,
            worst["row"] / bound, worst["cell"] / bound, min(worst["lg"]), max(worst["lg"]), worst["top"]))
        with pytest.raises(hip.HipError, match="(?i)invalid"):
            es.wide_mix_matrix(20, 0)    # a hom tile
        with pytest.raises(hip.HipError, match="(?i)invalid"):
            es.wide_mix_matrix(15, 2)
        assert chains == list(chain_rule(segs, 64, 512, **RULE)), chains
        if model != "mild":
            print("MIXTEST harsh %s n %d: %s rechained %s" % (model, n, work(d), again))
            return
        assert d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0 and again == [0, 0], (d, again)
        gate = (2 * n + 2) * U
        out, kinds = [], []
        for dr in (0, 1):
            w, seen = chain_errors(n, M_gap, M_hom, lambda t: es.wide_mix_matrix(t, dr)[0], e0, cls_want, vec[dr], chains[dr], dr == 1)
            assert sum(seen) == sum(c[1] for c in chains[dr]) and seen[0] == 2 and seen[1] == 2 and seen[2] >= 55, seen
            out.append(w); kinds.append(seen)
        print("MIXTEST mixchain n %d: worst cell per application forward %.2e backward %.2e bound %.2e -- shares %.3f / %.3f (gap, hom, mix applications: %s forward, %s backward)" % (
            n, out[0], out[1], gate, out[0] / gate, out[1] / gate, kinds[0], kinds[1]))
        assert out[0] <= gate and out[1] <= gate, (n, out, gate)
    finally:
        es.close()


# ------------------------------------------------------------------ (c) the benchmark genome's tile
def test_mixmat_long_tile(hip, wide):
    """T = 7360, 200 states: six tiles of symbol 0 with three short stretches of N each, as the simulated genome carries them; the inner
    four are one run of mix tiles.  Tile 1 starts with N, so D_lo = I and the mean of the rows of EITHER of its matrices is its pilot's
    own vector.  Both matrices: no entry inf or NaN, every row's maximum divided by the pilot's maximum finite and > 0 (no row lost), no
    entry above n times the pilot's, the pilot's sum within [2^-8, 2]; the products of the 1840 factors are printed."""
    n, T = 200, 7360
    par = params(n, wide)
    rng = np.random.default_rng(5)
    s = np.zeros(6 * T, np.uint8)
    for b in range(6):
        for at in rng.integers(1, T - 41, 3):
            s[b * T + at:b * T + at + int(rng.integers(5, 40))] = MISSING
    s[T] = MISSING
    r, d, es = run(hip, n, [s], par, chunk=T, warmup=512, wide_hom_tiles=1, wide_mix_tiles=1)
    try:
        cls = es.wide_plan_tiles()["cls"]
        assert list(cls) == [0, 6, 6, 6, 6, 0]
        for dr in (0, 1):
            M, fac = es.wide_mix_matrix(1, dr)
            assert fac.shape == (T // 4,) and (np.frexp(fac)[0] == 0.5).all()
            assert np.isfinite(M).all() and (M >= 0).all() and not M[:, n:].any()
            pilot = M[:, :n].sum(0) / n
            ratio = M[:, :n].max(1) / pilot.max()
            print("MIXTEST longtile n %d T %d dir %d: row maximum / pilot maximum in [%.3g, %.3g]; pilot sum %.3g; product of the factors 2^%d; %s" % (
                n, T, dr, float(ratio.min()), float(ratio.max()), float(pilot.sum()), int(np.log2(fac).sum()), work(d)))
            assert np.isfinite(ratio).all() and (ratio > 0).all()
            assert (M[:, :n] <= n * pilot[None, :] * (1 + 1e-9)).all()
            assert 2.0 ** -8 <= pilot.sum() <= 2.0
    finally:
        es.close()


# ------------------------------------------------------------------ (d) harsh models: the statistics
@pytest.mark.parametrize("model", list(HARSH))
def test_mix_sandwich_harsh_models(hip, golden, oracle, wide, model):
    """rho0 = 1e-6 and t_max = 60 at 200 states on the sandwich: right against the oracle, and never ECONVERGE; repair rounds may happen
    and are printed."""
    par = params(200, wide, model)
    segs = [mix_sandwich(golden.segs_mid[3])]
    want = reference(hip, oracle, ("mix sandwich", 200, model), 200, par, segs)
    r, d, es = run(hip, 200, segs, par, **ALL3, **SAND)    # (ECONVERGE would raise)
    again = es.wide_gap_rechained()
    es.close()
    print("MIXTEST harsh %s n 200 statistics: on %s rechained %s" % (model, work(d), again))
    check(r, want[0], want[1], want[2], ("mix sandwich", model, work(d)), (par[0], par[1]), segs)
