"""The transfer-matrix chain of "wide_gap_tiles" looked at directly (psmc_amd/csrc/estep_wide_gap.hip k_wf_gapmat / k_wf_gapchain,
api_wide_fast.hip plan_wide_gaps and the re-chaining repair of wide_rounds).  tests/test_gpu_wide_gap.py judges the E-step's
statistics only, and a wrong matrix or chain is invisible there: k_wf_verify catches the vector and a repair walks the run.  Here
  (a) the matrix is compared with the long-double power of a (tests/wide_gap_model.py matrix_ref / matrix_rows_ref),
  (b) every application of the chain with the long-double product of the DEVICE's matrix and the DEVICE's previous vector,
  (c) the planner's chains with chain_rule, on inputs that reach every branch (levels beyond 0, a chain of count 0, a chain that
      starts inside its run, a run that is skipped, walks on a segment's first and last tile),
  (d) inputs whose chains start from exact vectors need no repair round at the sizes on and just past every padded width,
  (e) inputs whose chains start from failing tiles are chained again, reproducibly,
  (f) the counts pass and the batch over plans with more than one level,
through the diagnostics psmc_hip_wide_gap_chains / _rechained / _matrix and psmc_hip_wide_tile_vectors (include/psmc_hip_diag.h).
Lines that start with GAPTEST (shown with -s) are the figures profiles/wide_gap_tests.txt records.

Bounds, u = 2^-53.  (a) per row max_j |M - Mref| / max_j Mref <= 4 T n u, and the same per cell on the cells of at least 1e-6 x the
row's largest (the project's cell rule): each of the T steps forms an entry from at most n non-negative products and a fixed number
of scan levels; the plain float64 restatement measures 1.2e-14 at n = 200, T = 64 against 5.7e-12 (tests/test_wide_gap_model.py).
(b) per cell 2 n u on the cells of at least 1e-6 x the vector's largest: one sum of n non-negative products, one sum of n terms for
the norm, one reciprocal, one product.  Neither bound was taken from what the kernels give.

The clause "entry[first] is the neighbour's exit row bit for bit" has no reader of its own: no entry point returns a row of the wide
path's X table.  It is held by the bits tests of (e) (a fresh context and "wide_ckpt" -- the other source of that row -- agree)."""
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal, GOLD
from test_gpu_wide_fast import check, tri_sums, psmc_params
from test_gpu_wide_gap import reference, run, same_bits, work, level
from wide_gap_model import plan_rule, chain_rule, chain_errors, matrix_ref, matrix_rows_ref, twin, triple, head_run, tail_run, tiles_missing

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
HARSH = {"rho_1e-6": [0.02, 1e-6, 15.0], "tmax_60": [0.02, 0.004, 60.0]}   # tests/test_gpu_wide_fast_edges.py MODELS / test_gpu_wide_fast_mw.py
TWIN = dict(chunk=64, warmup=512)


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module")
def wide():
    return dict(np.load(os.path.join(GOLD, "estep_wide.npz")))


_PAR = {}


def params(n, wide, model="mild"):
    """the size tables of the wide tests: the goldens at 149 / 200 states, SIZES of tests/test_gpu_wide_fast_edges.py up to 256 and of
    tests/test_gpu_wide_fast_mw.py beyond; the two harsh models as those files build them"""
    if (n, model) not in _PAR:
        if model != "mild":
            from psmc_amd import hostlib
            pat, m = {200: ("100*2", 100), 1024: ("128*8", 128)}[n]
            p = hostlib.hmm_params(pat, HARSH[model] + [1.0] * m)
        elif n in (149, 200):
            p = (wide["n%d.a" % n], wide["n%d.e" % n], wide["n%d.a0" % n])
        elif n <= 256:
            from test_gpu_wide_fast_edges import mild_model
            p = mild_model(n)
        else:
            from test_gpu_wide_fast_mw import params as mw
            p = mw(n)
        _PAR[(n, model)] = p
    return _PAR[(n, model)]


def width(n):
    return 64 * ((n + 63) // 64) if n <= 256 else 256 * ((n + 255) // 256)


def boundary_rows(n):
    """lane, wave and padding boundaries of the layout (four states per lane, 256 per wave)"""
    return sorted({r for r in (0, 1, 255, 256, 257, 511, 512, 767, 768, n - 2, n - 1) if r < n})


# ------------------------------------------------------------------ (a) k_wf_gapmat
GAPMAT = [(n, T, "mild") for n in (129, 149, 192, 193, 200, 256, 257, 300) for T in (7, 64)] + [(n, 64, "mild") for n in (513, 769, 1024)] + \
         [(n, 64, m) for m in HARSH for n in (200, 1024)]


@pytest.mark.parametrize("n, T, model", GAPMAT, ids=lambda v: str(v))
def test_gapmat_against_long_double(hip, golden, wide, n, T, model):
    """The device's matrix of one full tile of T missing bins against a to the power T in long double: the whole matrix up to 300
    states, beyond them the rows on the lane, wave and padding boundaries.  Per row and per cell within 4 T n u; the padded columns are
    exactly 0; every row sums to 1 within T n u; a second E-step builds the same bits."""
    par = params(n, wide, model)
    segs = [twin(golden.segs_mid[3])]
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), wide_gap_tiles=1, chunk=T, warmup=512)
    es.load_segments(segs)
    try:
        es.estep_factored(par[0], par[1][:2], par[2])
        M = es.wide_gap_matrix()
        es.estep_factored(par[0], par[1][:2], par[2])
        M2 = es.wide_gap_matrix()
    finally:
        es.close()
    S = width(n)
    assert M.shape == (n, S) and np.isfinite(M).all()
    assert bits_equal(M, M2)
    assert not M[:, n:].any()
    rows = list(range(n)) if n <= 300 else boundary_rows(n)
    ref = matrix_ref(par[0], T) if n <= 300 else matrix_rows_ref(par[0], T, rows)
    got = M[rows, :n].astype(np.longdouble)
    bound = 4 * T * n * U
    top = ref.max(1)
    d = np.abs(got - ref)
    row_err = d.max(1) / top
    big = ref >= 1e-6 * top[:, None]
    cell_err = np.where(big, d / np.where(big, ref, 1), 0).max(1)
    sum_err = np.abs(M[:, :n].astype(np.longdouble).sum(1) - 1)
    print("GAPTEST gapmat n %d T %d %s: worst row %.2e (row %d) worst cell %.2e (row %d) bound %.2e; row sums off 1 by %.2e (bound %.2e); smallest row maximum %.1e" % (
        n, T, model, float(row_err.max()), rows[int(row_err.argmax())], float(cell_err.max()), rows[int(cell_err.argmax())], bound,
        float(sum_err.max()), T * n * U, float(top.min())))
    assert (M[:, :n] >= 0).all()
    assert float(row_err.max()) <= bound, (n, T, model, float(row_err.max()), bound)
    assert float(cell_err.max()) <= bound, (n, T, model, float(cell_err.max()), bound)
    assert float(sum_err.max()) <= T * n * U, (n, T, model, float(sum_err.max()))


# ------------------------------------------------------------------ (b) k_wf_gapchain
@pytest.mark.parametrize("chunk", [64, 37])
@pytest.mark.parametrize("n", [129, 149, 192, 193, 200, 256, 257, 300, 513, 1024])
def test_gapchain_one_application(hip, golden, wide, n, chunk):
    """twin, warm-up 512: both directions need no repair round, so entry / bentry of the chained tiles are the chain's own vectors.
    Every one of them is the normalised product of the device's matrix and the vector before it, per cell within 2 n u; the padded
    states are exactly 0.  At 200 states and tiles of 64 bins the same from checkpoints ("wide_ckpt": the chain starts from xhi)."""
    par = params(n, wide)
    segs = [twin(golden.segs_mid[3])]
    for extra in [dict()] + ([dict(wide_ckpt=1)] if (n, chunk) == (200, 64) else []):
        r, d, es = run(hip, n, segs, par, wide_gap_tiles=1, chunk=chunk, warmup=512, **extra)
        try:
            chains = es.wide_gap_chains()
            M = es.wide_gap_matrix()
            vec = [es.wide_tile_vectors(0), es.wide_tile_vectors(1)]
            again = es.wide_gap_rechained()
            iv = es.wide_table_info()["interval"]
        finally:
            es.close()
        assert iv == (8 if extra else 1)
        assert chains == list(chain_rule(segs, chunk, 512)), chains
        assert d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0 and again == [0, 0], (d, again)
        assert vec[0].shape == (d["n_chunks"], width(n)) and vec[1].shape == vec[0].shape
        bound = 2 * n * U
        out = []
        for dr in (0, 1):
            worst, seen = chain_errors(n, M, vec[dr], chains[dr], dr == 1)
            assert seen == sum(c[1] for c in chains[dr]) > 0
            out.append(worst)
        print("GAPTEST gapchain n %d chunk %d%s: worst cell per application forward %.2e backward %.2e bound %.2e (%d + %d applications)" % (
            n, chunk, " wide_ckpt" if extra else "", out[0], out[1], bound, sum(c[1] for c in chains[0]), sum(c[1] for c in chains[1])))
        assert out[0] <= bound and out[1] <= bound, (n, chunk, out, bound)


# ------------------------------------------------------------------ (c) the planner's branches
def plan_cases(golden):
    """name -> (segments, options, what the input is for)"""
    src = golden.segs_mid[3]
    b60 = dict(chunk=64, warmup=256, wide_gap_min=128)
    c = {"twin-%d" % T: ([twin(src)], dict(chunk=T, warmup=512), {"level": 1}) for T in (64, 37, 8)}
    c["triple"] = ([triple(src)], b60, {"level": 2, "rechain": 1})
    c["head_run"] = ([head_run(src)], dict(chunk=64, warmup=512, wide_gap_min=128), {"count0": 1, "inside": 1})
    c["tail_run"] = ([tail_run(src)], dict(chunk=64, warmup=512, wide_gap_min=128), {"count0": 1, "inside": 1})
    c["tiles-3-8"] = ([tiles_missing(None, 60, 64, (3, 8))], b60, {"inside": 1})
    c["tiles-2-4"] = ([tiles_missing(None, 60, 64, (2, 4))], b60, {"count0": 1})
    c["tiles-55-57"] = ([tiles_missing(None, 60, 64, (55, 57))], b60, {"count0": 1})
    # (a segment of missing data only has LL = log 1: the gates' relative LL bound means nothing against a reference of 6.7e-16, so a
    # segment of called bins follows it -- 960 bins, no chain -- as the multisets of tests/test_gpu_wide_fast_edges.py do)
    c["all-missing"] = ([tiles_missing(None, 40, 64, (0, 39)), tiles_missing(golden.segs_small[8], 15, 64)], b60, {"ends": 1, "inside": 1})
    # the first segment's run is anchored through to the segment's end both ways (five tiles, warm-up 256): no chain there
    c["skipped+triple"] = ([tiles_missing(src, 5, 64, (1, 3)), triple(src)], b60, {"level": 2, "skipped": 1, "rechain": 1})
    return c


PLAN_CASES = ["twin-64", "twin-37", "twin-8", "triple", "head_run", "tail_run", "tiles-3-8", "tiles-2-4", "tiles-55-57", "all-missing", "skipped+triple"]


@pytest.mark.parametrize("name", PLAN_CASES)
@pytest.mark.parametrize("n", [200, 300])
def test_planner_branches(hip, golden, oracle, wide, n, name):
    """Classes, glue bits and chains of the device's plan are the numpy rule's, the input reaches the branch it was made for, and the
    statistics pass every gate against the oracle (200 states) or the exact kernels (300)."""
    segs, opts, purpose = plan_cases(golden)[name]
    par = params(n, wide)
    want = reference(hip, oracle, ("plan", name, n), n, par, segs)
    r, d, es = run(hip, n, segs, par, wide_gap_tiles=1, **opts)
    try:
        pt = es.wide_plan_tiles()
        chains = es.wide_gap_chains()
        again = es.wide_gap_rechained()
    finally:
        es.close()
    T, W, gm = opts["chunk"], opts["warmup"], opts.get("wide_gap_min", 0)
    cls, glue = plan_rule(segs, T, W, gm)
    assert np.array_equal(pt["cls"], cls) and np.array_equal(pt["glue"], glue), (pt, cls, glue)
    rule = chain_rule(segs, T, W, gm)
    assert chains == list(rule), (chains, rule)
    nts = [(len(s) + T - 1) // T for s in segs]
    seg_first = np.concatenate([[0], np.cumsum(nts)])[:-1]
    ends = set(int(x) for x in seg_first) | set(int(x + k - 1) for x, k in zip(seg_first, nts))
    both = chains[0] + chains[1]
    has = {"level": max(c[3] for c in both),
           "count0": int(any(c[1] == 0 for c in both)),
           "inside": int(any(cls[c[0]] == 2 and cls[c[0] - st] == 2 for dr, st in ((0, 1), (1, -1)) for c in chains[dr])),
           "ends": int(any(c[2] in ends for c in chains[0]) and any(c[2] in ends for c in chains[1])),
           "skipped": int((cls[:nts[0]] == 2).any() and not any(c[0] < nts[0] for c in both)),
           "rechain": min(again)}   # (the data tile in front of the first run speculates and fails: chains of levels 0 .. 2 run again)
    for k, v in purpose.items():
        assert has[k] >= v, (name, k, has, chains)
    print("GAPTEST plan %s n %d: forward %s backward %s; %s; rechained %s" % (name, n, chains[0], chains[1], work(d), again))
    check(r, want[0], want[1], want[2], ("plan", name, n, work(d)), (par[0], par[1]), segs)


# ------------------------------------------------------------------ (d) exact inputs need no repair
# compare of tests/test_gpu_wide_fast_decode.py caps the near-ties of the exact posterior (two largest entries within 2e-9) at 0.1 % of
# the positions, counted from the exact context alone.  On twin at 1024 states that cap cannot hold whatever the fast path does: 2048
# of the 2776 bins are missing data, where the posterior over a dense grid of states (largest entry 0.0065) drifts by about 1e-9 per
# bin, and the exact kernels alone have 3 such bins (1239, 2585, 2771) against a cap of 2.776; none at the other sizes.  There the
# cap is replaced by compare's tie_rule: at every near-tie the fast path is one of the exact posterior's two largest states.
TIES_BEYOND_THE_CAP = (1024,)


def exact_ctx(hip, n, par, segs):
    ex = hip.HipEStep(n, mode=hip.MODE_EXACT)
    ex.load_segments(segs)
    o = ex.estep(*par)
    return ex, (tri_sums(o["A"]), o["E"], o["LL"], o["A"])


@pytest.mark.parametrize("n", [129, 192, 193, 200, 256, 257, 300, 513, 769, 1024])
def test_twin_needs_no_repair(hip, golden, oracle, wide, n):
    """twin at tiles of 64 bins and a warm-up of 512 leaves no unanchored tile speculating: with an accurate chain no boundary fails in
    either direction, nothing is chained again, the statistics pass every gate and so do posterior, path and scales of every bin
    (compare of tests/test_gpu_wide_fast_decode.py; at 1024 states with its tie_rule: TIES_BEYOND_THE_CAP) -- from the full table and
    from checkpoints.  Without the option the same input needs repair rounds (printed)."""
    from test_gpu_wide_fast_decode import compare
    par = params(n, wide)
    segs = [twin(golden.segs_mid[3])]
    ex, xref = exact_ctx(hip, n, par, segs)
    try:
        want = reference(hip, oracle, ("twin", n), n, par, segs) if n <= 200 else xref
        rounds = []
        for extra in (dict(), dict(wide_ckpt=1, wide_decode_ckpt=1)):
            r, d, es = run(hip, n, segs, par, wide_gap_tiles=1, wide_decode=1, **TWIN, **extra)
            try:
                again = es.wide_gap_rechained()
                assert es.wide_table_info()["interval"] == (8 if extra else 1)
                assert d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0 and again == [0, 0], (n, extra, d, again)
                check(r, want[0], want[1], want[2], ("twin", n, extra, work(d)), (par[0], par[1]), segs)
                w = compare(es, ex, segs, n, tie_rule=n in TIES_BEYOND_THE_CAP, E=r["E"])
            finally:
                es.close()
            rounds.append((d["fwd_rounds"], d["bwd_rounds"]))
    finally:
        ex.close()
    r0, d0, e0 = run(hip, n, segs, par, **TWIN)
    e0.close()
    print("GAPTEST norepair n %d: rounds on %s (checkpoints %s) rechained %s, near-ties of the exact posterior %d; off: %s" % (n, rounds[0], rounds[1], again, w.get("near_ties", 0), work(d0)))
    check(r0, want[0], want[1], want[2], ("twin, option off", n), (par[0], par[1]), segs)


@pytest.mark.parametrize("model", list(HARSH))
def test_twin_harsh_models(hip, golden, oracle, wide, model):
    """rho0 = 1e-6 (a matrix close to the identity: the chain barely forgets) and t_max = 60 (entries far down the double range) at 200
    states: right against the oracle, and never ECONVERGE; repair rounds may happen and are printed."""
    par = params(200, wide, model)
    segs = [twin(golden.segs_mid[3])]
    want = reference(hip, oracle, ("twin", 200, model), 200, par, segs)
    r, d, es = run(hip, 200, segs, par, wide_gap_tiles=1, **TWIN)    # (ECONVERGE would raise)
    again = es.wide_gap_rechained()
    es.close()
    r0, d0, e0 = run(hip, 200, segs, par, **TWIN)
    e0.close()
    print("GAPTEST harsh %s n 200: on %s rechained %s; off %s" % (model, work(d), again, work(d0)))
    check(r, want[0], want[1], want[2], ("twin", model, work(d)), (par[0], par[1]), segs)


# ------------------------------------------------------------------ (e) re-chaining
@pytest.mark.parametrize("learn", [1, 0])
@pytest.mark.parametrize("name", ["twin", "triple", "triple-w256"])
@pytest.mark.parametrize("n", [200, 300])
def test_rechain(hip, golden, oracle, n, name, learn):
    """Without a warm-up every unanchored data tile starts cold: the tile in front of each run fails, the run's first chained tile heads a
    failing run and the run is chained again.  That happens in both directions, the result is right, never ECONVERGE, the same bits
    (statistics, fast_diag, re-chain counts) from two fresh contexts and from checkpoints, and the third E-step of a context whose
    parameters move is a fresh context's first with the final ones.  Without a warm-up nothing but the runs is glued and every chain
    is level 0; triple-w256 is triple at a warm-up of 256 bins, where the chains are levels 0, 1, 2 and the data tile in front of the
    first run still fails: the same assertions with levels and re-chaining in play together."""
    src = golden.segs_mid[3]
    segs = [twin(src)] if name == "twin" else [triple(src)]
    W = 256 if name == "triple-w256" else 0
    rng = np.random.default_rng(23)
    pat = {200: ("100*2", 100), 300: ("150*2", 150)}[n]
    pars = [psmc_params(pat[0], pat[1], rng) for _ in range(3)]
    par = pars[2]
    want = reference(hip, oracle, ("rechain", name.split("-")[0], n), n, par, segs)
    o = dict(chunk=64, warmup=W, wide_gap_min=128, learn=learn, wide_gap_tiles=1)
    got = []
    for extra in (dict(), dict(), dict(wide_ckpt=1)):
        r, d, es = run(hip, n, segs, par, **o, **extra)
        got.append((r, d, es.wide_gap_rechained(), es.wide_gap_chains()))
        assert es.wide_table_info()["interval"] == (8 if extra else 1)
        es.close()
    (r1, d1, a1, c1), (r2, d2, a2, c2), (rc, dc, ac, cc) = got
    print("GAPTEST rechain %s n %d learn %d: rechained %s, %s; chains %d + %d, levels to %d" % (name, n, learn, a1, work(d1), len(c1[0]), len(c1[1]), max(c[3] for c in c1[0])))
    assert c1 == list(chain_rule(segs, 64, W, 128)) and len(c1[0]) >= 2 and len(c1[1]) >= 2
    assert [max(c[3] for c in d) for d in c1] == ([2, 2] if W else [0, 0])
    assert a1[0] >= 1 and a1[1] >= 1, (a1, d1)
    check(r1, want[0], want[1], want[2], ("rechain", name, n, learn, work(d1)), (par[0], par[1]), segs)
    assert same_bits(r1, r2) and d1 == d2 and a1 == a2
    assert same_bits(rc, r1) and ac == a1 and (dc["fwd_rounds"], dc["bwd_rounds"], dc["fwd_tiles"], dc["bwd_tiles"]) == (d1["fwd_rounds"], d1["bwd_rounds"], d1["fwd_tiles"], d1["bwd_tiles"])
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), **o)
    es.load_segments(segs)
    for a, e, a0 in pars:
        r3 = es.estep_factored(a, e[:2], a0)
    a3 = es.wide_gap_rechained()
    es.close()
    assert same_bits(r3, r1) and a3 == a1, ("third E-step", a3, a1)


# ------------------------------------------------------------------ (f) counts and batch over levels
@pytest.mark.parametrize("n", [200, 513])
def test_counts_over_levels(hip, golden, oracle, wide, n):
    """ "wide_counts" on twin (two levels per direction): the full count matrix under the gates of tests/test_gpu_wide_counts.py, and the
    same bits from checkpoints ("wide_counts_ckpt")."""
    from test_gpu_wide_counts import gate
    par = params(n, wide)
    segs = [twin(golden.segs_mid[3])]
    want = reference(hip, oracle, ("twin", n), n, par, segs)
    got = []
    for extra in (dict(), dict(wide_ckpt=1, wide_counts_ckpt=1)):
        es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), wide_counts=1, wide_gap_tiles=1, **TWIN, **extra)
        es.load_segments(segs)
        r = es.estep(*par)
        d = es.fast_diag()
        chains = es.wide_gap_chains()
        assert es.wide_table_info()["interval"] == (8 if extra else 1)
        es.close()
        assert max(c[3] for c in chains[0]) == 1 and max(c[3] for c in chains[1]) == 1
        assert d["back_half"] == 4 and d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0, d
        gate(r, dict(A=want[3], E=want[1], LL=want[2]), (par[0], par[1]), ("twin counts", n, extra))
        got.append(r)
    assert bits_equal(got[0]["A"], got[1]["A"]) and bits_equal(got[0]["E"], got[1]["E"]) and got[0]["LL"] == got[1]["LL"]


@pytest.mark.parametrize("n", [200, 300])
def test_batch_over_levels(hip, golden, wide, n):
    """ "wide_batch": two multisets over twin, triple and a segment of data only, one repeating a gapped segment, equal two single E-steps
    bit for bit; the plans hold chains of levels 0, 1 and 2."""
    src = golden.segs_mid[3]
    segs = [twin(src), triple(src), golden.segs_small[7]]
    par = params(n, wide)
    sels = [[0, 0, 2], [1, 2, 0]]
    opts = dict(wide_gap_tiles=1, chunk=64, warmup=256, wide_gap_min=128)
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), wide_batch=1, **opts)
    es.load_segments(segs)
    b = es.estep_batch([par, par], sels, want="sums")
    es.close()
    for i, sel in enumerate(sels):
        one = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), **opts)
        one.load_segments(segs)
        one.select(sel)
        r = one.estep_factored(par[0], par[1][:2], par[2])
        chains = one.wide_gap_chains()
        one.close()
        assert chains == list(chain_rule([segs[j] for j in dict.fromkeys(sel)], 64, 256, 128)), (sel, chains)   # (the plan: first appearance)
        assert max(c[3] for c in chains[0]) == (1 if i == 0 else 2)
        assert bits_equal(b["sums"][i], r["sums"]) and bits_equal(b["E"][i], r["E"]) and b["LL"][i] == r["LL"], (n, i)
