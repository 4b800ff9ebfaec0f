"""The full count matrix from the wide fast path: psmc_hip_estep of a fast-mode context with "wide_fast" + "wide_counts" = 1 at
129 .. 1024 states (psmc_amd/csrc/estep_wide_counts.hip: per slab of whole tiles one more backward sweep that writes V_p =
mult bt_{p+1} / G_p, then C += X^T V on the f64 matrix cores, split-K with one owner per partial; A = a . C).  References: the
reference's goldens at 200 and 149 states, the CPU oracle, and the exact kernels on the same device -- never the code under
test.  Gates: fast mode's own (tests/test_gpu_estep.py): A and E 1e-10 of the largest cell, LL 1e-12 relative, cells >= 1e-6 of
the largest 1e-9, L1 1e-10, the two sums of hmm_Q 1e-10.  Every test asserts fast_info's back half 4 ("full counts of the wide
path"): a silent fall-back to the exact kernels would pass every gate bit for bit.

Observed on the MI355X (-s prints every comparison):
  against the goldens, the oracle and the exact kernels, every size, tiling and slab size (168 comparisons):
    A_cell <= 1.2e-13, E_cell <= 1.1e-13 (the anchored tiles at 200 states), A_max / E_max <= 7.1e-14, A_l1 <= 1.7e-14,
    QA / QE <= 1.7e-14 (the multiset against the oracle), LL <= 2.6e-14 relative
  tri_sums(A) against the factored sums of the same context (gate FAST_TOL_STATS = 1e-10 of the largest cell):
    <= 7.0e-16 with the default tiling at every size, <= 3.4e-15 with tiles of 64 bins and one tile per slab (1024 states)
"""
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal
from test_gpu_estep import FAST_TOL_STATS, FAST_TOL_CELL, FAST_TOL_L1, FAST_TOL_Q, FAST_TOL_LL
from test_gpu_wide_fast import TILINGS, tri_sums, relmax, psmc_params
from test_gpu_wide_fast_mw import SIZES as MW_SIZES, params as mw_params, short_segs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_WAVE = {129: ("129*1", 129), 192: ("192*1", 192), 193: ("193*1", 193), 256: ("128*2", 128)}
MULTI_WAVE = [257, 300, 512, 513, 768, 769, 1024]
WORST = {}


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module")
def wide():
    from conftest import GOLD
    return dict(np.load(os.path.join(GOLD, "estep_wide.npz")))


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for k in sorted(WORST):
        print("worst %-8s %.3e  %s" % (k, WORST[k][0], WORST[k][1]))


def level(n):
    return 1 if n <= 256 else 2


def params(n):
    if n in ONE_WAVE:
        return psmc_params(ONE_WAVE[n][0], ONE_WAVE[n][1], np.random.default_rng(3000 + n))
    return mw_params(n)


def par_of(n):
    """200 states: the host model of "100*2"; 300: tests/test_gpu_wide_fast_mw.py params"""
    return psmc_params("100*2", 100, np.random.default_rng(5)) if n == 200 else mw_params(n)


def ctx(hip, n, segs, wide_counts=1, **opts):
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=opts.pop("wide_fast", level(n)), wide_counts=wide_counts, **opts)
    es.load_segments(segs)
    return es


def back_half(es):
    """fast_info's back half of the last fast E-step; None when the context has run no fast E-step at all"""
    try:
        return es.fast_diag()["back_half"]
    except Exception:
        return None


def ran_counts(es):
    d = es.fast_diag()
    assert d["back_half"] == 4 and d["recounted"] == 2 and d["n_chunks"] > 0, d
    return d


def gate(r, o, par, what):
    """r against its reference o (A, E, LL) through the gates of tests/test_gpu_estep.py check_fast"""
    from psmc_amd.parity import fast_error_metrics
    m = fast_error_metrics(r, o, par[0], par[1])
    for k, v in m.items():
        if not v <= WORST.get(k, (-1.0, None))[0]:
            WORST[k] = (v, what)
    print("wide counts vs reference", what, "  ".join("%s %.2e" % (k, m[k]) for k in sorted(m)))
    assert np.isfinite(r["A"]).all(), what
    assert relmax(r["A"], o["A"]) < FAST_TOL_STATS, (what, m)
    assert relmax(r["E"], o["E"][:2]) < FAST_TOL_STATS, (what, m)
    assert abs(r["LL"] - o["LL"]) <= FAST_TOL_LL * abs(o["LL"]), (what, r["LL"], o["LL"])
    assert m["A_cell"] <= FAST_TOL_CELL and m["E_cell"] <= FAST_TOL_CELL, (what, m)
    assert m["A_l1"] <= FAST_TOL_L1, (what, m)
    assert m["QA"] <= FAST_TOL_Q and m["QE"] <= FAST_TOL_Q, (what, m)
    assert not r["A0"].any() and (r["chk"] == 1.0).all(), what   # as every fast-mode E-step
    return m


def transitions_ok(r, segs, what):
    trans = float(sum(len(s) - 1 for s in segs))
    assert np.isfinite(r["A"]).all() and abs(r["A"].sum() - trans) <= 1e-9 * max(trans, 1.0), (what, r["A"].sum(), trans)


def same_bits(r, w):
    return bits_equal(r["A"], w["A"]) and bits_equal(r["E"], w["E"]) and r["LL"] == w["LL"]


_EXACT = {}


def exact(hip, key, n, par, segs, sel=None):
    """the exact kernels' A, E, LL on the same device, computed once per key"""
    if key not in _EXACT:
        ex = hip.HipEStep(n, mode=hip.MODE_EXACT)
        ex.load_segments(segs)
        if sel is not None:
            ex.select(sel)
        _EXACT[key] = ex.estep(*par)
        ex.close()
    return _EXACT[key]


# ------------------------------------------------------------------ the reference's goldens
@pytest.mark.parametrize("slab", [0, 64, 300])
@pytest.mark.parametrize("opts", TILINGS)
@pytest.mark.parametrize("key", ["n200", "n149"])
def test_wide_counts_golden(hip, golden, wide, key, opts, slab):
    """estep_wide.npz on segs_small[:8]: A, E and LL of the reference, in every tiling of tests/test_gpu_wide_fast.py and with
    one tile per slab (64), several tiles per slab (300) and everything in one slab (auto); three calls, the same bits."""
    a, e, a0 = wide[key + ".a"], wide[key + ".e"], wide[key + ".a0"]
    segs = golden.segs_small[:8]
    o = dict(A=wide[key + ".A"], E=wide[key + ".E"], LL=float(wide[key + ".LL"]))
    es = ctx(hip, a.shape[0], segs, wide_counts_slab=slab, **opts)
    first = None
    for it in range(3):
        r = es.estep(a, e, a0)
        d = ran_counts(es)
        if first is None:
            first = r
            gate(r, o, (a, e), (key, opts, slab))
            transitions_ok(r, segs, (key, opts, slab))
        else:
            assert same_bits(r, first), (key, opts, slab, it)
    if opts.get("chunk") == 37:
        assert d["fwd_rounds"] + d["bwd_rounds"] > 0, d   # the tiling does exercise the repairs
    es.close()


# ------------------------------------------------------------------ every size, against the exact kernels
@pytest.mark.parametrize("n", sorted(ONE_WAVE) + MULTI_WAVE)
def test_wide_counts_sizes(hip, golden, n):
    """Both kernel families at both sides of every padding step, on short_segs (1661 bins; segments of 1, 2, 3, 4, 5, 63, 64, 65,
    127 and 129 bins: K not a multiple of 4, segments without a transition, tiles that hold only position L): the gates and the
    invariants against the exact kernels, default tiling and one tile of 64 bins per slab; tri_sums(A) against the factored
    statistics of the same context."""
    par = params(n)
    a, e, a0 = par
    segs = short_segs(golden)
    o = exact(hip, ("sizes", n), n, par, segs)
    for opts in (dict(), dict(chunk=64, warmup=0, wide_counts_slab=64)):
        es = ctx(hip, n, segs, **opts)
        r = es.estep(a, e, a0)
        ran_counts(es)
        gate(r, o, (a, e), (n, opts))
        transitions_ok(r, segs, (n, opts))
        f = es.estep_factored(a, e[:2], a0)
        assert back_half(es) == 3
        err = relmax(tri_sums(r["A"]), f["sums"])
        print("tri_sums(A) vs the factored sums", n, opts, "%.2e" % err)
        if not err <= WORST.get("tri_sums", (-1.0, None))[0]:
            WORST["tri_sums"] = (err, (n, opts))
        assert err < FAST_TOL_STATS, (n, opts, err)
        assert bits_equal(r["E"], f["E"]) and r["LL"] == f["LL"]   # the same sweeps
        es.close()


def test_wide_counts_multiset(hip, golden, oracle, wide):
    """select() with repeats (tests/test_gpu_wide_fast.py test_wide_fast_golden_multiset) against the CPU oracle at 200 states:
    the multiplicities reach A."""
    a, e, a0 = wide["n200.a"], wide["n200.e"], wide["n200.a0"]
    segs = golden.segs_small[:8] + golden.segs_mid[4:]
    sel = [8, 3, 8, 9, 9, 9, 0, 7]
    ms = [segs[i] for i in sel]
    o = oracle.estep(a, e, a0, ms)
    es = ctx(hip, 200, segs, chunk=300, warmup=64)
    es.select(sel)
    r = es.estep(a, e, a0)
    ran_counts(es)
    gate(r, o, (a, e), "multiset")
    transitions_ok(r, ms, "multiset")
    es.close()


@pytest.mark.parametrize("chunk", [37, 38, 39, 41])
def test_wide_counts_anchored_tiles(hip, golden, oracle, wide, chunk):
    """The inputs of test_wide_fast_anchored_tile_below_segment_end: the second-to-last tile's top on every residue modulo 4."""
    a, e, a0 = wide["n200.a"], wide["n200.e"], wide["n200.a0"]
    segs = [golden.segs_mid[0][:L] for L in (1003, 1004, 1005, 1006)] + [golden.segs_mid[1][:2000]]
    if "anchored" not in _EXACT:
        _EXACT["anchored"] = oracle.estep(a, e, a0, segs)
    es = ctx(hip, 200, segs, chunk=chunk, warmup=5)
    r = es.estep(a, e, a0)
    ran_counts(es)
    gate(r, _EXACT["anchored"], (a, e), ("anchored", chunk))
    transitions_ok(r, segs, ("anchored", chunk))
    es.close()


# ------------------------------------------------------------------ fallbacks and inertness
def test_wide_counts_fallbacks(hip, golden, wide):
    """Where the option does not apply psmc_hip_estep is the wide exact kernels, bit for bit: a matrix without the PSMC form,
    "structured" = 0, 300 states with "wide_fast" = 1."""
    segs = short_segs(golden)
    a, e, a0 = wide["n200.a"], wide["n200.e"], wide["n200.a0"]
    rng = np.random.default_rng(3)
    ar = rng.random((200, 200)) ** 4 * 0.02 + np.eye(200) * 0.9
    ar /= ar.sum(1, keepdims=True)
    for what, n, par, opts in (("no PSMC form", 200, (ar, e, a0), dict()), ("structured=0", 200, (a, e, a0), dict(structured=0)),
                               ("300 states, wide_fast=1", 300, mw_params(300), dict(wide_fast=1))):
        x = exact(hip, ("fallback", what), n, par, segs)
        es = ctx(hip, n, segs, **opts)
        r = es.estep(*par)
        assert same_bits(r, x) and bits_equal(r["A0"], x["A0"]), what
        assert back_half(es) != 4, what
        es.close()
    # ... and on a context whose previous E-step did run the wide counts
    es = ctx(hip, 200, segs)
    es.estep(a, e, a0)
    ran_counts(es)
    r = es.estep(ar, e, a0)
    assert same_bits(r, exact(hip, ("fallback", "no PSMC form"), 200, (ar, e, a0), segs)) and back_half(es) != 4
    es.close()


def test_wide_counts_inert_elsewhere(hip, golden):
    """Exact mode beyond 128 states, and 64 states in fast mode: the same bits with and without the option; 2 is EINVAL."""
    segs = short_segs(golden)
    p = golden.params("n64_curve")
    for n, mode, par in ((200, hip.MODE_EXACT, par_of(200)), (64, hip.MODE_FAST, (p["a"], p["e"], p["a0"]))):
        rs = []
        for wc in (0, 1):
            es = hip.HipEStep(n, mode=mode, wide_fast=1, wide_counts=wc)
            es.load_segments(segs)
            rs.append(es.estep(*par))
            assert back_half(es) != 4
            es.close()
        assert same_bits(rs[0], rs[1]), (n, mode)
    es = hip.HipEStep(200, mode=hip.MODE_FAST)
    with pytest.raises(hip.HipError):
        es.set_option("wide_counts", 2)
    with pytest.raises(hip.HipError):
        es.set_option("wide_counts_slab", -1)
    es.close()


def test_estep_device_beyond_128_is_enotsup(hip, golden):
    """psmc_hip_estep_device is not covered: beyond 128 states it answers ENOTSUP, with the option or without, and launches nothing
    (psmc_hip_group_estep falls back to the shards' psmc_hip_estep on that answer)."""
    import torch
    a, e, a0 = par_of(200)
    stats = torch.zeros(200 * 200 + 2 * 200 + 1, dtype=torch.float64, device="cuda")
    for wc in (0, 1):
        es = ctx(hip, 200, short_segs(golden), wide_counts=wc)
        with pytest.raises(hip.HipError, match="not supported"):
            es.estep_device(a, e, a0, stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
        es.close()
    assert not stats.cpu().numpy().any()


def test_wide_counts_econverge_and_recovery(hip, golden, wide):
    """max_rounds = 1 with tiles of 37 bins, warm-up 5 and learn = 0: ECONVERGE, as the factored wide E-step answers it.  With the
    defaults restored the next call has the bits of a fresh context."""
    a, e, a0 = wide["n200.a"], wide["n200.e"], wide["n200.a0"]
    segs = golden.segs_small[:8]
    es = ctx(hip, 200, segs, chunk=37, warmup=5, learn=0, max_rounds=1)
    with pytest.raises(hip.HipError, match="converge"):
        es.estep(a, e, a0)
    for k, v in dict(chunk=0, warmup=16384, learn=1, max_rounds=4096).items():
        es.set_option(k, v)
    r = es.estep(a, e, a0)
    ran_counts(es)
    gate(r, dict(A=wide["n200.A"], E=wide["n200.E"], LL=float(wide["n200.LL"])), (a, e), "after ECONVERGE")
    es.close()
    fresh = ctx(hip, 200, segs)
    r2 = fresh.estep(a, e, a0)
    ran_counts(fresh)
    assert same_bits(r, r2)
    fresh.close()


# ------------------------------------------------------------------ interplay with the other options of the path
@pytest.mark.parametrize("n", [200, 300])
def test_wide_counts_with_ckpt(hip, golden, n):
    """ "wide_ckpt" = 1: a wide-counts E-step keeps the full table (interval 1) and has the bits of the run without "wide_ckpt";
    the factored E-step that follows is checkpointed again (interval 8) and keeps its own bits."""
    par = par_of(n)
    a, e, a0 = par
    segs = short_segs(golden)
    plain = ctx(hip, n, segs)
    r0 = plain.estep(a, e, a0)
    ran_counts(plain)
    f0 = plain.estep_factored(a, e[:2], a0)
    plain.close()
    gate(r0, exact(hip, ("ckpt", n), n, par, segs), (a, e), ("ckpt reference", n))
    es = ctx(hip, n, segs, wide_ckpt=1)
    for it in range(2):
        r = es.estep(a, e, a0)
        ran_counts(es)
        assert es.wide_table_info()["interval"] == 1
        assert same_bits(r, r0), (n, it)
        f = es.estep_factored(a, e[:2], a0)
        assert es.wide_table_info()["interval"] == 8 and back_half(es) == 3
        assert bits_equal(f["sums"], f0["sums"]) and bits_equal(f["E"], f0["E"]) and f["LL"] == f0["LL"], (n, it)
    es.close()


@pytest.mark.parametrize("n", [200, 300])
def test_wide_counts_then_decode(hip, golden, n):
    """ "wide_decode" = 1: decode / posterior after a wide-counts E-step are, bit for bit, those after estep_factored with the same
    parameters (the E-step is "the last single E-step" either way)."""
    a, e, a0 = par_of(n)
    segs = short_segs(golden)
    seg = len(segs) - 1
    out = []
    for counts in (False, True):
        es = ctx(hip, n, segs, wide_decode=1)
        if counts:
            es.estep(a, e, a0)
            ran_counts(es)
        else:
            es.estep_factored(a, e[:2], a0)
        out.append(es.decode(seg) + es.posterior(seg))
        es.close()
    assert np.array_equal(out[0][0], out[1][0])
    for x, y in zip(out[0][1:], out[1][1:]):
        assert bits_equal(x, y)


# ------------------------------------------------------------------ batch and group
@pytest.mark.parametrize("n", [200, 300])
def test_wide_counts_batch(hip, golden, n):
    """ "wide_batch" + "wide_counts": four replicates with their own parameters and multisets, A beside sums -- every row has the
    bits of select + estep / estep_factored on a fresh context; batch_info {4, 0}; the caller's selection comes back.  With
    "wide_counts" = 0 a batch that asks for A takes the exact launch groups: the bits of an exact context's batch."""
    from test_gpu_wide_fast_batch import rep_params, sels, N_REP
    segs = short_segs(golden)
    pars, ss = rep_params(n), sels(len(segs))
    es = ctx(hip, n, segs, wide_batch=1)
    es.select([3, 3, 16])
    b = es.estep_batch(pars, ss, want="both")
    assert es.batch_info() == dict(groups=N_REP, replicate_contexts=0)
    assert back_half(es) == 4
    after = es.estep(*pars[0])   # on the selection the context had before the batch
    ran_counts(es)
    es.close()
    x = exact(hip, ("batch sel", n), n, pars[0], segs, [3, 3, 16])
    gate(after, x, (pars[0][0], pars[0][1]), ("selection restored", n))
    for r in range(N_REP):
        fr = ctx(hip, n, segs)
        fr.select(ss[r])
        one = fr.estep(*pars[r])
        ran_counts(fr)
        f = fr.estep_factored(pars[r][0], pars[r][1][:2], pars[r][2])
        fr.close()
        assert bits_equal(b["A"][r], one["A"]) and bits_equal(b["E"][r], one["E"]) and b["LL"][r] == one["LL"], (n, r)
        assert bits_equal(b["sums"][r], f["sums"]), (n, r)
        o = exact(hip, ("batch", n, r), n, pars[r], segs, ss[r])
        gate(dict(A=b["A"][r], E=b["E"][r], LL=float(b["LL"][r]), A0=np.zeros(n), chk=np.ones(1)), o, (pars[r][0], pars[r][1]), ("batch", n, r))
        transitions_ok(dict(A=b["A"][r]), [segs[i] for i in ss[r]], ("batch", n, r))
    # A alone
    es = ctx(hip, n, segs, wide_batch=1)
    b2 = es.estep_batch(pars, ss, want="A")
    assert back_half(es) == 4 and es.batch_info() == dict(groups=N_REP, replicate_contexts=0)
    es.close()
    assert bits_equal(b2["A"], b["A"]) and bits_equal(b2["E"], b["E"]) and bits_equal(b2["LL"], b["LL"])
    # without "wide_counts": the exact launch groups
    ex = hip.HipEStep(n, mode=hip.MODE_EXACT)
    ex.load_segments(segs)
    xb = ex.estep_batch(pars, ss, want="A")
    ex.close()
    es = ctx(hip, n, segs, wide_counts=0, wide_batch=1)
    b0 = es.estep_batch(pars, ss, want="A")
    assert back_half(es) != 4
    es.close()
    assert bits_equal(b0["A"], xb["A"]) and bits_equal(b0["E"], xb["E"]) and bits_equal(b0["LL"], xb["LL"])


def test_wide_counts_group_300(hip, golden):
    """psmc_hip_group over devices [0, 0] at 300 states: the shards' psmc_hip_estep run the wide counts, and the sum passes the gates."""
    par = mw_params(300)
    a, e, a0 = par
    segs = short_segs(golden)
    o = exact(hip, ("sizes", 300), 300, par, segs)
    g = hip.HipGroup(300, [0, 0], mode=hip.MODE_FAST, wide_fast=2, wide_counts=1)
    g.load_segments(segs)
    r = g.estep(a, e, a0)
    from psmc_amd.parity import fast_error_metrics
    m = fast_error_metrics(r, o, a, e)
    print("wide counts group [0, 0] 300", "  ".join("%s %.2e" % (k, m[k]) for k in sorted(m)))
    assert relmax(r["A"], o["A"]) < FAST_TOL_STATS and relmax(r["E"], o["E"][:2]) < FAST_TOL_STATS
    assert abs(r["LL"] - o["LL"]) <= FAST_TOL_LL * abs(o["LL"])
    assert m["A_cell"] <= FAST_TOL_CELL and m["E_cell"] <= FAST_TOL_CELL and m["A_l1"] <= FAST_TOL_L1, m
    assert m["QA"] <= FAST_TOL_Q and m["QE"] <= FAST_TOL_Q, m
    transitions_ok(r, segs, "group")
    import ctypes as C
    for seg in (0, len(segs) - 1):   # the context that holds the segment: its last E-step was a wide-counts one
        c, loc, fi = C.c_void_p(), C.c_int(0), (C.c_int * 8)()
        g.lib.psmc_hip_group_route.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        assert g.lib.psmc_hip_group_route(g.g, seg, C.byref(c), C.byref(loc)) == 0
        g.lib.psmc_hip_fast_info.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        assert g.lib.psmc_hip_fast_info(c, fi) == 0 and fi[4] == 4, list(fi)
    g.close()
