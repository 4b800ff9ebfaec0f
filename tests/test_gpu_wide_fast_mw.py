"""Fast mode at 257 .. 1024 hidden states: psmc_hip_estep_factored with the option "wide_fast" = 2 (the kernels of
psmc_amd/csrc/estep_wide_fast.hip at W > 1: a tile is one work-group of 2, 3 or 4 waves at the padded widths 512, 768 and 1024; the
waves exchange their scan totals through LDS once per position).  References: the exact wide kernels on the same device (which
the suite pins bit for bit against the reference up to 1024 states), the CPU oracle at 300 states, and a fresh context for the
bit-for-bit claims.  Gates and tolerances: the ones of tests/test_gpu_wide_fast.py (fast mode's own, tests/test_gpu_estep.py):
statistics 1e-10 of the largest cell, LL 1e-12 relative, per vector cell 1e-9 / L1 1e-10 / QA, QE 1e-10.  There are no NPL = 3
widths on this path, so the sizes are the issue's own: both sides of every padding step (512 | 513, 768 | 769), the first size
beyond the one-wave path (257), the largest (1024) and sizes inside each width.

Observed on the MI355X (-s prints every comparison; the fixture report_worst where each metric was largest):
bounds FAST_TOL_CELL 1e-9, FAST_TOL_L1 / FAST_TOL_Q 1e-10, block gates 1e-10, LL 1e-12.  This file, 83 comparisons:
  mild models (seeded random lambdas), every size and tiling, against the exact kernels and the oracle:
    cell <= 8.0e-14 (DG / E0 / E1, the anchored tiles at 512 states; 6.6e-14 at 1024 states), L1 <= 1.9e-14, QA / QE <= 1.7e-14
    (the oracle comparison at 300 states), block gates <= 5.5e-14 (1024 states), LL <= 4.7e-16 relative
  model extremes at 1024 states, default tiling:
    rho0 = 1e-6: cell SL 4.5e-13  SU 5.1e-13  DG 6.6e-13  CL 7.8e-13  CU 4.6e-13  E0 6.6e-13  E1 6.4e-13, L1 <= 2.3e-13 (CL),
                 QA 1.7e-13, block gates 5.9e-13, LL 2.3e-15 -- the figures of the one-wave path at 256 states on that model
                 (tests/test_gpu_wide_fast_edges.py: cell <= 1.0e-12)
    t_max = 60:  cell <= 6.6e-14, L1 <= 1.4e-14, QA / QE <= 8.7e-15, LL 1.4e-15
  (tests/test_wide_fast_mw_model.py: the numpy model of fast mode against the oracle, untiled, 2.4e-14 / 3.4e-14 at 512 / 1024 states)
tests/test_host_cli_wide_fast_mw.py, psmc -N2 -p "150*2" against exact E-steps: LK 8.6e-10, theta_0 / rho_0 6.2e-6, lambda_k 1.3e-2.
"""
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal
from test_gpu_wide_fast import check, ran_wide, tri_sums, psmc_params, WORST

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# states: pattern, free lambdas (a pattern has at most 255 groups, and a group repeats at most 255 times)
SIZES = {257: ("1+128*2", 129), 300: ("150*2", 150), 511: ("3+254*2", 255), 512: ("128*4", 128), 513: ("1+128*4", 129),
         768: ("128*6", 128), 769: ("1+128*6", 129), 1000: ("250*4", 250), 1024: ("128*8", 128)}
TILINGS = [dict(), dict(chunk=500, warmup=40)]
TILINGS_MORE = [dict(chunk=37, warmup=5), dict(chunk=64, warmup=0), dict(chunk=100, warmup=30, learn=0)]   # at 300 and 1024 states


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    """after the module: where each metric of the per-vector gates was largest (shown with -s)"""
    yield
    for k in sorted(WORST):
        print("worst %-8s %.3e  %s" % (k, WORST[k][0], WORST[k][1]))


def params(n, seed=None):
    pat, m = SIZES[n]
    return psmc_params(pat, m, np.random.default_rng(2000 + n if seed is None else seed))


def short_segs(golden):
    """golden.segs_small[:8] (1, 2, 3, 63, 64, 65, 127, 129 bins) plus segments of 1, 2, 3, 4, 5, 63, 64 and 65 bins cut from other
    data, and one of 1000 bins so that the default tiling has more than one tile per segment: 1661 bins"""
    src = golden.segs_mid[4]
    extra, at = [], 100
    for L in (1, 2, 3, 4, 5, 63, 64, 65):
        extra.append(src[at:at + L]); at += L + 7
    return golden.segs_small[:8] + extra + [golden.segs_small[8]]


def exact(hip, n, par, segs, sel=None):
    ex = hip.HipEStep(n, mode=hip.MODE_EXACT)
    ex.load_segments(segs)
    if sel is not None:
        ex.select(sel)
    x = ex.estep(*par)
    ex.close()
    return tri_sums(x["A"]), x["E"], x["LL"]


_REF = {}


def exact_ref(hip, golden, n):
    """the exact kernels' statistics of params(n) on short_segs, computed once per size"""
    if n not in _REF:
        _REF[n] = exact(hip, n, params(n), short_segs(golden))
    return _REF[n]


def same_bits(r, w):
    return bits_equal(r["sums"], w["sums"]) and bits_equal(r["E"], w["E"]) and r["LL"] == w["LL"]


def wide2(hip, n, segs, **opts):
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=2, **opts)
    es.load_segments(segs)
    return es


# ------------------------------------------------------------------ against the exact kernels on the same device
@pytest.mark.parametrize("n", list(SIZES))
def test_mw_vs_exact(hip, golden, n):
    """Every size, every tiling it is asked at: three factored E-steps in a row on one context pass all gates and the invariants
    against the exact kernels and give the same bits; the wide path ran (fast_repairs out[5] = 2, fast_info back half 3)."""
    a, e, a0 = params(n)
    segs = short_segs(golden)
    sums, E, LL = exact_ref(hip, golden, n)
    for opts in TILINGS + (TILINGS_MORE if n in (300, 1024) else []):
        es = wide2(hip, n, segs, **opts)
        first = None
        for it in range(3):
            r = es.estep_factored(a, e[:2], a0)
            check(r, sums, E, LL, (n, opts, it), (a, e), segs)
            d = ran_wide(es)
            if first is None:
                first = r
            else:
                assert same_bits(r, first), (n, opts, it)
        if opts.get("chunk") == 37:
            assert d["fwd_rounds"] + d["bwd_rounds"] > 0, d   # the tiling does exercise the repairs
        es.close()


def test_mw_vs_oracle_300(hip, golden, oracle):
    """One reference that is not this library: the CPU oracle at 300 states on 9800 bins (segments of 1 .. 5000 bins), default
    tiles and tiles small enough to repair."""
    a, e, a0 = params(300)
    segs = golden.segs_small[:10] + [golden.segs_mid[4][:4200]]
    assert sum(len(s) for s in segs) <= 10000
    o = oracle.estep(a, e, a0, segs)
    want = tri_sums(o["A"])
    for opts in (dict(), dict(chunk=500, warmup=40)):
        es = wide2(hip, 300, segs, **opts)
        r = es.estep_factored(a, e[:2], a0)
        check(r, want, o["E"], o["LL"], ("oracle 300", opts), (a, e), segs)
        ran_wide(es)
        es.close()


def test_mw_multiset_300(hip, golden):
    """select() with repeated segments (a bootstrap multiset) against the exact kernels on the same multiset."""
    a, e, a0 = params(300)
    segs = golden.segs_small[:10] + [golden.segs_mid[5]]
    sel = [8, 3, 8, 9, 9, 10, 0, 7, 10, 10]
    sums, E, LL = exact(hip, 300, (a, e, a0), segs, sel)
    es = wide2(hip, 300, segs, chunk=300, warmup=64)
    es.select(sel)
    r = es.estep_factored(a, e[:2], a0)
    check(r, sums, E, LL, "multiset 300", (a, e), [segs[i] for i in sel])
    ran_wide(es)
    es.close()


@pytest.mark.parametrize("chunk", [37, 38, 39, 41])
def test_mw_anchored_tile_below_segment_end(hip, golden, chunk):
    """tests/test_gpu_wide_fast.py test_wide_fast_anchored_tile_below_segment_end at 512 states: tiles whose backward warm-up
    starts at the segment's last position, the second-to-last tile's top on every residue modulo 4."""
    a, e, a0 = params(512)
    segs = [golden.segs_mid[0][:L] for L in (1003, 1004, 1005, 1006)] + [golden.segs_mid[1][:2000]]
    if "anchored" not in _REF:
        _REF["anchored"] = exact(hip, 512, (a, e, a0), segs)
    sums, E, LL = _REF["anchored"]
    es = wide2(hip, 512, segs, chunk=chunk, warmup=5)
    r = es.estep_factored(a, e[:2], a0)
    check(r, sums, E, LL, ("anchored 512", chunk), (a, e), segs)
    ran_wide(es)
    es.close()


@pytest.mark.parametrize("name,pa", [("rho_1e-6", [0.02, 1e-6, 15.0]), ("tmax_60", [0.02, 0.004, 60.0])])
def test_mw_model_extremes_1024(hip, golden, name, pa):
    """The two harsh ends of tests/test_gpu_wide_fast_edges.py at 1024 states, default tiling: rho0 = 1e-6 (a chain that barely
    forgets) and t_max = 60 (matrix entries far down the double range), against the exact kernels on 11500 bins."""
    from psmc_amd import hostlib
    a, e, a0 = hostlib.hmm_params("128*8", pa + [1.0] * 128)
    segs = golden.segs_small[:10] + [golden.segs_mid[3][:6000]]
    sums, E, LL = exact(hip, 1024, (a, e, a0), segs)
    assert np.isfinite(sums).all() and np.isfinite(LL)
    es = wide2(hip, 1024, segs)
    r = es.estep_factored(a, e[:2], a0)
    check(r, sums, E, LL, (name, 1024), (a, e), segs)
    ran_wide(es)
    es.close()


# ------------------------------------------------------------------ option edges
def test_mw_option_edges(hip, golden):
    """ "wide_fast" = 2 at 200 states: the bits of = 1; = 3: EINVAL; a matrix without the PSMC form at 300 states: ENOTSUP;
    "wide_fast" = 1 at 300 states: ENOTSUP naming 256, as before."""
    segs = short_segs(golden)
    a, e, a0 = psmc_params("100*2", 100, np.random.default_rng(11))
    rs = []
    for v in (1, 2):
        es = hip.HipEStep(200, mode=hip.MODE_FAST, wide_fast=v)
        es.load_segments(segs)
        rs.append(es.estep_factored(a, e[:2], a0))
        ran_wide(es)
        es.close()
    assert same_bits(rs[0], rs[1])
    es = hip.HipEStep(300, mode=hip.MODE_FAST)
    with pytest.raises(hip.HipError):
        es.set_option("wide_fast", 3)
    es.set_option("wide_fast", 1)
    es.load_segments(segs)
    a, e, a0 = params(300)
    with pytest.raises(hip.HipError, match="256"):
        es.estep_factored(a, e[:2], a0)
    es.set_option("wide_fast", 2)
    rng = np.random.default_rng(3)
    ar = rng.random((300, 300)) ** 4 * 0.02 + np.eye(300) * 0.9
    ar /= ar.sum(1, keepdims=True)
    with pytest.raises(hip.HipError, match="PSMC form"):
        es.estep_factored(ar, e[:2], a0)
    es.set_option("structured", 0)
    with pytest.raises(hip.HipError, match="structured"):
        es.estep_factored(a, e[:2], a0)
    es.close()


def test_mw_econverge_and_recovery(hip, golden):
    """max_rounds = 1 with tiles of 37 bins, warm-up 5 and learn = 0: ECONVERGE.  Options back to the defaults: the next E-step
    passes the gates and has the bits of a fresh context."""
    a, e, a0 = params(300)
    segs = short_segs(golden)
    sums, E, LL = exact_ref(hip, golden, 300)
    es = wide2(hip, 300, segs, chunk=37, warmup=5, learn=0, max_rounds=1)
    with pytest.raises(hip.HipError, match="converge"):
        es.estep_factored(a, e[:2], a0)
    for k, v in dict(chunk=0, warmup=16384, learn=1, max_rounds=4096).items():
        es.set_option(k, v)
    r = es.estep_factored(a, e[:2], a0)
    check(r, sums, E, LL, "after ECONVERGE", (a, e), segs)
    assert ran_wide(es)["warmup"] == 16384
    es.close()
    fresh = wide2(hip, 300, segs)
    r2 = fresh.estep_factored(a, e[:2], a0)
    assert ran_wide(fresh)["warmup"] == 16384
    assert same_bits(r, r2)
    fresh.close()


def test_mw_everything_else_stays_exact(hip, golden):
    """psmc_hip_estep of a "wide_fast" = 2 context at 300 states is bit-identical to an exact context's, tables() is unchanged by a
    wide fast E-step in between, and with "wide_decode" = 1 the decoding after psmc_hip_estep is the exact context's, bit for
    bit (beyond 256 states "wide_decode" has no effect)."""
    a, e, a0 = params(300)
    segs = short_segs(golden)
    ex = hip.HipEStep(300, mode=hip.MODE_EXACT)
    ex.load_segments(segs)
    x = ex.estep(a, e, a0)
    seg = len(segs) - 1
    xpath, xmp = ex.decode(seg)
    xpost, xrec = ex.posterior(seg)
    ex.close()
    es = wide2(hip, 300, segs, wide_decode=1)
    r = es.estep(a, e, a0)
    assert bits_equal(r["A"], x["A"]) and bits_equal(r["E"], x["E"]) and r["LL"] == x["LL"]
    f, b, sc = es.tables(seg)
    es.estep_factored(a, e[:2], a0)
    ran_wide(es)
    f2, b2, sc2 = es.tables(seg)
    assert bits_equal(f2, f) and bits_equal(b2, b) and bits_equal(sc2, sc)
    r = es.estep(a, e, a0)
    assert bits_equal(r["A"], x["A"]) and r["LL"] == x["LL"]
    path, mp = es.decode(seg)
    post, rec = es.posterior(seg)
    assert np.array_equal(path, xpath) and bits_equal(mp, xmp) and bits_equal(post, xpost) and bits_equal(rec, xrec)
    es.close()


def test_mw_group_300(hip, golden):
    """psmc_hip_group over devices [0, 0] with "wide_fast" = 2 at 300 states: the sharded factored E-step within tolerance of the
    single context's reference."""
    a, e, a0 = params(300)
    segs = short_segs(golden)
    sums, E, LL = exact_ref(hip, golden, 300)
    g = hip.HipGroup(300, [0, 0], mode=hip.MODE_FAST, wide_fast=2)
    g.load_segments(segs)
    r = g.estep_factored(a, e[:2], a0)
    check(r, sums, E, LL, "group [0, 0] 300", (a, e), segs)
    g.close()
