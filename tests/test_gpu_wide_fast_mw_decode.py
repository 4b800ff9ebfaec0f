"""Decoding on the multi-wave wide fast path: a fast-mode context of 257..1024 states with "wide_fast" = 2 and "wide_decode" = 1
answers psmc_hip_decode / _posterior / _post_counts / _scales from what its last wide fast factored E-step left (X at the padded
width 512 / 768 / 1024, 1/d, the tiles' start vectors; no backward table -- psmc_amd/csrc/estep_wide_post.hip).  Every
comparison is against an EXACT context given the same parameters and segments, with compare() of
tests/test_gpu_wide_fast_decode.py: compare_decoding's tolerances, the library's own for fast decoding (include/psmc_hip.h) --
posterior rows, maxp, recomb 1e-9 absolute; scales 1e-11 relative; post_counts 1e-9 relative on cells >= 1e-6 of the largest;
path equal wherever the exact posterior's two largest entries differ by more than 2e-9 -- and fewer than 0.1 % of the positions
of a case may be such near-ties (counted from the exact context alone; tests/test_wide_decode_mw_model.py counts them from the
oracle and checks the formulas against it on the CPU).  The posterior's per-symbol sums are checked against the E-step's E.
compare_decoding prints the observed maxima of every case; the fixture report_worst the largest of the module.

Observed on the MI355X, the worst of each output over this file's 27 comparisons: posterior rows 1.5e-14, maxp 1.2e-14, recomb
1.9e-13, scales 5.6e-14 relative, post_counts 9.9e-13 relative -- all five at rho0 = 1e-6 and 1024 states; the mild models at every
size and tiling stay below 1e-13 (post_counts 6.8e-14).  No path difference anywhere, no near-tie in any case.
tests/test_host_cli_wide_fast_mw_decode.py: every printed digit within one unit of the exact run's."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal
from test_gpu_fast_decode import TOL_POST
from test_gpu_wide_fast import ran_wide
from test_gpu_wide_fast_mw import params, short_segs
from test_gpu_wide_fast_decode import compare, _all_outputs, _same_bits
from test_wide_decode_mw_model import RHO_1E6, SEED2, extreme_segs, GPU_SIZES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    """after the module: the largest error of each output over its comparisons (shown with -s)"""
    yield
    for ex in _EXACT.values():
        ex.close()
    _EXACT.clear()
    for k in sorted(WORST):
        print("worst %-7s %.3e  %s" % (k, WORST[k][0], WORST[k][1]))


def note(w, what):
    for k in ("post", "maxp", "recomb", "scales"):
        if k not in WORST or w[k] > WORST[k][0]:
            WORST[k] = (w[k], what)
    WORST["ties"] = (WORST.get("ties", (0, ""))[0] + w["ties"], "path differences at near-ties, all cases")


def fast_ctx(hip, n, segs, **opts):
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=2, wide_decode=1, **opts)
    es.load_segments(segs)
    return es


def exact_ctx(hip, n, segs, par):
    ex = hip.HipEStep(n, mode=hip.MODE_EXACT)
    ex.load_segments(segs)
    ex.estep(*par)
    return ex


_EXACT = {}


def exact_short(hip, golden, n):
    """the exact context of params(n) on short_segs after its E-step, made once per size and only read afterwards"""
    if n not in _EXACT:
        _EXACT[n] = exact_ctx(hip, n, short_segs(golden), params(n))
    return _EXACT[n]


def cells_close(cf, cx):
    big = np.abs(cx) >= 1e-6 * np.abs(cx).max()
    cell = float((np.abs(cf - cx)[big] / np.abs(cx)[big]).max())
    if "counts" not in WORST or cell > WORST["counts"][0]:
        WORST["counts"] = (cell, "post_counts cases")
    print("post_counts vs exact: %.2e" % cell)
    return cell <= 1e-9


# ---- 1. sizes on both sides of every padding step, all three W; tilings with repairs, tiny tiles, a tile that holds only position L
MORE = [dict(chunk=37, warmup=5), dict(chunk=64, warmup=0), dict(chunk=8, warmup=3), dict(chunk=4, warmup=0), dict(chunk=5, warmup=64)]
SIZE_CASES = [(n, o) for n in GPU_SIZES for o in [dict(), dict(chunk=500, warmup=40)] + (MORE if n in (300, 1024) else [])]


@pytest.mark.parametrize("n,opts", SIZE_CASES, ids=["%d-%s" % (n, "-".join("%s%d" % kv for kv in o.items()) or "default") for n, o in SIZE_CASES])
def test_mw_decode_sizes(hip, golden, n, opts):
    a, e, a0 = params(n)
    segs = short_segs(golden)
    exact = exact_short(hip, golden, n)
    fast = fast_ctx(hip, n, segs, **opts)
    rf = fast.estep_factored(a, e[:2], a0)
    d = ran_wide(fast)
    if opts.get("chunk") == 37:
        assert d["fwd_rounds"] + d["bwd_rounds"] > 0, d   # bentry of repaired tiles is what gets decoded
    note(compare(fast, exact, segs, n, E=rf["E"]), (n, opts))
    fast.close()


# ---- 2. a chain that barely forgets, at the largest width
def test_mw_decode_model_extreme_rho(hip, golden):
    from psmc_amd import hostlib
    a, e, a0 = hostlib.hmm_params("128*8", RHO_1E6)
    segs = extreme_segs(golden)
    assert sum(len(s) for s in segs) == 8551
    exact = exact_ctx(hip, 1024, segs, (a, e, a0))
    fast = fast_ctx(hip, 1024, segs)
    rf = fast.estep_factored(a, e[:2], a0)
    ran_wide(fast)
    note(compare(fast, exact, segs, 1024, E=rf["E"]), "rho0 = 1e-6, 1024 states")
    fast.close(); exact.close()


# ---- 3. post_counts
@pytest.mark.parametrize("opts", [dict(), dict(chunk=8, warmup=3)], ids=["default", "chunk8"])
def test_mw_post_counts_one_column(hip, golden, opts):
    """n_cnt = 1, l shorter and longer than L, running totals carried from segment to segment"""
    a, e, a0 = params(300)
    segs = short_segs(golden)
    exact = exact_short(hip, golden, 300)
    fast = fast_ctx(hip, 300, segs, **opts)
    fast.estep_factored(a, e[:2], a0)
    ran_wide(fast)
    rng = np.random.default_rng(5)
    cf = np.zeros((300, 1)); cx = np.zeros((300, 1))
    for seg, obs in enumerate(segs):
        for l in (max(0, len(obs) - 2), len(obs), len(obs) + 7):
            c1 = rng.integers(0, 50, size=(l, 1), dtype=np.int32)
            fast.post_counts(seg, c1, cf); exact.post_counts(seg, c1, cx)
    assert cells_close(cf, cx)
    fast.close()


def test_mw_post_counts_five_columns(hip, golden):
    """n_cnt = 5: two sweeps of four count columns, at 513 states (three waves, 255 padded states)"""
    a, e, a0 = params(513)
    segs = short_segs(golden)
    exact = exact_short(hip, golden, 513)
    fast = fast_ctx(hip, 513, segs)
    fast.estep_factored(a, e[:2], a0)
    ran_wide(fast)
    rng = np.random.default_rng(6)
    cf = np.zeros((513, 5)); cx = np.zeros((513, 5))
    for seg, obs in enumerate(segs):
        c1 = rng.integers(0, 50, size=(len(obs), 5), dtype=np.int32)
        fast.post_counts(seg, c1, cf); exact.post_counts(seg, c1, cx)
    assert cells_close(cf, cx)
    fast.close()


# ---- 4. selections
def test_mw_decode_selections(hip, golden):
    """A segment selected twice is decoded once (all copies are equal); segments outside the selection are refused."""
    a, e, a0 = params(300)
    segs = short_segs(golden)
    exact = exact_short(hip, golden, 300)
    fast = fast_ctx(hip, 300, segs, chunk=100, warmup=30)
    fast.select([8, 3, 8, 5, 5, 5, 0])
    fast.estep_factored(a, e[:2], a0)
    ran_wide(fast)
    note(compare(fast, exact, segs, 300, ids=[0, 3, 5, 8]), "selection, 300 states")
    for seg in (1, 2, 4, 6, 7, 16):
        with pytest.raises(hip.HipError, match="call order violated.*selection"):
            fast.decode(seg)
    fast.close()


# ---- 5. the last single E-step decides
def test_mw_decode_follows_the_last_estep(hip, golden):
    a, e, a0 = params(300)
    a2, e2, a02 = params(300, SEED2)
    segs = short_segs(golden)
    ex1 = exact_short(hip, golden, 300)
    ex2 = exact_ctx(hip, 300, segs, (a2, e2, a02))
    want1 = _all_outputs(ex1, segs, 300)
    for wd in (1, 0):
        es = hip.HipEStep(300, mode=hip.MODE_FAST, wide_fast=2, wide_decode=wd, chunk=100, warmup=30)
        es.load_segments(segs)
        es.estep(a, e, a0)                         # exact E-step -> the exact tables, bit for bit, with or without the option
        assert _same_bits(_all_outputs(es, segs, 300), want1)
        rf = es.estep_factored(a2, e2[:2], a02)    # wide fast E-step at other parameters
        ran_wide(es)
        if wd:                                     # ... -> its tables: the decoding of the NEW parameters
            note(compare(es, ex2, segs, 300, E=rf["E"]), "after estep_factored, 300 states")
            p_new, _ = es.posterior(16)
            p_old, _ = ex1.posterior(16)
            assert float(np.abs(p_new - p_old).max()) > 1e3 * TOL_POST   # (not the stale exact tables)
            es.estep(a, e, a0)                     # and an exact E-step afterwards takes over again
            assert _same_bits(_all_outputs(es, segs, 300), want1)
        else:                                      # "wide_decode" = 0: the exact tables whatever ran last, as before the option
            assert _same_bits(_all_outputs(es, segs, 300), want1)
        es.close()
    ex2.close()


# ---- 6. refusals
def test_mw_decode_refusals(hip, golden):
    a, e, a0 = params(300)
    segs = short_segs(golden)
    calls = [lambda c: c.decode(5), lambda c: c.posterior(5), lambda c: c.scales(5),
             lambda c: c.post_counts(5, np.ones((len(segs[5]), 1), np.int32), np.zeros((c.n, 1)))]

    def refused(es, match="call order violated"):
        for f in calls:
            with pytest.raises(hip.HipError, match=match):
                f(es)

    es = fast_ctx(hip, 300, segs)
    refused(es)                                   # no E-step yet
    es.estep_factored(a, e[:2], a0)
    for f in calls:
        f(es)
    es.estep_batch([(a, e, a0)] * 2, [[0, 1], [2, 3]])   # a batch: a single E-step is needed again
    refused(es)
    es.estep_factored(a, e[:2], a0)
    for f in calls:
        f(es)
    es.select([5, 6, 7])                          # the selection changed since
    refused(es, "call order violated.*selection")
    es.estep_factored(a, e[:2], a0)
    for f in calls:
        f(es)
    with pytest.raises(hip.HipError, match="call order violated.*selection"):
        es.decode(0)                              # outside the selection
    es.load_segments(segs)                        # a reload
    refused(es)
    es.close()

    es = fast_ctx(hip, 300, segs, chunk=37, warmup=5, learn=0, max_rounds=0)
    with pytest.raises(hip.HipError, match="converge"):
        es.estep_factored(a, e[:2], a0)
    refused(es, "call order violated.*returned an error")   # bentry is not converged
    es.set_option("max_rounds", 4096)
    es.estep_factored(a, e[:2], a0)
    for f in calls:
        f(es)
    es.close()

    # "wide_fast" = 1 with "wide_decode" = 1 at 300 states: the exact kernels, bit for bit
    es = hip.HipEStep(300, mode=hip.MODE_FAST, wide_fast=1, wide_decode=1)
    es.load_segments(segs)
    es.estep(a, e, a0)
    assert _same_bits(_all_outputs(es, segs, 300), _all_outputs(exact_short(hip, golden, 300), segs, 300))
    es.close()


# ---- 7. a decoding call reads only
def test_mw_decode_has_no_side_effects(hip, golden):
    a, e, a0 = params(512)
    a2, e2, a02 = params(512, 11)
    segs = short_segs(golden)
    ctx = [fast_ctx(hip, 512, segs, chunk=100, warmup=30) for _ in range(2)]
    for c in ctx:
        c.estep_factored(a, e[:2], a0)
    for seg in range(len(segs)):
        ctx[1].decode(seg); ctx[1].posterior(seg); ctx[1].scales(seg)
        ctx[1].post_counts(seg, np.ones((len(segs[seg]), 2), np.int32), np.zeros((512, 2)))
    for pa in ((a2, e2, a02), (a, e, a0)):
        r = [c.estep_factored(pa[0], pa[1][:2], pa[2]) for c in ctx]
        assert bits_equal(r[0]["sums"], r[1]["sums"]) and bits_equal(r[0]["E"], r[1]["E"]) and r[0]["LL"] == r[1]["LL"]
    for c in ctx:
        c.close()


# ---- 8. determinism
def test_mw_decode_is_deterministic(hip, golden):
    a, e, a0 = params(769)
    segs = short_segs(golden)
    outs = []
    for _ in range(2):
        es = fast_ctx(hip, 769, segs, chunk=64, warmup=8)
        es.estep_factored(a, e[:2], a0)
        ran_wide(es)
        outs.append(_all_outputs(es, segs, 769))
        outs.append(_all_outputs(es, segs, 769))   # and the same context again
        es.close()
    for o in outs[1:]:
        assert _same_bits(o, outs[0])


# ---- 9. a group of two shards on one device
def test_mw_decode_group_300(hip, golden):
    """psmc_hip_group over devices [0, 0] with both options: after the sharded factored E-step a segment's posterior and path,
    read from its shard through psmc_hip_group_route, are the exact context's within the tolerances."""
    a, e, a0 = params(300)
    segs = short_segs(golden)
    exact = exact_short(hip, golden, 300)
    g = hip.HipGroup(300, [0, 0], mode=hip.MODE_FAST, wide_fast=2, wide_decode=1)
    g.load_segments(segs)
    g.estep_factored(a, e[:2], a0)
    lib = g.lib
    lib.psmc_hip_group_route.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    dp = C.POINTER(C.c_double)
    lib.psmc_hip_posterior.argtypes = [C.c_void_p, C.c_int, dp, dp]
    lib.psmc_hip_decode.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), dp]
    seg = 16                                       # the 1000-bin segment
    ctx, local = C.c_void_p(), C.c_int(-1)
    assert lib.psmc_hip_group_route(g.g, seg, C.byref(ctx), C.byref(local)) == 0
    L = len(segs[seg])
    post = np.zeros((L, 300)); rec = np.zeros(L); path = np.zeros(L, np.int32); mp = np.zeros(L)
    assert lib.psmc_hip_posterior(ctx, local.value, post.ctypes.data_as(dp), rec.ctypes.data_as(dp)) == 0
    assert lib.psmc_hip_decode(ctx, local.value, path.ctypes.data_as(C.POINTER(C.c_int32)), mp.ctypes.data_as(dp)) == 0
    px, rx = exact.posterior(seg)
    xp, xm = exact.decode(seg)
    assert float(np.abs(post - px).max()) <= TOL_POST and float(np.abs(rec - rx).max()) <= TOL_POST
    assert float(np.abs(mp - xm).max()) <= TOL_POST
    top2 = np.sort(px, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2e-9
    assert clear.mean() > 0.999 and np.array_equal(path[clear], xp[clear])
    g.close()
