"""psmc_hip_post_mean (include/psmc_hip.h): per-bin posterior expectations mean[u][j] = sum_k gamma_u(k) w[j][k] on the device,
from every kind of table the decoding entry points read (api_decode.hip).

Weights, four columns at every size: 0.1 (exp(k/n ln 151) - 1) + 1e-3 (a time axis), its square, the indicator k >= n/2, and
standard normal draws with mixed signs, none zero.  Calls are made with n_w = 1, 3 and 4.

Bounds (none of them measured):
  (B1) exact sources: bit identity with  m = post[:,0]*w[j,0]; for k in 1..n-1: m = m + post[:,k]*w[j,k]  over the rows
       psmc_hip_posterior returns on the same context (numpy does not fuse the multiply and the add).
  (B2) fast and wide fast sources against their own rows: |mean - ref| <= (n + 8) 2^-52 max_k |w_jk|, ref the np.longdouble sum over
       psmc_hip_posterior's rows of the same context -- the first-order bound for n products added in any order plus the roundings of
       the normalisation, doubled (the posterior sums to one).
  (B3) fast and wide fast against an exact context with the same parameters: |delta| <= 1e-9 sum_k |w_jk| (the header's posterior
       tolerance, 1e-9 absolute per state).
Columns: the result for n_w = 4 equals, column by column and bit for bit, four calls with n_w = 1 -- on every source.
The worst observed fraction of (B2) and (B3) per case is printed, and written to the file PSMC_POST_MEAN_REPORT names when set
(profiles/post_mean.txt).

Observed on the MI355X: every bit comparison holds; (B2) at most 0.036 of its bound (23 states, fast tables), (B3) at most 5e-5 of
its bound on the fast tables and 1.2e-7 on the wide fast ones; the file's 53 cases and the 11 GPU cases of
tests/test_host_cli_tmrca.py take 31 s together."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal
from test_gpu_estep import random_hmm
from test_gpu_fast_decode import CASES, _capped, _n128
from test_gpu_wide_fast import ran_wide
from test_gpu_wide_fast_mw import short_segs
from test_gpu_wide_fast_ckpt import par_of
from test_gpu_wide_fast_ckpt_decode import SMALL_TILES, CK
from test_gpu_wide_fast_mw_decode import exact_ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_W = (1, 3, 4)
WORST = {}    # case -> [largest |mean - ref| / (B2), largest |delta| / (B3)]


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for ex in _EXACT.values():
        ex.close()
    _EXACT.clear()
    lines = ["%-44s (B2) %.3f  (B3) %.3e" % (k, v[0], v[1]) for k, v in sorted(WORST.items())]
    print("\nworst observed, as a fraction of the bound:\n" + "\n".join(lines))
    if os.environ.get("PSMC_POST_MEAN_REPORT"):
        with open(os.environ["PSMC_POST_MEAN_REPORT"], "w") as f:
            f.write("\n".join(lines) + "\n")


def weights(n):
    k = np.arange(n, dtype=np.float64)
    w0 = 0.1 * (np.exp(k / n * np.log(151.0)) - 1.0) + 1e-3
    w3 = np.random.default_rng(100 + n).standard_normal(n)
    w3[w3 == 0.0] = 0.5
    w3[0] = -abs(w3[0])
    if n > 1:
        w3[1] = abs(w3[1])
    return np.ascontiguousarray(np.stack([w0, w0 * w0, (k >= n / 2).astype(np.float64), w3]))


def loop_sum(post, w):
    """(B1)'s reference: state order, the first term taken as it is, one rounding per product and per sum"""
    out = np.empty((post.shape[0], w.shape[0]))
    for j in range(w.shape[0]):
        m = post[:, 0] * w[j, 0]
        for k in range(1, post.shape[1]):
            m = m + post[:, k] * w[j, k]
        out[:, j] = m
    return out


def means(es, seg, W):
    """the calls with 1, 3 and 4 columns, and the four calls with one column each: a dict n_w -> (L, n_w), 'single' -> (L, 4);
    asserts what holds on every source -- the columns do not depend on how many are asked for"""
    got = {nw: es.post_mean(seg, W[:nw]) for nw in N_W}
    got["single"] = np.concatenate([es.post_mean(seg, W[j]) for j in range(4)], axis=1)
    L = int(es.lens[seg])
    for nw in N_W:
        assert got[nw].shape == (L, nw)
        assert bits_equal(got[nw], got["single"][:, :nw]), (seg, nw)
    return got


def check_exact(es, n_seg, n, what):
    """(B1) on every segment"""
    W = weights(n)
    for seg in range(n_seg):
        post, _ = es.posterior(seg, want_recomb=False)
        got = means(es, seg, W)
        assert bits_equal(got[4], loop_sum(post, W)), (what, seg)


def check_fast(es, exact, n_seg, n, what):
    """(B2) against the context's own rows, (B3) against the exact context"""
    W = weights(n)
    wl = W.astype(np.longdouble)
    b2 = (n + 8) * 2.0 ** -52 * np.abs(W).max(1)
    b3 = 1e-9 * np.abs(W).sum(1)
    worst = WORST.setdefault(what, [0.0, 0.0])
    for seg in range(n_seg):
        post, _ = es.posterior(seg, want_recomb=False)
        got = means(es, seg, W)[4]
        ref = np.stack([(post.astype(np.longdouble) * wl[j]).sum(1) for j in range(4)], axis=1)
        d2 = np.abs(got.astype(np.longdouble) - ref).max(0).astype(np.float64)
        d3 = np.abs(got - exact.post_mean(seg, W)).max(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst[0] = max(worst[0], float(np.nanmax(np.where(b2 > 0, d2 / b2, 0.0))))
            worst[1] = max(worst[1], float(np.nanmax(np.where(b3 > 0, d3 / b3, 0.0))))
        print("%s segment %d: (B2) %s of %s, (B3) %s of %s" % (what, seg, d2, b2, d3, b3))
        assert np.isfinite(got).all() and (d2 <= b2).all(), (what, seg, d2, b2)
        assert (d3 <= b3).all(), (what, seg, d3, b3)
    return got


# ------------------------------------------------------------------ 1. exact tables, up to 128 states
@pytest.mark.parametrize("n", [1, 2, 23, 64, 65, 127, 128])
def test_post_mean_exact(hip, golden, n):
    segs = short_segs(golden)
    es = exact_ctx(hip, n, segs, random_hmm(np.random.default_rng(n), n))
    check_exact(es, len(segs), n, "exact %d" % n)
    es.close()


# ------------------------------------------------------------------ 2. exact tables beyond 128 states, and the exact fallback
@pytest.mark.parametrize("n", [129, 200, 257, 1024])
def test_post_mean_exact_wide(hip, golden, n):
    segs = short_segs(golden)
    es = exact_ctx(hip, n, segs, random_hmm(np.random.default_rng(n), n))
    check_exact(es, len(segs), n, "exact %d" % n)
    es.close()


def test_post_mean_exact_fallback(hip, golden):
    """128 states in fast mode and a matrix without the PSMC form: the E-step ran the exact kernels, and so does post_mean"""
    a, e, a0 = _n128(golden)
    segs = short_segs(golden)
    es = hip.HipEStep(128, mode=hip.MODE_FAST)
    es.load_segments(segs)
    r = es.estep(_capped(a, 90), e, a0)
    # the path that ran: no structured sweeps (and 128 states have no dense fast ones), and the exact kernels' own A0 -- a fast-mode
    # E-step returns zeros there
    assert not es.fast_diag()["structured"] and r["A0"].any()
    x = exact_ctx(hip, 128, segs, (_capped(a, 90), e, a0))
    assert all(bits_equal(es.tables(seg)[k], x.tables(seg)[k]) for seg in (7, 16) for k in range(3))   # f, b, s are the exact tables
    x.close()
    check_exact(es, len(segs), 128, "fast mode, exact fallback")
    es.close()


# ------------------------------------------------------------------ 3. fast tables up to 128 states
def _n23(g):
    p = g.params("n23_curve")
    return p["a"].shape[0], g.segs_small + g.segs_mid[2:4], (p["a"], p["e"], p["a0"]), dict(fuse=0, chunk=257, warmup=300)


FAST_CASES = dict(CASES, n23_short_tiles=_n23)   # every case of tests/test_gpu_fast_decode.py, and 23 states


@pytest.mark.parametrize("case", sorted(FAST_CASES))
def test_post_mean_fast(hip, golden, case):
    n, segs, par, opts = FAST_CASES[case](golden)
    fast = hip.HipEStep(n, mode=hip.MODE_FAST, **opts)
    fast.load_segments(segs)
    fast.estep(*par)
    d = fast.fast_diag()
    assert d["back_half"] == 0   # the back half that keeps bt ran: the fast tables are what is read
    if "chunk" in opts:          # several tiles per segment, the last one not full
        assert any(len(s) > 2 * opts["chunk"] and len(s) % opts["chunk"] for s in segs)
    exact = exact_ctx(hip, n, segs, par)
    check_fast(fast, exact, len(segs), n, "fast " + case)
    fast.close(); exact.close()


# ------------------------------------------------------------------ 4. wide fast tables, full and checkpoints
WIDE_CASES = [(n, o) for n in (150, 300) for o in SMALL_TILES + [dict()]] + [(n, o) for n in (200, 257, 769, 1024) for o in (dict(), dict(chunk=37, warmup=5))]
_EXACT = {}


def exact_short(hip, golden, n):
    """the exact context of par_of(n) on short_segs after its E-step: made once per size and only read afterwards"""
    if n not in _EXACT:
        _EXACT[n] = exact_ctx(hip, n, short_segs(golden), par_of(n))
    return _EXACT[n]


def wide_ctx(hip, n, segs, **opts):
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=2, wide_decode=1, **opts)
    es.load_segments(segs)
    return es


@pytest.mark.parametrize("n,opts", WIDE_CASES, ids=["%d-%s" % (n, "-".join("%s%d" % kv for kv in o.items()) or "default") for n, o in WIDE_CASES])
def test_post_mean_wide_fast(hip, golden, n, opts):
    a, e, a0 = par_of(n)
    segs = short_segs(golden)
    exact = exact_short(hip, golden, n)
    W = weights(n)
    full = wide_ctx(hip, n, segs, **opts)
    full.estep_factored(a, e[:2], a0)
    assert not ran_wide(full)["ckpt"] and full.wide_table_info()["interval"] == 1
    check_fast(full, exact, len(segs), n, "wide fast %d %s" % (n, opts or "default"))
    ck = wide_ctx(hip, n, segs, **CK, **opts)
    ck.estep_factored(a, e[:2], a0)
    assert ran_wide(ck)["ckpt"] and ck.wide_table_info()["interval"] == 8
    for seg in range(len(segs)):
        want, got = means(full, seg, W), means(ck, seg, W)
        for k in want:
            assert bits_equal(got[k], want[k]), (seg, k)
    full.close(); ck.close()


# ------------------------------------------------------------------ 6. state rules
def test_post_mean_state_rules(hip, golden):
    g = golden.params("n64_curve")
    a, e, a0 = g["a"], g["e"], g["a0"]
    segs = golden.segs_small
    W = weights(64)
    for mode in (hip.MODE_EXACT, hip.MODE_FAST):   # before any E-step
        es = hip.HipEStep(64, mode=mode)
        es.load_segments(segs)
        with pytest.raises(hip.HipError, match="call order violated"):
            es.post_mean(0, W)
        es.close()
    es = hip.HipEStep(64, mode=hip.MODE_FAST)
    es.load_segments(segs)
    es.estep(a, e, a0)                              # the fused back half (default): no bt
    assert es.fast_diag()["back_half"] == 1
    with pytest.raises(hip.HipError, match="call order violated.*fuse=0"):
        es.post_mean(0, W)
    es.set_option("fuse", 0)
    es.estep(a, e, a0)
    es.post_mean(0, W)                              # now there is something to read ...
    es.estep_batch([(a, e, a0)] * 2, [[0, 1], [2, 3]])   # ... and a batch takes the tables
    with pytest.raises(hip.HipError, match="call order violated"):
        es.post_mean(0, W)
    es.estep(a, e, a0)
    # arguments: checked before the state
    lib = es.lib
    dp = C.POINTER(C.c_double)
    lib.psmc_hip_post_mean.argtypes = [C.c_void_p, C.c_int, dp, C.c_int32, dp]
    out = np.zeros((len(segs[0]), 5))
    w5 = np.ascontiguousarray(np.concatenate([W, W[:1]]))
    EINVAL = -1
    assert lib.psmc_hip_post_mean(es.h, 0, w5.ctypes.data_as(dp), 0, out.ctypes.data_as(dp)) == EINVAL
    assert lib.psmc_hip_post_mean(es.h, 0, w5.ctypes.data_as(dp), 5, out.ctypes.data_as(dp)) == EINVAL
    assert lib.psmc_hip_post_mean(es.h, 0, None, 1, out.ctypes.data_as(dp)) == EINVAL
    assert lib.psmc_hip_post_mean(es.h, 0, w5.ctypes.data_as(dp), 1, None) == EINVAL
    assert lib.psmc_hip_post_mean(es.h, len(segs), w5.ctypes.data_as(dp), 1, out.ctypes.data_as(dp)) == EINVAL
    assert not out.any()
    assert lib.psmc_hip_post_mean(es.h, 0, w5.ctypes.data_as(dp), 4, out.ctypes.data_as(dp)) == 0
    es.close()


@pytest.mark.parametrize("kind", ["exact64", "fast64", "wide300"])
def test_post_mean_has_no_side_effects(hip, golden, kind):
    """Two contexts with the same call history: the second E-step returns the same bits whether or not post_mean ran in between."""
    segs = short_segs(golden)
    if kind == "wide300":
        a, e, a0 = par_of(300)
        ctx = [wide_ctx(hip, 300, segs, chunk=37, warmup=5) for _ in range(2)]
        step = lambda c: c.estep_factored(a, e[:2], a0)
        keys = ("sums", "E")
    else:
        g = golden.params("n64_curve")
        a, e, a0 = g["a"], g["e"], g["a0"]
        ctx = [hip.HipEStep(64, mode=hip.MODE_EXACT) if kind == "exact64" else hip.HipEStep(64, mode=hip.MODE_FAST, fuse=0, chunk=256, warmup=128) for _ in range(2)]
        for c in ctx:
            c.load_segments(segs)
        step = lambda c: c.estep(a, e, a0)
        keys = ("A", "E")
    W = weights(ctx[0].n)
    for c in ctx:
        step(c)
    for seg in range(len(segs)):
        ctx[1].post_mean(seg, W)
    r = [step(c) for c in ctx]
    assert all(bits_equal(r[0][k], r[1][k]) for k in keys) and r[0]["LL"] == r[1]["LL"]
    for c in ctx:
        c.close()


# ------------------------------------------------------------------ 7. a group of two shards on one device
def test_post_mean_group(hip, golden):
    g64 = golden.params("n64_curve")
    par = (g64["a"], g64["e"], g64["a0"])
    segs = short_segs(golden)
    W = weights(64)
    single = exact_ctx(hip, 64, segs, par)
    g = hip.HipGroup(64, [0, 0], mode=hip.MODE_EXACT)
    g.load_segments(segs)
    g.estep(*par)
    assert g.info()["n_shards"] == 2
    lib = g.lib
    dp = C.POINTER(C.c_double)
    lib.psmc_hip_group_route.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    lib.psmc_hip_post_mean.argtypes = [C.c_void_p, C.c_int, dp, C.c_int32, dp]
    for seg in range(len(segs)):
        ctx, local = C.c_void_p(), C.c_int(-1)
        assert lib.psmc_hip_group_route(g.g, seg, C.byref(ctx), C.byref(local)) == 0
        out = np.zeros((len(segs[seg]), 4))
        assert lib.psmc_hip_post_mean(ctx, local.value, W.ctypes.data_as(dp), 4, out.ctypes.data_as(dp)) == 0
        assert bits_equal(out, single.post_mean(seg, W)), seg
    g.close(); single.close()
