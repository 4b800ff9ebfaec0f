"""psmc_hip_post_quantile (include/psmc_hip.h): per bin the state at up to four posterior quantiles, on the device, from every kind
of table the decoding entry points read (api_decode.hip):  state = min(n-1, #{k < n : c_k < q c_{n-1}}) over the running sums c of
the posterior row.

Checks (no bound is measured):
  (Q1) exact sources: bit identity with the sequential numpy loop over the rows psmc_hip_posterior returns on the same context --
       c = post[:, 0]; c = c + post[:, k] (one add per step, the first term as it is), x = q * c_{n-1},
       (c < x[:, None]).sum(1) clipped to n-1 -- at q = (0, 0.025, 0.5, 1): both ends pinned.  Every state at n = 1 is 0.
  (Q2) fast and wide fast sources against their own rows: with C the np.longdouble sequential cdf of psmc_hip_posterior's rows of
       the same context (C_{-1} = -inf) the returned state i satisfies (i == 0 or C_{i-1} < q + d) and (i == n-1 or C_i >= q - d),
       d = 2 (n + 8) 2^-52 (the header derives it from _post_mean's bound).
  (Q3) the same against the rows of an exact context with the same parameters, d = 1e-9 n.
  Condition of (Q3): on every case at most 1 % of the (bin, q) pairs have more than one acceptable state under (Q3), computed from
  the exact context's rows alone and asserted -- so the slack cannot hide a failure.  q = (0.025, 0.25, 0.5, 0.975) meets it on
  every case with the CPU oracle's rows (tests/orc.py: at most 4e-5 up to 128 states, 0 at 150..300, 0.0014 at 769 and 0.0020 at
  1024 states); Q_OF would hold a case's own q if one did not.  No q of 0 or 1
  here: the cdf saturates there and almost every state is acceptable.
  CKPT results are bit-equal to the full table's.  Columns: n_q = 4 equals four calls with n_q = 1, bit for bit, on every source.
The slack used -- how far beyond q the cdf at the returned state's neighbours lies, max(C_{i-1} - q, q - C_i, 0), as a fraction of
d -- is printed per case, and written to the file PSMC_POST_QUANTILE_REPORT names when set (profiles/post_quantile.txt).

Observed on the MI355X: every bit comparison holds; the slack used is 0 under (Q2) and (Q3) on all 36 cases -- every returned state
is the quantile of the reference cdf itself; the share of pairs with a choice under (Q3) is what the CPU oracle gave (at most
0.0020, at 1024 states); the file's 53 cases and the 9 GPU cases of tests/test_host_cli_band.py take 29 s together."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from test_gpu_post_mean import (CASES, CK, FAST_CASES, SMALL_TILES, WIDE_CASES, _capped, _n128, exact_ctx, par_of, random_hmm,  # noqa: F401
                                ran_wide, short_segs, wide_ctx)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_PIN = np.array([0.0, 0.025, 0.5, 1.0])
Q_TOL = np.array([0.025, 0.25, 0.5, 0.975])
Q_OF = {}       # case -> its own q, where Q_TOL left more than 1 % of the pairs with two acceptable states (none does)
AMBIGUOUS_CAP = 0.01
WORST = {}      # case -> [slack / d of (Q2), slack / d of (Q3), share of pairs with more than one acceptable state under (Q3)]
_EXACT = {}


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
    lines = ["%-44s (Q2) %.3f  (Q3) %.3e  ambiguous under (Q3) %.4f" % (k, v[0], v[1], v[2]) for k, v in sorted(WORST.items())]
    print("\nworst slack used, as a fraction of d, and the share of (bin, q) pairs with more than one acceptable state:\n" + "\n".join(lines))
    if os.environ.get("PSMC_POST_QUANTILE_REPORT"):
        with open(os.environ["PSMC_POST_QUANTILE_REPORT"], "w") as f:
            f.write("\n".join(lines) + "\n")


def loop_count(post, q):
    """(Q1)'s reference: the running sums in state order, one rounding per sum, one per threshold"""
    c = post[:, 0].copy()
    cs = [c]
    for k in range(1, post.shape[1]):
        c = c + post[:, k]
        cs.append(c)
    cs = np.stack(cs, axis=1)
    out = np.empty((post.shape[0], len(q)), dtype=np.int32)
    for j, qj in enumerate(q):
        x = qj * cs[:, -1]
        out[:, j] = np.minimum((cs < x[:, None]).sum(1), post.shape[1] - 1)
    return out


def cdf(post):
    return np.cumsum(post.astype(np.longdouble), axis=1)   # sequential, in state order


def slack(state, Cd, q, d):
    """per (bin, column): whether the state is acceptable at slack d, and the slack it needs: max(C_{i-1} - q, q - C_i, 0)"""
    L, n = Cd.shape
    rows = np.arange(L)[:, None]
    below = np.where(state > 0, Cd[rows, np.maximum(state - 1, 0)], -np.inf)          # C_{i-1}
    here = np.where(state < n - 1, Cd[rows, state], np.inf)                            # C_i (no condition at n-1)
    ql = q.astype(np.longdouble)[None, :]
    ok = (below < ql + d) & (here >= ql - d)
    need = np.maximum(np.maximum(below - ql, ql - here), 0.0)
    return ok, need.astype(np.float64)


def ambiguous_share(Cd, q, d):
    """the share of (bin, q) pairs with more than one acceptable state: i is acceptable iff (i == 0 or C_{i-1} < q + d) and
    (i == n-1 or C_i >= q - d)"""
    L, n = Cd.shape
    many = 0
    for qj in q.astype(np.longdouble):
        lo = np.concatenate([np.ones((L, 1), bool), Cd[:, :-1] < qj + d], axis=1)
        hi = np.concatenate([Cd[:, :-1] >= qj - d, np.ones((L, 1), bool)], axis=1)
        many += int(((lo & hi).sum(1) > 1).sum())
    return many / float(L * len(q))


def quants(es, seg, q):
    """the call with all columns and the calls with one column each; asserts what holds on every source -- a column does not depend
    on how many are asked for"""
    got = es.post_quantile(seg, q)
    L = int(es.lens[seg])
    assert got.shape == (L, len(q)) and got.dtype == np.int32
    single = np.concatenate([es.post_quantile(seg, q[j]) for j in range(len(q))], axis=1)
    assert np.array_equal(got, single), seg
    assert np.array_equal(es.post_quantile(seg, q[:3]), got[:, :3]), seg
    return got


def segs_q1(golden):
    s = short_segs(golden)
    return s + [s[-1][:1]]   # and one more segment of a single bin, last


def check_exact(es, n_seg, n, what):
    """(Q1) on every segment"""
    for seg in range(n_seg):
        post, _ = es.posterior(seg, want_recomb=False)
        got = quants(es, seg, Q_PIN)
        assert np.array_equal(got, loop_count(post, Q_PIN)), (what, seg)
        assert (got[:, 0] == 0).all() and (got >= 0).all() and (got <= n - 1).all()
        if n == 1:
            assert not got.any()


def check_fast(es, exact, n_seg, n, what):
    """(Q2) against the context's own rows, (Q3) against the exact context's, and (Q3)'s condition"""
    q = Q_OF.get(what, Q_TOL)
    d2, d3 = 2.0 * (n + 8) * 2.0 ** -52, 1e-9 * n
    worst = WORST.setdefault(what, [0.0, 0.0, 0.0])
    many, pairs, out = 0.0, 0, []
    for seg in range(n_seg):
        got = quants(es, seg, q)
        out.append(got)
        assert (got >= 0).all() and (got <= n - 1).all()
        own, ref = cdf(es.posterior(seg, want_recomb=False)[0]), cdf(exact.posterior(seg, want_recomb=False)[0])
        ok2, need2 = slack(got, own, q, d2)
        ok3, need3 = slack(got, ref, q, d3)
        worst[0] = max(worst[0], float(need2.max()) / d2); worst[1] = max(worst[1], float(need3.max()) / d3)
        many += ambiguous_share(ref, q, d3) * got.size; pairs += got.size
        print("%s segment %d: slack used (Q2) %.3e of %.3e, (Q3) %.3e of %.3e" % (what, seg, need2.max(), d2, need3.max(), d3))
        assert ok2.all(), (what, seg, np.argwhere(~ok2)[:5])
        assert ok3.all(), (what, seg, np.argwhere(~ok3)[:5])
    worst[2] = max(worst[2], many / pairs)
    print("%s: %.4f of the (bin, q) pairs have more than one acceptable state under (Q3)" % (what, many / pairs))
    assert many / pairs <= AMBIGUOUS_CAP, (what, many / pairs)
    return out


# ------------------------------------------------------------------ 1. exact tables, up to 128 states
@pytest.mark.parametrize("n", [1, 2, 23, 64, 65, 127, 128])
def test_post_quantile_exact(hip, golden, n):
    segs = segs_q1(golden)
    es = exact_ctx(hip, n, segs, random_hmm(np.random.default_rng(n), n))
    check_exact(es, len(segs), n, "exact %d" % n)
    es.close()


# ------------------------------------------------------------------ 2. exact tables beyond 128 states, and the exact fallback
@pytest.mark.parametrize("n", [129, 200, 257, 1024])
def test_post_quantile_exact_wide(hip, golden, n):
    segs = segs_q1(golden)
    es = exact_ctx(hip, n, segs, random_hmm(np.random.default_rng(n), n))
    check_exact(es, len(segs), n, "exact %d" % n)
    es.close()


def test_post_quantile_exact_fallback(hip, golden):
    """128 states in fast mode and a matrix without the PSMC form: the E-step ran the exact kernels, and so does post_quantile"""
    a, e, a0 = _n128(golden)
    segs = segs_q1(golden)
    es = hip.HipEStep(128, mode=hip.MODE_FAST)
    es.load_segments(segs)
    r = es.estep(_capped(a, 90), e, a0)
    assert not es.fast_diag()["structured"] and r["A0"].any()   # the exact kernels ran (test_gpu_post_mean.py)
    check_exact(es, len(segs), 128, "fast mode, exact fallback")
    es.close()


# ------------------------------------------------------------------ 3. fast tables up to 128 states
@pytest.mark.parametrize("case", sorted(FAST_CASES))
def test_post_quantile_fast(hip, golden, case):
    n, segs, par, opts = FAST_CASES[case](golden)
    fast = hip.HipEStep(n, mode=hip.MODE_FAST, **opts)
    fast.load_segments(segs)
    fast.estep(*par)
    assert fast.fast_diag()["back_half"] == 0   # the back half that keeps bt ran: the fast tables are what is read
    exact = exact_ctx(hip, n, segs, par)
    check_fast(fast, exact, len(segs), n, "fast " + case)
    fast.close(); exact.close()


# ------------------------------------------------------------------ 4. wide fast tables, full and checkpoints
def exact_short(hip, golden, n):
    """the exact context of par_of(n) on short_segs after its E-step: made once per size and only read afterwards"""
    if n not in _EXACT:
        _EXACT[n] = exact_ctx(hip, n, short_segs(golden), par_of(n))
    return _EXACT[n]


@pytest.mark.parametrize("n,opts", WIDE_CASES, ids=["%d-%s" % (n, "-".join("%s%d" % kv for kv in o.items()) or "default") for n, o in WIDE_CASES])
def test_post_quantile_wide_fast(hip, golden, n, opts):
    a, e, a0 = par_of(n)
    segs = short_segs(golden)
    exact = exact_short(hip, golden, n)
    what = "wide fast %d %s" % (n, opts or "default")
    full = wide_ctx(hip, n, segs, **opts)
    full.estep_factored(a, e[:2], a0)
    assert not ran_wide(full)["ckpt"] and full.wide_table_info()["interval"] == 1
    want = check_fast(full, exact, len(segs), n, what)
    ck = wide_ctx(hip, n, segs, **CK, **opts)
    ck.estep_factored(a, e[:2], a0)
    assert ran_wide(ck)["ckpt"] and ck.wide_table_info()["interval"] == 8
    q = Q_OF.get(what, Q_TOL)
    for seg in range(len(segs)):
        assert np.array_equal(quants(ck, seg, q), want[seg]), seg        # from checkpoints: the bits of the full table
        assert np.array_equal(ck.post_quantile(seg, Q_PIN), full.post_quantile(seg, Q_PIN)), seg
    full.close(); ck.close()


# ------------------------------------------------------------------ 5. state rules
def test_post_quantile_state_rules(hip, golden):
    g = golden.params("n64_curve")
    a, e, a0 = g["a"], g["e"], g["a0"]
    segs = golden.segs_small
    for mode in (hip.MODE_EXACT, hip.MODE_FAST):   # before any E-step
        es = hip.HipEStep(64, mode=mode)
        es.load_segments(segs)
        with pytest.raises(hip.HipError, match="call order violated"):
            es.post_quantile(0, Q_TOL)
        es.close()
    es = hip.HipEStep(64, mode=hip.MODE_FAST)
    es.load_segments(segs)
    es.estep(a, e, a0)                              # the fused back half (default): no bt
    assert es.fast_diag()["back_half"] == 1
    with pytest.raises(hip.HipError, match="call order violated.*fuse=0"):
        es.post_quantile(0, Q_TOL)
    es.set_option("fuse", 0)
    es.estep(a, e, a0)
    es.post_quantile(0, Q_TOL)                      # now there is something to read ...
    es.estep_batch([(a, e, a0)] * 2, [[0, 1], [2, 3]])   # ... and a batch takes the tables
    with pytest.raises(hip.HipError, match="call order violated"):
        es.post_quantile(0, Q_TOL)
    es.estep(a, e, a0)
    # arguments: checked before the state
    lib = es.lib
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.psmc_hip_post_quantile.argtypes = [C.c_void_p, C.c_int, dp, C.c_int32, ip]
    out = np.zeros((len(segs[0]), 5), dtype=np.int32)
    q5 = np.array([0.1, 0.2, 0.3, 0.4, 0.5])
    call = lambda seg, q, n_q, o=out: lib.psmc_hip_post_quantile(es.h, seg, None if q is None else q.ctypes.data_as(dp), n_q, None if o is None else o.ctypes.data_as(ip))
    EINVAL = -1
    assert call(0, q5, 0) == EINVAL and call(0, q5, 5) == EINVAL and call(0, q5, -1) == EINVAL
    assert call(0, None, 1) == EINVAL and call(0, q5, 1, None) == EINVAL
    assert call(len(segs), q5, 1) == EINVAL and call(-1, q5, 1) == EINVAL
    for bad in (np.nan, -1e-300, 1.0 + 2.0 ** -52, np.inf, -np.inf, 2.0):
        for at in range(4):
            qb = q5.copy(); qb[at] = bad
            assert call(0, qb, 4) == EINVAL, (bad, at)
        qb = q5.copy(); qb[3] = bad
        assert call(0, qb, 3) == 0                  # a column that is not asked for is not read
    out[:] = 0
    qb = q5.copy(); qb[0] = np.nan
    assert call(0, qb, 4) == EINVAL and not out.any()
    assert call(0, q5, 4) == 0
    assert call(0, np.array([0.0, 1.0, -0.0, 0.5]), 4) == 0   # the ends are allowed
    es.close()


@pytest.mark.parametrize("kind", ["exact64", "fast64", "wide300"])
def test_post_quantile_has_no_side_effects(hip, golden, kind):
    """Two contexts with the same call history: the second E-step returns the same bits whether or not post_quantile ran in between."""
    from conftest import bits_equal
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
    for c in ctx:
        step(c)
    first = [ctx[1].post_quantile(seg, Q_TOL) for seg in range(len(segs))]
    again = [ctx[1].post_quantile(seg, Q_TOL) for seg in range(len(segs))]
    assert all(np.array_equal(x, y) for x, y in zip(first, again))   # the tables and q alone decide
    r = [step(c) for c in ctx]
    assert all(bits_equal(r[0][k], r[1][k]) for k in keys) and r[0]["LL"] == r[1]["LL"]
    for c in ctx:
        c.close()


# ------------------------------------------------------------------ 6. a group of two shards on one device
def test_post_quantile_group(hip, golden):
    g64 = golden.params("n64_curve")
    par = (g64["a"], g64["e"], g64["a0"])
    segs = short_segs(golden)
    single = exact_ctx(hip, 64, segs, par)
    g = hip.HipGroup(64, [0, 0], mode=hip.MODE_EXACT)
    g.load_segments(segs)
    g.estep(*par)
    assert g.info()["n_shards"] == 2
    lib = g.lib
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.psmc_hip_group_route.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    lib.psmc_hip_post_quantile.argtypes = [C.c_void_p, C.c_int, dp, C.c_int32, ip]
    for seg in range(len(segs)):
        ctx, local = C.c_void_p(), C.c_int(-1)
        assert lib.psmc_hip_group_route(g.g, seg, C.byref(ctx), C.byref(local)) == 0
        out = np.full((len(segs[seg]), 4), -1, dtype=np.int32)
        assert lib.psmc_hip_post_quantile(ctx, local.value, Q_PIN.ctypes.data_as(dp), 4, out.ctypes.data_as(ip)) == 0
        assert np.array_equal(out, single.post_quantile(seg, Q_PIN)), seg
    g.close(); single.close()
