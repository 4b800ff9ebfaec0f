"""The bootstrap batch on the wide fast path: psmc_hip_estep_batch with the option "wide_batch" = 1 on a fast-mode context of
129 .. 1024 states whose size "wide_fast" covers (psmc_amd/csrc/api_batch.hip batch_wide).  The wide path learns nothing between
E-steps, so the batch is the single factored E-step run once per replicate on the context itself: every replicate must have the
BITS of psmc_hip_select + psmc_hip_estep_factored on a fresh context with the same options, and everything around it -- the
selection, the decoding state, the diagnostics, the fallbacks, every call the option does not cover -- is pinned here.

Inputs: short_segs of tests/test_gpu_wide_fast_mw.py (1661 bins in 17 segments of 1 .. 1000 bins); four replicates, each with the
host model's parameters from its own seed, over the multisets SELS (all segments; repeats; the one-bin segment alone; a segment
three times).  References: a fresh context (bits), an exact-mode context's batch on the same device through the gates of
tests/test_gpu_wide_fast.py (statistics 1e-10 of the largest cell, LL 1e-12 relative, per vector cell 1e-9 / L1 1e-10 / QA, QE
1e-10), and at 300 states the CPU oracle."""
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal
from test_gpu_wide_fast import check, ran_wide, tri_sums, psmc_params
from test_gpu_wide_fast_mw import short_segs, SIZES as MW_SIZES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# states -> (pattern, free lambdas, "wide_fast"): both sides of every padding step and the ends of each kernel family, and the two
# sizes (200, 300) the state, fallback and option tests use
SIZES = {129: ("129*1", 129, 1), 192: ("192*1", 192, 1), 193: ("193*1", 193, 1), 200: ("100*2", 100, 1), 256: ("128*2", 128, 1)}
for _n in (257, 300, 512, 513, 1024):
    SIZES[_n] = MW_SIZES[_n] + (2,)
T_DEFAULT, T_REPAIR, T_NOWARM, T_ROUNDS = dict(), dict(chunk=37, warmup=5), dict(chunk=64, warmup=0), dict(chunk=100, warmup=30, learn=0)
CASES = [(n, t) for n in sorted(SIZES) for t in (T_DEFAULT, T_REPAIR, T_NOWARM)] + [(n, T_ROUNDS) for n in (200, 300)]
N_REP = 4
MSG_EXACT = "repeating this E-step with the exact kernels"


def sels(n_seg):
    return [list(range(n_seg)), [7, 7, 3], [0], [16, 16, 16, 2, 5, 5]]


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


def rep_params(n):
    """the parameters of the four replicates: the host model of the size's pattern, lambdas from the replicate's own seed"""
    pat, m, _ = SIZES[n]
    return [psmc_params(pat, m, np.random.default_rng(7000 + 10 * n + r)) for r in range(N_REP)]


def wide_ctx(hip, n, segs, wide_batch=1, **opts):
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=SIZES[n][2], wide_batch=wide_batch, **opts)
    es.load_segments(segs)
    return es


def row(b, r):
    return dict(sums=b["sums"][r], E=b["E"][r], LL=float(b["LL"][r]))


def same_bits(r, w):
    return bits_equal(r["sums"], w["sums"]) and bits_equal(r["E"], w["E"]) and r["LL"] == w["LL"]


def fresh_single(hip, n, segs, par, sel, **opts):
    """select(sel) + estep_factored on a context of its own (without "wide_batch": a single E-step never reads it)"""
    es = wide_ctx(hip, n, segs, wide_batch=0, **opts)
    es.select(sel)
    r = es.estep_factored(par[0], par[1][:2], par[2])
    ran_wide(es)
    es.close()
    return r


_BATCH, _EXACT = {}, {}


def wide_batch(hip, golden, n, opts):
    """the wide batch of the four replicates at (n, tiling), run once: its rows, the callback's record and the diagnostics after it"""
    key = (n, tuple(sorted(opts.items())))
    if key not in _BATCH:
        segs = short_segs(golden)
        es = wide_ctx(hip, n, segs, **opts)
        calls = []
        b = es.estep_batch(rep_params(n), sels(len(segs)), want="sums", on_done=lambda reps, out: calls.append(list(reps)))
        _BATCH[key] = dict(b=b, calls=calls, info=es.batch_info(), diag=ran_wide(es))
        es.close()
    return _BATCH[key]


def exact_batch(hip, golden, n):
    """an exact-mode context's batch over the same replicates (A, its sums, E, LL), once per size"""
    if n not in _EXACT:
        segs = short_segs(golden)
        ex = hip.HipEStep(n, mode=hip.MODE_EXACT)
        ex.load_segments(segs)
        _EXACT[n] = ex.estep_batch(rep_params(n), sels(len(segs)), want="both")
        ex.close()
    return _EXACT[n]


# ------------------------------------------------------------------ 1. bits
@pytest.mark.parametrize("n,opts", CASES)
def test_wide_batch_bits(hip, golden, n, opts):
    """Every replicate's sums, E and LL are, bit for bit, what a FRESH context with the same options gives for select(idx_r) +
    estep_factored with that replicate's parameters (a mix-up of parameters or selections between replicates shows here); the
    callback named 0, 1, 2, 3 once each, in order; batch_info is {4, 0}; the diagnostics are the wide path's."""
    segs = short_segs(golden)
    w = wide_batch(hip, golden, n, opts)
    pars, ss = rep_params(n), sels(len(segs))
    for r in range(N_REP):
        f = fresh_single(hip, n, segs, pars[r], ss[r], **opts)
        assert same_bits(row(w["b"], r), f), (n, opts, r)
    assert w["calls"] == [[0], [1], [2], [3]], w["calls"]
    assert w["info"] == dict(groups=N_REP, replicate_contexts=0), w["info"]
    if opts.get("chunk") == 37:   # (the diagnostics describe the last replicate: six segments in tiles of 37 bins, warm-up 5)
        assert w["diag"]["fwd_rounds"] + w["diag"]["bwd_rounds"] > 0, w["diag"]


# ------------------------------------------------------------------ 2. against the exact kernels
@pytest.mark.parametrize("n,opts", CASES)
def test_wide_batch_vs_exact(hip, golden, n, opts):
    """Every replicate against an exact-mode context's batch over the same replicates: tri_sums(A), E, LL through the gates of
    tests/test_gpu_wide_fast.py, and the invariants on the replicate's own multiset."""
    segs = short_segs(golden)
    w, x = wide_batch(hip, golden, n, opts), exact_batch(hip, golden, n)
    pars, ss = rep_params(n), sels(len(segs))
    for r in range(N_REP):
        check(row(w["b"], r), tri_sums(x["A"][r]), x["E"][r], float(x["LL"][r]), ("wide batch", n, opts, r),
              (pars[r][0], pars[r][1]), [segs[i] for i in ss[r]])


def test_wide_batch_vs_oracle_300(hip, golden, oracle):
    """One reference that is not this library: replicate 3 (a segment three times, another twice) at 300 states against the CPU oracle."""
    segs = short_segs(golden)
    r = 3
    a, e, a0 = rep_params(300)[r]
    ms = [segs[i] for i in sels(len(segs))[r]]
    o = oracle.estep(a, e, a0, ms)
    for opts in (T_DEFAULT, T_REPAIR):
        check(row(wide_batch(hip, golden, 300, opts)["b"], r), tri_sums(o["A"]), o["E"], o["LL"], ("wide batch vs oracle", opts), (a, e), ms)


# ------------------------------------------------------------------ 3. state
@pytest.mark.parametrize("n", [200, 300])
def test_wide_batch_restores_selection(hip, golden, n):
    """A single estep_factored over a selection of the caller's gives the same bits before the batch, after it, and after a
    batch that ended in an error (replicate 1's matrix has no PSMC form: ENOTSUP naming it, after replicate 0 was reported)."""
    segs = short_segs(golden)
    pars, ss = rep_params(n), sels(len(segs))
    a, e, a0 = pars[0]
    mine = [16, 4, 4, 9]
    es = wide_ctx(hip, n, segs, **T_REPAIR)
    es.select(mine)
    before = es.estep_factored(a, e[:2], a0)
    tiles = ran_wide(es)["n_chunks"]
    assert same_bits(before, fresh_single(hip, n, segs, pars[0], mine, **T_REPAIR))
    b = es.estep_batch(pars, ss, want="sums")
    assert same_bits(row(b, 0), row(wide_batch(hip, golden, n, T_REPAIR)["b"], 0))
    ran_wide(es)
    after = es.estep_factored(a, e[:2], a0)
    assert same_bits(after, before) and ran_wide(es)["n_chunks"] == tiles
    rng = np.random.default_rng(3)
    ar = rng.random((n, n)) ** 4 * 0.02 + np.eye(n) * 0.9
    ar /= ar.sum(1, keepdims=True)
    bad = [pars[0], (ar, pars[1][1], pars[1][2]), pars[2], pars[3]]
    calls = []
    with pytest.raises(hip.HipError, match="replicate 1: .*PSMC form"):
        es.estep_batch(bad, ss, want="sums", on_done=lambda reps, out: calls.append(list(reps)))
    assert calls == [[0]], calls
    after = es.estep_factored(a, e[:2], a0)
    assert same_bits(after, before) and ran_wide(es)["n_chunks"] == tiles
    es.close()


@pytest.mark.parametrize("n", [200, 300])
def test_wide_batch_then_decode(hip, golden, n):
    """With "wide_decode" = 1 a decoding call after the batch answers ESTATE, as after any batch; after one more single E-step it
    reads that E-step's tables again: the path and posterior it gave before the batch, bit for bit."""
    segs = short_segs(golden)
    pars, ss = rep_params(n), sels(len(segs))
    a, e, a0 = pars[0]
    seg = len(segs) - 1
    es = wide_ctx(hip, n, segs, wide_decode=1)
    es.estep_factored(a, e[:2], a0)
    path0, mp0 = es.decode(seg)
    es.estep_batch(pars, ss, want="sums")
    for call in (lambda: es.decode(seg), lambda: es.posterior(seg), lambda: es.scales(seg)):
        with pytest.raises(hip.HipError, match="call order violated"):
            call()
    es.estep_factored(a, e[:2], a0)
    path, mp = es.decode(seg)
    assert np.array_equal(path, path0) and bits_equal(mp, mp0)
    es.close()


# ------------------------------------------------------------------ 4. fallback
@pytest.mark.parametrize("n", [200, 300])
def test_wide_batch_fallback(hip, golden, capfd, n):
    """max_rounds = 0 with tiles of 37 bins and a warm-up of 5: replicates 0, 1 and 3 cannot converge and come back with the exact
    kernels' statistics -- E and LL bit for bit an exact context's select + estep, sums = tri_sums of its A (to 1e-13 of the largest
    cell: the host adds the same doubles in another order) -- each with its line on stderr naming the replicate and the path;
    replicate 2 is one bin, has no tile boundary, and stays wide: the bits of a fresh context's single E-step.  With
    "structured" = 0 the call answers ENOTSUP naming replicate 0, and the selection is restored."""
    segs = short_segs(golden)
    pars, ss = rep_params(n), sels(len(segs))
    opts = dict(max_rounds=0, **T_REPAIR)
    es = wide_ctx(hip, n, segs, **opts)
    capfd.readouterr()
    calls = []
    b = es.estep_batch(pars, ss, want="sums", on_done=lambda reps, out: calls.append(list(reps)))
    err = capfd.readouterr().err
    assert calls == [[0], [1], [2], [3]] and es.batch_info() == dict(groups=N_REP, replicate_contexts=0)
    assert err.count(MSG_EXACT) == 3, err
    for r in (0, 1, 3):
        assert "replicate %d: wide fast E-step did not converge" % r in err, err
    assert "replicate 2" not in err, err
    ex = hip.HipEStep(n, mode=hip.MODE_EXACT)
    ex.load_segments(segs)
    for r in (0, 1, 3):
        ex.select(ss[r])
        x = ex.estep(*pars[r])
        assert bits_equal(b["E"][r], x["E"]) and b["LL"][r] == x["LL"], r
        want = tri_sums(x["A"])
        gap = np.abs(b["sums"][r] - want).max() / np.abs(want).max()
        print("fallback, %d states, replicate %d: sums against tri_sums(A) %.2e of the largest cell" % (n, r, gap))
        assert gap <= 1e-13, (r, gap)
    ex.close()
    assert same_bits(row(b, 2), fresh_single(hip, n, segs, pars[2], ss[2], **opts))
    # "structured" = 0: ENOTSUP from the first replicate; the selection of the caller is back
    es.close()
    es = wide_ctx(hip, n, segs, **T_REPAIR)
    mine = [16, 4, 4, 9]
    es.select(mine)
    a, e, a0 = pars[0]
    before = es.estep_factored(a, e[:2], a0)
    es.set_option("structured", 0)
    calls = []
    with pytest.raises(hip.HipError, match="not supported.*replicate 0: .*structured"):
        es.estep_batch(pars, ss, want="sums", on_done=lambda reps, out: calls.append(list(reps)))
    assert calls == []
    es.set_option("structured", 1)
    assert same_bits(es.estep_factored(a, e[:2], a0), before)
    es.close()


# ------------------------------------------------------------------ 5. nothing else moves
def same_exact(b, x, keys):
    return all(bits_equal(b[k], x[k]) for k in keys)


@pytest.mark.parametrize("n", [200, 300])
def test_wide_batch_leaves_the_rest_exact(hip, golden, n):
    """With "wide_batch" = 1 every call the option does not cover is the exact launch groups' batch, bit for bit in A (or the sums
    the batch makes of it), E and LL: a caller who wants A, or A and sums; "wide_fast" = 0; "wide_fast" = 1 at 300 states; an
    exact-mode context.  And "wide_batch" = 0 with "wide_fast" set is the exact batch, as it was before the option."""
    segs = short_segs(golden)
    pars, ss = rep_params(n), sels(len(segs))
    x = exact_batch(hip, golden, n)
    es = wide_ctx(hip, n, segs)
    assert same_exact(es.estep_batch(pars, ss, want="A"), x, ("A", "E", "LL"))
    assert same_exact(es.estep_batch(pars, ss, want="both"), x, ("A", "sums", "E", "LL"))
    es.set_option("wide_fast", 0)
    assert same_exact(es.estep_batch(pars, ss, want="sums"), x, ("sums", "E", "LL"))
    if n > 256:
        es.set_option("wide_fast", 1)
        assert same_exact(es.estep_batch(pars, ss, want="sums"), x, ("sums", "E", "LL"))
    es.set_option("wide_fast", SIZES[n][2])
    es.set_option("wide_batch", 0)
    assert same_exact(es.estep_batch(pars, ss, want="sums"), x, ("sums", "E", "LL"))
    with pytest.raises(hip.HipError, match="invalid argument"):
        es.set_option("wide_batch", 2)
    es.close()
    ex = hip.HipEStep(n, mode=hip.MODE_EXACT, wide_fast=SIZES[n][2], wide_batch=1)
    ex.load_segments(segs)
    assert same_exact(ex.estep_batch(pars, ss, want="sums"), x, ("sums", "E", "LL"))
    ex.close()


def test_wide_batch_inert_at_64_states(hip, golden):
    """A 64-state context does not read the option: in exact mode and in fast mode the batch with "wide_fast" = 2 and
    "wide_batch" = 1 has the bits of the batch of a context without them (fast mode: two contexts with the same call history
    agree bit for bit), for A and for the sums."""
    p = golden.params("n64_curve")
    par = (p["a"], p["e"], p["a0"])
    segs = golden.segs_small
    ss = [list(range(len(segs))), [7, 7, 3], [8]]
    for mode in (hip.MODE_EXACT, hip.MODE_FAST):
        for want, keys in (("A", ("A", "E", "LL")), ("sums", ("sums", "E", "LL"))):
            rs = []
            for o in (dict(), dict(wide_fast=2, wide_batch=1)):
                es = hip.HipEStep(64, mode=mode, **o)
                es.load_segments(segs)
                rs.append(es.estep_batch([par] * 3, ss, want=want))
                es.close()
            assert same_exact(rs[1], rs[0], keys), (mode, want)
