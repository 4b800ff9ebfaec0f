"""Decoding on a FAST context (include/psmc_hip.h, estep_post_fast.hip): psmc_hip_decode / _posterior / _post_counts / _scales
read the X and bt tables the last fast E-step left, scale-free.  Every case compares a fast context against an exact context
given the same parameters (the exact ones are the reference's doubles: tests/test_gpu_estep.py), within the stated tolerances:
posterior rows, maxp and recomb 1e-9 absolute; scales 1e-11 relative; post_counts 1e-9 relative on cells >= 1e-6 of the
largest; the path equal wherever the exact posterior's two largest entries differ by more than 2e-9.  And: the fast posteriors
summed per symbol give the same E-step's E; decoding changes nothing a later E-step reads; the refusals."""
import gzip
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal, GOLD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENOME = dict(two_phase=2, merge1=0, warm_shift=1, kc_sub=4)   # the genome's two-round plan (tests/test_gpu_estep.py)

TOL_POST = 1e-9       # posterior rows, maxp, recomb: absolute
TOL_SCALES = 1e-11    # relative
TOL_SCALES_GAPS = 2e-11   # ... with tile boundaries inside 2e5-bin runs of missing data (the stress fixture at 256-bin tiles: 1.1e-11 measured,
                          # the fast forward table's own direction error -- its posterior is off by 1.8e-11 there too -- not the decoding's)
TOL_CELL = 1e-9       # post_counts: relative, on cells >= 1e-6 of the largest
TOL_TIE = 2e-9        # the path may differ only where the exact posterior's two largest entries are closer than this
TOL_E = 1e-10         # sum of the fast posteriors per symbol against the fast E-step's E, relative


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


def _stress_segments():
    lut = np.full(256, 2, np.uint8); lut[ord("T")] = 0; lut[ord("K")] = 1
    segs, cur = [], []
    for line in gzip.open(os.path.join(GOLD, "stress", "stress.psmcfa.gz"), "rb"):
        if line.startswith(b">"):
            if cur: segs.append(np.concatenate(cur))
            cur = []
        else:
            cur.append(lut[np.frombuffer(line.rstrip(b"\n"), dtype=np.uint8)])
    segs.append(np.concatenate(cur))
    return segs


def _n64(golden):
    p = golden.params("n64_curve")
    return p["a"], p["e"], p["a0"]


def _n128(golden):
    g, k = golden.n128, "n128_curve"
    return g[k + ".a"], g[k + ".e"], g[k + ".a0"]


def _capped(a, k0):
    """psmc_cap_matrix-like (aux.c:115-127): columns >= k0 summed into k0 -- no longer of the PSMC form"""
    a = a.copy(); a[:, k0] = a[:, k0:].sum(1); a[:, k0 + 1:] = 0.0
    return a


def compare_decoding(fast, exact, segs, n, full_post=True, rng=None, E=None, tol_scales=TOL_SCALES):
    """Every decoding output of every segment: fast context against exact context (same parameters, E-step done on both)."""
    rng = rng or np.random.default_rng(1)
    worst = dict(post=0.0, maxp=0.0, recomb=0.0, scales=0.0, ties=0)
    cnt_f = np.zeros((n, 3)); cnt_x = np.zeros((n, 3))
    esum = np.zeros((3, n))
    for seg, obs in enumerate(segs):
        L = len(obs)
        px, rx = exact.posterior(seg, want_post=True, want_recomb=True)
        if full_post:
            pf, rf = fast.posterior(seg)
            worst["post"] = max(worst["post"], float(np.abs(pf - px).max()))
            for b in range(3):
                esum[b] += pf[:L - 1][obs[:L - 1] == b].sum(0)
            del pf
        else:
            _, rf = fast.posterior(seg, want_post=False)
        worst["recomb"] = max(worst["recomb"], float(np.abs(rf - rx).max()))
        gp, gm = fast.decode(seg)
        xp, xm = exact.decode(seg)
        worst["maxp"] = max(worst["maxp"], float(np.abs(gm - xm).max()))
        top2 = np.sort(px, axis=1)[:, -2:] if n > 1 else np.concatenate([np.zeros((L, 1)), px], 1)
        clear = (top2[:, 1] - top2[:, 0]) > TOL_TIE
        assert np.array_equal(gp[clear], xp[clear]), (seg, np.nonzero((gp != xp) & clear)[0][:10])
        worst["ties"] += int(((gp != xp) & ~clear).sum())
        sf, sx = fast.scales(seg), exact.scales(seg)
        worst["scales"] = max(worst["scales"], float(np.abs(sf / sx - 1.0).max()))
        _, _, st = exact.tables(seg, want_b=False)
        assert bits_equal(sx, st), seg   # exact mode: psmc_hip_scales is the table get_tables returns
        l1 = max(0, L + (-3 if seg == 1 else 5 if seg == 2 else 0))
        c1 = rng.integers(0, 50, size=(l1, 3), dtype=np.int32)
        fast.post_counts(seg, c1, cnt_f)
        exact.post_counts(seg, c1, cnt_x)
        del px
    big = np.abs(cnt_x) >= 1e-6 * np.abs(cnt_x).max()
    cell = float((np.abs(cnt_f - cnt_x)[big] / np.abs(cnt_x)[big]).max())
    print("\nfast decoding vs exact: post %.2e maxp %.2e recomb %.2e scales %.2e counts %.2e, path differences at near-ties: %d" % (
        worst["post"], worst["maxp"], worst["recomb"], worst["scales"], cell, worst["ties"]))
    assert worst["post"] <= TOL_POST and worst["maxp"] <= TOL_POST and worst["recomb"] <= TOL_POST, worst
    assert worst["scales"] <= tol_scales, worst
    assert cell <= TOL_CELL, cell
    if E is not None and full_post:   # the posterior of the counts kernel: per-symbol sums are the E-step's E (hom, het rows)
        assert float(np.abs(esum[:2] - E).max() / np.abs(E).max()) <= TOL_E
    return worst


def run_pair(hip, n, segs, a, e, a0, fast_opts, full_post=True, check_E=True, tol_scales=TOL_SCALES):
    fast = hip.HipEStep(n, mode=hip.MODE_FAST, **fast_opts)
    fast.load_segments(segs)
    exact = hip.HipEStep(n, mode=hip.MODE_EXACT)
    exact.load_segments(segs)
    rf = fast.estep(a, e, a0)
    exact.estep(a, e, a0)
    w = compare_decoding(fast, exact, segs, n, full_post=full_post, E=rf["E"] if check_E else None, tol_scales=tol_scales)
    info = fast.fast_diag()
    fast.close(); exact.close()
    return w, info


CASES = {
    "small_n64": lambda g: (64, g.segs_small, _n64(g), dict(fuse=0)),
    "mid_n64": lambda g: (64, g.segs_mid, _n64(g), dict(fuse=0)),
    "mid_n64_short_tiles": lambda g: (64, g.segs_mid, _n64(g), dict(fuse=0, chunk=256, warmup=512)),
    "mid_n64_odd_tiles": lambda g: (64, g.segs_mid, _n64(g), dict(fuse=0, chunk=1001, warmup=300)),
    "mid_n64_unstructured": lambda g: (64, g.segs_mid, _n64(g), dict(structured=0)),
    "mid_n64_dense_capped": lambda g: (64, g.segs_mid, (_capped(_n64(g)[0], 40),) + _n64(g)[1:], dict()),
    "small_n128": lambda g: (128, g.segs_small + g.segs_mid[2:], _n128(g), dict(fuse128=0)),
    "small_n128_short_tiles": lambda g: (128, g.segs_small + g.segs_mid[2:], _n128(g), dict(fuse128=0, chunk=512, warmup=256)),
    "small_n100": lambda g: (100, g.segs_small + g.segs_mid[2:],
                             (_n128(g)[0][:100, :100] / _n128(g)[0][:100, :100].sum(1, keepdims=True), _n128(g)[1][:, :100],
                              _n128(g)[2][:100] / _n128(g)[2][:100].sum()), dict(fuse128=0)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_fast_decode_matches_exact(hip, golden, case):
    n, segs, (a, e, a0), opts = CASES[case](golden)
    w, info = run_pair(hip, n, segs, a, e, a0, opts)
    assert info["back_half"] == 0   # the back half that keeps bt ran
    if case == "mid_n64_dense_capped" or case == "mid_n64_unstructured":
        assert not info["structured"]
    else:
        assert info["structured"]


def test_fast_decode_exact_fallback_is_bit_identical(hip, golden):
    """65..128 states and a matrix without the PSMC form: fast mode ran the exact kernels, and so does the decoding."""
    a, e, a0 = _n128(golden)
    a = _capped(a, 90)
    segs = golden.segs_small
    fast = hip.HipEStep(128, mode=hip.MODE_FAST)
    fast.load_segments(segs)
    exact = hip.HipEStep(128, mode=hip.MODE_EXACT)
    exact.load_segments(segs)
    fast.estep(a, e, a0); exact.estep(a, e, a0)
    cf = np.zeros((128, 2)); cx = np.zeros((128, 2))
    rng = np.random.default_rng(3)
    for seg in range(len(segs)):
        for x, y in zip(fast.posterior(seg), exact.posterior(seg)):
            assert bits_equal(x, y), seg
        pf, mf = fast.decode(seg); px, mx = exact.decode(seg)
        assert np.array_equal(pf, px) and bits_equal(mf, mx)
        assert bits_equal(fast.scales(seg), exact.scales(seg))
        c1 = rng.integers(0, 9, size=(len(segs[seg]), 2), dtype=np.int32)
        fast.post_counts(seg, c1, cf); exact.post_counts(seg, c1, cx)
    assert bits_equal(cf, cx)
    fast.close(); exact.close()


@pytest.mark.parametrize("chunk", [1001, 256])
def test_fast_decode_stress(hip, golden, chunk):
    """The stress fixture (2e5-bin runs of missing data, a long run of homozygosity, six segments, 2.2 M bins) at two tile
    lengths, parameters of its EM round 1."""
    segs = _stress_segments()
    g = dict(np.load(os.path.join(GOLD, "stress", "stress_estep.npz")))
    a, e, a0 = g["rd1.a"], g["rd1.e"], g["rd1.a0"]
    run_pair(hip, 64, segs, a, e, a0, dict(fuse=0, chunk=chunk, two_phase=2, merge1=0, warm_shift=1), tol_scales=TOL_SCALES_GAPS)


def test_fast_decode_two_round_plan(hip, golden):
    """A simulated multi-segment input planned in two rounds (more than 4096 tiles: two launches, glued runs, transfer-matrix chains)."""
    from psmc_amd.sim import simulate_genome
    a, e, a0 = _n64(golden)
    segs = simulate_genome(a, e, a0, [600000, 450000, 300000, 120000, 30000, 7, 1], seed=11)
    w, info = run_pair(hip, 64, segs, a, e, a0, dict(fuse=0, chunk=320, **GENOME), full_post=False, check_E=False)
    assert info["structured"] and info["n_chunks"] > 4096


def test_fast_decode_has_no_side_effects(hip, golden):
    """Two contexts with the same call history give bit-identical later E-steps when only one of them decodes in between."""
    a, e, a0 = _n64(golden)
    a2 = a * 0.999 + np.eye(64) * 0.001   # the next EM round's parameters (still of the PSMC form)
    segs = golden.segs_mid
    ctx = [hip.HipEStep(64, mode=hip.MODE_FAST, fuse=0, chunk=512, warmup=256) for _ in range(2)]
    for c in ctx:
        c.load_segments(segs)
        c.estep(a, e, a0)
    for seg in range(len(segs)):
        ctx[1].decode(seg); ctx[1].posterior(seg); ctx[1].scales(seg)
        ctx[1].post_counts(seg, np.ones((len(segs[seg]), 2), np.int32), np.zeros((64, 2)))
    r = [c.estep(a2, e, a0) for c in ctx]
    assert bits_equal(r[0]["A"], r[1]["A"]) and bits_equal(r[0]["E"], r[1]["E"]) and r[0]["LL"] == r[1]["LL"]
    assert ctx[0].fast_plan() == ctx[1].fast_plan()
    r = [c.estep_factored(a, e, a0) for c in ctx]
    assert bits_equal(r[0]["sums"], r[1]["sums"]) and r[0]["LL"] == r[1]["LL"]
    for c in ctx:
        c.close()


def test_fast_decode_refusals(hip, golden):
    a, e, a0 = _n64(golden)
    segs = golden.segs_small
    calls = [lambda c: c.decode(0), lambda c: c.posterior(0), lambda c: c.scales(0),
             lambda c: c.post_counts(0, np.ones((len(segs[0]), 1), np.int32), np.zeros((64, 1)))]
    es = hip.HipEStep(64, mode=hip.MODE_FAST)
    es.load_segments(segs)
    for f in calls:   # no E-step yet
        with pytest.raises(hip.HipError, match="call order violated"):
            f(es)
    es.estep(a, e, a0)   # the fused back half (default): no bt
    assert es.fast_diag()["back_half"] == 1
    for f in calls:
        with pytest.raises(hip.HipError, match="call order violated.*fuse=0"):
            f(es)
    es.set_option("fuse", 0)
    es.estep_factored(a, e, a0)   # the factored statistics: no bt either
    for f in calls:
        with pytest.raises(hip.HipError, match="call order violated.*fuse=0"):
            f(es)
    es.estep(a, e, a0)
    es.decode(0)   # now there is something to decode ...
    es.estep_batch([(a, e, a0)] * 2, [[0, 1], [2, 3]])   # ... and a batch takes the tables
    for f in calls:
        with pytest.raises(hip.HipError, match="call order violated"):
            f(es)
    es.close()
    es = hip.HipEStep(64, mode=hip.MODE_FAST, merge=1)   # the forward fix pass: X carries per-tile factors
    es.load_segments(golden.segs_mid)
    es.estep(a, e, a0)
    for f in (lambda c: c.decode(0), lambda c: c.posterior(0), lambda c: c.scales(0)):
        with pytest.raises(hip.HipError, match="not supported.*merge"):
            f(es)
    es.close()
    es = hip.HipEStep(64, mode=hip.MODE_FAST, fuse=0)   # a segment outside the last E-step's selection
    es.load_segments(segs)
    es.select([1, 2])
    es.estep(a, e, a0)
    es.decode(1)
    with pytest.raises(hip.HipError, match="selection"):
        es.decode(0)
    es.close()
