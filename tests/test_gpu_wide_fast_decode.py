"""Decoding on the wide fast path: a fast-mode context of 129..256 states with "wide_fast" = 1 and "wide_decode" = 1 answers
psmc_hip_decode / _posterior / _post_counts / _scales from what its last wide fast factored E-step left (X, the tiles' start
vectors; no backward table -- psmc_amd/csrc/estep_wide_post.hip).  Every comparison is against an EXACT context given the same
parameters and segments (the reference's doubles: tests/test_gpu_wide.py), with compare_decoding of tests/test_gpu_fast_decode.py
and its tolerances, the library's own for fast decoding (include/psmc_hip.h): posterior rows, maxp, recomb 1e-9 absolute; scales
1e-11 relative (2e-11 for the stress fixture, whose tile boundaries lie inside 2e5-bin gaps: the reason stated there); post_counts
1e-9 relative on cells >= 1e-6 of the largest; path equal wherever the exact posterior's two largest entries differ by more than
2e-9 -- and fewer than 0.1 % of the positions of a case may be such near-ties (counted from the exact context alone).  The
formulas themselves are checked against the oracle on the CPU in tests/test_wide_decode_model.py (1e-12).  compare_decoding
prints the observed maxima of every case.  Observed on the MI355X: goldens and sizes post / maxp <= 1.6e-14, recomb <= 9.7e-14,
scales <= 4.4e-15, counts <= 3.2e-13; the stress fixture post / maxp 2.2e-12, recomb 3.7e-12, scales 2.5e-13, counts 4.6e-12; no
path difference anywhere, no near-tie in any case."""
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal, GOLD
from test_gpu_fast_decode import compare_decoding, _stress_segments, TOL_SCALES, TOL_SCALES_GAPS, TOL_TIE, TOL_POST
from test_gpu_wide_fast import TILINGS, psmc_params, ran_wide

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_UNCLEAR = 1e-3   # of the positions of a case


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module")
def wide():
    return dict(np.load(os.path.join(GOLD, "estep_wide.npz")))


class View:
    """Segments `ids` of a context under the indices 0, 1, ... compare_decoding walks; on the exact side it also counts the
    positions whose two largest posteriors are within TOL_TIE (the ones whose path compare_decoding does not check)."""

    def __init__(self, es, ids, count_ties=False):
        self.es, self.ids, self.count_ties, self.unclear, self.total = es, list(ids), count_ties, 0, 0
        self.ties = {}   # count_ties: segment index -> (positions of the near-ties, the two largest states there)

    def posterior(self, i, **kw):
        post, rec = self.es.posterior(self.ids[i], **kw)
        if self.count_ties and post is not None:
            n = post.shape[1]
            top2 = np.partition(post, n - 2, axis=1)[:, -2:]
            near = np.nonzero(np.abs(top2[:, 1] - top2[:, 0]) <= TOL_TIE)[0]
            self.unclear += len(near); self.total += len(post)
            self.ties[i] = (near, np.argpartition(post[near], n - 2, axis=1)[:, -2:])
        return post, rec

    def decode(self, i): return self.es.decode(self.ids[i])
    def scales(self, i): return self.es.scales(self.ids[i])
    def tables(self, i, **kw): return self.es.tables(self.ids[i], **kw)
    def post_counts(self, i, c1, cnt): return self.es.post_counts(self.ids[i], c1, cnt)


def compare(fast, exact, segs, n, ids=None, tie_rule=False, **kw):
    """compare_decoding over the segments `ids`, and the cap on near-ties.  tie_rule: for an input whose exact posterior alone has
    more near-ties than the cap allows (the caller says why) the cap is replaced by a statement about each of them -- there the
    fast path is one of the exact posterior's two largest states."""
    ids = list(range(len(segs))) if ids is None else ids
    vx = View(exact, ids, count_ties=True)
    vf = View(fast, ids)
    w = compare_decoding(vf, vx, [segs[i] for i in ids], n, **kw)
    assert vx.total == sum(len(segs[i]) for i in ids)
    if not tie_rule:
        assert vx.unclear < MAX_UNCLEAR * vx.total, (vx.unclear, vx.total)   # the near-tie escape is a cap, not a licence
        return w
    for i, (near, two) in vx.ties.items():
        path = vf.decode(i)[0][near]
        assert ((path == two[:, 0]) | (path == two[:, 1])).all(), (ids[i], near, path, two)
    assert sum(len(t[0]) for t in vx.ties.values()) == vx.unclear
    w["near_ties"] = vx.unclear
    return w


def pair(hip, n, segs, **opts):
    fast = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=1, wide_decode=1, **opts)
    fast.load_segments(segs)
    exact = hip.HipEStep(n, mode=hip.MODE_EXACT)
    exact.load_segments(segs)
    return fast, exact


def run_pair(hip, n, segs, a, e, a0, opts, **kw):
    fast, exact = pair(hip, n, segs, **opts)
    rf = fast.estep_factored(a, e[:2], a0)
    d = ran_wide(fast)
    exact.estep(a, e, a0)
    w = compare(fast, exact, segs, n, E=rf["E"], **kw)
    fast.close(); exact.close()
    return w, d


# ---- 1. the reference's goldens, in the tilings of tests/test_gpu_wide_fast.py (repairs and glued runs happen)
@pytest.mark.parametrize("key", ["n200", "n149"])
@pytest.mark.parametrize("opts", TILINGS)
def test_wide_decode_golden(hip, golden, wide, key, opts):
    a, e, a0 = wide[key + ".a"], wide[key + ".e"], wide[key + ".a0"]
    w, d = run_pair(hip, a.shape[0], golden.segs_small[:8], a, e, a0, opts)
    if opts.get("chunk") == 37:
        assert d["fwd_rounds"] + d["bwd_rounds"] > 0, d   # bentry of repaired tiles is what gets decoded


# ---- 2. sizes around the padding steps, host-model parameters
@pytest.mark.parametrize("n", [129, 191, 192, 193, 255, 256])
def test_wide_decode_sizes(hip, golden, n):
    rng = np.random.default_rng(2000 + n)
    a, e, a0 = psmc_params("%d*1" % n, n, rng) if n < 256 else psmc_params("128*2", 128, rng)
    segs = golden.segs_small + golden.segs_mid[3:]
    for opts in (dict(), dict(chunk=500, warmup=40)):
        run_pair(hip, n, segs, a, e, a0, opts)


# ---- 3. the stress fixture (2e5-bin gaps, a long run of homozygosity) at two tile lengths, 200 states
@pytest.mark.parametrize("chunk", [1001, 256])
def test_wide_decode_stress(hip, chunk):
    segs = _stress_segments()
    a, e, a0 = psmc_params("100*2", 100, np.random.default_rng(7))
    run_pair(hip, 200, segs, a, e, a0, dict(chunk=chunk), full_post=chunk == 1001, tol_scales=TOL_SCALES_GAPS)


# ---- 4. short segments, tiles of a few bins, a tile that holds only position L, multisets and partial selections
def _short_segments(golden):
    src = golden.segs_mid[0]
    return [src[100:100 + L].copy() for L in (1, 2, 3, 4, 5, 41, 9, 33, 16)]   # chunk=8: 41 and 33 end in a tile of one position


@pytest.mark.parametrize("opts", [dict(chunk=8, warmup=3), dict(chunk=4, warmup=0), dict(chunk=5, warmup=64), dict()])
def test_wide_decode_short_segments(hip, golden, wide, opts):
    a, e, a0 = wide["n200.a"], wide["n200.e"], wide["n200.a0"]
    segs = _short_segments(golden)
    fast, exact = pair(hip, 200, segs, **opts)
    rf = fast.estep_factored(a, e[:2], a0)
    exact.estep(a, e, a0)
    compare(fast, exact, segs, 200, E=rf["E"])
    # post_counts with one column, l shorter and longer than L, running totals carried from segment to segment
    rng = np.random.default_rng(5)
    cf = np.zeros((200, 1)); cx = np.zeros((200, 1))
    for seg, obs in enumerate(segs):
        for l in (max(0, len(obs) - 2), len(obs), len(obs) + 7):
            c1 = rng.integers(0, 50, size=(l, 1), dtype=np.int32)
            fast.post_counts(seg, c1, cf); exact.post_counts(seg, c1, cx)
    big = np.abs(cx) >= 1e-6 * np.abs(cx).max()
    assert float((np.abs(cf - cx)[big] / np.abs(cx)[big]).max()) <= 1e-9
    fast.close(); exact.close()


def test_wide_decode_selections(hip, golden, wide):
    """A segment selected twice is decoded once (all copies are equal); segments outside the selection are refused."""
    a, e, a0 = wide["n149.a"], wide["n149.e"], wide["n149.a0"]
    segs = golden.segs_small[3:10] + golden.segs_mid[4:]
    fast, exact = pair(hip, 149, segs, chunk=100, warmup=30)
    exact.estep(a, e, a0)
    sel = [8, 3, 8, 5, 5, 5, 0]
    fast.select(sel)
    fast.estep_factored(a, e[:2], a0)
    compare(fast, exact, segs, 149, ids=[0, 3, 5, 8])
    for seg in (1, 2, 4, 6, 7):
        with pytest.raises(hip.HipError, match="call order violated.*selection"):
            fast.decode(seg)
    fast.close(); exact.close()


# ---- 5. a decoding call reads only
def test_wide_decode_has_no_side_effects(hip, golden, wide):
    a, e, a0 = wide["n200.a"], wide["n200.e"], wide["n200.a0"]
    rng = np.random.default_rng(11)
    a2, e2, a02 = psmc_params("100*2", 100, rng)
    segs = golden.segs_small[:11]
    ctx = [hip.HipEStep(200, mode=hip.MODE_FAST, wide_fast=1, wide_decode=1, chunk=100, warmup=30) for _ in range(2)]
    for c in ctx:
        c.load_segments(segs)
        c.estep_factored(a, e[:2], a0)
    for seg in range(len(segs)):
        ctx[1].decode(seg); ctx[1].posterior(seg); ctx[1].scales(seg)
        ctx[1].post_counts(seg, np.ones((len(segs[seg]), 2), np.int32), np.zeros((200, 2)))
    for pa in ((a2, e2, a02), (a, e, a0)):
        r = [c.estep_factored(pa[0], pa[1][:2], pa[2]) for c in ctx]
        assert bits_equal(r[0]["sums"], r[1]["sums"]) and bits_equal(r[0]["E"], r[1]["E"]) and r[0]["LL"] == r[1]["LL"]
    for c in ctx:
        c.close()


def _all_outputs(es, segs, n, seed=3):
    rng = np.random.default_rng(seed)
    out, cnt = [], np.zeros((n, 2))
    for seg in range(len(segs)):
        out += list(es.posterior(seg)) + list(es.decode(seg)) + [es.scales(seg)]
        es.post_counts(seg, rng.integers(0, 9, size=(len(segs[seg]), 2), dtype=np.int32), cnt)
    return out + [cnt]


def _same_bits(x, y):
    return len(x) == len(y) and all(np.array_equal(u, v) if u.dtype.kind == "i" else bits_equal(u, v) for u, v in zip(x, y))


# ---- 6. the last single E-step decides
def test_wide_decode_follows_the_last_estep(hip, golden, wide):
    a, e, a0 = wide["n200.a"], wide["n200.e"], wide["n200.a0"]
    a2, e2, a02 = psmc_params("100*2", 100, np.random.default_rng(12))
    segs = golden.segs_small[3:10]
    ex1 = hip.HipEStep(200, mode=hip.MODE_EXACT); ex1.load_segments(segs); ex1.estep(a, e, a0)
    ex2 = hip.HipEStep(200, mode=hip.MODE_EXACT); ex2.load_segments(segs); ex2.estep(a2, e2, a02)
    want1 = _all_outputs(ex1, segs, 200)
    for wd in (1, 0):
        es = hip.HipEStep(200, mode=hip.MODE_FAST, wide_fast=1, wide_decode=wd, chunk=100, warmup=30)
        es.load_segments(segs)
        es.estep(a, e, a0)                         # exact E-step -> the exact tables, bit for bit, with or without the option
        assert _same_bits(_all_outputs(es, segs, 200), want1)
        rf = es.estep_factored(a2, e2[:2], a02)    # wide fast E-step at other parameters
        if wd:                                     # ... -> its tables: the decoding of the NEW parameters
            compare(es, ex2, segs, 200, E=rf["E"])
            p_new, _ = es.posterior(6)
            p_old, _ = ex1.posterior(6)
            assert float(np.abs(p_new - p_old).max()) > 1e3 * TOL_POST   # (not the stale exact tables)
            es.estep(a, e, a0)                     # and an exact E-step afterwards takes over again
            assert _same_bits(_all_outputs(es, segs, 200), want1)
        else:                                      # "wide_decode" = 0: the exact tables whatever ran last, as before the option
            assert _same_bits(_all_outputs(es, segs, 200), want1)
        es.close()
    ex1.close(); ex2.close()


# ---- 7. refusals
def test_wide_decode_refusals(hip, golden, wide):
    a, e, a0 = wide["n200.a"], wide["n200.e"], wide["n200.a0"]
    segs = golden.segs_small[:10]
    calls = [lambda c: c.decode(5), lambda c: c.posterior(5), lambda c: c.scales(5),
             lambda c: c.post_counts(5, np.ones((len(segs[5]), 1), np.int32), np.zeros((c.n, 1)))]

    def refused(es, match="call order violated"):
        for f in calls:
            with pytest.raises(hip.HipError, match=match):
                f(es)

    es = hip.HipEStep(200, mode=hip.MODE_FAST, wide_fast=1, wide_decode=1)
    es.load_segments(segs)
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

    es = hip.HipEStep(200, mode=hip.MODE_FAST, wide_fast=1, wide_decode=1, chunk=37, warmup=5, learn=0, max_rounds=0)
    es.load_segments(segs)
    with pytest.raises(hip.HipError, match="converge"):
        es.estep_factored(a, e[:2], a0)
    refused(es, "call order violated.*returned an error")   # bentry is not converged
    es.set_option("max_rounds", 4096)
    es.estep_factored(a, e[:2], a0)
    for f in calls:
        f(es)
    es.close()

    # 300 states with both options: the exact kernels, bit for bit
    a3, e3, a03 = psmc_params("150*2", 150, np.random.default_rng(13))
    es = hip.HipEStep(300, mode=hip.MODE_FAST, wide_fast=1, wide_decode=1)
    ex = hip.HipEStep(300, mode=hip.MODE_EXACT)
    for c in (es, ex):
        c.load_segments(segs)
        c.estep(a3, e3, a03)
    assert _same_bits(_all_outputs(es, segs, 300), _all_outputs(ex, segs, 300))
    es.close(); ex.close()


def test_wide_decode_unknown_without_the_feature(hip):
    """The option is a 0/1 switch of psmc_hip_set_option (and of a group: it passes every key on)."""
    es = hip.HipEStep(200, mode=hip.MODE_FAST)
    es.set_option("wide_decode", 1); es.set_option("wide_decode", 0)
    with pytest.raises(hip.HipError):
        es.set_option("wide_decode", 2)
    es.close()
    g = hip.HipGroup(200, [0, 0], mode=hip.MODE_FAST, wide_fast=1, wide_decode=1)
    g.close()


# ---- 8. determinism
def test_wide_decode_is_deterministic(hip, golden, wide):
    a, e, a0 = wide["n149.a"], wide["n149.e"], wide["n149.a0"]
    segs = golden.segs_small[:11] + golden.segs_mid[4:]
    outs = []
    for _ in range(2):
        es = hip.HipEStep(149, mode=hip.MODE_FAST, wide_fast=1, wide_decode=1, chunk=64, warmup=8)
        es.load_segments(segs)
        es.estep_factored(a, e[:2], a0)
        outs.append(_all_outputs(es, segs, 149))
        outs.append(_all_outputs(es, segs, 149))   # and the same context again
        es.close()
    for o in outs[1:]:
        assert _same_bits(o, outs[0])
