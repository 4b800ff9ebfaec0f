"""Fast mode beyond 128 hidden states: psmc_hip_estep_factored with the option "wide_fast" = 1 at 129 .. 256 states (the
kernels of psmc_amd/csrc/estep_wide_fast.hip: one tile per wave, 64 lanes x 3 or 4 states).  Against the reference's goldens at
200 and 149 states, the oracle on PSMC-form HMMs of the host model at sizes around the padding steps, real-data-shaped input
(long runs of missing data and of homozygosity) against the exact wide kernels, and the boundaries of the option.  Tolerances:
the ones fast mode states in tests/test_gpu_estep.py."""
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal, GOLD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST_TOL_STATS = 1e-10   # of the largest cell
FAST_TOL_LL = 1e-12      # relative


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module")
def wide():
    return dict(np.load(os.path.join(GOLD, "estep_wide.npz")))


def tri_sums(A):
    """SL, SU, DG, CL, CU of a count matrix (what the O(N) objective of psmc_amd/host/mstep.c reads)."""
    lo, up = np.tril(A, -1), np.triu(A, 1)
    return np.stack([lo.sum(1), up.sum(1), np.diag(A).copy(), lo.sum(0), up.sum(0)])


def relmax(x, y):
    return float(np.abs(np.asarray(x) - np.asarray(y)).max() / max(np.abs(np.asarray(y)).max(), 1e-300))


# what the two block gates are silent about (psmc_amd/parity.py factored_error_metrics): each of the seven vectors SL, SU, DG, CL, CU,
# E0, E1 by itself -- the block's largest cell is the diagonal count of the most occupied state, and a weakly occupied state (lane
# 0 or 63 of the whole-wave scans, the last real state beside the padding) can be wrong in its fourth digit under it.  The bounds
# are fast mode's own, stated in tests/test_gpu_estep.py for the paths up to 128 states; tests/test_fastmodel.py shows on the CPU
# that the algorithm itself (tests/fastmodel.py, untiled, in double) meets the cell bound a hundred times over on these inputs.
# Observed on the MI355X: cell <= 4.3e-12, L1 and Q <= 8.9e-13 in this file (test_wide_fast_stress), 1.0e-12 / 3.2e-13 in
# tests/test_gpu_wide_fast_edges.py, whose header lists them per vector.
FAST_TOL_CELL = 1e-9     # tests/test_gpu_estep.py: largest relative error of a cell >= 1e-6 x the largest cell of its vector
FAST_TOL_L1 = 1e-10      # tests/test_gpu_estep.py: sum |x - ref| / sum |ref|, per vector
FAST_TOL_Q = 1e-10       # tests/test_gpu_estep.py: sum sums . log factors and sum E log e, relative
WORST = {}               # metric -> (largest value of the session, which comparison)


def gate_factored(r, sums, E, LL, what="", par=None):
    """The per-vector gates of a factored result against its reference (par = (a, e): the two sums of the M-step as well)."""
    import conftest
    from psmc_amd.parity import factored_error_metrics, FACTORED_NAMES
    m = factored_error_metrics(r, dict(sums=sums, E=E, LL=LL), par[0] if par else None, par[1] if par else None)
    conftest.FAST_METRICS.append(m)
    for k, v in m.items():
        if not v <= WORST.get(k, (-1.0, None))[0]:
            WORST[k] = (v, what)
    print("wide fast vs reference", what, "  ".join("%s %.2e" % (k, m[k]) for k in sorted(m)))
    for v in FACTORED_NAMES:
        assert m[v + "_cell"] <= FAST_TOL_CELL, (what, v, m)
        assert m[v + "_l1"] <= FAST_TOL_L1, (what, v, m)
    if par:
        assert m["QA"] <= FAST_TOL_Q and m["QE"] <= FAST_TOL_Q, (what, m)
    return m


def check_invariants(r, sums, segs, what=""):
    """What needs no reference (tests/test_gpu_estep.py test_fast_full_size_properties): both ways of adding the counts up give
    the number of transitions of the multiset `segs`, E the number of observed bins among them (positions 1 .. L-1, khmm.c),
    everything is finite, and the four sums over no cell at all -- SL_0, SU_{n-1}, CL_{n-1}, CU_0 -- are what the reference has."""
    S, E = np.asarray(r["sums"]), np.asarray(r["E"])
    assert np.isfinite(S).all() and np.isfinite(E).all() and np.isfinite(r["LL"]), what
    trans = float(sum(len(s) - 1 for s in segs))
    seen = float(sum(int((np.asarray(s)[:-1] != 2).sum()) for s in segs))
    assert abs(S[0].sum() + S[1].sum() + S[2].sum() - trans) <= 1e-9 * max(trans, 1.0), (what, S[:3].sum(), trans)
    assert abs(S[3].sum() + S[4].sum() + S[2].sum() - trans) <= 1e-9 * max(trans, 1.0), (what, S[2:].sum(), trans)
    assert abs(E.sum() - seen) <= 1e-9 * max(seen, 1.0), (what, E.sum(), seen)
    for v, k in ((0, 0), (1, -1), (3, -1), (4, 0)):
        assert S[v, k] == sums[v][k], (what, v, k, S[v, k], sums[v][k])


def check(r, sums, E, LL, what="", par=None, segs=None):
    assert relmax(r["sums"], sums) < FAST_TOL_STATS, (what, relmax(r["sums"], sums))
    assert relmax(r["E"], E) < FAST_TOL_STATS, (what, relmax(r["E"], E))
    assert abs(r["LL"] - LL) <= FAST_TOL_LL * abs(LL), (what, r["LL"], LL)
    gate_factored(r, sums, E, LL, what, par)
    if segs is not None:
        check_invariants(r, sums, segs, what)


def ran_wide(es):
    """fast_diag / fast_repairs / fast_info of the last E-step: the wide path ran (recounted = 2, back half 3)."""
    d = es.fast_diag()
    assert d["recounted"] == 2 and d["back_half"] == 3 and d["n_chunks"] > 0, d
    return d


def psmc_params(pattern, n, rng):
    """the host model of `pattern` with n free lambdas, seeded random"""
    from psmc_amd import hostlib
    lam = np.exp(rng.normal(0.0, 0.7, size=n))
    return hostlib.hmm_params(pattern, [0.02, 0.004, 15.0] + list(lam))


TILINGS = [dict(), dict(chunk=100, warmup=30), dict(chunk=37, warmup=5), dict(chunk=64, warmup=0), dict(chunk=100, warmup=30, learn=0)]


@pytest.mark.parametrize("key", ["n200", "n149"])
@pytest.mark.parametrize("opts", TILINGS)
def test_wide_fast_golden(hip, golden, wide, key, opts):
    """The reference's goldens (segments_small[:8]): three factored E-steps in a row on one context, in several tilings
    (chunk=37 / warmup=5 and warmup=0 repair most tiles; learn=0 repairs one tile per round)."""
    a, e, a0 = wide[key + ".a"], wide[key + ".e"], wide[key + ".a0"]
    n = a.shape[0]
    want = tri_sums(wide[key + ".A"])
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=1, **opts)
    es.load_segments(golden.segs_small[:8])
    first = None
    for it in range(3):
        r = es.estep_factored(a, e[:2], a0)
        check(r, want, wide[key + ".E"], float(wide[key + ".LL"]), (key, opts, it), (a, e), golden.segs_small[:8])
        d = ran_wide(es)
        if first is None:
            first = r
        else:   # the same call history: the same bits
            assert bits_equal(r["sums"], first["sums"]) and bits_equal(r["E"], first["E"]) and r["LL"] == first["LL"]
    if opts.get("chunk") == 37:
        assert d["fwd_rounds"] + d["bwd_rounds"] > 0, d   # the tiling does exercise the repairs
    es.close()


def test_wide_fast_golden_multiset(hip, golden, oracle, wide):
    """select() with a repeated segment (a bootstrap multiset) against the oracle on the same multiset."""
    a, e, a0 = wide["n200.a"], wide["n200.e"], wide["n200.a0"]
    n = a.shape[0]
    segs = golden.segs_small[:8] + golden.segs_mid[4:]
    sel = [8, 3, 8, 9, 9, 9, 0, 7]
    o = oracle.estep(a, e, a0, [segs[i] for i in sel])
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=1, chunk=300, warmup=64)
    es.load_segments(segs)
    es.select(sel)
    r = es.estep_factored(a, e[:2], a0)
    check(r, tri_sums(o["A"]), o["E"], o["LL"], "multiset", (a, e), [segs[i] for i in sel])
    ran_wide(es)
    es.close()


@pytest.mark.parametrize("n", [129, 150, 192, 193, 200, 224, 255, 256])
def test_wide_fast_vs_oracle(hip, golden, oracle, n):
    """PSMC-form HMMs of the host model (psmc_amd.hostlib.hmm_params, pinned against the reference's psmc_update_hmm) with
    seeded random lambdas, both padded widths (192, 256), default tiles and tiles small enough to repair."""
    rng = np.random.default_rng(1000 + n)
    a, e, a0 = psmc_params("%d*1" % n, n, rng) if n < 256 else psmc_params("128*2", 128, rng)   # (a group repeats at most 255 times)
    segs = golden.segs_small + golden.segs_mid[3:]
    o = oracle.estep(a, e, a0, segs)
    want = tri_sums(o["A"])
    for opts in (dict(), dict(chunk=500, warmup=40)):
        es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=1, **opts)
        es.load_segments(segs)
        r = es.estep_factored(a, e[:2], a0)
        check(r, want, o["E"], o["LL"], (n, opts), (a, e), segs)
        ran_wide(es)
        es.close()


@pytest.fixture(scope="module")
def stress_segs():
    import gzip
    lut = np.full(256, 2, np.uint8); lut[ord("T")] = 0; lut[ord("K")] = 1
    segs, cur = [], []
    for line in gzip.open(os.path.join(GOLD, "stress", "stress.psmcfa.gz"), "rb"):
        if line.startswith(b">"):
            if cur: segs.append(np.concatenate(cur))
            cur = []
        else:
            cur.append(lut[np.frombuffer(line.rstrip(b"\n"), dtype=np.uint8)])
    segs.append(np.concatenate(cur))
    assert [len(s) for s in segs] == [700000, 500000, 400000, 250000, 150000, 200200]
    return segs


def test_wide_fast_stress(hip, stress_segs):
    """tests/golden/stress (2e5-bin runs of N, a 5e4-bin run of homozygosity, an all-gap segment) at 200 states: the first and
    the third factored E-step of one context, parameters moving, against the exact wide kernels on the same device."""
    rng = np.random.default_rng(7)
    pars = [psmc_params("100*2", 100, rng) for _ in range(3)]
    ex = hip.HipEStep(200, mode=hip.MODE_EXACT)
    ex.load_segments(stress_segs)
    es = hip.HipEStep(200, mode=hip.MODE_FAST, wide_fast=1)
    es.load_segments(stress_segs)
    for it, (a, e, a0) in enumerate(pars):
        r = es.estep_factored(a, e[:2], a0)
        d = ran_wide(es)
        if it in (0, 2):
            x = ex.estep(a, e, a0)
            check(r, tri_sums(x["A"]), x["E"], x["LL"], ("E-step %d" % (it + 1), "repair rounds fwd %d bwd %d, tiles fwd %d bwd %d" %
                                                          (d["fwd_rounds"], d["bwd_rounds"], d["fwd_tiles"], d["bwd_tiles"])), (a, e), stress_segs)
    es.close(); ex.close()


def test_wide_fast_boundaries(hip, golden, wide):
    """257 states: ENOTSUP naming the limit; a matrix without the PSMC form: ENOTSUP; psmc_hip_estep of a wide_fast context
    stays bit-identical to the reference; max_rounds reached: ECONVERGE, and the context recovers."""
    from psmc_amd import hostlib
    segs = golden.segs_small[:8]
    a, e, a0 = hostlib.hmm_params("1+128*2", [0.02, 0.004, 15.0] + [1.0] * 129)
    es = hip.HipEStep(257, mode=hip.MODE_FAST, wide_fast=1)
    es.load_segments(segs)
    with pytest.raises(hip.HipError, match="256"):
        es.estep_factored(a, e[:2], a0)
    es.close()

    g = wide
    a, e, a0 = g["n200.a"], g["n200.e"], g["n200.a0"]
    rng = np.random.default_rng(3)
    ar = rng.random((200, 200)) ** 4 * 0.02 + np.eye(200) * 0.9
    ar /= ar.sum(1, keepdims=True)
    es = hip.HipEStep(200, mode=hip.MODE_FAST, wide_fast=1)
    es.load_segments(segs)
    with pytest.raises(hip.HipError, match="PSMC form"):
        es.estep_factored(ar, e[:2], a0)
    r = es.estep(a, e, a0)   # full counts: the exact kernels, bit for bit
    assert bits_equal(r["A"], g["n200.A"]) and bits_equal(r["E"], g["n200.E"]) and r["LL"] == float(g["n200.LL"])
    f, b, sc = es.tables(5)
    es.estep_factored(a, e[:2], a0)
    f2, b2, sc2 = es.tables(5)   # the wide path keeps its own tables
    assert bits_equal(f2, f) and bits_equal(b2, b) and bits_equal(sc2, sc)
    assert bits_equal(f[::7], g["n200.f65"])
    es.close()

    es = hip.HipEStep(200, mode=hip.MODE_FAST, wide_fast=1, chunk=37, warmup=5, learn=0, max_rounds=1)
    es.load_segments(segs)
    with pytest.raises(hip.HipError, match="converge"):
        es.estep_factored(a, e[:2], a0)
    # back to the defaults ("warmup", once set, is the caller's: set to the wide path's own default, 16384): the same bits as a
    # fresh context with default options
    for k, v in dict(chunk=0, warmup=16384, learn=1, max_rounds=4096).items():
        es.set_option(k, v)
    r = es.estep_factored(a, e[:2], a0)
    check(r, tri_sums(g["n200.A"]), g["n200.E"], float(g["n200.LL"]), "after ECONVERGE", (a, e), segs)
    assert ran_wide(es)["warmup"] == 16384
    es.close()
    fresh = hip.HipEStep(200, mode=hip.MODE_FAST, wide_fast=1)
    fresh.load_segments(segs)
    r2 = fresh.estep_factored(a, e[:2], a0)
    assert ran_wide(fresh)["warmup"] == 16384
    assert bits_equal(r["sums"], r2["sums"]) and bits_equal(r["E"], r2["E"]) and r["LL"] == r2["LL"]
    fresh.close()


@pytest.mark.parametrize("chunk", [37, 38, 39, 41])
def test_wide_fast_anchored_tile_below_segment_end(hip, golden, oracle, wide, chunk):
    """Tiles whose backward warm-up starts at the segment's last position (anchored: never verified) must get the exact start
    vector bt_{top+1} whatever top is modulo 4 -- segments of 1003 .. 1006 bins with warmup=5 put the second-to-last tile's top
    on every residue (chunk=37: top = 999 = 3 mod 4)."""
    a, e, a0 = wide["n200.a"], wide["n200.e"], wide["n200.a0"]
    segs = [golden.segs_mid[0][:L] for L in (1003, 1004, 1005, 1006)] + [golden.segs_mid[1][:2000]]
    o = oracle.estep(a, e, a0, segs)
    es = hip.HipEStep(200, mode=hip.MODE_FAST, wide_fast=1, chunk=chunk, warmup=5)
    es.load_segments(segs)
    r = es.estep_factored(a, e[:2], a0)
    check(r, tri_sums(o["A"]), o["E"], o["LL"], ("anchored", chunk), (a, e), segs)
    ran_wide(es)
    es.close()


def test_wide_fast_option_is_inert_elsewhere(hip, golden):
    """Exact mode, and fast mode up to 128 states, accept "wide_fast" and do not change: same bits with and without it."""
    p = golden.params("n64_curve")
    for mode in (hip.MODE_EXACT, hip.MODE_FAST):
        rs = []
        for wf in (0, 1):
            es = hip.HipEStep(64, mode=mode, wide_fast=wf)
            es.load_segments(golden.segs_small)
            rs.append(es.estep(p["a"], p["e"], p["a0"]))
            es.close()
        assert bits_equal(rs[0]["A"], rs[1]["A"]) and bits_equal(rs[0]["E"], rs[1]["E"]) and rs[0]["LL"] == rs[1]["LL"]
