"""The wide fast E-step (option "wide_fast", psmc_amd/csrc/estep_wide_fast.hip) where tests/test_gpu_wide_fast.py does not look:
per vector and per cell (the gates of gate_factored there), at the extremes of the model, on segments and tiles of a few bins, and
over sequences of calls on one context.  State counts: 129, 192, 193, 256 -- both padded widths (192, 256), each at its fullest
and at its emptiest; the goldens at 149 and 200 states stand for the two widths where the reference's own numbers are wanted.
Expected values: the CPU oracle on the same (multi)set of segments; bit-for-bit claims: a fresh context given only the final
inputs.  tests/test_fastmodel.py holds the CPU side: the factorisation criterion on the models of MODELS, and the numpy model of
fast mode against the oracle per cell on the inputs used here."""
import math
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal, GOLD
from test_gpu_wide_fast import check, ran_wide, tri_sums, WORST   # the block gates + the per-vector gates + the invariants

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Observed on the MI355X (the session summary of conftest.py prints the worst of each metric, the fixture report_worst where it
# occurred).  Bounds: FAST_TOL_CELL 1e-9, FAST_TOL_L1 / FAST_TOL_Q 1e-10.  This file, 102 comparisons:
#   cell  SL 1.0e-12  SU 6.0e-13  DG 6.3e-13  CL 6.6e-13  E0 6.4e-13  E1 6.6e-13: rho0 = 1e-6 at 256 states, default tiling
#         (the numpy model of fast mode against the oracle on the same model and data, untiled, at 200 states: 4.2e-13)
#         CU 3.1e-13: t_max = 0.5 at 256 states
#   L1    <= 3.2e-13 (every vector), QA 2.8e-13, QE 3.1e-13: t_max = 0.5 at 129 states
#   block gates 5.0e-13 (rho0 = 1e-6); LL 4.5e-15 relative (the one-bin segment three times + the all-missing one twice, 149 states)
# tests/test_gpu_wide_fast.py under the same gates, 54 comparisons: cell <= 4.3e-12 (E0; DG 4.2e-12), L1 <= 8.9e-13, QA / QE 8.5e-13,
# all in test_wide_fast_stress (2.2 M bins, against the exact wide kernels), first and third E-step.
# Parts A, B and D found nothing wrong in the kernels; part C found the LL of a one-bin segment one unit in the last place of its sum off
# (test_wide_fast_one_bin_segment_alone), which k_wf_ll now adds up without rounding.


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


@pytest.fixture(scope="module")
def wide():
    return dict(np.load(os.path.join(GOLD, "estep_wide.npz")))


SIZES = {129: ("129*1", 129), 192: ("192*1", 192), 193: ("193*1", 193), 256: ("128*2", 128)}   # states: pattern, free lambdas
                                                                                                  # (a group repeats at most 255 times)
MILD = [0.02, 0.004, 15.0]   # theta0, rho0, t_max of every other wide test


def _alt(m, lo, hi):
    return list(np.where(np.arange(m) % 2 == 0, lo, hi))


# PA-line parameters [theta0, rho0, t_max, lambda_0 ..] of m free lambdas
MODELS = {
    "lambda_alt_1e-3_1e3": lambda m: MILD + _alt(m, 1e-3, 1e3),
    "lambda_alt_1e-1_1e1": lambda m: MILD + _alt(m, 1e-1, 1e1),
    "lambda_ramp_up_1e-3_1e3": lambda m: MILD + list(np.logspace(-3, 3, m)),
    "lambda_ramp_down_1e3_1e-3": lambda m: MILD + list(np.logspace(3, -3, m)),
    "lambda_ramp_down_1e2_1e-2": lambda m: MILD + list(np.logspace(2, -2, m)),
    "lambda_equal": lambda m: MILD + [1.0] * m,
    "rho_1e-6": lambda m: [0.02, 1e-6, 15.0] + [1.0] * m,
    "rho_0.5": lambda m: [0.02, 0.5, 15.0] + [1.0] * m,
    "rho_0.1": lambda m: [0.02, 0.1, 15.0] + [1.0] * m,
    "theta_0.3": lambda m: [0.3, 0.004, 15.0] + [1.0] * m,
    "theta_1e-6": lambda m: [1e-6, 0.004, 15.0] + [1.0] * m,
    "tmax_0.5": lambda m: [0.02, 0.004, 0.5] + [1.0] * m,
    "tmax_60": lambda m: [0.02, 0.004, 60.0] + [1.0] * m,
}
# The models api.hip factor_structure refuses (at all four sizes, and at 200 states), with the entry that refuses them:
# tests/test_fastmodel.py test_factorisation_criterion_on_the_extreme_models holds the numpy restatement to exactly this list.
# Three of thirteen.  None of the three is an HMM at all -- the host model itself breaks down there; the oracle and the exact
# kernels still have the reference's answer (NaN in every cell under the first two, finite under rho0 = 0.5), gated bit for bit in
# tests/test_gpu_exact_extremes.py -- and each has a milder neighbour in the list that is accepted and runs: lambda alternating
# 0.1 / 10, the ramp from 100 down to 0.01 (matrix entries down to 1e-237, a0 down to 1e-231), rho0 = 0.1.
REFUSED = {
    "lambda_alt_1e-3_1e3": "corner a[0][n-1] = 0 and a[n-1][0] = NaN: survival past an interval with lambda = 1e-3 underflows in the host model",
    "lambda_ramp_down_1e3_1e-3": "corner a[0][n-1] = 0 and a[n-1][0] = NaN: as above, the last intervals have lambda -> 1e-3",
    "rho_0.5": "dd[k] = a[k][k] - P[k] qa[k] - R[k] c[k] < 0 (min -0.6): the host model's matrix has negative entries (min -0.5) at this rho0",
}
HARSH = ("rho_1e-6", "lambda_ramp_down_1e2_1e-2")   # accepted: no warm-up forgets / entries at the edge of the double range


def model(name, n):
    from psmc_amd import hostlib
    pat, m = SIZES[n] if n in SIZES else ("%d*2" % (n // 2), n // 2)
    return hostlib.hmm_params(pat, MODELS[name](m))


def mild_model(n):
    from psmc_amd import hostlib
    pat, m = SIZES[n]
    return hostlib.hmm_params(pat, MILD + list(1.0 + 0.6 * np.sin(0.37 * np.arange(m))))


def extremes_segs(golden):
    """part B: about 3e4 bins (segments of 1, 2, 3 .. 20000 bins) -- the oracle at 256 states takes 1.7 s per 1e4 bins and model"""
    return golden.segs_small + [golden.segs_mid[3][:6000]]


def wide_estep(hip, n, segs, par, sel=None, **opts):
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=1, **opts)
    es.load_segments(segs)
    if sel is not None:
        es.select(sel)
    r = es.estep_factored(par[0], par[1][:2], par[2])
    d = ran_wide(es)
    es.close()
    return r, d


def same_bits(r, w):
    return bits_equal(r["sums"], w["sums"]) and bits_equal(r["E"], w["E"]) and r["LL"] == w["LL"]


# ------------------------------------------------------------------ B. model extremes
@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("n", list(SIZES))
def test_wide_fast_model_extremes(hip, golden, oracle, n, name):
    """Every model ends either in a result that passes all gates against the oracle, at the default tiling and at chunk=500 /
    warmup=40 (tiles that have to be repaired), or -- the three of REFUSED, no others -- in ENOTSUP with the "PSMC form" message:
    never in a wrong or non-finite result, and never in ECONVERGE."""
    a, e, a0 = model(name, n)
    segs = extremes_segs(golden)
    if name in REFUSED:
        es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=1)
        es.load_segments(segs)
        with pytest.raises(hip.HipError, match="PSMC form"):
            es.estep_factored(a, e[:2], a0)
        es.close()
        return
    o = oracle.estep(a, e, a0, segs)
    assert np.isfinite(o["A"]).all() and np.isfinite(o["LL"])
    want = tri_sums(o["A"])
    for opts in (dict(), dict(chunk=500, warmup=40)):
        r, d = wide_estep(hip, n, segs, (a, e, a0), **opts)
        check(r, want, o["E"], o["LL"], (name, n, opts, "rounds %d+%d" % (d["fwd_rounds"], d["bwd_rounds"])), (a, e), segs)


@pytest.mark.parametrize("n", list(SIZES))
def test_wide_fast_mild_harsh_mild(hip, golden, n):
    """One context: mild model, a harsh one, the mild one again (twice over, with either harsh model): the mild results are the
    same bits -- with learn=1 the plan of the wide path does not change, and nothing of a harsh E-step's repairs may stay behind."""
    segs = extremes_segs(golden)
    mild = mild_model(n)
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=1, chunk=500, warmup=40)
    es.load_segments(segs)
    first = es.estep_factored(mild[0], mild[1][:2], mild[2])
    tiles = ran_wide(es)["n_chunks"]
    for name in HARSH:
        a, e, a0 = model(name, n)
        h = es.estep_factored(a, e[:2], a0)
        assert np.isfinite(h["sums"]).all() and ran_wide(es)["n_chunks"] == tiles
        again = es.estep_factored(mild[0], mild[1][:2], mild[2])
        assert same_bits(again, first), name
    es.close()


# ------------------------------------------------------------------ C. short and ragged geometry
def ragged_segs(golden):
    """Slices of the fixture data: 1 .. 65 bins, missing data only (3 and 70 bins: shorter than a tile, and across tiles), a
    segment that starts and ends in six bins of missing data, an ordinary one of 2000 bins and one of 2001."""
    src, miss = golden.segs_mid[0], golden.segs_mid[0][34204:34294]
    assert (miss == 2).all() and len(miss) == 90
    segs = [golden.segs_small[0]]
    for i, L in enumerate((2, 3, 4, 5, 7, 8, 9, 63, 64, 65), 1):   # around a heterozygous / a missing bin, at bin i % L of the slice
        p = int(np.flatnonzero(src[1000 * i:] == 1 + i % 2)[0]) + 1000 * i - i % L
        segs.append(src[p:p + L])
    segs += [miss[:3], miss[:70], np.concatenate([miss[:6], src[12000:12288], miss[:6]]), src[20000:22000], src[30000:32001]]
    assert [len(s) for s in segs] == [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 3, 70, 300, 2000, 2001]
    assert len(np.unique(np.concatenate(segs[1:11]))) == 3   # the short ones are not all homozygous
    return segs


I_ONE, I_MISS3, I_MISS70, I_2000 = 0, 11, 12, 14
# "chunk" has no documented minimum (include/psmc_hip.h: 0 = auto, negative = EINVAL), so every tile length from one bin up must
# be right.  chunk=8: the 64-bin segment is exactly 8 tiles, the 65-bin one 8 tiles and a bin; chunk=250: the same of 2000 / 2001.
RAGGED_TILINGS = [dict(chunk=c, warmup=w) for c in (1, 2, 3, 4, 5, 8) for w in (0, 1, 5)] + \
                 [dict(chunk=1, warmup=0, learn=0), dict(chunk=5, warmup=1, learn=0), dict(chunk=250, warmup=5), dict(chunk=250, warmup=0),
                  dict()]


@pytest.mark.parametrize("key", ["n149", "n200"])
def test_wide_fast_short_segments_and_tiles(hip, golden, oracle, wide, key):
    """Segments of 1 .. 5 bins, tiles of 1 .. 5 bins, a segment of exactly 8 tiles and of 8 tiles and one bin, missing data
    only, missing data at both ends, with and without glued repairs -- one size per padded width, the reference's parameters."""
    a, e, a0 = wide[key + ".a"], wide[key + ".e"], wide[key + ".a0"]
    n = a.shape[0]
    segs = ragged_segs(golden)
    o = oracle.estep(a, e, a0, segs)
    want = tri_sums(o["A"])
    for opts in RAGGED_TILINGS:
        r, d = wide_estep(hip, n, segs, (a, e, a0), **opts)
        T = opts.get("chunk", 256)
        assert d["n_chunks"] == sum((len(s) + T - 1) // T for s in segs), (opts, d)
        if opts.get("warmup") == 0:   # no speculation at all: every tile past a segment's first is repaired
            assert d["fwd_rounds"] > 0 and d["bwd_rounds"] > 0, (opts, d)
            if opts.get("learn") == 0:   # ... one tile per segment and round (but for a tile that starts right by chance)
                assert d["fwd_rounds"] >= 1800 // T and d["bwd_rounds"] >= 1800 // T, (opts, d)
        check(r, want, o["E"], o["LL"], (key, "ragged", opts, "rounds %d+%d" % (d["fwd_rounds"], d["bwd_rounds"])), (a, e), segs)


@pytest.mark.parametrize("key", ["n149", "n200"])
def test_wide_fast_short_multisets(hip, golden, oracle, wide, key):
    """select(): the one-bin segment three times and the all-missing one twice -- by themselves (no observed bin at all: E is
    the seeds) and among others."""
    a, e, a0 = wide[key + ".a"], wide[key + ".e"], wide[key + ".a0"]
    n = a.shape[0]
    segs = ragged_segs(golden)
    for sel in ([I_ONE, I_ONE, I_ONE, I_MISS3, I_MISS3], [I_ONE, I_MISS3, I_2000, I_ONE, I_MISS70, I_MISS3, I_ONE, 5]):
        ms = [segs[i] for i in sel]
        o = oracle.estep(a, e, a0, ms)
        for opts in (dict(), dict(chunk=2, warmup=1), dict(chunk=4, warmup=0, learn=0)):
            r, d = wide_estep(hip, n, segs, (a, e, a0), sel=sel, **opts)
            check(r, tri_sums(o["A"]), o["E"], o["LL"], (key, "multiset", sel, opts), (a, e), ms)


@pytest.mark.parametrize("key", ["n149", "n200"])
def test_wide_fast_one_bin_segment_alone(hip, golden, wide, key):
    """The one-bin segment alone: one tile, no transition and no counted bin (the seeds only), and LL = log sum_k a0[k] e[o_1][k]
    to 1e-15 relative -- the products as the kernel forms them, summed exactly (math.fsum), so the reference has no rounding of
    its own.

    This test found the one thing the kernels had to change for.  k_wf_ll added the 149 / 200 products in a fixed tree, in double,
    and ended one unit in the last place of the sum (0.93292 / 0.93328) away from the exact sum: LL -0.06943605406361747 against
    -0.06943605406361758 (1.60e-15 relative) at 149 states, -0.06904683892951673 against -0.06904683892951662 (1.61e-15) at 200,
    in either tiling -- log at 0.933 magnifies a relative error 14.4 times; the reference's own sequential sum (khmm.c, the oracle)
    is off by the same unit.  For a segment of one bin k_wf_ll now adds the products up without rounding (two-sum, tile_total_comp);
    every longer segment keeps the plain sum, and every result of tests/test_gpu_wide_fast.py its bits."""
    a, e, a0 = wide[key + ".a"], wide[key + ".e"], wide[key + ".a0"]
    n = a.shape[0]
    segs = ragged_segs(golden)
    o1 = int(segs[I_ONE][0])
    ref = math.log(math.fsum((a0 * e[o1]).tolist()))
    got = []
    for opts in (dict(), dict(chunk=1, warmup=0)):
        r, d = wide_estep(hip, n, segs, (a, e, a0), sel=[I_ONE], **opts)
        assert d["n_chunks"] == 1
        assert np.isfinite(r["sums"]).all() and r["sums"].sum() < 1e-18 and r["E"].sum() < 1e-18
        assert abs(r["LL"] - ref) <= 1e-14 * abs(ref)   # within a few units in the last place of the sum, whatever else
        print("one-bin LL", key, opts, repr(r["LL"]), repr(ref), abs(r["LL"] - ref) / abs(ref))
        got.append(r["LL"])
    assert got[0] == got[1]
    for ll in got:
        assert abs(ll - ref) <= 1e-15 * abs(ref), (key, ll, ref, abs(ll - ref) / abs(ref))


# ------------------------------------------------------------------ D. call sequences on one context
SEQ_OPTS = dict(chunk=100, warmup=30)   # tiles that need repairs on every set below


@pytest.mark.parametrize("key", ["n149", "n200"])
def test_wide_fast_call_sequence(hip, golden, oracle, wide, key):
    """One context through everything that touches the wide path's own state (wf_chunks / wf_cap, the X table and inv, warmup_set,
    the streams): after every wide E-step the result is, bit for bit, that of a fresh context given only the current segments,
    selection, options and parameters, fast_diag names the wide path with the tile count of the current selection, and each
    distinct input is right against the oracle."""
    import torch
    a, e, a0 = wide[key + ".a"], wide[key + ".e"], wide[key + ".a0"]
    n = a.shape[0]
    par = (a, e, a0)
    set1 = golden.segs_small[:8] + golden.segs_mid[4:]   # 6254 bins
    set2 = golden.segs_small                             # 26051 bins: about four times as many
    set3 = golden.segs_small[:8]                         # 454 bins: the goldens' input
    sel3 = [9, 2, 9, 7, 9, 2]
    gA, gE, gLL = wide[key + ".A"], wide[key + ".E"], float(wide[key + ".LL"])
    checked = {}

    def step(es, what, segs, sel=None):
        """a wide E-step on the sequence's context, against a fresh context and (once per input) the oracle"""
        if sel is not None:
            es.select(sel)
        r = es.estep_factored(a, e[:2], a0)
        d = ran_wide(es)
        ms = [segs[i] for i in sel] if sel is not None else segs
        used = [segs[i] for i in sorted(set(sel))] if sel is not None else segs
        assert d["n_chunks"] == sum((len(s) + 99) // 100 for s in used) and d["warmup"] == 30, (what, d)
        f, _ = wide_estep(hip, n, segs, par, sel=sel, **SEQ_OPTS)
        assert same_bits(r, f), what
        k = (id(segs), tuple(sel) if sel is not None else None)
        if k not in checked:
            o = oracle.estep(a, e, a0, ms)
            check(r, tri_sums(o["A"]), o["E"], o["LL"], (key, "sequence", what), (a, e), ms)
            checked[k] = True
        return r

    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=1, **SEQ_OPTS)
    es.load_segments(set1)
    full1 = step(es, "1 full selection", set1)
    step(es, "2 select with repeats", set1, sel3)
    assert same_bits(step(es, "3 full selection again", set1, list(range(len(set1)))), full1)
    es.load_segments(set2)
    step(es, "4 four times the bins", set2)
    es.load_segments(set3)
    small = step(es, "5 fewer bins", set3)
    x = es.estep(a, e, a0)   # full counts: the exact kernels, the reference's bits
    assert bits_equal(x["A"], gA) and bits_equal(x["E"], gE) and x["LL"] == gLL
    assert same_bits(step(es, "6 after an exact E-step", set3), small)
    b = es.estep_batch([par, par], [list(range(8)), [7, 7, 3]])
    assert bits_equal(b["A"][0], gA) and bits_equal(b["E"][0], gE) and b["LL"][0] == gLL and np.isfinite(b["A"][1]).all()
    assert same_bits(step(es, "7 after a batch", set3), small)
    es.set_cu_range(0, 32)
    assert same_bits(step(es, "8 on 32 compute units", set3), small)
    es.set_cu_range(0, 0)
    assert same_bits(step(es, "8 on the whole device again", set3), small)
    for k, v in dict(chunk=37, warmup=5, learn=0, max_rounds=1).items():
        es.set_option(k, v)
    with pytest.raises(hip.HipError, match="converge"):
        es.estep_factored(a, e[:2], a0)
    for k, v in dict(chunk=100, warmup=30, learn=1, max_rounds=4096).items():
        es.set_option(k, v)
    assert same_bits(step(es, "9 after ECONVERGE", set3), small)
    lens = np.array([len(s) for s in set1], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum((lens.astype(np.int64) + 63) // 64 * 64)])
    host = np.full(int(off[-1]) + 256, 2, dtype=np.uint8)
    for s, o_ in zip(set1, off[:-1]):
        host[o_:o_ + len(s)] = s
    d_obs = torch.from_numpy(host).cuda()
    es.load_segments_device(d_obs.data_ptr(), off[:-1], lens, keepalive=d_obs)
    assert same_bits(step(es, "10 observations in a torch buffer", set1), full1)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        stats = torch.zeros(7 * n + 1, dtype=torch.float64, device="cuda")
    stream.synchronize()
    es.estep_factored_device(a, e, a0, stats.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    h = stats.cpu().numpy()
    ran_wide(es)
    assert same_bits(dict(sums=h[:5 * n].reshape(5, n), E=h[5 * n:7 * n].reshape(2, n), LL=float(h[7 * n])), full1), "11 device entry point"
    es.close()
