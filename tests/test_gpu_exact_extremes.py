"""The exact E-step bit for bit where tests/test_gpu_estep.py and tests/test_gpu_wide.py do not look: the statistics A, E, A0, LL
and chk of psmc_hip_estep, the per-segment `he` of psmc_hip_estep_segments, the tables and psmc_hip_estep_batch under the thirteen
extreme PSMC models (tests/test_gpu_wide_fast_edges.py MODELS; three of them are no HMM: NaN and -inf or negative entries in the
matrix) and four synthetic matrices (negative cells, exact zeros, a 0 / 0 in some segments only, an infinite row), at every state
count at which another kernel family or another padding runs (tests/exact_extremes.py FAMILIES).  The expected values are the CPU
oracle's, which tests/test_exact_extremes_model.py holds to the real reference's bits (tests/golden/exact_extremes.npz); every
comparison is equality of float64 bit patterns, NaN payloads and signs included, and every condition that keeps a case from
passing by accident is asserted on the oracle before the device is asked (exact_extremes.conditions).

  X1  psmc_hip_estep after psmc_hip_select (a multiset: one segment three times, one twice, one left out): A, E, A0, LL, chk.
  X2  psmc_hip_estep_segments: seg_A, the three rows of seg_E, seg_LL, chk; seg_A0 against the oracle on each segment alone.
  X3  psmc_hip_get_tables of the 65-bin and of the longest segment: f, b, s.
  X4  psmc_hip_estep_batch(want="A"): the case's model, lambda_equal at the same size, the case's model on a second multiset, in
      two or more launches; exact_refwd 2 / 1 / 0 up to 64 states, batch_sort 1 / 0 beyond.  The lambda_equal replicate must come
      back with the finite oracle's bits while NaN and negative neighbours share its launches.  A work-group holds entries of one
      replicate only; what k_expect_exact_rf2 (exact_refwd = 2) shares is the LDS rings and consumer waves of two SEGMENTS of a
      replicate, and under "dead het" at least one such pair is a NaN segment beside a finite one (exact_extremes.mixed_pairs,
      asserted before the device is asked).
  X5  a MODE_FAST context at 150 and 300 states: psmc_hip_estep runs the exact kernels there.
  X6  the exact group on two shards at 64, 128 and 200 states.
  X7  the general wide kernels at 129, 200 and 224 states (PSMC_HIP_WIDE_L2=1, a fresh child process).

The NaN rule: a cell that is NaN in the oracle is NaN on the device and no other is, sign included -- x86 gives every NaN it makes
the sign bit and a propagated NaN keeps its sign, so where no parameter is a positive NaN every NaN of the reference is negative.
Observed on the MI355X (profiles/exact_extremes_tests.txt): 654 passed in 155 s, about nine tenths of it the oracle on the CPU (the
slowest case 4.5 s: the batch at 1024 states); nothing differed in any kernel family, and every NaN came back with the oracle's sign,
those the device makes itself (0 / 0, inf * 0) included."""
import functools
import os
import subprocess
import sys
import numpy as np
import pytest
from conftest import bits_equal

import exact_extremes as xx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_MODEL = xx.ONE_NAN_MODEL
COMPARISONS = [0]


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module", autouse=True)
def report_comparisons():
    yield
    print("exact extremes: %d bit comparisons" % COMPARISONS[0])


def describe(got, want):
    """where two arrays differ, for the assertion message: finite bits, NaN cells, NaN signs"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return "shapes %s %s" % (got.shape, want.shape)
    diff = got.view(np.uint64) != want.view(np.uint64)
    gn, wn = np.isnan(got), np.isnan(want)
    first = tuple(int(i) for i in np.argwhere(diff)[0]) if diff.any() else None
    return "%d of %d differ: %d NaN cells misplaced, %d NaN of another sign or payload, %d finite; first at %s: %r for %r" % (
        diff.sum(), diff.size, (gn != wn).sum(), (diff & gn & wn).sum(), (diff & ~gn & ~wn).sum(), first,
        got[first] if first is not None else None, want[first] if first is not None else None)


def same(got, want, what):
    COMPARISONS[0] += 1
    assert bits_equal(np.atleast_1d(got), np.atleast_1d(want)), (what, describe(np.atleast_1d(got), np.atleast_1d(want)))


def sel_segs(segs, sel):
    return [segs[i] for i in sel]


# ---------------------------------------------------------------- what the oracle expects of one context (X1, X2, X3)
def single_expect(oracle, segs, case, with_segments=True):
    """{name: array}: the oracle's E-step on the multiset SEL, per segment too, the A0 of each selected segment alone, and the
    tables of the 65-bin and of the longest segment -- after exact_extremes.conditions on that result"""
    a, e, a0 = xx.params(*case)
    sel = sel_segs(segs, xx.SEL)
    o = oracle.estep(a, e, a0, sel, per_seg=True)
    xx.conditions(case, o, sel)
    exp = dict(A=o["A"], E=o["E"], A0=o["A0"], LL=np.float64(o["LL"]), chk=o["seg_chk"])
    if with_segments:
        alone = {i: oracle.estep(a, e, a0, [segs[i]])["A0"] for i in sorted(set(xx.SEL))}
        exp.update(seg_A=o["seg_A"], seg_E=o["seg_E"], seg_LL=o["seg_LL"], seg_A0=np.stack([alone[i] for i in xx.SEL]))
    for k in (xx.SEG65, xx.LONGEST):
        f, b, s, lk, chk = oracle.fwd_bwd(a, e, a0, segs[k])
        exp.update({"f%d" % k: f[1:], "b%d" % k: b[1:], "s%d" % k: s[1:]})
    return exp


def check_estep(r, exp, what):
    """(X1)"""
    for key in ("A", "E", "A0", "LL", "chk"):
        same(r[key], exp[key], (what, "estep", key))


def check_single(es, case, exp, what):
    """(X1), (X2) where exp holds the per-segment values, (X3) on a context that has the segments loaded"""
    a, e, a0 = xx.params(*case)
    es.select(list(xx.SEL))
    check_estep(es.estep(a, e, a0), exp, what)
    if "seg_A" in exp:
        s = es.estep_segments(a, e, a0)
        for key in ("seg_A", "seg_E", "seg_LL", "seg_A0"):
            same(s[key], exp[key], (what, "estep_segments", key))
        same(s["chk"], exp["chk"], (what, "estep_segments", "chk"))
    for k in (xx.SEG65, xx.LONGEST):
        f, b, s = es.tables(k)
        for key, got in (("f", f), ("b", b), ("s", s)):
            same(got, exp["%s%d" % (key, k)], (what, "tables of segment %d" % k, key))


# ---------------------------------------------------------------- X1, X2, X3: one exact context per case
@pytest.mark.parametrize("n,name", xx.cases())
def test_exact_statistics(hip, golden, oracle, n, name):
    segs = xx.segments(golden, n)
    xx.assert_selection(xx.SEL)
    exp = single_expect(oracle, segs, (n, name))
    es = hip.HipEStep(n, mode=hip.MODE_EXACT)
    es.load_segments(segs)
    check_single(es, (n, name), exp, (n, name))
    es.close()


# ---------------------------------------------------------------- X4: the batch
@functools.lru_cache(maxsize=2)
def mild_expect(oracle, golden, n, sel):
    """the lambda_equal replicate is the same in every case of a size"""
    return oracle.estep(*xx.params(n, xx.MILD), sel_segs(xx.segments(golden, n), sel))


@pytest.mark.parametrize("n,name", xx.batch_cases())
def test_exact_batch(hip, golden, oracle, n, name):
    segs = xx.segments(golden, n)
    xx.assert_selection(xx.SEL2)
    reps = [(name, xx.SEL), (xx.MILD, xx.SEL[::-1]), (name, xx.SEL2)]
    want = [oracle.estep(*xx.params(n, name), sel_segs(segs, xx.SEL), per_seg=True), mild_expect(oracle, golden, n, reps[1][1]),
            oracle.estep(*xx.params(n, name), sel_segs(segs, xx.SEL2))]
    xx.conditions((n, name), want[0], sel_segs(segs, xx.SEL))
    if name == "dead_het" and n <= 64:   # exact_refwd = 2: a NaN entry and a finite one in one work-group, in both of its replicates
        assert xx.mixed_pairs(segs, xx.SEL) and xx.mixed_pairs(segs, xx.SEL2), (xx.rf2_pairs(segs, xx.SEL), xx.rf2_pairs(segs, xx.SEL2))
    mild = want[1]
    assert all(np.isfinite(mild[k]).all() for k in ("A", "E", "LL")), "the partner is finite"
    pad = lambda L: (L + 63) // 64 * 64
    total = sum(pad(len(segs[i])) for _, sel in reps for i in sel)
    batch_bins = max(4 * pad(len(segs[xx.LONGEST])), total // 3)   # a block of entries (at most four) has to fit one launch
    for v in ((2, 1, 0) if n <= 64 else (1, 0)):
        opt = dict(exact_refwd=v) if n <= 64 else dict(batch_sort=v)
        es = hip.HipEStep(n, mode=hip.MODE_EXACT, batch_bins=batch_bins, **opt)
        es.load_segments(segs)
        got = es.estep_batch([xx.params(n, m) for m, _ in reps], [list(sel) for _, sel in reps], want="A")
        info = es.batch_info()
        assert info["groups"] >= 2, (info, batch_bins, total)
        for r, w in enumerate(want):
            for key in ("A", "E", "LL"):
                same(got[key][r], w[key], (n, name, opt, "replicate %d (%s)" % (r, reps[r][0]), key))
        es.close()


# ---------------------------------------------------------------- X5: a fast-mode context beyond 128 states
@pytest.mark.parametrize("n,name", xx.FAST_CONTEXT_CASES)
def test_fast_context_runs_the_exact_kernels(hip, golden, oracle, n, name):
    segs = xx.segments(golden, n)
    exp = single_expect(oracle, segs, (n, name), with_segments=False)
    es = hip.HipEStep(n, mode=hip.MODE_FAST)
    es.load_segments(segs)
    es.select(list(xx.SEL))
    check_estep(es.estep(*xx.params(n, name)), exp, (n, name, "MODE_FAST"))
    es.close()


# ---------------------------------------------------------------- X6: the exact group
@pytest.mark.parametrize("n,name", xx.GROUP_CASES)
def test_exact_group(hip, golden, oracle, n, name):
    segs = xx.segments(golden, n)
    a, e, a0 = xx.params(n, name)
    o = oracle.estep(a, e, a0, segs, per_seg=True)   # a group has no selection: the loaded segments in input order
    xx.conditions((n, name), o, segs)
    g = hip.HipGroup(n, [0, 0], mode=hip.MODE_EXACT)
    g.load_segments(segs)
    r = g.estep(a, e, a0)
    assert g.info()["n_shards"] == 2
    check_estep(r, dict(A=o["A"], E=o["E"], A0=o["A0"], LL=np.float64(o["LL"]), chk=o["seg_chk"]), (n, name, "group"))
    g.close()


# ---------------------------------------------------------------- X7: the general wide kernels at the register kernels' sizes
def child_main(npz, n, name):
    """in the child process: (X1) and (X3) against the expectations the parent computed"""
    from conftest import Golden
    from psmc_amd import hip as h
    assert os.environ.get("PSMC_HIP_WIDE_L2") == "1"
    exp = dict(np.load(npz))
    es = h.HipEStep(n, mode=h.MODE_EXACT)
    es.load_segments(xx.segments(Golden(), n))
    check_single(es, (n, name), exp, (n, name, "PSMC_HIP_WIDE_L2=1"))
    es.close()
    print("wide l2 ok: %d comparisons" % COMPARISONS[0])


@pytest.mark.parametrize("n,name", xx.WIDE_L2_CASES)
def test_general_wide_kernels_at_register_kernel_sizes(hip, golden, oracle, tmp_path, n, name):
    segs = xx.segments(golden, n)
    exp = single_expect(oracle, segs, (n, name), with_segments=False)
    npz = str(tmp_path / "expect.npz")
    np.savez(npz, **exp)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_exact_extremes as t; t.child_main(%r, %d, %r)" % (
        ROOT, os.path.join(ROOT, "tests"), npz, n, name)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, PSMC_HIP_WIDE_L2="1"), timeout=300)
    assert r.returncode == 0 and "wide l2 ok: 11 comparisons" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])
