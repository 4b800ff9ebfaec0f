"""Cases shared by the gate of the exact E-step at the model extremes (tests/test_gpu_exact_extremes.py), its CPU side
(tests/test_exact_extremes_model.py) and the maker of its golden (tests/golden/make_golden_exact_extremes.py): the state counts by
kernel family, the thirteen extreme PSMC models and four synthetic matrices at each, the short and ragged data, the bootstrap
multisets, and the conditions that keep a case from passing by accident.  TEST INFRASTRUCTURE, CPU only: nothing here touches a
device."""
import hashlib
import numpy as np

import path_extremes as px

# states by the kernel family that runs them (psmc_amd/csrc/estep_exact.hip, estep_wide.hip)
FAMILIES = {
    "wave64": (2, 3, 23, 63, 64),                     # up to 64 states: one wave, padded to 64
    "exact128": (65, 100, 127, 128),                  # 65 .. 128: k_*_exact128
    "register": (129, 192, 193, 208, 209, 224),       # 129 .. 224: register kernels, C = 96 / 104 / 112
    "general": (225, 256, 300, 513, 1024),            # 225 and up: general kernels, the matrix from the L2
}
SIZES = tuple(n for fam in FAMILIES.values() for n in fam)
GOLDEN_SIZES = (64, 65, 200)
FULL_TABLE_MAX = 256          # up to here all thirteen models; beyond: LARGE_MODELS and the three that are no HMM
NON_HMM = ("lambda_alt_1e-3_1e3", "lambda_ramp_down_1e3_1e-3", "rho_0.5")
NAN_MODELS = px.NAN_MODELS
# The host model itself breaks down under the steepest upward ramp at two and three states (e and a hold NaN, all negative, a0 is
# (1, 0 ..)): the reference's answer there is NaN in every cell, like under NAN_MODELS from 23 states on, and is gated as such.
# Of NAN_MODELS, lambda_alt_1e-3_1e3 is NaN at these two sizes as well and lambda_ramp_down_1e3_1e-3 is finite there.
BREAKS_DOWN = ((2, "lambda_ramp_up_1e-3_1e3"), (3, "lambda_ramp_up_1e-3_1e3"))
SYNTHETIC = ("clamp", "upper_half", "dead_het", "inf_row")
MILD = "lambda_equal"         # the finite partner of the batch cases
BATCH_FEW_ABOVE = 300         # beyond: the batch under BATCH_FEW only (the oracle's time)
BATCH_FEW = (MILD, "rho_0.5", "dead_het")

# of the thirteen segments of segments(): 8 (the longest) three times, 5 (65 bins) twice, 7 left out / 4 three times, 6 twice, 5 left out
SEL = (8, 3, 12, 8, 0, 5, 10, 1, 5, 8, 2, 4, 6, 9, 11)
SEL2 = (11, 4, 4, 9, 0, 8, 12, 4, 2, 6, 6, 1, 3, 10, 7)
SEG65, LONGEST = 5, 8
EXTRA_BINS = (16, 17, 33, 129)   # 16: the block of k_expect_exact and the ring half of the recompute kernels


def pattern(n):
    """(pattern, free lambdas) of n states: the one the suite already uses where the size has one, else "<n>*1" (a group repeats
    at most 255 times)"""
    from test_gpu_wide_fast_edges import SIZES as one_wave
    from test_gpu_wide_fast_mw import SIZES as multi_wave
    if n in one_wave:
        return one_wave[n]
    if n in multi_wave:
        return multi_wave[n]
    assert n <= 255, n
    return "%d*1" % n, n


def model_names(n):
    from test_gpu_wide_cells import LARGE_MODELS
    names = px.model_names()
    if n <= FULL_TABLE_MAX:
        return names
    return [m for m in names if m in LARGE_MODELS or m in NON_HMM]


def case_names(n):
    return model_names(n) + list(SYNTHETIC)


# the cases of the gate's smaller parts: (X5) a fast-mode context, (X6) the exact group, (X7) the general wide kernels
ONE_NAN_MODEL = "lambda_alt_1e-3_1e3"
FAST_CONTEXT_CASES = [(n, name) for n in (150, 300) for name in ("rho_0.5", "lambda_ramp_down_1e2_1e-2", ONE_NAN_MODEL, "dead_het")]
GROUP_CASES = [(n, name) for n in (64, 128, 200) for name in ("rho_0.5", ONE_NAN_MODEL, "dead_het")]
WIDE_L2_CASES = [(n, name) for n in (129, 200, 224) for name in ("rho_0.5", ONE_NAN_MODEL, "dead_het")]


def cases(sizes=SIZES):
    return [(n, name) for n in sizes for name in case_names(n)]


def all_cases():
    """every (n, case) some part of the gate runs: cases() and what (X5), (X6), (X7) add at 150 and 200 states"""
    out = cases()
    return out + [c for c in dict.fromkeys(FAST_CONTEXT_CASES + GROUP_CASES + WIDE_L2_CASES) if c not in out]


def batch_cases():
    return [(n, name) for n, name in cases() if n <= BATCH_FEW_ABOVE or name in BATCH_FEW]


_PARAMS = {}


def params(n, name):
    """(a (n, n), e (3, n), a0 (n,)) of a case: computed once, shared, never changed.  The synthetic matrices are seeded by n."""
    key = (n, name)
    if key in _PARAMS:
        return _PARAMS[key]
    if name in SYNTHETIC:
        rng = np.random.default_rng(n)
        if name == "clamp":
            a, e, a0 = px.clamp_hmm(n, 3.0, rng)
        elif name == "upper_half":
            a, e, a0 = px.upper_half_hmm(n, rng)
        else:
            a, e, a0 = px.subnormal_hmm(n, rng)
        e3 = np.ones((3, n))
        e3[:2] = e
        if name == "dead_het":      # 0 / 0 at the first het bin of a segment
            e3[0], e3[1] = 1.0, 0.0
        if name == "inf_row":       # inf * 0 wherever the forward vector has a zero
            a[n // 3, :] = np.inf
        par = (a, e3, a0)
    else:
        from psmc_amd import hostlib
        from test_gpu_wide_fast_edges import MODELS
        pat, m = pattern(n)
        par = hostlib.hmm_params(pat, MODELS[name](m))
    par = tuple(np.ascontiguousarray(x, dtype=np.float64) for x in par)
    assert par[0].shape == (n, n) and par[1].shape == (3, n) and par[2].shape == (n,), (n, name)
    for x in par:
        x.setflags(write=False)
    _PARAMS[key] = par
    return par


def long_bins(n):
    return 200 if n >= 1024 else 700


def segments(golden, n):
    """path_extremes.short_segs (1, 3, 2, 63, 64, 65, 70, 32 and long_bins(n) bins) and four more slices of 16, 17, 33 and 129
    bins, cut as short_segs cuts: L bins with a het (even i) or a missing (odd i) bin of the fixture data at bin i % L"""
    src = golden.segs_mid[0]

    def cut(i, L):
        p = int(np.flatnonzero(src[1000 * i:] == 1 + i % 2)[0]) + 1000 * i - i % L
        return src[p:p + L]
    segs = px.short_segs(golden, long_bins(n)) + [cut(6 + k, L) for k, L in enumerate(EXTRA_BINS)]
    assert [len(s) for s in segs[9:]] == list(EXTRA_BINS) and len(segs) == 13 and len(segs[SEG65]) == 65
    assert len(segs[LONGEST]) == max(len(s) for s in segs) and sum(len(s) for s in segs) == 495 + long_bins(n)
    return segs


def rf2_pairs(segs, sel):
    """The pairs of segments that share a work-group of k_expect_exact_rf2 (its LDS rings, its consumer waves) when a replicate
    with the multiset `sel` runs in the batch at up to 64 states, as psmc_amd/csrc/api_batch.hip batch_exact deals them: the
    replicate's distinct segments in the order of their first occurrence, a stable sort by length, longest first ("batch_sort" =
    1), blocks of four, and in a block the entries 0 and 1, 2 and 3.  A work-group never holds entries of two replicates.  An entry
    without a partner is paired with None."""
    work = list(dict.fromkeys(int(i) for i in sel))
    order = sorted(work, key=lambda i: -len(segs[i]))   # sorted() is stable
    pairs = []
    for b in range(0, len(order), 4):
        block = order[b:b + 4]
        for k in range(0, len(block), 2):
            pairs.append((block[k], block[k + 1] if k + 1 < len(block) else None))
    return pairs


def mixed_pairs(segs, sel):
    """the pairs of rf2_pairs that hold a segment with a het bin and one without: under "dead het" a NaN entry beside a finite one"""
    het = [bool((s == 1).any()) for s in segs]
    return [(x, y) for x, y in rf2_pairs(segs, sel) if y is not None and het[x] != het[y]]


def assert_selection(sel, n_seg=13):
    """a multiset with one segment three times, one twice and one loaded segment left out, in a non-monotonic order"""
    count = np.bincount(sel, minlength=n_seg)
    assert len(count) == n_seg and sorted(count)[-3:] == [1, 2, 3] and sorted(count)[:2] == [0, 1], count
    d = np.diff(sel)
    assert (d > 0).any() and (d < 0).any(), sel


def is_neg_nan(x):
    x = np.asarray(x, dtype=np.float64)
    return np.isnan(x) & np.signbit(x)


def result_arrays(o):
    return [np.asarray(o[k], dtype=np.float64) for k in ("A", "E", "A0", "LL", "seg_A", "seg_E", "seg_LL", "seg_chk")]


def conditions(case, o, segs):
    """The conditions that keep case = (n, name) from passing by accident, asserted on o = the oracle's per-segment E-step on the
    loaded segments, before a device is asked.  Returns a short record of what the case holds."""
    n, name = case
    a, e, a0 = params(n, name)
    for x in (a, e, a0):   # the NaN rule's premise: x86 gives a NaN it makes the sign bit and keeps a propagated NaN's sign
        assert not (np.isnan(x) & ~np.signbit(x)).any(), (case, "a parameter is a positive NaN")
    arrays = result_arrays(o)
    nans = sum(int(np.isnan(x).sum()) for x in arrays)
    rec = dict(nan=nans, negative=int((o["A"] < 0).sum()), zero_A0=int((o["A0"] == 0).sum()))
    for x in arrays:
        assert (is_neg_nan(x) == np.isnan(x)).all(), (case, "a NaN of the reference is positive")
    if name == "clamp":
        assert (o["A"] < 0).any(), case
    elif name == "upper_half":
        assert int((o["A0"] == 0).sum()) == n // 2, case
    elif name == "dead_het":
        het = np.array([bool((s == 1).any()) for s in segs])
        seg_nan = np.isnan(o["seg_LL"])
        assert np.array_equal(seg_nan, het) and het.any() and not het.all(), (case, seg_nan, het)
        assert np.array_equal(np.isnan(o["seg_chk"]), het), case
        assert all(np.isnan(o["seg_A"][i]).all() if h else np.isfinite(o["seg_A"][i]).all() for i, h in enumerate(het)), case
        rec["nan_segments"] = int(het.sum())
    elif name == "inf_row":
        assert nans > 0, case
    elif name in NAN_MODELS or case in BREAKS_DOWN:
        assert np.isnan(a).any() or (name in NAN_MODELS and n < 23), (case, "the matrix holds no NaN")
        if np.isnan(a).any():
            assert np.isnan(o["A"]).all() and np.isnan(o["E"]).all(), case
        else:
            assert nans == 0, case
    else:   # the ten HMM models and rho_0.5
        assert all(np.isfinite(x).all() for x in (a, e, a0)), (case, "a parameter is not finite")
        assert all(np.isfinite(x).all() for x in arrays), (case, "not finite")
    return rec


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x, dtype=np.float64).tobytes()).hexdigest()


def bits(x):
    return np.ascontiguousarray(np.atleast_1d(np.asarray(x, dtype=np.float64))).view(np.uint64)
