"""The CPU side of the exact E-step's gate at the model extremes (tests/test_gpu_exact_extremes.py): the oracle against the real
reference's bits under the extreme models and the synthetic matrices (tests/golden/exact_extremes.npz: 64, 65 and 200 states), the
conditions that keep a case of the gate from passing by accident, on every case of it, and the case table itself."""
import os
import sys
import numpy as np
import pytest
from conftest import GOLD

import exact_extremes as xx

sys.path.insert(0, GOLD)
import make_golden_exact_extremes as mg


@pytest.fixture(scope="module")
def gold_x():
    return dict(np.load(os.path.join(GOLD, "exact_extremes.npz")))


def full(oracle, golden, n, name):
    segs = xx.segments(golden, n)
    return oracle.estep(*xx.params(n, name), segs, per_seg=True), segs


def test_golden_holds_the_expected_cases(gold_x):
    want = [mg.case_name(n, name) for n in (64, 65, 200) for name in xx.case_names(n)]
    assert [str(c) for c in gold_x["cases"]] == want and len(want) == 3 * 17
    assert sorted(gold_x) == sorted(["cases"] + ["%s.%s" % (c, k) for c in want for k in mg.KEYS + ("A_sha256", "seg_A_sha256")])
    assert all(gold_x["%s.%s" % (c, k)].dtype == np.uint64 for c in want for k in mg.KEYS)
    assert os.path.getsize(os.path.join(GOLD, "exact_extremes.npz")) < 400 << 10


@pytest.mark.parametrize("n,name", xx.cases(xx.GOLDEN_SIZES))
def test_oracle_reproduces_the_reference(oracle, golden, gold_x, n, name):
    """every double of E, A0, LL, seg_LL and seg_chk, NaN signs included, and A and seg_A through their SHA-256"""
    o, segs = full(oracle, golden, n, name)
    for key, want in mg.record(mg.case_name(n, name), o).items():
        assert np.array_equal(want, gold_x[key]), key


def test_maker_reproduces_the_golden_file(tmp_path):
    """where oracle/_ref is built: the maker writes the committed file again, byte for byte"""
    import orc
    if not orc.have_reference():
        pytest.skip("oracle/_ref is not built (no reference checkout)")
    before = open(os.path.join(GOLD, "exact_extremes.npz"), "rb").read()
    here, mg.HERE = mg.HERE, str(tmp_path)
    try:
        mg.main()
    finally:
        mg.HERE = here
    assert open(str(tmp_path / "exact_extremes.npz"), "rb").read() == before


@pytest.mark.parametrize("n,name", xx.all_cases())
def test_conditions_hold_on_every_case(oracle, golden, n, name):
    """every case of every part of the gate, (X5) to (X7) at 150 and 200 states included: on the loaded segments and, below 1024
    states (the oracle's time), on the gate's multiset as well; what the case holds is printed (-s)"""
    xx.assert_selection(xx.SEL)
    xx.assert_selection(xx.SEL2)
    o, segs = full(oracle, golden, n, name)
    rec = xx.conditions((n, name), o, segs)
    print("n %4d %-28s NaN %8d  negative cells of A %4d  zeros of A0 %3d  NaN segments %s" % (
        n, name, rec["nan"], rec["negative"], rec["zero_A0"], rec.get("nan_segments", "-")))
    if n < 1024:   # the multiset's own pass: the gate asserts it again before it asks the device
        sel = [segs[i] for i in xx.SEL]
        xx.conditions((n, name), oracle.estep(*xx.params(n, name), sel, per_seg=True), sel)
    if name in xx.NAN_MODELS and n >= 23:
        assert rec["nan"] > 0 and np.isnan(xx.params(n, name)[0]).any(), (n, name)
    if name == "rho_0.5" and n >= 23:
        assert (xx.params(n, name)[0] < 0).any(), (n, name)


@pytest.mark.parametrize("n", [n for n in xx.SIZES if n <= 64])
def test_rf2_pairs_hold_a_nan_and_a_finite_segment(oracle, golden, n):
    """Under "dead het" both multisets of the batch put a segment with a het bin and one without into one work-group of
    k_expect_exact_rf2, and the oracle says the first is NaN and the second finite; the pairing is the host's (api_batch.hip)."""
    segs = xx.segments(golden, n)
    o = oracle.estep(*xx.params(n, "dead_het"), segs, per_seg=True)
    for sel in (xx.SEL, xx.SEL2):
        pairs = xx.rf2_pairs(segs, sel)
        assert sorted(i for p in pairs for i in p if i is not None) == sorted(set(sel))
        assert all(y is None or len(segs[x]) >= len(segs[y]) for x, y in pairs)
        mixed = xx.mixed_pairs(segs, sel)
        assert mixed, pairs
        for x, y in mixed:
            assert np.isnan(o["seg_LL"][x]) != np.isnan(o["seg_LL"][y]), (x, y)
            assert np.isnan(o["seg_A"][x]).all() != np.isnan(o["seg_A"][y]).all(), (x, y)
    lens = [len(s) for s in segs]
    assert xx.rf2_pairs(segs, (0, 5, 5, 8, 3)) == [(8, 5), (3, 0)] and xx.rf2_pairs(segs, (4, 1, 4, 2, 8, 0, 3)) == [(8, 4), (3, 1), (2, 0)], lens
    assert xx.rf2_pairs(segs, (8, 3, 5)) == [(8, 5), (3, None)]


def test_case_table():
    assert xx.FAMILIES == {"wave64": (2, 3, 23, 63, 64), "exact128": (65, 100, 127, 128),
                           "register": (129, 192, 193, 208, 209, 224), "general": (225, 256, 300, 513, 1024)}
    assert xx.SIZES == (2, 3, 23, 63, 64, 65, 100, 127, 128, 129, 192, 193, 208, 209, 224, 225, 256, 300, 513, 1024)
    from test_gpu_wide_cells import LARGE_MODELS
    from test_gpu_wide_fast_edges import MODELS, SIZES as one_wave
    from test_gpu_wide_fast_mw import SIZES as multi_wave
    assert len(MODELS) == 13 and set(xx.NON_HMM) <= set(MODELS) and set(xx.NAN_MODELS) <= set(xx.NON_HMM) and xx.MILD in MODELS
    for n in xx.SIZES:
        names = xx.case_names(n)
        assert names[-4:] == ["clamp", "upper_half", "dead_het", "inf_row"]
        if n <= 256:
            assert names[:-4] == list(MODELS)
        else:
            assert sorted(names[:-4]) == sorted(LARGE_MODELS + xx.NON_HMM) and len(names) == 11
        pat, m = xx.pattern(n)
        assert (pat, m) == (one_wave[n] if n in one_wave else multi_wave[n] if n in multi_wave else ("%d*1" % n, n))
    assert len(xx.cases()) == 17 * 17 + 3 * 11
    assert xx.all_cases()[:len(xx.cases())] == xx.cases() and sorted({n for n, _ in xx.all_cases()[len(xx.cases()):]}) == [150, 200]
    assert len(xx.all_cases()) == 322 + 4 + 3 and set(xx.FAST_CONTEXT_CASES + xx.GROUP_CASES + xx.WIDE_L2_CASES) <= set(xx.all_cases())
    assert [c for c in xx.cases() if c not in xx.batch_cases()] == [(n, name) for n in (513, 1024) for name in xx.case_names(n)
                                                                   if name not in ("lambda_equal", "rho_0.5", "dead_het")]
    assert xx.BREAKS_DOWN == ((2, "lambda_ramp_up_1e-3_1e3"), (3, "lambda_ramp_up_1e-3_1e3"))
    assert xx.long_bins(513) == 700 and xx.long_bins(1024) == 200 and xx.EXTRA_BINS == (16, 17, 33, 129)


def test_synthetic_matrices():
    """seeded by n; what each is for, on the parameters themselves"""
    for n in xx.SIZES:
        a, e, a0 = xx.params(n, "clamp")
        assert (a[0, 1::2] < 0).all() and (a[1:] > 0).all()
        a, e, a0 = xx.params(n, "upper_half")
        assert int((a0 == 0).sum()) == n // 2 and (a[:n // 2, n // 2:] == 0).all()
        a, e, a0 = xx.params(n, "dead_het")
        assert (e[1] == 0).all() and (e[0] == 1).all() and (e[2] == 1).all()
        a, e, a0 = xx.params(n, "inf_row")
        assert np.isposinf(a[n // 3]).all() and np.isfinite(np.delete(a, n // 3, axis=0)).all()
        assert all(np.array_equal(xx.params(n, "dead_het")[k], xx.params(n, "inf_row")[k]) for k in (2,))
