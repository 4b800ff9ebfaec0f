"""The numpy restatement of the Viterbi arithmetic (tests/viterbi_model.py) against the reference's hmm_Viterbi: every
golden of tests/golden/viterbi.npz and of tests/golden/viterbi_extremes.npz (the extreme PSMC models at 64, 65 and 200 states) bit
for bit, and -- where oracle/_ref is built -- the live reference on a fresh case."""
import os
import sys
import numpy as np
import pytest
from conftest import GOLD, ROOT

import viterbi_model as vm

SETS = ["n23_curve", "n64_flat", "n128_curve", "n149", "n200"]


def load_sets():
    g = lambda f: np.load(os.path.join(GOLD, f))
    hp, n128, wide = g("hmm_params.npz"), g("estep_n128.npz"), g("estep_wide.npz")
    src = dict(n23_curve=hp, n64_flat=hp, n128_curve=n128, n149=wide, n200=wide)
    return {k: (src[k][k + ".a"], src[k][k + ".e"], src[k][k + ".a0"]) for k in SETS}


def golden_segments():
    mid, small = np.load(os.path.join(GOLD, "segments_mid.npz")), np.load(os.path.join(GOLD, "segments_small.npz"))
    out = {"mid_" + k: mid[k][:20000] for k in sorted(mid.files)}
    out.update({"small_" + k: small[k] for k in sorted(small.files)})
    return out


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "viterbi.npz"))


@pytest.mark.parametrize("name", SETS)
def test_model_reproduces_goldens(gold, name):
    a, e, a0 = load_sets()[name]
    tables = vm.log_tables(a, e, a0)
    segs = golden_segments()
    assert len(segs) == 19 and sorted(len(s) for s in segs.values())[:6] == [1, 2, 3, 63, 64, 65]
    n_runs = 0
    for sname, seq in segs.items():
        path, score = vm.viterbi(tables, seq)
        want = gold["%s.%s.path" % (name, sname)]
        assert want.dtype == np.int16 and np.array_equal(path, want), (name, sname)
        assert np.float64(score).view(np.uint64) == gold["%s.%s.score" % (name, sname)].view(np.uint64), (name, sname)
        n_runs = max(n_runs, len(vm.runs(path)))
    assert n_runs >= 4  # the goldens are paths, not constants


def extreme_cases():
    """[(case, n, model)] of tests/golden/viterbi_extremes.npz, from the file's own list"""
    cases = [str(c) for c in np.load(os.path.join(GOLD, "viterbi_extremes.npz"))["cases"]]
    return [(c, int(c.split(".", 1)[0][1:]), c.split(".", 1)[1]) for c in cases]


def extreme_golden(gold_x, case, segs):
    """(paths [int16 views of the file's array], scores) of one case, cut by the segments' lengths"""
    path, score = gold_x[case + ".path"], gold_x[case + ".score"]
    ends = np.cumsum([len(s) for s in segs.values()])
    assert path.dtype == np.int16 and len(path) == ends[-1] and score.shape == (len(segs),) and score.dtype == np.float64
    return [path[end - len(s):end] for end, s in zip(ends, segs.values())], score


def test_extreme_goldens_are_the_expected_cases():
    """11 of the 13 models at each of 64, 65 and 200 states: all but the two whose matrix holds NaN, on which the reference's assert fires"""
    import path_extremes as px
    gold_x = np.load(os.path.join(GOLD, "viterbi_extremes.npz"))
    want = ["n%d.%s" % (n, name) for n in px.GOLDEN_SIZES for name in px.model_names() if name not in px.NAN_MODELS]
    assert [c for c, _, _ in extreme_cases()] == want and len(want) == 33
    assert [str(s) for s in gold_x["segments"]] == list(px.golden_segments())
    segs = px.golden_segments()
    for n in px.GOLDEN_SIZES:   # the goldens are paths, not constants
        n_runs = {name: len(vm.runs(extreme_golden(gold_x, "n%d.%s" % (n, name), segs)[0][-1])) for c, m, name in extreme_cases() if m == n}
        assert sum(r >= 4 for r in n_runs.values()) >= 8 and all(r >= 2 for name, r in n_runs.items() if name != "tmax_0.5"), n_runs


@pytest.mark.parametrize("case,n,name", extreme_cases())
def test_model_reproduces_extreme_goldens(case, n, name):
    """The restatement against the real hmm_Viterbi at the model extremes, paths and score bits, as the goldens stand.  rho_0.5 has
    negative entries in a: libm's log gives NaN there, viterbi_model._log gives -inf, and the golden -- made with libm's NaN -- is
    reproduced all the same: neither a NaN candidate nor a -inf one ever passes `m < c`."""
    import path_extremes as px
    a, e, a0 = px.extreme_model(name, n)
    if name == "rho_0.5":
        assert (a < 0).any() and np.isfinite(a).all()
    gold_x = np.load(os.path.join(GOLD, "viterbi_extremes.npz"))
    segs = px.golden_segments()
    want_paths, want_scores = extreme_golden(gold_x, case, segs)
    tables = vm.log_tables(a, e, a0)
    for i, (sname, seq) in enumerate(segs.items()):
        path, score = vm.viterbi(tables, seq)
        assert np.array_equal(path, want_paths[i]), (case, sname)
        assert np.float64(score).view(np.uint64) == want_scores[i].view(np.uint64), (case, sname)


@pytest.mark.parametrize("n", [64, 65, 200])
def test_nan_models_have_no_finite_path(n):
    """the two cases per size the goldens leave out: no state at position 2 has a predecessor (a segment of one bin still has a path)"""
    import path_extremes as px
    for name in px.NAN_MODELS:
        a, e, a0 = px.extreme_model(name, n)
        assert np.isnan(a).any()
        tables = vm.log_tables(a, e, a0)
        with pytest.raises(vm.NoFinitePath, match="position 2"):
            vm.viterbi(tables, np.array([0, 0, 1, 0], dtype=np.uint8))
        vm.viterbi(tables, np.array([0], dtype=np.uint8))


def test_no_finite_path_raises():
    a, e, a0 = load_sets()["n23_curve"]
    e = e.copy()
    e[1] = 0.0
    with pytest.raises(vm.NoFinitePath):
        vm.viterbi(vm.log_tables(a, e, a0), np.array([0, 0, 1, 0, 0], dtype=np.uint8))
    vm.viterbi(vm.log_tables(a, e, a0), np.array([0, 2, 0], dtype=np.uint8))


def test_model_against_live_reference():
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libpsmc_ref.so")):
        pytest.skip("oracle/_ref is not built (no reference checkout)")
    sys.path.insert(0, GOLD)
    import make_golden_viterbi as mg
    lib = mg.load_ref()
    rng = np.random.default_rng(20261020)
    n, L = 37, 3000
    a = rng.random((n, n)) ** 4 + np.eye(n)
    a /= a.sum(1, keepdims=True)
    e = np.zeros((2, n))
    e[1] = np.exp(np.linspace(np.log(0.002), np.log(0.6), n))
    e[0] = 1.0 - e[1]
    a0 = rng.random(n)
    a0 /= a0.sum()
    rate = np.repeat(rng.choice([0.01, 0.1, 0.4], size=L // 40), 40)
    seq = (rng.random(L) < rate).astype(np.uint8)
    seq[rng.random(L) < 0.03] = 2
    path, score = vm.viterbi(vm.log_tables(a, e, a0), seq)
    rpath, rscore = mg.ref_viterbi(lib, a, e, a0, seq)
    assert np.array_equal(path, rpath)
    assert np.float64(score).view(np.uint64) == np.float64(rscore).view(np.uint64)
    assert len(vm.runs(path)) >= 4
