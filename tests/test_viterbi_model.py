"""The numpy restatement of the Viterbi arithmetic (tests/viterbi_model.py) against the reference's hmm_Viterbi: every
golden of tests/golden/viterbi.npz bit for bit, and -- where oracle/_ref is built -- the live reference on a fresh case."""
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
