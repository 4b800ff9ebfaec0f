"""psmc_hip_viterbi on the device: the reference's hmm_Viterbi bit for bit (tests/golden/viterbi.npz, made by
tests/golden/make_golden_viterbi.py from the real khmm.c) and the numpy restatement of the pinned arithmetic
(tests/viterbi_model.py) at every width the kernels treat differently -- 64 / 128 / 192 padded states with the matrix in
registers, the streamed kernel beyond, one or two bytes per back-pointer -- across backtrace tile boundaries, with ties,
and without touching anything else of the context."""
import ctypes as C
import os
import numpy as np
import pytest
from conftest import GOLD

import viterbi_model as vm
from test_viterbi_model import SETS, golden_segments, load_sets

pytestmark = pytest.mark.gpu

DEFAULT_TILE = 2048
TILES = [None, 16, 64]  # None: the default
WIDTHS = [1, 2, 3, 23, 63, 64, 65, 127, 128, 129, 192, 224, 225, 256, 257, 512, 513, 1024]


def seg_lengths(n):
    """1, 2 and T - 1, T, T + 1, 2 T + 1 for every tile length tried; the longest 4097 up to 128 states, 600 beyond"""
    cap = 4097 if n <= 128 else 600
    ls = {1, 2, cap}
    for t in (16, 64, DEFAULT_TILE):
        ls |= {t - 1, t, t + 1, 2 * t + 1}
    return sorted(l for l in ls if l <= cap)


def banded_hmm(n, rng):
    """a banded random matrix with 0.6 on the diagonal (zeros -- log 0 = -inf -- outside the band), het rates rising
    log-uniformly from 0.002 to 0.6 with the state index"""
    if n == 1:
        return np.ones((1, 1)), np.array([[0.9], [0.1]]), np.ones(1)
    band = max(1, n // 4)  # (a narrower band freezes the path at 513 states: the way across the het rates gets too many hops)
    k = np.arange(n)
    off = rng.random((n, n)) * ((np.abs(k[:, None] - k[None, :]) <= band) & (k[:, None] != k[None, :]))
    a = 0.4 * off / off.sum(1, keepdims=True) + 0.6 * np.eye(n)
    e = np.zeros((2, n))
    e[1] = np.exp(np.linspace(np.log(0.002), np.log(0.6), n))
    e[0] = 1.0 - e[1]
    a0 = rng.random(n) + 0.5
    return a, e, a0 / a0.sum()


def block_data(L, rng):
    """blocks of 40 bins with het rates 0.01 / 0.1 / 0.4, 3 % missing"""
    rate = np.repeat(rng.choice([0.01, 0.1, 0.4], size=L // 40 + 1), 40)[:L]
    seq = (rng.random(L) < rate).astype(np.uint8)
    seq[rng.random(L) < 0.03] = 2
    return seq


_CASES = {}


def case(n):
    """(a, e, a0, segments, reference paths, reference scores) of width n: computed once, shared, never changed"""
    if n not in _CASES:
        for attempt in range(12):  # the first seed whose REFERENCE path moves (the test asserts it): the longest segment is the last
            rng = np.random.default_rng(7000 + n + 100000 * attempt)
            a, e, a0 = banded_hmm(n, rng)
            segs = [block_data(L, rng) for L in seg_lengths(n)]
            tables = vm.log_tables(a, e, a0)
            last = vm.viterbi(tables, segs[-1])
            if n < 3 or (len(vm.runs(last[0])) >= 5 and len(set(last[0].tolist())) >= min(n, 4)):
                break
        ref = [vm.viterbi(tables, s) for s in segs[:-1]] + [last]
        for x in (a, e, a0, *segs, *(p for p, _ in ref)):
            x.setflags(write=False)
        _CASES[n] = (a, e, a0, segs, [p for p, _ in ref], np.array([s for _, s in ref]))
    return _CASES[n]


def ctx(n, mode, segs, **opts):
    from psmc_amd import hip
    h = hip.HipEStep(n, mode=mode, **opts)
    h.load_segments(segs)
    return h


def same_bits(x, y):
    return np.array_equal(np.asarray(x, dtype=np.float64).view(np.uint64), np.asarray(y, dtype=np.float64).view(np.uint64))


def check(paths, scores, ref_paths, ref_scores, what):
    for i, (p, r) in enumerate(zip(paths, ref_paths)):
        assert p.dtype == np.int32 and np.array_equal(p, r), (what, "segment", i, "first difference at", int(np.flatnonzero(p != r)[0]) if len(p) == len(r) else -1)
    assert same_bits(scores, ref_scores), (what, scores, ref_scores)


# ---- (a) the reference's own bits
@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("name", SETS)
def test_goldens(name, mode):
    from psmc_amd import hip
    gold = np.load(os.path.join(GOLD, "viterbi.npz"))
    a, e, a0 = load_sets()[name]
    segs = golden_segments()
    h = ctx(len(a0), hip.MODE_EXACT if mode == "exact" else hip.MODE_FAST, list(segs.values()))
    paths, scores = h.viterbi(a, e, a0)
    check(paths, scores, [gold["%s.%s.path" % (name, s)].astype(np.int32) for s in segs],
          np.array([gold["%s.%s.score" % (name, s)] for s in segs]), (name, mode))


# ---- (b) the restatement, every width and tile length
@pytest.mark.parametrize("n", WIDTHS)
def test_against_restatement(n):
    from psmc_amd import hip
    a, e, a0, segs, ref_paths, ref_scores = case(n)
    if n >= 3:  # a constant output cannot pass: the reference path itself moves
        longest = ref_paths[int(np.argmax([len(s) for s in segs]))]
        assert len(vm.runs(longest)) >= 4 and len(set(longest.tolist())) >= 3, (len(vm.runs(longest)), set(longest.tolist()))
    assert (np.concatenate(segs) == 2).any()
    h = ctx(n, hip.MODE_FAST if n % 2 else hip.MODE_EXACT, segs)
    for tile in TILES:
        if tile is not None:
            h.set_option("vit_tile", tile)
        paths, scores = h.viterbi(a, e, a0)
        check(paths, scores, ref_paths, ref_scores, (n, tile))


# ---- (c) ties
@pytest.mark.parametrize("n", [5, 64, 65, 200])
def test_uniform_hmm_gives_state_zero(n):
    from psmc_amd import hip
    a = np.full((n, n), 1.0 / n)
    e = np.vstack([np.full(n, 0.9), np.full(n, 0.1)])
    a0 = np.full(n, 1.0 / n)
    rng = np.random.default_rng(n)
    segs = [block_data(L, rng) for L in (1, 2, 17, 300)]
    h = ctx(n, hip.MODE_EXACT, segs, vit_tile=16)
    paths, scores = h.viterbi(a, e, a0)
    tables = vm.log_tables(a, e, a0)
    for p, s, seq in zip(paths, scores, segs):
        assert not p.any()
        assert same_bits(s, vm.viterbi(tables, seq)[1])


@pytest.mark.parametrize("n", [64, 130, 400])
def test_duplicated_states_resolve_to_the_lower_copy(n):
    from psmc_amd import hip
    m = n // 2
    rng = np.random.default_rng(900 + n)
    a, e, a0 = banded_hmm(m, rng)
    a2, e2, a02 = np.tile(a, (2, 2)) / 2, np.tile(e, (1, 2)), np.tile(a0, 2) / 2
    segs = [block_data(L, rng) for L in (33, 600)]
    tables = vm.log_tables(a2, e2, a02)
    ref = [vm.viterbi(tables, s) for s in segs]
    assert all(p.max() < m for p, _ in ref) and len(vm.runs(ref[1][0])) >= 4
    h = ctx(n, hip.MODE_FAST, segs, vit_tile=64)
    paths, scores = h.viterbi(a2, e2, a02)
    check(paths, scores, [p for p, _ in ref], np.array([s for _, s in ref]), n)


# ---- (d) nothing else matters: the tile length, the mode, an E-step before
def test_independent_of_tile_mode_and_history(golden):
    from psmc_amd import hip
    p = golden.params("n64_curve")
    a, e, a0 = p["a"], p["e"], p["a0"]
    segs = [s[:6000] for s in golden.segs_mid] + golden.segs_small[:9]
    base = None
    for mode in (hip.MODE_EXACT, hip.MODE_FAST):
        for tile, estep_first in ((None, False), (16, False), (1000, True), (16777216, False)):
            h = ctx(64, mode, segs)
            if tile is not None:
                h.set_option("vit_tile", tile)
            if estep_first:
                h.estep(a, e, a0)
            got = h.viterbi(a, e, a0)
            if base is None:
                base = got
                assert len(vm.runs(base[0][0])) >= 4
            check(got[0], got[1], base[0], base[1], (mode, tile, estep_first))


# ---- (e) the call reads the observations only
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_leaves_the_context_alone(golden, mode):
    from psmc_amd import hip
    p = golden.params("n64_curve")
    q = golden.params("n64_flat")
    a, e, a0 = p["a"], p["e"], p["a0"]
    segs = golden.segs_small
    opts = dict(fuse=0) if mode == "fast" else {}

    def run(with_viterbi):
        h = ctx(64, hip.MODE_FAST if mode == "fast" else hip.MODE_EXACT, segs, **opts)
        out = [h.estep(a, e, a0)]
        if with_viterbi:
            h.viterbi(q["a"], q["e"], q["a0"])  # other parameters than the E-step's: nothing of them may stay behind
        for seg in (8, 9):
            out.append(h.decode(seg))
            out.append(h.posterior(seg))
        out.append(h.estep(a, e, a0))
        return out

    def flat(x):
        if isinstance(x, dict):
            return [x[k] for k in sorted(x)]
        return list(x) if isinstance(x, (tuple, list)) else [x]

    for x, y in zip(run(False), run(True)):
        for u, v in zip(flat(x), flat(y)):
            u, v = np.asarray(u), np.asarray(v)
            assert u.shape == v.shape and u.tobytes() == v.tobytes()


# ---- (f) scores without a path
def test_scores_without_a_path():
    from psmc_amd import hip
    a, e, a0, segs, ref_paths, ref_scores = case(65)
    h = ctx(65, hip.MODE_EXACT, segs)
    paths, scores = h.viterbi(a, e, a0, want_path=False)
    assert paths is None and same_bits(scores, ref_scores)


# ---- (g) error returns
def test_error_returns(golden):
    from psmc_amd import hip
    p = golden.params("n23_curve")
    a, e, a0 = [np.ascontiguousarray(p[k], dtype=np.float64) for k in ("a", "e", "a0")]
    e = np.ascontiguousarray(e[:2])
    h = hip.HipEStep(23, mode=hip.MODE_EXACT)
    score = np.zeros(4)

    def raw(*args):  # the C call itself, NULLs allowed (HipEStep.viterbi sets typed pointers: set ours every time)
        h.lib.psmc_hip_viterbi.argtypes = [C.c_void_p] * 6
        return h.lib.psmc_hip_viterbi(h.h, *[x if x is None else x.ctypes.data for x in args])
    assert raw(a, e, a0, None, score) == -5           # PSMC_HIP_ESTATE: no segments
    assert "no segments" in h.lib.psmc_hip_last_error(h.h).decode()
    segs = [np.zeros(50, dtype=np.uint8), np.array([0, 0, 0, 1, 0, 2, 0], dtype=np.uint8), np.zeros(3, dtype=np.uint8)]
    h.load_segments(segs)
    assert raw(a, e, a0, None, None) == -1            # EINVAL: neither output
    assert raw(None, e, a0, None, score) == -1 and raw(a, None, a0, None, score) == -1 and raw(a, e, None, None, score) == -1
    for bad in (15, 0, -1, 64.5, 2.0 ** 40):
        with pytest.raises(hip.HipError):
            h.set_option("vit_tile", bad)
    e_bad = e.copy()
    e_bad[1] = 0.0
    with pytest.raises(hip.HipError, match="segment 1"):
        h.viterbi(a, e_bad, a0)
    assert raw(a, e_bad, a0, None, score) == -1
    # the context is usable afterwards
    tables = vm.log_tables(a, e, a0)
    paths, scores = h.viterbi(a, e, a0)
    check(paths, scores, [vm.viterbi(tables, s)[0] for s in segs], np.array([vm.viterbi(tables, s)[1] for s in segs]), "after the error")
