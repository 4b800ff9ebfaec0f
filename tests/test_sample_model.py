"""Posterior path sampling on the CPU: the numpy restatement of the pinned definition (tests/sample_model.py) against the oracle's
forward vectors, the host's plain C statement (psmc_sample_host, through psmc_amd.hostlib) against the restatement entry for entry,
independence of the call's shape, and the distribution of the samples against an exact forward-backward."""
import numpy as np
import pytest
from conftest import bits_equal

import sample_model as sm
from test_gpu_viterbi import banded_hmm, block_data


def dense_hmm(n, rng):
    a = rng.random((n, n)) ** 3 + 2.0 * np.eye(n)
    a /= a.sum(1, keepdims=True)
    e = np.zeros((2, n))
    e[1] = np.exp(np.linspace(np.log(0.002), np.log(0.6), n)) if n > 1 else 0.1
    e[0] = 1.0 - e[1]
    a0 = rng.random(n) + 0.5
    return a, e, a0 / a0.sum()


# ---- forward bits
@pytest.mark.parametrize("n", [1, 3, 23, 64, 65, 200])
def test_forward_is_the_oracles(oracle, n):
    rng = np.random.default_rng(100 + n)
    for a, e, a0 in (dense_hmm(n, rng), banded_hmm(n, rng)):
        seq = block_data(300, rng)
        assert (seq == 2).any() and (seq == 1).any()
        e3 = np.vstack([e, np.ones((1, n))])
        f, _, _, _, _ = oracle.fwd_bwd(a, e3, a0, seq)
        assert bits_equal(sm.forward(a, e, a0, seq), f[1:])


# ---- the host's C against the restatement
@pytest.mark.parametrize("n", [1, 2, 3, 23, 64, 65, 200])
def test_host_equals_model(n):
    from psmc_amd import hostlib
    rng = np.random.default_rng(4000 + n)
    a, e, a0 = banded_hmm(n, rng)
    if n >= 23:
        assert (a == 0.0).any()                       # the band: zero weights inside the draw
    moved = 0
    for L in (1, 2, 17, 600):
        seq = block_data(L, rng)
        if L >= 17:
            seq[3] = 2
            seq[L - 2] = 2
        f = sm.forward(a, e, a0, seq)
        for seed, q in ((1, 0), (2 ** 64 - 1, 7), (123456789012345, 2 ** 40 + 3)):
            got = hostlib.sample_host(a, e, a0, seq, seed, q, n_samp=4)
            assert got.dtype == np.int32 and got.shape == (4, L)
            for j in range(4):
                want = sm.sample(a, e, a0, seq, seed, j, q, f=f)
                assert np.array_equal(got[j], want), (n, L, seed, q, j, int(np.flatnonzero(got[j] != want)[0]))
            assert got.min() >= 0 and got.max() < n
            if L == 600:
                moved = max(moved, len(sm.runs(got[0])))
                assert n == 1 or not np.array_equal(got[0], got[1])  # two samples are two paths
    if n >= 3:
        assert moved >= 4


def test_streams_and_seeds_give_other_paths():
    from psmc_amd import hostlib
    rng = np.random.default_rng(5)
    a, e, a0 = banded_hmm(23, rng)
    seq = block_data(600, rng)
    base = hostlib.sample_host(a, e, a0, seq, 11, 3)[0]
    assert not np.array_equal(base, hostlib.sample_host(a, e, a0, seq, 12, 3)[0])
    assert not np.array_equal(base, hostlib.sample_host(a, e, a0, seq, 11, 4)[0])
    assert np.array_equal(base, hostlib.sample_host(a, e, a0, seq, 11, 3)[0])


# ---- the shape of the call
def test_sample_j_does_not_depend_on_the_call():
    from psmc_amd import hostlib
    rng = np.random.default_rng(77)
    a, e, a0 = banded_hmm(23, rng)
    seq = block_data(600, rng)
    five = hostlib.sample_host(a, e, a0, seq, 9, 5, n_samp=5)
    assert np.array_equal(hostlib.sample_host(a, e, a0, seq, 9, 5, n_samp=1)[0], five[0])
    assert np.array_equal(hostlib.sample_host(a, e, a0, seq, 9, 5, n_samp=3), five[:3])
    for j in range(5):                                 # the one-sample statement of sample j
        assert np.array_equal(sm.sample(a, e, a0, seq, 9, j, 5), five[j]), j
    assert len({five[j].tobytes() for j in range(5)}) == 5


def test_zero_and_nan_totals_draw_state_zero():
    assert sm.draw(np.zeros(5), 0.7) == 0
    assert sm.draw(np.array([0.0, np.nan, 1.0]), 0.7) == 0
    assert sm.draw(np.array([0.0, 0.0, 1.0, 0.0]), 2.0 ** -53) == 2     # a leading run of zeros is never drawn
    assert sm.draw(np.array([0.25, 0.25, 0.5, 0.0]), 1.0) == 2          # r = 1: the last state that carries weight
    from psmc_amd import hostlib
    a = np.zeros((3, 3))
    e = np.full((2, 3), 0.5)
    got = hostlib.sample_host(a, e, np.array([0.2, 0.3, 0.5]), np.zeros(6, dtype=np.uint8), 1, 0, n_samp=3)
    assert not got[:, :5].any()                        # f_2 .. are 0 / 0: NaN totals


# ---- the distribution
def test_samples_follow_the_posterior():
    """n = 4, L = 12, J = 4096 samples of one seed: every state frequency per bin against the exact posterior gamma, every pair
    frequency of neighbouring bins against the exact xi, each within 5 sqrt(p (1 - p) / J) + 2 / J.  A condition, not a
    measurement: the restatement meets it with room (worst deviation over seeds 1-5: 3.7 sigma)."""
    from psmc_amd import hostlib
    rng = np.random.default_rng(2026)
    n, L, J = 4, 12, 4096
    a = rng.random((n, n)) + np.eye(n)
    a /= a.sum(1, keepdims=True)
    e = np.zeros((2, n))
    e[1] = [0.02, 0.1, 0.3, 0.6]
    e[0] = 1.0 - e[1]
    a0 = rng.random(n)
    a0 /= a0.sum()
    seq = np.array([0, 0, 1, 0, 2, 0, 1, 1, 0, 2, 0, 0], dtype=np.uint8)
    em = np.vstack([e, np.ones((1, n))])
    # plain forward-backward
    al = np.zeros((L, n))
    be = np.ones((L, n))
    al[0] = a0 * em[seq[0]]
    for u in range(1, L):
        al[u] = (al[u - 1] @ a) * em[seq[u]]
    for u in range(L - 2, -1, -1):
        be[u] = a @ (em[seq[u + 1]] * be[u + 1])
    Z = al[L - 1].sum()
    gamma = al * be / Z
    xi = np.array([al[u][:, None] * a * (em[seq[u + 1]] * be[u + 1])[None, :] / Z for u in range(L - 1)])
    assert np.allclose(gamma.sum(1), 1.0) and np.allclose(xi.sum((1, 2)), 1.0)

    paths = hostlib.sample_host(a, e, a0, seq, 1, 0, n_samp=J)
    for j in range(0, J, 512):
        assert np.array_equal(paths[j], sm.sample(a, e, a0, seq, 1, j, 0))

    def bound(p):
        return 5.0 * np.sqrt(p * (1.0 - p) / J) + 2.0 / J
    freq = np.stack([(paths == k).mean(0) for k in range(n)], axis=1)            # (L, n)
    dev = np.abs(freq - gamma) / np.sqrt(gamma * (1 - gamma) / J)
    print("states: worst deviation %.2f sigma" % dev.max())
    assert (np.abs(freq - gamma) <= bound(gamma)).all(), (freq, gamma)
    pair = np.zeros((L - 1, n, n))
    for u in range(L - 1):
        np.add.at(pair[u], (paths[:, u], paths[:, u + 1]), 1.0 / J)
    print("pairs: worst deviation %.2f sigma, smallest pair probability %.1e" % ((np.abs(pair - xi) / np.sqrt(xi * (1 - xi) / J)).max(), xi.min()))
    assert (np.abs(pair - xi) <= bound(xi)).all()
