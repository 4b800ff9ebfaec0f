"""Cases shared by the gates of psmc_hip_viterbi and psmc_hip_sample_paths at the model extremes (tests/test_gpu_path_extremes.py,
tests/test_viterbi_model.py, tests/golden/make_golden_viterbi_extremes.py): the thirteen extreme PSMC models at any state count, the
data of the goldens, the short and ragged segments, the synthetic matrices of the degenerate draws, and the counts of those draws
along the restatement's own paths.  TEST INFRASTRUCTURE, CPU only: nothing here touches a device."""
import os
import numpy as np

import sample_model as sm
import viterbi_model as vm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

GOLDEN_SIZES = (64, 65, 200)
SMALL_CAP = 2000     # bins kept of every segment of segments_small.npz in the goldens
SLICE_BINS = 6000    # ... and of segments_mid.npz's fourth segment, the longest segment of a case
NAN_MODELS = ("lambda_alt_1e-3_1e3", "lambda_ramp_down_1e3_1e-3")   # a[n-1][0] = NaN, a[0][n-1] = 0: no finite path, every draw 0


def model_names():
    from test_gpu_wide_fast_edges import MODELS
    return list(MODELS)


def extreme_model(name, n):
    """(a, e (3, n), a0) of MODELS[name] at n states: the host model of "<n>*1" up to 128 states (tests/test_gpu_fast_cells.py
    host_model), of tests/test_gpu_wide_fast_edges.py model() up to 510, and of "<n/4>*4+<n%4>*1" beyond (a group repeats at most
    255 times)"""
    from psmc_amd import hostlib
    from test_gpu_wide_fast_edges import MODELS, model
    if n <= 128:
        return hostlib.hmm_params("%d*1" % n, MODELS[name](n))
    if n <= 510:
        return model(name, n)
    assert n % 4 and n // 4 <= 255, n
    return hostlib.hmm_params("%d*4+%d*1" % (n // 4, n % 4), MODELS[name](n // 4 + n % 4))


def _npz_segs(name):
    s = np.load(os.path.join(GOLD, name))
    return [s[k] for k in sorted(s.files)]


def golden_segments():
    """{name: observations}: tests/test_gpu_wide_fast_edges.py extremes_segs, every segment of segments_small.npz cut to SMALL_CAP
    bins; the last is the 6000-bin slice, the longest"""
    out = {"small_s%02d" % i: s[:SMALL_CAP] for i, s in enumerate(_npz_segs("segments_small.npz"))}
    out["mid_s03"] = _npz_segs("segments_mid.npz")[3][:SLICE_BINS]
    return out


def finds_path(par, segs):
    """True when tests/viterbi_model.py finds a path on every segment, else the NoFinitePath message of the first that has none"""
    tables = vm.log_tables(par[0], par[1], par[2])
    try:
        for s in segs:
            vm.viterbi(tables, s)
    except vm.NoFinitePath as ex:
        return str(ex)
    return True


def viterbi_reference(par, segs):
    """(paths, scores) of tests/viterbi_model.py, or the index of the first segment in load order without a path"""
    tables = vm.log_tables(par[0], par[1], par[2])
    paths, scores = [], []
    for i, s in enumerate(segs):
        try:
            p, sc = vm.viterbi(tables, s)
        except vm.NoFinitePath:
            return i
        paths.append(p)
        scores.append(sc)
    return paths, np.array(scores)


# ---- short and ragged data: at most 1000 bins
def short_segs(golden, long_bins=700):
    """1, 3 (all missing), 2, 63, 64, 65, 70 (all missing), 32 (six missing bins at either end) and long_bins bins: slices of the
    fixture data, the longest last"""
    src = golden.segs_mid[0]
    miss = src[34204:34294]
    assert (miss == 2).all() and len(miss) == 90
    def cut(i, L):   # L bins around a heterozygous (i even) or a missing (i odd) bin, at bin i % L of the slice
        p = int(np.flatnonzero(src[1000 * i:] == 1 + i % 2)[0]) + 1000 * i - i % L
        return src[p:p + L]
    segs = [golden.segs_small[0], miss[:3], cut(1, 2), cut(2, 63), cut(3, 64), cut(4, 65), miss[:70],
            np.concatenate([miss[:6], cut(5, 20), miss[:6]]), golden.segs_mid[3][:long_bins]]
    assert [len(s) for s in segs] == [1, 3, 2, 63, 64, 65, 70, 32, long_bins]
    assert len(np.unique(np.concatenate(segs[2:6]))) == 3 and (segs[8] == 1).any()
    return segs


# ---- the degenerate draws: synthetic matrices
def het_rates(n):
    e = np.zeros((2, n))
    e[1] = np.exp(np.linspace(np.log(0.002), np.log(0.6), n))
    e[0] = 1.0 - e[1]
    return e


def stochastic(n, rng):
    a = rng.random((n, n)) + 0.05
    return a / a.sum(1, keepdims=True)


def clamp_hmm(n, factor, rng):
    """a row-stochastic random matrix whose row 0 is multiplied by -factor on the odd columns: below an odd state the weights start
    with a negative one, and where it outweighs the others every running sum lies below r times the (negative) total -- a count of n"""
    a = stochastic(n, rng)
    a[0, 1::2] *= -factor
    a0 = rng.random(n) + 0.5
    return a, het_rates(n), a0 / a0.sum()


def subnormal_hmm(n, rng):
    """a row-stochastic random matrix, the entries farther than n / 8 from the diagonal scaled by 1e-300, rows renormalised"""
    a = stochastic(n, rng)
    k = np.arange(n)
    a[np.abs(k[:, None] - k[None, :]) > n / 8] *= 1e-300
    a /= a.sum(1, keepdims=True)
    a0 = rng.random(n) + 0.5
    return a, het_rates(n), a0 / a0.sum()


def upper_half_hmm(n, rng):
    """block diagonal, two halves, a0 on the upper half [n // 2, n) only: the weights of every draw begin with n // 2 zeros"""
    a = stochastic(n, rng)
    h = n // 2
    a[:h, h:] = 0.0
    a[h:, :h] = 0.0
    a /= a.sum(1, keepdims=True)
    a0 = rng.random(n) + 0.5
    a0[:h] = 0.0
    return a, het_rates(n), a0 / a0.sum()


TINY = np.finfo(np.float64).tiny


def draw_conditions(a, e, a0, seq, seed, j, q, path):
    """along `path` (the restatement's sample j of a segment with stream id q): how often a count of n was clamped, how many terms
    f * a of the drawn-from weights were subnormal, and how many draws began with a zero weight"""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    f = sm.forward(a, e, a0, seq)
    r = sm.uniforms(seed, j, q, len(seq))
    out = dict(clamp=0, subnormal=0, leading_zero=0)
    for u in range(len(seq), 0, -1):                     # position u, 1-based: the draw of path[u - 1]
        w = f[u - 1] if u == len(seq) else f[u - 1] * a[:, path[u]]
        c = np.cumsum(w)
        with np.errstate(invalid="ignore"):
            cnt = int((c < r[u - 1] * c[-1]).sum())
            out["subnormal"] += int(((np.abs(w) > 0) & (np.abs(w) < TINY)).sum())
        drawn = min(cnt, n - 1) if (c[-1] > 0.0 or c[-1] < 0.0) else 0
        assert drawn == path[u - 1], (u, drawn, path[u - 1])
        out["clamp"] += int(cnt == n and (c[-1] > 0.0 or c[-1] < 0.0))
        out["leading_zero"] += int(w[0] == 0.0 and drawn > 0)
    return out
