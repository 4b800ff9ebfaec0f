"""The identities the decoding kernels of the wide fast path rest on (psmc_amd/csrc/estep_wide_post.hip), on the CPU: with the
lag-normalised forward vectors X_p and the self-scaled backward vectors bt_p = e[o_p] (a bt_{p+1}) sb_p of tests/fastmodel.py's
untiled model, stepped with the O(N) structured steps,
    gamma_p(k) = X_p(k) (a bt_{p+1})(k) / G_p,  G_p = sum_k X_p(k) (a bt_{p+1})(k),      gamma_L = X_L / sum X_L
    recomb_p   = 1 - sum_l X_p(l) a_ll bt_{p+1}(l) / G_p,                                  recomb_L = 0
    s_p        = sum X_p / sum X_{p-1} / inv_p  (inv_p = 1/d_p at p % 4 == 0, else 1),     s_1 = sum_k a0_k e_k(o_1)
are the oracle's posterior, recombination probability and scaling factors (khmm.c, aux.c:183-200) within 1e-12 at 150..200
states -- so a failure of tests/test_gpu_wide_fast_decode.py can be told apart from a wrong formula.  Also: how many positions
of that file's golden fixtures are near-ties under its 2e-9 rule (computed from the oracle alone), and the host driver's
decision about PSMC_HIP_MODE / PSMC_HIP_WIDE / PSMC_HIP_DECODE (psmc_amd/host/run.c psmc_mode_plan)."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from conftest import GOLD
import fastmodel as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def wide_decode_model(a, e, a0, seg):
    """post (L, n), recomb (L,), scales (L,), path (L,) by the kernels' formulas, untiled."""
    f = fm.factor_structure(a)
    assert f is not None
    n, L = a.shape[0], len(seg)
    X = np.zeros((L + 1, n)); inv = np.ones(L + 1)
    X[1] = a0 * e[seg[0]]
    for p in range(2, L + 1):
        if p % fm.NORM_EVERY == 0:
            inv[p] = 2.0 ** -np.floor(np.log2(X[p - 1].sum()))   # a power of two, as pow2_rcp
        X[p] = e[seg[p - 1]] * fm.struct_step_forward(f, X[p - 1]) * inv[p]
    s = np.zeros(L)
    s[0] = X[1].sum()
    for p in range(2, L + 1):
        s[p - 1] = X[p].sum() / X[p - 1].sum() / inv[p]
    post = np.zeros((L, n)); rec = np.zeros(L)
    post[L - 1] = X[L] / X[L].sum()
    bt = e[seg[L - 1]].copy()   # bt_L (B_L = 1)
    akk = np.diag(a)
    for p in range(L - 1, 0, -1):
        y = fm.struct_step_backward(f, bt)
        g = X[p] * y
        G = g.sum()
        post[p - 1] = g / G
        rec[p - 1] = 1.0 - (X[p] * akk * bt).sum() / G
        sb = 1.0 / bt.sum() if p % fm.NORM_EVERY == 0 else 1.0
        bt = y * e[seg[p - 1]] * sb
    return post, rec, s, post.argmax(1)


def _params(golden, n):
    from psmc_amd import hostlib
    if n == 200:
        w = dict(np.load(os.path.join(GOLD, "estep_wide.npz")))
        return w["n200.a"], w["n200.e"], w["n200.a0"]
    rng = np.random.default_rng(1000 + n)
    lam = np.exp(rng.normal(0.0, 0.7, size=n))
    return hostlib.hmm_params("%d*1" % n, [0.02, 0.004, 15.0] + list(lam))


@pytest.fixture(scope="module")
def hostlib_built():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "host"), "libpsmc_host.so"], check=True)


@pytest.mark.parametrize("n", [150, 175, 200])
def test_wide_decode_formulas_match_oracle(golden, oracle, hostlib_built, n):
    a, e, a0 = _params(golden, n)
    segs = golden.segs_small[:8] + [golden.segs_small[8], golden.segs_mid[5], golden.segs_mid[4][:1500]]
    worst = dict(post=0.0, recomb=0.0, scales=0.0)
    for seg in segs:
        L = len(seg)
        f, b, s, _, _ = oracle.fwd_bwd(a, e, a0, seg)
        px, rx = oracle.post_full(a, e, seg, f, b, s)
        xp, _ = oracle.post_decode(f, b, s)
        post, rec, sc, path = wide_decode_model(a, e, a0, np.asarray(seg))
        worst["post"] = max(worst["post"], float(np.abs(post - px[1:]).max()))
        worst["recomb"] = max(worst["recomb"], float(np.abs(rec - rx[1:]).max()))
        worst["scales"] = max(worst["scales"], float(np.abs(sc / s[1:] - 1.0).max()))
        top2 = np.sort(px[1:], axis=1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 2e-9
        assert np.array_equal(path[clear], xp[1:][clear])
        assert rec[L - 1] == 0.0
    print("\nwide decoding formulas vs oracle, n = %d: post %.2e recomb %.2e scales %.2e (relative)" % (n, worst["post"], worst["recomb"], worst["scales"]))
    assert worst["post"] <= TOL and worst["recomb"] <= TOL and worst["scales"] <= TOL, worst


@pytest.mark.parametrize("key", ["n200", "n149"])
def test_golden_fixtures_have_no_near_ties(golden, oracle, key):
    """tests/test_gpu_wide_fast_decode.py may leave the path unchecked where the exact posterior's two largest entries are
    within 2e-9, and asserts that fewer than 0.1 % of a case's positions are: on its golden cases none is."""
    w = dict(np.load(os.path.join(GOLD, "estep_wide.npz")))
    a, e, a0 = w[key + ".a"], w[key + ".e"], w[key + ".a0"]
    unclear = total = 0
    for seg in golden.segs_small[:8]:
        f, b, s, _, _ = oracle.fwd_bwd(a, e, a0, seg)
        px, _ = oracle.post_full(a, e, seg, f, b, s)
        top2 = np.sort(px[1:], axis=1)[:, -2:]
        unclear += int(((top2[:, 1] - top2[:, 0]) <= 2e-9).sum()); total += len(seg)
    assert unclear < 1e-3 * total, (unclear, total)
    assert unclear == 0


def test_mode_plan(hostlib_built):
    """psmc_mode_plan(mode_fast, wide_fast, decode_fast, n_states, decoding): bit 0 the run is a fast run, bit 1 the wide fast
    path is on, bit 2 the decoding reads its tables.  Everything but the new combination is what the driver did before."""
    lib = C.CDLL(os.path.join(ROOT, "psmc_amd", "host", "libpsmc_host.so"))
    plan = lib.psmc_mode_plan
    plan.argtypes = [C.c_int] * 5
    FAST, WIDE, WDEC = 1, 2, 4
    for n in (129, 200, 256):
        assert plan(1, 1, 1, n, 1) == FAST | WIDE | WDEC          # the new combination
        assert plan(1, 1, 0, n, 1) == 0                            # decoding without PSMC_HIP_DECODE: exact throughout
        assert plan(1, 1, 0, n, 0) == FAST | WIDE                  # no decoding: the wide path as before
        assert plan(1, 1, 1, n, 0) == FAST | WIDE                  # PSMC_HIP_DECODE without a decoding flag changes nothing
        assert plan(1, 0, 1, n, 1) == FAST                         # no PSMC_HIP_WIDE: fast mode whose E-steps are the exact kernels
        assert plan(1, 0, 0, n, 0) == FAST
        assert plan(0, 1, 1, n, 1) == 0 and plan(0, 1, 1, n, 0) == 0   # exact mode ignores both
    for n in (64, 128, 257, 300):                                  # outside 129..256 the wide path never comes on
        for dec in (0, 1):
            assert plan(1, 1, 1, n, dec) == FAST
            assert plan(1, 1, 0, n, dec) == (0 if dec else FAST)
