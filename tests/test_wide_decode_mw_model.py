"""The CPU side of tests/test_gpu_wide_fast_mw_decode.py (decoding from the multi-wave wide fast E-step's tables at 257 .. 1024
states, options "wide_fast" = 2 + "wide_decode", PSMC_HIP_WIDE=fast-all PSMC_HIP_DECODE=fast-all):
  a. the host driver's decision (psmc_amd/host/run.c psmc_mode_plan) with the decode level 2;
  b. the kernels' formulas -- wide_decode_model of tests/test_wide_decode_model.py, untiled, in double -- against the oracle at
     300, 513 and 1024 states within 1e-12 (posterior, recombination, relative scales), and, from the oracle alone, how many
     positions of every case of the GPU file are near-ties under its 2e-9 rule: fewer than 0.1 % in each.
Observed: short_segs at every size 0 near-ties of 1661 bins, path equal everywhere, post <= 2.3e-15, recomb <= 7.0e-15, scales
<= 4.3e-15; rho0 = 1e-6 at 1024 states 0 near-ties of 8551 bins."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from test_wide_decode_model import wide_decode_model
from test_gpu_wide_fast_mw import params, short_segs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
TOL_TIE = 2e-9
MAX_UNCLEAR = 1e-3
GPU_SIZES = [257, 300, 512, 513, 768, 769, 1024]
RHO_1E6 = [0.02, 1e-6, 15.0] + [1.0] * 128   # with the pattern 128*8: 1024 states
SEED2 = 12                                   # params(300, SEED2): the second model of "the last single E-step decides"


def extreme_segs(golden):
    """the 8551 bins of the model extreme of the GPU file"""
    return golden.segs_small[:10] + [golden.segs_mid[3][:3000]]


@pytest.fixture(scope="module")
def plan():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "host"), "libpsmc_host.so"], check=True)
    lib = C.CDLL(os.path.join(ROOT, "psmc_amd", "host", "libpsmc_host.so"))
    f = lib.psmc_mode_plan
    f.argtypes = [C.c_int] * 5
    return f


def test_mode_plan_decode_level_2(plan):
    """psmc_mode_plan(mode_fast, wide, decode level, n_states, decoding): level 2 (PSMC_HIP_DECODE=fast-all) with wide = 2 keeps a
    decoding run of 257..1024 states on the wide fast path and decodes from its tables; everywhere else it answers as level 1."""
    FAST, WIDE, WDEC = 1, 2, 4
    for n in (257, 300, 1024):
        assert plan(1, 2, 2, n, 1) == FAST | WIDE | WDEC          # the new combination
        assert plan(1, 2, 1, n, 1) == FAST                         # PSMC_HIP_DECODE=fast keeps its meaning
        assert plan(1, 2, 0, n, 1) == 0
    for n in (64, 128, 129, 256):
        for dec in (0, 1):
            for wide in (0, 1, 2):
                assert plan(1, wide, 2, n, dec) == plan(1, wide, 1, n, dec), (n, dec, wide)
    for n in (257, 300, 1024, 1025):                               # ... and beyond 256 states in every other case
        for wide in (0, 1, 2):
            assert plan(1, wide, 2, n, 0) == plan(1, wide, 1, n, 0)
            if wide < 2 or n > 1024:
                assert plan(1, wide, 2, n, 1) == plan(1, wide, 1, n, 1) == FAST
    assert plan(1, 1, 2, 300, 1) == FAST
    assert plan(1, 2, 2, 300, 0) == FAST | WIDE
    for n in (64, 200, 300, 1024):
        for d in (0, 1):
            assert plan(0, 2, 2, n, d) == 0


def _near_ties(oracle, a, e, a0, segs):
    unclear = total = 0
    for seg in segs:
        f, b, s, _, _ = oracle.fwd_bwd(a, e, a0, seg)
        px, _ = oracle.post_full(a, e, seg, f, b, s)
        top2 = np.partition(px[1:], px.shape[1] - 2, axis=1)[:, -2:]
        unclear += int((np.abs(top2[:, 1] - top2[:, 0]) <= TOL_TIE).sum()); total += len(seg)
    return unclear, total


@pytest.mark.parametrize("n", GPU_SIZES)
def test_mw_decode_formulas_and_near_ties(golden, oracle, n):
    """short_segs with params(n), the inputs of the GPU file's sizes: the near-ties of the oracle's posterior, and at 300, 513
    and 1024 states the formulas against the oracle."""
    a, e, a0 = params(n)
    segs = short_segs(golden)
    worst = dict(post=0.0, recomb=0.0, scales=0.0)
    unclear = total = 0
    for seg in segs:
        L = len(seg)
        f, b, s, _, _ = oracle.fwd_bwd(a, e, a0, seg)
        px, rx = oracle.post_full(a, e, seg, f, b, s)
        top2 = np.partition(px[1:], n - 2, axis=1)[:, -2:]
        clear = np.abs(top2[:, 1] - top2[:, 0]) > TOL_TIE
        unclear += int((~clear).sum()); total += L
        if n not in (300, 513, 1024):
            continue
        xp, _ = oracle.post_decode(f, b, s)
        post, rec, sc, path = wide_decode_model(a, e, a0, np.asarray(seg))
        worst["post"] = max(worst["post"], float(np.abs(post - px[1:]).max()))
        worst["recomb"] = max(worst["recomb"], float(np.abs(rec - rx[1:]).max()))
        worst["scales"] = max(worst["scales"], float(np.abs(sc / s[1:] - 1.0).max()))
        assert np.array_equal(path[clear], xp[1:][clear])
        assert rec[L - 1] == 0.0
    print("\nmulti-wave decoding inputs, n = %d: near-ties %d of %d" % (n, unclear, total))
    if n in (300, 513, 1024):
        print("formulas vs oracle: post %.2e recomb %.2e scales %.2e (relative)" % (worst["post"], worst["recomb"], worst["scales"]))
    assert total == 1661
    assert unclear < MAX_UNCLEAR * total, (unclear, total)
    assert worst["post"] <= TOL and worst["recomb"] <= TOL and worst["scales"] <= TOL, worst


def test_second_model_has_few_near_ties(golden, oracle):
    a, e, a0 = params(300, SEED2)
    unclear, total = _near_ties(oracle, a, e, a0, short_segs(golden))
    print("\nparams(300, %d): near-ties %d of %d" % (SEED2, unclear, total))
    assert unclear < MAX_UNCLEAR * total, (unclear, total)


def test_model_extreme_has_few_near_ties(golden, oracle):
    """rho0 = 1e-6 at 1024 states on 8551 bins, the model extreme of the GPU file (t_max = 60 on the same bins has 18 near-ties,
    0.21 %: over the cap, so the GPU file leaves that model out)."""
    from psmc_amd import hostlib
    a, e, a0 = hostlib.hmm_params("128*8", RHO_1E6)
    unclear, total = _near_ties(oracle, a, e, a0, extreme_segs(golden))
    print("\nrho0 = 1e-6, 1024 states: near-ties %d of %d" % (unclear, total))
    assert total == 8551
    assert unclear < MAX_UNCLEAR * total, (unclear, total)
