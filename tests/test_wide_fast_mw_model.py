"""The CPU side of tests/test_gpu_wide_fast_mw.py (the wide fast E-step at 257 .. 1024 states, option "wide_fast" = 2,
PSMC_HIP_WIDE=fast-all): the host driver's decision (psmc_amd/host/run.c psmc_mode_plan) with wide = 2, and the algorithm itself
-- tests/fastmodel.py, untiled, in double -- against the oracle per vector and per cell at 512 and 1024 states, so that the
bounds the GPU tests hold the kernels to are known to be within the algorithm's reach at these widths."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import fastmodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "host"), "libpsmc_host.so"], check=True)
    lib = C.CDLL(os.path.join(ROOT, "psmc_amd", "host", "libpsmc_host.so"))
    f = lib.psmc_mode_plan
    f.argtypes = [C.c_int] * 5
    return f


def test_mode_plan_wide_all(plan):
    """psmc_mode_plan(mode_fast, wide, decode_fast, n_states, decoding) with wide = 2: at 129..256 states what wide = 1 answers; at
    257..1024 states FAST | WIDE without a decoding flag, and with one what wide = 1 answers there (FAST with decode-fast, else 0:
    decoding keeps such a run on the exact kernels); up to 128 states and in exact mode nothing changes.  wide = 1 and 0 keep
    their answers."""
    FAST, WIDE, WDEC = 1, 2, 4
    for n in (64, 128, 129, 256, 257, 300, 1024):
        for dec in (0, 1):
            for dfast in (0, 1):
                got = plan(1, 2, dfast, n, dec)
                if n <= 128:
                    want = FAST if (not dec or dfast) else 0
                elif n <= 256:
                    want = plan(1, 1, dfast, n, dec)
                    assert want == ((FAST | WIDE | (WDEC if dec else 0)) if (not dec or dfast) else 0)
                elif not dec:
                    want = FAST | WIDE
                else:
                    want = FAST if dfast else 0
                    assert want == plan(1, 1, dfast, n, dec)
                assert got == want, (n, dec, dfast, got, want)
                assert plan(0, 2, dfast, n, dec) == 0                       # exact mode ignores the variable
                if n > 256:                                                 # wide = 1 beyond 256 states: as before
                    assert plan(1, 1, dfast, n, dec) == (FAST if (not dec or dfast) else 0)
    assert plan(1, 2, 0, 300, 0) == FAST | WIDE and plan(1, 1, 0, 300, 0) == FAST and plan(1, 0, 0, 300, 0) == FAST


@pytest.mark.parametrize("n,pattern,free,bins", [(512, "128*4", 128, 2000), (1024, "128*8", 128, 1000)])
def test_untiled_model_meets_the_cell_bound(golden, oracle, n, pattern, free, bins):
    """fastmodel (lagged power-of-two normalisation, O(N) structured steps, per-tile posterior normalisation) against the oracle on
    a PSMC-form model of the host library with seeded random lambdas: every gated cell of each of the seven vectors ten times
    inside FAST_TOL_CELL = 1e-9, L1 / QA / QE inside 1e-11, LL inside 1e-13.  Prints the margin."""
    from psmc_amd import hostlib
    from psmc_amd.parity import factored_error_metrics, tri_sums, FACTORED_NAMES
    rng = np.random.default_rng(2000 + n)
    lam = np.exp(rng.normal(0.0, 0.7, size=free))
    a, e, a0 = hostlib.hmm_params(pattern, [0.02, 0.004, 15.0] + list(lam))
    assert a.shape == (n, n) and fastmodel.factor_structure(a) is not None
    segs = golden.segs_small[:8] + [golden.segs_mid[4][:bins - 454]]
    assert sum(len(s) for s in segs) <= 2000
    o = oracle.estep(a, e, a0, segs)
    m = fastmodel.estep_fast_model(a, e, a0, segs, T=1 << 30, W=0)
    x = factored_error_metrics(dict(sums=tri_sums(m["A"]), E=m["E"], LL=m["LL"]), dict(sums=tri_sums(o["A"]), E=o["E"], LL=o["LL"]), a, e)
    cell = max(x[v + "_cell"] for v in FACTORED_NAMES)
    l1 = max(x[v + "_l1"] for v in FACTORED_NAMES)
    print("\nfastmodel vs oracle at %d states, %d bins: worst gated cell %.2e (bound 1e-9: margin %.0fx)  L1 %.2e  QA %.2e  QE %.2e  LL %.2e"
          % (n, sum(len(s) for s in segs), cell, 1e-9 / max(cell, 1e-300), l1, x["QA"], x["QE"], x["LL"]))
    assert cell <= 1e-9 / 10, x
    assert l1 <= 1e-11 and x["QA"] <= 1e-11 and x["QE"] <= 1e-11 and x["LL"] <= 1e-13, x


@pytest.mark.parametrize("pa", [[0.02, 1e-6, 15.0], [0.02, 0.004, 60.0]])
def test_extreme_models_factor_at_1024_states(pa):
    """The two model extremes tests/test_gpu_wide_fast_mw.py runs at 1024 states have the PSMC form by the library's own
    criterion (fastmodel.factor_structure restates api.hip factor_structure): the GPU test must get a result, not ENOTSUP."""
    from psmc_amd import hostlib
    a, e, a0 = hostlib.hmm_params("128*8", pa + [1.0] * 128)
    assert a.shape == (1024, 1024) and np.isfinite(a).all() and (a >= 0).all()
    assert fastmodel.factor_structure(a) is not None
