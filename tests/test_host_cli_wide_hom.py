"""The `psmc` binary with PSMC_HIP_OPTIONS=wide_hom_tiles=1 on the wide fast path (PSMC_HIP_MODE=fast PSMC_HIP_WIDE=fast, 200 states):
the input with a planted run of homozygosity (tests/wide_hom_model.py hom_sandwich) gives, round for round, what the run on the exact
kernels gives within the fast-mode gates of tests/test_host_cli_wide_fast.py, and the usage text names the option."""
import os
import subprocess
import numpy as np
import pytest
from test_host_cli_wide_fast import run, rounds, EM_TOL, NOTE_WIDE, NOTE_OLD, PSMC, HOST
from wide_hom_model import hom_sandwich

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planted(golden, tmp_path_factory):
    """hom_sandwich of golden.segs_mid[3] as a one-sequence .psmcfa"""
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    s = hom_sandwich(golden.segs_mid[3])
    d = tmp_path_factory.mktemp("widehom")
    c = np.frombuffer(b"TKN", dtype=np.uint8)[s]
    with open(d / "hom.psmcfa", "wb") as fh:
        fh.write(b">1\n")
        for j in range(0, len(c), 60):
            fh.write(c[j:j + 60].tobytes() + b"\n")
    return str(d)


@pytest.mark.parametrize("options", ["wide_hom_tiles=1", "wide_hom_tiles=1,chunk=64,warmup=512"], ids=["default-plan", "chunk64"])
def test_wide_hom_binary_em(planted, options):
    """-N2 -p "100*2": LK, theta_0, rho_0 and lambda_k of every round within the bounds of tests/test_host_cli_wide_fast.py of the run
    whose E-steps are exact (PSMC_HIP_MODE=fast without PSMC_HIP_WIDE).  With the default plan every tile of so short an input is
    anchored and the option has nothing to chain; at tiles of 64 bins and a warm-up of 512 the run is crossed by the chain."""
    args = ["-N2", "-t15", "-r5", "-p", "100*2", "hom.psmcfa"]
    r0 = run(args, planted, PSMC_HIP_MODE="fast")
    assert NOTE_OLD in r0.stderr, r0.stderr
    r1 = run(args, planted, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast", PSMC_HIP_OPTIONS=options)
    assert NOTE_WIDE in r1.stderr, r1.stderr
    got, want = rounds(r1.stdout), rounds(r0.stdout)
    assert len(got) == len(want) == 3
    worst = dict(LK=0.0, theta=0.0, rho=0.0, lam=0.0)
    for g, w in zip(got, want):
        worst["LK"] = max(worst["LK"], abs(g["LK"] - w["LK"]) / max(abs(w["LK"]), 1.0))
        worst["theta"] = max(worst["theta"], abs(g["theta"] - w["theta"]) / w["theta"])
        worst["rho"] = max(worst["rho"], abs(g["rho"] - w["rho"]) / w["rho"])
        worst["lam"] = max(worst["lam"], max(abs(x - y) / y for x, y in zip(g["lam"], w["lam"])))
    print("wide_hom_tiles=1 (%s) against the exact run:" % options, worst)
    for k, tol in EM_TOL.items():
        assert worst[k] <= tol, (k, worst)


def test_usage_names_the_option():
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    r = subprocess.run([PSMC], capture_output=True, text=True, timeout=60)
    assert "wide_hom_tiles=1" in r.stderr and "wide_hom_min" in r.stderr, r.stderr
