"""The `psmc` binary with PSMC_HIP_MODE=fast PSMC_HIP_WIDE=fast-all at 300 states (-p "150*2"): factored E-steps on the multi-wave
wide fast path (psmc_amd/csrc/estep_wide_fast.hip) against runs of the same binary on the exact kernels, under the bounds of
tests/test_host_cli_wide_fast.py; PSMC_HIP_WIDE=fast and decoding runs of that size stay what they were."""
import os
import pytest
from test_host_cli_wide_fast import run, rounds, EM_TOL, CLI, HOST, NOTE_OLD

pytestmark = pytest.mark.gpu
ARGS = ["-N2", "-p", "150*2", "small.psmcfa"]
NOTE_ALL = "PSMC_HIP_WIDE=fast-all: factored E-steps on the wide fast kernels"


@pytest.fixture(scope="module", autouse=True)
def built():
    import subprocess
    subprocess.run(["make", "-s", "-C", HOST], check=True)


def test_fast_all_em_vs_exact():
    """Every round's LK, theta_0, rho_0 and lambda_k against the run whose E-steps are the exact kernels' (PSMC_HIP_MODE=fast
    without PSMC_HIP_WIDE: full counts, the same O(N) objective); the stderr note names the state count and the path."""
    ref = run(ARGS, CLI, PSMC_HIP_MODE="fast")
    assert NOTE_OLD in ref.stderr, ref.stderr
    r = run(ARGS, CLI, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast-all")
    assert "300 hidden states" in r.stderr and NOTE_ALL in r.stderr and NOTE_OLD not in r.stderr, r.stderr
    got, want = rounds(r.stdout), rounds(ref.stdout)
    assert len(got) == len(want) == 3
    worst = dict(LK=0.0, theta=0.0, rho=0.0, lam=0.0)
    for g, w in zip(got, want):
        worst["LK"] = max(worst["LK"], abs(g["LK"] - w["LK"]) / max(abs(w["LK"]), 1.0))
        worst["theta"] = max(worst["theta"], abs(g["theta"] - w["theta"]) / w["theta"])
        worst["rho"] = max(worst["rho"], abs(g["rho"] - w["rho"]) / w["rho"])
        worst["lam"] = max(worst["lam"], max(abs(x - y) / y for x, y in zip(g["lam"], w["lam"])))
    print("fast-all vs exact E-steps, 300 states, worst over the rounds:", worst)
    for k, tol in EM_TOL.items():
        assert worst[k] <= tol, (k, worst)


def test_fast_all_changes_nothing_else():
    """PSMC_HIP_WIDE=fast at 300 states is the run without the variable, byte for byte (the one-wave path stops at 256); with -d
    and fast-all the output is the exact run's, byte for byte (decoding keeps a run beyond 256 states exact throughout).  The two
    -d runs take the O(N) objective (PSMC_FAST_MSTEP=1): the reference's objective with 150 free lambdas at 300 states costs
    a CPU half a minute per run whatever the input, and which objective the M-step uses is not what this compares."""
    plain = run(ARGS, CLI, PSMC_HIP_MODE="fast")
    r = run(ARGS, CLI, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast")
    assert r.stdout == plain.stdout and NOTE_OLD in r.stderr and "wide fast kernels" not in r.stderr, r.stderr
    exact_d = run(["-d"] + ARGS, CLI, PSMC_FAST_MSTEP="1")
    r = run(["-d"] + ARGS, CLI, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast-all", PSMC_FAST_MSTEP="1")
    assert r.stdout == exact_d.stdout and "wide fast kernels" not in r.stderr, r.stderr
    assert any(l.startswith("DC") for l in r.stdout.splitlines())
