"""The `psmc` binary with PSMC_HIP_WIDE_COUNTS=1: a fast-mode run beyond 128 states that asks for full counts (PSMC_FACTORED=0)
gets them from the wide fast path (options "wide_fast" + "wide_counts": psmc_amd/csrc/estep_wide_counts.hip) instead of the wide
exact kernels.  References: the reference's golden output at 200 states (tests/golden/cli/small_n200_N2.psmc) and the output of
the same command WITHOUT the variable, recorded from the build before the variable existed
(tests/golden/cli/small_n200_N2_fast_fullcounts.stdout / .stderr: exact E-steps, the same O(N) objective).  Tolerances: those of
tests/test_host_cli_wide_fast.py -- LK 1e-5 relative against the golden; LK 1e-8, theta_0 / rho_0 2e-5, lambda_k 5e-2 against the
exact E-steps of the same binary (EM_TOL); lambda_k 5e-2 against the golden too (the recorded exact run is 2.4e-2 from it: the
O(N) objective's direct search lands elsewhere whatever the E-step).

Observed on the MI355X: against the golden LK 8.0e-7, lambda_k 2.3e-2; against the exact E-steps LK 0 (as printed), theta_0 / rho_0
4.3e-6, lambda_k 5.1e-3.
"""
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "psmc_amd", "host")
CLI = os.path.join(ROOT, "tests", "golden", "cli")
PSMC = os.path.join(HOST, "psmc")
EM_TOL = {"LK": 1e-8, "theta": 2e-5, "rho": 2e-5, "lam": 5e-2}   # tests/test_host_cli_wide_fast.py
NOTE_COUNTS = "full-count E-steps on the wide fast kernels"
NOTE_OLD = "every E-step of this run uses the exact ones"
ENV = dict(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast", PSMC_FACTORED="0")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-s", "-C", HOST], check=True)


def run(args, **env):
    e = dict(os.environ)
    for k in ("PSMC_HIP_MODE", "PSMC_HIP_WIDE", "PSMC_HIP_WIDE_COUNTS", "PSMC_HIP_DECODE", "PSMC_HIP_OPTIONS", "PSMC_HIP_DEVICES", "PSMC_FACTORED",
              "PSMC_FAST_MSTEP"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([PSMC] + args, cwd=CLI, capture_output=True, text=True, env=e, timeout=900)
    assert r.returncode == 0, r.stderr
    return r


def rounds(text):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import em_parity
    return em_parity.parse_psmc(text)


def worst(got, want):
    assert len(got) == len(want) == 3
    w = dict(LK=0.0, theta=0.0, rho=0.0, lam=0.0)
    for g, x in zip(got, want):
        w["LK"] = max(w["LK"], abs(g["LK"] - x["LK"]) / max(abs(x["LK"]), 1.0))
        w["theta"] = max(w["theta"], abs(g["theta"] - x["theta"]) / x["theta"])
        w["rho"] = max(w["rho"], abs(g["rho"] - x["rho"]) / x["rho"])
        w["lam"] = max(w["lam"], max(abs(a - b) / b for a, b in zip(g["lam"], x["lam"])))
    return w


def test_wide_counts_binary_n200():
    """-N2 -p "100*2" on small.psmcfa with the variable: the new stderr line, and every round against the reference's golden and
    against the recorded run whose E-steps were exact."""
    args = open(os.path.join(CLI, "small_n200_N2.args")).read().split()
    r = run(args, PSMC_HIP_WIDE_COUNTS="1", **ENV)
    assert NOTE_COUNTS in r.stderr and NOTE_OLD not in r.stderr, r.stderr
    got = rounds(r.stdout)
    gold = rounds(open(os.path.join(CLI, "small_n200_N2.psmc")).read())
    exact = rounds(open(os.path.join(CLI, "small_n200_N2_fast_fullcounts.stdout")).read())
    wg, wx = worst(got, gold), worst(got, exact)
    print("psmc with PSMC_HIP_WIDE_COUNTS=1 against the golden", wg, "against exact E-steps", wx)
    assert wg["LK"] <= 1e-5 and wg["lam"] <= EM_TOL["lam"], wg
    for k, tol in EM_TOL.items():
        assert wx[k] <= tol, (k, wx)


def test_without_the_variable_nothing_changes():
    """Without PSMC_HIP_WIDE_COUNTS the run is, byte for byte on stdout and stderr, what the build before the variable printed;
    so it is with the variable where it does not apply (no PSMC_HIP_WIDE; a factored run: PSMC_FACTORED unset)."""
    args = open(os.path.join(CLI, "small_n200_N2.args")).read().split()
    out = open(os.path.join(CLI, "small_n200_N2_fast_fullcounts.stdout")).read()
    err = open(os.path.join(CLI, "small_n200_N2_fast_fullcounts.stderr")).read()
    r = run(args, **ENV)
    assert r.stdout == out and r.stderr == err
    r = run(args, PSMC_HIP_MODE="fast", PSMC_FACTORED="0", PSMC_HIP_WIDE_COUNTS="1")
    assert r.stdout == out and r.stderr == err
    r = run(args, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast", PSMC_HIP_WIDE_COUNTS="1")
    assert NOTE_COUNTS not in r.stderr and "factored E-steps on the wide fast kernels" in r.stderr, r.stderr
