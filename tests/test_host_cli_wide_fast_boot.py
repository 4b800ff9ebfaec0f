"""The `psmc_boot` binary with PSMC_HIP_MODE=fast PSMC_HIP_WIDE=fast | fast-all beyond 128 states: the replicates' E-steps on the wide
fast path (options "wide_fast" + "wide_batch": psmc_amd/csrc/api_batch.hip batch_wide), -p "100*2" (200 states, four replicates) and
-p "150*2" (300 states, the multi-wave kernels, two replicates) on tests/golden/cli/small.psmcfa with tiles of 100 bins and a warm-up
of 30, so that the tiles of a 5 k-bin input do speculate.

Against the same binary without the variable (PSMC_HIP_MODE=fast: the exact kernels' E-steps, the same O(N) objective), every round
of every replicate under EM_TOL of tests/test_host_cli_wide_fast.py (LK 1e-8, theta_0 / rho_0 2e-5, lambda_k 5e-2).  The path keeps no
history, so everything else is byte identity: over the device list, the M-step threads, --main, and every setting that must not
reach it.

Observed on the MI355X (printed by the first test, -s), worst over every round of every replicate:
  200 states, PSMC_HIP_WIDE=fast, 4 replicates:      LK 1.9e-9  theta_0 4.0e-6  rho_0 3.8e-6  lambda_k 1.4e-2
  300 states, PSMC_HIP_WIDE=fast-all, 2 replicates:  LK 1.7e-9  theta_0 5.8e-8  rho_0 4.7e-7  lambda_k 4.2e-2
(lambda_k: 150 free lambdas on 5 k bins are barely determined; the direct search turns the 1e-13 differences of the statistics into
these, as tests/test_host_cli_wide_fast.py says of its own input.)
"""
import os
import subprocess
import pytest
from test_host_cli_wide_fast import rounds, EM_TOL, CLI, HOST, PSMC

pytestmark = pytest.mark.gpu
BOOT = os.path.join(HOST, "psmc_boot")
INPUT = os.path.join(CLI, "small.psmcfa")
OPTIONS = "chunk=100,warmup=30"
NOTE = "the replicates' E-steps run on the wide fast kernels"
CLEAN = ("PSMC_HIP_MODE", "PSMC_HIP_WIDE", "PSMC_HIP_DECODE", "PSMC_HIP_OPTIONS", "PSMC_HIP_DEVICES", "PSMC_FACTORED", "PSMC_FAST_MSTEP",
         "PSMC_SEED", "PSMC_TIMING", "PSMC_BOOT_MAIN_CUS", "OMP_NUM_THREADS")
_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-s", "-C", os.path.join(os.path.dirname(HOST), "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", HOST], check=True)


def environ(env):
    e = {k: v for k, v in os.environ.items() if k not in CLEAN}
    e["PSMC_HIP_OPTIONS"] = OPTIONS
    e.update(env)
    return e


def boot(root, pattern, n_rep, main=False, **env):
    """one psmc_boot job (run once per distinct job): (the replicates' files, stderr, main.psmc or None)"""
    key = (pattern, n_rep, main, tuple(sorted(env.items())))
    if key not in _RUNS:
        d = root.mktemp("boot")
        cmd = [BOOT, "-R", str(n_rep), "-S", "40", "-O", str(d / "r-%d.psmc")]
        if main:
            cmd += ["--main", str(d / "main.psmc"), "--main-input", INPUT]
        r = subprocess.run(cmd + ["--", "-N2", "-p", pattern, INPUT], capture_output=True, text=True, env=environ(env), timeout=600)
        assert r.returncode == 0, r.stderr[-1500:]
        _RUNS[key] = ([open(d / ("r-%d.psmc" % k)).read() for k in range(n_rep)], r.stderr, open(d / "main.psmc").read() if main else None)
    return _RUNS[key]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory


WIDE = dict(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast")
CASES = [("100*2", 4, "fast", 200), ("150*2", 2, "fast-all", 300)]


@pytest.mark.parametrize("pattern,n_rep,level,n", CASES)
def test_boot_wide_em_vs_exact_esteps(root, pattern, n_rep, level, n):
    """Every round of every replicate -- LK, theta_0, rho_0, lambda_k -- against the job without the variable, whose E-steps are the
    exact kernels'; the stderr note names the state count and the variable's value with the variable, and is absent without it."""
    ref, ref_err, _ = boot(root, pattern, n_rep, PSMC_HIP_MODE="fast")
    got, err, _ = boot(root, pattern, n_rep, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE=level)
    assert NOTE not in ref_err, ref_err
    assert "psmc_boot: %d hidden states: PSMC_HIP_WIDE=%s: %s" % (n, level, NOTE) in err, err
    assert "repeating this E-step" not in err, err
    worst = dict(LK=0.0, theta=0.0, rho=0.0, lam=0.0)
    for k in range(n_rep):
        g, w = rounds(got[k]), rounds(ref[k])
        assert len(g) == len(w) == 3, k
        for x, y in zip(g, w):
            worst["LK"] = max(worst["LK"], abs(x["LK"] - y["LK"]) / max(abs(y["LK"]), 1.0))
            worst["theta"] = max(worst["theta"], abs(x["theta"] - y["theta"]) / y["theta"])
            worst["rho"] = max(worst["rho"], abs(x["rho"] - y["rho"]) / y["rho"])
            worst["lam"] = max(worst["lam"], max(abs(p - q) / q for p, q in zip(x["lam"], y["lam"])))
    print("psmc_boot, %d states, PSMC_HIP_WIDE=%s against exact E-steps, worst over every round of %d replicates:" % (n, level, n_rep), worst)
    for key, tol in EM_TOL.items():
        assert worst[key] <= tol, (key, worst)


def test_boot_wide_bytes_over_devices_and_threads(root):
    """The path keeps no history: the replicates' files are the same bytes on one context and on two (PSMC_HIP_DEVICES=0 / 0,0,
    the replicates dealt round robin), and with one M-step thread and four."""
    base = boot(root, "100*2", 4, PSMC_HIP_DEVICES="0", **WIDE)[0]
    for env in (dict(PSMC_HIP_DEVICES="0,0"), dict(PSMC_HIP_DEVICES="0", OMP_NUM_THREADS="1"), dict(PSMC_HIP_DEVICES="0", OMP_NUM_THREADS="4")):
        got, err, _ = boot(root, "100*2", 4, **dict(WIDE, **env))
        assert NOTE in err
        for k in range(4):
            assert got[k] == base[k], (env, k)


@pytest.mark.parametrize("pattern,n_rep,level,n", CASES)
def test_boot_wide_main_run(root, pattern, n_rep, level, n):
    """--main: main.psmc is, byte for byte, what `psmc` writes under the same environment (its E-steps on the wide fast path too),
    and the replicates write the bytes of the job without --main, although the main run shares the device with them."""
    env = dict(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE=level, PSMC_HIP_DEVICES="0")
    plain = boot(root, pattern, n_rep, **env)[0]
    got, err, main = boot(root, pattern, n_rep, main=True, **env)
    one = subprocess.run([PSMC, "-N2", "-p", pattern, INPUT], capture_output=True, text=True, env=environ(env), timeout=600)
    assert one.returncode == 0, one.stderr
    assert "PSMC_HIP_WIDE=%s: factored E-steps on the wide fast kernels" % level in one.stderr, one.stderr
    assert main == one.stdout and "RD\t2" in main
    for k in range(n_rep):
        assert got[k] == plain[k], k


def test_boot_wide_variable_changes_nothing_else(root):
    """In exact mode, and in fast mode with PSMC_FACTORED=0 (full counts asked for: beyond 128 states only the exact kernels have
    them), the variable does nothing: no note, and the bytes of the job without it.  (The exact-mode jobs take the O(N) objective,
    PSMC_FAST_MSTEP=1: the reference's objective with 100 free lambdas costs a CPU seconds per M-step, and which objective the
    M-step uses is not what this compares.)"""
    for env in (dict(PSMC_FAST_MSTEP="1"), dict(PSMC_HIP_MODE="fast", PSMC_FACTORED="0")):
        ref = boot(root, "100*2", 2, **env)[0]
        got, err, _ = boot(root, "100*2", 2, PSMC_HIP_WIDE="fast", **env)
        assert NOTE not in err, err
        for k in range(2):
            assert got[k] == ref[k], (env, k)
