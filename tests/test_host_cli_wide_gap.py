"""The `psmc` binary with PSMC_HIP_OPTIONS=wide_gap_tiles=1 on the wide fast path (PSMC_HIP_MODE=fast PSMC_HIP_WIDE=fast, 200 states):
an input with a planted run of `N` bins gives, round for round, what the same run without the option gives, and the usage text
names the option."""
import os
import subprocess
import numpy as np
import pytest
from test_host_cli_wide_fast import run, rounds, EM_TOL, NOTE_WIDE, PSMC, HOST, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gapped(tmp_path_factory):
    """1e5 bins simulated from the 64-state golden model in two sequences, 20 000 bins of the first replaced by N, as a .psmcfa"""
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    from psmc_amd import sim
    g = np.load(os.path.join(ROOT, "tests", "golden", "hmm_params.npz"))
    segs = sim.simulate_genome(g["n64_curve.a"], g["n64_curve.e"], g["n64_curve.a0"], np.array([60000, 40000]), seed=9)
    segs = [np.array(s, dtype=np.uint8) for s in segs]
    segs[0][25000:45000] = 2
    d = tmp_path_factory.mktemp("widegap")
    conv = np.frombuffer(b"TKN", dtype=np.uint8)
    with open(d / "gapped.psmcfa", "wb") as fh:
        for i, s in enumerate(segs):
            fh.write(b">%d\n" % (i + 1))
            c = conv[s]
            for j in range(0, len(c), 60):
                fh.write(c[j:j + 60].tobytes() + b"\n")
    return str(d)


def test_wide_gap_binary_em(gapped):
    """-N2 -p "100*2": LK, theta_0, rho_0 and lambda_k of every round within the bounds of tests/test_host_cli_wide_fast.py of the
    run without the option."""
    args = ["-N2", "-t15", "-r5", "-p", "100*2", "gapped.psmcfa"]
    env = dict(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast")
    r0 = run(args, gapped, **env)
    r1 = run(args, gapped, PSMC_HIP_OPTIONS="wide_gap_tiles=1", **env)
    assert NOTE_WIDE in r0.stderr and NOTE_WIDE in r1.stderr, r1.stderr
    got, want = rounds(r1.stdout), rounds(r0.stdout)
    assert len(got) == len(want) == 3
    worst = dict(LK=0.0, theta=0.0, rho=0.0, lam=0.0)
    for g, w in zip(got, want):
        worst["LK"] = max(worst["LK"], abs(g["LK"] - w["LK"]) / max(abs(w["LK"]), 1.0))
        worst["theta"] = max(worst["theta"], abs(g["theta"] - w["theta"]) / w["theta"])
        worst["rho"] = max(worst["rho"], abs(g["rho"] - w["rho"]) / w["rho"])
        worst["lam"] = max(worst["lam"], max(abs(x - y) / y for x, y in zip(g["lam"], w["lam"])))
    print("wide_gap_tiles=1 against the run without it:", worst)
    for k, tol in EM_TOL.items():
        assert worst[k] <= tol, (k, worst)


def test_usage_names_the_option(gapped):
    r = subprocess.run([PSMC], capture_output=True, text=True, timeout=60)
    assert "wide_gap_tiles=1" in r.stderr and "wide_gap_min" in r.stderr, r.stderr
