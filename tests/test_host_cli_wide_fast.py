"""The `psmc` binary with PSMC_HIP_MODE=fast PSMC_HIP_WIDE=fast beyond 128 states: factored E-steps on the wide fast path
(psmc_amd/csrc/estep_wide_fast.hip), against the reference's golden output and against exact runs of the same binary."""
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "psmc_amd", "host")
CLI = os.path.join(ROOT, "tests", "golden", "cli")
PSMC = os.path.join(HOST, "psmc")
# the end-to-end bound fast mode states against the reference (tests/test_host_cli.py EM_TOL) for LK, theta_0 and rho_0.  lambda_k:
# 100 free lambdas on 3e5 bins are barely determined, and the direct search turns the 1e-10 differences of the statistics into
# lambda differences of up to 1.9e-2 after five rounds (measured; LK 9.5e-10, theta / rho 1.4e-6): the bound is 2.5x that
EM_TOL = {"LK": 1e-8, "theta": 2e-5, "rho": 2e-5, "lam": 5e-2}
NOTE_WIDE = "PSMC_HIP_WIDE=fast"
NOTE_OLD = "the fast kernels stop at 128"


def run(args, cwd, **env):
    e = dict(os.environ)
    for k in ("PSMC_HIP_MODE", "PSMC_HIP_WIDE", "PSMC_HIP_DECODE", "PSMC_HIP_OPTIONS", "PSMC_HIP_DEVICES", "PSMC_FACTORED", "PSMC_FAST_MSTEP"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([PSMC] + args, cwd=cwd, capture_output=True, text=True, env=e, timeout=900)
    assert r.returncode == 0, r.stderr
    return r


def rounds(text):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import em_parity
    return em_parity.parse_psmc(text)


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """a few hundred thousand bins simulated from the 64-state golden model, as a .psmcfa"""
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    from psmc_amd import sim
    g = np.load(os.path.join(ROOT, "tests", "golden", "hmm_params.npz"))
    segs = sim.simulate_genome(g["n64_curve.a"], g["n64_curve.e"], g["n64_curve.a0"], np.array([160000, 90000, 50000]), seed=5)
    d = tmp_path_factory.mktemp("wide")
    conv = np.frombuffer(b"TKN", dtype=np.uint8)
    with open(d / "synth.psmcfa", "wb") as fh:
        for i, s in enumerate(segs):
            fh.write(b">%d\n" % (i + 1))
            c = conv[s]
            for j in range(0, len(c), 60):
                fh.write(c[j:j + 60].tobytes() + b"\n")
    return str(d)


def test_wide_fast_binary_golden_n200():
    """small_n200_N2 (the reference's output at 200 states): exit 0, the one stderr line, LK within 1e-5 relative."""
    args = open(os.path.join(CLI, "small_n200_N2.args")).read().split()
    r = run(args, CLI, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast")
    assert NOTE_WIDE in r.stderr and NOTE_OLD not in r.stderr, r.stderr
    got = [l for l in r.stdout.splitlines() if l.startswith("LK")]
    want = [l for l in open(os.path.join(CLI, "small_n200_N2.psmc")).read().splitlines() if l.startswith("LK")]
    assert len(got) == len(want)
    for g, w in zip(got[1:], want[1:]):
        assert abs(float(g.split()[1]) - float(w.split()[1])) <= 1e-5 * abs(float(w.split()[1]))


def compare_em(text, ref):
    got, want = rounds(text), rounds(ref)
    assert len(got) == len(want) == 6
    worst = dict(LK=0.0, theta=0.0, rho=0.0, lam=0.0)
    for g, w in zip(got, want):
        worst["LK"] = max(worst["LK"], abs(g["LK"] - w["LK"]) / max(abs(w["LK"]), 1.0))
        worst["theta"] = max(worst["theta"], abs(g["theta"] - w["theta"]) / w["theta"])
        worst["rho"] = max(worst["rho"], abs(g["rho"] - w["rho"]) / w["rho"])
        worst["lam"] = max(worst["lam"], max(abs(x - y) / y for x, y in zip(g["lam"], w["lam"])))
    for k, tol in EM_TOL.items():
        assert worst[k] <= tol, (k, worst)


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_wide_fast_binary_em_vs_exact(synth, devices):
    """-p "100*2" -N5 on the synthetic input: every round's LK, theta_0, rho_0 and lambda_k against a run of the same binary whose
    E-steps are exact (PSMC_HIP_MODE=fast without PSMC_HIP_WIDE: the exact kernels' full counts, the same O(N) objective -- against
    the reference's objective the direct search of 100 free lambdas on 3e5 bins lands elsewhere whatever the E-step); one device,
    and the segments sharded over two contexts of device 0."""
    args = ["-N5", "-t15", "-r5", "-p", "100*2", "synth.psmcfa"]
    r0 = run(args, synth, PSMC_HIP_MODE="fast")
    assert NOTE_OLD in r0.stderr, r0.stderr
    ref = r0.stdout
    env = dict(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast")
    if devices:
        env["PSMC_HIP_DEVICES"] = devices
    r = run(args, synth, **env)
    assert NOTE_WIDE in r.stderr, r.stderr
    compare_em(r.stdout, ref)


def test_wide_variable_changes_nothing_else():
    """Without PSMC_HIP_WIDE a fast run beyond 128 states keeps the old note; in exact mode the variable does nothing (the
    output stays the reference's, byte for byte); with a decoding flag the run stays exact beyond 128 states."""
    args = open(os.path.join(CLI, "small_n200_N2.args")).read().split()
    r = run(args, CLI, PSMC_HIP_MODE="fast")
    assert NOTE_OLD in r.stderr and NOTE_WIDE not in r.stderr, r.stderr
    r = run(args, CLI, PSMC_HIP_WIDE="fast")
    assert r.stdout == open(os.path.join(CLI, "small_n200_N2.psmc")).read() and NOTE_WIDE not in r.stderr
    plain = run(args, CLI, PSMC_HIP_MODE="fast").stdout
    # full counts asked for (PSMC_FACTORED=0), or the reference's objective (PSMC_FAST_MSTEP=0): the wide path does not apply,
    # and the run is the one without PSMC_HIP_WIDE, byte for byte
    r = run(args, CLI, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast", PSMC_FACTORED="0")
    assert NOTE_OLD in r.stderr and NOTE_WIDE not in r.stderr, r.stderr
    assert r.stdout == plain
    r = run(args, CLI, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast", PSMC_FAST_MSTEP="0")
    assert NOTE_WIDE not in r.stderr, r.stderr
    assert r.stdout == run(args, CLI, PSMC_HIP_MODE="fast", PSMC_FAST_MSTEP="0").stdout
    r = run(["-d"] + args, CLI, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast")
    assert NOTE_WIDE not in r.stderr, r.stderr
    assert r.stdout == run(["-d"] + args, CLI, PSMC_HIP_MODE="fast").stdout


def _lines(text):
    """the output without its QD lines (Q0 is computed from the full count matrix, which the factored path never has) and RI
    lines, split off for a numeric comparison"""
    keep, ri = [], []
    for l in text.splitlines():
        if l.startswith("RI"):
            ri.append(float(l.split()[1]))
        elif not l.startswith("QD"):
            keep.append(l)
    return keep, ri


@pytest.mark.parametrize("case", ["not_supported", "no_convergence"])
def test_wide_fast_binary_fallbacks(case):
    """The fallbacks of hb_estep_factored on this path.  "structured" = 0 makes the wide path answer ENOTSUP (psmc's own matrices
    always have the PSMC form: -C caps the matrix of decoding runs only, and those stay exact beyond 128 states); tile boundaries
    that may not be repaired (max_rounds=0, tiles of 37 bins, warm-up 5) make it answer ECONVERGE.  Either way the E-step is the
    exact kernels' full counts, summed on the host: the statistics of the run without PSMC_HIP_WIDE, so the same output."""
    args = open(os.path.join(CLI, "small_n200_N2.args")).read().split()
    env = dict(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast")
    env["PSMC_HIP_OPTIONS"] = "structured=0" if case == "not_supported" else "max_rounds=0,chunk=37,warmup=5"
    ref = run(args, CLI, PSMC_HIP_MODE="fast")
    r = run(args, CLI, **env)
    assert NOTE_WIDE in r.stderr, r.stderr
    if case == "no_convergence":
        assert "did not converge" in r.stderr, r.stderr
    got, want = _lines(r.stdout), _lines(ref.stdout)
    assert got[0] == want[0]
    assert len(got[1]) == len(want[1]) and all(x == y or abs(x - y) <= 1e-9 for x, y in zip(got[1], want[1]))   # (RD 0: inf)
