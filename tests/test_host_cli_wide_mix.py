"""The `psmc` binary with PSMC_HIP_OPTIONS=wide_hom_tiles=1,wide_mix_tiles=1 on the wide fast path (PSMC_HIP_MODE=fast
PSMC_HIP_WIDE=fast, 200 states): the input with a planted run of homozygosity that carries scattered `N` bins
(tests/wide_mix_model.py mix_sandwich) gives, round for round, what the run on the exact kernels gives within the fast-mode gates of
tests/test_host_cli_wide_fast.py, and the usage text names the option."""
import subprocess
import numpy as np
import pytest
from test_host_cli_wide_fast import run, rounds, EM_TOL, NOTE_WIDE, NOTE_OLD, PSMC, HOST
from wide_mix_model import mix_sandwich

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planted(golden, tmp_path_factory):
    """mix_sandwich of golden.segs_mid[3] as a one-sequence .psmcfa"""
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    s = mix_sandwich(golden.segs_mid[3])
    d = tmp_path_factory.mktemp("widemix")
    c = np.frombuffer(b"TKN", dtype=np.uint8)[s]
    with open(d / "mix.psmcfa", "wb") as fh:
        fh.write(b">1\n")
        for j in range(0, len(c), 60):
            fh.write(c[j:j + 60].tobytes() + b"\n")
    return str(d)


ARGS = ["-N2", "-t15", "-r5", "-p", "100*2", "mix.psmcfa"]


@pytest.fixture(scope="module")
def exact_rounds(planted):
    r0 = run(ARGS, planted, PSMC_HIP_MODE="fast")
    assert NOTE_OLD in r0.stderr, r0.stderr
    return rounds(r0.stdout)


def worst_of(got, want):
    assert len(got) == len(want) >= 1
    worst = dict(LK=0.0, theta=0.0, rho=0.0, lam=0.0)
    for g, w in zip(got, want):
        worst["LK"] = max(worst["LK"], abs(g["LK"] - w["LK"]) / max(abs(w["LK"]), 1.0))
        worst["theta"] = max(worst["theta"], abs(g["theta"] - w["theta"]) / w["theta"])
        worst["rho"] = max(worst["rho"], abs(g["rho"] - w["rho"]) / w["rho"])
        worst["lam"] = max(worst["lam"], max(abs(x - y) / y for x, y in zip(g["lam"], w["lam"])))
    return worst


@pytest.mark.parametrize("base", ["wide_hom_tiles=1", "wide_hom_tiles=1,chunk=64,warmup=512", "wide_gap_tiles=1,wide_hom_tiles=1,chunk=64,warmup=512"],
                         ids=["default-plan", "chunk64", "chunk64-gap"])
def test_wide_mix_binary_em(planted, exact_rounds, base):
    """-N2 -p "100*2": LK, theta_0, rho_0 and lambda_k of every round within the bounds of tests/test_host_cli_wide_fast.py of the run
    without the option (the same PSMC_HIP_OPTIONS less wide_mix_tiles=1).  Against the run whose E-steps are exact (PSMC_HIP_MODE=fast
    without PSMC_HIP_WIDE) the first round is held to the same bounds: it is the one E-step both runs do with the same parameters.
    (Later rounds of that run have been through another M-step search, and on an input of 4 696 bins LK, printed with six decimals,
    moves in steps of 9.6e-9 of itself -- the whole LK bound; they are printed, not asserted.)  With the default plan every tile of so short
    an input is anchored and the option has nothing to chain; at tiles of 64 bins and a warm-up of 512 the planted run is crossed by
    the chain with the mix tiles' own matrices -- in two runs around the two tiles of missing data, in one with "wide_gap_tiles"."""
    r1 = run(ARGS, planted, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast", PSMC_HIP_OPTIONS=base + ",wide_mix_tiles=1")
    assert NOTE_WIDE in r1.stderr, r1.stderr
    r2 = run(ARGS, planted, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast", PSMC_HIP_OPTIONS=base)
    assert NOTE_WIDE in r2.stderr, r2.stderr
    got = rounds(r1.stdout)
    assert len(got) == 3
    print("wide_mix_tiles=1 (%s) against the exact run, all rounds:" % base, worst_of(got, exact_rounds))
    for name, worst in (("the run without the option", worst_of(got, rounds(r2.stdout))), ("the exact run, first round", worst_of(got[:1], exact_rounds[:1]))):
        print("wide_mix_tiles=1 (%s) against %s:" % (base, name), worst)
        for k, tol in EM_TOL.items():
            assert worst[k] <= tol, (name, k, worst)


def test_usage_names_the_option():
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    r = subprocess.run([PSMC], capture_output=True, text=True, timeout=60)
    assert "wide_hom_tiles=1,wide_mix_tiles=1" in r.stderr and "wide_mix_mb" in r.stderr, r.stderr
