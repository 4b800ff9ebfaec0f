"""`psmc` with PSMC_HIP_MODE=fast PSMC_HIP_WIDE=fast PSMC_HIP_DECODE=fast at 129..256 hidden states: the EM rounds stay on the
wide fast path and -d / -D / -c / -s decode from its tables (options "wide_fast" + "wide_decode", include/psmc_hip.h).  -N0
decodes the starting parameters, so the fast and the exact run decode the same model: same lines, numbers within the library's
tolerances (to the last printed digit), DC runs identical except at near-ties which the exact run's own -D output shows to be
ties (compare() of tests/test_host_cli_fast_decode.py).  Without PSMC_HIP_DECODE=fast a decoding flag still makes the run exact."""
import os
import subprocess
import pytest
from conftest import GOLD
from test_host_cli_fast_decode import compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "psmc_amd", "host")
CLI = os.path.join(GOLD, "cli")
WIDE_DEC = dict(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast", PSMC_HIP_DECODE="fast")
SAYS_WIDE = "the decoding reads the wide fast tables"
SAYS_EXACT = "decoding needs the exact forward/backward tables; using PSMC_HIP_MODE=exact"
PATTERNS = {"n200": ["-p", "100*2"], "n149": ["-p", "4+47*3+4"]}   # (the second: tests/golden/cli/small_n149_d.args)
SMALL = ["small.psmcfa"]
CNT = ["-c", "small.cnt"]


@pytest.fixture(scope="module")
def psmc():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    return os.path.join(HOST, "psmc")


def run(psmc, args, **env):
    e = dict(os.environ)
    for k in ("PSMC_HIP_MODE", "PSMC_HIP_DECODE", "PSMC_HIP_WIDE", "PSMC_HIP_OPTIONS", "PSMC_HIP_DEVICES", "PSMC_FACTORED", "PSMC_FAST_MSTEP"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([psmc] + args, cwd=CLI, capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stderr[-800:]
    return r.stdout, r.stderr


CASES = [(p, f) for p in sorted(PATTERNS) for f in (["-d"], ["-D"], ["-s"], CNT)]


@pytest.mark.parametrize("pat,flags", CASES, ids=["%s%s" % (p, "".join(x for x in f if x.startswith("-"))) for p, f in CASES])
def test_wide_fast_decode_cli_matches_exact(psmc, pat, flags):
    args = ["-N0"] + PATTERNS[pat] + flags + SMALL
    fast, err = run(psmc, args, **WIDE_DEC)
    assert SAYS_WIDE in err and SAYS_EXACT not in err and "exact kernels" not in err, err
    exact, _ = run(psmc, args)
    exact_D = run(psmc, ["-N0"] + PATTERNS[pat] + ["-D"] + SMALL)[0] if "-d" in flags else None
    compare(fast, exact, exact_D)


def test_wide_fast_decode_cli_em_rounds_stay_wide(psmc):
    """-N2 -d: the EM rounds are those of the same run without -d, byte for byte (only MM is_decoding differs) -- they stayed on
    the wide fast path -- then the decoding."""
    a = ["-N2"] + PATTERNS["n200"]
    with_d, err = run(psmc, a + ["-d"] + SMALL, **WIDE_DEC)
    assert SAYS_WIDE in err
    plain, err2 = run(psmc, a + SMALL, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast")
    assert "factored E-steps on the wide fast kernels" in err2
    head = with_d[:with_d.index("TC\t")]
    assert head.replace("MM\tis_decoding:1\n", "MM\tis_decoding:0\n") == plain
    assert [l for l in head.splitlines() if l[:2] in ("RD", "LK")] == [l for l in plain.splitlines() if l[:2] in ("RD", "LK")]
    assert "DC\t" in with_d


def test_without_the_decode_switch_nothing_changes(psmc):
    """PSMC_HIP_MODE=fast PSMC_HIP_WIDE=fast with -d and no PSMC_HIP_DECODE: an exact run throughout, the reference's bytes."""
    args = open(os.path.join(CLI, "small_n149_d.args")).read().split()
    out, err = run(psmc, args, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast")
    assert SAYS_EXACT in err and SAYS_WIDE not in err
    assert out == open(os.path.join(CLI, "small_n149_d.psmc")).read()


def test_without_the_wide_switch_nothing_changes(psmc):
    """PSMC_HIP_MODE=fast PSMC_HIP_DECODE=fast without PSMC_HIP_WIDE beyond 128 states: every E-step and the decoding on the
    exact kernels, as before (-N0: no M-step, whose fast-mode objective would move the parameters in the sixth digit -- the
    decoding of the starting parameters is the exact run's, byte for byte)."""
    args = ["-N0", "-d"] + PATTERNS["n149"] + SMALL
    out, err = run(psmc, args, PSMC_HIP_MODE="fast", PSMC_HIP_DECODE="fast")
    assert SAYS_WIDE not in err and "every E-step of this run uses the exact ones" in err
    exact, _ = run(psmc, args)
    assert out == exact


def test_wide_fast_decode_cli_device_list(psmc):
    """PSMC_HIP_DEVICES=0,0: the decoding entry points reach each segment's shard through psmc_hip_group_route."""
    args = ["-N0"] + PATTERNS["n200"] + ["-D"] + CNT + SMALL
    fast, err = run(psmc, args, PSMC_HIP_DEVICES="0,0", **WIDE_DEC)
    assert SAYS_WIDE in err
    exact, _ = run(psmc, args)
    compare(fast, exact)


def test_wide_fast_decode_cli_exact_fallback(psmc):
    """A decoding E-step whose tile boundaries cannot converge (tiny tiles, no repair round): the exact twin repeats it and the
    decoding reads the twin's tables -- the exact decoding of the same parameters, byte for byte."""
    for flag in ("-d", "-s"):
        a = ["-N0"] + PATTERNS["n200"] + [flag] + SMALL
        fast, err = run(psmc, a, PSMC_HIP_OPTIONS="max_rounds=0,chunk=37,warmup=5", **WIDE_DEC)
        assert err.count("repeating this E-step with the exact kernels") == 1, err[-600:]
        exact, _ = run(psmc, a)
        assert fast == exact
