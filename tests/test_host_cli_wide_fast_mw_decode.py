"""`psmc` with PSMC_HIP_MODE=fast PSMC_HIP_WIDE=fast-all PSMC_HIP_DECODE=fast-all at 300 hidden states (-p "150*2"): the EM rounds
stay on the multi-wave wide fast path and -d / -D / -c / -s decode from its tables (options "wide_fast" = 2 + "wide_decode",
include/psmc_hip.h; kernels: psmc_amd/csrc/estep_wide_post.hip).  -N0 decodes the starting parameters, so the fast and the
exact run decode the same model: same lines, numbers within the library's tolerances (to the last printed digit), DC runs
identical except at near-ties which the exact run's own -D output shows to be ties (compare() of
tests/test_host_cli_fast_decode.py).  PSMC_HIP_DECODE=fast keeps what it meant beyond 256 states: a fast-mode run on the exact
kernels."""
import os
import pytest
from test_host_cli_fast_decode import compare
from test_host_cli_wide_fast_decode import psmc, run, SAYS_WIDE, SAYS_EXACT, SMALL, CNT   # noqa: F401 (psmc: the fixture)

pytestmark = pytest.mark.gpu
MW_DEC = dict(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast-all", PSMC_HIP_DECODE="fast-all")
P300 = ["-p", "150*2"]
CASES = [["-d"], ["-D"], ["-s"], CNT]


@pytest.fixture(scope="module")
def exact_runs(psmc):
    """the exact run of every flag, once"""
    return {f[0]: run(psmc, ["-N0"] + P300 + f + SMALL)[0] for f in CASES}


@pytest.mark.parametrize("flags", CASES, ids=[f[0] for f in CASES])
def test_mw_decode_cli_matches_exact(psmc, exact_runs, flags):
    args = ["-N0"] + P300 + flags + SMALL
    fast, err = run(psmc, args, **MW_DEC)
    assert SAYS_WIDE in err and "300 hidden states" in err and SAYS_EXACT not in err and "exact kernels" not in err, err
    compare(fast, exact_runs[flags[0]], exact_runs["-D"] if "-d" in flags else None)


def test_decode_fast_beyond_256_states_is_unchanged(psmc, exact_runs):
    """PSMC_HIP_DECODE=fast (not fast-all) with PSMC_HIP_WIDE=fast-all at 300 states: a fast-mode run on the exact kernels, as before
    -- the exact run byte for byte, and nothing said about the wide fast tables."""
    out, err = run(psmc, ["-N0"] + P300 + ["-d"] + SMALL, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast-all", PSMC_HIP_DECODE="fast")
    assert SAYS_WIDE not in err and "every E-step of this run uses the exact ones" in err, err
    assert out == exact_runs["-d"]


def test_mw_decode_cli_em_rounds_stay_wide(psmc):
    """-N1 -d: the RD / LK lines are those of the same run without -d under PSMC_HIP_WIDE=fast-all -- the EM round stayed on the
    multi-wave wide fast path -- then the decoding."""
    a = ["-N1"] + P300
    with_d, err = run(psmc, a + ["-d"] + SMALL, **MW_DEC)
    assert SAYS_WIDE in err
    plain, err2 = run(psmc, a + SMALL, PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast-all")
    assert "factored E-steps on the wide fast kernels" in err2
    head = with_d[:with_d.index("TC\t")]
    assert [l for l in head.splitlines() if l[:2] in ("RD", "LK")] == [l for l in plain.splitlines() if l[:2] in ("RD", "LK")]
    assert "DC\t" in with_d


def test_mw_decode_cli_device_list(psmc):
    """PSMC_HIP_DEVICES=0,0: the decoding entry points reach each segment's shard through psmc_hip_group_route."""
    args = ["-N0"] + P300 + ["-D"] + CNT + SMALL
    fast, err = run(psmc, args, PSMC_HIP_DEVICES="0,0", **MW_DEC)
    assert SAYS_WIDE in err
    exact, _ = run(psmc, args)
    compare(fast, exact)


def test_mw_decode_cli_exact_fallback(psmc, exact_runs):
    """A decoding E-step whose tile boundaries cannot converge (tiny tiles, no repair round): the exact twin repeats it and the
    decoding reads the twin's tables -- the exact decoding of the same parameters, byte for byte."""
    fast, err = run(psmc, ["-N0"] + P300 + ["-d"] + SMALL, PSMC_HIP_OPTIONS="max_rounds=0,chunk=37,warmup=5", **MW_DEC)
    assert err.count("repeating this E-step with the exact kernels") == 1, err[-600:]
    assert fast == exact_runs["-d"]
