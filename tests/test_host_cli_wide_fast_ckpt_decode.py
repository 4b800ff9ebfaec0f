"""`psmc -d / -D / -c / -s` with PSMC_HIP_OPTIONS=wide_ckpt=1,wide_decode_ckpt=1 on the wide fast path: the decoding E-step keeps
checkpoints (X at every 8th bin) and the decoding recomputes the rows between them (option "wide_decode_ckpt", include/psmc_hip.h).
Decoding from checkpoints returns the bits of decoding from the full table, so stdout is byte-identical to the run without
PSMC_HIP_OPTIONS, and stderr says what the decoding read.  With wide_ckpt=1 alone the decoding E-step keeps the full table as
before: no such notice, the same bytes."""
import os
import pytest
from test_host_cli_wide_fast import CLI
from test_host_cli_wide_fast_ckpt import built, psmc  # noqa: F401 (built: the module's autouse build fixture)

pytestmark = pytest.mark.gpu
SAYS_WIDE = "the decoding reads the wide fast tables"
SAYS_CKPT = "the decoding reads the wide fast tables (checkpoints: X at every 8th bin)"
CNT = ["-c", os.path.join(CLI, "small.cnt")]
CASES = [(p, lv, f) for p, lv in (("100*2", "fast"), ("150*2", "fast-all")) for f in (["-d"], ["-D"], CNT, ["-s"])]


@pytest.mark.parametrize("pattern,level,flags", CASES, ids=["%s%s" % (p.replace("*", "x"), f[0]) for p, _, f in CASES])
def test_psmc_decodes_from_checkpoints(pattern, level, flags):
    env = dict(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE=level, PSMC_HIP_DECODE=level)
    args = ["-N1", "-p", pattern] + flags
    ref, err = psmc(args, **env)
    assert SAYS_WIDE in err and "checkpoints: X at every 8th bin" not in err, err
    got, err = psmc(args, PSMC_HIP_OPTIONS="wide_ckpt=1,wide_decode_ckpt=1", **env)
    assert SAYS_CKPT in err, err
    assert "RD\t1" in ref and got == ref
    got, err = psmc(args, PSMC_HIP_OPTIONS="wide_ckpt=1", **env)   # as before: the full table for the decoding E-step
    assert SAYS_WIDE in err and "checkpoints: X at every 8th bin" not in err, err
    assert got == ref
