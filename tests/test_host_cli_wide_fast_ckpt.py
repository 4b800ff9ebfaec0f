"""`psmc` and `psmc_boot` with PSMC_HIP_OPTIONS=wide_ckpt=1 on the wide fast path (PSMC_HIP_MODE=fast PSMC_HIP_WIDE=fast | fast-all):
the E-steps keep their forward table at every 8th bin only and recompute the rest (option "wide_ckpt", include/psmc_hip.h).  The
option changes no bit of the statistics, so every output is byte-identical to the run without it: the EM rounds at 200 and 300
states, a decoding run (whose one decoding E-step keeps the full table: "wide_decode" wins) and every bootstrap replicate."""
import os
import subprocess
import pytest
from test_host_cli_wide_fast import CLI, HOST, PSMC

pytestmark = pytest.mark.gpu
BOOT = os.path.join(HOST, "psmc_boot")
INPUT = os.path.join(CLI, "small.psmcfa")
CLEAN = ("PSMC_HIP_MODE", "PSMC_HIP_WIDE", "PSMC_HIP_DECODE", "PSMC_HIP_OPTIONS", "PSMC_HIP_DEVICES", "PSMC_FACTORED", "PSMC_FAST_MSTEP",
         "PSMC_SEED", "PSMC_TIMING", "PSMC_BOOT_MAIN_CUS", "OMP_NUM_THREADS")
CKPT = "wide_ckpt=1"


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-s", "-C", os.path.join(os.path.dirname(HOST), "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", HOST], check=True)


def environ(env):
    e = {k: v for k, v in os.environ.items() if k not in CLEAN}
    e.update(env)
    return e


def psmc(args, **env):
    r = subprocess.run([PSMC] + args + [INPUT], capture_output=True, text=True, env=environ(env), timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    return r.stdout, r.stderr


@pytest.mark.parametrize("pattern,level", [("100*2", "fast"), ("150*2", "fast-all")])
def test_psmc_ckpt_bytes(pattern, level):
    env = dict(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE=level)
    ref, err = psmc(["-N2", "-p", pattern], **env)
    assert "factored E-steps on the wide fast kernels" in err, err
    got, err = psmc(["-N2", "-p", pattern], PSMC_HIP_OPTIONS=CKPT, **env)
    assert "factored E-steps on the wide fast kernels" in err, err
    assert "RD\t2" in ref and got == ref


def test_psmc_ckpt_decoding_bytes():
    """-d with PSMC_HIP_DECODE=fast: the decoding E-step sets "wide_decode" first and so keeps the full table"""
    env = dict(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast", PSMC_HIP_DECODE="fast")
    ref, err = psmc(["-N1", "-d", "-p", "100*2"], **env)
    assert "the decoding reads the wide fast tables" in err, err
    got, err = psmc(["-N1", "-d", "-p", "100*2"], PSMC_HIP_OPTIONS=CKPT, **env)
    assert "the decoding reads the wide fast tables" in err, err
    assert "\nDC\t" in ref and got == ref


def test_boot_ckpt_bytes(tmp_path):
    """psmc_boot -R 3 -S 1 at 200 states, tiles of 100 bins (tests/test_host_cli_wide_fast_boot.py): every replicate file"""
    outs = []
    for opt in ("chunk=100,warmup=30", "chunk=100,warmup=30," + CKPT):
        d = tmp_path / ("ckpt" if CKPT in opt else "full")
        d.mkdir()
        cmd = [BOOT, "-R", "3", "-S", "1", "-O", str(d / "r-%d.psmc"), "--", "-N2", "-p", "100*2", INPUT]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                           env=environ(dict(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast", PSMC_HIP_OPTIONS=opt)))
        assert r.returncode == 0, r.stderr[-1500:]
        assert "the replicates' E-steps run on the wide fast kernels" in r.stderr, r.stderr
        outs.append([open(d / ("r-%d.psmc" % k)).read() for k in range(3)])
    for k in range(3):
        assert "RD\t2" in outs[0][k] and outs[1][k] == outs[0][k], k
