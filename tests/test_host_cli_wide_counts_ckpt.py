"""`psmc` and `psmc_boot` with PSMC_HIP_OPTIONS=wide_ckpt=1,wide_counts_ckpt=1 beside PSMC_HIP_WIDE_COUNTS=1: the full-count E-steps
of the wide fast path keep X at every 8th bin and the counts pass recomputes the rows between the checkpoints (option
"wide_counts_ckpt", include/psmc_hip.h; psmc_amd/csrc/estep_wide_counts.hip).  The statistics have the bits of the full-table run
(tests/test_gpu_wide_counts_ckpt.py), so the claim here is byte identity of everything written, and the stderr note that says what
the first counts E-step kept.  The full-table run itself is held against the reference's golden by tests/test_host_cli_wide_counts.py.
"""
import os
import subprocess
import pytest
from test_host_cli_wide_counts import run, CLI, HOST, ENV, NOTE_COUNTS

pytestmark = pytest.mark.gpu
BOOT = os.path.join(HOST, "psmc_boot")
INPUT = os.path.join(CLI, "small.psmcfa")
CKPT = "wide_ckpt=1,wide_counts_ckpt=1"
NOTE_CKPT = NOTE_COUNTS + ", X at every 8th bin\n"


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-s", "-C", os.path.join(os.path.dirname(HOST), "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", HOST], check=True)


def test_psmc_counts_from_checkpoints():
    """-N2 -p "100*2" on small.psmcfa: stdout byte for byte that of the run without the two options; the checkpointed run's note
    ends in the new wording, the other run's does not carry it; stderr differs in nothing else."""
    args = open(os.path.join(CLI, "small_n200_N2.args")).read().split()
    full = run(args, PSMC_HIP_WIDE_COUNTS="1", **ENV)
    ck = run(args, PSMC_HIP_WIDE_COUNTS="1", PSMC_HIP_OPTIONS=CKPT, **ENV)
    assert "RD\t2" in full.stdout and ck.stdout == full.stdout
    assert NOTE_CKPT in ck.stderr, ck.stderr
    assert NOTE_COUNTS + "\n" in full.stderr and "X at every 8th bin" not in full.stderr, full.stderr
    assert ck.stderr.replace(NOTE_CKPT, NOTE_COUNTS + "\n") == full.stderr
    # "wide_ckpt" alone: the counts E-steps keep the full table, and the note says nothing else
    one = run(args, PSMC_HIP_WIDE_COUNTS="1", PSMC_HIP_OPTIONS="wide_ckpt=1", **ENV)
    assert one.stdout == full.stdout and one.stderr == full.stderr


def test_psmc_boot_counts_from_checkpoints(tmp_path):
    """One psmc_boot job of two replicates with PSMC_FACTORED=0 PSMC_HIP_WIDE_COUNTS=1, with and without the two options: the
    replicates' files are the same bytes.  (psmc_boot sets "wide_batch" only for factored jobs; the options "wide_fast", "wide_batch"
    and "wide_counts" given through PSMC_HIP_OPTIONS send the replicates' full-count E-steps to the wide fast path in both jobs.)"""
    clean = ("PSMC_HIP_MODE", "PSMC_HIP_WIDE", "PSMC_HIP_WIDE_COUNTS", "PSMC_HIP_DECODE", "PSMC_HIP_OPTIONS", "PSMC_HIP_DEVICES", "PSMC_FACTORED",
             "PSMC_FAST_MSTEP", "PSMC_SEED", "PSMC_TIMING", "PSMC_BOOT_MAIN_CUS", "OMP_NUM_THREADS")
    base = "chunk=100,warmup=30,wide_fast=1,wide_batch=1,wide_counts=1"
    files = []
    for name, options in (("full", base), ("ckpt", base + "," + CKPT)):
        d = tmp_path / name
        d.mkdir()
        e = {k: v for k, v in os.environ.items() if k not in clean}
        e.update(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast", PSMC_FACTORED="0", PSMC_HIP_WIDE_COUNTS="1", PSMC_HIP_DEVICES="0", PSMC_HIP_OPTIONS=options)
        r = subprocess.run([BOOT, "-R", "2", "-S", "40", "-O", str(d / "r-%d.psmc"), "--", "-N2", "-p", "100*2", INPUT],
                           capture_output=True, text=True, env=e, timeout=600)
        assert r.returncode == 0, r.stderr[-1500:]
        files.append([open(d / ("r-%d.psmc" % k)).read() for k in range(2)])
    for k in range(2):
        assert "RD\t2" in files[0][k] and files[1][k] == files[0][k], k
