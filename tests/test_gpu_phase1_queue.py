"""Phase 1 from a work queue ("phase1" = 1, estep_struct.hip k_phase1_queue) against the two launches it replaces ("phase1" = 0):
which wave runs a block must not change what the block computes, so A, E and LL are the same bits over a moving-parameter
trajectory -- on the fixture inputs (plans with repairs, learned runs, coarse items, the fix pass), on rank 0's share of the
genome at 8 GPUs and on the benchmark genome itself."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENOME = dict(two_phase=2, merge1=0, warm_shift=1, kc_sub=4)   # the genome's plan at fixture size (tests/test_gpu_estep.py)


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


def trajectory(n):
    from psmc_amd import hostlib
    tj = json.load(open(os.path.join(ROOT, "tests", "golden", "traj_n64.json")))
    return [hostlib.hmm_params(tj["pattern"], r["params"]) for r in tj["rounds"] if r["round"] >= 1][:n]


def same_bits(hip, segs, steps, **opts):
    """phase1=1 and phase1=0 side by side over `steps` E-steps of the trajectory; returns the last diag of the queue context"""
    q = hip.HipEStep(64, mode=hip.MODE_FAST, phase1=1, **opts)
    s = hip.HipEStep(64, mode=hip.MODE_FAST, phase1=0, **opts)
    q.load_segments(segs); s.load_segments(segs)
    for it, (a, e, a0) in enumerate(trajectory(steps)):
        rq, rs = q.estep(a, e, a0), s.estep(a, e, a0)
        assert np.array_equal(rq["A"], rs["A"]) and np.array_equal(rq["E"], rs["E"]), (it, opts)
        assert rq["LL"] == rs["LL"], (it, rq["LL"], rs["LL"], opts)
        dq, ds = q.fast_diag(), s.fast_diag()
        for k in ("fwd_rounds", "bwd_rounds", "fwd_tiles", "bwd_tiles", "n_chunks"):   # the same repairs, the same plan
            assert dq[k] == ds[k], (it, k, dq[k], ds[k], opts)
    q.close(); s.close()
    return dq


@pytest.mark.parametrize("opts", [dict(chunk=768, warmup=64, merge1=0), dict(chunk=256, warmup=512, **GENOME),
                                  dict(chunk=1000, warmup=100, **GENOME), dict(chunk=768, warmup=64, merge=1, adapt=1, prev_start=1, **GENOME),
                                  dict(chunk=256, warmup=512, coarse=2, **GENOME), dict(chunk=1000, warmup=100, kc_min=2, **GENOME),
                                  dict(chunk=768, warmup=64, learn=0, **GENOME)])
def test_phase1_queue_bit_identical_fixture(hip, golden, opts):
    """Short warm-ups: repairs in every E-step (learn=0: forced in every one), glued runs walked and chained once learned."""
    same_bits(hip, golden.segs_mid, 6, **opts)


def test_phase1_queue_bit_identical_share(hip):
    """Rank 0's LPT share of the genome at 8 GPUs, planned as two rounds so that the queue runs (its own plan is one grid)."""
    from psmc_amd import sim
    from psmc_amd.dist import partition_segments
    a, e, a0 = trajectory(1)[0]
    lens = sim.human_like_lengths(30_000_000, n_seg=90)
    share = partition_segments(lens, 8)[0]
    segs = sim.simulate_genome(a, e, a0, lens[share], seed=43)
    same_bits(hip, segs, 5, two_phase=2, merge1=0)


def test_phase1_queue_bit_identical_genome(hip, golden):
    """The benchmark's workload (config 3, 30 M bins) with its own plan: the queue is the default path there."""
    from psmc_amd import sim
    p = golden.params("n64_curve")
    lens = sim.human_like_lengths(30_000_000, n_seg=90)
    segs = sim.simulate_genome(p["a"], p["e"], p["a0"], lens, seed=43)
    same_bits(hip, segs, 5)


@pytest.mark.parametrize("phase1", [1, 0])
def test_phase1_option_selects_the_launch(hip, phase1):
    """The option really switches paths: with PSMC_HIP_DEBUG_SYNC every launch names itself on stderr (a fresh process: the
    library reads that variable once)."""
    code = ("import sys; sys.path.insert(0, %r); import numpy as np; from psmc_amd import hip, sim\n"
            "import json\n"
            "from psmc_amd import hostlib\n"
            "tj = json.load(open(%r)); a, e, a0 = hostlib.hmm_params(tj['pattern'], tj['rounds'][1]['params'])\n"
            "segs = [sim.simulate_segment(a, e, a0, n, np.random.default_rng(n)) for n in (40000, 25000, 9000)]\n"
            "es = hip.HipEStep(64, mode=hip.MODE_FAST, phase1=%d, chunk=768, warmup=64, merge1=0)\n"
            "es.load_segments(segs); es.estep(a, e, a0); es.close()\n"
            % (ROOT, os.path.join(ROOT, "tests", "golden", "traj_n64.json"), phase1))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PSMC_HIP_DEBUG_SYNC="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert ("launch_phase1_queue" in r.stderr) == (phase1 == 1), r.stderr[-2000:]
    assert ("launch_bwd_struct(4," in r.stderr) == (phase1 == 0), r.stderr[-2000:]
