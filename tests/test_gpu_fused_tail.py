"""The tail of the fused back half ("tail" = 1: the counts waves verify the backward boundaries themselves, the reductions follow
the counts and sum list A's partials beside list B -- estep_fused.hip tail_verify, estep_fast.hip launch_fast) against the launches
it replaces ("tail" = 0).  Who tests a boundary and when the partials are summed must not change a bit: two contexts on the same
segments, five E-steps over a moving-parameter trajectory, and after every step the same statistics (bits), the same repairs and
the same boundary errors; then the "tail" = 1 result against the oracle with the suite's bounds."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENOME = dict(two_phase=2, merge1=0, warm_shift=1, kc_sub=4)   # the genome's plan at fixture size (tests/test_gpu_estep.py)
REPAIRS = ("fwd_rounds", "bwd_rounds", "fwd_tiles", "bwd_tiles", "merged", "recounted", "n_chunks")
ERRORS = ("warm_err_fwd", "warm_err_bwd")
# the warm-up of the cases whose backward speculation must FAIL: on the CPU model (tests/fastmodel.py) 32 bins leave a boundary
# mismatch far above warm_tol = 1e-12 for these parameters (asserted in test_short_warmup_fails_on_the_cpu_model)
W_SHORT = 32


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


def simulated(lens):
    from psmc_amd import sim
    a, e, a0 = trajectory(1)[0]
    return [sim.simulate_segment(a, e, a0, n, np.random.default_rng(n)) for n in lens]


@pytest.fixture(scope="module")
def segs_two():
    return simulated((4099, 1031))


@pytest.fixture(scope="module")
def n128(golden, oracle):
    """model, segments and oracle result of the fused 128-state kernel's test (tests/test_gpu_estep.py test_fast_n128), computed once"""
    g, k = golden.n128, "n128_curve"
    par = (g[k + ".a"], g[k + ".e"], g[k + ".a0"])
    segs = golden.segs_small + golden.segs_mid[2:]
    return par, segs, oracle.estep(par[0], par[1], par[2], segs)


def same_step(t0, t1, r0, r1, where):
    assert np.array_equal(r1["A"], r0["A"]) and np.array_equal(r1["E"], r0["E"]), where
    assert r1["LL"] == r0["LL"], (where, r1["LL"], r0["LL"])
    d0, d1 = t0.fast_diag(), t1.fast_diag()
    for k in REPAIRS + ERRORS:   # the same tiles flagged and repaired, the same largest mismatch of the last verify (bits)
        assert d1[k] == d0[k], (where, k, d1[k], d0[k])
    return d1


def pair(hip, n, segs, **opts):
    t0 = hip.HipEStep(n, mode=hip.MODE_FAST, tail=0, **opts)
    t1 = hip.HipEStep(n, mode=hip.MODE_FAST, tail=1, **opts)
    t0.load_segments(segs); t1.load_segments(segs)
    return t0, t1


def side_by_side(hip, oracle, segs, steps=5, **opts):
    """64 states: `steps` E-steps of the trajectory on both contexts; returns the diag of every step ("tail" = 1)"""
    from test_gpu_estep import check_fast
    t0, t1 = pair(hip, 64, segs, **opts)
    diags = []
    for it, (a, e, a0) in enumerate(trajectory(steps)):
        r0, r1 = t0.estep(a, e, a0), t1.estep(a, e, a0)
        diags.append(same_step(t0, t1, r0, r1, (it, opts)))
    assert diags[-1]["back_half"] == 1 and diags[-1]["structured"], diags[-1]
    check_fast(r1, oracle.estep(a, e, a0, segs), dict(a=a, e=e))
    t0.close(); t1.close()
    return diags


def test_short_warmup_fails_on_the_cpu_model(segs_two):
    """Cases (b), (c), (e) rely on a failing backward speculation: at W_SHORT bins of warm-up a boundary exceeds warm_tol."""
    import fastmodel
    a, e, a0 = trajectory(1)[0]
    st = {}
    fastmodel.estep_fast_model(a, e, a0, segs_two[1:], T=256, W=W_SHORT, tol=1e-12, stats=st)
    assert st["bwd_rounds"] > 0, st


def test_tail_from_above_tiles(hip, oracle, segs_two):
    """(a) tile lengths that are no multiple of 4, a short last tile, from-above tiles in list B; nothing flagged once learned"""
    d = side_by_side(hip, oracle, segs_two, chunk=256, warmup=512, **GENOME)
    assert d[-1]["fused_launches"] == 2, d[-1]


def test_tail_flagged_tiles(hip, oracle, segs_two):
    """(b) the backward speculation fails: flags from the counts waves, repair rounds, recount and the second tail"""
    d = side_by_side(hip, oracle, segs_two, chunk=256, warmup=W_SHORT, **GENOME)
    assert d[0]["bwd_tiles"] > 0 and d[0]["recounted"] == 1, d[0]


def test_tail_glued_runs(hip, oracle, segs_two):
    """(c) the plan of (b) until learn_groups has glued runs (their pairs are left to k_verify), then two more steps"""
    from test_gpu_estep import check_fast
    t0, t1 = pair(hip, 64, segs_two, chunk=256, warmup=W_SHORT, **GENOME)
    tr = trajectory(5)
    glued_at = None
    for it in range(10):
        a, e, a0 = tr[it % len(tr)]
        same_step(t0, t1, t0.estep(a, e, a0), t1.estep(a, e, a0), it)
        p0, p1 = t0.fast_plan(), t1.fast_plan()
        assert p0 == p1, (it, p0, p1)
        if p1["glued_bwd"] > 0 and glued_at is None:
            glued_at = it
        if glued_at is not None and it >= glued_at + 2:
            break
    assert glued_at is not None, p1
    r1 = t1.estep(a, e, a0)
    check_fast(r1, oracle.estep(a, e, a0, segs_two), dict(a=a, e=e))
    t0.close(); t1.close()


@pytest.mark.parametrize("lens", [(300,), (257,), (300, 257)])
def test_tail_single_tiles(hip, oracle, lens):
    """(d) one tile with nothing to compare; 257 bins at chunk 256: the upper tile holds only position L and owns no transition"""
    side_by_side(hip, oracle, simulated(lens), chunk=256, warmup=512, **GENOME)
    side_by_side(hip, oracle, simulated(lens), chunk=256, warmup=W_SHORT, **GENOME)


@pytest.mark.parametrize("warmup", [512, W_SHORT])
def test_tail_n128(hip, n128, warmup):
    """(e) 128 states (k_bwd_count8x_struct: sixteen tiles per work-group, each wave its own four)"""
    from test_gpu_estep import check_fast
    (a, e, a0), segs, o = n128
    t0, t1 = pair(hip, 128, segs, chunk=256, warmup=warmup, **GENOME)
    for it in range(5):
        r0, r1 = t0.estep(a, e, a0), t1.estep(a, e, a0)
        d = same_step(t0, t1, r0, r1, (it, warmup))
        if it == 0 and warmup == W_SHORT:
            assert d["bwd_tiles"] > 0, d
    assert d["back_half"] == 1, d
    check_fast(r1, o)
    t0.close(); t1.close()


def test_tail_is_inert_elsewhere(hip, segs_two):
    """(f) the factored back half and the unfused one have no such tail: the option changes nothing"""
    for opts in (dict(chunk=256, warmup=512, **GENOME), dict(chunk=256, warmup=W_SHORT, fuse=0)):
        t0, t1 = pair(hip, 64, segs_two, **opts)
        for it, (a, e, a0) in enumerate(trajectory(3)):
            if "fuse" in opts:
                same_step(t0, t1, t0.estep(a, e, a0), t1.estep(a, e, a0), (it, opts))
            else:
                r0, r1 = t0.estep_factored(a, e, a0), t1.estep_factored(a, e, a0)
                assert np.array_equal(r1["sums"], r0["sums"]) and np.array_equal(r1["E"], r0["E"]) and r1["LL"] == r0["LL"], it
                d0, d1 = t0.fast_diag(), t1.fast_diag()
                assert all(d1[k] == d0[k] for k in REPAIRS + ERRORS) and d1["back_half"] == 2, (d0, d1)
        t0.close(); t1.close()


def test_tail_option_is_validated(hip):
    es = hip.HipEStep(64, mode=hip.MODE_FAST)
    for bad in (-1, 2, 0.5):
        with pytest.raises(hip.HipError):
            es.set_option("tail", bad)
    es.set_option("tail", 0); es.set_option("tail", 1)
    es.close()
