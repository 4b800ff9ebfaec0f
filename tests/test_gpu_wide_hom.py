"""Option "wide_hom_tiles": the wide fast path (129..1024 states) across runs of homozygosity by the transfer-matrix chain
(psmc_amd/csrc/estep_wide_gap.hip k_wf_hompilot / k_wf_hommat / k_wf_gapchain HOM, api_wide_fast.hip plan_wide_gaps).  Inputs are cut
from golden.segs_mid with planted runs of symbol 0 (tests/wide_hom_model.py, which also holds the numpy restatement of the generalised
plan rule).  References, gates and helpers are those of tests/test_gpu_wide_gap.py: the CPU oracle at 149 / 200 states, the exact
wide kernels on the same device beyond; bit-for-bit claims against a fresh context."""
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal, GOLD
from test_gpu_wide_fast import check, ran_wide
from test_gpu_wide_gap import reference, run, work, same_bits, params, level, SANDWICH
from wide_gap_model import sandwich, _called
from wide_hom_model import plan_rule, chain_rule, hom_sandwich, hom_mixed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module")
def wide():
    return dict(np.load(os.path.join(GOLD, "estep_wide.npz")))


# ------------------------------------------------------------------ (a) anchored sandwich
@pytest.mark.parametrize("n", [149, 200, 300, 768, 1024])
def test_hom_sandwich(hip, golden, oracle, wide, n):
    """300 called bins, 4096 homozygous, 300 called, tiles of 64 bins and a warm-up of 512: with the option the plan is the numpy rule's
    (63 tiles of class 4, at least 59 glued each way), no boundary fails in either direction (the chain starts at an anchored tile's
    exact exit vector) and the statistics pass every gate; without it the same input needs repair rounds each way -- a 512-bin window
    inside a homozygous run is 0.1 off -- and still passes."""
    segs = [hom_sandwich(golden.segs_mid[3])]
    par = params(n, wide)
    want = reference(hip, oracle, ("hom sandwich", n), n, par, segs)
    r, d, es = run(hip, n, segs, par, wide_hom_tiles=1, **SANDWICH)
    pt = es.wide_plan_tiles()
    chains = es.wide_gap_chains()
    es.close()
    cls, glue = plan_rule(segs, 64, 512)
    assert (cls == 4).sum() == 63 and (glue & 1).sum() >= 59 and (glue & 2).sum() >= 59
    assert np.array_equal(pt["cls"], cls) and np.array_equal(pt["glue"], glue), (pt, cls, glue)
    assert chains == list(chain_rule(segs, 64, 512)), chains
    print("hom sandwich", n, "on:", work(d))
    assert d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0, d
    check(r, want[0], want[1], want[2], ("hom sandwich", n, work(d)), (par[0], par[1]), segs)
    r0, d0, es0 = run(hip, n, segs, par, **SANDWICH)
    es0.close()
    print("hom sandwich", n, "off:", work(d0))
    assert d0["fwd_rounds"] > 0 and d0["bwd_rounds"] > 0, d0
    check(r0, want[0], want[1], want[2], ("hom sandwich, option off", n), (par[0], par[1]), segs)


# ------------------------------------------------------------------ (b) mixed
@pytest.mark.parametrize("both", [0, 1], ids=["hom", "hom+gap"])
@pytest.mark.parametrize("opts", [dict(chunk=100, warmup=30), dict(chunk=100, warmup=30, learn=0), dict(chunk=37, warmup=5)],
                         ids=lambda o: "-".join("%s%d" % kv for kv in o.items()))
@pytest.mark.parametrize("n", [200, 300])
def test_hom_mixed(hip, golden, oracle, wide, n, opts, both):
    """hom runs of 3000, 1200 (behind a stretch of tiles that hold both symbols 0 and 2), 200 (below "wide_hom_min" = 1000) and 1000 bins
    (directly behind 1000 missing bins), a second segment of data only, in tilings whose data tiles fail and are repaired around the
    runs -- with "wide_hom_tiles" alone and together with "wide_gap_tiles": classes, glue bits and chains are the numpy rule's, the
    result is right, and never ECONVERGE (it would raise)."""
    segs = hom_mixed(golden.segs_mid[3], golden.segs_mid[4])
    par = params(n, wide)
    want = reference(hip, oracle, ("hom mixed", n), n, par, segs)
    o = dict(wide_hom_tiles=1, wide_hom_min=1000)
    if both:
        o.update(wide_gap_tiles=1, wide_gap_min=1000)
    r, d, es = run(hip, n, segs, par, **o, **opts)
    pt = es.wide_plan_tiles()
    chains = es.wide_gap_chains()
    es.close()
    rule = dict(gap_min=1000, hom_min=1000, gap=bool(both), hom=True)
    cls, glue = plan_rule(segs, opts["chunk"], opts["warmup"], **rule)
    # (at tiles of 37 bins neither the 1000 missing bins nor the 1000 hom bins behind them hold 1000 bins of full tiles, and the tile
    # across their border holds both symbols: classes 1 and 3 there, one run of classes 2 and 4 at tiles of 100)
    assert (cls == 4).any() and (cls == 3).any() and (cls == 2).any() == (bool(both) and opts["chunk"] == 100)
    assert np.array_equal(pt["cls"], cls) and np.array_equal(pt["glue"], glue)
    assert chains == list(chain_rule(segs, opts["chunk"], opts["warmup"], **rule)), chains
    msg = ("hom mixed", n, opts, both, work(d), "chains %d + %d" % (len(chains[0]), len(chains[1])))
    print(msg)
    check(r, want[0], want[1], want[2], msg, (par[0], par[1]), segs)


# ------------------------------------------------------------------ (c) bits
def test_hom_bits(hip, golden, wide):
    """200 states on input (a): two E-steps of one context and a fresh context give the same bits, and the same matrix; on an input
    without a het-free tile the option gives the bits of the option off, and builds no matrix; "wide_hom_tiles" = 0 with
    "wide_gap_tiles" = 1 on the gap sandwich gives the bits of a run that never names the option."""
    n = 200
    par = params(n, wide)
    segs = [hom_sandwich(golden.segs_mid[3])]
    o = dict(wide_hom_tiles=1, **SANDWICH)
    r1, d1, e1 = run(hip, n, segs, par, steps=2, **o)
    M1, f1 = e1.wide_hom_matrix()
    r2, d2, e2 = run(hip, n, segs, par, **o)
    M2, f2 = e2.wide_hom_matrix()
    e1.close(); e2.close()
    assert same_bits(r1, r2) and d1 == d2 and bits_equal(M1, M2) and bits_equal(f1, f2)
    busy = _called(golden.segs_mid[4][:2500]).copy()
    busy[31::60] = 1   # a het in every window of 64 bins
    assert not plan_rule([busy], 64, 256)[0].any()
    ra, da, ea = run(hip, n, [busy], par, chunk=64, warmup=256, wide_hom_tiles=1)
    rb, db, eb = run(hip, n, [busy], par, chunk=64, warmup=256)
    assert same_bits(ra, rb) and da == db
    assert not ea.wide_plan_tiles()["cls"].any() and ea.wide_gap_chains() == [[], []]
    with pytest.raises(hip.HipError, match="built no matrix of a homozygous tile"):
        ea.wide_hom_matrix()
    ea.close(); eb.close()
    gs = [sandwich(golden.segs_mid[3])]
    rg, dg, eg = run(hip, n, gs, par, wide_gap_tiles=1, **SANDWICH)               # the path of tests/test_gpu_wide_gap.py, untouched
    rh, dh, eh = run(hip, n, gs, par, wide_gap_tiles=1, wide_hom_tiles=0, wide_hom_min=64, **SANDWICH)
    assert same_bits(rg, rh) and dg == dh
    assert np.array_equal(eg.wide_plan_tiles()["cls"], eh.wide_plan_tiles()["cls"]) and bits_equal(eg.wide_gap_matrix(), eh.wide_gap_matrix())
    eg.close(); eh.close()


def test_gap_run_through_the_hom_chain(hip, golden, wide):
    """A run of gap tiles alone gives the same bits whichever instantiation of the chain crosses it: the gap sandwich beside the hom
    sandwich with both options on (every chain of the plan runs in the HOM instantiation) leaves, on the gap segment's tiles, the
    start vectors of both directions that the gap sandwich alone leaves with "wide_gap_tiles" alone (the plain instantiation)."""
    n = 200
    par = params(n, wide)
    g, h = sandwich(golden.segs_mid[3]), hom_sandwich(golden.segs_mid[3])
    r1, d1, e1 = run(hip, n, [g, h], par, wide_gap_tiles=1, wide_hom_tiles=1, **SANDWICH)
    r0, d0, e0 = run(hip, n, [g], par, wide_gap_tiles=1, **SANDWICH)
    nt = len(e0.wide_plan_tiles()["cls"])
    c1 = e1.wide_plan_tiles()["cls"]
    assert (c1[:nt] == 2).sum() == 63 and (c1[nt:] == 4).sum() == 63
    assert d1["fwd_rounds"] == 0 and d1["bwd_rounds"] == 0 and d0["fwd_rounds"] == 0 and d0["bwd_rounds"] == 0
    for which in (0, 1):   # (a segment's first tile builds on a0 and has no forward start vector: nobody writes that row)
        assert bits_equal(e1.wide_tile_vectors(which)[1 - which:nt], e0.wide_tile_vectors(which)[1 - which:]), which
    assert bits_equal(e1.wide_gap_matrix(), e0.wide_gap_matrix())
    e1.close(); e0.close()


# ------------------------------------------------------------------ (d) consumers, 200 states on input (a)
def test_hom_ckpt_and_decode(hip, golden, wide):
    """ "wide_ckpt" = 1: the bits of the full table.  "wide_decode" after an E-step with the option: posterior, path and scales against
    the exact kernels under the tolerances of tests/test_gpu_wide_fast_decode.py."""
    from test_gpu_wide_fast_decode import compare
    n = 200
    segs = [hom_sandwich(golden.segs_mid[3])]
    a, e, a0 = params(n, wide)
    o = dict(wide_hom_tiles=1, **SANDWICH)
    r1, d1, e1 = run(hip, n, segs, (a, e, a0), **o)
    rc, dc, ec = run(hip, n, segs, (a, e, a0), wide_ckpt=1, **o)
    assert ec.wide_table_info()["interval"] == 8 and same_bits(rc, r1)
    assert dc["fwd_rounds"] == 0 and dc["bwd_rounds"] == 0, dc
    e1.close(); ec.close()
    ex = hip.HipEStep(n, mode=hip.MODE_EXACT)
    ex.load_segments(segs)
    ex.estep(a, e, a0)
    rf, d, fast = run(hip, n, segs, (a, e, a0), wide_decode=1, **o)
    assert d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0, d
    compare(fast, ex, segs, n, E=rf["E"])
    fast.close(); ex.close()


def test_hom_counts(hip, golden, oracle, wide):
    """ "wide_counts": the full count matrix after an E-step with the option, against the oracle under the gates of
    tests/test_gpu_wide_counts.py."""
    from test_gpu_wide_counts import gate
    n = 200
    segs = [hom_sandwich(golden.segs_mid[3])]
    par = params(n, wide)
    want = reference(hip, oracle, ("hom sandwich", n), n, par, segs)
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), wide_counts=1, wide_hom_tiles=1, **SANDWICH)
    es.load_segments(segs)
    r = es.estep(*par)
    d = es.fast_diag()
    es.close()
    assert d["back_half"] == 4 and d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0, d
    gate(r, dict(A=want[3], E=want[1], LL=want[2]), (par[0], par[1]), ("hom counts", n))


def test_hom_batch_and_group(hip, golden, oracle, wide):
    """ "wide_batch": a batch of two multisets, one repeating the segment with the run, equals two single E-steps bit for bit.  A group
    of two shards on one device with the option set through psmc_hip_group_set_option passes the gates."""
    n = 200
    segs = [hom_sandwich(golden.segs_mid[3]), golden.segs_mid[4][:2500], golden.segs_small[7]]
    par = params(n, wide)
    sels = [[0, 0, 2], [1, 2, 0]]
    opts = dict(wide_hom_tiles=1, **SANDWICH)
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), wide_batch=1, **opts)
    es.load_segments(segs)
    b = es.estep_batch([par, par], sels, want="sums")
    es.close()
    for i, sel in enumerate(sels):
        one = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), **opts)
        one.load_segments(segs)
        one.select(sel)
        r = one.estep_factored(par[0], par[1][:2], par[2])
        assert (one.wide_plan_tiles()["cls"] == 4).any()
        one.close()
        assert bits_equal(b["sums"][i], r["sums"]) and bits_equal(b["E"][i], r["E"]) and b["LL"][i] == r["LL"], (n, i)
    want = reference(hip, oracle, ("hom group", n), n, par, segs)
    g = hip.HipGroup(n, [0, 0], mode=hip.MODE_FAST, wide_fast=level(n))
    for k, v in opts.items():
        g.set_option(k, v)
    g.load_segments(segs)
    r = g.estep_factored(par[0], par[1][:2], par[2])
    g.close()
    check(r, want[0], want[1], want[2], ("hom group [0, 0]", n), (par[0], par[1]), segs)


# ------------------------------------------------------------------ options
def test_hom_options(hip, golden, wide):
    """Bad values are EINVAL; the matrix diagnostic is ESTATE before any E-step; without "wide_fast" the option changes nothing."""
    a, e, a0 = params(200, wide)
    segs = [hom_sandwich(golden.segs_mid[3])]
    es = hip.HipEStep(200, mode=hip.MODE_FAST, wide_fast=1)
    for k, v in (("wide_hom_tiles", 2), ("wide_hom_tiles", -1), ("wide_hom_tiles", 0.5), ("wide_hom_min", -1)):
        with pytest.raises(hip.HipError, match="(?i)invalid"):
            es.set_option(k, v)
    es.set_option("wide_hom_tiles", 1); es.set_option("wide_hom_min", 0); es.set_option("wide_hom_min", 2048)
    es.load_segments(segs)
    for k, v in SANDWICH.items():
        es.set_option(k, v)
    with pytest.raises(hip.HipError, match="no current wide plan"):
        es.wide_hom_matrix()
    es.estep_factored(a, e[:2], a0)
    M, fac = es.wide_hom_matrix()
    assert M.shape == (200, 256) and fac.shape == (16,) and (np.frexp(fac)[0] == 0.5).all()
    with pytest.raises(hip.HipError, match="built no transfer matrix"):   # no gap tile in the plan: no matrix of one
        es.wide_gap_matrix()
    es.set_option("wide_hom_min", 8192)   # the plan is dirty; then: the run is too short, class 3, no chain, no matrix
    with pytest.raises(hip.HipError, match="no current wide plan"):
        es.wide_hom_matrix()
    es.estep_factored(a, e[:2], a0)
    assert (es.wide_plan_tiles()["cls"] == 3).sum() >= 63 and es.wide_gap_chains() == [[], []]
    with pytest.raises(hip.HipError, match="built no matrix of a homozygous tile"):
        es.wide_hom_matrix()
    es.close()
    out = []
    for opts in (dict(), dict(wide_hom_tiles=1)):   # without "wide_fast": the exact wide kernels, whatever the option says
        es = hip.HipEStep(200, mode=hip.MODE_FAST, **opts)
        es.load_segments(segs)
        out.append(es.estep(a, e, a0))
        es.close()
    assert bits_equal(out[0]["A"], out[1]["A"]) and bits_equal(out[0]["E"], out[1]["E"]) and out[0]["LL"] == out[1]["LL"]
