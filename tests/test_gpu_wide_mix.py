"""Option "wide_mix_tiles": the wide fast path (129..1024 states) across het-free tiles that hold both symbol 0 and `N`, by the
transfer-matrix chain with two matrices per such tile (psmc_amd/csrc/estep_wide_gap.hip k_wf_mixpilot / k_wf_mixmat / k_wf_gapchain MIX,
api_wide_fast.hip plan_wide_gaps).  Inputs: mix_sandwich of tests/wide_mix_model.py (which also holds the numpy restatement of the
rule) and hom_mixed of tests/wide_hom_model.py.  References, gates and helpers are those of tests/test_gpu_wide_gap.py: the CPU oracle
at 149 / 200 states, the exact wide kernels on the same device beyond; bit-for-bit claims against a fresh context."""
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal, GOLD
from test_gpu_wide_fast import check
from test_gpu_wide_gap import reference, run, work, same_bits, params, level, SANDWICH
from wide_gap_model import _called
from wide_hom_model import hom_mixed, hom_sandwich
import wide_hom_model as hm
from wide_mix_model import plan_rule, chain_rule, mix_sandwich, cap_tiles

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL3 = dict(wide_gap_tiles=1, wide_hom_tiles=1, wide_mix_tiles=1)
HOM_MIX = dict(wide_hom_tiles=1, wide_mix_tiles=1)
SIZES = [149, 200, 300, 1024]


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module")
def wide():
    return dict(np.load(os.path.join(GOLD, "estep_wide.npz")))


def plan_of(es):
    pt = es.wide_plan_tiles()
    return pt["cls"], pt["glue"], es.wide_gap_chains()


# ------------------------------------------------------------------ (a) the sandwich
@pytest.mark.parametrize("n", SIZES)
def test_mix_sandwich(hip, golden, oracle, wide, n):
    """mix_sandwich at tiles of 64 bins and a warm-up of 512, all three options: the plan and the chains are the numpy rule's (59 tiles
    of class 6, two of class 4, two of class 2: one run), no boundary fails in either direction -- 0 rounds at the run, and the data tiles
    are anchored -- and the statistics pass every gate.  With "wide_gap_tiles" and "wide_hom_tiles" alone the mix tiles are data tiles
    between two lone two-tile runs: not fewer repair rounds (printed), and the same gates."""
    segs = [mix_sandwich(golden.segs_mid[3])]
    par = params(n, wide)
    want = reference(hip, oracle, ("mix sandwich", n), n, par, segs)
    r, d, es = run(hip, n, segs, par, **ALL3, **SANDWICH)
    cls, glue, chains = plan_of(es)
    es.close()
    wc, wg = plan_rule(segs, 64, 512, gap=True, hom=True)
    assert (wc == 6).sum() == 59 and (wc == 4).sum() == 2 and (wc == 2).sum() == 2
    assert np.array_equal(cls, wc) and np.array_equal(glue, wg), (cls, wc, glue, wg)
    assert chains == list(chain_rule(segs, 64, 512, gap=True, hom=True)), chains
    r0, d0, es0 = run(hip, n, segs, par, wide_gap_tiles=1, wide_hom_tiles=1, **SANDWICH)
    c0, g0, ch0 = plan_of(es0)
    es0.close()
    oc, og = hm.plan_rule(segs, 64, 512, gap=True, hom=True)
    assert np.array_equal(c0, oc) and np.array_equal(g0, og)
    print("mix sandwich", n, "with wide_mix_tiles:", work(d), "| without:", work(d0))
    assert d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0, d
    assert d["fwd_rounds"] <= d0["fwd_rounds"] and d["bwd_rounds"] <= d0["bwd_rounds"], (d, d0)
    check(r, want[0], want[1], want[2], ("mix sandwich", n, work(d)), (par[0], par[1]), segs)
    check(r0, want[0], want[1], want[2], ("mix sandwich, wide_mix_tiles off", n), (par[0], par[1]), segs)


def test_mix_sandwich_without_the_gap_option(hip, golden, oracle, wide):
    """wide_hom_tiles=1,wide_mix_tiles=1 alone, as the psmc binary's users would set it: the two gap tiles are data tiles, the stretch is
    two runs, the second chained one level later behind the walk through them; the plan is the rule's, no round runs, the result is right."""
    n = 200
    segs = [mix_sandwich(golden.segs_mid[3])]
    par = params(n, wide)
    want = reference(hip, oracle, ("mix sandwich", n), n, par, segs)
    r, d, es = run(hip, n, segs, par, **HOM_MIX, **SANDWICH)
    cls, glue, chains = plan_of(es)
    es.close()
    wc, wg = plan_rule(segs, 64, 512)
    assert np.array_equal(cls, wc) and np.array_equal(glue, wg) and not cls[40:42].any() and (cls == 6).sum() == 59
    assert chains == list(chain_rule(segs, 64, 512)) and max(c[3] for c in chains[0]) == 1, chains
    print("mix sandwich, hom + mix", n, work(d))
    assert d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0, d
    check(r, want[0], want[1], want[2], ("mix sandwich, hom + mix", n, work(d)), (par[0], par[1]), segs)


# ------------------------------------------------------------------ (b) hom_mixed
@pytest.mark.parametrize("opts", [dict(chunk=100, warmup=400), dict(chunk=100, warmup=30), dict(chunk=37, warmup=5)],
                         ids=lambda o: "-".join("%s%d" % kv for kv in o.items()))
@pytest.mark.parametrize("n", SIZES)
def test_mix_hom_mixed(hip, golden, oracle, wide, n, opts):
    """hom_mixed with "wide_hom_min" = 1000: the 300 alternating bins join the runs on both sides into one (at tiles of 100); at tiles of
    37 bins most tiles of that stretch hold both symbols too.  Classes, glue bits and chains are the numpy rule's, the result is right,
    never ECONVERGE (it would raise), and not more repair rounds than with "wide_hom_tiles" alone (both printed; the data tiles of these
    tilings fail and are repaired around the runs either way)."""
    segs = hom_mixed(golden.segs_mid[3], golden.segs_mid[4])
    par = params(n, wide)
    want = reference(hip, oracle, ("hom mixed", n), n, par, segs)
    r, d, es = run(hip, n, segs, par, wide_hom_min=1000, **HOM_MIX, **opts)
    cls, glue, chains = plan_of(es)
    es.close()
    wc, wg = plan_rule(segs, opts["chunk"], opts["warmup"], hom_min=1000)
    assert (wc == 6).any() and (wc == 4).any()
    if opts["chunk"] == 100:
        assert list(wc[44:49]) == [4, 6, 6, 6, 4]
    assert np.array_equal(cls, wc) and np.array_equal(glue, wg)
    assert chains == list(chain_rule(segs, opts["chunk"], opts["warmup"], hom_min=1000)), chains
    r0, d0, es0 = run(hip, n, segs, par, wide_hom_min=1000, wide_hom_tiles=1, **opts)
    es0.close()
    msg = ("hom mixed", n, opts, "with wide_mix_tiles:", work(d), "| without:", work(d0), "chains %d + %d" % (len(chains[0]), len(chains[1])))
    print(*msg)
    check(r, want[0], want[1], want[2], msg, (par[0], par[1]), segs)
    assert d["fwd_rounds"] <= d0["fwd_rounds"] and d["bwd_rounds"] <= d0["bwd_rounds"], (d, d0)


# ------------------------------------------------------------------ (c) bits
def test_mix_bits(hip, golden, wide):
    """200 states.  Two E-steps of one context and a fresh context give the same bits, statistics and matrices.  "wide_mix_tiles" = 0
    gives the bits and the plan of leaving it unset; so does "wide_mix_tiles" = 1 without "wide_hom_tiles".  On inputs without a class-3
    chain tile (a pure hom run; no het-free tile at all) the option on gives the plan and the bits of the option off and builds no
    matrix of a mix tile."""
    n = 200
    par = params(n, wide)
    segs = [mix_sandwich(golden.segs_mid[3])]
    o = dict(**ALL3, **SANDWICH)
    r1, d1, e1 = run(hip, n, segs, par, steps=2, **o)
    r2, d2, e2 = run(hip, n, segs, par, **o)
    assert same_bits(r1, r2) and d1 == d2
    for t, dr in ((9, 0), (10, 1), (30, 1), (67, 0), (5, 1)):
        (Ma, fa), (Mb, fb) = e1.wide_mix_matrix(t, dr), e2.wide_mix_matrix(t, dr)
        assert bits_equal(Ma, Mb) and bits_equal(fa, fb)
    e1.close(); e2.close()
    base = dict(wide_gap_tiles=1, wide_hom_tiles=1, **SANDWICH)
    ru, du, eu = run(hip, n, segs, par, **base)
    rz, dz, ez = run(hip, n, segs, par, wide_mix_tiles=0, wide_mix_mb=64, **base)
    assert same_bits(ru, rz) and du == dz and all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(plan_of(eu), plan_of(ez)))
    with pytest.raises(hip.HipError, match="built no matrix of a mix tile"):
        ez.wide_mix_matrix(5, 0)
    eu.close(); ez.close()
    rg, dg, eg = run(hip, n, segs, par, wide_gap_tiles=1, **SANDWICH)
    rm, dm, em = run(hip, n, segs, par, wide_gap_tiles=1, wide_mix_tiles=1, **SANDWICH)   # without "wide_hom_tiles": no effect
    assert same_bits(rg, rm) and dg == dm and np.array_equal(eg.wide_plan_tiles()["cls"], em.wide_plan_tiles()["cls"])
    eg.close(); em.close()
    busy = _called(golden.segs_mid[4][:2500]).copy()
    busy[31::60] = 1   # a het in every window of 64 bins
    for inp, has_run in (([hom_sandwich(golden.segs_mid[3])], True), ([busy], False)):   # (neither holds a missing bin)
        wc, wg = hm.plan_rule(inp, 64, 256)
        assert not (plan_rule(inp, 64, 256)[0] >= 5).any() and (wc == 4).any() == has_run
        ra, da, ea = run(hip, n, inp, par, chunk=64, warmup=256, **HOM_MIX)
        rb, db, eb = run(hip, n, inp, par, chunk=64, warmup=256, wide_hom_tiles=1)
        assert same_bits(ra, rb) and da == db
        assert np.array_equal(ea.wide_plan_tiles()["cls"], wc) and ea.wide_gap_chains() == eb.wide_gap_chains()
        with pytest.raises(hip.HipError, match="built no matrix of a mix tile"):
            ea.wide_mix_matrix(5, 0)
        ea.close(); eb.close()


def test_mix_cap(hip, golden, wide):
    """ "wide_mix_mb" = 1 at 1024 states admits no tile (a tile's two matrices are 16.8 MB): glue, chains and bits are those of the option
    off, and the refused tiles are reported as class 5 where the option off reports 0.  At 200 states 1 MB admits one tile, tile 5,
    which alone is a run of 64 bins and does not qualify (class 5, no class 6); 8 MB admits nine, tiles 5 .. 13, one qualifying run in
    front of the first refused tile: classes, glue and chains are the rule's under that cap."""
    segs = [mix_sandwich(golden.segs_mid[3])]
    n = 1024
    par = params(n, wide)
    assert cap_tiles(n, 1) == 0
    base = dict(wide_gap_tiles=1, wide_hom_tiles=1, **SANDWICH)
    r1, d1, e1 = run(hip, n, segs, par, wide_mix_tiles=1, wide_mix_mb=1, **base)
    r0, d0, e0 = run(hip, n, segs, par, **base)
    c1, g1, ch1 = plan_of(e1)
    c0, g0, ch0 = plan_of(e0)
    e1.close(); e0.close()
    assert same_bits(r1, r0) and d1 == d0 and np.array_equal(g1, g0) and ch1 == ch0
    wc, wg = plan_rule(segs, 64, 512, gap=True, hom=True, mix_tiles=0)
    assert np.array_equal(c1, wc) and (c1 == 5).sum() >= 59 and not (c1 == 6).any() and np.array_equal(np.where(c1 == 5, 0, c1), c0)
    n = 200
    par = params(n, wide)
    for mb in (1, 8):
        k = cap_tiles(n, mb)
        r, d, es = run(hip, n, segs, par, wide_mix_tiles=1, wide_mix_mb=mb, **base)
        c, g, ch = plan_of(es)
        es.close()
        wc, wg = plan_rule(segs, 64, 512, gap=True, hom=True, mix_tiles=k)
        assert np.array_equal(c, wc) and np.array_equal(g, wg) and ch == list(chain_rule(segs, 64, 512, gap=True, hom=True, mix_tiles=k)), (mb, k)
        assert (c == 6).sum() == (9 if mb == 8 else 0) and (c == 5).sum() == 59 - (c == 6).sum(), (mb, k, c)


# ------------------------------------------------------------------ (d) consumers, 200 states on the sandwich
def test_mix_ckpt_and_decode(hip, golden, wide):
    """ "wide_ckpt" = 1: the bits of the full table.  "wide_decode" after an E-step with the option: posterior, path and scales against
    the exact kernels under the tolerances of tests/test_gpu_wide_fast_decode.py."""
    from test_gpu_wide_fast_decode import compare
    n = 200
    segs = [mix_sandwich(golden.segs_mid[3])]
    a, e, a0 = params(n, wide)
    o = dict(**ALL3, **SANDWICH)
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


def test_mix_counts(hip, golden, oracle, wide):
    """ "wide_counts": the full count matrix after an E-step with the option, against the oracle under the gates of
    tests/test_gpu_wide_counts.py."""
    from test_gpu_wide_counts import gate
    n = 200
    segs = [mix_sandwich(golden.segs_mid[3])]
    par = params(n, wide)
    want = reference(hip, oracle, ("mix sandwich", n), n, par, segs)
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), wide_counts=1, **ALL3, **SANDWICH)
    es.load_segments(segs)
    r = es.estep(*par)
    d = es.fast_diag()
    assert (es.wide_plan_tiles()["cls"] == 6).sum() == 59
    es.close()
    assert d["back_half"] == 4 and d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0, d
    gate(r, dict(A=want[3], E=want[1], LL=want[2]), (par[0], par[1]), ("mix counts", n))


def test_mix_batch_and_group(hip, golden, oracle, wide):
    """ "wide_batch": a batch of two multisets, one repeating the segment with the run, equals two single E-steps bit for bit.  A group
    of two shards on one device with the options set through psmc_hip_group_set_option passes the gates."""
    n = 200
    segs = [mix_sandwich(golden.segs_mid[3]), golden.segs_mid[4][:2500], golden.segs_small[7]]
    par = params(n, wide)
    sels = [[0, 0, 2], [1, 2, 0]]
    opts = dict(**ALL3, **SANDWICH)
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), wide_batch=1, **opts)
    es.load_segments(segs)
    b = es.estep_batch([par, par], sels, want="sums")
    es.close()
    for i, sel in enumerate(sels):
        one = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), **opts)
        one.load_segments(segs)
        one.select(sel)
        r = one.estep_factored(par[0], par[1][:2], par[2])
        assert (one.wide_plan_tiles()["cls"] == 6).sum() == 59   # (a repeated segment is planned once, with a multiplicity)
        one.close()
        assert bits_equal(b["sums"][i], r["sums"]) and bits_equal(b["E"][i], r["E"]) and b["LL"][i] == r["LL"], (n, i)
    want = reference(hip, oracle, ("mix group", n), n, par, segs)
    g = hip.HipGroup(n, [0, 0], mode=hip.MODE_FAST, wide_fast=level(n))
    for k, v in opts.items():
        g.set_option(k, v)
    g.load_segments(segs)
    r = g.estep_factored(par[0], par[1][:2], par[2])
    g.close()
    check(r, want[0], want[1], want[2], ("mix group [0, 0]", n), (par[0], par[1]), segs)


# ------------------------------------------------------------------ options
def test_mix_options(hip, golden, wide):
    """Bad values are EINVAL; the matrix diagnostic is ESTATE before any E-step and when none was built, EINVAL for a tile that is not
    class 6; without "wide_fast" the options change nothing."""
    a, e, a0 = params(200, wide)
    segs = [mix_sandwich(golden.segs_mid[3])]
    es = hip.HipEStep(200, mode=hip.MODE_FAST, wide_fast=1)
    for k, v in (("wide_mix_tiles", 2), ("wide_mix_tiles", -1), ("wide_mix_tiles", 0.5), ("wide_mix_mb", 0), ("wide_mix_mb", -1),
                 ("wide_mix_mb", 262145), ("wide_mix_mb", 1.5)):
        with pytest.raises(hip.HipError, match="(?i)invalid"):
            es.set_option(k, v)
    for k, v in (("wide_mix_mb", 1), ("wide_mix_mb", 262144), ("wide_mix_mb", 2048), ("wide_mix_tiles", 1), ("wide_hom_tiles", 1)):
        es.set_option(k, v)
    es.load_segments(segs)
    for k, v in SANDWICH.items():
        es.set_option(k, v)
    with pytest.raises(hip.HipError, match="no current wide plan"):
        es.wide_mix_matrix(5, 0)
    es.estep_factored(a, e[:2], a0)
    M, fac = es.wide_mix_matrix(5, 1)
    assert M.shape == (200, 256) and fac.shape == (16,) and (np.frexp(fac)[0] == 0.5).all()
    for t, dr in ((4, 0), (20, 0), (40, 0), (5, 2), (5, -1), (-1, 0), (10 ** 6, 0)):   # data, hom, (gap option off:) data; bad dir; bad tile
        with pytest.raises(hip.HipError, match="not a mix tile of a qualifying run"):
            es.wide_mix_matrix(t, dr)
    for t, dr in ((5, 0), (67, 1)):   # class 6, but anchored in that direction: no chain crosses it, the E-step built no such matrix
        with pytest.raises(hip.HipError, match="no chain of the plan crosses"):
            es.wide_mix_matrix(t, dr)
    es.set_option("wide_mix_tiles", 0)   # the plan is dirty; then no mix tile, and no matrix of one
    with pytest.raises(hip.HipError, match="no current wide plan"):
        es.wide_mix_matrix(5, 0)
    es.estep_factored(a, e[:2], a0)
    with pytest.raises(hip.HipError, match="built no matrix of a mix tile"):
        es.wide_mix_matrix(5, 0)
    es.close()
    out = []
    for opts in (dict(), HOM_MIX):   # without "wide_fast": the exact wide kernels, whatever the options say
        es = hip.HipEStep(200, mode=hip.MODE_FAST, **opts)
        es.load_segments(segs)
        out.append(es.estep(a, e, a0))
        es.close()
    assert bits_equal(out[0]["A"], out[1]["A"]) and bits_equal(out[0]["E"], out[1]["E"]) and out[0]["LL"] == out[1]["LL"]
