"""The option "wide_ckpt" = 1: the wide fast E-step (129..1024 states, "wide_fast") keeps its forward table X at every 8th position
only, plus every tile's last row, and the accumulate sweep recomputes the seven rows between two checkpoints into LDS with the
forward sweep's own step (fstep of psmc_amd/csrc/wide_prims.h) and its stored scale factors.  The claim
is bit identity with the full-table E-step -- statistics, LL and the repair counters -- so everything the suite establishes about
the wide path's accuracy carries over; the exact kernels are compared directly as well, at the library's own tolerances (check()
of tests/test_gpu_wide_fast.py).  Data: short_segs of tests/test_gpu_wide_fast_mw.py, 1661 bins in segments of 1 .. 1000 bins.

Tile lengths: 1, 7, 8, 9, 16, 17, 37, 64 (both sides of the block of eight positions, tiles shorter than a block, tile starts on
every residue modulo 8 and modulo 4), the default tiling and chunk = 100 without chained repairs.  Sizes: 150 (S = 192, three
states per lane), 200 (256), 257 and 300 (512, two waves), 769 (1024) and 1024 (four waves; 56 KB of staged rows).

Observed on the MI355X: every bit comparison holds at every size and tiling; against the exact kernels (-s prints each figure)
cell <= 6.7e-14 (DG, 1024 states), L1 <= 1.3e-14, QA / QE <= 2.4e-15, LL <= 4.7e-16 relative -- the full-table path's figures
(tests/test_gpu_wide_fast_mw.py).  The file takes 8 s.
"""
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal
from test_gpu_wide_fast import check, ran_wide, tri_sums, psmc_params
from test_gpu_wide_fast_mw import SIZES, params, short_segs, exact_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ONE_WAVE = {150: ("75*2", 75), 200: ("100*2", 100)}     # sizes of the one-wave path (SIZES holds the multi-wave ones)
BIT_SIZES = [150, 200, 257, 300, 769, 1024]
TILINGS = [dict()] + [dict(chunk=c, warmup=5) for c in (1, 7, 8, 9, 16, 17, 37, 64)] + [dict(chunk=100, warmup=30, learn=0)]
_EXACT = {}


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


def par_of(n):
    if n in ONE_WAVE:
        pat, m = ONE_WAVE[n]
        return psmc_params(pat, m, np.random.default_rng(2000 + n))
    return params(n)


def width(n):
    return 64 * ((n + 63) // 64) if n <= 256 else 256 * ((n + 255) // 256)


def ctx(hip, n, segs, **opts):
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=2, **opts)
    es.load_segments(segs)
    return es


def same_bits(r, w):
    return bits_equal(r["sums"], w["sums"]) and bits_equal(r["E"], w["E"]) and r["LL"] == w["LL"]


def exact_of(hip, golden, n):
    """the exact kernels' statistics on short_segs, once per size (the multi-wave sizes share tests/test_gpu_wide_fast_mw.py's)"""
    if n in SIZES:
        return exact_ref(hip, golden, n)
    if n not in _EXACT:
        ex = hip.HipEStep(n, mode=hip.MODE_EXACT)
        ex.load_segments(short_segs(golden))
        x = ex.estep(*par_of(n))
        ex.close()
        _EXACT[n] = (tri_sums(x["A"]), x["E"], x["LL"])
    return _EXACT[n]


REPAIR_KEYS = ("fwd_rounds", "bwd_rounds", "fwd_tiles", "bwd_tiles")


# ------------------------------------------------------------------ 1. bit identity
@pytest.mark.parametrize("n", BIT_SIZES)
def test_ckpt_bits(hip, golden, n):
    """Every tiling: a "wide_ckpt" = 1 context returns, three E-steps in a row, the bits of a fresh full-table context with the same
    options; fast_info says checkpointed, back half 3; the repair counters are the full-table run's; chunk = 37 does repair."""
    a, e, a0 = par_of(n)
    segs = short_segs(golden)
    for opts in TILINGS:
        full = ctx(hip, n, segs, wide_ckpt=0, **opts)
        want = full.estep_factored(a, e[:2], a0)
        dw = ran_wide(full)
        assert not dw["ckpt"], dw
        assert full.wide_table_info()["interval"] == 1
        full.close()
        es = ctx(hip, n, segs, wide_ckpt=1, **opts)
        for it in range(3):
            r = es.estep_factored(a, e[:2], a0)
            d = ran_wide(es)
            assert d["ckpt"] and d["back_half"] == 3, (n, opts, d)
            assert same_bits(r, want), (n, opts, it, np.abs(r["sums"] - want["sums"]).max(), r["LL"], want["LL"])
            assert [d[k] for k in REPAIR_KEYS] == [dw[k] for k in REPAIR_KEYS], (n, opts, it, d, dw)
        if opts.get("chunk") == 37:
            assert d["fwd_rounds"] + d["bwd_rounds"] > 0, d
        es.close()


# ------------------------------------------------------------------ 2. against the exact kernels directly
@pytest.mark.parametrize("n", [150, 300, 1024])
def test_ckpt_vs_exact(hip, golden, n):
    a, e, a0 = par_of(n)
    segs = short_segs(golden)
    sums, E, LL = exact_of(hip, golden, n)
    for opts in (dict(), dict(chunk=37, warmup=5)):
        es = ctx(hip, n, segs, wide_ckpt=1, **opts)
        r = es.estep_factored(a, e[:2], a0)
        check(r, sums, E, LL, ("ckpt", n, opts), (a, e), segs)
        assert ran_wide(es)["ckpt"]
        es.close()


# ------------------------------------------------------------------ 3. multiset
def test_ckpt_multiset_300(hip, golden):
    a, e, a0 = params(300)
    segs = golden.segs_small[:10] + [golden.segs_mid[5]]
    sel = [8, 3, 8, 9, 9, 10, 0, 7, 10, 10]
    rs = []
    for ck in (0, 1):
        es = ctx(hip, 300, segs, chunk=300, warmup=64, wide_ckpt=ck)
        es.select(sel)
        rs.append(es.estep_factored(a, e[:2], a0))
        assert ran_wide(es)["ckpt"] == bool(ck)
        es.close()
    assert same_bits(rs[1], rs[0])


# ------------------------------------------------------------------ 4. anchored tiles
@pytest.mark.parametrize("chunk", [37, 38, 39, 41])
def test_ckpt_anchored_tile_below_segment_end(hip, golden, chunk):
    """the segments of test_mw_anchored_tile_below_segment_end (1003 .. 1006 bins) at 512 states"""
    a, e, a0 = params(512)
    segs = [golden.segs_mid[0][:L] for L in (1003, 1004, 1005, 1006)] + [golden.segs_mid[1][:2000]]
    rs = []
    for ck in (0, 1):
        es = ctx(hip, 512, segs, chunk=chunk, warmup=5, wide_ckpt=ck)
        rs.append(es.estep_factored(a, e[:2], a0))
        assert ran_wide(es)["ckpt"] == bool(ck)
        es.close()
    assert same_bits(rs[1], rs[0])


# ------------------------------------------------------------------ 5. memory
@pytest.mark.parametrize("n", [200, 300])
def test_ckpt_memory(hip, golden, n):
    """psmc_hip_wide_table_info: zeros before the path ran; with checkpoints interval 8 and rows <= bins / 8 + 2 tiles + 64, without
    them interval 1 and rows >= bins (bins: the segment lengths padded to 64, as the library lays them out); 1 -> 0 -> 1 on one
    context: every E-step has the bits of the first and the info follows."""
    a, e, a0 = par_of(n)
    segs = short_segs(golden)
    bins = sum(64 * ((len(s) + 63) // 64) for s in segs)
    S = width(n)
    es = ctx(hip, n, segs, wide_ckpt=1)
    assert es.wide_table_info() == dict(rows=0, width=0, interval=0, bytes=0)
    first = es.estep_factored(a, e[:2], a0)
    tiles = ran_wide(es)["n_chunks"]

    def ckpt_info():
        t = es.wide_table_info()
        assert t["interval"] == 8 and t["width"] == S and t["bytes"] == t["rows"] * S * 8, t
        assert 0 < t["rows"] <= bins // 8 + 2 * tiles + 64, (t, bins, tiles)
    ckpt_info()
    es.set_option("wide_ckpt", 0)
    r = es.estep_factored(a, e[:2], a0)
    assert same_bits(r, first) and not ran_wide(es)["ckpt"]
    t = es.wide_table_info()
    assert t["interval"] == 1 and t["width"] == S and t["rows"] >= bins and t["bytes"] == t["rows"] * S * 8, (t, bins)
    es.set_option("wide_ckpt", 1)
    r = es.estep_factored(a, e[:2], a0)
    assert same_bits(r, first) and ran_wide(es)["ckpt"]
    ckpt_info()
    es.close()


# ------------------------------------------------------------------ 6. decoding
@pytest.mark.parametrize("n", [200, 300])
def test_ckpt_decoding(hip, golden, n):
    """ "wide_decode" = 1 wins: the E-step keeps the full table and the decoding of the last segment has the bits of a context
    without "wide_ckpt".  A checkpointed E-step followed by "wide_decode" = 1 and a decoding call: ESTATE naming the checkpoints;
    after the next E-step (full, now) decoding works."""
    a, e, a0 = par_of(n)
    segs = short_segs(golden)
    seg = len(segs) - 1
    outs = []
    for ck in (0, 1):
        es = ctx(hip, n, segs, wide_decode=1, wide_ckpt=ck)
        r = es.estep_factored(a, e[:2], a0)
        assert not ran_wide(es)["ckpt"] and es.wide_table_info()["interval"] == 1
        outs.append((r, es.decode(seg), es.posterior(seg), es.scales(seg)))
        es.close()
    (r0, d0, p0, s0), (r1, d1, p1, s1) = outs
    assert same_bits(r1, r0)
    assert np.array_equal(d1[0], d0[0]) and bits_equal(d1[1], d0[1])
    assert bits_equal(p1[0], p0[0]) and bits_equal(p1[1], p0[1]) and bits_equal(np.asarray(s1), np.asarray(s0))
    es = ctx(hip, n, segs, wide_ckpt=1)
    r = es.estep_factored(a, e[:2], a0)
    assert same_bits(r, r0) and es.wide_table_info()["interval"] == 8
    es.set_option("wide_decode", 1)
    for call in (lambda: es.decode(seg), lambda: es.posterior(seg), lambda: es.scales(seg)):
        with pytest.raises(hip.HipError, match="checkpoint") as ei:
            call()
        assert "call order violated" in str(ei.value), ei.value   # PSMC_HIP_ESTATE
    es.estep_factored(a, e[:2], a0)
    assert es.wide_table_info()["interval"] == 1
    d2 = es.decode(seg)
    assert np.array_equal(d2[0], d0[0]) and bits_equal(d2[1], d0[1])
    es.close()


# ------------------------------------------------------------------ 7. batch
@pytest.mark.parametrize("n", [200, 300])
def test_ckpt_batch(hip, golden, n):
    segs = short_segs(golden)
    pat, m = ONE_WAVE[n] if n in ONE_WAVE else SIZES[n]
    pars = [psmc_params(pat, m, np.random.default_rng(7000 + 10 * n + r)) for r in range(3)]
    sels = [list(range(len(segs))), [7, 7, 3], [16, 16, 16, 2, 5, 5]]
    bs = []
    for ck in (0, 1):
        es = ctx(hip, n, segs, wide_batch=1, wide_ckpt=ck)
        bs.append(es.estep_batch(pars, sels, want="sums"))
        assert ran_wide(es)["ckpt"] == bool(ck)
        es.close()
    for r in range(3):
        assert bits_equal(bs[1]["sums"][r], bs[0]["sums"][r]) and bits_equal(bs[1]["E"][r], bs[0]["E"][r]) and bs[1]["LL"][r] == bs[0]["LL"][r], r


# ------------------------------------------------------------------ 8. group
def test_ckpt_group_300(hip, golden):
    a, e, a0 = params(300)
    segs = short_segs(golden)
    rs = []
    for ck in (0, 1):
        g = hip.HipGroup(300, [0, 0], mode=hip.MODE_FAST, wide_fast=2, wide_ckpt=ck)
        g.load_segments(segs)
        rs.append(g.estep_factored(a, e[:2], a0))
        g.close()
    assert same_bits(rs[1], rs[0])


# ------------------------------------------------------------------ 9. option edges
def test_ckpt_option_edges(hip, golden):
    """2 and -1: EINVAL.  An exact-mode context and a 64-state fast context accept the option, and estep returns the bits it
    returned without it."""
    segs = short_segs(golden)
    es = hip.HipEStep(300, mode=hip.MODE_FAST, wide_fast=2)
    for v in (2, -1):
        with pytest.raises(hip.HipError, match="set_option"):
            es.set_option("wide_ckpt", v)
    es.close()
    g = golden.params("n64_curve")
    a, e, a0 = g["a"], g["e"], g["a0"]
    for mode in (hip.MODE_EXACT, hip.MODE_FAST):
        rs = []
        for ck in (0, 1):
            es = hip.HipEStep(64, mode=mode)
            es.set_option("wide_ckpt", ck)
            es.load_segments(segs)
            rs.append(es.estep(a, e, a0))
            assert es.wide_table_info() == dict(rows=0, width=0, interval=0, bytes=0)
            es.close()
        assert bits_equal(rs[1]["A"], rs[0]["A"]) and bits_equal(rs[1]["E"], rs[0]["E"]) and rs[1]["LL"] == rs[0]["LL"], mode


# ------------------------------------------------------------------ 10. ECONVERGE
def test_ckpt_econverge_and_recovery(hip, golden):
    a, e, a0 = params(300)
    segs = short_segs(golden)
    sums, E, LL = exact_ref(hip, golden, 300)
    es = ctx(hip, 300, segs, chunk=37, warmup=5, learn=0, max_rounds=1, wide_ckpt=1)
    with pytest.raises(hip.HipError, match="converge"):
        es.estep_factored(a, e[:2], a0)
    for k, v in dict(chunk=0, warmup=16384, learn=1, max_rounds=4096).items():
        es.set_option(k, v)
    r = es.estep_factored(a, e[:2], a0)
    check(r, sums, E, LL, "ckpt after ECONVERGE", (a, e), segs)
    assert ran_wide(es)["ckpt"]
    es.close()
    fresh = ctx(hip, 300, segs, wide_ckpt=1)
    r2 = fresh.estep_factored(a, e[:2], a0)
    assert same_bits(r, r2)
    fresh.close()
