"""The option "wide_counts_ckpt" = 1: the full count matrix from the checkpoints of a "wide_ckpt" wide fast E-step (129..1024 states).
With "wide_fast", "wide_counts", "wide_ckpt" and "wide_counts_ckpt" psmc_hip_estep keeps X at every 8th position plus every tile's
last row, and the V pass of the counts (k_wc_v CKPT, psmc_amd/csrc/estep_wide_counts.hip) recomputes the seven rows between two
checkpoints into LDS with the forward sweep's own step and its stored scale factors and writes the slab's X rows beside its V rows;
the GEMM reads them through the same ranges, in the same order.  The claim is bit identity with the full-table wide-counts E-step
of the same inputs and options -- context C ("wide_ckpt" + "wide_counts_ckpt") against context F (neither) -- and F itself is
anchored to references that are not the code under test: the exact kernels on the same device and the reference's goldens
(tests/golden/estep_wide.npz), through gate() of tests/test_gpu_wide_counts.py (fast mode's own tolerances).  Data: short_segs of
tests/test_gpu_wide_fast_mw.py, 1661 bins in 17 segments of 1 .. 1000 bins.

Tilings (tests/test_gpu_wide_fast_ckpt.py TILINGS): the default, tiles of 1, 7, 8, 9, 16, 17, 37 and 64 bins with a warm-up of 5
(tiles shorter than a block of eight, tile starts and ends on every residue modulo 8, tiles that hold only position L; 37 repairs)
and chunk = 100 without chained repairs; crossed with "wide_counts_slab" 0, 64 and 300.
"""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal
from test_gpu_wide_counts import ctx, gate, ran_counts, same_bits, exact, par_of, params, transitions_ok, back_half
from test_gpu_wide_fast_mw import short_segs
from test_gpu_wide_fast_ckpt import TILINGS
from test_gpu_wide_fast_ckpt_decode import rows_bound

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [129, 192, 193, 200, 256, 257, 300, 512, 513, 768, 769, 1024]   # every S and W, below and at the padding edges
CK = dict(wide_ckpt=1, wide_counts_ckpt=1)
SLABS = [0, 64, 300]   # "wide_counts_slab": auto (one slab) | with tiles of 64 bins one tile per slab | several tiles per slab


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module")
def wide():
    from conftest import GOLD
    return dict(np.load(os.path.join(GOLD, "estep_wide.npz")))


def P(n):
    return par_of(200) if n == 200 else params(n)


def exact_key(n):
    return ("ckpt", 200) if n == 200 else ("sizes", n)   # the keys under which tests/test_gpu_wide_counts.py computes the same E-steps


def tid(o):
    return "-".join("%s%d" % kv for kv in o.items()) or "default"


def ran_ckpt(es):
    """the last E-step was a wide-counts one that kept checkpoints"""
    d = ran_counts(es)
    assert es.wide_table_info()["interval"] == 8 and d["ckpt"], (es.wide_table_info(), d)


def ran_full(es):
    d = ran_counts(es)
    assert es.wide_table_info()["interval"] == 1 and not d["ckpt"], (es.wide_table_info(), d)


def fast_like(r):
    return not r["A0"].any() and (r["chk"] == 1.0).all()


# ------------------------------------------------------------------ 1. bit identity, anchored to independent references
@pytest.mark.parametrize("n", SIZES)
def test_counts_ckpt_sizes(hip, golden, n):
    """Default tiling on short_segs: F passes the gates against the exact kernels, C has F's bits; interval 8, back half 4."""
    par = P(n)
    segs = short_segs(golden)
    f = ctx(hip, n, segs)
    r0 = f.estep(*par)
    ran_full(f)
    f.close()
    gate(r0, exact(hip, exact_key(n), n, par, segs), (par[0], par[1]), ("full table", n))
    c = ctx(hip, n, segs, **CK)
    r = c.estep(*par)
    ran_ckpt(c)
    c.close()
    assert same_bits(r, r0) and fast_like(r), n


@pytest.mark.parametrize("key", ["n200", "n149"])
def test_counts_ckpt_golden(hip, golden, wide, key):
    """The reference's goldens on segs_small[:8]: F passes the gates, C has F's bits."""
    a, e, a0 = wide[key + ".a"], wide[key + ".e"], wide[key + ".a0"]
    segs = golden.segs_small[:8]
    f = ctx(hip, a.shape[0], segs)
    r0 = f.estep(a, e, a0)
    ran_full(f)
    f.close()
    gate(r0, dict(A=wide[key + ".A"], E=wide[key + ".E"], LL=float(wide[key + ".LL"])), (a, e), ("golden", key))
    c = ctx(hip, a.shape[0], segs, **CK)
    r = c.estep(a, e, a0)
    ran_ckpt(c)
    c.close()
    assert same_bits(r, r0) and fast_like(r), key


@pytest.mark.parametrize("opts", TILINGS, ids=[tid(o) for o in TILINGS])
@pytest.mark.parametrize("n", [200, 300, 1024])
def test_counts_ckpt_tilings(hip, golden, n, opts):
    """Every tiling crossed with every slab size: C has F's bits, and two calls in a row give the same bits."""
    par = P(n)
    segs = short_segs(golden)
    for slab in SLABS:
        f = ctx(hip, n, segs, wide_counts_slab=slab, **opts)
        r0 = f.estep(*par)
        ran_full(f)
        f.close()
        transitions_ok(r0, segs, (n, opts, slab))
        c = ctx(hip, n, segs, wide_counts_slab=slab, **dict(opts, **CK))
        for it in range(2):
            r = c.estep(*par)
            ran_ckpt(c)
            assert same_bits(r, r0) and fast_like(r), (n, opts, slab, it)
        c.close()


# ------------------------------------------------------------------ 2. transitions, selections
@pytest.mark.parametrize("n", [200, 300])
def test_counts_ckpt_transitions_and_select(hip, golden, n):
    """A sums to the number of transitions; a selection with repeats has the bits of the full-table path with the same selection."""
    par = P(n)
    segs = short_segs(golden)
    sel = [16, 3, 16, 7, 7, 0, 12]
    out = []
    for opts in (dict(), CK):
        es = ctx(hip, n, segs, chunk=100, warmup=30, **opts)
        r = es.estep(*par)
        transitions_ok(r, segs, (n, opts))
        es.select(sel)
        rs = es.estep(*par)
        transitions_ok(rs, [segs[i] for i in sel], (n, opts, "selection"))
        (ran_ckpt if opts else ran_full)(es)
        out.append((r, rs))
        es.close()
    assert same_bits(out[1][0], out[0][0]) and same_bits(out[1][1], out[0][1]), n
    gate(out[0][1], exact(hip, ("ckpt select", n), n, par, segs, sel), (par[0], par[1]), ("selection, full table", n))


# ------------------------------------------------------------------ 3. alternation and memory
@pytest.mark.parametrize("n", [200, 300])
def test_counts_ckpt_alternation(hip, golden, n):
    """estep, estep_factored, estep, estep_factored on one context: interval 8 and the same bytes after every call (the table is
    not sized anew), rows within the bound of the checkpointed table, and every result has the bits of a fresh context's."""
    par = P(n)
    a, e, a0 = par
    segs = short_segs(golden)
    fresh = ctx(hip, n, segs)
    r0 = fresh.estep(a, e, a0)
    fresh.close()
    fresh = ctx(hip, n, segs)
    f0 = fresh.estep_factored(a, e[:2], a0)
    fresh.close()
    es = ctx(hip, n, segs, **CK)
    infos = []
    for it in range(2):
        r = es.estep(a, e, a0)
        ran_ckpt(es)
        infos.append(es.wide_table_info())
        assert same_bits(r, r0), (n, it)
        f = es.estep_factored(a, e[:2], a0)
        assert back_half(es) == 3
        infos.append(es.wide_table_info())
        assert bits_equal(f["sums"], f0["sums"]) and bits_equal(f["E"], f0["E"]) and f["LL"] == f0["LL"], (n, it)
    tiles = es.fast_diag()["n_chunks"]
    es.close()
    for i in infos:
        assert i["interval"] == 8 and i["bytes"] == infos[0]["bytes"] and i["rows"] == infos[0]["rows"], infos
    assert infos[0]["rows"] <= rows_bound(segs, tiles), (infos[0], tiles)


# ------------------------------------------------------------------ 4. option algebra
def test_counts_ckpt_option_algebra(hip, golden):
    """Either option alone keeps the full table and the plain run's bits; 2 and -1 are EINVAL; exact mode and 64 states accept the
    option and ignore it."""
    n = 200
    par = P(n)
    segs = short_segs(golden)
    plain = ctx(hip, n, segs)
    r0 = plain.estep(*par)
    plain.close()
    for opts in (dict(wide_counts_ckpt=1), dict(wide_ckpt=1)):
        es = ctx(hip, n, segs, **opts)
        r = es.estep(*par)
        ran_full(es)
        assert same_bits(r, r0), opts
        es.close()
    es = hip.HipEStep(n, mode=hip.MODE_FAST)
    for v in (2, -1):
        with pytest.raises(hip.HipError):
            es.set_option("wide_counts_ckpt", v)
    es.close()
    p = golden.params("n64_curve")
    for m, mode, mpar in ((200, hip.MODE_EXACT, par), (64, hip.MODE_FAST, (p["a"], p["e"], p["a0"]))):
        rs = []
        for opts in (dict(), CK):
            es = hip.HipEStep(m, mode=mode, wide_fast=1, wide_counts=1, **opts)
            es.load_segments(segs)
            rs.append(es.estep(*mpar))
            assert back_half(es) != 4 and es.wide_table_info()["interval"] == 0
            es.close()
        assert same_bits(rs[0], rs[1]) and bits_equal(rs[0]["A0"], rs[1]["A0"]), (m, mode)


# ------------------------------------------------------------------ 5. decoding
@pytest.mark.parametrize("n", [200, 300])
def test_counts_ckpt_then_decode(hip, golden, n):
    """ "wide_decode" + "wide_decode_ckpt": decode / posterior of the last segment after the checkpointed counts E-step are, bit for
    bit, those after estep_factored with the same parameters.  "wide_decode" without "wide_decode_ckpt": the counts E-step keeps
    the full table and its bits."""
    a, e, a0 = P(n)
    segs = short_segs(golden)
    seg = len(segs) - 1
    out = []
    for counts in (False, True):
        es = ctx(hip, n, segs, wide_decode=1, wide_decode_ckpt=1, **CK)
        if counts:
            es.estep(a, e, a0)
            ran_ckpt(es)
        else:
            es.estep_factored(a, e[:2], a0)
            assert es.wide_table_info()["interval"] == 8
        out.append(es.decode(seg) + es.posterior(seg))
        es.close()
    assert np.array_equal(out[0][0], out[1][0])
    for x, y in zip(out[0][1:], out[1][1:]):
        assert bits_equal(x, y)
    plain = ctx(hip, n, segs)
    r0 = plain.estep(a, e, a0)
    plain.close()
    es = ctx(hip, n, segs, wide_decode=1, **CK)
    r = es.estep(a, e, a0)
    ran_full(es)
    assert same_bits(r, r0), n
    full = es.decode(seg) + es.posterior(seg)   # ... and decodes from the full table
    es.close()
    assert np.array_equal(full[0], out[0][0])
    for x, y in zip(full[1:], out[0][1:]):
        assert bits_equal(x, y)


# ------------------------------------------------------------------ 6. batch, 7. group
@pytest.mark.parametrize("n", [200, 300])
def test_counts_ckpt_batch(hip, golden, n):
    """ "wide_batch" + "wide_counts" with and without the two options: every replicate's A, E, LL and factored sums bit-equal; the
    checkpointed run's table says interval 8."""
    from test_gpu_wide_fast_batch import rep_params, sels, N_REP
    segs = short_segs(golden)
    pars, ss = rep_params(n), sels(len(segs))
    out = []
    for opts in (dict(), CK):
        es = ctx(hip, n, segs, wide_batch=1, **opts)
        b = es.estep_batch(pars, ss, want="both")
        assert es.batch_info() == dict(groups=N_REP, replicate_contexts=0) and back_half(es) == 4
        assert es.wide_table_info()["interval"] == (8 if opts else 1)
        assert es.fast_diag()["ckpt"] == bool(opts)
        out.append(b)
        es.close()
    for r in range(N_REP):
        for k in ("A", "E", "sums"):
            assert bits_equal(out[1][k][r], out[0][k][r]), (n, r, k)
        assert out[1]["LL"][r] == out[0]["LL"][r], (n, r)
        transitions_ok(dict(A=out[1]["A"][r]), [segs[i] for i in ss[r]], ("batch", n, r))


def test_counts_ckpt_group_300(hip, golden):
    """psmc_hip_group over devices [0, 0] at 300 states: the same bits with and without the two options, and both shards' last
    E-step was a checkpointed wide-counts one."""
    par = params(300)
    segs = short_segs(golden)
    out = []
    for opts in (dict(), CK):
        g = hip.HipGroup(300, [0, 0], mode=hip.MODE_FAST, wide_fast=2, wide_counts=1, **opts)
        g.load_segments(segs)
        out.append(g.estep(*par))
        g.lib.psmc_hip_group_route.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        g.lib.psmc_hip_fast_info.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        g.lib.psmc_hip_wide_table_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        shards = set()
        for seg in range(len(segs)):
            c, loc, fi, ti = C.c_void_p(), C.c_int(0), (C.c_int * 8)(), (C.c_int64 * 4)()
            assert g.lib.psmc_hip_group_route(g.g, seg, C.byref(c), C.byref(loc)) == 0
            shards.add(c.value)
            assert g.lib.psmc_hip_fast_info(c, fi) == 0 and fi[4] == 4 and fi[5] == (1 if opts else 0), list(fi)
            assert g.lib.psmc_hip_wide_table_info(c, ti) == 0 and ti[2] == (8 if opts else 1), list(ti)
        assert len(shards) == 2
        g.close()
    assert same_bits(out[1], out[0])
    transitions_ok(out[1], segs, "group")
    gate(out[0], exact(hip, ("sizes", 300), 300, par, segs), (par[0], par[1]), "group, full table")


# ------------------------------------------------------------------ 8. ECONVERGE
def test_counts_ckpt_econverge_and_recovery(hip, golden, wide):
    """max_rounds = 1 with tiles of 37 bins, warm-up 5 and learn = 0 (tests/test_gpu_wide_counts.py): ECONVERGE; with the defaults
    restored the next call on the same context has the bits of a fresh context."""
    a, e, a0 = wide["n200.a"], wide["n200.e"], wide["n200.a0"]
    segs = golden.segs_small[:8]
    es = ctx(hip, 200, segs, chunk=37, warmup=5, learn=0, max_rounds=1, **CK)
    with pytest.raises(hip.HipError, match="converge"):
        es.estep(a, e, a0)
    for k, v in dict(chunk=0, warmup=16384, learn=1, max_rounds=4096).items():
        es.set_option(k, v)
    r = es.estep(a, e, a0)
    ran_ckpt(es)
    es.close()
    gate(r, dict(A=wide["n200.A"], E=wide["n200.E"], LL=float(wide["n200.LL"])), (a, e), "after ECONVERGE")
    fresh = ctx(hip, 200, segs, **CK)
    r2 = fresh.estep(a, e, a0)
    ran_ckpt(fresh)
    fresh.close()
    assert same_bits(r, r2)
