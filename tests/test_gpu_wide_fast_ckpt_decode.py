"""The option "wide_decode_ckpt" = 1: decoding from the checkpoints of a "wide_ckpt" wide fast E-step (129..1024 states).  Such an
E-step keeps X at every 8th position plus every tile's last row even while "wide_decode" is on, and psmc_hip_decode / _posterior /
_post_counts / _scales recompute the seven rows between two checkpoints into LDS with the forward sweep's own step and its stored
scale factors (the CKPT variants of k_wp_dec and of the scales kernels: psmc_amd/csrc/estep_wide_post.hip).  The recomputed rows are the forward sweep's bits (tests/test_gpu_wide_fast_ckpt.py), so the claim is bit
identity with decoding from the full table: context C ("wide_ckpt" + "wide_decode_ckpt") against context F (neither), same tiling.
The exact kernels are compared directly as well, with compare() of tests/test_gpu_wide_fast_decode.py (the library's tolerances
for wide decoding, include/psmc_hip.h).  Data: short_segs of tests/test_gpu_wide_fast_mw.py, 1661 bins in 17 segments of 1 .. 1000
bins (L = 1, 2, 3 among them).

Tile lengths at 150 (S = 192) and 300 states (two waves): 1, 7, 8, 9, 16, 17, 37, 64 with warmup = 5 (both sides of a block of
eight, tiles shorter than a block, tile starts on every residue modulo 8 and modulo 4; 37 repairs), the default tiling, and
chunk = 100 without chained repairs.  200, 257, 769 and 1024 states: the default tiling and chunk = 37.

Observed on the MI355X: every bit comparison holds at every size and tiling; the file's 35 cases take 2.4 s.
"""
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal
from test_gpu_wide_fast import ran_wide
from test_gpu_wide_fast_mw import params, short_segs
from test_gpu_wide_fast_ckpt import par_of
from test_gpu_wide_fast_decode import compare
from test_gpu_wide_fast_mw_decode import exact_ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CNT = 5   # two sweeps of four count columns, the second partial

SMALL_TILES = [dict(chunk=c, warmup=5) for c in (1, 7, 8, 9, 16, 17, 37, 64)]
ALL_TILINGS = SMALL_TILES + [dict(), dict(chunk=100, warmup=30, learn=0)]
BIT_CASES = [(n, o) for n in (150, 300) for o in ALL_TILINGS] + [(n, o) for n in (200, 257, 769, 1024) for o in (dict(), dict(chunk=37, warmup=5))]
CK = dict(wide_ckpt=1, wide_decode_ckpt=1)
_F = {}


def case_id(n, o):
    return "%d-%s" % (n, "-".join("%s%d" % kv for kv in o.items()) or "default")


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


def ctx(hip, n, segs, **opts):
    opts.setdefault("wide_decode", 1)
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=2, **opts)
    es.load_segments(segs)
    return es


def same_stats(r, w):
    return bits_equal(r["sums"], w["sums"]) and bits_equal(r["E"], w["E"]) and r["LL"] == w["LL"]


def outputs(es, segs, n, ids=None):
    """every decoding output of every segment: decode, the three kinds of posterior call, post_counts with N_CNT columns (running
    totals; l = L - 2 on the even segments, the 1000-bin one among them), scales -- a flat list of (name, array)"""
    rng = np.random.default_rng(3)
    out, cnt = [], np.zeros((n, N_CNT))
    for seg in (range(len(segs)) if ids is None else ids):
        L = len(segs[seg])
        path, maxp = es.decode(seg)
        post, rec = es.posterior(seg)
        post1, _ = es.posterior(seg, want_recomb=False)
        _, rec1 = es.posterior(seg, want_post=False)
        l = L if seg % 2 else max(0, L - 2)
        es.post_counts(seg, rng.integers(0, 50, size=(l, N_CNT), dtype=np.int32), cnt)
        here = [("path", path), ("maxp", maxp), ("post+", post), ("rec+", rec), ("post", post1), ("rec", rec1),
                ("counts", cnt.copy()), ("scales", np.asarray(es.scales(seg)))]
        out += [("%s of segment %d" % (k, seg), v) for k, v in here]
    return out


def first_difference(x, y):
    """None when the two lists of outputs() have the same bits, else the name of the first output that differs"""
    if len(x) != len(y):
        return "lengths %d %d" % (len(x), len(y))
    for (k, u), (_, v) in zip(x, y):
        if not (np.array_equal(u, v) if u.dtype.kind == "i" else bits_equal(u, v)):
            return k
    return None


def full_default(hip, golden, n):
    """context F at the default tiling: the statistics and outputs() of decoding from the full table, once per size"""
    if n not in _F:
        a, e, a0 = par_of(n)
        segs = short_segs(golden)
        es = ctx(hip, n, segs)
        r = es.estep_factored(a, e[:2], a0)
        assert es.wide_table_info()["interval"] == 1
        _F[n] = (r, outputs(es, segs, n))
        es.close()
    return _F[n]


def rows_bound(segs, tiles):
    return sum(64 * ((len(s) + 63) // 64) for s in segs) // 8 + 2 * tiles + 64   # the bound of test_ckpt_memory


# ------------------------------------------------------------------ 1. bit identity
@pytest.mark.parametrize("n,opts", BIT_CASES, ids=[case_id(n, o) for n, o in BIT_CASES])
def test_ckpt_decode_bits(hip, golden, n, opts):
    a, e, a0 = par_of(n)
    segs = short_segs(golden)
    if opts:
        full = ctx(hip, n, segs, **opts)
        want_r = full.estep_factored(a, e[:2], a0)
        assert not ran_wide(full)["ckpt"] and full.wide_table_info()["interval"] == 1
        want = outputs(full, segs, n)
        full.close()
    else:
        want_r, want = full_default(hip, golden, n)
    es = ctx(hip, n, segs, **CK, **opts)
    r = es.estep_factored(a, e[:2], a0)
    d = ran_wide(es)
    t = es.wide_table_info()
    assert d["ckpt"] and t["interval"] == 8 and 0 < t["rows"] <= rows_bound(segs, d["n_chunks"]), (d, t)
    assert same_stats(r, want_r)
    if opts.get("chunk") == 37:
        assert d["fwd_rounds"] + d["bwd_rounds"] > 0, d
    assert first_difference(outputs(es, segs, n), want) is None
    es.close()


# ------------------------------------------------------------------ 2. against the exact kernels
@pytest.mark.parametrize("n", [200, 1024])
def test_ckpt_decode_vs_exact(hip, golden, n):
    a, e, a0 = par_of(n)
    segs = short_segs(golden)
    exact = exact_ctx(hip, n, segs, (a, e, a0))
    for opts in (dict(), dict(chunk=37, warmup=5)):
        es = ctx(hip, n, segs, **CK, **opts)
        r = es.estep_factored(a, e[:2], a0)
        assert ran_wide(es)["ckpt"] and es.wide_table_info()["interval"] == 8
        compare(es, exact, segs, n, E=r["E"])
        es.close()
    exact.close()


# ------------------------------------------------------------------ 3. late switch
@pytest.mark.parametrize("n", [200, 300])
def test_ckpt_decode_late_switch(hip, golden, n):
    a, e, a0 = par_of(n)
    segs = short_segs(golden)
    want_r, want = full_default(hip, golden, n)
    es = ctx(hip, n, segs, wide_decode=0, **CK)
    r = es.estep_factored(a, e[:2], a0)
    assert same_stats(r, want_r) and es.wide_table_info()["interval"] == 8
    es.set_option("wide_decode", 1)                 # switched on only now: nothing has to be re-run
    assert first_difference(outputs(es, segs, n), want) is None
    es.set_option("wide_decode_ckpt", 0)            # read at decode time too
    seg = len(segs) - 1
    for call in (lambda: es.decode(seg), lambda: es.posterior(seg), lambda: es.scales(seg),
                 lambda: es.post_counts(seg, np.ones((len(segs[seg]), 1), np.int32), np.zeros((n, 1)))):
        with pytest.raises(hip.HipError, match="checkpoint") as ei:
            call()
        assert "call order violated" in str(ei.value), ei.value   # PSMC_HIP_ESTATE
    r = es.estep_factored(a, e[:2], a0)             # "wide_decode" wins again: the full table
    assert same_stats(r, want_r) and es.wide_table_info()["interval"] == 1 and not ran_wide(es)["ckpt"]
    assert first_difference(outputs(es, segs, n), want) is None
    es.close()


# ------------------------------------------------------------------ 4. option edges
def test_ckpt_decode_option_edges(hip, golden):
    segs = short_segs(golden)
    es = hip.HipEStep(300, mode=hip.MODE_FAST, wide_fast=2)
    for v in (2, -1):
        with pytest.raises(hip.HipError, match="set_option"):
            es.set_option("wide_decode_ckpt", v)
    es.close()
    g = golden.params("n64_curve")
    a, e, a0 = g["a"], g["e"], g["a0"]
    for mode in (hip.MODE_EXACT, hip.MODE_FAST):    # accepted, no effect
        rs = []
        for on in (0, 1):
            es = hip.HipEStep(64, mode=mode)
            es.set_option("wide_decode_ckpt", on)
            es.load_segments(segs)
            r = es.estep(a, e, a0)
            assert es.wide_table_info() == dict(rows=0, width=0, interval=0, bytes=0)
            rs.append([r["A"], r["E"], np.float64(r["LL"])] + (list(es.decode(16)) + list(es.posterior(16)) if mode == hip.MODE_EXACT else []))
            es.close()
        assert all(np.array_equal(u, v) if np.asarray(u).dtype.kind == "i" else bits_equal(np.asarray(u), np.asarray(v)) for u, v in zip(*rs)), mode
    # without "wide_ckpt": the full table and its bits
    a, e, a0 = par_of(300)
    want_r, want = full_default(hip, golden, 300)
    es = ctx(hip, 300, segs, wide_decode_ckpt=1)
    r = es.estep_factored(a, e[:2], a0)
    assert same_stats(r, want_r) and es.wide_table_info()["interval"] == 1 and not ran_wide(es)["ckpt"]
    assert first_difference(outputs(es, segs, 300), want) is None
    es.close()


# ------------------------------------------------------------------ 5. state rules in checkpoint mode
def test_ckpt_decode_state_rules(hip, golden):
    a, e, a0 = params(300)
    segs = short_segs(golden)
    want_r, want = full_default(hip, golden, 300)
    calls = [lambda c: c.decode(5), lambda c: c.posterior(5), lambda c: c.scales(5),
             lambda c: c.post_counts(5, np.ones((len(segs[5]), 1), np.int32), np.zeros((c.n, 1)))]

    def refused(es, match="call order violated"):
        for f in calls:
            with pytest.raises(hip.HipError, match=match):
                f(es)

    def works(es):
        assert es.wide_table_info()["interval"] == 8 and ran_wide(es)["ckpt"]
        for f in calls:
            f(es)

    es = ctx(hip, 300, segs, wide_batch=1, **CK)
    refused(es)                                     # before any E-step
    es.estep_factored(a, e[:2], a0)
    works(es)
    assert first_difference(outputs(es, segs, 300), want) is None
    es.estep_batch([(a, e, a0)] * 2, [[0, 1], [2, 3]], want="sums")   # a wide fast batch
    assert ran_wide(es)["ckpt"]
    refused(es)
    es.estep_factored(a, e[:2], a0)
    works(es)
    es.select([5, 6, 7])                            # the selection changed since
    refused(es, "call order violated.*selection")
    es.estep_factored(a, e[:2], a0)
    works(es)
    with pytest.raises(hip.HipError, match="call order violated.*selection"):
        es.decode(0)                                # outside the selection
    es.close()

    # an E-step forced to ECONVERGE (the recipe of test_ckpt_econverge_and_recovery), then a good one
    es = ctx(hip, 300, segs, chunk=37, warmup=5, learn=0, max_rounds=1, **CK)
    with pytest.raises(hip.HipError, match="converge"):
        es.estep_factored(a, e[:2], a0)
    refused(es, "call order violated.*returned an error")
    for k, v in dict(chunk=0, warmup=16384, learn=1, max_rounds=4096).items():
        es.set_option(k, v)
    r = es.estep_factored(a, e[:2], a0)
    works(es)
    assert same_stats(r, want_r) and first_difference(outputs(es, segs, 300), want) is None
    es.close()


# ------------------------------------------------------------------ 6. multiset selection
def test_ckpt_decode_multiset_300(hip, golden):
    a, e, a0 = params(300)
    segs = golden.segs_small[:10] + [golden.segs_mid[5]]
    sel = [8, 3, 8, 9, 9, 10, 0, 7, 10, 10]
    outs = []
    for opts in (dict(), CK):
        es = ctx(hip, 300, segs, chunk=300, warmup=64, **opts)
        es.select(sel)
        r = es.estep_factored(a, e[:2], a0)
        assert ran_wide(es)["ckpt"] == bool(opts)
        outs.append((r, outputs(es, segs, 300, ids=sorted(set(sel)))))
        es.close()
    assert same_stats(outs[1][0], outs[0][0]) and first_difference(outs[1][1], outs[0][1]) is None
