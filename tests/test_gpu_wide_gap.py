"""Option "wide_gap_tiles": the wide fast path (129..1024 states) across runs of missing data by a transfer-matrix chain
(psmc_amd/csrc/estep_wide_gap.hip, api_wide_fast.hip plan_wide_gaps).  Inputs are cut from golden.segs_mid with planted runs of
symbol 2 (tests/wide_gap_model.py, which also holds the numpy restatement of the plan rule).  References: the CPU oracle at 149 /
200 states, the exact wide kernels on the same device beyond; bit-for-bit claims: a fresh context given only the final inputs."""
import gzip
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal, GOLD
from test_gpu_wide_fast import check, ran_wide, tri_sums, psmc_params
from wide_gap_model import plan_rule, sandwich, mixed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANDWICH = dict(chunk=64, warmup=512)   # every data tile of input (a) is anchored: only the gap can fail


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module")
def wide():
    return dict(np.load(os.path.join(GOLD, "estep_wide.npz")))


def params(n, wide):
    if n in (149, 200):
        return wide["n%d.a" % n], wide["n%d.e" % n], wide["n%d.a0" % n]
    from test_gpu_wide_fast_mw import params as mw
    return mw(n)


def level(n):
    return 1 if n <= 256 else 2


_REF = {}


def reference(hip, oracle, key, n, par, segs):
    """factored statistics of the reference, once per key: the CPU oracle at 149 / 200 states, the exact wide kernels beyond"""
    if key not in _REF:
        a, e, a0 = par
        if n <= 200:
            o = oracle.estep(a, e, a0, segs)
        else:
            ex = hip.HipEStep(n, mode=hip.MODE_EXACT)
            ex.load_segments(segs)
            o = ex.estep(a, e, a0)
            ex.close()
        _REF[key] = (tri_sums(o["A"]), o["E"], o["LL"], o["A"])
    return _REF[key]


def run(hip, n, segs, par, steps=1, **opts):
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), **opts)
    es.load_segments(segs)
    for _ in range(steps):
        r = es.estep_factored(par[0], par[1][:2], par[2])
    d = ran_wide(es)
    return r, d, es


def same_bits(r, w):
    return bits_equal(r["sums"], w["sums"]) and bits_equal(r["E"], w["E"]) and r["LL"] == w["LL"]


def work(d):
    return "rounds %d+%d, head tiles %d+%d, mismatch %.1e / %.1e" % (d["fwd_rounds"], d["bwd_rounds"], d["fwd_tiles"], d["bwd_tiles"],
                                                                     d["warm_err_fwd"], d["warm_err_bwd"])


# ------------------------------------------------------------------ (a) anchored sandwich
@pytest.mark.parametrize("n", [149, 200, 300, 768, 1024])
def test_gap_sandwich(hip, golden, oracle, wide, n):
    """300 called bins, 4096 missing, 300 called, tiles of 64 bins and a warm-up of 512: with the option no boundary fails (the chain
    starts at an anchored tile's exact exit vector), the plan is the numpy rule's, and the statistics pass every gate; without it the
    same input needs repair rounds -- it exercises what the option removes."""
    segs = [sandwich(golden.segs_mid[3])]
    par = params(n, wide)
    want = reference(hip, oracle, ("sandwich", n), n, par, segs)
    r, d, es = run(hip, n, segs, par, wide_gap_tiles=1, **SANDWICH)
    pt = es.wide_plan_tiles()
    es.close()
    cls, glue = plan_rule(segs, 64, 512)
    assert (cls == 2).sum() == 63 and (glue & 1).sum() >= 59 and (glue & 2).sum() >= 59   # the rule does glue the run
    assert np.array_equal(pt["cls"], cls) and np.array_equal(pt["glue"], glue), (pt, cls, glue)
    print("sandwich", n, "on:", work(d))
    assert d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0, d
    check(r, want[0], want[1], want[2], ("sandwich", n, work(d)), (par[0], par[1]), segs)
    r0, d0, es0 = run(hip, n, segs, par, **SANDWICH)
    es0.close()
    print("sandwich", n, "off:", work(d0))
    assert d0["fwd_rounds"] > 0 and d0["bwd_rounds"] > 0, d0
    check(r0, want[0], want[1], want[2], ("sandwich, option off", n), (par[0], par[1]), segs)


# ------------------------------------------------------------------ (b) mixed
@pytest.mark.parametrize("opts", [dict(chunk=100, warmup=30), dict(chunk=100, warmup=30, learn=0), dict(chunk=37, warmup=5)],
                         ids=lambda o: "-".join("%s%d" % kv for kv in o.items()))
@pytest.mark.parametrize("n", [200, 300])
def test_gap_mixed(hip, golden, oracle, wide, n, opts):
    """A run of 3000 missing bins in the middle of a segment, a second run of 200 (below "wide_gap_min" = 1000), a second segment of
    data only, in tilings whose data tiles fail and are repaired around the run: right, and never ECONVERGE."""
    segs = mixed(golden.segs_mid[3], golden.segs_mid[4])
    par = params(n, wide)
    want = reference(hip, oracle, ("mixed", n), n, par, segs)
    r, d, es = run(hip, n, segs, par, wide_gap_tiles=1, wide_gap_min=1000, **opts)
    pt = es.wide_plan_tiles()
    es.close()
    cls, glue = plan_rule(segs, opts["chunk"], opts["warmup"], 1000)
    assert (cls == 2).any() and (cls == 1).any()
    assert np.array_equal(pt["cls"], cls) and np.array_equal(pt["glue"], glue)
    r0, d0, es0 = run(hip, n, segs, par, **opts)
    es0.close()
    msg = ("mixed", n, opts, "on: " + work(d), "off: " + work(d0))
    print(msg)
    check(r, want[0], want[1], want[2], msg, (par[0], par[1]), segs)
    check(r0, want[0], want[1], want[2], msg, (par[0], par[1]), segs)


# ------------------------------------------------------------------ (c) bits
@pytest.mark.parametrize("n", [200, 300])
def test_gap_bits(hip, golden, wide, n):
    """Two fresh contexts agree bit for bit; the third E-step of one context with moving parameters is a fresh context's first with
    the final ones; "wide_ckpt" gives the bits of the full table at chunk 7, 8 and 64; "wide_gap_tiles" = 0 is the default."""
    segs = mixed(golden.segs_mid[3], golden.segs_mid[4]) + [sandwich(golden.segs_mid[3])]
    rng = np.random.default_rng(11)
    pats = {200: ("100*2", 100), 300: ("150*2", 150)}[n]
    pars = [psmc_params(pats[0], pats[1], rng) for _ in range(3)]
    for chunk in (7, 8, 64):
        o = dict(chunk=chunk, warmup=256, wide_gap_tiles=1, wide_gap_min=512)
        r1, d1, e1 = run(hip, n, segs, pars[2], **o)
        assert (e1.wide_plan_tiles()["cls"] == 2).any()
        r2, d2, e2 = run(hip, n, segs, pars[2], **o)
        assert same_bits(r1, r2) and d1 == d2, chunk
        rc, dc, ec = run(hip, n, segs, pars[2], wide_ckpt=1, **o)
        assert ec.wide_table_info()["interval"] == 8
        assert same_bits(rc, r1), ("wide_ckpt", chunk)
        for e in (e1, e2, ec):
            e.close()
        if chunk == 64:
            for ck in (0, 1):
                es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), wide_ckpt=ck, **o)
                es.load_segments(segs)
                for a, e, a0 in pars:
                    r3 = es.estep_factored(a, e[:2], a0)
                es.close()
                assert same_bits(r3, r1), ("third E-step", ck)
    base = dict(chunk=64, warmup=256)
    rd, dd, ed = run(hip, n, segs, pars[2], **base)
    r0, d0, e0 = run(hip, n, segs, pars[2], wide_gap_tiles=0, wide_gap_min=512, **base)
    assert same_bits(rd, r0) and dd == d0
    assert not e0.wide_plan_tiles()["cls"].any() and not e0.wide_plan_tiles()["glue"].any()
    ed.close(); e0.close()


# ------------------------------------------------------------------ (d) consumers
@pytest.mark.parametrize("n", [200, 300])
def test_gap_decode(hip, golden, wide, n):
    """ "wide_decode" after an E-step with the option: posterior, path and scales against the exact kernels under the tolerances of
    tests/test_gpu_wide_fast_decode.py; decoding from checkpoints gives the same outputs."""
    from test_gpu_wide_fast_decode import compare
    segs = [sandwich(golden.segs_mid[3])]
    a, e, a0 = params(n, wide)
    ex = hip.HipEStep(n, mode=hip.MODE_EXACT)
    ex.load_segments(segs)
    ex.estep(a, e, a0)
    for extra in (dict(), dict(wide_ckpt=1, wide_decode_ckpt=1)):
        rf, d, fast = run(hip, n, segs, (a, e, a0), wide_decode=1, wide_gap_tiles=1, **SANDWICH, **extra)
        assert d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0, d
        compare(fast, ex, segs, n, E=rf["E"])
        fast.close()
    ex.close()


@pytest.mark.parametrize("n", [200, 1024])
def test_gap_counts(hip, golden, oracle, wide, n):
    """ "wide_counts": the full count matrix after an E-step with the option, against the exact kernels (the oracle at 200 states)
    under the gates of tests/test_gpu_wide_counts.py; from checkpoints the same bits."""
    from test_gpu_wide_counts import gate
    segs = [sandwich(golden.segs_mid[3])]
    par = params(n, wide)
    want = reference(hip, oracle, ("sandwich", n), n, par, segs)
    got = []
    for extra in (dict(), dict(wide_ckpt=1, wide_counts_ckpt=1)):
        es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), wide_counts=1, wide_gap_tiles=1, **SANDWICH, **extra)
        es.load_segments(segs)
        r = es.estep(*par)
        d = es.fast_diag()
        es.close()
        assert d["back_half"] == 4 and d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0, d
        gate(r, dict(A=want[3], E=want[1], LL=want[2]), (par[0], par[1]), ("gap counts", n, extra))
        got.append(r)
    assert bits_equal(got[0]["A"], got[1]["A"]) and bits_equal(got[0]["E"], got[1]["E"]) and got[0]["LL"] == got[1]["LL"]


@pytest.mark.parametrize("n", [200, 300])
def test_gap_batch_and_group(hip, golden, oracle, wide, n):
    """ "wide_batch": a batch of two multisets, one repeating the gapped segment, equals two single E-steps bit for bit.  A group of
    two shards on one device with the option set through psmc_hip_group_set_option passes the gates."""
    gapped = sandwich(golden.segs_mid[3])
    segs = [gapped, golden.segs_mid[4][:2500], golden.segs_small[7]]
    par = params(n, wide)
    sels = [[0, 0, 2], [1, 2, 0]]
    opts = dict(wide_gap_tiles=1, **SANDWICH)
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), wide_batch=1, **opts)
    es.load_segments(segs)
    b = es.estep_batch([par, par], sels, want="sums")
    es.close()
    for i, sel in enumerate(sels):
        one = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=level(n), **opts)
        one.load_segments(segs)
        one.select(sel)
        r = one.estep_factored(par[0], par[1][:2], par[2])
        assert (one.wide_plan_tiles()["cls"] == 2).any()
        one.close()
        assert bits_equal(b["sums"][i], r["sums"]) and bits_equal(b["E"][i], r["E"]) and b["LL"][i] == r["LL"], (n, i)
    want = reference(hip, oracle, ("group", n), n, par, segs)
    g = hip.HipGroup(n, [0, 0], mode=hip.MODE_FAST, wide_fast=level(n))
    for k, v in opts.items():
        g.set_option(k, v)
    g.load_segments(segs)
    r = g.estep_factored(par[0], par[1][:2], par[2])
    g.close()
    check(r, want[0], want[1], want[2], ("group [0, 0]", n), (par[0], par[1]), segs)


# ------------------------------------------------------------------ (e) stress fixture
def test_gap_stress(hip):
    """tests/golden/stress at 200 states, default plan, one E-step against one exact E-step: right, and fewer head tiles than without
    the option -- segment 5 is one run of missing data whose tiles speculate from a0 today and must fail; with the option they start
    from an anchored tile's exact exit vector."""
    lut = np.full(256, 2, np.uint8); lut[ord("T")] = 0; lut[ord("K")] = 1
    segs, cur = [], []
    for line in gzip.open(os.path.join(GOLD, "stress", "stress.psmcfa.gz"), "rb"):
        if line.startswith(b">"):
            if cur: segs.append(np.concatenate(cur))
            cur = []
        else:
            cur.append(lut[np.frombuffer(line.rstrip(b"\n"), dtype=np.uint8)])
    segs.append(np.concatenate(cur))
    par = psmc_params("100*2", 100, np.random.default_rng(7))
    ex = hip.HipEStep(200, mode=hip.MODE_EXACT)
    ex.load_segments(segs)
    x = ex.estep(*par)
    ex.close()
    r1, d1, e1 = run(hip, 200, segs, par, wide_gap_tiles=1)
    pt = e1.wide_plan_tiles()
    e1.close()
    r0, d0, e0 = run(hip, 200, segs, par)
    e0.close()
    cls, glue = plan_rule(segs, d1["tile_len"], 16384)
    assert np.array_equal(pt["cls"], cls) and np.array_equal(pt["glue"], glue)
    msg = ("stress", "on: " + work(d1), "off: " + work(d0), "run tiles %d" % int((cls == 2).sum()))
    print(msg)
    check(r1, tri_sums(x["A"]), x["E"], x["LL"], msg, (par[0], par[1]), segs)
    assert d1["fwd_tiles"] + d1["bwd_tiles"] < d0["fwd_tiles"] + d0["bwd_tiles"], msg


# ------------------------------------------------------------------ (f) options
def test_gap_options(hip, golden, wide):
    """Bad values are EINVAL; wide_plan_tiles and the chain diagnostics (wide_gap_chains, wide_gap_rechained, wide_gap_matrix,
    wide_tile_vectors) are ESTATE before any E-step and after an option that dirties the plan; with the option off there are no chains and
    no matrix; without "wide_fast" the option changes nothing."""
    a, e, a0 = params(200, wide)
    segs = [sandwich(golden.segs_mid[3])]
    es = hip.HipEStep(200, mode=hip.MODE_FAST, wide_fast=1)
    for k, v in (("wide_gap_tiles", 2), ("wide_gap_tiles", -1), ("wide_gap_tiles", 0.5), ("wide_gap_min", -1)):
        with pytest.raises(hip.HipError, match="(?i)invalid"):
            es.set_option(k, v)
    es.set_option("wide_gap_tiles", 1); es.set_option("wide_gap_min", 0); es.set_option("wide_gap_min", 4096)
    es.load_segments(segs)
    for k, v in dict(wide_gap_min=2048, **SANDWICH).items():   # the tiling of test_gap_sandwich: one chain per direction
        es.set_option(k, v)
    probes = (es.wide_plan_tiles, es.wide_gap_chains, es.wide_gap_rechained, es.wide_gap_matrix, lambda: es.wide_tile_vectors(0), lambda: es.wide_tile_vectors(1))
    for f in probes:
        with pytest.raises(hip.HipError, match="no current wide plan"):
            f()
    es.estep_factored(a, e[:2], a0)
    nt = ran_wide(es)["n_chunks"]
    assert len(es.wide_plan_tiles()["cls"]) == nt
    ch = es.wide_gap_chains()
    assert len(ch) == 2 and len(ch[0]) == 1 and len(ch[1]) == 1 and es.wide_gap_rechained() == [0, 0]
    assert es.wide_gap_matrix().shape == (200, 256) and es.wide_tile_vectors(0).shape == (nt, 256) and es.wide_tile_vectors(1).shape == (nt, 256)
    es.set_option("wide_gap_min", 100)   # the plan is dirty again
    for f in probes:
        with pytest.raises(hip.HipError, match="no current wide plan"):
            f()
    es.set_option("wide_gap_tiles", 0)   # off: a plan without chains, and an E-step that builds no matrix
    es.estep_factored(a, e[:2], a0)
    assert es.wide_gap_chains() == [[], []] and es.wide_gap_rechained() == [0, 0] and es.wide_tile_vectors(0).shape == (nt, 256)
    with pytest.raises(hip.HipError, match="built no transfer matrix"):
        es.wide_gap_matrix()
    es.close()
    out = []
    for opts in (dict(), dict(wide_gap_tiles=1)):   # without "wide_fast": the exact wide kernels, whatever the option says
        es = hip.HipEStep(200, mode=hip.MODE_FAST, **opts)
        es.load_segments(segs)
        out.append(es.estep(a, e, a0))
        es.close()
    assert bits_equal(out[0]["A"], out[1]["A"]) and bits_equal(out[0]["E"], out[1]["E"]) and out[0]["LL"] == out[1]["LL"]
