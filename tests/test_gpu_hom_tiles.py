"""Fast mode, "hom_tiles": runs of homozygosity found at plan time (include/psmc_hip.h; the rule: psmc_amd/csrc/psmc_hip_ctx.h; the
finding and its evidence: DESIGN.md section 9 (5)).

The classifier kernel at its edges against a numpy restatement of the rule, the options, and the finding itself: a 45 k-bin run of
homozygous bins at 256-bin tiles costs a context without the option hundreds of repair rounds in its first E-step; with it the plan
knows the run before the first sweep.  Reference statistics: the CPU oracle (tests/orc.py), computed once per (input, parameter set)
and shared by the tests of this module."""
import json
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal, GOLD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "psmc_amd", "host")
RUN = (40000, 85000)   # the planted run of the long segment, 0-based [lo, hi)


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


def _traj(n, rounds):
    from psmc_amd import hostlib
    tj = json.load(open(os.path.join(GOLD, "traj_n%d.json" % n)))
    return [hostlib.hmm_params(tj["pattern"], tj["rounds"][r]["params"]) for r in rounds]


def _p(t):
    return dict(a=t[0], e=t[1], a0=t[2])


class Inputs:
    """The inputs of tests 2-4 and their oracle statistics, each computed on first use and kept."""

    def __init__(self, golden, oracle):
        from psmc_amd import sim
        self.oracle = oracle
        p = golden.params("n64_curve")
        self.curve = dict(a=p["a"], e=p["e"], a0=p["a0"])
        self.traj = dict(zip((1, 2, 0), (_p(t) for t in _traj(64, (1, 2, 0)))))
        rng = np.random.default_rng(20234)
        short = sim.simulate_segment(p["a"], p["e"], p["a0"], 2761, rng)
        raw = sim.simulate_segment(p["a"], p["e"], p["a0"], 120000, rng)
        run = slice(*RUN)
        long0 = raw.copy(); long0[run] = 0
        mix = raw.copy(); mix[run][mix[run] != 2] = 0     # keeps the simulator's missing stretches: het-free tiles of both kinds
        assert int((mix[run] == 2).sum()) > 0
        self.segs = dict(main=[short, long0], mix=[short, mix])
        self.p128 = dict(zip((1, 2), (_p(t) for t in _traj(128, (1, 2)))))
        q = self.p128[1]
        s128 = sim.simulate_segment(q["a"], q["e"], q["a0"], 60000, np.random.default_rng(40160))
        s128[15000:45000] = 0
        self.segs["n128"] = [s128]
        self._orc = {}

    def params(self, key):
        return self.curve if key == "curve" else (self.p128[key[1]] if isinstance(key, tuple) else self.traj[key])

    def ref(self, name, key):
        """oracle statistics of input `name` at parameter set `key`, per segment as well"""
        if (name, key) not in self._orc:
            p = self.params(key)
            self._orc[(name, key)] = self.oracle.estep(p["a"], p["e"], p["a0"], self.segs[name], per_seg=True)
        return self._orc[(name, key)]


@pytest.fixture(scope="module")
def inputs(golden, oracle):
    return Inputs(golden, oracle)


# ------------------------------------------------------------------ the rule, restated
def rule(segs, T, W, hom_min, gap_tiles=True):
    """(cls, glue) per tile, segments in order: what psmc_hip_plan_tiles must show for tiles of T bins under warm-ups of W bins -- cls 0,
    1 = gap tile, 2 = hom tile outside a qualifying run, 3 = hom tile of a qualifying run; glue = the bits the two plan rules demand."""
    need = hom_min if hom_min > 0 else W // 4
    cls_all, glue_all = [], []
    for s in segs:
        L = len(s)
        nt = (L + T - 1) // T
        gap = np.zeros(nt, bool); hom = np.zeros(nt, bool)
        for k in range(1, nt - 1):                      # neither the first nor the last tile; those in between are full
            t = s[k * T:(k + 1) * T]
            if (t == 2).all(): gap[k] = gap_tiles
            elif not (t == 1).any(): hom[k] = True
        inq = np.zeros(nt, bool)
        k = 0
        while k < nt:
            if not (gap[k] or hom[k]): k += 1; continue
            e = k
            while e < nt and (gap[e] or hom[e]): e += 1
            n_hom = int(hom[k:e].sum())
            if n_hom >= 1 and n_hom * T >= need: inq[k:e] = True
            k = e
        pos = np.repeat(inq, T)[:L]                     # per position (0-based): inside a tile of a qualifying run
        cls = np.where(gap, 1, np.where(hom & inq, 3, np.where(hom, 2, 0)))
        glue = np.zeros(nt, int)
        for k in range(nt):
            lo, hi = k * T, min(L, (k + 1) * T)          # 0-based [lo, hi)
            if k > 0 and pos[max(0, lo - W):lo].any(): glue[k] |= 1
            if k + 1 < nt and pos[hi:min(L, hi + W)].any(): glue[k] |= 2
            if gap[k]: glue[k] |= 3                      # (a gap tile is never first or last)
            if k > 0 and gap[k - 1]: glue[k] |= 1
            if k + 1 < nt and gap[k + 1]: glue[k] |= 2
        cls_all.append(cls); glue_all.append(glue)
    return np.concatenate(cls_all), np.concatenate(glue_all)


def planted(golden, T):
    """~3000 simulated bins with het-free runs at every edge of a T-bin tiling (a het bin planted beside each, so that the edge is where
    it is meant to be), and a second segment shorter than a tile."""
    from psmc_amd import sim
    p = golden.params("n64_curve")
    s = sim.simulate_segment(p["a"], p["e"], p["a0"], 3005, np.random.default_rng(5))
    nt = len(s) // T                                        # full tiles; the ragged one behind them is the segment's last
    assert nt >= 60 and len(s) % T
    def run(lo, hi, v=0):
        s[lo:hi] = v
        if lo > 0: s[lo - 1] = 1
        if hi < len(s): s[hi] = 1
    run(0, 2 * T)                                           # the first two tiles of the segment
    run(5 * T, 9 * T - 1)                                   # ends one bin before a tile's end
    run(12 * T + 1, 16 * T)                                 # starts one bin after a tile's start
    run(20 * T, 25 * T)                                     # exactly five tiles
    run(29 * T, 34 * T); s[31 * T + 3] = 2                  # a single missing bin inside
    run(38 * T, 41 * T, 2); run(41 * T, 44 * T); s[41 * T - 1] = 2   # three tiles of missing data next to three homozygous ones
    run(48 * T, 49 * T)                                     # one isolated tile (T = 8, hom_min = 16: not a qualifying run)
    run((nt - 1) * T, len(s))                               # the last two tiles of the segment
    return [s, np.zeros(5, np.uint8)]


@pytest.mark.parametrize("T", [8, 37])
def test_classifier_at_its_edges(hip, golden, oracle, T):
    """k_tile_class and the plan rule against numpy, tile for tile: 8-bin tiles (inside one aligned 16 bytes, or exactly one half), then
    37-bin tiles, which start at every byte alignment.  The glue flags hold every bit the rule demands (learning may have added more),
    and the E-step on that plan is inside the fast tolerance."""
    from test_gpu_estep import check_fast
    segs = planted(golden, T)
    p = golden.params("n64_curve")
    es = hip.HipEStep(64, mode=hip.MODE_FAST, chunk=T, warmup=64, hom_tiles=1, hom_min=16)
    es.load_segments(segs)
    with pytest.raises(hip.HipError):
        es.plan_tiles()                                      # no plan yet
    r = es.estep(p["a"], p["e"], p["a0"])
    pt = es.plan_tiles()
    cls, glue = rule(segs, T, 64, 16)
    assert len(pt["cls"]) == len(cls) == es.fast_plan()["tiles"]
    assert {1, 2, 3} <= set(cls.tolist()) if T == 8 else {1, 3} <= set(cls.tolist())     # the input shows every class
    bad = np.nonzero(pt["cls"] != cls)[0]
    assert len(bad) == 0, (bad[:20], pt["cls"][bad[:20]], cls[bad[:20]])
    miss = np.nonzero((pt["glue"] & glue) != glue)[0]
    assert len(miss) == 0, (miss[:20], pt["glue"][miss[:20]], glue[miss[:20]])
    if T == 8:
        k = 48 + 0                                           # the isolated tile: a hom tile, no qualifying run
        assert cls[k] == 2 and cls[k - 1] == 0 and cls[k + 1] == 0
    check_fast(r, oracle.estep(p["a"], p["e"], p["a0"], segs), p)
    es.close()


def test_options_and_inertness(hip, golden, inputs):
    """Values outside the options' domains are refused; exact mode ignores the option (the golden bits); hom_tiles = 0 is the context
    without the option, bit for bit, over two E-steps on the input of the finding."""
    for k, v in (("hom_tiles", 2), ("hom_tiles", -1), ("hom_tiles", 0.5), ("hom_min", -1)):
        es = hip.HipEStep(64, mode=hip.MODE_FAST)
        with pytest.raises(hip.HipError):
            es.set_option(k, v)
        es.close()
    key = "n64_curve"
    p = golden.params(key); g = golden.small
    es = hip.HipEStep(64, mode=hip.MODE_EXACT, hom_tiles=1, hom_min=5)
    es.load_segments(golden.segs_small)
    r = es.estep(p["a"], p["e"], p["a0"])
    assert bits_equal(r["A"], g[key + ".A"]) and bits_equal(r["E"], g[key + ".E"]) and bits_equal(r["A0"], g[key + ".A0"])
    assert r["LL"] == float(g[key + ".LL"]) and bits_equal(r["chk"], g[key + ".seg_chk"])
    es.close()
    ctx = [hip.HipEStep(64, mode=hip.MODE_FAST), hip.HipEStep(64, mode=hip.MODE_FAST, hom_tiles=0)]
    for es in ctx: es.load_segments(inputs.segs["main"])
    for key in ("curve", 1):
        q = inputs.params(key)
        r0, r1 = (es.estep(q["a"], q["e"], q["a0"]) for es in ctx)
        assert bits_equal(r0["A"], r1["A"]) and bits_equal(r0["E"], r1["E"]) and r0["LL"] == r1["LL"], key
        assert ctx[0].fast_plan() == ctx[1].fast_plan()
        assert all(np.array_equal(x, y) for x, y in zip(ctx[0].plan_tiles().values(), ctx[1].plan_tiles().values()))
    assert not (ctx[1].plan_tiles()["cls"] >= 2).any()
    for es in ctx: es.close()


def test_the_finding(hip, inputs):
    """A 45 k-bin run of homozygous bins, default plan (256-bin tiles, 3072-bin warm-ups), the FIRST E-step of a context.  Without the
    option the run is learned one repair round at a time and leaves cells outside the 1e-9 cell bound (profiles/r06_fuzz.txt sections
    9-10); with it the plan holds the run before the first sweep: inside every bound of check_fast, and at most a quarter of the repair
    rounds of the unchanged path in the same process (what is left to learning are the tiles at the run's edges).

    The plan: every full tile inside the run is a hom tile of a qualifying run and a member of one glued forward item -- each glued to
    its predecessor, except the run's first tile, which heads the item (its warm-up window lies in ordinary data: the rule does not reach
    it) -- and the rule alone glues nothing more than a warm-up past the run's end."""
    from test_gpu_estep import check_fast, relmax, tri_sums, FAST_TOL_STATS
    segs = inputs.segs["main"]
    p = inputs.curve
    on = hip.HipEStep(64, mode=hip.MODE_FAST, hom_tiles=1)
    off = hip.HipEStep(64, mode=hip.MODE_FAST, hom_tiles=0)
    res, d = {}, {}
    for name, es in (("on", on), ("off", off)):
        es.load_segments(segs)
        res[name] = es.estep(p["a"], p["e"], p["a0"])
        d[name] = es.fast_diag()
    off.close()
    rounds = {k: v["fwd_rounds"] + v["bwd_rounds"] for k, v in d.items()}
    repairs = {k: v["fwd_tiles"] + v["bwd_tiles"] for k, v in d.items()}
    print("\nhom_tiles finding, first E-step: repair rounds on %d off %d, tile repairs on %d off %d" % (rounds["on"], rounds["off"], repairs["on"], repairs["off"]))
    o = inputs.ref("main", "curve")
    check_fast(res["on"], o, p)
    assert rounds["off"] >= 20, d["off"]                    # a condition on the input: it shows the problem
    assert 4 * rounds["on"] <= rounds["off"], (d["on"], d["off"])
    pl = on.fast_plan(); pt = on.plan_tiles()
    T, W = pl["tile_len"], d["on"]["warmup"]
    assert T == 256 and W == 3072
    cls, glue = rule(segs, T, W, 0)
    n0 = (len(segs[0]) + T - 1) // T                         # tiles of the short segment
    inside = n0 + np.arange((RUN[0] + T - 1) // T, RUN[1] // T)
    assert len(inside) >= 170 and set(np.nonzero(cls == 3)[0].tolist()) == set(inside.tolist())   # (a condition on the input: no other qualifying run)
    assert (pt["cls"][inside] == 3).all() and np.array_equal(pt["cls"], cls)
    assert (pt["glue"][inside[1:]] & 1).all()
    assert ((pt["glue"] & glue) == glue).all()
    assert pl["glued_fwd"] <= len(inside) + (W + T - 1) // T + d["on"]["fwd_tiles"], (pl, d["on"])
    assert pl["glued_bwd"] <= len(inside) + (W + T - 1) // T + d["on"]["bwd_tiles"], (pl, d["on"])
    for key in (1, 2, 0):                                   # the parameters move; the plan stays
        q = inputs.params(key)
        check_fast(on.estep(q["a"], q["e"], q["a0"]), inputs.ref("main", key), q)
    f = on.estep_factored(q["a"], q["e"], q["a0"])
    o = inputs.ref("main", 0)
    assert relmax(f["sums"], tri_sums(o["A"])) < FAST_TOL_STATS and relmax(f["E"], o["E"]) < FAST_TOL_STATS
    on.close()


@pytest.mark.parametrize("variant", ["chunk1001", "two_launches", "walked", "mix"])
def test_variants(hip, inputs, variant):
    """The same input on the other paths of the item lists: a tile length that is no multiple of four (no shared matrix: one per tile),
    two launches of the back half with the run in the second list, the run walked instead of chained, and a run of homozygous AND missing
    bins (het-free tiles of both kinds: a matrix each).  First E-step, then a second one with other parameters."""
    from test_gpu_estep import check_fast
    from test_gpu_stress import GENOME
    opts = dict(chunk1001=dict(chunk=1001), two_launches=dict(GENOME, chunk=256, warmup=512), walked=dict(kc_min=0), mix=dict())[variant]
    name = "mix" if variant == "mix" else "main"
    es = hip.HipEStep(64, mode=hip.MODE_FAST, hom_tiles=1, **opts)
    es.load_segments(inputs.segs[name])
    for key in ("curve", 1):
        q = inputs.params(key)
        check_fast(es.estep(q["a"], q["e"], q["a0"]), inputs.ref(name, key), q)
        if key == "curve":
            pt = es.plan_tiles(); d = es.fast_diag()
            assert (pt["cls"] == 3).sum() >= 40 and d["structured"], d
            if variant == "two_launches": assert d["fused_launches"] == 2, d
            if variant == "mix":
                cls, _ = rule(inputs.segs[name], d["tile_len"], d["warmup"], 0)
                assert np.array_equal(pt["cls"], cls)
                T = d["tile_len"]; long = inputs.segs[name][1]
                assert any((long[k * T:(k + 1) * T] == 2).any() for k in range((RUN[0] + T - 1) // T, RUN[1] // T))   # (the input has such tiles)
    es.close()


def test_variant_n128(hip, inputs):
    """65..128 states (the other transfer-matrix and chain kernels): a 30 k-bin run in a 60 k-bin segment."""
    from test_gpu_estep import check_fast
    es = hip.HipEStep(128, mode=hip.MODE_FAST, hom_tiles=1)
    es.load_segments(inputs.segs["n128"])
    for key in (("n128", 1), ("n128", 2)):
        q = inputs.params(key)
        check_fast(es.estep(q["a"], q["e"], q["a0"]), inputs.ref("n128", key), q)
        assert (es.plan_tiles()["cls"] == 3).sum() >= 100 and es.fast_diag()["structured"]
    es.close()


def test_variant_batch(hip, inputs):
    """psmc_hip_estep_batch hands the option to its replicate contexts: two replicates over multisets of the segments, each inside the fast
    tolerance of the oracle on its multiset (per-segment statistics times the multiplicities)."""
    from test_gpu_estep import check_fast
    sels = [[1, 0, 1], [1]]
    keys = ["curve", 1]
    es = hip.HipEStep(64, mode=hip.MODE_FAST, hom_tiles=1)
    es.load_segments(inputs.segs["main"])
    got = es.estep_batch([(inputs.params(k)["a"], inputs.params(k)["e"], inputs.params(k)["a0"]) for k in keys], sels)
    for r, (sel, k) in enumerate(zip(sels, keys)):
        o = inputs.ref("main", k)
        want = dict(A=sum(o["seg_A"][i] for i in sel), E=sum(o["seg_E"][i][:2] for i in sel), LL=float(sum(o["seg_LL"][i] for i in sel)))
        check_fast(dict(A=got["A"][r], E=got["E"][r], LL=got["LL"][r]), want, inputs.params(k))
    es.close()
