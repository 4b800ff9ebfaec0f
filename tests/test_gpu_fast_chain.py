"""The transfer-matrix chain of the fast path up to 128 states looked at directly (psmc_amd/csrc/estep_struct.hip k_kcol2_struct<2> at
64 lanes, k_kcol_struct<8> at 65..128 states, k_kchain_struct<1|2>; api_fast.hip build_items add_runs / push_kc).  Every other test
that reaches this code judges the E-step's statistics only, and there a wrong matrix or chain is either repaired (the verify catches
the vector, the repair walks the run: only rounds and time show it) or, on tiles anchored to a segment's end, guarded by nothing
but the 1e-9 cell bound of check_fast.  Here, through the diagnostics psmc_hip_fast_chain_info / _list / _matrices and
psmc_hip_fast_tile_vectors (include/psmc_hip_diag.h):
  (a) every distinct matrix (slot x range) against the long-double product of its steps (tests/fast_chain_model.py range_matrix_ref),
  (b) every tile of every chain against the long-double product of the DEVICE's matrices, exponents and previous vector,
  (c) entry and bentry of every tile -- chained, walked or bulk -- against the long-double sweep from the segment's end,
  (d) the chain lists, slots and range count against chain_rule,
  (e) the statistics against the oracle (check_fast), at a second parameter set as well; where noted, walks against chains.
Regime: warm-ups at least as long as the segments.  Every tile is then anchored both ways, every walk starts at position 1 or L,
nothing is verified and nothing can be repaired (asserted: no tile repairs), so entry and bentry are what walks and chains wrote.

Bounds, u = 2^-53, n the state count (not the padded width), none taken from what the kernels return:
  (a) per column, on the cells of at least 1e-6 x the column's largest: 2 steps (n + 70) u -- per step a cell is a sum of at most n
      non-negative products, the factorisation gate admits 64 ulp on an entry of a, about six further roundings; doubled;
  (b) forward 2 sub (2 n + 4) u (per range an n-term sum, an n-term norm, the reciprocal, the product), backward 2 x 4 x (2 n + 73) u
      more for the at most four tail steps, referenced with the dense a;
  (c) 2 d (n + 70) u, d the steps from the end of the segment the sweep started at (at least 1: the start vector and the normalisation).
Lines that start with CHAINTEST (shown with -s) are the figures profiles/fast_chain_tests.txt records."""
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal
import fast_chain_model as fc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_COLS = (0, 1, 31, 32, 63, 64, 65)   # beyond 64 states: the columns the matrices past the eighth are compared on, and n - 1


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "host"), "libpsmc_host.so"], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


def build_input(golden, kind, T):
    src = golden.segs_mid[3]
    if kind == "gaps":
        return fc.gaps_input(src, T)
    if kind == "gaps-all":                       # all 12000 bins: 46 tiles of 256 and 224 bins
        return fc.gaps_input(src, T, n_tiles=len(src) // T, rest=len(src) % T)
    if kind == "gaps-45":
        return fc.gaps_input(src, T, n_tiles=45, rest=5)
    if kind == "head":
        return fc.head_input(src, T)
    if kind == "hom":
        return fc.hom_input(src, T)
    if kind == "budget":
        return fc.budget_input(src, T)
    raise KeyError(kind)


def tile_table(segs, T):
    """[(segment, lo, hi)] of the plan"""
    return [(s, lo, hi) for s, d in enumerate(segs) for lo, hi in fc.tiles_of(len(d), T)]


_ORC, _REFS = {}, {}


def oracle_of(oracle, key, par, segs):
    if key not in _ORC:
        _ORC[key] = oracle.estep(par[0], par[1], par[2], segs)
    return _ORC[key]


def refs_of(key, par, segs, T):
    """long-double entry / bentry of every tile, segments in order"""
    if key not in _REFS:
        r = [fc.boundary_refs(par[0], par[1], par[2], s, T) for s in segs]
        _REFS[key] = (np.concatenate([x[0] for x in r]), np.concatenate([x[1] for x in r]))
    return _REFS[key]


def check_lists(ch, rule):
    assert (ch["runs"][0], ch["runs"][1]) == (rule["runs"][0], rule["runs"][1]), (ch["runs"], rule["runs"])
    assert ch["kc"] == rule["kc"] and list(ch["kslot"]) == rule["kslot"] and list(ch["kuniq"]) == rule["kuniq"], (ch["kc"], rule["kc"], ch["kslot"], rule["kslot"])
    assert ch["sub"] == rule["sub"], (ch["sub"], rule["sub"])


def check_matrices(ch, par, segs, tt, n):
    """(a): worst error / bound over every slot and range, and the number of matrices looked at"""
    S, sub = ch["S"], ch["sub"]
    K, Kexp = ch["K"], ch["Kexp"]
    assert K.shape == (len(ch["kuniq"]), sub, S, S) and Kexp.shape == (len(ch["kuniq"]), sub, S)
    assert np.isfinite(K).all() and (K >= 0).all()
    assert np.array_equal(Kexp, np.round(Kexp)) and np.abs(Kexp).max() < 2 ** 30
    E = Kexp.astype(np.int64)
    worst, worst_abs, seen, full = 0.0, (0.0, 0.0), 0, 0
    for u, j in enumerate(ch["kuniq"]):
        t, d = ch["kc"][j]
        s, lo, hi = tt[t]
        ranges, _ = fc.kc_ranges(lo, hi, len(segs[s]), d == 1, sub)
        # tiles that share the slot hold the same observations over the same ranges, at the same positions mod 4
        for j2 in np.nonzero(np.asarray(ch["kslot"]) == u)[0]:
            t2, d2 = ch["kc"][j2]
            s2, lo2, hi2 = tt[t2]
            r2, _ = fc.kc_ranges(lo2, hi2, len(segs[s2]), d2 == 1, sub)
            assert d2 == d and [len(x) for x in r2] == [len(x) for x in ranges], (u, j, j2)
            for x, y in zip(ranges, r2):
                assert [(p % 4, int(segs[s][p - 1])) for p in x] == [(p % 4, int(segs[s2][p - 1])) for p in y], (u, j, j2)
        for js, r in enumerate(ranges):
            Kj, Ej = K[u, js], E[u, js]
            if not r:                               # a range of zero steps: the identity, exponents 0
                assert np.array_equal(Kj, np.eye(S)) and not Ej.any(), (u, js)
                seen += 1
                continue
            # (the exponent of a padded column is whatever the sweep of an all-zero column leaves: the chain reads exponents of positive entries only)
            assert not Kj[n:, :].any() and not Kj[:, n:].any(), "padded rows / columns of slot %d range %d" % (u, js)
            cols = None
            if n > 64:
                full += 1
                if full > 8:
                    cols = sorted({c for c in EDGE_COLS + (n - 1,) if c < n})
            ref = fc.range_matrix_ref(par[0], par[1], segs[s], r, d == 1, cols)
            err, bound = fc.matrix_error(Kj, Ej, ref, n, cols), fc.matrix_bound(len(r), n)
            if err / bound > worst:
                worst, worst_abs = err / bound, (err, bound)
            seen += 1
    return worst, worst_abs, seen


def check_chain(ch, vec, par, segs, tt, n):
    """(b): per direction the worst error / bound over every tile of every chain, and the tiles looked at"""
    S, sub = ch["S"], ch["sub"]
    E = ch["Kexp"].astype(np.int64)
    out = []
    for d in (0, 1):
        worst, worst_abs, seen = 0.0, (0.0, 0.0), 0
        bound = fc.apply_bound(sub, n, d == 1)
        for first, count, kc0 in ch["runs"][d]:
            order = list(range(first, first + count - 1)) if d == 0 else list(range(first + count - 1, first, -1))
            for i, t in enumerate(order):
                assert ch["kc"][kc0 + i] == (t, d), (first, count, kc0, i)
                u = int(ch["kslot"][kc0 + i])
                s, lo, hi = tt[t]
                nxt = t + 1 if d == 0 else t - 1
                x, got = vec[d][t], vec[d][nxt]
                assert not got[n:].any() and (got[:n] >= 0).all(), "padded states of a chain vector"
                want = fc.chain_tile_ref(par[0], par[1], segs[s], lo, hi, d == 1, [(ch["K"][u, js], E[u, js]) for js in range(sub)], x, n)
                err = fc.vector_error(got[:n], want)
                if err / bound > worst:
                    worst, worst_abs = err / bound, (err, bound)
                seen += 1
        out.append((worst, worst_abs, seen))
    return out


def check_vectors(vec, refs, tt, segs, n, other=None):
    """(c): per direction the worst error / bound over every tile that has the vector (other: a second set of device vectors, compared
    with vec within the sum of both bounds instead)"""
    out = []
    for d in (0, 1):
        worst, worst_abs, seen = 0.0, (0.0, 0.0), 0
        for t, (s, lo, hi) in enumerate(tt):
            L = len(segs[s])
            if np.isnan(refs[d][t]).any():
                continue                              # a segment's first tile forward, a tile of position L alone backward
            dist = lo - 1 if d == 0 else L - min(hi, L - 1) - 1
            bound = fc.vector_bound(dist, n) * (2 if other is not None else 1)
            assert not vec[d][t][n:].any(), "padded states of tile %d" % t
            err = fc.vector_error(vec[d][t][:n], refs[d][t] if other is None else other[d][t][:n])
            if err / bound > worst:
                worst, worst_abs = err / bound, (err, bound)
            seen += 1
        out.append((worst, worst_abs, seen))
    return out


#        id,                 input,      model,        T,   warm-up, options,                     what the input is for
CASES = [("gaps-" + m, "gaps", m, 64, 4096, {}, {}) for m in ("n64_curve", "n64_flat", "n23_curve", "n128_curve", "psmc3", "psmc63", "psmc65", "psmc100", "psmc127",
                                                               "rho_1e-6", "tmax_60")] + [
    ("gaps-n128_curve-kc_min2", "gaps", "n128_curve", 64, 4096, dict(kc_min=2), {}),
    ("gaps-psmc65-kc_min2", "gaps", "psmc65", 64, 4096, dict(kc_min=2), {}),
    ("gaps-T37-n64_curve", "gaps", "n64_curve", 37, 4096, {}, {}),
    ("gaps-T37-psmc63", "gaps", "psmc63", 37, 4096, {}, {}),
    ("gaps-T37-psmc127", "gaps", "psmc127", 37, 4096, dict(kc_min=2), {}),
    ("gaps-T256-n64_curve", "gaps-all", "n64_curve", 256, 16384, dict(kc_sub=4), {}),
    ("gaps-T256-rho_1e-6", "gaps-all", "rho_1e-6", 256, 16384, dict(kc_sub=4), {}),
    ("gaps-T8-n64_curve", "gaps-45", "n64_curve", 8, 4096, dict(kc_sub=16), dict(empty=1)),
    ("gaps-T8-psmc63", "gaps-45", "psmc63", 8, 4096, dict(kc_sub=16), dict(empty=1)),
    ("gaps-sub1-n64_flat", "gaps", "n64_flat", 64, 4096, dict(kc_sub=1), {}),
    ("gaps-sub3-n64_flat", "gaps", "n64_flat", 64, 4096, dict(kc_sub=3), {}),
    ("gaps-sub3-psmc3", "gaps", "psmc3", 64, 4096, dict(kc_sub=3), {}),
    ("head-n64_curve", "head", "n64_curve", 64, 4096, {}, dict(first_tile=1)),
    ("head-psmc63", "head", "psmc63", 64, 4096, {}, dict(first_tile=1)),
    ("head-psmc100", "head", "psmc100", 64, 4096, {}, dict(first_tile=1)),
    ("hom-n64_curve", "hom", "n64_curve", 64, 4096, dict(hom_tiles=1, hom_min=128, group_cap=1024), dict(hom=1)),
    ("hom-tmax_60", "hom", "tmax_60", 64, 4096, dict(hom_tiles=1, hom_min=128, group_cap=1024), dict(hom=1)),
    ("hom-n128_curve", "hom", "n128_curve", 64, 4096, dict(hom_tiles=1, hom_min=128, group_cap=1024, kc_min=4), dict(hom=1)),
    ("budget-n64_curve", "budget", "n64_curve", 8, 4096, dict(hom_tiles=1, hom_min=16, group_cap=160), dict(budget=1)),
]
# the figures of "gaps" by hand (tests/test_fast_chain_model.py test_chain_rule_gaps), tiles counted inside the long segment
GAPS_RUNS = [(4, 10), (29, 6), (39, 4)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_chain(hip, golden, oracle, case):
    from test_gpu_estep import check_fast
    name, kind, model, T, W, opts, purpose = case
    par = fc.model(golden, model)
    par2 = fc.model(golden, model, second=True)
    n = par[0].shape[0]
    segs = build_input(golden, kind, T)
    assert W >= max(len(s) for s in segs)
    tt = tile_table(segs, T)
    F = fc.front_tiles(T)
    es = hip.HipEStep(n, mode=hip.MODE_FAST, chunk=T, warmup=W, **opts)
    es.load_segments(segs)
    try:
        with pytest.raises(hip.HipError):
            es.fast_chains()                          # no plan with built lists yet
        r1 = es.estep(*par)
        d = es.fast_diag()
        pt = es.plan_tiles()
        ch = es.fast_chains()
        vec = [es.fast_tile_vectors(i) for i in range(3)]
        es.estep(*par)
        ch_again = es.fast_chains()
        vec_again = [es.fast_tile_vectors(i) for i in range(3)]
        r2 = es.estep(*par2)
        d2 = es.fast_diag()
        ch2 = es.fast_chains()
        vec2 = [es.fast_tile_vectors(i) for i in range(2)]
    finally:
        es.close()
    # conditions of the regime: the structured path, nothing repaired
    for dd in (d, d2):
        assert dd["structured"] and dd["fwd_tiles"] == 0 and dd["bwd_tiles"] == 0 and dd["n_chunks"] == len(tt) and dd["tile_len"] == T, dd
    assert ch["S"] == (64 if n <= 64 else 128) and ch["tiles"] == len(tt) and ch["tile_len"] == T
    assert all(v.shape == (len(tt), ch["S"]) for v in vec)
    # (d) the lists
    rule = fc.chain_rule(segs, T, W, pt["glue"], pt["cls"], n, **{k: v for k, v in opts.items() if k in ("kc_min", "kc_sub", "group_cap")})
    check_lists(dict(ch, runs=([r[:2] for r in ch["runs"][0]], [r[:2] for r in ch["runs"][1]])), rule)
    assert len(ch["runs"][0]) >= 1 and len(ch["runs"][1]) >= 1
    if kind == "gaps" and T == 64:
        want = [(F + a, b) for a, b in GAPS_RUNS] if (n <= 64 or opts.get("kc_min") == 2) else [(F + 4, 10)]
        assert sorted(r[:2] for r in ch["runs"][0]) == want and sorted(r[:2] for r in ch["runs"][1]) == want, ch["runs"]
        assert len(ch["kuniq"]) == 2 * (len(want) + 1)              # per direction one matrix per chain's data tile and one shared by the gap tiles
    if kind == "gaps" and T == 37:
        assert list(ch["kslot"]) == list(range(len(ch["kc"])))      # no shared slot
        assert {tt[t][1] % 4 for t, _ in ch["kc"]} == {0, 1, 2, 3}   # every lo % 4
    if purpose.get("first_tile"):
        assert any(tt[f - 1][1] == 1 for f, c, k in ch["runs"][0]), ch["runs"]      # chained from the second tile of its segment
    if purpose.get("empty"):
        assert ch["sub"] == 16
    if purpose.get("hom"):
        assert len(ch["runs"][0]) >= 2 and len(ch["runs"][1]) >= 2 and (pt["cls"][F + 20:F + 25] == 3).all()
        slot = {kt: int(ch["kslot"][j]) for j, kt in enumerate(ch["kc"])}
        for dr in (0, 1):
            assert slot[(F + 20 + dr, dr)] == slot[(F + 23, dr)] != slot[(F + 22, dr)], slot
        glued = sum(c for f, c, k in ch["runs"][0]), sum(c for f, c, k in ch["runs"][1])
        assert min(glued) >= 25                                       # every glued run is chained: data-bearing matrices with het bins
        assert any((segs[tt[t][0]][tt[t][1] - 1:tt[t][2]] == 1).any() for t, _ in ch["kc"])
    if purpose.get("budget"):
        for dr in (0, 1):    # about eight glued runs of 20 data tiles per direction, 19 of the budget of 64 each: some are chained, not all
            assert len(rule["glued"][dr]) >= 7 and 2 <= len(ch["runs"][dr]) < len(rule["glued"][dr]), (rule["glued"], ch["runs"])
    # a second E-step with the same parameters builds the same bits
    assert bits_equal(ch["K"], ch_again["K"]) and bits_equal(ch["Kexp"], ch_again["Kexp"])
    assert all(bits_equal(x, y) for x, y in zip(vec, vec_again))
    assert ch2["kc"] == ch["kc"] and ch2["runs"] == ch["runs"] and not bits_equal(ch2["K"], ch["K"])
    # (a), (b), (c) at both parameter sets
    figures = []
    for tag, p, c, v in (("", par, ch, vec), (" second", par2, ch2, vec2)):
        wa, fa, na = check_matrices(c, p, segs, tt, n)
        wb = check_chain(c, v, p, segs, tt, n)
        wc = check_vectors(v, refs_of((kind, model, T, tag), p, segs, T), tt, segs, n)
        assert na == len(c["kuniq"]) * c["sub"]
        assert wb[0][2] == sum(cnt - 1 for f, cnt, k in c["runs"][0]) and wb[1][2] == sum(cnt - 1 for f, cnt, k in c["runs"][1])
        print("\nCHAINTEST %s%s n %d T %d sub %d: chains %d + %d, (a) %d matrices worst %.2e of %.2e; (b) forward %.2e of %.2e, backward %.2e of %.2e (%d + %d tiles); "
              "(c) entry %.2e of %.2e, bentry %.2e of %.2e (%d + %d tiles)" % (
                  name, tag, n, T, c["sub"], len(c["runs"][0]), len(c["runs"][1]), na, fa[0], fa[1], wb[0][1][0], wb[0][1][1], wb[1][1][0], wb[1][1][1], wb[0][2], wb[1][2],
                  wc[0][1][0], wc[0][1][1], wc[1][1][0], wc[1][1][1], wc[0][2], wc[1][2]))
        figures.append((wa, wb[0][0], wb[1][0], wc[0][0], wc[1][0]))
    for f in figures:
        assert max(f) <= 1.0, (name, figures)
    # (e) the statistics
    pd = lambda p: dict(a=p[0], e=p[1], a0=p[2])
    check_fast(r1, oracle_of(oracle, (kind, model, T, ""), par, segs), pd(par))
    check_fast(r2, oracle_of(oracle, (kind, model, T, "second"), par2, segs), pd(par2))


@pytest.mark.parametrize("model", ["n64_curve", "rho_1e-6", "psmc63"])
def test_walks_against_chains(hip, golden, oracle, model):
    """ "gaps" at up to 64 states with kc_min = 0: every run is walked.  No chain is listed, the statistics pass check_fast, and entry and
    bentry of every tile agree with those the chains left within the sum of their (c) bounds."""
    from test_gpu_estep import check_fast
    T, W = 64, 4096
    par = fc.model(golden, model)
    n = par[0].shape[0]
    segs = build_input(golden, "gaps", T)
    tt = tile_table(segs, T)
    got = []
    for kc_min in (-1, 0):
        es = hip.HipEStep(n, mode=hip.MODE_FAST, chunk=T, warmup=W, kc_min=kc_min)
        es.load_segments(segs)
        try:
            r = es.estep(*par)
            d = es.fast_diag()
            ch = es.fast_chains()
            got.append((r, ch, [es.fast_tile_vectors(i) for i in range(2)]))
        finally:
            es.close()
        assert d["structured"] and d["fwd_tiles"] == 0 and d["bwd_tiles"] == 0, d
    assert len(got[0][1]["runs"][0]) == 3 and got[1][1]["runs"] == ([], []) and got[1][1]["kc"] == [] and got[1][1]["K"].size == 0
    refs = refs_of(("gaps", model, T, ""), par, segs, T)
    w = check_vectors(got[0][2], refs, tt, segs, n, other=got[1][2])
    ww = check_vectors(got[1][2], refs, tt, segs, n)
    print("\nCHAINTEST walks-%s n %d: chains against walks entry %.2e of %.2e, bentry %.2e of %.2e; walks against long double entry %.2e of %.2e, bentry %.2e of %.2e" % (
        model, n, w[0][1][0], w[0][1][1], w[1][1][0], w[1][1][1], ww[0][1][0], ww[0][1][1], ww[1][1][0], ww[1][1][1]))
    assert max(w[0][0], w[1][0], ww[0][0], ww[1][0]) <= 1.0
    check_fast(got[1][0], oracle_of(oracle, ("gaps", model, T, ""), par, segs), dict(a=par[0], e=par[1], a0=par[2]))


def test_no_lists_without_a_fast_plan(hip, golden):
    """PSMC_HIP_ESTATE before the first fast E-step, after an option that drops the plan, and on an exact context"""
    par = fc.model(golden, "n64_curve")
    segs = build_input(golden, "gaps", 64)
    es = hip.HipEStep(64, mode=hip.MODE_FAST, chunk=64, warmup=4096)
    es.load_segments(segs)
    try:
        for fn in (es.fast_chains, lambda: es.fast_tile_vectors(0)):
            with pytest.raises(hip.HipError):
                fn()
        es.estep_factored(*par)
        assert len(es.fast_chains()["runs"][0]) == 3 and es.fast_tile_vectors(2).shape == (len(tile_table(segs, 64)), 64)
        es.set_option("chunk", 128)
        with pytest.raises(hip.HipError):
            es.fast_chains()
    finally:
        es.close()
    ex = hip.HipEStep(64, mode=hip.MODE_EXACT)
    ex.load_segments(segs)
    try:
        ex.estep(*par)
        with pytest.raises(hip.HipError):
            ex.fast_chains()
    finally:
        ex.close()
