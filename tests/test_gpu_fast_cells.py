"""The fast E-step up to 128 states cell by cell, where nothing is speculated (psmc_amd/csrc: the fused back halves k_bwd_count4f_struct
and k_bwd_count8x_struct of estep_fused.hip, the unfused counts of estep_fast.hip, the factored sums k_bwd_acc_struct / k_bwd_acc_ckpt of
estep_factored.hip, the dense sweeps of estep_fast.hip).  Everywhere else these kernels are judged by check_fast alone
(tests/test_gpu_estep.py): 1e-9 relative on the cells of at least 1e-6 of the largest, nothing below -- a bound that has to absorb what
speculation and warm_tol leave behind, four orders of magnitude above the kernels' arithmetic, and silent on most cells (63 of 4225 cells
are above the floor at 65 states with rho0 = 1e-6).

Regime (that of tests/test_gpu_fast_chain.py): warmup = 4096 bins, at least the longest segment.  Every tile is anchored at a segment end
in both directions, nothing is verified, nothing repaired (asserted on every context: no tile repairs, the planned tiles and tile length).
The device and the oracle then differ by rounding alone, and every cell can be held at rounding level.

Cases: the thirteen models of tests/test_gpu_wide_fast_edges.py MODELS through the host model of the pattern "<n>*1" at 2, 3, 63, 64 (the
64-lane width at its emptiest and fullest) and 65, 127, 128 states (the 128-state width); a pair is a case where a, e and a0 are finite and
a >= 0 (NOT_HMM is the literal table of the others, STRUCT_REFUSED that of the cases the factorisation criterion refuses;
tests/test_fastmodel.py test_fast_cells_case_table holds the host model and the numpy criterion to both).  Data: 4827 bins in segments of 1, 2,
3, 63, 64, 65, 127, 129, 1000 and 3000 bins, all-missing ones of 3 and 70 bins and one of 300 bins with missing data at both ends.  Tilings:
chunk 37, 64, 1000 and the default (256): segments of 1, 2, 3, 4, 5, .. 47 and 82 tiles, so the groups of four (64 states) and sixteen (128)
tiles of the fused back halves come up full, ragged and shared between segments.

Gates on every back half (BACK_HALVES), every one an assert:
  (G1) check_fast, unchanged, on the full counts;
  (G2) every cell of A and every entry of E[0], E[1] whose oracle value is above 2^-900: relative error <= B = 32 max(E_ref, 64 x 2^-53);
       no cell non-finite or negative.  E_ref (tests/fastmodel.py reference_error) is the larger of the untiled dense and the untiled
       structured numpy model's worst relative error over the same cells against the oracle: the distance of two float64 evaluations of the
       same sums of non-negative terms.  The device is a third one in yet another association (16-lane row scans, four-deep matrix-core
       accumulation, per-tile partials added by the reductions, lag-4 normalisation); the maxima over up to 16384 cells of two such draws
       differ by small factors, hence 32.  The 64 ulp floor is the factorisation criterion's own allowance per entry of a.  B comes to
       2.3e-13 .. 1.4e-11 here, and it has no floor on the cell's size;
  (G3) the factored sums SL, SU, DG, CL, CU against tri_sums of the oracle's A under the same B with E_ref taken over the model's tri_sums;
       the structural zeros SL[0], SU[n-1], CL[n-1], CU[0] at most B x the vector's largest entry;
  (G4) LL within FAST_TOL_LL (the measured difference is printed beside the model's own);
  (G5) entries n .. of every tile's start vector (psmc_hip_fast_tile_vectors, entry and bentry) exactly zero.
A model the criterion refuses runs the dense sweeps up to 64 states (asserted) and has no factored statistics (ENOTSUP, asserted); beyond 64
states psmc_hip_estep is then the exact fallback and must equal the oracle bit for bit (no case of the table is refused there).
test_decoding_at_padded_sizes: the first run of k_post_fast<64> / <128> and k_post_mean_fast with 61, 1, 63 and 1 padded states, under the
tolerances of tests/test_gpu_fast_decode.py and tests/test_gpu_post_mean.py.

Lines that start with CELLTEST (shown with -s) are the figures profiles/fast_cells_tests.txt records: per case and back half the worst
error over the tilings, B, their ratio, the cell and tiling, E_ref.

Observed on the MI355X (78 tests, 16 s; 297 case x back-half lines): the worst error / B per back half is
  fused 0.041 (65 states, t_max = 60, A[5, 1], chunk 1000)      unfused 0.033 (2 states: the dense sweeps; 128 states 0.032)
  factored, with checkpoints, lanes8: 0.039 (3 states, lambda 1e3 .. 1e-3, E0[0])      dense 0.042 (3 states, rho0 = 1e-6, A[0, 1])
that is, the device is as far from the oracle as the numpy model is (1 / 32 = 0.031 is E_ref itself) -- at most 4.5e-13 on any cell;
LL within 9.1e-16 relative.  (G1) to (G4) found nothing wrong.  (G5) found one defect, at every size that leaves padded states (3, 63, 65,
127), in every structured back half: the bentry of a segment's last tile was 1.0 on ALL padded states when the segment ends in a missing
bin.  The backward start vector `B_q := 1` is e[o_q], and for a missing bin the sweeps took it from rows that hold 1 on every lane
(estep_struct.hip fill_lds_e; walk_ev in k_walk1_struct).  A step clears it (a padded state receives nothing), so no statistic moved, but
the ones sat in the first normalisation's sum and among the "positive entries" whose column exponents k_kchain_struct reads.  Start
vectors now come from the emission table's own row for a missing bin, which api.hip fill_params fills on the model's states only in fast
mode; 64 and 128 states keep their bits.  The all-missing segments of 3 and 70 bins and the 300-bin one are the cases that failed.
"""
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal
import fastmodel
from test_gpu_wide_fast_edges import MODELS, ragged_segs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = (2, 3, 63, 64, 65, 127, 128)
WARMUP = 4096
TILINGS = (37, 64, 1000, 0)            # "chunk"; 0: the plan's own choice, 256 bins on this input
DEFAULT_TILE = 256
# (model, n) pairs that are no HMM: a, e or a0 not finite, or a negative entry of a (survival past an interval underflows, or rho0 too large)
NOT_HMM = {
    "lambda_alt_1e-3_1e3": SIZES,
    "rho_0.5": SIZES,
    "lambda_ramp_down_1e3_1e-3": (63, 64, 65, 127, 128),
    "lambda_ramp_up_1e-3_1e3": (2, 3),
}
CASES = [(n, name) for n in SIZES for name in MODELS if n not in NOT_HMM.get(name, ())]
# cases api.hip factor_structure refuses at the default structured = 1: fewer than three states; dd < 0 at three states with rho0 = 0.1
STRUCT_REFUSED = {(2, name) for n, name in CASES if n == 2} | {(3, "rho_0.1")}
DECODE_SIZES = (3, 63, 65, 127)

#              tag,               entry point,      options up to 64 states, beyond (None: not built),  back_half
BACK_HALVES = [("fused",           "estep",          dict(),                  dict(),                    1),
               ("unfused",         "estep",          dict(fuse=0),            dict(fuse128=0),           0),
               ("factored-ckpt",   "estep_factored", dict(ckpt=1),            None,                      2),
               ("factored",        "estep_factored", dict(ckpt=0),            dict(ckpt=0),              2),
               ("factored-lanes8", "estep_factored", dict(lanes8=1),          None,                      2),
               ("dense",           "estep",          dict(structured=0),      None,                      0)]
SUMS = ("SL", "SU", "DG", "CL", "CU")
WORST = {}   # back half -> (ratio, what)


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "host"), "libpsmc_host.so"], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    """after the module: the worst error / B of every back half (shown with -s)"""
    yield
    for k in sorted(WORST):
        print("CELLTEST worst %-16s %.3f of B  %s" % (k, WORST[k][0], WORST[k][1]))


def host_model(name, n):
    """(a, e (3, n), a0) of MODELS[name] at n states: the host model of the pattern "<n>*1" """
    from psmc_amd import hostlib
    return hostlib.hmm_params("%d*1" % n, MODELS[name](n))


def is_hmm(par):
    a, e, a0 = par
    return bool(np.isfinite(a).all() and np.isfinite(e).all() and np.isfinite(a0).all() and (a >= 0).all())


def cells_segs(golden):
    rag = ragged_segs(golden)
    segs = golden.segs_small[:9] + [golden.segs_mid[3][:3000]] + [rag[11], rag[12], rag[13]]
    assert [len(s) for s in segs] == [1, 2, 3, 63, 64, 65, 127, 129, 1000, 3000, 3, 70, 300]
    assert (segs[10] == 2).all() and (segs[11] == 2).all() and (segs[12][:6] == 2).all() and (segs[12][-6:] == 2).all()
    return segs


_REF = {}


def reference(oracle, golden, n, name):
    """(par, oracle result, E_ref) of a case: computed once, only read afterwards"""
    if (n, name) not in _REF:
        par = host_model(name, n)
        segs = cells_segs(golden)
        o = oracle.estep(par[0], par[1], par[2], segs)
        _REF[(n, name)] = (par, o, fastmodel.reference_error(par[0], par[1], par[2], segs, o))
    return _REF[(n, name)]


def tile_table(segs, T):
    return [(s, lo, min(len(d), lo + T - 1)) for s, d in enumerate(segs) for lo in range(1, len(d) + 1, T)]


def check_padding(es, segs, T, n, bad, what):
    """(G5): the padded states of every start vector the sweeps wrote -- all but the entry of a segment's first tile and the bentry of a tile
    that holds position L alone -- are exactly zero, and the vector itself is one (finite, non-negative, not all zero); failures go to bad"""
    tt = tile_table(segs, T)
    for which in (0, 1):
        v = es.fast_tile_vectors(which)
        assert v.shape == (len(tt), 64 if n <= 64 else 128), (what, v.shape)
        for t, (s, lo, hi) in enumerate(tt):
            if (which == 0 and lo == 1) or (which == 1 and min(hi, len(segs[s]) - 1) < lo):
                continue
            if v[t, n:].any():
                bad.append("%s (G5) padded states of %s of tile %d (segment %d, %d .. %d): %d non-zero, largest %.3e" % (
                    what, ("entry", "bentry")[which], t, s, lo, hi, np.count_nonzero(v[t, n:]), np.abs(v[t, n:]).max()))
            if not (np.isfinite(v[t, :n]).all() and (v[t, :n] >= 0).all() and v[t, :n].sum() > 0):
                bad.append("%s (G5) %s of tile %d is no vector" % (what, ("entry", "bentry")[which], t))


def gate(got, ref, B, names, bad, what):
    """(G2) / (G3) on one array: (error, bound, cell); failures go to bad"""
    got = np.asarray(got)
    if not (np.isfinite(got).all() and (got >= 0).all()):
        bad.append("%s: a non-finite or negative cell" % (what,))
    err, at = fastmodel.cell_error(got, ref)
    if not err <= B:
        bad.append("%s: %.3e > B = %.3e at %s%s" % (what, err, B, names[at[0]] if names else "", list(at[1:] if names else at)))
    return err, ("%s%s" % (names[at[0]] if names else "", list(at[1:] if names else at))) if at is not None else "-"


def run_back_half(hip, segs, par, o, eref, n, chunk, entry, opts, want_struct, want_bh, what):
    """One context, one E-step: a record of its figures and the list of the gates it missed"""
    from test_gpu_estep import check_fast, FAST_TOL_LL
    a, e, a0 = par
    T = chunk or DEFAULT_TILE
    es = hip.HipEStep(n, mode=hip.MODE_FAST, warmup=WARMUP, **(dict(chunk=chunk) if chunk else {}), **opts)
    es.load_segments(segs)
    bad = []
    try:
        r = getattr(es, entry)(a, e, a0)
        d = es.fast_diag()
        # the regime, and the kernels that ran
        assert d["fwd_tiles"] == 0 and d["bwd_tiles"] == 0, (what, d)
        assert d["n_chunks"] == sum((len(s) + T - 1) // T for s in segs) and d["tile_len"] == T and d["warmup"] == WARMUP, (what, d)
        assert d["structured"] == want_struct and d["back_half"] == want_bh, (what, d)
        if entry == "estep_factored":
            assert d["ckpt"] == bool(opts.get("ckpt", 1) and n <= 64 and T % 8 == 0), (what, d)
        if want_struct:
            check_padding(es, segs, T, n, bad, what)
    finally:
        es.close()
    B, Bt = fastmodel.cell_bound(eref["cell"]), fastmodel.cell_bound(eref["tri"])
    rec = dict(chunk=chunk, B=B)
    errE, atE = gate(r["E"], o["E"], B, ("E0", "E1"), bad, what + " (G2) E")
    if entry == "estep":
        errA, atA = gate(r["A"], o["A"], B, None, bad, what + " (G2) A")
        rec["err"], rec["at"] = (errA, "A" + atA) if errA >= errE else (errE, atE)
        try:
            check_fast(r, o, dict(a=a, e=e, a0=a0))
        except AssertionError as ex:
            bad.append("%s (G1) check_fast: %s" % (what, ex))
    else:
        want = fastmodel.tri_sums(o["A"])
        errS, atS = gate(r["sums"], want, Bt, SUMS, bad, what + " (G3) sums")
        for v, k in ((0, 0), (1, n - 1), (3, n - 1), (4, 0)):   # the empty sums
            if not (want[v, k] == 0.0 and r["sums"][v, k] <= Bt * want[v].max()):
                bad.append("%s (G3) structural zero %s[%d] = %.3e" % (what, SUMS[v], k, r["sums"][v, k]))
        rec["err"], rec["at"], rec["B"] = (errS, atS, Bt) if errS / Bt >= errE / B else (errE, atE, B)
    rec["LL"] = abs(r["LL"] - o["LL"]) / abs(o["LL"])
    if not rec["LL"] <= FAST_TOL_LL:
        bad.append("%s (G4) LL %.3e" % (what, rec["LL"]))
    return rec, bad


@pytest.mark.parametrize("n,name", CASES, ids=["%d-%s" % c for c in CASES])
def test_cells(hip, golden, oracle, n, name):
    par, o, eref = reference(oracle, golden, n, name)
    segs = cells_segs(golden)
    assert is_hmm(par) and max(len(s) for s in segs) <= WARMUP
    refused = (n, name) in STRUCT_REFUSED
    failures = []
    for tag, entry, opts64, opts128, bh in BACK_HALVES:
        opts = opts64 if n <= 64 else opts128
        if opts is None:
            continue
        if refused and entry == "estep_factored":     # no factored statistics without the form
            es = hip.HipEStep(n, mode=hip.MODE_FAST, warmup=WARMUP, **opts)
            es.load_segments(segs)
            try:
                with pytest.raises(hip.HipError, match="PSMC form"):
                    es.estep_factored(*par)
            finally:
                es.close()
            continue
        if refused and n > 64:                        # the exact fallback: the oracle's bits
            es = hip.HipEStep(n, mode=hip.MODE_FAST, warmup=WARMUP, **opts)
            es.load_segments(segs)
            try:
                r = es.estep(*par)
                assert not es.fast_diag()["structured"]
            finally:
                es.close()
            assert bits_equal(r["A"], o["A"]) and bits_equal(r["E"], o["E"]) and r["LL"] == o["LL"], (n, name, tag)
            continue
        want_struct = not refused and tag != "dense"
        recs = []
        for chunk in TILINGS:
            if tag == "factored-ckpt" and (chunk or DEFAULT_TILE) % 8:
                continue                               # checkpoints every 8 positions: tile lengths that are multiples of 8
            what = "n %d %s %s chunk %d" % (n, name, tag, chunk)
            rec, bad = run_back_half(hip, segs, par, o, eref, n, chunk, entry, opts, want_struct, bh if want_struct else 0, what)
            recs.append(rec)
            failures += bad
        w = max(recs, key=lambda x: x["err"] / x["B"])
        ratio = w["err"] / w["B"]
        print("\nCELLTEST n %3d %-26s %-15s%s worst %.2e of B %.2e ratio %.3f at %s chunk %d; E_ref %.2e (sums %.2e); LL %.1e (model %.1e)" % (
            n, name, tag, " (dense sweeps: refused)" if refused else "", w["err"], w["B"], ratio, w["at"], w["chunk"], eref["cell"], eref["tri"],
            max(x["LL"] for x in recs), eref["LL"]), end="")
        if ratio > WORST.get(tag, (0.0, ""))[0]:
            WORST[tag] = (ratio, "n %d %s %s chunk %d" % (n, name, w["at"], w["chunk"]))
    print()
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind", ["mild", "rho_1e-6"])
@pytest.mark.parametrize("n", DECODE_SIZES)
def test_decoding_at_padded_sizes(hip, golden, n, kind):
    """k_post_fast<64> / <128> and k_post_mean_fast with 61, 1, 63 and 1 padded states: every decoding output and the per-bin posterior
    means of a fast context that kept bt against an exact context with the same parameters, under those files' own tolerances"""
    import fast_chain_model as fc
    from test_gpu_fast_decode import compare_decoding
    import test_gpu_post_mean as pm
    a, e, a0 = fc.model(golden, "psmc%d" % n) if kind == "mild" else host_model("rho_1e-6", n)
    segs = cells_segs(golden)
    fast = hip.HipEStep(n, mode=hip.MODE_FAST, chunk=64, warmup=WARMUP, **(dict(fuse=0) if n <= 64 else dict(fuse128=0)))
    fast.load_segments(segs)
    exact = hip.HipEStep(n, mode=hip.MODE_EXACT)
    exact.load_segments(segs)
    try:
        rf = fast.estep(a, e, a0)
        exact.estep(a, e, a0)
        d = fast.fast_diag()
        assert d["structured"] and d["back_half"] == 0 and d["fwd_tiles"] == 0 and d["bwd_tiles"] == 0 and d["tile_len"] == 64, d
        compare_decoding(fast, exact, segs, n, E=rf["E"])
        what = "fast cells %d %s" % (n, kind)
        try:
            pm.check_fast(fast, exact, len(segs), n, what)
        finally:   # (that file's report lists its own cases)
            print("CELLTEST post_mean %s: worst fraction of (B2), (B3): %s" % (what, pm.WORST.pop(what, None)))
    finally:
        fast.close(); exact.close()
