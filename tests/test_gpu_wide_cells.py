"""The wide fast path at 129 .. 1024 states cell by cell, where nothing is speculated (psmc_amd/csrc: the factored sweeps k_wf_fwd / k_wf_bwarm /
k_wf_acc of estep_wide_fast.hip at one wave and at 2 to 4 waves per tile, with and without "wide_ckpt"; the V pass k_wc_v and the split-K FP64
MFMA GEMM k_wc_gemm of estep_wide_counts.hip, with and without "wide_counts_ckpt").  Everywhere else these kernels are judged by the gates of
check_fast alone: 1e-9 relative on the cells of at least 1e-6 of the largest, nothing below, 1e-10 of the largest cell -- bounds that have to
absorb what speculation and warm_tol leave behind, and silent on most cells (with rho0 = 1e-6, 0.8 % of the cells of A are above that floor at
129 states and 0.1 % at 1024).  What a fault in the GEMM's edge handling would hit -- the masked ragged step, a one-row range, the empty splits of
a slab with fewer ranges than n_split, the read-back of a partial matrix on the second slab, the 64 x 64 block that holds a single real row at
129, 193, 257, 513 and 769 states -- are small off-diagonal cells under that floor.  This file is tests/test_gpu_fast_cells.py for these sizes.

Regime (that of tests/test_gpu_fast_cells.py): warmup = 4096 bins, at least the longest segment.  Every tile is anchored at a segment end in both
directions, nothing is verified, nothing repaired, no transfer-matrix chain is planned.  Asserted on every context: no repair round and no
repaired tile (fast_repairs out[0 .. 3]), the planned tiles sum(ceil(L / T)) and the tile length T, back half 3 (estep_factored) or 4 (estep with
"wide_counts"), and the checkpoint interval of wide_table_info the options ask for -- a silent fall-back to the exact kernels fails the test.

Sizes: each padded width at its emptiest and its fullest -- one wave 129, 192 | 193, 256; several waves ("wide_fast" = 2) 257, 512 | 513, 768 |
769, 1024.  Models: MODELS of tests/test_gpu_wide_fast_edges.py through the host model of the size's pattern (the tables of that file and of
tests/test_gpu_wide_fast_mw.py); up to 256 states all thirteen, beyond the four of LARGE_MODELS.  REFUSED is the literal table of the pairs that
are no HMM (a, e or a0 not finite, or a negative entry of a), which are also the pairs the factorisation criterion refuses: three models at every
size; tests/test_fastmodel.py test_wide_cells_case_table holds the host model and the numpy criterion to it.  A refused pair gets one assertion:
ENOTSUP with the "PSMC form" message from both entry points of the factored statistics (estep_factored and estep_factored_device).  psmc_hip_estep
has no such answer by design -- without the form it is the exact wide kernels (tests/test_gpu_wide_counts.py test_wide_counts_fallbacks) -- and
on a matrix that is no HMM neither they nor the oracle have a result to compare.
Data: up to 256 states cells_segs of tests/test_gpu_fast_cells.py (4827 bins: segments of 1, 2, 3, 63, 64, 65, 127, 129, 1000 and 3000 bins,
all-missing ones of 3 and 70 bins, one of 300 bins with missing data at both ends); beyond, small_segs (1127 bins: 1, 2, 3, 63, 64, 65, 127, 129,
300, 3, 70, 300).  Reference: the CPU oracle, once per case.  Tilings: chunk 37 (every range of the GEMM ends in a one-row masked step), 64 (every
range is 16 steps of 4), 1000 (a tile holds several ranges of WC_KC = 256 rows) and the plan's own 256; tiles that hold only position L come up.

Paths:  P1 estep_factored (all four tilings)                         P2 estep_factored, "wide_ckpt" (37, default)
        P3 estep, "wide_counts", one slab (all four)                 P4 estep, "wide_counts", "wide_counts_slab" = 64: several slabs (37, default)
        P5 estep, "wide_counts" + "wide_ckpt" + "wide_counts_ckpt", one slab (P5) and slabs of 64 rows (P5s) (37, default)
Gates, every one an assert, collected per case:
  (W1) gate() of tests/test_gpu_wide_counts.py, unchanged, on P3 and P4;
  (W2) on P3 and P4 every cell of A and every entry of E[0], E[1] whose oracle value is above 2^-900: relative error <= B =
       fastmodel.cell_bound(E_ref cell) = 32 max(E_ref, 64 x 2^-53); no cell non-finite or negative; no floor on the cell's size.  E_ref
       (tests/fastmodel.py reference_error) is the distance of two float64 evaluations of the same sums of non-negative terms, the numpy model
       against the oracle; the device is a third association (whole-wave scans, four-deep MFMA accumulation, n_split partials added in split
       order), hence the project's margin of 32;
  (W3) on P1 the sums SL, SU, DG, CL, CU against tri_sums of the oracle's A under Bt = cell_bound(E_ref tri), the four structural zeros at most
       Bt x their vector's largest entry, E under B;
  (W4) LL within FAST_TOL_LL (the measured difference is printed beside the model's own);
  (W5) bit for bit, at the same tiling: P2 = P1; P5 = P3 and P5s = P4; E and LL of P3 = those of P1;
  (W6) after P1 and P3, entries n .. of every start vector the sweeps wrote (wide_tile_vectors: all but the entry of a segment's first tile and the
       bentry of a tile that holds position L alone) exactly zero, entries 0 .. n-1 finite, non-negative and not all zero.
test_multiset: select() with repeats (the 129-bin segment three times, the all-missing 70-bin one twice, the one-bin one twice) at 193 and 769
states against the oracle on the expanded list under (W2) to (W4) and (W6): the multiplicity enters V through `mult` and must reach every cell.

Lines that start with WIDECELL (shown with -s) are the figures profiles/wide_cells_tests.txt records: per case and path the worst error over the
tilings, B, their ratio, the cell and tiling, E_ref.  PSMC_WIDE_CELLS_BITS=<file> appends one digest per context (for a bit comparison of two builds).

Observed on the MI355X (80 tests, 47 s, the slowest case 3.6 s; 392 case x path lines in profiles/wide_cells_tests.txt): the worst error / B per path is
  P1, P2 0.034 (192 states, lambda = 1, DG[4], chunk 37)      P3, P5 0.033 (192 states, theta0 = 1e-6, A[4, 5])
  P4, P5s 0.035 (256 states, lambda 100 .. 0.01, A[1, 171], default tiling)
that is, far below 1: the device is as far from the oracle as the numpy model is (1 / 32 = 0.031 is E_ref itself) -- at most 5.3e-13 on any cell
at any size, under B = 6.6e-13 .. 1.7e-11; LL within 1.8e-15 relative.  (W1) to (W5) found nothing wrong: the masked ragged step, the one-row
ranges, the empty splits, the read-back of the partials and the blocks with a single real row all hold every cell at rounding level, and the
checkpointed variants keep the bits under the extreme models too.  (W6) found the defect tests/test_gpu_fast_cells.py had found up to 128 states,
at every size that leaves padded states (129, 193, 257, 513, 769; 36 of the 80 tests failed): the bentry of a segment's last tile was 1.0 on ALL
padded states -- 63 at 129 and 193 states, 255 at 257, 513 and 769 -- when the segment ends in a missing bin (the all-missing segments of 3 and 70
bins and the 300-bin one).  k_wf_bwarm seeds the backward start vector `B_q := 1` with e[o_q], and emis() of wide_prims.h answers 1.0 on every
lane for a missing bin.  A step clears it (a padded state has zero matrix entries), but the ones sit in the sum of the first normalisation when
that falls on the seed (top % 4 == 0), and k_wc_v writes them into V's padded columns, which the GEMM multiplies into columns of C nobody reads.
k_wf_bwarm now zeroes the padded states of the vector it stores (behind a warm-up step they are zero already, so only a vector that no step
followed changes; its other start vectors need nothing: the forward seeds are a0 . e, and the rows of the gap / hom / mix chains are unit vectors
on real states).  Against the parent commit all 1040 contexts of this file keep their bits -- 192, 256, 512, 768 and 1024 states as they must, and
the padded sizes too: no statistic moved, since no segment here that ends in a missing bin has (L - 1) % 4 == 0; where one has, the ones entered
the factor that tile's first scaling applies to all of bt, a factor the posterior normalisation divides out again up to rounding.  Zeroing the
seed itself passes every gate here as well, but moves the last bits of speculated start vectors (a warm-up that starts on a missing bin with a
scaled first step), which the EM comparison of tests/test_host_cli_wide_fast.py amplifies beyond its bound: profiles/wide_cells_tests.txt.
"""
import hashlib
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal
import fastmodel
from test_gpu_fast_cells import cells_segs, is_hmm, tile_table
import test_gpu_wide_fast_edges as edges
import test_gpu_wide_fast_mw as mw
from test_gpu_wide_fast_edges import MODELS, ragged_segs
from test_gpu_wide_fast import ran_wide
from test_gpu_wide_counts import ONE_WAVE, gate as counts_gate, ran_counts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES_1W = (129, 192, 193, 256)
SIZES_MW = (257, 512, 513, 768, 769, 1024)
SIZES = SIZES_1W + SIZES_MW
PATTERNS = {n: (edges.SIZES if n in edges.SIZES else mw.SIZES)[n] for n in SIZES}   # states: pattern, free lambdas
assert all(ONE_WAVE[n] == edges.SIZES[n] for n in SIZES_1W)
LARGE_MODELS = ("lambda_equal", "rho_1e-6", "tmax_60", "lambda_ramp_down_1e2_1e-2")
WARMUP = 4096
TILINGS = (37, 64, 1000, 0)            # "chunk"; 0: the plan's own choice, 256 bins on these inputs
FEW = (37, 0)
DEFAULT_TILE = 256
# (model: sizes) that are no HMM -- survival past an interval with lambda -> 1e-3 underflows in the host model (a[0][n-1] = 0, a[n-1][0] = NaN), or
# the host model's matrix has negative entries at rho0 = 0.5 -- and that the factorisation criterion refuses; every other pair is accepted
REFUSED = {"lambda_alt_1e-3_1e3": SIZES, "lambda_ramp_down_1e3_1e-3": SIZES, "rho_0.5": SIZES}
CASES = [(n, name) for n in SIZES_1W for name in MODELS] + [(n, name) for n in SIZES_MW for name in LARGE_MODELS]

#         tag,   entry point,      options,                                                                     tilings, back half, interval
PATHS = [("P1",  "estep_factored", dict(),                                                                      TILINGS, 3, 1),
         ("P2",  "estep_factored", dict(wide_ckpt=1),                                                           FEW,     3, 8),
         ("P3",  "estep",          dict(wide_counts=1, wide_counts_slab=0),                                     TILINGS, 4, 1),
         ("P4",  "estep",          dict(wide_counts=1, wide_counts_slab=64),                                    FEW,     4, 1),
         ("P5",  "estep",          dict(wide_counts=1, wide_ckpt=1, wide_counts_ckpt=1, wide_counts_slab=0),    FEW,     4, 8),
         ("P5s", "estep",          dict(wide_counts=1, wide_ckpt=1, wide_counts_ckpt=1, wide_counts_slab=64),   FEW,     4, 8)]
SAME_BITS = (("P2", "P1"), ("P5", "P3"), ("P5s", "P4"))   # (W5), whole results; and E, LL of P3 against P1
SUMS = ("SL", "SU", "DG", "CL", "CU")
WORST = {}   # path -> (ratio, what)


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "host"), "libpsmc_host.so"], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    """after the module: the worst error / B of every path (shown with -s)"""
    yield
    for k in sorted(WORST):
        print("WIDECELL worst %-4s %.3f of B  %s" % (k, WORST[k][0], WORST[k][1]))


def host_model(name, n):
    """(a, e (3, n), a0) of MODELS[name] at n states: the host model of the size's pattern"""
    from psmc_amd import hostlib
    pat, m = PATTERNS[n]
    return hostlib.hmm_params(pat, MODELS[name](m))


def small_segs(golden):
    segs = golden.segs_small[:8] + [golden.segs_mid[3][:300]] + ragged_segs(golden)[11:14]
    assert [len(s) for s in segs] == [1, 2, 3, 63, 64, 65, 127, 129, 300, 3, 70, 300]
    assert (segs[9] == 2).all() and (segs[10] == 2).all() and (segs[11][:6] == 2).all() and (segs[11][-6:] == 2).all()
    return segs


def data(golden, n):
    return cells_segs(golden) if n <= 256 else small_segs(golden)


_REF = {}


def reference(oracle, golden, n, name, multiset=False):
    """(par, oracle result, E_ref) of a case (multiset: of small_segs expanded by MULTISET): computed once, only read afterwards"""
    key = (n, name, multiset)
    if key not in _REF:
        par = host_model(name, n)
        segs = [small_segs(golden)[i] for i in MULTISET] if multiset else data(golden, n)
        o = oracle.estep(par[0], par[1], par[2], segs)
        _REF[key] = (par, o, fastmodel.reference_error(par[0], par[1], par[2], segs, o))
    return _REF[key]


def check_padding(es, used, T, n, bad, what):
    """(W6): the padded states of every start vector the sweeps wrote -- all but the entry of a segment's first tile and the bentry of a tile
    that holds position L alone -- are exactly zero, and the vector itself is one (finite, non-negative, not all zero); failures go to bad"""
    tt = tile_table(used, T)
    S = 64 * ((n + 63) // 64) if n <= 256 else 256 * ((n + 255) // 256)
    for which in (0, 1):
        v = es.wide_tile_vectors(which)
        assert v.shape == (len(tt), S), (what, v.shape)
        for t, (s, lo, hi) in enumerate(tt):
            if (which == 0 and lo == 1) or (which == 1 and min(hi, len(used[s]) - 1) < lo):
                continue
            if v[t, n:].any():
                bad.append("%s (W6) padded states of %s of tile %d (segment %d, %d .. %d): %d non-zero, largest %.3e" % (
                    what, ("entry", "bentry")[which], t, s, lo, hi, np.count_nonzero(v[t, n:]), np.abs(v[t, n:]).max()))
            if not (np.isfinite(v[t, :n]).all() and (v[t, :n] >= 0).all() and v[t, :n].sum() > 0):
                bad.append("%s (W6) %s of tile %d is no vector" % (what, ("entry", "bentry")[which], t))


def gate(got, ref, B, names, bad, what):
    """(W2) / (W3) on one array: (error, cell); failures go to bad"""
    got = np.asarray(got)
    if not (np.isfinite(got).all() and (got >= 0).all()):
        bad.append("%s: a non-finite or negative cell" % (what,))
    err, at = fastmodel.cell_error(got, ref)
    if not err <= B:
        bad.append("%s: %.3e > B = %.3e at %s%s" % (what, err, B, names[at[0]] if names else "", list(at[1:] if names else at)))
    return err, ("%s%s" % (names[at[0]] if names else "", list(at[1:] if names else at))) if at is not None else "-"


def digest(what, r):
    path = os.environ.get("PSMC_WIDE_CELLS_BITS")
    if path:
        h = hashlib.sha1()
        for k in ("A", "sums", "E"):
            if k in r:
                h.update(np.ascontiguousarray(r[k], dtype=np.float64).tobytes())
        h.update(np.float64(r["LL"]).tobytes())
        with open(path, "a") as f:
            f.write("%s %s\n" % (what, h.hexdigest()))


def run_path(hip, segs, par, o, eref, n, chunk, tag, entry, opts, want_bh, want_iv, what, sel=None):
    """One context, one E-step: the result, a record of its figures and the list of the gates it missed"""
    from test_gpu_estep import FAST_TOL_LL
    a, e, a0 = par
    T = chunk or DEFAULT_TILE
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=1 if n <= 256 else 2, warmup=WARMUP, **(dict(chunk=chunk) if chunk else {}), **opts)
    es.load_segments(segs)
    used = segs
    if sel is not None:
        es.select(sel)
        used = [segs[i] for i in dict.fromkeys(sel)]   # the plan's order: first occurrence
    bad = []
    try:
        r = getattr(es, entry)(a, e, a0)
        # the regime, and the kernels that ran
        d = ran_wide(es) if want_bh == 3 else ran_counts(es)
        assert d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0 and d["fwd_tiles"] == 0 and d["bwd_tiles"] == 0, (what, d)
        assert d["n_chunks"] == sum((len(s) + T - 1) // T for s in used) and d["tile_len"] == T and d["warmup"] == WARMUP, (what, d)
        assert d["structured"] and d["back_half"] == want_bh, (what, d)
        assert es.wide_table_info()["interval"] == want_iv, (what, es.wide_table_info())
        if tag in ("P1", "P3"):
            check_padding(es, used, T, n, bad, what)
    finally:
        es.close()
    digest(what, r)
    B, Bt = fastmodel.cell_bound(eref["cell"]), fastmodel.cell_bound(eref["tri"])
    rec = dict(chunk=chunk, B=B)
    errE, atE = gate(r["E"], o["E"], B, ("E0", "E1"), bad, what + " (W2) E")
    if entry == "estep":
        errA, atA = gate(r["A"], o["A"], B, None, bad, what + " (W2) A")
        rec["err"], rec["at"] = (errA, "A" + atA) if errA >= errE else (errE, atE)
        try:
            counts_gate(r, o, (a, e), what)
        except AssertionError as ex:
            bad.append("%s (W1) gate: %s" % (what, ex))
    else:
        want = fastmodel.tri_sums(o["A"])
        errS, atS = gate(r["sums"], want, Bt, SUMS, bad, what + " (W3) sums")
        for v, k in ((0, 0), (1, n - 1), (3, n - 1), (4, 0)):   # the empty sums
            if not (want[v, k] == 0.0 and r["sums"][v, k] <= Bt * want[v].max()):
                bad.append("%s (W3) structural zero %s[%d] = %.3e" % (what, SUMS[v], k, r["sums"][v, k]))
        rec["err"], rec["at"], rec["B"] = (errS, atS, Bt) if errS / Bt >= errE / B else (errE, atE, B)
    rec["LL"] = abs(r["LL"] - o["LL"]) / abs(o["LL"])
    if not rec["LL"] <= FAST_TOL_LL:
        bad.append("%s (W4) LL %.3e" % (what, rec["LL"]))
    return r, rec, bad


def report(n, name, tag, recs, eref):
    w = max(recs, key=lambda x: x["err"] / x["B"])
    ratio = w["err"] / w["B"]
    print("WIDECELL n %4d %-26s %-4s worst %.2e of B %.2e ratio %.3f at %s chunk %d; E_ref %.2e (sums %.2e); LL %.1e (model %.1e)" % (
        n, name, tag, w["err"], w["B"], ratio, w["at"], w["chunk"], eref["cell"], eref["tri"], max(x["LL"] for x in recs), eref["LL"]))
    if ratio > WORST.get(tag, (0.0, ""))[0]:
        WORST[tag] = (ratio, "n %d %s %s chunk %d" % (n, name, w["at"], w["chunk"]))


def same_bits(r, w, keys):
    return all(bits_equal(r[k], w[k]) for k in keys if k != "LL") and r["LL"] == w["LL"]


@pytest.mark.parametrize("n,name", CASES, ids=["%d-%s" % c for c in CASES])
def test_wide_cells(hip, golden, oracle, n, name):
    segs = data(golden, n)
    assert max(len(s) for s in segs) <= WARMUP
    if n in REFUSED.get(name, ()):                     # no factored statistics without the form, from either entry point
        import torch
        a, e, a0 = host_model(name, n)
        es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=1 if n <= 256 else 2, warmup=WARMUP)
        es.load_segments(segs)
        stats = torch.zeros(7 * n + 1, dtype=torch.float64, device="cuda")
        try:
            with pytest.raises(hip.HipError, match="PSMC form") as e1:
                es.estep_factored(a, e, a0)
            with pytest.raises(hip.HipError, match="PSMC form") as e2:
                es.estep_factored_device(a, e, a0, stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert "not supported" in str(e1.value) and "not supported" in str(e2.value), (str(e1.value), str(e2.value))
        finally:
            es.close()
        return
    par, o, eref = reference(oracle, golden, n, name)
    assert is_hmm(par)
    failures, res = [], {}
    for tag, entry, opts, tilings, bh, iv in PATHS:
        recs = []
        for chunk in tilings:
            what = "n %d %s %s chunk %d" % (n, name, tag, chunk)
            res[(tag, chunk)], rec, bad = run_path(hip, segs, par, o, eref, n, chunk, tag, entry, opts, bh, iv, what)
            recs.append(rec)
            failures += bad
        report(n, name, tag, recs, eref)
    for x, y in SAME_BITS:                             # (W5)
        for chunk in FEW:
            if not same_bits(res[(x, chunk)], res[(y, chunk)], ("A", "E", "LL") if "A" in res[(y, chunk)] else ("sums", "E", "LL")):
                failures.append("n %d %s (W5) %s and %s differ at chunk %d" % (n, name, x, y, chunk))
    for chunk in TILINGS:
        if not same_bits(res[("P3", chunk)], res[("P1", chunk)], ("E", "LL")):
            failures.append("n %d %s (W5) E, LL of P3 and P1 differ at chunk %d" % (n, name, chunk))
    assert not failures, "\n".join(failures)


MULTISET = [7, 10, 0, 7, 10, 7, 0]   # of small_segs: the 129-bin segment three times, the all-missing 70-bin one twice, the one-bin one twice


@pytest.mark.parametrize("name", ["rho_1e-6", "lambda_equal"])
@pytest.mark.parametrize("n", [193, 769])
def test_multiset(hip, golden, oracle, n, name):
    """select() with repeats against the oracle on the expanded list: (W2) to (W4) and (W6) on P1 and P3, chunk 37 and the default"""
    segs = small_segs(golden)
    assert [len(segs[i]) for i in MULTISET] == [129, 70, 1, 129, 70, 129, 1]
    par, o, eref = reference(oracle, golden, n, name, multiset=True)
    failures = []
    for tag, entry, opts, tilings, bh, iv in PATHS:
        if tag not in ("P1", "P3"):
            continue
        recs = []
        for chunk in FEW:
            what = "n %d %s multiset %s chunk %d" % (n, name, tag, chunk)
            r, rec, bad = run_path(hip, segs, par, o, eref, n, chunk, tag, entry, opts, bh, iv, what, sel=MULTISET)
            if entry == "estep":                       # every transition adds its multiplicity to the sum of A
                trans = float(sum(len(segs[i]) - 1 for i in MULTISET))
                if not abs(r["A"].sum() - trans) <= 1e-9 * trans:
                    bad.append("%s: sum of A %.12g, transitions %g" % (what, r["A"].sum(), trans))
            recs.append(rec)
            failures += bad
        report(n, name + " multiset", tag, recs, eref)
    assert not failures, "\n".join(failures)
