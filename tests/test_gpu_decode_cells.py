"""Decoding from the tables of a fast E-step entry by entry against the CPU oracle, where nothing is speculated (psmc_amd/csrc: k_post_fast,
k_post_mean_fast, k_scales_fast and k_post_counts_fast of estep_post_fast.hip up to 128 states; k_wp_dec in all its flag combinations and its
CKPT variants, k_wp_scales, k_wp_scales_ck and k_wp_cnt_add of estep_wide_post.hip at 129 .. 1024 states; the host path api_decode.hip that picks
the tables).  Everywhere else these kernels are compared with an EXACT CONTEXT under 1e-9 absolute on posterior rows, maxp and recomb, 1e-9
relative on the post-count cells of at least 1e-6 of the largest and a 2e-9 tie rule for the path -- at 1024 states the mean posterior entry is
1e-3, so 1e-9 absolute is 1e-6 relative on a typical entry and silent on the rest -- and at the golden parameters only.  A wrong small posterior
entry moves a -D row and a TMRCA track without moving any sum those tests see.  This file is tests/test_gpu_fast_cells.py and
tests/test_gpu_wide_cells.py for what the project hands out per bin.

Regime (that of the two cell files): warmup = 4096 bins, at least the longest segment; nothing is verified, nothing repaired.  Asserted on every
context: no repair round and no repaired tile, the planned tiles sum(ceil(L / T)) and the tile length T, the back half that keeps the tables
(0 up to 128 states, with the sweeps the case must run: structured or dense; 3 and "recounted" = 2 beyond: the wide fast E-step whose X, entry
and bentry the wide decoding reads) and the checkpoint interval of wide_table_info -- a silent fall-back to the exact tables fails the test.

Cases, imported: CASES of tests/test_gpu_fast_cells.py at 2, 3, 63, 64, 65, 127, 128 states (70); at 129, 192, 193, 256 every model of MODELS
that REFUSED of tests/test_gpu_wide_cells.py does not list (40); at 257, 512, 513, 768, 769, 1024 its LARGE_MODELS (24).
tests/test_fastmodel.py test_decode_cells_case_table holds the tables to NOT_HMM, STRUCT_REFUSED and REFUSED of those files.  Data: cells_segs up
to 256 states (4827 bins), small_segs beyond (1127 bins): segments of 1, 2 and 3 bins, all-missing ones of 3 and 70 bins, one that begins and
ends in missing data.  Reference: the oracle's fwd_bwd / post_full / post_decode / post_counts of every segment and post_oracle @ w in
numpy.longdouble, once per case (reference(); the last case is kept: up to 10 MB each).

Paths:  D1  up to 128 states, unfused back half (fuse=0 / fuse128=0), structured sweeps (the dense ones where STRUCT_REFUSED lists the case): chunk
            37, 64, 1000, default          D2  up to 64 states, dense sweeps (structured=0): 37, default
        D3  129 .. 1024 states, "wide_fast" = 1 (2 beyond 256 states), "wide_decode" = 1: all four tilings
        D4  D3 + "wide_ckpt" = 1, "wide_decode_ckpt" = 1: 37, default      D0  an exact context, at D0_CASES
Calls, on every segment of every path: posterior (rows and recomb together and each alone: all flag combinations of k_wp_dec), decode, scales,
post_counts with 1, 5 and 9 columns, once into a fresh table per segment and once into running totals over the segments
(fastmodel.count_tables: rng.integers(0, 50); fastmodel.count_lengths: l = L, except L - 3 = 126 on the 129-bin segment -- it ends inside a tile at
every tiling and inside a block of eight rows, and at chunk 64 the tile that holds position L alone counts nothing --, L + 5 on the 1000-bin
segment (300 bins beyond 256 states), L // 2 + 1 = 151 on the last, 300-bin one, whose later tiles count nothing, 2051 on the 3000-bin one, three
positions into the second block of PCNT_BLK = 2048, and as compare_decoding has them an empty record on the 2-bin segment and L + 5 on the 3-bin one),
post_mean with four columns and with one (fastmodel.decode_weights: the host model's t_k, t_k^2, the indicator k >=
n // 2, all ones -- non-negative).

Gates, every one an assert, collected per case.  B_x = fastmodel.cell_bound(E_ref of output x) = 32 max(E_ref, 64 x 2^-53), E_ref
(fastmodel.decode_reference_error) the distance of the untiled numpy model of the same formulas, dense and structured, from the oracle: two
float64 evaluations of the same sums of non-negative terms; the device is a third association, hence the project's margin of 32.
  (P1) every posterior entry whose oracle value is above 2^-900: relative error <= B_post; every entry finite and >= 0; an entry the oracle puts
       at or below 2^-900 at most 2^-899; every row sums to 1 within B_post;
  (P2) maxp: relative <= B_maxp;
  (P3) recomb: absolute <= B_recomb (it is 1 - x with x near 1), inside [-B_recomb, 1 + B_recomb], exactly 0 at position L;
  (P4) scales: relative <= B_scales at every position;
  (P5) path: the oracle's at every position where the oracle's two largest entries differ by more than 2 B_post x maxp.  The excused positions
       are a condition on the input: at most 0.1 % of a case's positions, none in a case whose smallest relative top-two gap exceeds 1e-9.  No
       case has one, the 1000- and 3000-bin segments of cells_segs included (checked on the CPU, all 134 cases): the smallest relative gap is
       5.9e-10 (lambda = 1 at 1024 states, where 2 B_post = 2.2e-11), on cells_segs 3.8e-9 (theta0 = 1e-6 at 128 states, 2 B_post = 7.3e-12), so
       no segment had to be dropped from the path gate, and the numpy model's path is the oracle's at every position of every case;
  (P6) post_counts cells above 2^-900, of every segment alone and of the running totals: relative <= B_counts, and a cell the oracle leaves at 0
       is 0; post_mean: relative <= B_mean per column, the all-ones column 1 within B_mean;
  (P7) D4 = D3 bit for bit at the same tiling on every output; the post_mean of a fast context within B_mean of numpy.longdouble over its own
       rows; D0 = the oracle bit for bit on rows, recomb, path, maxp, scales and post_counts (per segment and running totals);
  (P8) after all the calls a second E-step on the context returns the bits of the first.

Lines that start with DECODECELL (shown with -s) are the figures profiles/decode_cells_tests.txt records: per case and path the worst error / B
over outputs, segments and tilings with its output, bound, entry, tiling and E_ref, then the ratio of every output; after the module the worst
ratio of every path, the largest error of every output and the number of path positions (P5) excused.
PSMC_DECODE_CELLS_BITS=<file> appends one digest per context (for a bit comparison of two builds).

Observed on the MI355X (134 tests, 70 s, the slowest case 1.7 s; 238 case x path lines in profiles/decode_cells_tests.txt): the worst error / B per
path is
  D1 0.035 (65 states, lambda 100 .. 0.01, post_mean, chunk 1000)      D2 0.032 (63 states, lambda = 1, post_mean, chunk 37)
  D3, D4 0.035 (193 states, lambda = 1, a posterior entry of the all-missing 70-bin segment)
that is, far below 1: the device is as far from the oracle as the numpy model is (1 / 32 = 0.031 is E_ref itself) on every output -- posterior
entries within 7.0e-13 relative (256 states, rho0 = 1e-6), maxp 4.6e-13, recomb 1.7e-13 absolute, scales 5.2e-14, post_counts cells 6.1e-13 (one
segment alone), post_mean 1.7e-13, under bounds of 2.3e-13 .. 2.3e-11.  No position is excused under (P5) and the path is the oracle's at every
position of every case, path and tiling.  (P1) to (P8) found nothing wrong: the sums over all 64 or 128 lanes with padded states, position L, the
tile-first denominators of the scales, the extra backward sweep from bentry, the exchange slots, the blocks of eight recomputed rows, the passes of
eight and four count columns, count records that end inside a tile, a block of eight rows or the second block of 2048 positions, tiles behind a
record's end, records longer than the segment and the empty one all hold every entry at rounding level under the extreme models too; D4 has the
bits of D3 and the exact contexts the oracle's.  No bound was raised.
"""
import hashlib
import os
import subprocess
import numpy as np
import pytest
from conftest import bits_equal
import fastmodel
import test_gpu_fast_cells as cells
import test_gpu_wide_cells as wc
from test_gpu_wide_fast_edges import MODELS
from test_gpu_wide_fast import ran_wide

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WARMUP = 4096
TILINGS = (37, 64, 1000, 0)            # "chunk"; 0: the plan's own choice, 256 bins on these inputs
FEW = (37, 0)
DEFAULT_TILE = 256
CASES = list(cells.CASES) + [(n, name) for n, name in wc.CASES if n not in wc.REFUSED.get(name, ())]
D0_SIZES = (3, 65, 129, 257)           # sizes that leave padded states, one per kernel width and table kind
D0_MODELS = ("rho_1e-6", "lambda_ramp_down_1e2_1e-2")
D0_CASES = {(n, name) for n in D0_SIZES for name in D0_MODELS}
OUTPUTS = fastmodel.DECODE_OUTPUTS
TINY_ENTRY = 2.0 ** -899               # what an entry the oracle puts at or below CELL_FLOOR may be at most
MAX_EXCUSED = 1e-3                     # of a case's positions
WORST = {}       # path -> (ratio, what)
LARGEST = {}     # output -> (error, its bound, what)
EXCUSED = [0]    # positions excused under (P5), all cases


def paths(n, refused):
    """[(tag, entry point, options, tilings, structured sweeps?, back half, checkpoint interval)] of a size"""
    if n <= 128:
        unfused = dict(fuse=0) if n <= 64 else dict(fuse128=0)
        out = [("D1", "estep", unfused, TILINGS, not refused, 0, 0)]
        if n <= 64:
            out.append(("D2", "estep", dict(structured=0), FEW, False, 0, 0))
        return out
    wide = dict(wide_fast=1 if n <= 256 else 2, wide_decode=1)
    return [("D3", "estep_factored", wide, TILINGS, True, 3, 1),
            ("D4", "estep_factored", dict(wide, wide_ckpt=1, wide_decode_ckpt=1), FEW, True, 3, 8)]


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "host"), "libpsmc_host.so"], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    """after the module: the worst error / B of every path, the largest error of every output and the positions excused under (P5) (shown
    with -s)"""
    yield
    for k in sorted(WORST):
        print("DECODECELL worst %-3s %.3f of B  %s" % (k, WORST[k][0], WORST[k][1]))
    for k in OUTPUTS:
        if k in LARGEST:
            print("DECODECELL largest %-6s %.2e (B %.2e)  %s" % ((k,) + LARGEST[k]))
    print("DECODECELL path positions excused under (P5), all cases: %d" % EXCUSED[0])


def host_model(name, n):
    return cells.host_model(name, n) if n <= 128 else wc.host_model(name, n)


def data(golden, n):
    return cells.cells_segs(golden) if n <= 256 else wc.small_segs(golden)


_REF = {}


def reference(oracle, golden, n, name):
    """dict(par, w, tables, ref (fastmodel.decode_oracle), eref (decode_reference_error), B {output: bound}, clear [per segment: the positions
    whose path (P5) holds]) of a case: computed once, only read afterwards; the last case is kept"""
    if (n, name) not in _REF:
        _REF.clear()
        par = host_model(name, n)
        segs = data(golden, n)
        w = fastmodel.decode_weights(n, MODELS[name](4)[2])
        tables = fastmodel.count_tables(segs)
        ref = fastmodel.decode_oracle(par[0], par[1], par[2], segs, oracle, w, tables)
        eref = fastmodel.decode_reference_error(par[0], par[1], par[2], segs, oracle, w=w, ref=ref)
        B = {k: fastmodel.cell_bound(eref[k]) for k in OUTPUTS}
        clear = [fastmodel.top_two_gap(p) > 2 * B["post"] for p in ref["post"]]
        _REF[(n, name)] = dict(par=par, w=w, tables=tables, ref=ref, eref=eref, B=B, clear=clear)
    return _REF[(n, name)]


class Outputs:
    """What one context returned: a digest per output and segment (for the bit comparisons) and the worst error of every gated output"""

    def __init__(self):
        self.sha = {}
        self.err = {k: (0.0, "-") for k in OUTPUTS}

    def keep(self, name, x):
        self.sha[name] = hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()

    def note(self, k, err, at):
        if err > self.err[k][0]:
            self.err[k] = (err, at)


def rel_gate(k, got, want, B, out, bad, what, at):
    """relative error of got over the entries of want above CELL_FLOOR under B[k]; finite and non-negative; failures go to bad"""
    got = np.asarray(got)
    if not (np.isfinite(got).all() and (got >= 0).all()):
        bad.append("%s: a non-finite or negative entry" % (what,))
    err, i = fastmodel.cell_error(got, want)
    out.note(k, err, "%s%s" % (at, list(i) if i is not None else ""))
    if not err <= B[k]:
        bad.append("%s: %.3e > B = %.3e at %s" % (what, err, B[k], list(i)))


def gate_post(post, want, B, out, bad, what, at):
    """(P1)"""
    rel_gate("post", post, want, B, out, bad, what + " (P1) post", at)
    small = want <= fastmodel.CELL_FLOOR
    if small.any() and not post[small].max() <= TINY_ENTRY:
        bad.append("%s (P1) an entry the oracle puts at or below 2^-900 is %.3e" % (what, post[small].max()))
    rows = float(np.abs(post.sum(1) - 1.0).max())
    if not rows <= B["post"]:
        bad.append("%s (P1) a row sums to 1 -+ %.3e > B = %.3e" % (what, rows, B["post"]))


def gate_recomb(rec, want, B, out, bad, what, at):
    """(P3)"""
    err = np.abs(rec - want)
    i = int(np.argmax(err)) if np.isfinite(err).all() else int(np.argmax(~np.isfinite(err)))
    out.note("recomb", float(err[i]), "%s[%d]" % (at, i))
    if not (err[i] <= B["recomb"] and rec.min() >= -B["recomb"] and rec.max() <= 1.0 + B["recomb"]):
        bad.append("%s (P3) recomb: %.3e > B = %.3e at %d, or outside [0, 1] (%.17g .. %.17g)" % (what, err[i], B["recomb"], i, rec.min(), rec.max()))
    if not rec[-1] == 0.0:
        bad.append("%s (P3) recomb at position L is %.3e" % (what, rec[-1]))


def decode_all(es, segs, R, out, bad, what):
    """every call on every segment of a fast context, gated against the oracle's outputs of R; the number of path positions (P5) excuses"""
    ref, B, w, tables = R["ref"], R["B"], R["w"], R["tables"]
    n = es.n
    cnt = {j: np.zeros((n, j)) for j in tables}
    excused = 0
    for s, seg in enumerate(segs):
        L, at, ws = len(seg), "seg %d " % s, "%s segment %d" % (what, s)
        post, rec = es.posterior(s)
        post1, _ = es.posterior(s, want_recomb=False)
        _, rec1 = es.posterior(s, want_post=False)
        assert post.shape == (L, n) and post1.shape == (L, n) and rec.shape == (L,) and rec1.shape == (L,)
        gate_post(post, ref["post"][s], B, out, bad, ws + " rows + recomb", at)
        gate_recomb(rec, ref["recomb"][s], B, out, bad, ws + " rows + recomb", at)
        if not bits_equal(post1, post):
            gate_post(post1, ref["post"][s], B, out, bad, ws + " rows alone", at)
        if not bits_equal(rec1, rec):
            gate_recomb(rec1, ref["recomb"][s], B, out, bad, ws + " recomb alone", at)
        path, maxp = es.decode(s)
        rel_gate("maxp", maxp, ref["maxp"][s], B, out, bad, ws + " (P2) maxp", at)
        clear = R["clear"][s]
        excused += int((~clear).sum())
        if not np.array_equal(path[clear], ref["path"][s][clear]):
            d = np.nonzero((path != ref["path"][s]) & clear)[0]
            bad.append("%s (P5) path differs at %d clear positions, the first %s: %s, oracle %s" % (ws, len(d), d[:5], path[d[:5]], ref["path"][s][d[:5]]))
        sc = es.scales(s)
        rel_gate("scales", sc, ref["scales"][s], B, out, bad, ws + " (P4) scales", at)
        for j in tables:
            es.post_counts(s, tables[j][s], cnt[j])
            own = es.post_counts(s, tables[j][s], np.zeros((n, j)))      # the segment alone: no long segment hides a short one
            rel_gate("counts", own, ref["counts_seg"][j][s], B, out, bad, "%s (P6) post_counts, %d columns" % (ws, j), "%s%d columns " % (at, j))
            if own[ref["counts_seg"][j][s] == 0.0].any():
                bad.append("%s (P6) post_counts, %d columns: a cell the oracle leaves at 0 is not" % (ws, j))
            out.keep("counts %d of segment %d" % (j, s), own)
        m4 = es.post_mean(s, w)
        m1 = es.post_mean(s, w[0])
        assert m4.shape == (L, 4) and m1.shape == (L, 1)
        rel_gate("mean", m4, ref["mean"][s], B, out, bad, ws + " (P6) post_mean, four columns", at)
        rel_gate("mean", m1, ref["mean"][s][:, :1], B, out, bad, ws + " (P6) post_mean, one column", at)
        ones = float(np.abs(m4[:, 3] - 1.0).max())
        if not ones <= B["mean"]:
            bad.append("%s (P6) the all-ones column is 1 -+ %.3e > B = %.3e" % (ws, ones, B["mean"]))
        own, _ = fastmodel.cell_error(m4, fastmodel.long_mean(post, w))
        if not own <= B["mean"]:
            bad.append("%s (P7) post_mean is %.3e > B = %.3e from its own rows" % (ws, own, B["mean"]))
        for k, v in (("post+", post), ("rec+", rec), ("post", post1), ("rec", rec1), ("path", path), ("maxp", maxp), ("scales", sc), ("mean4", m4),
                     ("mean1", m1)):
            out.keep("%s of segment %d" % (k, s), v)
    for j in tables:
        rel_gate("counts", cnt[j], ref["counts"][j], B, out, bad, "%s (P6) post_counts, %d columns, running totals" % (what, j), "totals, %d columns " % j)
        out.keep("counts %d" % j, cnt[j])
    return excused


def same_result(r, w):
    return all(bits_equal(r[k], w[k]) for k in ("A", "sums", "E") if k in w) and r["LL"] == w["LL"]


def run_path(hip, segs, R, n, chunk, tag, entry, opts, want_struct, want_bh, want_iv, what):
    """One context: the E-step, every decoding call, the E-step again.  (Outputs, the gates it missed, positions excused)"""
    a, e, a0 = R["par"]
    T = chunk or DEFAULT_TILE
    es = hip.HipEStep(n, mode=hip.MODE_FAST, warmup=WARMUP, **(dict(chunk=chunk) if chunk else {}), **opts)
    es.load_segments(segs)
    out, bad = Outputs(), []

    def regime():
        d = ran_wide(es) if n > 128 else es.fast_diag()
        assert d["fwd_rounds"] == 0 and d["bwd_rounds"] == 0 and d["fwd_tiles"] == 0 and d["bwd_tiles"] == 0, (what, d)
        assert d["n_chunks"] == sum((len(s) + T - 1) // T for s in segs) and d["tile_len"] == T and d["warmup"] == WARMUP, (what, d)
        assert d["structured"] == want_struct and d["back_half"] == want_bh, (what, d)
        assert es.wide_table_info()["interval"] == want_iv, (what, es.wide_table_info())

    try:
        r = getattr(es, entry)(a, e, a0)
        regime()
        excused = decode_all(es, segs, R, out, bad, what)
        r2 = getattr(es, entry)(a, e, a0)              # (P8)
        regime()
        if not same_result(r2, r):
            bad.append("%s (P8) the E-step after the decoding calls differs from the one before" % (what,))
    finally:
        es.close()
    path = os.environ.get("PSMC_DECODE_CELLS_BITS")
    if path:
        h = hashlib.sha1("".join(out.sha[k] for k in sorted(out.sha)).encode()).hexdigest()
        with open(path, "a") as f:
            f.write("%s %s\n" % (what, h))
    return out, bad, excused


def run_exact(hip, segs, R, n, bad, what):
    """(P7) D0: an exact context at the same parameters returns the oracle's bits"""
    ref, tables = R["ref"], R["tables"]
    es = hip.HipEStep(n, mode=hip.MODE_EXACT)
    es.load_segments(segs)
    cnt = {j: np.zeros((n, j)) for j in tables}
    try:
        es.estep(*R["par"])
        for s in range(len(segs)):
            post, rec = es.posterior(s)
            post1, _ = es.posterior(s, want_recomb=False)
            _, rec1 = es.posterior(s, want_post=False)
            path, maxp = es.decode(s)
            got = dict(post=post, recomb=rec, maxp=maxp, scales=es.scales(s))
            for k, v in list(got.items()) + [("post", post1), ("recomb", rec1)]:
                if not bits_equal(v, ref[k][s]):
                    bad.append("%s (P7) %s of segment %d is not the oracle's bits" % (what, k, s))
            if not np.array_equal(path, ref["path"][s]):
                bad.append("%s (P7) path of segment %d is not the oracle's" % (what, s))
            for j in tables:
                es.post_counts(s, tables[j][s], cnt[j])
                if not bits_equal(es.post_counts(s, tables[j][s], np.zeros((n, j))), ref["counts_seg"][j][s]):
                    bad.append("%s (P7) post_counts of segment %d with %d columns is not the oracle's bits" % (what, s, j))
    finally:
        es.close()
    for j in tables:
        if not bits_equal(cnt[j], ref["counts"][j]):
            bad.append("%s (P7) the running totals of post_counts with %d columns are not the oracle's bits" % (what, j))


def report(n, name, tag, outs, R, note=""):
    """one DECODECELL line: the worst error / B over the outputs and tilings of a path"""
    B, eref = R["B"], R["eref"]
    ratio, k, chunk = max((o.err[k][0] / B[k], k, c) for c, o in outs.items() for k in OUTPUTS)
    w = outs[chunk].err[k]
    print("DECODECELL n %4d %-26s %-3s%s worst %-6s %.2e of B %.2e ratio %.3f at %s chunk %d; E_ref %.2e; ratios %s" % (
        n, name, tag, note, k, w[0], B[k], ratio, w[1], chunk, eref[k],
        " ".join("%s %.3f" % (x, max(o.err[x][0] for o in outs.values()) / B[x]) for x in OUTPUTS)))
    if ratio > WORST.get(tag, (0.0, ""))[0]:
        WORST[tag] = (ratio, "n %d %s %s %s chunk %d" % (n, name, k, w[1], chunk))
    for x in OUTPUTS:
        err, c = max((o.err[x][0], c) for c, o in outs.items())
        if err > LARGEST.get(x, (0.0,))[0]:
            LARGEST[x] = (err, B[x], "n %d %s %s %s chunk %d" % (n, name, tag, outs[c].err[x][1], c))


@pytest.mark.parametrize("n,name", CASES, ids=["%d-%s" % c for c in CASES])
def test_decode_cells(hip, golden, oracle, n, name):
    segs = data(golden, n)
    R = reference(oracle, golden, n, name)
    total = sum(len(s) for s in segs)
    assert cells.is_hmm(R["par"]) and max(len(s) for s in segs) <= WARMUP
    # (P5)'s condition on the input, from the oracle alone
    unclear = sum(int((~c).sum()) for c in R["clear"])
    assert unclear <= MAX_EXCUSED * total and (unclear == 0 or R["eref"]["gap"] <= 1e-9), (unclear, total, R["eref"]["gap"])
    assert R["eref"]["ties"] == 0 or unclear > 0, R["eref"]
    refused = (n, name) in cells.STRUCT_REFUSED
    failures, res = [], {}
    for tag, entry, opts, tilings, want_struct, bh, iv in paths(n, refused):
        outs = {}
        for chunk in tilings:
            what = "n %d %s %s chunk %d" % (n, name, tag, chunk)
            outs[chunk], bad, excused = run_path(hip, segs, R, n, chunk, tag, entry, opts, want_struct, bh, iv, what)
            assert excused == unclear
            failures += bad
        res[tag] = outs
        report(n, name, tag, outs, R, " (dense sweeps: refused)" if refused and tag == "D1" else "")
    EXCUSED[0] += unclear
    if n > 128:                                        # (P7): the checkpointed decoding returns the bits of the full table
        for chunk in FEW:
            x, y = res["D4"][chunk].sha, res["D3"][chunk].sha
            assert sorted(x) == sorted(y)
            diff = [k for k in sorted(x) if x[k] != y[k]]
            if diff:
                failures.append("n %d %s (P7) D4 and D3 differ at chunk %d on %d outputs, the first: %s" % (n, name, chunk, len(diff), diff[:4]))
    if (n, name) in D0_CASES:
        run_exact(hip, segs, R, n, failures, "n %d %s D0" % (n, name))
    assert not failures, "\n".join(failures[:40] + (["... %d more" % (len(failures) - 40)] if len(failures) > 40 else []))
