"""psmc_hip_viterbi and psmc_hip_sample_paths where tests/test_gpu_viterbi.py and tests/test_gpu_sample.py do not look: both are
pinned bit for bit on every context, and both had run on one mild family only (banded_hmm: entries 1e-3 .. 0.6).  Every comparison
here is equality of int32 paths or of float64 bit patterns; the expected values are the reference's own hmm_Viterbi
(tests/golden/viterbi_extremes.npz) and the numpy restatements (tests/viterbi_model.py, tests/sample_model.py); every condition that
keeps a case from passing by accident -- a path that moves, a clamp that is taken, a subnormal term, a leading zero weight, more
segments than k_vit_compose has threads in eight blocks -- is asserted on the reference before the device is asked.

  B1  Viterbi against the real hmm_Viterbi at the thirteen extreme PSMC models (tests/test_gpu_wide_fast_edges.py MODELS) at 64, 65
      and 200 states: the 33 cases with a path, both modes, default tile and vit_tile = 16, with and without the path.
  B2  Viterbi and sampling at every kernel flavour -- 3 / 63 / 64, 65 / 128, 130 / 192 states (matrix or column in registers),
      200 / 256 (streamed, one byte per entry), 300 / 514 (two bytes) -- under rho_1e-6, lambda_ramp_down_1e2_1e-2 (entries down to
      1e-232), rho_0.5 (negative entries: NaN logs beside finite ones), lambda_alt_1e-3_1e3 (NaN and exact zeros in a) and
      lambda_equal, on segments of 1, 2, 63, 64, 65 and 700 bins, all-missing ones of 3 and 70 bins and one that begins and ends in
      missing bins (1000 bins in all).  Where the restatement finds no path the call must answer PSMC_HIP_EINVAL and name the first
      such segment in load order; the context must then serve a good model.  Under the NaN-bearing model every drawn state is 0.
      The sampler's longest segment is 6000 bins where 700 do not move the reference four times (rho_1e-6 at every size, and every
      model at 3 states).
  B3  Sampling under all thirteen models at 64, 65 and 200 states on the 6000-bin slice and segments_small.npz (32 051 bins).
  B4  The draws the header pins and a real model never reaches, on synthetic matrices at 5 .. 300 states: a count of n clamped to
      n - 1 (row 0 negative on the odd columns), running sums of subnormal products (entries off a band scaled by 1e-300), a
      leading run of zero weights (block diagonal, a0 on the upper half).  The same matrices go through Viterbi.
  B5  2000 segments (lengths 1 .. 40 and five of 300 .. 700 bins, 43 k bins): k_vit_compose's blocks past the first, end_state's
      [sample][segment] layout, the longest-first sort with at least 1955 tied segments, thousands of one-tile segments.
  B6  Viterbi's error path at 23, 100, 150, 200 and 300 states: e[1] = 0 with het bins in the 2nd and 5th of six segments names
      segment 1, with and without the path; a state without a predecessor (an all-zero column of a) is an error and the same
      model with the column restored is none, so the padded states raise nothing.

Observed on the MI355X (profiles/path_extremes_tests.txt): 255 passed in 149 s, nearly all of it the restatements on the CPU -- B3
80 s (4.4 s per case at 200 states), B2 30 s, B5 27 s (2000 segments at 300 states: 12.5 s for the sampler's two id arrays, 4.2 s
for Viterbi), B1, B4 and B6 together 11 s.  Every case passed on the first device run: the gates found nothing to change.
Counted on the restatement, not on the device: B4's clamps (181 .. 519 of 1800 draws; the factor is -40 below 100 states and -400
beyond, -40 clamps nothing from 128 states on), subnormal terms (2468 .. 54 180 from 64 states on) and leading zeros (1800 of 1800);
B2's runs of sample 0 (4 .. 294; rho_1e-6 has one run on 700 bins and four on 6000); B5's 1955 tied segments and 788 .. 807 one-tile
segments at vit_tile = 16."""
import ctypes as C
import os
import re
import numpy as np
import pytest

import path_extremes as px
import sample_model as sm
import viterbi_model as vm
from test_gpu_sample import check as sample_check
from test_gpu_viterbi import banded_hmm, block_data, check, ctx, same_bits
from test_viterbi_model import extreme_cases, extreme_golden
from conftest import GOLD

pytestmark = pytest.mark.gpu

SEED = 20261021
EINVAL = -1
FLAVOUR_SIZES = [3, 63, 64, 65, 128, 130, 192, 200, 256, 300, 514]
HARSH_MODELS = ["rho_1e-6", "lambda_ramp_down_1e2_1e-2", "rho_0.5", "lambda_alt_1e-3_1e3", "lambda_equal"]
DRAW_SIZES = [5, 64, 65, 128, 130, 192, 200, 300]
MANY_SIZES = [23, 200, 300]
ERROR_SIZES = [23, 100, 150, 200, 300]


def mode_of(i):
    """the mode alternates by case: both modes run the same kernels, and the bits must not know the difference"""
    from psmc_amd import hip
    return hip.MODE_FAST if i % 2 else hip.MODE_EXACT


def raw_viterbi(h, par, want_path):
    """(return code, message) of the C call itself"""
    a, e, a0 = h._params(*par)
    path, score = np.zeros(int(np.sum(h.lens)), dtype=np.int32), np.zeros(len(h.lens))
    h.lib.psmc_hip_viterbi.argtypes = [C.c_void_p] * 6
    rc = h.lib.psmc_hip_viterbi(h.h, a.ctypes.data, e.ctypes.data, a0.ctypes.data, path.ctypes.data if want_path else None, score.ctypes.data)
    return rc, h.lib.psmc_hip_last_error(h.h).decode()


def viterbi_gate(h, par, ref, what):
    """ref = px.viterbi_reference(par, the loaded segments): its paths and score bits, with and without the path -- or EINVAL naming
    the first segment without a path, with and without the path"""
    if isinstance(ref, int):
        for want_path in (True, False):
            rc, msg = raw_viterbi(h, par, want_path)
            named = re.search(r"segment (\d+) has no path of finite probability", msg)
            assert rc == EINVAL and named and int(named.group(1)) == ref, (what, want_path, rc, msg, ref)
        return
    paths, scores = h.viterbi(*par)
    check(paths, scores, ref[0], ref[1], what)
    none, scores = h.viterbi(*par, want_path=False)
    assert none is None and same_bits(scores, ref[1]), (what, "scores without a path")


def freeze(*arrays):
    for x in arrays:
        x.setflags(write=False)


# ---------------------------------------------------------------- B1. the reference's own bits at the model extremes
_GOLD_X = {}


def gold_x():
    if not _GOLD_X:
        z = np.load(os.path.join(GOLD, "viterbi_extremes.npz"))
        segs = px.golden_segments()
        _GOLD_X.update(segs=segs, cases={c: extreme_golden(z, c, segs) for c, _, _ in extreme_cases()})
    return _GOLD_X


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case,n,name", extreme_cases())
def test_viterbi_extreme_goldens(case, n, name, mode):
    g = gold_x()
    segs = list(g["segs"].values())
    longest = int(np.argmax([len(s) for s in segs]))
    n_runs = {c.split(".", 1)[1]: len(vm.runs(g["cases"][c][0][longest])) for c, m, _ in extreme_cases() if m == n}
    assert len(n_runs) == 11 and sum(r >= 4 for r in n_runs.values()) >= 8, n_runs       # the goldens alone: paths, not constants
    assert all(r >= 2 for k, r in n_runs.items() if k != "tmax_0.5"), n_runs
    want_paths, want_scores = g["cases"][case]
    want_paths = [p.astype(np.int32) for p in want_paths]
    par = px.extreme_model(name, n)
    h = ctx(n, mode_of(mode), segs)
    for tile in (None, 16):
        if tile is not None:
            h.set_option("vit_tile", tile)
        paths, scores = h.viterbi(*par)
        check(paths, scores, want_paths, want_scores, (case, mode, tile))
    none, scores = h.viterbi(*par, want_path=False)
    assert none is None and same_bits(scores, want_scores), (case, mode, "scores without a path")


# ---------------------------------------------------------------- B2. every kernel flavour at the harsh models
_HARSH = {}


def harsh_viterbi(golden, n, name):
    """(par, segments, px.viterbi_reference) on the short segments: computed once, shared, never changed"""
    key = ("vit", n, name)
    if key not in _HARSH:
        par, segs = px.extreme_model(name, n), px.short_segs(golden)
        _HARSH[key] = (par, segs, px.viterbi_reference(par, segs))
    return _HARSH[key]


def long_bins(n, name):
    """bins of the sampler's longest segment: 700, or the 6000 at which the reference's sample 0 has four runs (tried on the CPU)"""
    return 6000 if n == 3 or name == "rho_1e-6" else 700


@pytest.mark.parametrize("name", HARSH_MODELS)
@pytest.mark.parametrize("n", FLAVOUR_SIZES)
def test_viterbi_flavours_at_harsh_models(golden, n, name):
    par, segs, ref = harsh_viterbi(golden, n, name)
    assert sum(len(s) for s in segs) == 1000 and (segs[1] == 2).all() and (segs[6] == 2).all() and (segs[7][:6] == 2).all() and (segs[7][-6:] == 2).all()
    if name == "lambda_alt_1e-3_1e3":
        assert ref == 1 and np.isnan(par[0]).any() and (par[0] == 0).any()   # segment 0 has one bin; segment 1, all missing, has three
    else:
        assert not isinstance(ref, int)
    if name == "rho_0.5":
        assert (par[0] < 0).any()
    h = ctx(n, mode_of(FLAVOUR_SIZES.index(n) + HARSH_MODELS.index(name)), segs)
    for tile in (None, 16):
        if tile is not None:
            h.set_option("vit_tile", tile)
        viterbi_gate(h, par, ref, (n, name, tile))
    if isinstance(ref, int):   # the context after the error: a good model's bits
        good, _, good_ref = harsh_viterbi(golden, n, "lambda_equal")
        viterbi_gate(h, good, good_ref, (n, "lambda_equal after", name))


@pytest.mark.parametrize("name", HARSH_MODELS)
@pytest.mark.parametrize("n", FLAVOUR_SIZES)
def test_sampling_flavours_at_harsh_models(golden, n, name):
    par = px.extreme_model(name, n)
    segs = px.short_segs(golden, long_bins(n, name))
    ref = sm.sample_segments(par[0], par[1], par[2], segs, SEED, 3)
    if name in px.NAN_MODELS:
        assert np.isnan(par[0]).any() and not any(p.any() for row in ref for p in row)   # a total of NaN: state 0, everywhere
    else:
        assert len(sm.runs(ref[0][-1])) >= 4 and not np.array_equal(ref[0][-1], ref[1][-1]), len(sm.runs(ref[0][-1]))
    h = ctx(n, mode_of(FLAVOUR_SIZES.index(n) + HARSH_MODELS.index(name) + 1), segs)
    for group in (0, 2):
        h.set_option("samp_group", group)
        sample_check(h.sample_paths(par[0], par[1], par[2], SEED, 3), ref, (n, name, group))


# ---------------------------------------------------------------- B3. the full model table for sampling
@pytest.mark.parametrize("name", px.model_names())
@pytest.mark.parametrize("n", px.GOLDEN_SIZES)
def test_sampling_model_table(golden, n, name):
    par = px.extreme_model(name, n)
    segs = golden.segs_small + [golden.segs_mid[3][:6000]]
    longest = int(np.argmax([len(s) for s in segs]))
    assert sum(len(s) for s in segs) == 32051 and len(segs[longest]) == 20000
    ref = sm.sample_segments(par[0], par[1], par[2], segs, SEED, 2)
    if name in px.NAN_MODELS:
        assert np.isnan(par[0]).any() and not any(p.any() for row in ref for p in row)
    else:
        assert len(sm.runs(ref[0][longest])) >= 4 and len(sm.runs(ref[0][-1])) >= 4, (len(sm.runs(ref[0][longest])), len(sm.runs(ref[0][-1])))
    h = ctx(n, mode_of(px.GOLDEN_SIZES.index(n) + px.model_names().index(name)), segs)
    sample_check(h.sample_paths(par[0], par[1], par[2], SEED, 2), ref, (n, name))


# ---------------------------------------------------------------- B4. the degenerate draws
DRAW_KINDS = ["clamp", "subnormal", "leading_zero"]


def clamp_factor(n):
    """row 0 has to outweigh the n - 1 other weights of a draw: chosen per size on the CPU (-40 clamps nothing from 128 states on)"""
    return 40.0 if n < 100 else 400.0


def draw_hmm(kind, n):
    rng = np.random.default_rng(5000 + n)
    return px.clamp_hmm(n, clamp_factor(n), rng) if kind == "clamp" else px.subnormal_hmm(n, rng) if kind == "subnormal" else px.upper_half_hmm(n, rng)


@pytest.mark.parametrize("kind", DRAW_KINDS)
@pytest.mark.parametrize("n", DRAW_SIZES)
def test_degenerate_draws(n, kind):
    rng = np.random.default_rng(4000 + n)
    segs = [block_data(L, rng) for L in (1, 65, 600)]
    par = draw_hmm(kind, n)
    a, e, a0 = par
    ref = sm.sample_segments(a, e, a0, segs, SEED, 3)
    cond = [px.draw_conditions(a, e, a0, segs[2], SEED, j, 2, ref[j][2]) for j in range(3)]
    count = sum(c[kind] for c in cond)
    print("DRAWS n %3d %-12s over 3 x 600 draws: clamps %d, subnormal terms %d, draws past leading zeros %d; runs of sample 0: %d"
          % (n, kind, sum(c["clamp"] for c in cond), sum(c["subnormal"] for c in cond), sum(c["leading_zero"] for c in cond), len(sm.runs(ref[0][2]))))
    if kind == "clamp":
        assert count >= 10 and (a[0, 1::2] < 0).all()
    elif kind == "subnormal":
        assert count >= 100 or n < 64
    else:
        assert count == 3 * 600 and min(p.min() for row in ref for p in row) >= n // 2   # every draw; no state of the lower half
    assert len(sm.runs(ref[0][2])) >= 4 or (kind == "subnormal" and n < 64)               # ... and the reference moves
    vref = px.viterbi_reference(par, segs)
    if kind == "leading_zero":
        assert vref == 1   # log a0 = -inf on the lower half, log a = -inf between the halves: a lower state has no predecessor at position 2
    elif kind == "clamp":
        assert not isinstance(vref, int) and len(vm.runs(vref[0][2])) >= 4                # NaN logs in row 0 beside finite ones
    h = ctx(n, mode_of(DRAW_SIZES.index(n) + DRAW_KINDS.index(kind)), segs, vit_tile=64)
    for group in (0, 2):
        h.set_option("samp_group", group)
        sample_check(h.sample_paths(a, e, a0, SEED, 3), ref, (n, kind, group))
    viterbi_gate(h, par, vref, (n, kind))


# ---------------------------------------------------------------- B5. many segments
_MANY = {}


def many_segments(n):
    """(a, e, a0, 2000 segments) with banded_hmm: lengths 1 .. 40, five of 300 .. 700 bins scattered among them"""
    if n not in _MANY:
        rng = np.random.default_rng(6000 + n)
        a, e, a0 = banded_hmm(n, rng)
        lens = rng.integers(1, 41, size=2000)
        lens[rng.choice(2000, size=5, replace=False)] = rng.integers(300, 701, size=5)
        segs = [block_data(int(L), rng) for L in lens]
        freeze(a, e, a0, *segs)
        _MANY[n] = (a, e, a0, segs)
    return _MANY[n]


def assert_many(segs):
    lens = [len(s) for s in segs]
    assert len(segs) == 2000 > 64 * 8 and sum(L >= 300 for L in lens) == 5 and sum(L > 40 for L in lens) == 5
    assert np.diff([i for i, L in enumerate(lens) if L >= 300]).min() > 1   # scattered: short segments between any two long ones
    # at most 40 + 5 distinct lengths: at least 1955 segments tie with an earlier one, so the stable sort's order among equals is used
    assert len(segs) - len(set(lens)) >= 1955
    assert sum(L <= 16 for L in lens) >= 500   # one-tile segments even at vit_tile = 16: 2000 x 16 / 40 expected


@pytest.mark.parametrize("n", MANY_SIZES)
def test_viterbi_many_segments(n):
    a, e, a0, segs = many_segments(n)
    assert_many(segs)
    ref = px.viterbi_reference((a, e, a0), segs)
    assert not isinstance(ref, int) and sum(len(vm.runs(p)) >= 2 for p in ref[0]) >= 5
    h = ctx(n, mode_of(n), segs)
    for tile in (None, 16):
        if tile is not None:
            h.set_option("vit_tile", tile)
        viterbi_gate(h, (a, e, a0), ref, (n, tile))


@pytest.mark.parametrize("n", MANY_SIZES)
def test_sampling_many_segments(n):
    a, e, a0, segs = many_segments(n)
    assert_many(segs)
    fs = [sm.forward(a, e, a0, s) for s in segs]   # the restatement's forward vectors once, its walk per id array

    def reference(ids):
        return [[sm.walk(a, f, sm.uniforms(SEED, j, int(q), len(s))) for f, s, q in zip(fs, segs, ids)] for j in range(3)]
    plain_ids = np.arange(2000, dtype=np.uint64)
    mixed_ids = np.random.default_rng(n).permutation(2000).astype(np.uint64)
    plain, mixed = reference(plain_ids), reference(mixed_ids)
    long5 = [i for i, s in enumerate(segs) if len(s) >= 300]
    assert all(len(sm.runs(plain[0][i])) >= 4 for i in long5) and any(not np.array_equal(plain[0][i], mixed[0][i]) for i in long5)
    assert len({int(p[-1]) for p in plain[2]}) >= 4   # the end states of the last sample differ between segments
    h = ctx(n, mode_of(n + 1), segs)
    for group, tile in ((0, None), (2, 16)):
        h.set_option("samp_group", group)
        if tile is not None:
            h.set_option("vit_tile", tile)
        sample_check(h.sample_paths(a, e, a0, SEED, 3), plain, (n, group, "default ids"))
        sample_check(h.sample_paths(a, e, a0, SEED, 3, stream=mixed_ids), mixed, (n, group, "permuted ids"))


# ---------------------------------------------------------------- B6. Viterbi's error path at every flavour
def error_segs(rng):
    """six segments; the 2nd and the 5th hold a het bin followed by another bin, the others no het bin at all"""
    segs = [block_data(L, rng) for L in (40, 90, 1, 300, 70, 33)]
    for s in segs:
        s[s == 1] = 0
    segs[1][[17, 60]] = 1
    segs[1][[18, 61]] = (0, 2)
    segs[4][5] = 1
    segs[4][6] = 0
    assert [bool((s[:-1] == 1).any()) for s in segs] == [False, True, False, False, True, False] and all(s[-1] != 1 for s in segs)
    return segs


@pytest.mark.parametrize("n", ERROR_SIZES)
def test_viterbi_error_names_the_first_segment(n):
    rng = np.random.default_rng(7700 + n)
    a, e, a0 = banded_hmm(n, rng)
    segs = error_segs(rng)
    e_bad = e.copy()
    e_bad[1] = 0.0
    bad, good = (a, e_bad, a0), (a, e, a0)
    assert px.viterbi_reference(bad, segs) == 1 and px.viterbi_reference(bad, segs[2:]) == 2   # segments 1 and 4 fail, no other
    good_ref = px.viterbi_reference(good, segs)
    assert not isinstance(good_ref, int)
    h = ctx(n, mode_of(n), segs)
    for tile in (None, 16):
        if tile is not None:
            h.set_option("vit_tile", tile)
        viterbi_gate(h, bad, 1, (n, tile, "e[1] = 0"))
        viterbi_gate(h, good, good_ref, (n, tile, "afterwards"))


@pytest.mark.parametrize("n", ERROR_SIZES)
def test_viterbi_state_without_predecessor(n):
    """state n - 1 with an all-zero column of a has no predecessor: an error; with the column back it has one, and the padded
    states n .. -- whose columns of la hold -inf in the same way -- must not raise anything"""
    rng = np.random.default_rng(7800 + n)
    a, e, a0 = banded_hmm(n, rng)
    segs = [block_data(L, rng) for L in (1, 2, 130, 64)]
    a_bad = a.copy()
    a_bad[:, n - 1] = 0.0
    bad, good = (a_bad, e, a0), (a, e, a0)
    assert px.viterbi_reference(bad, segs) == 1   # the first segment has one bin: no transition
    good_ref = px.viterbi_reference(good, segs)
    assert not isinstance(good_ref, int)
    h = ctx(n, mode_of(n + 1), segs)
    viterbi_gate(h, good, good_ref, (n, "every state has a predecessor"))
    viterbi_gate(h, bad, 1, (n, "column n - 1 is zero"))
    viterbi_gate(h, good, good_ref, (n, "afterwards"))
