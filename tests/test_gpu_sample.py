"""psmc_hip_sample_paths on the device against the numpy restatement of the pinned definition (tests/sample_model.py), entry for
entry: at every width the sweep treats differently -- 64 / 128 / 192 padded states with the column in registers, the streamed
kernel beyond, one or two bytes per map entry -- across backtrace tile boundaries, with every grouping of the samples, with stream
ids, in both modes, and without touching anything else of the context."""
import ctypes as C
import numpy as np
import pytest

import sample_model as sm
from test_gpu_viterbi import DEFAULT_TILE, TILES, banded_hmm, block_data, ctx, seg_lengths

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 23, 63, 64, 65, 127, 128, 129, 192, 193, 224, 225, 256, 257, 512, 513, 1024]
SEED = 20261020
N_SAMP = 3

_CASES = {}


def case(n):
    """(a, e, a0, segments, reference paths [j][i]) of width n: computed once, shared, never changed"""
    if n not in _CASES:
        rng = np.random.default_rng(9000 + n)
        a, e, a0 = banded_hmm(n, rng)
        segs = [block_data(L, rng) for L in seg_lengths(n)]
        ref = sm.sample_segments(a, e, a0, segs, SEED, N_SAMP)
        for x in (a, e, a0, *segs, *(p for row in ref for p in row)):
            x.setflags(write=False)
        _CASES[n] = (a, e, a0, segs, ref)
    return _CASES[n]


def check(got, ref, what):
    assert len(got) == len(ref), what
    for j, (gj, rj) in enumerate(zip(got, ref)):
        assert len(gj) == len(rj), what
        for i, (p, r) in enumerate(zip(gj, rj)):
            assert p.dtype == np.int32 and p.shape == r.shape, (what, j, i)
            assert np.array_equal(p, r), (what, "sample", j, "segment", i, "first difference at", int(np.flatnonzero(p != r)[0]))


# ---- (a) every width and tile length
@pytest.mark.parametrize("n", WIDTHS)
def test_against_restatement(n):
    from psmc_amd import hip
    a, e, a0, segs, ref = case(n)
    assert [len(s) for s in segs] == seg_lengths(n) and max(len(s) for s in segs) == (4097 if n <= 128 else 600)
    assert (np.concatenate(segs) == 2).any()
    longest = int(np.argmax([len(s) for s in segs]))
    if n >= 2:  # a constant output cannot pass: the reference samples move, and differ from each other
        for j in range(N_SAMP):
            p = ref[j][longest]
            assert len(sm.runs(p)) >= 4 and len(set(p.tolist())) >= min(n, 4), (j, len(sm.runs(p)), set(p.tolist()))
        assert not np.array_equal(ref[0][longest], ref[1][longest])
    h = ctx(n, hip.MODE_FAST if n % 2 else hip.MODE_EXACT, segs)
    for tile in TILES:
        if tile is not None:
            h.set_option("vit_tile", tile)
        check(h.sample_paths(a, e, a0, SEED, N_SAMP), ref, (n, tile))


# ---- (b) the grouping of the samples and the tile length change nothing
@pytest.mark.parametrize("n", [23, 128, 200, 513])
def test_groups_and_tiles_give_the_same_bits(n):
    from psmc_amd import hip
    a, e, a0, segs, ref = case(n)
    segs = segs[-4:]
    ref7 = sm.sample_segments(a, e, a0, segs, 5, 7)
    h = ctx(n, hip.MODE_EXACT, segs)
    for group, tile in ((0, DEFAULT_TILE), (1, DEFAULT_TILE), (3, 16), (64, 64), (2, 100)):  # 7 samples: groups of 3 cut unevenly
        h.set_option("samp_group", group)
        h.set_option("vit_tile", tile)
        check(h.sample_paths(a, e, a0, 5, 7), ref7, (n, group, tile))
    # sample j does not depend on n_samp
    h.set_option("samp_group", 0)
    check(h.sample_paths(a, e, a0, 5, 2), ref7[:2], (n, "two of seven"))


def test_sixty_four_samples_in_one_group():
    from psmc_amd import hip
    a, e, a0, segs, _ = case(65)
    segs = [segs[3], segs[9]]
    ref = sm.sample_segments(a, e, a0, segs, 3, 64)
    h = ctx(65, hip.MODE_EXACT, segs, samp_group=64, vit_tile=16)
    check(h.sample_paths(a, e, a0, 3, 64), ref, "64 in one group")
    assert len({r[1].tobytes() for r in ref}) == 64


# ---- (c) the call reads the observations only; both modes draw the same samples
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_leaves_the_context_alone(golden, mode):
    from psmc_amd import hip
    p = golden.params("n64_curve")
    q = golden.params("n64_flat")
    a, e, a0 = p["a"], p["e"], p["a0"]
    segs = golden.segs_small
    opts = dict(fuse=0) if mode == "fast" else {}

    def run(with_sampling):
        h = ctx(64, hip.MODE_FAST if mode == "fast" else hip.MODE_EXACT, segs, **opts)
        out = [h.estep(a, e, a0)]
        drawn = h.sample_paths(q["a"], q["e"], q["a0"], 17, 3) if with_sampling else None  # other parameters than the E-step's
        for seg in (8, 9):
            out.append(h.decode(seg))
            out.append(h.posterior(seg))
        out.append(h.estep(a, e, a0))
        return out, drawn

    def flat(x):
        if isinstance(x, dict):
            return [x[k] for k in sorted(x)]
        return list(x) if isinstance(x, (tuple, list)) else [x]

    (plain, _), (mixed, drawn) = run(False), run(True)
    for x, y in zip(plain, mixed):
        for u, v in zip(flat(x), flat(y)):
            u, v = np.asarray(u), np.asarray(v)
            assert u.shape == v.shape and u.tobytes() == v.tobytes()
    check(drawn, sm.sample_segments(q["a"], q["e"], q["a0"], segs, 17, 3), mode)


def test_both_modes_and_a_fresh_context_agree(golden):
    from psmc_amd import hip
    p = golden.params("n64_curve")
    a, e, a0 = p["a"], p["e"], p["a0"]
    segs = [s[:6000] for s in golden.segs_mid] + golden.segs_small[:9]
    base = None
    for mode in (hip.MODE_EXACT, hip.MODE_FAST):
        for estep_first in (False, True):
            h = ctx(64, mode, segs)
            if estep_first:
                h.estep(a, e, a0)
            got = h.sample_paths(a, e, a0, 99, 2)
            if base is None:
                base = got
                assert len(sm.runs(base[0][0])) >= 4
            check(got, base, (mode, estep_first))
    check([base[0][:1]], sm.sample_segments(a, e, a0, segs[:1], 99, 1), "the restatement, first segment")


# ---- (d) stream ids
def test_stream_ids():
    from psmc_amd import hip
    a, e, a0, segs, ref = case(23)
    segs = segs[:10]
    h = ctx(23, hip.MODE_EXACT, segs)
    ids = [5, 9, 2 ** 63 + 1, 0, 7, 7, 1, 2, 3, 2 ** 64 - 1]
    got = h.sample_paths(a, e, a0, SEED, 2, stream=ids)
    check(got, sm.sample_segments(a, e, a0, segs, SEED, 2, stream=ids), "ids")
    check(h.sample_paths(a, e, a0, SEED, 2, stream=np.arange(10)), [r[:10] for r in ref[:2]], "arange equals NULL")
    check(h.sample_paths(a, e, a0, SEED, 2), [r[:10] for r in ref[:2]], "NULL")


# ---- (e) a sharded input: per-shard calls with global ids equal the single context
def test_two_shards_with_global_ids():
    from psmc_amd import hip
    a, e, a0, segs, ref = case(65)
    segs = segs[:12]
    shards = ([0, 3, 4, 7, 8, 11], [1, 2, 5, 6, 9, 10])
    got = [[None] * 12 for _ in range(N_SAMP)]
    for idx in shards:
        h = ctx(65, hip.MODE_FAST, [segs[i] for i in idx])
        part = h.sample_paths(a, e, a0, SEED, N_SAMP, stream=idx)
        for j in range(N_SAMP):
            for i, p in zip(idx, part[j]):
                got[j][i] = p
    check(got, [r[:12] for r in ref], "shards")


# ---- (f) error returns
def test_error_returns(golden):
    from psmc_amd import hip
    p = golden.params("n23_curve")
    a, e, a0 = [np.ascontiguousarray(p[k], dtype=np.float64) for k in ("a", "e", "a0")]
    e = np.ascontiguousarray(e[:2])
    h = hip.HipEStep(23, mode=hip.MODE_EXACT)
    path = np.zeros(200, dtype=np.int32)

    def raw(a_, e_, a0_, n_samp, path_):  # the C call itself, NULLs allowed (HipEStep.sample_paths sets typed pointers: set ours every time)
        h.lib.psmc_hip_sample_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p]
        return h.lib.psmc_hip_sample_paths(h.h, *[x if x is None else x.ctypes.data for x in (a_, e_, a0_)], 1, n_samp, None,
                                           None if path_ is None else path_.ctypes.data)

    def last():
        return h.lib.psmc_hip_last_error(h.h).decode()
    assert raw(a, e, a0, 1, path) == -5                 # PSMC_HIP_ESTATE: no segments
    assert "no segments" in last()
    segs = [np.zeros(50, dtype=np.uint8), np.array([0, 0, 0, 1, 0, 2, 0], dtype=np.uint8), np.zeros(3, dtype=np.uint8)]
    h.load_segments(segs)
    assert raw(a, e, a0, 1, None) == -1 and "null path" in last()
    assert raw(None, e, a0, 1, path) == -1 and "null parameters" in last()
    assert raw(a, None, a0, 1, path) == -1 and raw(a, e, None, 1, path) == -1
    assert raw(a, e, a0, 0, path) == -1 and "n_samp" in last()
    assert raw(a, e, a0, -3, path) == -1
    for bad in (-1, 65, 2.5, 1e9):
        with pytest.raises(hip.HipError):
            h.set_option("samp_group", bad)
    # the context is usable afterwards
    check(h.sample_paths(a, e, a0, 1, 2), sm.sample_segments(a, e, a0, segs, 1, 2), "after the errors")


def test_table_that_does_not_fit_is_enomem():
    """one sample's table beyond any device's memory: 1024 states x 2 bytes x 200 M bins = 410 GB (the observations themselves are 200 MB)"""
    from psmc_amd import hip
    n = 1024
    a = np.full((n, n), 1.0 / n)
    e = np.vstack([np.full(n, 0.9), np.full(n, 0.1)])
    a0 = np.full(n, 1.0 / n)
    segs = [np.zeros(50_000_000, dtype=np.uint8)] * 4
    h = ctx(n, hip.MODE_EXACT, segs)
    with pytest.raises(hip.HipError, match=r"map table: 409\.6\d\d GB \(200000000 bins x 1024 states x 2\)"):
        h.sample_paths(a, e, a0, 1, 1)
