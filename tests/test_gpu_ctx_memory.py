"""What a context holds on the device comes back when it is closed: a net for leaked TABLES under the owning buffer type of
psmc_amd/csrc/psmc_hip_ctx.h (Buf, Scratch).

One cycle creates, uses and closes contexts over every owner of device memory: exact mode at 64 states (E-step, tables, decode,
post_counts, a second load_segments on the live context); fast mode at 64 and 128 states on 2e4 bins in tiles of 512 (E-step,
factored E-step, "prev_start" / "merge" / "adapt" once, the decoding calls with the unfused back half); the wide fast path at 200
states with "wide_decode", "wide_counts" and the gap / hom / mix chains on mix_sandwich of tests/wide_mix_model.py (a planted run of
N, a planted run of homozygosity, het-free mixes), then post_mean and post_quantile; a fast batch of three replicates (child
contexts); an exact batch of three with "exact_refwd" = 1; viterbi with a path and sample_paths with two samples at 200 states on
4e4 bins; load_segments_device over a torch tensor.  Device memory in use is total - free of hipMemGetInfo, asked of the runtime
the library is linked against.

Cycle 0 warms up code objects and the runtime's pools.  With U_k the memory in use after cycle k has closed everything, the test
asserts U_k - U_1 <= B for k = 2, 3, 4.  B was set from the same cycles run on the commit before the buffer type existed, whose
hand-written free lists are taken as leak-free: the largest U_k - U_1 seen there was 0 bytes, plus 2 MiB for one allocation
granule: B = 2097152 bytes (profiles/ctx_memory.txt).  Every table-class buffer of the cycle is at least twice that: f and b at 64
states 10.3 MB each, the wide X 15.2 MB, the back-pointer table and one sample map table 10.3 MB each.  A leaked small buffer (a
tile list, a parameter block) stays under B and is NOT caught here: the type is what guards those -- a buffer frees what it owns
when it is reset, allocated again or destroyed, and nothing in the host layer frees by hand."""
import os
import subprocess
import ctypes as C
import numpy as np
import pytest
from wide_mix_model import mix_sandwich

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRANULE = 2 << 20
PARENT_GROWTH = 0          # bytes: the largest U_k - U_1 (k = 2, 3, 4) of these cycles before the buffer type existed
B = PARENT_GROWTH + GRANULE
CYCLES = 5
ALL3 = dict(wide_gap_tiles=1, wide_hom_tiles=1, wide_mix_tiles=1)


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


def in_use(hip):
    """total - free of hipMemGetInfo, found through the library's own handle (as scripts/wide_fast_timing.py does)"""
    fn = hip.load_library().hipMemGetInfo
    fn.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert fn(C.byref(free), C.byref(total)) == 0
    return int(total.value - free.value)


def cut(src, lens):
    """segments of the given lengths out of the golden segments, repeated as often as it takes"""
    flat = np.concatenate(src)
    flat = np.tile(flat, -(-sum(lens) // len(flat)))
    ends = np.cumsum(lens)
    return [np.ascontiguousarray(flat[e - l:e]) for e, l in zip(ends, lens)]


def device_layout(segs):
    lens = np.array([len(s) for s in segs], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum((lens.astype(np.int64) + 63) // 64 * 64)])
    host = np.full(int(off[-1]) + 256, 2, dtype=np.uint8)
    for s, o in zip(segs, off[:-1]):
        host[o:o + len(s)] = s
    return host, off[:-1], lens


def decoding_calls(es, segs, n):
    for i in range(len(segs)):
        es.decode(i)
    es.posterior(0)
    es.scales(0)
    es.post_counts(0, np.ones((len(segs[0]), 3), np.int32), np.zeros((n, 3)))


def cycle(hip, golden, d_obs, layout, probe):
    """every owner of device memory once; probe: a list that receives (memory in use before the 64-state exact context exists,
    after its E-step, the bytes of its f and b tables)"""
    segs = cut(golden.segs_mid, [9000, 7000, 4000])
    big = cut(golden.segs_mid, [17000, 15000, 8000])
    p64 = golden.params("n64_curve")
    p64 = (p64["a"], p64["e"], p64["a0"])
    p128 = tuple(golden.n128["n128_curve." + k] for k in ("a", "e", "a0"))
    wide = dict(np.load(os.path.join(ROOT, "tests", "golden", "estep_wide.npz")))
    p200 = tuple(wide["n200." + k] for k in ("a", "e", "a0"))
    sels = [[0, 1, 2], [2, 2, 0], [1, 0, 0]]

    # exact mode, 64 states
    before = in_use(hip)
    ex = hip.HipEStep(64, mode=hip.MODE_EXACT)
    ex.load_segments(segs)
    ex.estep(*p64)
    tab_bins = sum((len(s) + 63) // 64 * 64 for s in segs) + 128
    probe.append((before, in_use(hip), 2 * tab_bins * 64 * 8))
    ex.tables(1)
    decoding_calls(ex, segs, 64)
    ex.load_segments(segs[::-1])   # a second load on the live context
    ex.estep(*p64)
    ex.close()

    # fast mode, 64 and 128 states, dozens of tiles
    for n, par in ((64, p64), (128, p128)):
        es = hip.HipEStep(n, mode=hip.MODE_FAST, chunk=512, warmup=512)
        es.load_segments(segs)
        es.estep(*par)
        es.estep_factored(*par)
        for k in ("prev_start", "merge", "adapt"):
            es.set_option(k, 1)
        es.estep(*par)
        es.estep(*par)
        for k, v in dict(prev_start=0, merge=0, adapt=0, fuse=0, fuse128=0).items():
            es.set_option(k, v)
        es.estep(*par)
        decoding_calls(es, segs, n)
        es.close()

    # the wide fast path at 200 states: decoding tables, full counts, the gap / hom / mix chains
    wsegs = [mix_sandwich(golden.segs_mid[3]), golden.segs_mid[4][:2500]]
    es = hip.HipEStep(200, mode=hip.MODE_FAST, wide_fast=1, wide_decode=1, wide_counts=1, chunk=64, warmup=512, **ALL3)
    es.load_segments(wsegs)
    es.estep_factored(*p200)
    es.estep(*p200)
    cls = es.wide_plan_tiles()["cls"]
    assert (cls == 2).any() and (cls == 4).any() and (cls == 6).any(), cls   # gap, hom and mix tiles of a qualifying run
    es.post_mean(0, np.arange(200.0))
    es.post_quantile(0, [0.025, 0.5, 0.975])
    es.close()

    # a fast batch (child contexts) and an exact batch without the f table
    es = hip.HipEStep(64, mode=hip.MODE_FAST, chunk=512, warmup=512)
    es.load_segments(segs)
    es.estep_batch([p64] * 3, sels, want="A")
    assert es.batch_info()["replicate_contexts"] == 3
    es.close()
    ex = hip.HipEStep(64, mode=hip.MODE_EXACT, exact_refwd=1)
    ex.load_segments(segs)
    ex.estep_batch([p64] * 3, sels, want="A")
    ex.close()

    # the whole-input path calls: a back-pointer table, two sample map tables
    es = hip.HipEStep(200, mode=hip.MODE_EXACT)
    es.load_segments(big)
    es.viterbi(*p200)
    es.sample_paths(*p200, seed=7, n_samp=2)
    es.close()

    # borrowed observations
    es = hip.HipEStep(64, mode=hip.MODE_FAST, chunk=512, warmup=512)
    es.load_segments_device(d_obs.data_ptr(), layout[1], layout[2], keepalive=d_obs)
    es.estep(*p64)
    es.close()


def test_closed_contexts_give_their_memory_back(hip, golden):
    import torch
    layout = device_layout(cut(golden.segs_mid, [9000, 7000, 4000]))
    d_obs = torch.from_numpy(layout[0]).cuda()
    probe, U = [], []
    for k in range(CYCLES):
        cycle(hip, golden, d_obs, layout, probe)
        torch.cuda.synchronize()
        U.append(in_use(hip))
    growth = [u - U[1] for u in U]
    print("ctx memory: in use after cycle 0..%d: %s bytes; U_k - U_1: %s; bound %d" % (CYCLES - 1, U, growth, B))
    print("ctx memory: the 64-state exact context after its E-step: +%d bytes, f and b tables %d bytes" % (probe[1][1] - probe[1][0], probe[1][2]))
    # the probe sees the library's allocations
    for before, after, tables in probe:
        assert after - before >= tables, (before, after, tables)
    # no growth
    for k in range(2, CYCLES):
        assert growth[k] <= B, (k, growth, B)
    # the borrowed tensor is the caller's: still there, unchanged
    assert np.array_equal(d_obs.cpu().numpy(), layout[0])
