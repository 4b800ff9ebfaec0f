"""numpy restatement of "wide_gap_tiles" (include/psmc_hip.h; psmc_amd/csrc/api_wide_fast.hip plan_wide_gaps, estep_wide_gap.hip):
the plan rule -- classes and glue bits of the wide plan's tiles -- and the two ways across a tile of missing data, one application
of the transfer matrix against T single steps.  Written from the rule's text, position by position, not from the planner's code."""
import numpy as np

MISSING = 2


def plan_rule(segs, T, W, gap_min=0):
    """(cls, glue) per tile of the plan of `segs` (tiles of T bins per segment, warm-up W in both directions): cls 0, 1 = gap tile
    outside a qualifying run, 2 = gap tile of one; glue bit 0 = forward, bit 1 = backward."""
    need = gap_min if gap_min > 0 else W // 4
    cls, glue = [], []
    for s in segs:
        s = np.asarray(s)
        L = len(s)
        nt = (L + T - 1) // T
        lo = [1 + T * b for b in range(nt)]
        hi = [min(L, l + T - 1) for l in lo]
        anchor_f = [lo[b] - W <= 1 for b in range(nt)]
        anchor_b = [hi[b] + W + 1 >= L for b in range(nt)]
        gap = [hi[b] - lo[b] + 1 == T and lo[b] > 1 and hi[b] < L and bool((s[lo[b] - 1:hi[b]] == MISSING).all()) for b in range(nt)]
        c = [1 if g else 0 for g in gap]
        b = 0
        while b < nt:
            if not gap[b]:
                b += 1
                continue
            e = b
            while e < nt and gap[e]:
                e += 1
            if (e - b) * T >= need:
                c[b:e] = [2] * (e - b)
            b = e
        tile_of = lambda p: (p - 1) // T
        g = [0] * nt
        for b in range(nt):
            if not anchor_f[b] and b > 0:
                win = range(max(1, lo[b] - W), lo[b])                      # positions lo - wf .. lo - 1
                if c[b] == 2 or (W > 0 and len(win) and any(c[t] == 2 for t in range(tile_of(win[0]), tile_of(win[-1]) + 1))):
                    g[b] |= 1
            if not anchor_b[b] and b < nt - 1:
                win = range(hi[b] + 1, min(L, hi[b] + W) + 1)              # positions hi + 1 .. hi + wb
                if c[b] == 2 or (W > 0 and len(win) and any(c[t] == 2 for t in range(tile_of(win[0]), tile_of(win[-1]) + 1))):
                    g[b] |= 2
        cls += c
        glue += g
    return np.array(cls, dtype=np.int32), np.array(glue, dtype=np.int32)


def mismatch(u, v):
    """tile_mismatch of psmc_amd/csrc/wide_prims.h: max_k |u/|u| - v/|v|| / max_k v/|v|"""
    u = u / u.sum(); v = v / v.sum()
    return float(np.abs(u - v).max() / np.abs(v).max())


def chain_vs_sweep(a, x0, T, tiles, backward=False):
    """Largest mismatch, over `tiles` tiles in a row, between ONE application of M = a^T-th power (built row by row: the unit vector of
    state k stepped T times, as k_wf_gapmat does) and T single steps from the same vector -- forward x <- x a, backward y <- a y
    (the emission of a missing bin is 1).  The vector is normalised after every tile, as the chain keeps it."""
    n = a.shape[0]
    M = np.eye(n)
    for _ in range(T):
        M = M @ a            # row k: e_k stepped T times forward
    worst, x = 0.0, np.array(x0, dtype=np.float64)
    for _ in range(tiles):
        y = x.copy()
        for p in range(T):
            y = a @ y if backward else y @ a
            if (p & 3) == 3:
                y = y / y.sum()   # the sweeps rescale every fourth position
        z = M @ x if backward else x @ M
        worst = max(worst, mismatch(z, y))
        x = z / z.sum()
    return worst


def sandwich(src, called=300, missing=4096):
    """input (a) of tests/test_gpu_wide_gap.py: `called` called bins, `missing` missing ones, `called` called ones"""
    d = np.where(np.asarray(src) == MISSING, 0, np.asarray(src)).astype(np.uint8)
    return np.concatenate([d[:called], np.full(missing, MISSING, np.uint8), d[called:2 * called]])


def mixed(src, other):
    """input (b): a 12 000-bin segment with 3 000 missing bins in the middle and a second run of 200; a second segment, all data"""
    d = np.where(np.asarray(src[:12000]) == MISSING, 0, np.asarray(src[:12000])).astype(np.uint8)
    assert len(d) == 12000
    d[4500:7500] = MISSING
    d[9000:9200] = MISSING
    o = np.where(np.asarray(other[:2500]) == MISSING, 0, np.asarray(other[:2500])).astype(np.uint8)
    return [d, o]
