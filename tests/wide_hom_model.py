"""numpy restatement of "wide_hom_tiles" (include/psmc_hip.h; psmc_amd/csrc/api_wide_fast.hip plan_wide_gaps, estep_wide_gap.hip
k_wf_hompilot / k_wf_hommat / k_wf_gapchain HOM): the generalised plan rule -- chain tiles of two kinds, runs that qualify through
either threshold -- over plan_rule / chain_rule of tests/wide_gap_model.py, the pilot-scaled matrix of a homozygous tile against the
bin-by-bin sweep, the long-double references and the per-application gate of tests/test_gpu_wide_hom_chain.py, and the inputs of
tests/test_gpu_wide_hom.py.  Written from the rule's text (psmc_amd/csrc/psmc_hip_ctx.h), not from the planner's code."""
import numpy as np
import wide_gap_model as gm
from wide_gap_model import MISSING, mismatch, _called

HOM = 0   # the symbol of a homozygous bin


def plan_rule(segs, T, W, gap_min=0, hom_min=0, gap=False, hom=True):
    """(cls, glue) per tile of the plan of `segs`: cls 0, 1 / 2 = gap tile outside / inside a qualifying run, 3 / 4 = hom tile outside /
    inside one; glue bit 0 = forward, bit 1 = backward.  A chain tile is a gap tile (`gap` on) or a hom tile (`hom` on): a full tile,
    neither first nor last of its segment, of missing bins only / of symbol 0 only.  A run is a maximal sequence of chain tiles; it
    qualifies when `gap` is on and its gap tiles total gap_min bins, or `hom` is on and its hom tiles total hom_min bins (0: W // 4)."""
    need_g = gap_min if gap_min > 0 else W // 4
    need_h = hom_min if hom_min > 0 else W // 4
    cls, glue = [], []
    for s in segs:
        s = np.asarray(s)
        L = len(s)
        nt = (L + T - 1) // T
        lo = [1 + T * b for b in range(nt)]
        hi = [min(L, l + T - 1) for l in lo]
        c = [0] * nt
        for b in range(nt):
            if hi[b] - lo[b] + 1 != T or lo[b] == 1 or hi[b] == L:
                continue
            t = s[lo[b] - 1:hi[b]]
            if gap and (t == MISSING).all():
                c[b] = 1
            elif hom and (t == HOM).all():
                c[b] = 3
        b = 0
        while b < nt:
            if not c[b]:
                b += 1
                continue
            e = b
            while e < nt and c[e]:
                e += 1
            ng, nh = sum(1 for t in range(b, e) if c[t] == 1), sum(1 for t in range(b, e) if c[t] == 3)
            if (gap and ng and ng * T >= need_g) or (hom and nh and nh * T >= need_h):
                for t in range(b, e):
                    c[t] += 1
            b = e
        inrun = [v in (2, 4) for v in c]
        tile_of = lambda p: (p - 1) // T
        g = [0] * nt
        for b in range(nt):
            if not lo[b] - W <= 1 and b > 0:                                  # not anchored forward
                win = range(max(1, lo[b] - W), lo[b])
                if inrun[b] or (W > 0 and len(win) and any(inrun[t] for t in range(tile_of(win[0]), tile_of(win[-1]) + 1))):
                    g[b] |= 1
            if not hi[b] + W + 1 >= L and b < nt - 1:                         # not anchored backward
                win = range(hi[b] + 1, min(L, hi[b] + W) + 1)
                if inrun[b] or (W > 0 and len(win) and any(inrun[t] for t in range(tile_of(win[0]), tile_of(win[-1]) + 1))):
                    g[b] |= 2
        cls += c
        glue += g
    return np.array(cls, dtype=np.int32), np.array(glue, dtype=np.int32)


def chain_rule(segs, T, W, gap_min=0, hom_min=0, gap=False, hom=True):
    """The chains per direction, (first, count, walk, level) in launch order.  Chains, glue and levels do not look at what a tile holds,
    only at which tiles belong to a qualifying run: so this is chain_rule of tests/wide_gap_model.py on a surrogate input whose
    qualifying-run tiles are missing data and whose every other bin is called, every run of it qualifying (minimum: one tile)."""
    sur, at = [], 0
    cls, _ = plan_rule(segs, T, W, gap_min, hom_min, gap, hom)
    for s in segs:
        nt = (len(s) + T - 1) // T
        d = np.zeros(len(s), np.uint8)
        d[::3] = 1   # (no tile of the surrogate is a chain tile by itself)
        for b in range(nt):
            if cls[at + b] in (2, 4):
                d[b * T:(b + 1) * T] = MISSING
        sur.append(d)
        at += nt
    c2, _ = gm.plan_rule(sur, T, W, T)
    assert np.array_equal(c2 == 2, np.isin(cls, (2, 4)))
    return gm.chain_rule(sur, T, W, T)


# ------------------------------------------------------------------ the matrix of a hom tile
def pow2_rcp(x):
    """2^-E for x = 1.m x 2^E (struct_prims.h pow2_rcp): x * pow2_rcp(x) lies in [1, 2)"""
    return 2.0 ** -(np.frexp(x)[1] - 1)


def hom_pilot(a, e0, T):
    """k_wf_hompilot in float64: the uniform vector swept T bins under symbol 0, scaled at every fourth bin (0, 4, ...) by the power of
    two of its own sum.  Returns (the ceil(T / 4) factors, the smallest and the largest sum the vector had on the way)."""
    n = a.shape[0]
    x = np.full(n, 1.0 / n)
    fac, lo, hi = [], np.inf, 0.0
    for p in range(T):
        if p % 4 == 0:
            fac.append(pow2_rcp(x.sum()))
            x = x * fac[-1]
        x = (x @ a) * e0
        lo, hi = min(lo, x.sum()), max(hi, x.sum())
    return np.array(fac), lo, hi


def hom_matrix(a, e0, T, fac):
    """k_wf_hommat in float64: row k = the unit vector of state k swept T bins under symbol 0 with the pilot's factors"""
    M = np.eye(a.shape[0])
    for p in range(T):
        if p % 4 == 0:
            M = M * fac[p // 4]
        M = (M @ a) * e0[None, :]
    return M


def hom_chain_vs_sweep(a, e0, x0, T, tiles, backward=False):
    """Largest mismatch, over `tiles` tiles in a row, between ONE application of the pilot-scaled M_h (forward x <- x M_h, backward
    y <- D M_h D^-1 y, D = diag(e0)) and T single steps from the same vector (forward x <- e0 . (x a), backward y <- e0 . (a y), rescaled
    every fourth bin as the sweeps do).  The vector is normalised after every tile, as the chain keeps it."""
    fac, _, _ = hom_pilot(a, e0, T)
    M = hom_matrix(a, e0, T, fac)
    worst, x = 0.0, np.array(x0, dtype=np.float64)
    for _ in range(tiles):
        y = x.copy()
        for p in range(T):
            y = e0 * (a @ y) if backward else (y @ a) * e0
            if (p & 3) == 3:
                y = y / y.sum()
        z = e0 * (M @ (x / e0)) if backward else x @ M
        worst = max(worst, mismatch(z, y))
        x = z / z.sum()
    return worst


def hom_matrix_ref(a, e0, T, rows=None):
    """(a D) to the power T in long double, D = diag(e0): the unscaled M_h (all of it by binary exponentiation, or the given rows stepped)"""
    ad = np.asarray(a, dtype=np.longdouble) * np.asarray(e0, dtype=np.longdouble)[None, :]
    return gm.matrix_ref(ad, T) if rows is None else gm.matrix_rows_ref(ad, T, rows)


def chain_errors(n, M, Mh, e0, cls, vec, chains, backward):
    """chain_errors of tests/wide_gap_model.py with the matrix of the crossed tile's class: worst per-cell error of one application over
    all chained tiles of a direction -- vec[t] against the normalised long-double product of the device's matrix and the device's vector
    of the tile before it in the sweep (forward v M or v M_h; backward M v or D M_h D^-1 v) -- and the applications looked at, per kind"""
    Ml = None if M is None else M.astype(np.longdouble)
    Hl = None if Mh is None else Mh.astype(np.longdouble)
    el = np.asarray(e0, dtype=np.longdouble)
    step = -1 if backward else 1
    worst, seen = 0.0, [0, 0]
    for first, count, walk, lev in chains:
        assert walk == first + step * count
        for i in range(1, count + 1):
            tile = first + step * (i - 1)          # the tile this application crosses
            hom = cls[tile] == 4
            assert cls[tile] in (2, 4)
            A = Hl if hom else Ml
            prev = vec[tile].astype(np.longdouble)
            new = vec[first + step * i]
            assert not new[n:].any(), "padded states of a chain vector"
            if backward:
                z = el * (A @ np.concatenate([prev[:n] / el, prev[n:]])) if hom else A @ prev
            else:
                z = (prev[:n] @ A)[:n]
            z = z / z.sum()
            got = new[:n].astype(np.longdouble)
            big = z >= 1e-6 * z.max()
            worst = max(worst, float((np.abs(got - z)[big] / z[big]).max()))
            seen[1 if hom else 0] += 1
    return worst, seen


# ------------------------------------------------------------------ inputs
def hom_sandwich(src, called=300, homs=4096, second=345):
    """input (a) of tests/test_gpu_wide_hom.py: `called` called bins, `homs` bins of symbol 0, `called` called ones.  The second called
    piece is cut at bin `second` of src, where segs_mid[3] has a het 14 bins on: at tiles of 64 bins the tile in which the run ends then
    holds a het, and the hom tiles are the 63 that lie inside the planted run (the piece at 300 starts with 59 homozygous bins, which
    would make that tile a 64th)."""
    d = _called(src)
    return np.concatenate([d[:called], np.zeros(homs, np.uint8), d[second:second + called]])


def hom_mixed(src, other):
    """input (b): a 12 000-bin segment -- a 3 000-bin hom run at 1 500, directly behind it 300 bins that alternate five bins of symbol 0
    and five missing ones (every tile inside holds both: class 3 of k_tile_class) and 1 200 homozygous bins more, a 200-bin hom run at
    7 000, a 1 000-bin run of N at 8 500 directly followed by a 1 000-bin hom run -- and a second segment, all data"""
    d = _called(src[:12000]).copy()
    assert len(d) == 12000
    d[1500:4500] = HOM
    d[4500:4800] = np.where((np.arange(300) // 5) % 2 == 0, HOM, MISSING)
    d[4800:6000] = HOM
    d[7000:7200] = HOM
    d[8500:9500] = MISSING
    d[9500:10500] = HOM
    o = _called(other[:2500])
    return [d, o]
