"""numpy restatement of "wide_gap_tiles" (include/psmc_hip.h; psmc_amd/csrc/api_wide_fast.hip plan_wide_gaps, estep_wide_gap.hip):
the plan rule -- classes and glue bits of the wide plan's tiles, and the chains across its qualifying runs -- and the two ways across a
tile of missing data, one application of the transfer matrix against T single steps.  Written from the rule's text, position by
position, not from the planner's code.  Also the long-double references of the matrix, the gate on one application of the chain, and
the inputs of tests/test_gpu_wide_gap.py and tests/test_gpu_wide_gap_chain.py."""
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


def chain_rule(segs, T, W, gap_min=0):
    """The chains of the plan of `segs` per direction (forward, backward), in launch order: lists of (first, count, walk, level), tile
    numbers counted over all segments as plan_rule counts them.  Written from the text of the rule (psmc_hip_ctx.h, "wide_gap_tiles" and
    WgDir), for a segment seen in sweep order -- the backward direction is the forward rule on the mirrored segment.  (The three
    conditions of the count-0 clause and the tiles a walk covers were first read from plan_wide_gaps, whose header text did not state
    them; the text now does.  What anchors this function independently of the planner are the literals of tests/test_wide_gap_model.py.)
      * a chain starts behind the run's tiles that are anchored in the direction: `first` is the run's first tile that is not anchored,
        the chain applies the matrix once per tile from there to the run's last one, and its last vector is the start vector of the tile
        behind the run, where one walk goes on through the tiles glued behind it (glued, and no tile of a qualifying run);
      * a run that is anchored throughout has no tile to cross: a chain of count 0 stands on the first tile behind the run that is not
        anchored, if that tile is glued, belongs to no qualifying run and no earlier walk has been through it -- only the walk hangs on it;
      * when every tile from the run to the segment's end is anchored there is no chain;
      * a chain whose first vector (the exit vector of the tile before `first`) comes out of an earlier chain's tiles or walk is one
        level later than that chain; chains run level by level, within a level in sweep order."""
    out = ([], [])
    t0 = 0
    for s in segs:
        s = np.asarray(s)
        L = len(s)
        nt = (L + T - 1) // T
        cls, glue = plan_rule([s], T, W, gap_min)
        lo = [1 + T * b for b in range(nt)]
        hi = [min(L, l + T - 1) for l in lo]
        for d in (0, 1):
            # the segment in sweep order: position i of the sweep is tile order[i]
            order = list(range(nt)) if d == 0 else list(range(nt - 1, -1, -1))
            anch = [(lo[b] - W <= 1) if d == 0 else (hi[b] + W + 1 >= L) for b in order]
            run = [cls[b] == 2 for b in order]
            glued = [bool(glue[b] & (1 << d)) for b in order]
            level_of = {}     # sweep position -> level of the chain whose tiles or walk leave this tile's vectors
            found = []
            i = 0
            while i < nt:
                if not run[i]:
                    i += 1
                    continue
                e = i
                while e + 1 < nt and run[e + 1]:
                    e += 1
                f = i
                while f < nt and anch[f]:
                    f += 1
                nxt = e + 1
                if f == nt:
                    i = nxt
                    continue
                if f <= e:
                    count, walk = e - f + 1, e + 1
                elif glued[f] and not run[f] and f not in level_of:
                    count, walk = 0, f
                else:
                    i = nxt
                    continue
                lev = level_of[f - 1] + 1 if f - 1 in level_of else 0
                for b in range(f, walk + 1):
                    level_of[b] = lev
                b = walk + 1
                while b < nt and glued[b] and not run[b]:
                    level_of[b] = lev
                    b += 1
                found.append((t0 + order[f], count, t0 + order[walk], lev))
                i = nxt
            out[d].extend(found)
        t0 += nt
    # launch order over all segments: by level, then plan order of the segments in the sweep's direction
    fwd = sorted(out[0], key=lambda c: c[3])
    bwd = sorted(sorted(out[1], key=lambda c: -c[0]), key=lambda c: c[3])
    return fwd, bwd


def matrix_ref(a, T):
    """a to the power T in long double by binary exponentiation: row k is the unit vector of state k stepped T times forward under
    the missing symbol (emission 1), what k_wf_gapmat builds."""
    a = np.asarray(a, dtype=np.longdouble)
    r, p, t = np.eye(a.shape[0], dtype=np.longdouble), a.copy(), int(T)
    while t:
        if t & 1:
            r = r @ p
        t >>= 1
        if t:
            p = p @ p
    return r


def matrix_rows_ref(a, T, rows):
    """Rows `rows` of a to the power T in long double: the unit vectors stepped T times (for sizes where the full product is too slow)."""
    a = np.asarray(a, dtype=np.longdouble)
    x = np.zeros((len(rows), a.shape[0]), dtype=np.longdouble)
    x[np.arange(len(rows)), list(rows)] = 1
    for _ in range(int(T)):
        x = np.einsum("ik,kj->ij", x, a)   # (three times as fast as x @ a on long doubles)
    return x


def chain_errors(n, M, vec, chains, backward):
    """worst per-cell error of one application over all chained tiles of a direction: vec[t] against the normalised long-double product
    of the device's matrix and the device's vector of the tile before it in the sweep; and the number of applications looked at"""
    Ml = M.astype(np.longdouble)
    step = -1 if backward else 1
    worst, seen = 0.0, 0
    for first, count, walk, lev in chains:
        assert walk == first + step * count
        if count == 0:
            continue
        prev = vec[[first + step * (i - 1) for i in range(1, count + 1)]].astype(np.longdouble)
        new = vec[[first + step * i for i in range(1, count + 1)]]
        if backward:
            assert not new[:, n:].any(), "padded states of a backward chain vector"
            z = np.einsum("ij,kj->ik", prev, Ml)     # (M y)_k = sum_j M[k][j] y_j over the padded width
        else:
            z = np.einsum("ik,kj->ij", prev[:, :n], Ml)[:, :n]
            assert not new[:, n:].any(), "padded states of a forward chain vector"
        z = z / z.sum(1)[:, None]
        got = new[:, :n].astype(np.longdouble)
        big = z >= 1e-6 * z.max(1)[:, None]
        err = np.where(big, np.abs(got - z) / np.where(big, z, 1), 0)
        worst = max(worst, float(err.max()))
        seen += count
    return worst, seen


def _called(src):
    return np.where(np.asarray(src) == MISSING, 0, np.asarray(src)).astype(np.uint8)


def _pieces(src, *parts):
    """called and missing pieces in turn (called first), the called ones consecutive bins of src"""
    d, out, at = _called(src), [], 0
    for i, n in enumerate(parts):
        if i % 2 == 0:
            out.append(d[at:at + n]); at += n
            assert len(out[-1]) == n
        else:
            out.append(np.full(n, MISSING, np.uint8))
    return np.concatenate(out)


def twin(src, called=300, missing=1024, mid=128):
    """called + missing + mid + missing + called (2776 bins): two runs closer than a warm-up -- the second chain is one level later"""
    return _pieces(src, called, missing, mid, missing, called)


def head_run(src, head=300, missing=200, tail=450):
    """a short run close to the segment's start: at tiles of 64 bins its two full tiles lie in the zone a warm-up of 512 anchors forward"""
    return _pieces(src, head, missing, tail)


def tail_run(src, head=450, missing=200, tail=300):
    """head_run mirrored: the run lies in the zone anchored backward"""
    return _pieces(src, head, missing, tail)


def tiles_missing(src, n_tiles, T, *runs):
    """a segment of n_tiles tiles of T bins cut from src (None: of zeros), the tiles lo .. hi (inclusive) of every (lo, hi) in `runs` missing"""
    d = np.zeros(n_tiles * T, np.uint8) if src is None else _called(src)[:n_tiles * T].copy()
    assert len(d) == n_tiles * T
    for lo, hi in runs:
        d[lo * T:(hi + 1) * T] = MISSING
    return d


def triple(src, T=64):
    """70 tiles of T bins with runs on tiles 20-23, 26-29 and 32-35: three chains per direction, levels 0, 1, 2"""
    return tiles_missing(src, 70, T, (20, 23), (26, 29), (32, 35))


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
