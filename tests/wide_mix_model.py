"""numpy restatement of "wide_mix_tiles" (include/psmc_hip.h; psmc_amd/csrc/api_wide_fast.hip plan_wide_gaps, estep_wide_gap.hip
k_wf_mixpilot / k_wf_mixmat / k_wf_gapchain MIX): the plan rule with mix tiles as a third kind of chain tile and the memory cap, over
plan_rule / chain_rule of tests/wide_gap_model.py; the two matrices of a mix tile, built row by row as the kernels build them, against
the bin-by-bin sweeps; their long-double references; the per-application gate of tests/test_gpu_wide_mix_chain.py; and the input
mix_sandwich.  Written from the rule's text (psmc_amd/csrc/psmc_hip_ctx.h) and the algebra of the header of estep_wide_gap.hip, not
from the planner's or the kernels' code.

The algebra.  A tile covers bins lo .. hi with symbols o_lo .. o_hi, each 0 or N.  D_p = diag(e0) at a homozygous bin, the identity at a
missing one.  The forward sweep steps x <- (x a) D_p, the backward sweep y <- D_p (a y).  So
    F = a D_lo a D_lo+1 ... a D_hi,   X_hi  = X_{lo-1} F
    B = D_lo a D_lo+1 a ... D_hi a,   bt_lo = B bt_{hi+1}
Row k of F is e_k swept forward through o_lo .. o_hi.  Row k of B is D_lo(k) e_k swept forward through the SHIFTED sequence
o_lo+1 .. o_hi, N: both are forward sweeps of unit vectors.  On a pure hom tile row k of B is e0_k e_k (a D)^(T-1) a, which is
D (a D)^T D^-1."""
import numpy as np
import wide_gap_model as gm
import wide_hom_model as hm
from wide_gap_model import MISSING, mismatch, _called
from wide_hom_model import HOM, pow2_rcp


def plan_rule(segs, T, W, gap_min=0, hom_min=0, gap=False, hom=True, mix=True, mix_tiles=None):
    """(cls, glue) per tile of the plan of `segs`: cls 0, 1 / 2 = gap tile outside / inside a qualifying run, 3 / 4 = hom tile, 5 / 6 = mix
    tile (5 also: over the cap); glue bit 0 = forward, bit 1 = backward.  A mix tile is a full tile, neither first nor last of its
    segment, without a het, that holds both symbol 0 and missing bins; it exists only with `hom` and `mix` on.  The first `mix_tiles`
    mix tiles in plan order are ADMITTED (None: all -- the cap in tiles is "wide_mix_mb" x 10^6 bytes over the 16 n S bytes of a tile's
    two matrices), before runs are formed.  A chain tile is a gap tile (`gap`), a hom tile (`hom`) or an admitted mix tile; a run is a
    maximal sequence of chain tiles of one segment; it qualifies when `gap` is on and its gap tiles total gap_min bins, or `hom` is on
    and its hom and mix tiles together total hom_min bins (0: W // 4)."""
    need_g = gap_min if gap_min > 0 else W // 4
    need_h = hom_min if hom_min > 0 else W // 4
    cls, glue = [], []
    admitted = 0
    for s in segs:
        s = np.asarray(s)
        L = len(s)
        nt = (L + T - 1) // T
        lo = [1 + T * b for b in range(nt)]
        hi = [min(L, l + T - 1) for l in lo]
        c, chain = [0] * nt, [False] * nt
        for b in range(nt):
            if hi[b] - lo[b] + 1 != T or lo[b] == 1 or hi[b] == L:
                continue
            t = s[lo[b] - 1:hi[b]]
            if (t == MISSING).all():
                if gap:
                    c[b], chain[b] = 1, True
            elif (t == HOM).all():
                if hom:
                    c[b], chain[b] = 3, True
            elif ((t == HOM) | (t == MISSING)).all() and hom and mix:
                c[b] = 5
                if mix_tiles is None or admitted < mix_tiles:
                    chain[b] = True
                    admitted += 1
        b = 0
        while b < nt:
            if not chain[b]:
                b += 1
                continue
            e = b
            while e < nt and chain[e]:
                e += 1
            ng = sum(1 for t in range(b, e) if c[t] == 1)
            nh = sum(1 for t in range(b, e) if c[t] in (3, 5))
            if (gap and ng and ng * T >= need_g) or (hom and nh and nh * T >= need_h):
                for t in range(b, e):
                    c[t] += 1
            b = e
        inrun = [v in (2, 4, 6) for v in c]
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


def chain_rule(segs, T, W, **rule):
    """The chains per direction, (first, count, walk, level) in launch order: chain_rule of tests/wide_gap_model.py on the surrogate
    input whose qualifying-run tiles are missing data and whose every other bin is called (as chain_rule of tests/wide_hom_model.py)."""
    sur, at = [], 0
    cls, _ = plan_rule(segs, T, W, **rule)
    for s in segs:
        nt = (len(s) + T - 1) // T
        d = np.zeros(len(s), np.uint8)
        d[::3] = 1
        for b in range(nt):
            if cls[at + b] in (2, 4, 6):
                d[b * T:(b + 1) * T] = MISSING
        sur.append(d)
        at += nt
    c2, _ = gm.plan_rule(sur, T, W, T)
    assert np.array_equal(c2 == 2, np.isin(cls, (2, 4, 6)))
    return gm.chain_rule(sur, T, W, T)


def cap_tiles(n, mb):
    """tiles "wide_mix_mb" = mb admits at n states: mb x 10^6 bytes over two matrices of n x S doubles"""
    S = 64 * ((n + 63) // 64) if n <= 256 else 256 * ((n + 255) // 256)
    return min((mb * 1000000) // (16 * n * S), 65535)   # (and never more than 65535 tiles)


# ------------------------------------------------------------------ the two matrices of a mix tile
def sequence(sym, dr):
    """the symbols the matrix of direction dr is swept through: the tile's own (dr = 0), or shifted by one bin with N appended (dr = 1)"""
    sym = np.asarray(sym)
    return sym if dr == 0 else np.concatenate([sym[1:], [MISSING]])


def emis(e0, o):
    return e0 if o == HOM else np.ones_like(e0)


def mix_pilot(a, e0, sym, dr):
    """k_wf_mixpilot in float64: the uniform vector swept through sequence(sym, dr), scaled at every fourth bin (0, 4, ...) by the power
    of two of its own sum.  Returns (the ceil(T / 4) factors, the smallest and the largest sum the vector had on the way)."""
    n = a.shape[0]
    x = np.full(n, 1.0 / n)
    fac, lo, hi = [], np.inf, 0.0
    for p, o in enumerate(sequence(sym, dr)):
        if p % 4 == 0:
            fac.append(pow2_rcp(x.sum()))
            x = x * fac[-1]
        x = (x @ a) * emis(e0, o)
        lo, hi = min(lo, x.sum()), max(hi, x.sum())
    return np.array(fac), lo, hi


def mix_matrix(a, e0, sym, dr, fac):
    """k_wf_mixmat in float64: row k = e_k (dr = 1: times e0_k when the tile's first bin is homozygous) swept through
    sequence(sym, dr) with that direction's pilot factors: F for dr = 0, B for dr = 1"""
    M = np.eye(a.shape[0])
    if dr == 1 and sym[0] == HOM:
        M = M * e0[:, None]
    for p, o in enumerate(sequence(sym, dr)):
        if p % 4 == 0:
            M = M * fac[p // 4]
        M = (M @ a) * emis(e0, o)[None, :]
    return M


def mix_matrix_ref(a, e0, sym, dr, rows=None):
    """the unscaled F (dr = 0) or B (dr = 1) in long double, as the product of the T single steps: F = a D_lo ... a D_hi,
    B = D_lo a ... D_hi a (all of it, or the given rows)"""
    al = np.asarray(a, dtype=np.longdouble)
    el = np.asarray(e0, dtype=np.longdouble)
    n = al.shape[0]
    rows = list(range(n)) if rows is None else list(rows)
    x = np.zeros((len(rows), n), dtype=np.longdouble)
    x[np.arange(len(rows)), rows] = 1
    one = np.ones(n, dtype=np.longdouble)
    if dr == 0:
        for o in sym:
            x = np.einsum("ik,kj->ij", x, al) * (el if o == HOM else one)[None, :]
    else:
        for o in sym:
            x = np.einsum("ik,kj->ij", x * (el if o == HOM else one)[None, :], al)
    return x


def _mm(x, y):
    return np.einsum("ik,kj->ij", x, y)   # (three times as fast as x @ y on long doubles)


class PairRef:
    """Both unscaled matrices of a mix tile, ALL rows, in long double -- the product of the same T single-step matrices that
    mix_matrix_ref steps through, associated so that tiles of one model share work.  With A0 = a D (a step at a homozygous bin), A1 = a
    (at a missing one) and the core C = a D_lo+1 ... a D_hi, which F and B share:
        F = (a D_lo) C,      B = D_lo (C a).
    C is cut at its missing bins: r0 homozygous bins, N, r1 homozygous bins, N, ..., rk homozygous bins give
        C = P(r0) Q(r1) ... Q(rk),   P(r) = A0^r,   Q(r) = A1 P(r),
    k + 2 products of n x n matrices per tile instead of 2 T.  P and Q are kept per object (one model: a and e0)."""

    def __init__(self, a, e0):
        self.a = np.asarray(a, dtype=np.longdouble)
        self.e = np.asarray(e0, dtype=np.longdouble)
        self.A0 = self.a * self.e[None, :]
        self.P = [np.eye(self.a.shape[0], dtype=np.longdouble)]
        self.Q = {}

    def p(self, r):
        while len(self.P) <= r:
            self.P.append(_mm(self.P[-1], self.A0))
        return self.P[r]

    def q(self, r):
        if r not in self.Q:
            self.Q[r] = _mm(self.a, self.p(r)) if r else self.a
        return self.Q[r]

    def pair(self, sym):
        sym = np.asarray(sym)
        cuts = [-1] + [int(i) for i in np.flatnonzero(sym[1:] == MISSING)] + [len(sym) - 1]   # in the core's own numbering
        runs = [cuts[i + 1] - cuts[i] - 1 for i in range(len(cuts) - 1)]
        C = self.p(runs[0])
        for r in runs[1:]:
            C = _mm(C, self.q(r))
        first = self.A0 if sym[0] == HOM else self.a
        F = _mm(first, C)
        B = _mm(C, self.a)
        if sym[0] == HOM:
            B = B * self.e[:, None]
        return F, B


def sweep(a, e0, sym, v, backward):
    """T single steps of the sweeps from v: forward x <- (x a) D_p over lo .. hi, backward y <- D_p (a y) over hi .. lo; rescaled every
    fourth bin as the sweeps do"""
    y = np.array(v, dtype=np.float64)
    seq = sym[::-1] if backward else sym
    for p, o in enumerate(seq):
        y = emis(e0, o) * (a @ y) if backward else (y @ a) * emis(e0, o)
        if (p & 3) == 3:
            y = y / y.sum()
    return y


def chain_errors(n, M, Mh, mats, e0, cls, vec, chains, backward):
    """chain_errors of tests/wide_hom_model.py with a third kind: across a tile of class 6 the matrix is mats[tile] or mats(tile) (the
    device's F forward, its B backward), v F or B v with no D scaling.  Returns (worst per-cell error of one application, applications looked at
    as [gap, hom, mix])."""
    Ml = None if M is None else M.astype(np.longdouble)
    Hl = None if Mh is None else Mh.astype(np.longdouble)
    el = np.asarray(e0, dtype=np.longdouble)
    step = -1 if backward else 1
    worst, seen = 0.0, [0, 0, 0]
    for first, count, walk, lev in chains:
        assert walk == first + step * count
        for i in range(1, count + 1):
            tile = first + step * (i - 1)          # the tile this application crosses
            kind = {2: 0, 4: 1, 6: 2}[int(cls[tile])]
            A = (Ml, Hl, None)[kind] if kind < 2 else (mats(tile) if callable(mats) else mats[tile]).astype(np.longdouble)
            prev = vec[tile].astype(np.longdouble)
            new = vec[first + step * i]
            assert not new[n:].any(), "padded states of a chain vector"
            if backward:
                z = el * (A @ np.concatenate([prev[:n] / el, prev[n:]])) if kind == 1 else A @ prev
            else:
                z = (prev[:n] @ A)[:n]
            z = z / z.sum()
            got = new[:n].astype(np.longdouble)
            big = z >= 1e-6 * z.max()
            worst = max(worst, float((np.abs(got - z)[big] / z[big]).max()))
            seen[kind] += 1
    return worst, seen


# ------------------------------------------------------------------ inputs
HOM_PAIR, GAP_PAIR, N_FIRST, N_LAST = (20, 21), (40, 41), 10, 30   # tiles of mix_sandwich at tiles of 64 bins


def mix_sandwich(src, called=300, inner=4096, second=345, T=64, seed=20):
    """300 called bins of src, 4096 het-free bins, 300 called bins cut at bin `second` (as hom_sandwich of tests/wide_hom_model.py cuts
    them).  Inside the het-free stretch every bin is symbol 0 but for N bins at irregular positions drawn by a seeded generator, tile
    by tile of T bins: every full tile inside it holds between 1 and T / 3 missing bins (so both symbols: class 3) -- except tiles 20
    and 21, which are pure hom tiles, and tiles 40 and 41, which are pure gap tiles.  Tile 10 has N at its first bin (and symbol 0 at
    its last), tile 30 N at its last bin (and symbol 0 at its first).  One run of the plan so holds all three kinds of chain tile."""
    d = _called(src)
    mid = np.zeros(inner, np.uint8)
    rng = np.random.default_rng(seed)
    first = -(-called // T)                        # the first tile that lies inside the stretch
    last = (called + inner) // T - 1               # ... and the last
    for b in range(first, last + 1):
        at = b * T - called
        k = int(rng.integers(1, T // 3 + 1))
        pos = rng.choice(np.arange(1, T - 1), size=k, replace=False)   # (never the first or the last bin: those are set below)
        mid[at + pos] = MISSING
        if b in HOM_PAIR:
            mid[at:at + T] = HOM
        elif b in GAP_PAIR:
            mid[at:at + T] = MISSING
        elif b == N_FIRST:
            mid[at] = MISSING
        elif b == N_LAST:
            mid[at + T - 1] = MISSING
    return np.concatenate([d[:called], mid, d[second:second + called]])


def crossed(chains):
    """[forward, backward]: the tiles a direction's chains cross -- first, first +- 1, ..., `count` of them per chain.  A class-6 tile's
    F is built where a forward chain crosses it, its B where a backward chain does."""
    return [{first + (-j if d else j) for first, count, walk, lev in chains[d] for j in range(count)} for d in (0, 1)]


def tile_symbols(seg, T, b):
    return np.asarray(seg)[b * T:(b + 1) * T]
