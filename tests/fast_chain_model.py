"""The transfer-matrix chain of the fast path up to 128 states, restated for the tests (psmc_amd/csrc/estep_struct.hip k_kcol_struct,
k_kcol2_struct, k_kchain_struct; api_fast.hip build_items add_runs / push_kc).  Written from the kernels' comments and the definitions
of tests/fastmodel.py, position by position.  Three parts:
  * long-double references: the product of the steps over a list of positions (range_matrix_ref), the positions a chain tile's
    matrices and the chain itself cover (kc_ranges), every tile's boundary vectors (boundary_refs);
  * a float64 restatement of the algorithm (sweep_columns, chain_apply, tail_steps, chain_tile) with three deliberate faults, which the
    gates below must tell from the correct one (tests/test_fast_chain_model.py);
  * chain_rule: which glued runs are chained and which tiles share a matrix slot;
and the gates tests/test_gpu_fast_chain.py puts the device's matrices and vectors through (matrix_error, chain_tile_ref, vector_error)
with their bounds, and the inputs of both test files.

Notation (tests/fastmodel.py): positions p = 1 .. L, o_p the observation; one forward step x -> e[o_p] * (a^T x), one backward step
x -> e[o_p] * (a x); the emission of a missing bin is 1.  A matrix is kept as M[col][k] = element k of the unit vector of state `col`
after the steps (the layout of the device's d_Kcol)."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
MISSING = 2
CELL_FLOOR = 1e-6   # the project's cell rule: cells of at least this fraction of the largest carry weight


def emissions(e, dtype=np.float64):
    """(3, n): hom, het, missing (all ones)"""
    e = np.asarray(e, dtype=dtype)
    return np.vstack([e[0], e[1], np.ones(e.shape[1], dtype=dtype)])


def tiles_of(L, T):
    """[(lo, hi)] of a segment of L bins"""
    return [(lo, min(L, lo + T - 1)) for lo in range(1, L + 1, T)]


# ------------------------------------------------------------------ positions
def kc_ranges(lo, hi, L, backward, sub, fault=None):
    """The positions of a chain tile lo .. hi of a segment of L bins, in traversal order: (ranges, tail).  Forward the matrices cover
    lo .. hi.  Backward they cover top = min(hi, L - 1) down to min(((lo + 3) & ~3) + 1, top + 1), that is down to the position above
    the tile's lowest rescaled position p* = the first p >= lo with p % 4 == 0; the chain walks the tail p* .. lo itself (at most four
    steps).  Either way the matrices' n positions are cut into `sub` consecutive ranges [n js / sub, n (js + 1) / sub).
    fault = "split_shift": the backward split one position too high (the step at p* + 1 is in neither part)."""
    if not backward:
        pos, tail = list(range(lo, hi + 1)), []
    else:
        top = min(hi, L - 1)
        start = min(((lo + 3) & ~3) + 1, top + 1) + (1 if fault == "split_shift" else 0)
        pos = list(range(top, start - 1, -1))
        tail = list(range(min((lo + 3) & ~3, top), lo - 1, -1))
    n = len(pos)
    return [pos[n * js // sub:n * (js + 1) // sub] for js in range(sub)], tail


# ------------------------------------------------------------------ long-double references
def _power_apply(x, B, r):
    """x B^r by binary exponentiation"""
    while r:
        if r & 1:
            x = x @ B
        r >>= 1
        if r:
            B = B @ B
    return x


def range_matrix_ref(a, e, obs, positions, backward=False, cols=None):
    """Long double: rows = the unit vectors of the states `cols` (all, by default) taken through the steps at `positions` (1-based
    positions of the segment obs, in traversal order).  Stretches of one symbol are taken as a power of that symbol's step matrix --
    the same product, associated differently -- once they are long enough for that to be cheaper."""
    a = np.asarray(a, dtype=LD)
    n = a.shape[0]
    e3 = emissions(e, LD)
    cols = list(range(n)) if cols is None else list(cols)
    x = np.zeros((len(cols), n), dtype=LD)
    x[np.arange(len(cols)), cols] = 1
    at = a.T.copy() if backward else a
    step = {}
    i, m = 0, len(positions)
    while i < m:
        s = int(obs[positions[i] - 1])
        j = i
        while j < m and int(obs[positions[j] - 1]) == s:
            j += 1
        if s not in step:
            step[s] = at * e3[min(s, 2)][None, :]      # (x B)_j = e_j sum_k x_k at[k][j]
        if (j - i) * len(cols) > 8 * n:
            x = _power_apply(x, step[s], j - i)
        else:
            for _ in range(j - i):
                x = x @ step[s]
        i = j
    return x


def boundary_refs(a, e, a0, seg, T):
    """(entry, bentry), tiles x n in long double, each row with sum 1: entry[t] ~ X_{lo - 1}, the forward vector a tile builds on
    (k_walk1_struct stores x when p == the tile's lo, before the step at lo; the first tile has none: NaN), bentry[t] ~ bt_{top + 1}, top
    = min(hi, L - 1) (k_walk1_struct stores x when p == top, before the step at top; bt_L = e[o_L]; NaN for a last tile that holds
    position L only)."""
    a = np.asarray(a, dtype=LD)
    n = a.shape[0]
    e3 = emissions(e, LD)
    seg = np.asarray(seg)
    L = len(seg)
    tl = tiles_of(L, T)
    entry = np.full((len(tl), n), np.nan, dtype=LD)
    bentry = np.full((len(tl), n), np.nan, dtype=LD)
    starts = {lo: t for t, (lo, hi) in enumerate(tl)}
    x = np.asarray(a0, dtype=LD) * e3[min(int(seg[0]), 2)]
    for p in range(2, L + 1):
        x = x / x.sum()
        if p in starts:
            entry[starts[p]] = x
        x = (x @ a) * e3[min(int(seg[p - 1]), 2)]
    tops = {min(hi, L - 1): t for t, (lo, hi) in enumerate(tl) if min(hi, L - 1) >= lo}
    y = e3[min(int(seg[L - 1]), 2)].copy()
    for p in range(L - 1, 0, -1):
        y = y / y.sum()
        if p in tops:
            bentry[tops[p]] = y
        y = (a @ y) * e3[min(int(seg[p - 1]), 2)]
    return entry, bentry


# ------------------------------------------------------------------ float64 restatement
def sweep_columns(a, e, obs, positions, backward=False):
    """The column sweep: all unit vectors through `positions`; before the step at a position p % 4 == 0 a column is divided by the
    power of two 2^ex, s = m 2^ex its sum with 0.5 <= m < 1, and ex is added to the column's exponent.  (K, E): K[col] 2^E[col] is
    the true column.  Zero positions: the identity, exponents 0."""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    e3 = emissions(e)
    at = a.T if backward else a
    x, E = np.eye(n), np.zeros(n, dtype=np.int64)
    for p in positions:
        if p % 4 == 0:
            s = x.sum(1)
            ex = np.where(s > 0, np.frexp(s)[1], 0)
            x = np.ldexp(x, -ex[:, None])
            E += ex
        x = (x @ at) * e3[min(int(obs[p - 1]), 2)]
    return x, E


def chain_apply(K, E, x, fault=None):
    """One product of the chain: the positive entries of x are scaled by 2^(E - emax), emax the largest exponent among them, the
    others are 0; y_k = sum_col xs[col] K[col][k]; y is left with sum 1.
    fault = "drop_row": the source state with the largest weight is left out; "no_exp": the exponents are ignored."""
    pos = x > 0
    E = np.zeros_like(E) if fault == "no_exp" else E
    emax = E[pos].max()
    xs = np.where(pos, np.ldexp(x, np.where(pos, E - emax, 0)), 0.0)
    if fault == "drop_row":
        xs[int(np.argmax(xs))] = 0.0
    y = xs @ K
    return y / y.sum()


def tail_steps(a, e, obs, tail, y, dtype=np.float64):
    """The backward chain's own steps p* .. lo with the sweep's scaling: at p % 4 == 0 the step divides by the sum of the vector it
    starts from"""
    a = np.asarray(a, dtype=dtype)
    e3 = emissions(e, dtype)
    for p in tail:
        ev = e3[min(int(obs[p - 1]), 2)]
        if p % 4 == 0:
            ev = ev / y.sum()
        y = (a @ y) * ev
    return y


def chain_tile(a, e, obs, lo, hi, backward, sub, x, fault=None):
    """One tile of a chain in float64: (the vector at the tile's far boundary, [(K, E)] per range)"""
    L = len(obs)
    ranges, tail = kc_ranges(lo, hi, L, backward, sub, "split_shift" if fault == "split_shift" else None)
    mats = [sweep_columns(a, e, obs, r, backward) for r in ranges]
    for js, (K, E) in enumerate(mats):
        x = chain_apply(K, E, x, fault if js == 0 else None)
    if backward:
        x = tail_steps(a, e, obs, tail, x)
    return x, mats


# ------------------------------------------------------------------ gates and bounds
def matrix_bound(steps, n):
    """(a): per step a cell is a sum of at most n non-negative products; the factorisation gate admits 64 ulp on an entry of a; about six
    further roundings (emission, the scan's combination, the rescale is exact); doubled"""
    return 2 * max(steps, 1) * (n + 70) * U


def apply_bound(sub, n, backward):
    """(b): per range one n-term sum, one n-term norm, the reciprocal and the product, doubled; backward the at most four tail steps,
    referenced with the dense a (n-term sum, 64 ulp, the emission, an n-term norm at p % 4 == 0 with its reciprocal and product)"""
    return 2 * sub * (2 * n + 4) * U + (2 * 4 * (2 * n + 73) * U if backward else 0.0)


def vector_bound(d, n):
    """(c): d steps from the end of the segment the sweep started at, each within the per-step figure of (a); the start itself (the
    initial vector, or e[o_L]) and the normalisation to sum 1 count as one step"""
    return 2 * max(d, 1) * (n + 70) * U


def matrix_error(K, E, ref, n, cols=None):
    """Worst relative error of the device's (or the restatement's) columns K[col][:n] against ref[i] 2^-E[col] (ref: long double rows
    for `cols`), over the cells of at least CELL_FLOOR x the column's largest -- the largest itself is one of them."""
    cols = list(range(n)) if cols is None else list(cols)
    want = np.ldexp(np.asarray(ref, dtype=LD), -np.asarray(E, dtype=np.int64)[cols][:, None])
    got = np.asarray(K, dtype=LD)[cols][:, :n]
    top = want.max(1)
    assert (top > 0).all(), "a reference column is all zero"
    big = want >= CELL_FLOOR * top[:, None]
    err = np.where(big, np.abs(got - want) / np.where(big, want, 1), 0)
    return float(err.max())


def chain_tile_ref(a, e, obs, lo, hi, backward, mats, x, n):
    """Long double: the vector a chain leaves at the far boundary of tile lo .. hi, from ITS OWN matrices and exponents (mats: [(K, E)]
    per range, any padded width) and its previous vector x; sum 1."""
    y = np.asarray(x, dtype=LD)[:n]
    for K, E in mats:
        w = np.ldexp(y, np.asarray(E, dtype=np.int64)[:n] - int(np.asarray(E)[:n].max()))
        y = w @ np.asarray(K, dtype=LD)[:n, :n]
        y = y / y.sum()
    if backward:
        y = tail_steps(a, e, obs, kc_ranges(lo, hi, len(obs), True, 1)[1], y, dtype=LD)
    return y / y.sum()


def vector_error(got, want):
    """Worst relative error over the cells of at least CELL_FLOOR x the largest of want, both brought to sum 1 in long double"""
    g = np.asarray(got, dtype=LD)
    w = np.asarray(want, dtype=LD)
    g = g / g.sum()
    w = w / w.sum()
    big = w >= CELL_FLOOR * w.max()
    return float((np.abs(g - w)[big] / w[big]).max())


# ------------------------------------------------------------------ the list builder
def chain_rule(segs, T, W, glue, cls, n_states, group_cap=131072, kc_min=-1, kc_div=16, kc_sub=None):
    """What build_items makes of the glued runs of a plan (segments `segs` in tiles of T bins, warm-ups of W bins in both directions,
    glue bits and classes as psmc_hip_plan_tiles reports them): dict(runs = (forward, backward) lists of (first, count) in launch order,
    kc = [(tile, dir)], kslot, kuniq, sub; glued = every glued run of either direction, chained or walked, in tile order).
      * A run is a maximal stretch of tiles of one segment glued in the direction (forward: glue bit 0 ties a tile to the one before it;
        backward: bit 1 ties it to the one after it; a last tile that holds position L only never tops a backward run) that stays within
        group_cap bins; gap tiles count no bins, nor do the all-homozygous tiles of the qualifying runs of "hom_tiles" when T % 4 == 0.
      * The runs of a direction are taken longest first (forward: from the start of the head's warm-up to the last tile's end; backward:
        from the end of the top tile's warm-up down to the lowest tile's start; ties in tile order).  A run of at least kc_min tiles,
        kc_min >= 2, is chained while its cost fits what is left of the direction's budget max(64, tiles / kc_div): one per tile that
        needs a matrix of its own, less one, at least 1.  kc_min < 0: 4 (5 beyond 4096 tiles) up to 64 states, 8 (12) beyond.
      * A forward run that starts on its segment's first tile is walked through that tile and chained from its second one (if two
        tiles are left).
      * A chain of `count` tiles applies count - 1 tiles' matrices: forward those of first .. first + count - 2, backward those of
        first + count - 1 down to first + 1.  Gap tiles share one slot per direction when T % 4 == 0, the all-homozygous tiles of
        qualifying runs another; every other tile has its own.
      * Ranges per tile: kc_sub, or by the plan max(1, min(4, (8 T + T + W - 1) / (T + W))), up to 64 states; 1 beyond."""
    glue = np.asarray(glue); cls = np.asarray(cls)
    seg_of, lo, hi, Ls, zero = [], [], [], [], []
    for s, d in enumerate(segs):
        d = np.asarray(d)
        for l, h in tiles_of(len(d), T):
            seg_of.append(s); lo.append(l); hi.append(h); Ls.append(len(d)); zero.append(bool((d[l - 1:h] == 0).all()))
    nc = len(lo)
    assert len(glue) == nc and len(cls) == nc
    hom_shared = [cls[b] == 3 and zero[b] and T % 4 == 0 for b in range(nc)]
    free = [cls[b] == 1 or hom_shared[b] for b in range(nc)]                      # no bins towards group_cap
    shared = [(cls[b] == 1 and T % 4 == 0) or hom_shared[b] for b in range(nc)]   # no matrix of its own
    eff = np.concatenate([[0], np.cumsum([0 if free[b] else hi[b] - lo[b] + 1 for b in range(nc)])])
    span_ok = lambda b, e: eff[e + 1] - eff[b] <= group_cap
    runs_f, runs_b = [], []
    b = 0
    while b < nc:
        e = b + 1
        while e < nc and glue[e] & 1 and seg_of[e] == seg_of[b] and span_ok(b, e):
            e += 1
        if e - b > 1:
            runs_f.append((hi[e - 1] - max(1, lo[b] - W) + 1, b, e - b))
        b = e
    b = 0
    while b < nc:
        e = b + 1
        while e < nc and glue[e - 1] & 2 and seg_of[e] == seg_of[b] and span_ok(b, e) and lo[e] < Ls[e]:
            e += 1
        if e - b > 1:
            runs_b.append((min(hi[e - 1] + W + 1, Ls[b]) - lo[b], b, e - b))
        b = e
    if kc_min < 0:
        kc_min = (12 if nc > 4096 else 8) if n_states > 64 else (5 if nc > 4096 else 4)
    out = ([], [])
    kc, kslot, kuniq = [], [], []
    slot_of = {}

    def push(t, d):
        j = len(kc)
        kc.append((t, d))
        key = (d, "gap") if cls[t] == 1 and T % 4 == 0 else ((d, "hom") if hom_shared[t] else None)
        if key is None or key not in slot_of:
            u = len(kuniq)
            kuniq.append(j)
            if key is not None:
                slot_of[key] = u
        else:
            u = slot_of[key]
        kslot.append(u)

    for d, runs in ((0, runs_f), (1, runs_b)):
        budget = max(64, nc // kc_div)
        for steps, first, count in sorted(runs, key=lambda r: (-r[0], r[1], r[2])):
            cost = max(sum(0 if shared[t] else 1 for t in range(first, first + count)) - 1, 1)
            if not (kc_min >= 2 and count >= kc_min and cost <= budget):
                continue
            budget -= cost
            if d == 0 and lo[first] == 1:
                first, count = first + 1, count - 1
                if count < 2:
                    continue
            out[d].append((first, count))
            for t in (range(first, first + count - 1) if d == 0 else range(first + count - 1, first, -1)):
                push(t, d)
    sub = 1 if n_states > 64 else (kc_sub if kc_sub else max(1, min(4, (8 * T + T + W - 1) // (T + W))))
    glued = tuple(sorted((f, c) for _, f, c in runs) for runs in (runs_f, runs_b))
    return dict(runs=out, kc=kc, kslot=kslot, kuniq=kuniq, sub=sub, glued=glued)


# ------------------------------------------------------------------ inputs
FRONT = 300   # a segment in front of the one under test: tile numbers and offsets are then not the segment's own


def front_segment(src):
    """the last FRONT bins of src with a het bin planted every 7: no tile of it is free of hets, whatever the tile length from 8 on"""
    d = np.asarray(src)[-FRONT:].astype(np.uint8).copy()
    d[3::7] = 1
    return d


def front_tiles(T):
    return (FRONT + T - 1) // T


def base_segment(src, T, n_tiles=49, rest=21):
    return np.asarray(src)[:n_tiles * T + rest].astype(np.uint8).copy()


def gaps_input(src, T, n_tiles=49, rest=21, runs=((5, 12), (30, 33), (40, 41))):
    """[front, long]: n_tiles T + rest bins of src with the whole tiles of `runs` (inclusive) set to missing"""
    d = base_segment(src, T, n_tiles, rest)
    for l, h in runs:
        d[l * T:(h + 1) * T] = MISSING
    return [front_segment(src), d]


def hom_input(src, T, n_tiles=49, rest=21):
    """[front, long]: tiles 20 .. 24 homozygous, three missing bins inside tile 22 (a het-free mix: a matrix of its own)"""
    d = base_segment(src, T, n_tiles, rest)
    d[20 * T:25 * T] = 0
    d[22 * T + 5:22 * T + 8] = MISSING
    return [front_segment(src), d]


def budget_input(src, T=8, n_tiles=150, rest=5):
    """[front, long]: homozygous tiles 1 .. 2 and n_tiles - 3 .. n_tiles - 2: with "hom_tiles", hom_min = 2 T and a warm-up window that
    covers the segment every tile from 2 on is glued forward and every tile up to n_tiles - 3 backward.  Every other tile gets a het
    bin (most 8-bin tiles of the source have none, would be homozygous tiles of qualifying runs themselves and cost nothing of the
    budget): every glued run then holds group_cap bins of tiles that need a matrix each."""
    d = base_segment(src, T, n_tiles, rest)
    d[3::T] = 1
    d[T:3 * T] = 0
    d[(n_tiles - 3) * T:(n_tiles - 1) * T] = 0
    return [front_segment(src), d]


def head_input(src, T, n_tiles=49, rest=21):
    """[front, long]: tiles 1 .. 6 missing -- the forward run starts on the segment's first tile (walked through it, chained from the second)"""
    return gaps_input(src, T, n_tiles, rest, runs=((1, 6),))


def gap_plan(segs, T):
    """(cls, glue) of a plan under "gap_tiles" alone with warm-ups that cover every segment (nothing speculates, nothing is learned): a
    full tile of missing data that is neither first nor last in its segment is a gap tile, glued both ways, and so are the tile behind
    it forward and the tile before it backward"""
    cls, glue = [], []
    for d in segs:
        d = np.asarray(d)
        tl = tiles_of(len(d), T)
        g = [0 < t < len(tl) - 1 and h - l + 1 == T and bool((d[l - 1:h] == MISSING).all()) for t, (l, h) in enumerate(tl)]
        for t in range(len(tl)):
            cls.append(1 if g[t] else 0)
            glue.append((1 if g[t] or (t > 0 and g[t - 1]) else 0) | (2 if g[t] or (t + 1 < len(tl) and g[t + 1]) else 0))
    return np.array(cls, dtype=np.int32), np.array(glue, dtype=np.int32)


# ------------------------------------------------------------------ models
HARSH = {"rho_1e-6": [0.02, 1e-6, 15.0], "tmax_60": [0.02, 0.004, 60.0]}   # the harsh models of tests/test_gpu_wide_gap_chain.py
GOLDEN_MODELS = ("n64_curve", "n64_flat", "n23_curve", "n128_curve")
PSMC_SIZES = (3, 63, 65, 100, 127)
_PAR = {}


def model(golden, name, second=False):
    """(a, e (3, n), a0) of a model by name: the goldens, "psmc<n>" (the host model of the pattern "<n>*1", mild parameters, lambdas
    that vary smoothly), the two harsh 64-state models; second: another parameter set of the same size (the plan stays, the matrices
    move)"""
    from psmc_amd import hostlib
    if (name, second) in _PAR:
        return _PAR[(name, second)]
    if name in GOLDEN_MODELS and not second:
        if name == "n128_curve":
            g = golden.n128
            p = (g[name + ".a"], g[name + ".e"], g[name + ".a0"])
        else:
            q = golden.params(name)
            p = (q["a"], q["e"], q["a0"])
    else:
        n = {"n64_curve": 64, "n64_flat": 64, "n23_curve": 23, "n128_curve": 128}.get(name) or (64 if name in HARSH else int(name[4:]))
        if second:
            p = hostlib.hmm_params("%d*1" % n, [0.025, 0.005, 12.0] + list(1.0 + 0.5 * np.cos(0.23 * np.arange(n))))
        elif name in HARSH:
            p = hostlib.hmm_params("64*1", HARSH[name] + [1.0] * 64)
        else:
            p = hostlib.hmm_params("%d*1" % n, [0.02, 0.004, 15.0] + list(1.0 + 0.6 * np.sin(0.37 * np.arange(n))))
    _PAR[(name, second)] = p
    return p
