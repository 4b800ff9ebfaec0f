"""numpy model of the FAST-mode E-step algorithm (tiled sweeps: speculate,
verify at the tile boundaries, repair only where the chain had not forgotten
its start; lagged normalisation; counts as a GEMM over bins).

TEST INFRASTRUCTURE: an executable specification of what the fast HIP kernels
(psmc_amd/csrc/estep_fast.hip) compute, used on CPU to check the algebra
against the oracle and to study tolerance / work as a function of the tile
length T, the speculative warm-up W0 and the tolerances.  Not imported by the
product.

Notation (1-indexed positions p=1..L, o_p the observation):
  forward  X_p = e[o_p] * (a^T X_{p-1}) / d_p ,  d_p = sum(X_{p-1}) if p % NORM_EVERY == 0 else 1
           (LL = sum_p log d_p + log sum(X_L) telescopes for any positive d_p)
  backward bt_p = e[o_p] * (a bt_{p+1}) * sb_p,  sb_p = 1/sum(bt_{p+1}) if p % NORM_EVERY == 0 else 1
           (independent of the forward tables: the two sweeps run concurrently)
  counts   G_p = sum_k X_p bt_p / e[o_p]                    (posterior normaliser, per position)
           C  += (sb_p / G_p) X_p (x) bt_{p+1}             p = 1..L-1   (A = a .* C)
           E[o_p] += X_p * bt_p / e[o_p] / G_p               p = 1..L-1
Speculation: a tile [lo,hi] starts W0 bins outside itself from an arbitrary
vector.  Verification compares the vector a tile used at its boundary with the
value its neighbour computed with a whole tile of history behind it; tiles
whose mismatch exceeds `tol` are re-run from the neighbour's value until the new
trajectory meets the stored one to `tol` again (or the tile ends, which may make
the next tile dirty).  Both sweeps are self-normalising, so stored vectors of
neighbouring tiles agree in scale as well as in direction.
"""
import numpy as np

TINY = 1e-25
NORM_EVERY = 4  # psmc_hip_internal.h


def plan_chunks(L, T):
    """[(lo, hi)] tiles of 1..L of length T (last one shorter)."""
    out = []
    lo = 1
    while lo <= L:
        hi = min(L, lo + T - 1)
        out.append((lo, hi))
        lo = hi + 1
    return out


def _relmax(x, y):
    return np.abs(x - y).max() / np.abs(y).max()


def estep_fast_model(a, e, a0, segs, T=4096, W=2048, tol=None, stats=None, struct=False):
    """tol=None: pure warm-up tiling (no verification).  tol=float: speculate with W, verify, repair.
    struct=True: the products a^T x and a bt of both sweeps go through the O(N) two-scan steps of factor_structure(a) (below), as the
    structured kernels form them -- the model then shares the 64 ulp per entry of a the factorisation criterion admits; where the
    criterion refuses the matrix the dense products stay.  The counts read a itself either way (A = a .* C)."""
    n = a.shape[0]
    f = factor_structure(a) if struct else None
    fwd = (lambda x: x @ a) if f is None else (lambda x: struct_step_forward(f, x))
    bwd = (lambda z: a @ z) if f is None else (lambda z: struct_step_backward(f, z))
    A = np.zeros((n, n)); E = np.zeros((3, n)); LL = 0.0
    work = dict(fwd_steps=0, bwd_steps=0, fwd_rounds=0, bwd_rounds=0, bins=0)
    for seg in segs:
        seg = np.asarray(seg, dtype=np.int64)
        L = len(seg)
        work["bins"] += L
        o = np.concatenate([[2], seg, [2]])  # o[p], p=1..L
        tiles = plan_chunks(L, T)
        nc = len(tiles)
        X = np.zeros((L + 2, n)); d = np.ones(L + 2); bt = np.zeros((L + 2, n))

        def fstep(x, p):
            dp = x.sum() if p % NORM_EVERY == 0 else 1.0
            g = (x * e[o[p]]) if p == 1 else e[o[p]] * fwd(x)
            return g / dp, dp

        # ---------------- forward: speculative pass
        entry = [None] * nc
        for c, (lo, hi) in enumerate(tiles):
            ws = max(1, lo - W)
            x = a0.copy()
            for p in range(ws, hi + 1):
                if p == lo:
                    entry[c] = x.copy()
                x, dp = fstep(x, p)
                work["fwd_steps"] += 1
                if p >= lo:
                    X[p] = x; d[p] = dp
        # ---------------- forward: verify / repair rounds
        if tol is not None:
            while True:
                dirty = [c for c in range(1, nc) if _relmax(entry[c], X[tiles[c][0] - 1]) > tol]
                if not dirty:
                    break
                work["fwd_rounds"] += 1
                for c in dirty:
                    lo, hi = tiles[c]
                    x = X[lo - 1].copy(); entry[c] = x.copy()
                    for p in range(lo, hi + 1):
                        xn, dp = fstep(x, p)
                        work["fwd_steps"] += 1
                        done = _relmax(xn, X[p]) <= tol
                        X[p] = xn; d[p] = dp; x = xn
                        if done:
                            break
        LL += np.log(d[2:L + 1]).sum() + np.log(X[L].sum())

        # ---------------- backward: independent of the forward tables (own lagged scaling)
        sb = np.ones(L + 2)

        def bstep(btn, p):  # consumes bt_{p+1}; returns bt_p and the scale it applied
            sp = 1.0 / btn.sum() if p % NORM_EVERY == 0 else 1.0
            return e[o[p]] * bwd(btn) * sp, sp

        bentry = [None] * nc; bexit = [None] * nc
        for c, (lo, hi) in enumerate(tiles):
            top = min(hi, L - 1)
            if top < lo:
                continue
            q = min(hi + W + 1, L)
            btn = e[o[q]] * np.ones(n)
            for p in range(q - 1, lo - 1, -1):
                if p == top:
                    bt[top + 1] = btn; bentry[c] = btn.copy()
                btn, sp = bstep(btn, p)
                work["bwd_steps"] += 1
                if p <= top:
                    sb[p] = sp
                    if p > lo or p == 1:
                        bt[p] = btn
                    if p == lo:
                        bexit[c] = btn.copy()
        if tol is not None:
            while True:
                dirty = [c for c in range(nc - 1)
                         if bexit[c + 1] is not None and bentry[c] is not None
                         and tiles[c][1] + W + 1 < L and _relmax(bentry[c], bexit[c + 1]) > tol]
                if not dirty:
                    break
                work["bwd_rounds"] += 1
                for c in dirty:
                    lo, hi = tiles[c]
                    top = min(hi, L - 1)
                    btn = bexit[c + 1].copy(); bentry[c] = btn.copy()
                    bt[top + 1] = btn
                    for p in range(top, lo - 1, -1):
                        btn, sp = bstep(btn, p)
                        work["bwd_steps"] += 1
                        sb[p] = sp
                        if p > lo:
                            done = _relmax(btn, bt[p]) <= tol
                            bt[p] = btn
                            if done:
                                break
                        else:
                            bexit[c] = btn.copy()
                            if p == 1:
                                bt[1] = btn
        # ---------------- counts (GEMM over bins) from the stored tables, normalised per position:
        #   G_p = sum_k X_p bt_p / e[o_p]   (= sb_p * sum_kl X_p[k] a[k][l] bt_{p+1}[l])
        #   gamma_p = X_p bt_p / e[o_p] / G_p ;  xi_p = (sb_p / G_p) X_p (x) bt_{p+1} .* a
        if L > 1:
            re = np.where(e > 0, 1.0 / np.where(e > 0, e, 1.0), 0.0)
            g = X[1:L] * bt[1:L] * re[seg[:L - 1]]
            G = g.sum(1)
            C = (X[1:L] * (sb[1:L] / G)[:, None]).T @ bt[2:L + 1]
            A += a * C
            S = np.zeros((3, n))
            gam = g / G[:, None]
            for b in range(3):
                S[b] = gam[seg[:L - 1] == b].sum(0)
            E += S
        A += TINY; E += TINY
    if stats is not None:
        stats.update(work)
    return dict(A=A, E=E[:2].copy(), LL=LL)


# ---------------------------------------------------------------------------------------------
# Structured O(N) sweeps (psmc_amd/csrc/estep_struct.hip, api.hip factor_structure): numpy mirror.
def factor_structure(a, ulps=64):
    """a[k][l] = P_k qa_l (l<k), R_k c_l (l>k) with qa_0 = c_{n-1} = 1, dd = diag - P.qa - R.c >= 0,
    every off-diagonal entry checked to `ulps`; returns None when the matrix does not have the form
    (lh3/psmc core.c:112-122 builds it this way; psmc_cap_matrix, aux.c:115-127, destroys it)."""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    if n < 3 or not (a[n - 1, 0] > 1e-280 and a[0, n - 1] > 1e-280):
        return None
    P = np.zeros(n); R = np.zeros(n); qa = np.zeros(n); c = np.zeros(n)
    qa[:n - 1] = a[n - 1, :n - 1] / a[n - 1, 0]
    P[1:] = a[1:, 0]
    c[1:] = a[0, 1:] / a[0, n - 1]
    R[:n - 1] = a[:n - 1, n - 1]
    w = np.where(np.tri(n, k=-1, dtype=bool), np.outer(P, qa), np.outer(R, c))
    off = ~np.eye(n, dtype=bool)
    if not np.all(np.abs(a - w)[off] <= ulps * 2.220446049250313e-16 * np.abs(a)[off] + 1e-290):
        return None
    dd = np.diag(a) - P * qa - R * c
    if not np.all(dd >= 0):
        return None
    return dict(P=P, R=R, qa=qa, c=c, dd=dd)


def struct_step_forward(f, x):
    """(a^T x)_j = qa_j SUF_j(x.P) + c_j PRE_j(x.R) + dd_j x_j, inclusive suffix / prefix sums."""
    return f["qa"] * np.cumsum((x * f["P"])[::-1])[::-1] + f["c"] * np.cumsum(x * f["R"]) + f["dd"] * x


def struct_step_backward(f, z):
    """(a z)_k = R_k SUF_k(z.c) + P_k PRE_k(z.qa) + dd_k z_k."""
    return f["R"] * np.cumsum((z * f["c"])[::-1])[::-1] + f["P"] * np.cumsum(z * f["qa"]) + f["dd"] * z


# ---------------------------------------------------------------------------------------------
# The reference figure of the per-cell gates (tests/test_gpu_fast_cells.py): how far two float64 evaluations of the same E-step are apart.
CELL_FLOOR = 2.0 ** -900   # an oracle value above this is compared relatively, whatever its size against the largest
ULP64 = 64 * 2.0 ** -53    # the factorisation criterion's allowance per entry of a


def cell_error(x, ref):
    """(worst relative error over the entries of ref above CELL_FLOOR, the index of that entry); (0.0, None) when there is none"""
    x, ref = np.asarray(x, float), np.asarray(ref, float)
    big = ref > CELL_FLOOR
    if not big.any():
        return 0.0, None
    err = np.where(big, np.abs(x - ref) / np.where(big, ref, 1.0), 0.0)
    i = np.unravel_index(int(np.argmax(err)), err.shape)
    return float(err[i]), tuple(int(j) for j in i)


def tri_sums(A):
    """SL, SU, DG, CL, CU (5, n) of a count matrix (psmc_amd/parity.py tri_sums)"""
    A = np.asarray(A, float)
    lo, up = np.tril(A, -1), np.triu(A, 1)
    return np.stack([lo.sum(1), up.sum(1), np.diag(A).copy(), lo.sum(0), up.sum(0)])


def reference_error(a, e, a0, segs, o):
    """E_ref of an input: o is the oracle's result on it.  The untiled model (one tile per segment, nothing speculated) with the dense
    products and with the structured ones, each against the oracle; of the two the larger worst relative error
      cell: over every cell of A and every entry of E[0], E[1] above CELL_FLOOR,
      tri:  over every entry of the five triangular sums of A above CELL_FLOOR,
    and the models' relative distance in LL.  dict(cell, tri, LL, dense = (cell, tri), struct = (cell, tri))."""
    out = {}
    for key, st in (("dense", False), ("struct", True)):
        m = estep_fast_model(a, e, a0, segs, T=1 << 30, W=0, struct=st)
        out[key] = (max(cell_error(m["A"], o["A"])[0], cell_error(m["E"], o["E"])[0]), cell_error(tri_sums(m["A"]), tri_sums(o["A"]))[0])
        out[key + "_LL"] = abs(m["LL"] - o["LL"]) / abs(o["LL"])
    out["cell"] = max(out["dense"][0], out["struct"][0])
    out["tri"] = max(out["dense"][1], out["struct"][1])
    out["LL"] = max(out["dense_LL"], out["struct_LL"])
    return out


def cell_bound(e_ref, margin=32):
    """B of the per-cell gates: margin x max(E_ref, 64 ulp)"""
    return margin * max(e_ref, ULP64)


# ---------------------------------------------------------------------------------------------
# Decoding from the fast tables (psmc_amd/csrc/estep_post_fast.hip, estep_wide_post.hip): the formulas of that file's header, untiled, and the
# reference figure of the per-entry gates of tests/test_gpu_decode_cells.py.
DECODE_OUTPUTS = ("post", "maxp", "recomb", "scales", "counts", "mean")
N_CNT = (1, 5, 9)          # count columns of the post_counts calls: nine cross both PCNT_J = 8 and CB = 4


def decode_model(a, e, a0, seg, struct=False):
    """Every decoding output of one segment from the tables of an untiled fast E-step (one tile, nothing speculated; the conventions of
    estep_fast_model: lag-4 normalisation of both sweeps, position L on its own formula).  dict(
      post   (L, n)  gamma_p = X_p bt_p / e[o_p] / G_p for p < L, gamma_L = X_L / sum X_L,
      recomb (L,)    1 - sb_p sum_l X_p(l) a_ll bt_{p+1}(l) / G_p, 0 at p = L,
      path, maxp     the first maximum of every row and its value,
      scales (L,)    s_1 = sum a0 e[o_1], s_p = sum X_p / sum X_{p-1} * d_p).
    struct=True: the products of both sweeps through the two-scan steps of factor_structure(a); None where the criterion refuses a."""
    n = a.shape[0]
    f = factor_structure(a) if struct else None
    if struct and f is None:
        return None
    fwd = (lambda x: x @ a) if f is None else (lambda x: struct_step_forward(f, x))
    bwd = (lambda z: a @ z) if f is None else (lambda z: struct_step_backward(f, z))
    seg = np.asarray(seg, dtype=np.int64)
    L = len(seg)
    o = np.concatenate([[2], seg, [2]])  # o[p], p=1..L
    X = np.zeros((L + 2, n)); d = np.ones(L + 2); bt = np.zeros((L + 2, n)); sb = np.ones(L + 2)
    x = a0
    for p in range(1, L + 1):
        dp = x.sum() if p % NORM_EVERY == 0 else 1.0
        x = ((x * e[o[p]]) if p == 1 else e[o[p]] * fwd(x)) / dp
        X[p] = x; d[p] = dp
    bt[L] = e[o[L]] * np.ones(n)
    for p in range(L - 1, 0, -1):
        sb[p] = 1.0 / bt[p + 1].sum() if p % NORM_EVERY == 0 else 1.0
        bt[p] = e[o[p]] * bwd(bt[p + 1]) * sb[p]
    post = np.zeros((L, n)); recomb = np.zeros(L); scales = np.zeros(L)
    if L > 1:
        re = np.where(e > 0, 1.0 / np.where(e > 0, e, 1.0), 0.0)
        g = X[1:L] * bt[1:L] * re[seg[:L - 1]]
        G = g.sum(1)
        post[:L - 1] = g / G[:, None]
        recomb[:L - 1] = 1.0 - sb[1:L] * (X[1:L] * np.diag(a) * bt[2:L + 1]).sum(1) / G
    post[L - 1] = X[L] / X[L].sum()
    sx = X[1:L + 1].sum(1)
    scales[0] = (a0 * e[o[1]]).sum()
    scales[1:] = sx[1:] / sx[:-1] * d[2:L + 1]
    return dict(post=post, recomb=recomb, path=post.argmax(1).astype(np.int32), maxp=post.max(1), scales=scales)


def decode_weights(n, t_max, alpha=0.1):
    """(4, n) non-negative post_mean weights: the host model's t_k = alpha (exp(k / n ln(1 + t_max / alpha)) - 1) (the interval boundaries of
    lh3/psmc core.c:70-72), t_k^2, the indicator k >= n // 2, all ones"""
    k = np.arange(n, dtype=np.float64)
    t = alpha * (np.exp(k / n * np.log(1.0 + t_max / alpha)) - 1.0)
    return np.ascontiguousarray(np.stack([t, t * t, (np.arange(n) >= n // 2).astype(np.float64), np.ones(n)]))


def count_lengths(segs):
    """l of every segment's count record: L, except
      segment 1: L - 3 and segment 2: L + 5 (as compare_decoding of tests/test_gpu_fast_decode.py has them; on segments of 2 and 3 bins: an
                 empty record, for which the call returns before any launch, and one longer than a single tile),
      segment 7: L - 3 and segment 8: L + 5 (the 129-bin segment and the 1000- or 300-bin one: records shorter and longer than a segment of
                 several tiles; 126 ends inside a tile at chunk 37, 64 and 256 and inside a block of eight rows, and with chunk 64 the last tile,
                 which holds position L alone, counts nothing),
      the last segment: L // 2 + 1 (151 of 300: mid-tile and mid-block again, and every later tile counts nothing),
      a segment of more than 2048 bins: 2051 (three positions into the second block of PCNT_BLK = 2048)."""
    out = []
    for i, s in enumerate(segs):
        L = len(s)
        l = L - 3 if i in (1, 7) else L + 5 if i in (2, 8) else L // 2 + 1 if i == len(segs) - 1 and i > 8 else 2051 if L > 2048 else L
        out.append(max(0, l))
    return out


def count_tables(segs, seed=1):
    """{n_cnt: [cnt1 of every segment]} for n_cnt of N_CNT: rng.integers(0, 50), (l, n_cnt) int32 with l of count_lengths(segs)"""
    rng = np.random.default_rng(seed)
    return {j: [rng.integers(0, 50, size=(l, j), dtype=np.int32) for l in count_lengths(segs)] for j in N_CNT}


def add_counts(cnt, post, cnt1):
    """cnt (n, n_cnt) += sum over the first min(L, l) positions of post_p (x) cnt1_p (aux.c:202-219)"""
    m = min(len(post), len(cnt1))
    cnt += post[:m].T @ cnt1[:m].astype(np.float64)
    return cnt


def long_mean(post, w):
    """(L, n_w): post @ w^T in numpy.longdouble, rounded to double once"""
    return (post.astype(np.longdouble) @ np.asarray(w).astype(np.longdouble).T).astype(np.float64)


def top_two_gap(post):
    """per row of post: (largest - second largest) / largest; 1 for a single state"""
    if post.shape[1] < 2:
        return np.ones(len(post))
    top = np.partition(post, post.shape[1] - 2, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) / top[:, 1]


def decode_oracle(a, e, a0, segs, oracle, w, tables):
    """The oracle's decoding outputs of every segment: dict(post, recomb, path, maxp, scales, mean: lists per segment; counts: {n_cnt: (n,
    n_cnt)} running totals over all segments of `tables` (count_tables), counts_seg: {n_cnt: [(n, n_cnt) of every segment alone]}; gap: the smallest relative top-two gap of any posterior row)"""
    n = a.shape[0]
    out = dict(post=[], recomb=[], path=[], maxp=[], scales=[], mean=[], counts={j: np.zeros((n, j)) for j in tables},
               counts_seg={j: [] for j in tables}, gap=1.0)
    for i, seg in enumerate(segs):
        f, b, s, lk, chk = oracle.fwd_bwd(a, e, a0, seg)
        post, rec = oracle.post_full(a, e, seg, f, b, s)
        path, mp = oracle.post_decode(f, b, s)
        out["post"].append(post[1:].copy()); out["recomb"].append(rec[1:].copy()); out["path"].append(path[1:].copy())
        out["maxp"].append(mp[1:].copy()); out["scales"].append(s[1:].copy()); out["mean"].append(long_mean(post[1:], w))
        for j in tables:
            oracle.post_counts(f, b, s, tables[j][i], out["counts"][j])
            out["counts_seg"][j].append(oracle.post_counts(f, b, s, tables[j][i], np.zeros((n, j))))
        out["gap"] = min(out["gap"], float(top_two_gap(post[1:]).min()))
    return out


def decode_reference_error(a, e, a0, segs, oracle, w=None, ref=None):
    """E_ref of the decoding outputs, the counterpart of reference_error: decode_model with the dense and with the structured products
    (skipped where factor_structure refuses a), each against the oracle; of the two the larger of
      post    worst relative error over the entries whose oracle value is above CELL_FLOOR,
      maxp, scales  relative,
      recomb  ABSOLUTE (it is 1 - x with x near 1: its error is that of x),
      counts  relative over the cells of orc.post_counts above CELL_FLOOR, for count_tables(segs): of every segment alone and of the running
              totals over all segments,
      mean    relative, per column, against post_oracle @ w in numpy.longdouble (w: decode_weights(n, 15) unless given),
    and: ties = positions where a model's path differs from the oracle's, gap = the smallest relative top-two gap of the oracle's posterior,
    rowsum = the largest |sum of a model row - 1|, below = the largest model entry where the oracle is at or below CELL_FLOOR.
    ref: decode_oracle's result when the caller has it already."""
    n = a.shape[0]
    w = decode_weights(n, 15.0) if w is None else w
    tables = count_tables(segs)
    ref = decode_oracle(a, e, a0, segs, oracle, w, tables) if ref is None else ref
    out = dict(ties=0, gap=ref["gap"], rowsum=0.0, below=0.0)
    for key, st in (("dense", False), ("struct", True)):
        if st and factor_structure(a) is None:
            continue
        err = dict.fromkeys(DECODE_OUTPUTS, 0.0)
        cnt = {j: np.zeros((n, j)) for j in tables}
        for i, seg in enumerate(segs):
            m = decode_model(a, e, a0, seg, struct=st)
            err["post"] = max(err["post"], cell_error(m["post"], ref["post"][i])[0])
            err["maxp"] = max(err["maxp"], cell_error(m["maxp"], ref["maxp"][i])[0])
            err["scales"] = max(err["scales"], cell_error(m["scales"], ref["scales"][i])[0])
            err["recomb"] = max(err["recomb"], float(np.abs(m["recomb"] - ref["recomb"][i]).max()))
            err["mean"] = max(err["mean"], cell_error(m["post"] @ w.T, ref["mean"][i])[0])
            out["ties"] += int((m["path"] != ref["path"][i]).sum())
            out["rowsum"] = max(out["rowsum"], float(np.abs(m["post"].sum(1) - 1.0).max()))
            small = ref["post"][i] <= CELL_FLOOR
            if small.any():
                out["below"] = max(out["below"], float(m["post"][small].max()))
            for j in tables:
                add_counts(cnt[j], m["post"], tables[j][i])
                err["counts"] = max(err["counts"], cell_error(add_counts(np.zeros((n, j)), m["post"], tables[j][i]), ref["counts_seg"][j][i])[0])
        err["counts"] = max([err["counts"]] + [cell_error(cnt[j], ref["counts"][j])[0] for j in tables])
        out[key] = err
    for k in DECODE_OUTPUTS:
        out[k] = max(out[key][k] for key in ("dense", "struct") if key in out)
    return out
