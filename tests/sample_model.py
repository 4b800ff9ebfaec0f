"""A numpy restatement of the posterior path sampling that include/psmc_hip.h pins (psmc_hip_sample_paths): forward filtering with
hmm_forward's arithmetic (khmm.c:170-185), a counter-based generator on 64-bit unsigned integers, and the draw "number of l with
c_l < r * c_{n-1}" over the ordered running sum c.  TEST INFRASTRUCTURE: np.cumsum is the ordered running sum (each entry is the one
before plus one term, from the first term on -- 0.0 + w_0 is w_0), uint64 array arithmetic is the generator, (c < x).sum() is the
draw.  Nothing here is fused: numpy multiplies, then adds."""
import numpy as np

GOLD = np.uint64(0x9e3779b97f4a7c15)
_M1 = np.uint64(0xbf58476d1ce4e5b9)
_M2 = np.uint64(0x94d049bb133111eb)


def mix(z):
    """z: uint64 array (any shape); arithmetic wraps modulo 2^64"""
    z = np.array(z, dtype=np.uint64, ndmin=1)
    z = z ^ (z >> np.uint64(30))
    z = z * _M1
    z = z ^ (z >> np.uint64(27))
    z = z * _M2
    return z ^ (z >> np.uint64(31))


def u64(x):
    return np.array([int(x) & (2 ** 64 - 1)], dtype=np.uint64)


def uniforms(seed, j, q, L):
    """r[u - 1] for u = 1..L of sample j (0-based) and stream id q: in (0, 1]"""
    key = mix(mix(u64(seed) + GOLD * u64(j + 1)) + GOLD * u64(q + 1))
    z = mix(key + GOLD * np.arange(1, L + 1, dtype=np.uint64))
    return ((z >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53


def forward(a, e, a0, seq):
    """f (L, n): row u - 1 is f_u, normalised.  e: (2, n) or (3, n); the missing symbol has emission 1."""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    em = np.vstack([np.asarray(e, dtype=np.float64)[:2], np.ones((1, n))])
    f = np.zeros((len(seq), n))
    at = np.ascontiguousarray(a.T)                       # at[k, l] = a[l][k] (khmm.c:162-166)
    prod = np.empty((n, n))
    for u, sym in enumerate(seq):
        if u == 0:
            g = np.asarray(a0, dtype=np.float64) * em[sym]
        else:
            np.multiply(at, f[u - 1][None, :], out=prod)  # prod[k, l] = f_{u-1}[l] * a[l][k], rounded once
            np.cumsum(prod, axis=1, out=prod)             # the terms added in ascending l (in place: one buffer for all positions)
            g = em[sym] * prod[:, -1]                     # tmp_k
        f[u] = g / np.cumsum(g)[-1]
    return f


def draw(w, r):
    c = np.cumsum(w)
    total = c[-1]
    if not (total > 0.0 or total < 0.0):                 # 0 or NaN
        return 0
    return min(int((c < r * total).sum()), len(w) - 1)


def walk(a, f, r):
    """one path from the forward vectors f (L, n) and the uniforms r (L,)"""
    L = f.shape[0]
    path = np.zeros(L, dtype=np.int32)
    s = draw(f[L - 1], r[L - 1])
    path[L - 1] = s
    for u in range(L - 1, 0, -1):                        # position u, 1-based
        s = draw(f[u - 1] * a[:, s], r[u - 1])
        path[u - 1] = s
    return path


def sample(a, e, a0, seq, seed, j, q, f=None):
    a = np.asarray(a, dtype=np.float64)
    if f is None:
        f = forward(a, e, a0, seq)
    return walk(a, f, uniforms(seed, j, q, len(seq)))


def sample_segments(a, e, a0, segs, seed, n_samp, stream=None, first=0):
    """paths[j][i]: sample first + j of segment i; stream: one id per segment (None: its index)"""
    a = np.asarray(a, dtype=np.float64)
    fs = [forward(a, e, a0, s) for s in segs]
    ids = list(range(len(segs))) if stream is None else [int(x) for x in stream]
    return [[walk(a, f, uniforms(seed, first + j, q, len(s))) for f, s, q in zip(fs, segs, ids)] for j in range(n_samp)]


def runs(path):
    """[(start, end, state)], 0-based inclusive"""
    cut = np.flatnonzero(np.diff(path)) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut - 1, [len(path) - 1]])
    return [(int(s), int(t), int(path[s])) for s, t in zip(starts, ends)]
