"""numpy restatement of the Viterbi arithmetic psmc_hip_viterbi pins (include/psmc_hip.h; khmm.c:83-141).

Log tables by math.log -- libm's log(), one call per entry; numpy's vector log need not round as libm does.  Every
candidate V[l] + la[k][l] is one IEEE addition; the first maximum wins (np.argmax returns the first), a NaN never
does, and a state that no candidate lifts above -1e300 raises NoFinitePath, where the reference's assert fires."""
import math
import numpy as np


class NoFinitePath(ValueError):
    pass


def _log(x):
    return math.log(x) if x > 0 else -math.inf


def log_tables(a, e, a0):
    """la[k, l] = log a[l, k]; le (3, n) with le[2] = 0; l0 (n,)"""
    a = np.asarray(a, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    n = a.shape[0]
    la = np.array([[_log(a[l, k]) for l in range(n)] for k in range(n)], dtype=np.float64).reshape(n, n)
    le = np.zeros((3, n))
    for b in range(2):
        le[b] = [_log(x) for x in e[b]]
    l0 = np.array([_log(x) for x in np.asarray(a0, dtype=np.float64)], dtype=np.float64)
    return la, le, l0


def _rule(c, axis=-1):
    """khmm.c's loop over the last axis: (max, arg) with m = -1e300, arg = -1 to start from and `if (m < c)`."""
    with np.errstate(invalid="ignore"):
        ok = c > -1e300                       # a NaN and -inf never win
    cc = np.where(ok, c, -np.inf)
    arg = np.argmax(cc, axis=axis)            # the first among equal maxima
    m = np.take_along_axis(cc, np.expand_dims(arg, axis), axis).squeeze(axis)
    none = ~ok.any(axis=axis)
    return np.where(none, -1e300, m), np.where(none, -1, arg)


def viterbi(tables, seq):
    """(path int32 (L,), score) of one segment; tables = log_tables(a, e, a0); seq: symbols 0 / 1 / 2"""
    la, le, l0 = tables
    seq = np.asarray(seq)
    L, n = len(seq), len(l0)
    bp = np.zeros((L, n), dtype=np.int32)
    with np.errstate(invalid="ignore"):
        V = le[seq[0]] + l0
        for u in range(1, L):
            m, arg = _rule(V[None, :] + la)   # [k, l]: one rounded addition each
            if (arg < 0).any():
                raise NoFinitePath("position %d" % (u + 1))
            bp[u] = arg
            V = le[seq[u]] + m
    score, s = _rule(V)
    if s < 0:
        raise NoFinitePath("end")
    path = np.empty(L, dtype=np.int32)
    for u in range(L - 1, -1, -1):
        path[u] = s
        s = bp[u, s]
    return path, float(score)


def runs(path):
    """[(start, end, state)]: maximal runs of equal states, 0-based inclusive"""
    path = np.asarray(path)
    cut = np.flatnonzero(np.diff(path)) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut - 1, [len(path) - 1]])
    return [(int(s), int(t), int(path[s])) for s, t in zip(starts, ends)]
