"""What "fast mode agrees with exact mode" means, in numbers (tests/ and bench.py; not part of the E-step path).

The gate of the fast kernels has been max|x - ref| / max|ref| <= 1e-10 over the whole count matrix -- silent about small cells.
The M-step reads the counts through hmm_Q (khmm.c:363-382): Q = sum_kl A[k][l] log a[k][l] + sum_bk E[b][k] log e[b][k], so what
matters downstream is (i) the element-wise relative error of the cells that carry weight and (ii) the error of those two sums.
"""
import numpy as np


def fast_error_metrics(r, o, a=None, e=None, floor=1e-6):
    """r, o: dicts with A (n, n), E (2, n), LL -- a fast result and its exact / oracle reference.  Returns
    A_max, E_max   max |x - ref| / max |ref|                      (the gate since round 1)
    A_cell, E_cell largest RELATIVE error over the cells >= floor x the largest cell
    A_l1           sum |A - ref| / sum |ref|: bounds the error of any linear functional sum w A by max |w| x this x sum |ref|
    LL             relative
    QA, QE         (when a, e are given) relative error of sum A log a and of sum E log e, the two sums hmm_Q consumes"""
    A, Ao = np.asarray(r["A"], float), np.asarray(o["A"], float)
    E, Eo = np.asarray(r["E"], float)[:2], np.asarray(o["E"], float)[:2]
    m = dict(A_max=float(np.abs(A - Ao).max() / np.abs(Ao).max()), E_max=float(np.abs(E - Eo).max() / np.abs(Eo).max()))
    big = Ao >= floor * Ao.max()
    m["A_cell"] = float((np.abs(A - Ao)[big] / Ao[big]).max())
    bigE = Eo >= floor * Eo.max()
    m["E_cell"] = float((np.abs(E - Eo)[bigE] / Eo[bigE]).max())
    m["A_l1"] = float(np.abs(A - Ao).sum() / np.abs(Ao).sum())
    m["LL"] = float(abs(r["LL"] - o["LL"]) / abs(o["LL"]))
    if a is not None and e is not None:
        a = np.asarray(a, float); e2 = np.asarray(e, float)[:2]
        pa, pe = a > 0, e2 > 0
        qa_ref, qe_ref = float((Ao[pa] * np.log(a[pa])).sum()), float((Eo[pe] * np.log(e2[pe])).sum())
        m["QA"] = abs(float((A[pa] * np.log(a[pa])).sum()) - qa_ref) / abs(qa_ref)
        m["QE"] = abs(float((E[pe] * np.log(e2[pe])).sum()) - qe_ref) / abs(qe_ref)
    return m


FACTORED_NAMES = ("SL", "SU", "DG", "CL", "CU", "E0", "E1")


def tri_sums(A):
    """SL, SU, DG, CL, CU (5, n) of a count matrix: what psmc_hip_estep_factored returns in place of A."""
    A = np.asarray(A, float)
    lo, up = np.tril(A, -1), np.triu(A, 1)
    return np.stack([lo.sum(1), up.sum(1), np.diag(A).copy(), lo.sum(0), up.sum(0)])


def log_factors(a):
    """The five log factors the O(N) objective multiplies the triangular sums with (psmc_amd/host/mstep.c neg_Q_fast):
    log a[k][l] = log P_k + log qa_l (l < k), log R_k + log c_l (l > k), log a[k][k]; (5, n), 0 where a factor does not exist
    (P_0, R_{n-1}, qa_{n-1}, c_0: their sums are empty).  Plain divisions, no check of the form: see api.hip factor_structure."""
    a = np.asarray(a, float)
    n = a.shape[0]
    f = np.ones((5, n))
    f[0, 1:] = a[1:, 0]; f[1, :n - 1] = a[:n - 1, n - 1]; f[2] = np.diag(a)
    f[3, :n - 1] = a[n - 1, :n - 1] / a[n - 1, 0]; f[4, 1:] = a[0, 1:] / a[0, n - 1]
    return np.log(np.where(f > 0, f, 1.0))


def factored_error_metrics(r, o, a=None, e=None, floor=1e-6):
    """r, o: dicts with sums (5, n) = SL | SU | DG | CL | CU, E (2, n), LL -- a factored fast result and its reference.  The
    block gate (sums_max, E_max: max |x - ref| / max |ref| over all of sums, all of E) is scaled by the diagonal count of the
    most occupied state and says nothing about the other vectors or about weakly occupied states, so for each of the seven
    vectors V in FACTORED_NAMES SEPARATELY:
    V_cell  largest RELATIVE error over the cells >= floor x that vector's own largest cell
    V_l1    sum |x - ref| / sum |ref| of that vector
    and LL (relative), QA, QE (when a, e are given): the relative error of sum sums . log_factors(a) and of sum E log e, the two
    sums neg_Q_fast reads."""
    S, So = np.asarray(r["sums"], float), np.asarray(o["sums"], float)
    E, Eo = np.asarray(r["E"], float)[:2], np.asarray(o["E"], float)[:2]
    m = dict(sums_max=float(np.abs(S - So).max() / max(np.abs(So).max(), 1e-300)),
             E_max=float(np.abs(E - Eo).max() / max(np.abs(Eo).max(), 1e-300)))
    for name, x, ref in zip(FACTORED_NAMES, list(S) + list(E), list(So) + list(Eo)):
        big = (ref >= floor * ref.max()) & (ref > 0)
        m[name + "_cell"] = float((np.abs(x - ref)[big] / ref[big]).max()) if big.any() else 0.0
        tot = float(np.abs(ref).sum())
        m[name + "_l1"] = float(np.abs(x - ref).sum() / tot) if tot > 0 else float(np.abs(x - ref).sum())
    m["LL"] = float(abs(r["LL"] - o["LL"]) / max(abs(o["LL"]), 1e-300))
    if a is not None and e is not None:
        lf = log_factors(a)
        e2 = np.asarray(e, float)[:2]
        pe = e2 > 0
        qa_ref, qe_ref = float((So * lf).sum()), float((Eo[pe] * np.log(e2[pe])).sum())
        m["QA"] = abs(float((S * lf).sum()) - qa_ref) / max(abs(qa_ref), 1e-300)
        m["QE"] = abs(float((E[pe] * np.log(e2[pe])).sum()) - qe_ref) / max(abs(qe_ref), 1e-300)
    return m
