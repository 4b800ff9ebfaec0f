"""Generate tests/golden/exact_extremes.npz by driving the REAL reference's E-step (hmm_forward, hmm_backward, hmm_expect and
hmm_add_expect of khmm.c as em.c:33-55 calls them) through tests/orc.py Reference on oracle/_ref/libpsmc_ref.so (`make -C oracle
ref`): the statistics under the thirteen extreme PSMC models of tests/test_gpu_wide_fast_edges.py MODELS and the four synthetic
matrices of tests/exact_extremes.py at 64, 65 and 200 states, on exact_extremes.segments (thirteen segments, 1195 bins).  Data only.

Keys, per case "n<states>.<model>": `.E` (2, n), `.A0` (n,), `.LL` (1,), `.seg_LL` and `.seg_chk` (one per segment) as the raw bits of
the doubles (uint64: NaN signs and payloads are part of the golden), `.A_sha256` and `.seg_A_sha256`: the SHA-256 of the bytes of
A (n, n) and of seg_A (segments, n, n).  `cases` lists the cases in order.  The file holds no matrix.

Run from the repo root:  python tests/golden/make_golden_exact_extremes.py
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import exact_extremes as xx
import orc
from conftest import Golden

KEYS = ("E", "A0", "LL", "seg_LL", "seg_chk")


def record(case, o):
    """the golden's entries of one case from an E-step result with per-segment outputs"""
    out = {"%s.%s" % (case, k): xx.bits(o[k]).reshape(np.shape(o[k]) or (1,)) for k in KEYS}
    out[case + ".A_sha256"] = np.array(xx.sha(o["A"]))
    out[case + ".seg_A_sha256"] = np.array(xx.sha(o["seg_A"]))
    return out


def case_name(n, name):
    return "n%d.%s" % (n, name)


def main():
    ref = orc.Reference()
    golden = Golden()
    out, cases = {}, []
    for n, name in xx.cases(xx.GOLDEN_SIZES):
        a, e, a0 = xx.params(n, name)
        o = ref.estep(a, e, a0, xx.segments(golden, n), per_seg=True)
        out.update(record(case_name(n, name), o))
        cases.append(case_name(n, name))
    out["cases"] = np.array(cases)
    dst = os.path.join(HERE, "exact_extremes.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
