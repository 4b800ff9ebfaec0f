"""Generate tests/golden/viterbi_extremes.npz by driving the REAL reference's hmm_Viterbi (khmm.c:83-141) through ctypes on
oracle/_ref/libpsmc_ref.so (`make -C oracle ref`), as make_golden_viterbi.py does for viterbi.npz: Viterbi paths (int16) and scores
(float64) under the extreme PSMC models of tests/test_gpu_wide_fast_edges.py MODELS at 64, 65 and 200 states (tests/path_extremes.py
extreme_model: the host model of "<n>*1" up to 128 states, of "100*2" at 200).  Data only.

A case is kept when tests/viterbi_model.py finds a path on every segment: 11 of the 13 models at each size.  The reference is NOT
called on the other two (lambda_alt_1e-3_1e3, lambda_ramp_down_1e3_1e-3: NaN in the matrix, no state at position 2 has a predecessor) --
its assert(max_l >= 0) would abort this process.

Keys: `n<states>.<model>.path` (the paths of all segments one after the other), `n<states>.<model>.score` (one per segment), `cases`
(the kept "n<states>.<model>" in order) and `segments` (their names in order); segments: tests/path_extremes.py golden_segments --
small_s00.. (segments_small.npz, at most 2000 bins each) and mid_s03 (segments_mid.npz, the first 6000 bins).  One array per case, not
one per segment: a member of the archive costs more than a short path does.

Run from the repo root:  python tests/golden/make_golden_viterbi_extremes.py
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_golden_viterbi as mg
import path_extremes as px


def main():
    lib = mg.load_ref()
    segs = px.golden_segments()
    out, cases = {}, []
    for n in px.GOLDEN_SIZES:
        for name in px.model_names():
            a, e, a0 = px.extreme_model(name, n)
            found = px.finds_path((a, e, a0), list(segs.values()))
            if found is not True:
                print("n%d %s: left out, the restatement finds no path (%s)" % (n, name, found))
                continue
            case = "n%d.%s" % (n, name)
            ref = [mg.ref_viterbi(lib, a, e, a0, seq) for seq in segs.values()]
            assert max(path.max() for path, _ in ref) < 32768
            out[case + ".path"] = np.concatenate([path for path, _ in ref]).astype(np.int16)
            out[case + ".score"] = np.array([score for _, score in ref], dtype=np.float64)
            cases.append(case)
            print(case, "done")
    out["cases"] = np.array(cases)
    out["segments"] = np.array(list(segs))
    dst = os.path.join(HERE, "viterbi_extremes.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
