"""Generate tests/golden/viterbi.npz by driving the REAL reference's hmm_Viterbi (khmm.c:83-141) through ctypes on
oracle/_ref/libpsmc_ref.so (`make -C oracle ref`): Viterbi paths (int16) and scores (float64) of the fixtures' segments
under five parameter sets.  Data only.

Keys: `<set>.<seg>.path`, `<set>.<seg>.score`, sets n23_curve, n64_flat (hmm_params.npz), n128_curve (estep_n128.npz),
n149, n200 (estep_wide.npz); segments mid_s00.. (segments_mid.npz, the first 20 000 bins of each) and small_s00..
(segments_small.npz, whole).

Run from the repo root:  python tests/golden/make_golden_viterbi.py
"""
import ctypes as C
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
MID_BINS = 20000

_dp = C.POINTER(C.c_double)


class HmmPar(C.Structure):  # khmm.h hmm_par_t
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("a", C.POINTER(_dp)), ("e", C.POINTER(_dp)), ("ae", C.POINTER(_dp)), ("a0", _dp)]


class HmmData(C.Structure):  # khmm.h hmm_data_t
    _fields_ = [("L", C.c_int), ("status", C.c_uint), ("seq", C.c_char_p), ("f", C.POINTER(_dp)), ("b", C.POINTER(_dp)), ("s", _dp),
                ("v", C.POINTER(C.c_int)), ("p", C.POINTER(C.c_int))]


def load_ref():
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libpsmc_ref.so"))
    lib.hmm_new_par.restype = C.POINTER(HmmPar)
    lib.hmm_new_par.argtypes = [C.c_int, C.c_int]
    lib.hmm_delete_par.argtypes = [C.POINTER(HmmPar)]
    lib.hmm_new_data.restype = C.POINTER(HmmData)
    lib.hmm_new_data.argtypes = [C.c_int, C.c_void_p, C.POINTER(HmmPar)]
    lib.hmm_delete_data.argtypes = [C.POINTER(HmmData)]
    lib.hmm_Viterbi.restype = C.c_double
    lib.hmm_Viterbi.argtypes = [C.POINTER(HmmPar), C.POINTER(HmmData)]
    return lib


def ref_viterbi(lib, a, e, a0, seq):
    """(path int32 (L,), score) from hmm_Viterbi: path[u-1] = hd->v[u]"""
    n = len(a0)
    hp = lib.hmm_new_par(2, n)  # e[2][*] = 1
    for k in range(n):
        hp.contents.a0[k] = float(a0[k])
        hp.contents.e[0][k] = float(e[0][k])
        hp.contents.e[1][k] = float(e[1][k])
        for l in range(n):
            hp.contents.a[k][l] = float(a[k][l])
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    hd = lib.hmm_new_data(len(seq), seq.ctypes.data, hp)
    score = lib.hmm_Viterbi(hp, hd)
    path = np.array(hd.contents.v[1:len(seq) + 1], dtype=np.int32)
    lib.hmm_delete_data(hd)
    lib.hmm_delete_par(hp)
    return path, score


def parameter_sets():
    g = lambda f: np.load(os.path.join(HERE, f))
    hp, n128, wide = g("hmm_params.npz"), g("estep_n128.npz"), g("estep_wide.npz")
    out = {}
    for name, z in (("n23_curve", hp), ("n64_flat", hp), ("n128_curve", n128), ("n149", wide), ("n200", wide)):
        out[name] = (z[name + ".a"], z[name + ".e"], z[name + ".a0"])
    return out


def segments():
    mid = np.load(os.path.join(HERE, "segments_mid.npz"))
    small = np.load(os.path.join(HERE, "segments_small.npz"))
    out = {"mid_" + k: mid[k][:MID_BINS] for k in sorted(mid.files)}
    out.update({"small_" + k: small[k] for k in sorted(small.files)})
    return out


def main():
    lib = load_ref()
    out = {}
    segs = segments()
    for name, (a, e, a0) in parameter_sets().items():
        for sname, seq in segs.items():
            path, score = ref_viterbi(lib, a, e, a0, seq)
            assert path.max() < 32768
            out["%s.%s.path" % (name, sname)] = path.astype(np.int16)
            out["%s.%s.score" % (name, sname)] = np.float64(score)
        print(name, "done")
    dst = os.path.join(HERE, "viterbi.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
