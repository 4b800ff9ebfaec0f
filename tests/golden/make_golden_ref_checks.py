#!/usr/bin/env python3
"""Generate the reference side of the host-logic comparisons that used to call the reference at test time
(tests/test_host_cli.py, tests/test_oracle.py): the reference binary's output of three long EM runs, and the
reference's psmc_update_hmm, .psmcfa reader, kmin_hj and E-step on the tests' seeded inputs.

Needs oracle/_ref (built by `make -C oracle ref` from the unmodified reference sources).  The outputs are data --
inputs, the reference's outputs, or SHA-256 digests of its outputs where those are large -- and are committed.

    python tests/golden/make_golden_ref_checks.py
"""
import gzip
import hashlib
import os
import subprocess
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import orc  # noqa: E402

CLI = os.path.join(HERE, "cli")
OUT = os.path.join(HERE, "ref_checks")

# the command lines of test_host_cli.py::test_long_em_runs_equal_the_reference_binary, in its parametrize order
LONG_EM_ARGS = [["-N25", "-t15", "-r5", "-p", "4+25*2+4+6", "small.psmcfa"], ["-N30", "-t15", "-r5", "-p", "4+5*3+4", "t10k.psmcfa"],
                ["-N8", "-t15", "-r5", "-T", "0.1", "-p", "4+5*3+4", "small.psmcfa"]]
MODEL_PATTERNS = ("4+5*3+4", "4+25*2+4+6", "64*2", "1*10", "3+2*17+15*1+1*12")
ODD_PSMCFA = ">a desc\nTTKKN\n\nnnkt\r\n@b\nTKTK+\n+\nIIII\n>c\nKK>d x\nTTTT\n"


def digest(*arrays):
    h = hashlib.sha256()
    for x in arrays:
        h.update(np.ascontiguousarray(x, dtype=np.float64).tobytes())
    return h.hexdigest()


def long_em(ref_bin):
    for i, args in enumerate(LONG_EM_ARGS):
        r = subprocess.run([ref_bin] + args[:-1] + [os.path.join(CLI, args[-1])], capture_output=True, text=True, check=True)
        with gzip.GzipFile(os.path.join(OUT, "long_em_%d.psmc.gz" % i), "wb", mtime=0) as f:
            f.write(r.stdout.encode())


def model_update(ref, g):
    """psmc_update_hmm on the random parameter vectors of test_model_update_equals_reference_on_random_parameters"""
    rng = np.random.default_rng(20260927)
    for pattern in MODEL_PATTERNS:
        n_free = ref.parse_pattern(pattern)[1]
        params, sums = [], []
        for trial in range(40):
            theta = 10.0 ** rng.uniform(-4, -0.5); rho = 10.0 ** rng.uniform(-5, -0.5); max_t = 10.0 ** rng.uniform(-0.3, 1.7)
            lam = 10.0 ** rng.uniform(-2.5, 2.5, size=n_free) if trial % 3 else 10.0 ** rng.uniform(-0.3, 0.3, size=n_free)
            p = np.concatenate([[theta, rho, max_t], lam])
            w = ref.hmm_params(pattern, p)
            params.append(p)
            sums.append(digest(w["a"], w["e"][:2], w["a0"]))
        g["model.%s.params" % pattern] = np.array(params)
        g["model.%s.sha256" % pattern] = np.array(sums)


def odd_reader(ref, g):
    p = os.path.join(OUT, "odd.psmcfa.tmp")
    with open(p, "w") as f:
        f.write(ODD_PSMCFA)
    r = ref.read_psmcfa(p)
    os.remove(p)
    g["odd.L"] = np.array([len(s) for s in r["segs"]], dtype=np.int64)
    g["odd.seq"] = np.concatenate(r["segs"]).astype(np.uint8) if r["segs"] else np.zeros(0, np.uint8)
    g["odd.sum_L"] = np.int64(r["sum_L"]); g["odd.sum_n"] = np.int64(r["sum_n"])


def kmin(ref, g):
    """kmin_hj on the quadratic of oracle/ref_shim.c from the starts of test_hooke_jeeves_equals_reference_search_bit_for_bit"""
    rng = np.random.default_rng(7)
    n_, x0_, c_, x_, f_ = [], [], [], [], []
    for trial in range(60):
        n = int(rng.integers(1, 30))
        centre = rng.normal(size=n) * 10.0 ** rng.uniform(-2, 2)
        x0 = rng.normal(size=n) * 10.0 ** rng.uniform(-2, 2)
        x0[rng.random(n) < 0.15] = 0.0
        xr, fr = ref.kmin_quad(x0.copy(), centre.copy())
        n_.append(n); x0_.append(x0); c_.append(centre); x_.append(np.asarray(xr)); f_.append(fr)
    g["hj.n"] = np.array(n_, dtype=np.int64)
    g["hj.x0"] = np.concatenate(x0_); g["hj.centre"] = np.concatenate(c_); g["hj.x"] = np.concatenate(x_); g["hj.fx"] = np.array(f_)


def estep_random(ref, g):
    """the reference's per-segment E-step on the random HMMs of test_oracle.py::test_oracle_vs_reference_random"""
    rng = np.random.default_rng(5)
    for n in (3, 23, 64):
        a = rng.random((n, n)) ** 3 + np.eye(n) * 5
        a /= a.sum(1, keepdims=True)
        e = np.ones((3, n)); e[1] = rng.random(n) * 0.2; e[0] = 1 - e[1]
        a0 = rng.random(n); a0 /= a0.sum()
        segs = [rng.choice(3, size=L, p=[0.85, 0.1, 0.05]).astype(np.uint8) for L in (1, 2, 17, 500, 3000)]
        rr = ref.estep(a, e, a0, segs, per_seg=True)
        g["estep.%d.a" % n] = a; g["estep.%d.e" % n] = e; g["estep.%d.a0" % n] = a0
        g["estep.%d.seq" % n] = np.concatenate(segs); g["estep.%d.L" % n] = np.array([len(s) for s in segs], dtype=np.int64)
        g["estep.%d.keys" % n] = np.array(sorted(rr))
        g["estep.%d.sha256" % n] = np.array([digest(np.asarray(rr[k])) for k in sorted(rr)])


def main():
    orc.build_oracle(with_ref=True)
    os.makedirs(OUT, exist_ok=True)
    ref = orc.Reference()
    long_em(orc.REF_BIN)
    g = {}
    model_update(ref, g)
    odd_reader(ref, g)
    kmin(ref, g)
    estep_random(ref, g)
    np.savez_compressed(os.path.join(OUT, "ref_checks.npz"), **g)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
