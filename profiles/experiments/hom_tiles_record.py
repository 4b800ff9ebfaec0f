#!/usr/bin/env python3
"""The record behind profiles/hom_tiles.txt: "hom_tiles" = 0 and 1 on (a) the input of tests/test_gpu_hom_tiles.py::test_the_finding
(2 761 + 120 000 bins, bins 40 000-85 000 of the long segment homozygous; default plan: 256-bin tiles) and (b) the stress fixture
(tests/golden/stress, 2.2 M bins, a 5e4-bin run of homozygosity among its features) under the GENOME options of tests/test_gpu_stress.py.
Per case: repair rounds and tile repairs of a fresh context's first E-step, its A_cell / E_cell against the reference, and the wall time
of the first and of the fourth E-step (parameters moving: the plan learns in between).  Needs the GPU.
`python profiles/experiments/hom_tiles_record.py [FILE]`: the record is printed, and written to FILE when one is named."""
import gzip
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from psmc_amd import hip
from psmc_amd.parity import fast_error_metrics
import conftest
import orc
import test_gpu_hom_tiles as T
from test_gpu_stress import GENOME


def stress():
    d = os.path.join(conftest.GOLD, "stress")
    lut = np.full(256, 2, np.uint8); lut[ord("T")] = 0; lut[ord("K")] = 1
    segs, cur = [], []
    for line in gzip.open(os.path.join(d, "stress.psmcfa.gz"), "rb"):
        if line.startswith(b">"):
            if cur: segs.append(np.concatenate(cur))
            cur = []
        else:
            cur.append(lut[np.frombuffer(line.rstrip(b"\n"), dtype=np.uint8)])
    segs.append(np.concatenate(cur))
    g = dict(np.load(os.path.join(d, "stress_estep.npz")))
    steps = []
    for rd in (0, 1, 2, 0):
        k = "rd%d" % rd
        steps.append((dict(a=g[k + ".a"], e=g[k + ".e"], a0=g[k + ".a0"]), dict(A=g[k + ".A"], E=g[k + ".E"], LL=float(g[k + ".LL"]))))
    return segs, steps


def main():
    orc.build_oracle(with_ref=False)
    inp = T.Inputs(conftest.Golden(), orc.Oracle())
    cases = [("finding input, default plan", inp.segs["main"], [(inp.params(k), inp.ref("main", k)) for k in ("curve", 1, 2, 0)], {})]
    segs, steps = stress()
    cases.append(("stress fixture, GENOME options", segs, steps, dict(GENOME)))
    out = []
    for name, segs, steps, opts in cases:
        out.append("%s (%d bins in %d segments)" % (name, sum(len(s) for s in segs), len(segs)))
        for hom in (0, 1):
            es = hip.HipEStep(64, mode=hip.MODE_FAST, hom_tiles=hom, **opts)
            es.load_segments(segs)
            ms, first = [], None
            for i, (p, o) in enumerate(steps):
                t0 = time.perf_counter()
                r = es.estep(p["a"], p["e"], p["a0"])
                ms.append(1e3 * (time.perf_counter() - t0))
                m = fast_error_metrics(r, o, p["a"], p["e"])
                d = es.fast_diag()
                if i == 0: first = (d, m, es.fast_plan(), es.plan_tiles())
                out.append("    hom_tiles=%d E-step %d: %8.2f ms, repair rounds %d+%d, tile repairs %d+%d, A_cell %.2e E_cell %.2e A_max %.2e LL %.1e" % (
                    hom, i + 1, ms[-1], d["fwd_rounds"], d["bwd_rounds"], d["fwd_tiles"], d["bwd_tiles"], m["A_cell"], m["E_cell"], m["A_max"], m["LL"]))
            d, m, pl, pt = first
            out.append("  hom_tiles=%d: first E-step %d repair rounds, %d tile repairs, A_cell %.2e, E_cell %.2e; first / fourth E-step %.2f / %.2f ms; "
                       "%d tiles of %d bins, %d hom tiles in qualifying runs, glued after the first E-step %d fwd / %d bwd" % (
                           hom, d["fwd_rounds"] + d["bwd_rounds"], d["fwd_tiles"] + d["bwd_tiles"], m["A_cell"], m["E_cell"], ms[0], ms[3],
                           pl["tiles"], pl["tile_len"], int((pt["cls"] == 3).sum()), pl["glued_fwd"], pl["glued_bwd"]))
            es.close()
    txt = "\n".join(out) + "\n"
    print(txt)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(txt)


if __name__ == "__main__":
    main()
