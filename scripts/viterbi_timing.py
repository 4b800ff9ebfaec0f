#!/usr/bin/env python3
"""What psmc_hip_viterbi costs on an MI355X, piece by piece, and against what (profiles/viterbi.txt):

  cases     the 30 M-bin genome bench.py builds (psmc_amd/sim.py) at 64 and at 128 states; the stress fixture
            (tests/golden/stress, 2.2 M bins in six segments) at 200 states, and at 1024 states its segments cut to
            --wide-bins bins each (the streamed kernel reads the whole 8 MB matrix per position: see the report)
  per case  the sweep, the backtrace passes A, B, C and the copy-out, from the events the library records under
            PSMC_HIP_DEBUG_TIMES=1 (one line per call on stderr), for every "vit_tile" tried; scores only (no table) beside it
  against   the exact-mode E-step of the same build on the same input; and, where oracle/_ref is built, the reference's
            hmm_Viterbi on one core on the first --ref-bins bins of the longest segment (its back-trace matrix is 4 n bytes per bin)

One process, one session: every shape is warmed once, then the median of --reps calls.

    python scripts/viterbi_timing.py [--bins 30000000] [--out profiles/viterbi.txt]
"""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

TILES = [256, 1024, 2048, 4096, 16384, 65536]
LINE = re.compile(r"sweep ([\d.]+) ms, pass A ([\d.]+), pass B ([\d.]+), pass C ([\d.]+), copy-out ([\d.]+)")


class Stderr:
    """the process's stderr in a file, so that the library's timing lines can be read back"""

    def __init__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        self.pos = 0

    def new_lines(self):
        self.tmp.seek(self.pos)
        txt = self.tmp.read().decode(errors="replace")
        self.pos = self.tmp.tell()
        os.write(self.saved, txt.encode())
        return txt.splitlines()


def timed(es, err, params, reps, want_path=True):
    """medians (ms): wall, sweep, A, B, C, copy-out"""
    es.viterbi(*params, want_path=want_path)  # warm
    err.new_lines()
    rows = []
    for _ in range(reps):
        t = time.perf_counter()
        es.viterbi(*params, want_path=want_path)
        wall = (time.perf_counter() - t) * 1e3
        m = [LINE.search(l) for l in err.new_lines()]
        m = [x for x in m if x]
        rows.append([wall] + [float(v) for v in m[-1].groups()])
    return [statistics.median(c) for c in zip(*rows)]


def reference_us_per_bin(params, seq):
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libpsmc_ref.so")):
        return None
    import make_golden_viterbi as mg
    lib = mg.load_ref()
    mg.ref_viterbi(lib, *params, seq[:2000])
    t = time.perf_counter()
    mg.ref_viterbi(lib, *params, seq)
    return (time.perf_counter() - t) * 1e6 / len(seq)


def case(hip, name, n, params, segs, out, err, reps, ref_bins, exact=True, tiles=TILES):
    bins = sum(len(s) for s in segs)
    longest = max(segs, key=len)
    out.append("\n== %s: %d states, %d bins in %d segments, the longest %d bins" % (name, n, bins, len(segs), len(longest)))
    es = hip.HipEStep(n, mode=hip.MODE_EXACT)
    es.load_segments(segs)
    out.append("%-10s %10s %10s %9s %9s %9s %10s   (ms, medians of %d)" % ("vit_tile", "wall", "sweep", "pass A", "pass B", "pass C", "copy-out", reps))
    sweep = None
    for tile in tiles:
        es.set_option("vit_tile", tile)
        r = timed(es, err, params, reps)
        sweep = r[1]
        out.append("%-10d %10.2f %10.2f %9.3f %9.3f %9.3f %10.2f   backtrace A+B+C = %.3f ms = %.2f %% of the sweep" % (tile, *r, sum(r[2:5]), 100 * sum(r[2:5]) / r[1]))
    r = timed(es, err, params, reps, want_path=False)
    out.append("%-10s %10.2f %10.2f %9s %9s %9s %10.2f" % ("no path", r[0], r[1], "-", "-", "-", r[5]))
    out.append("sweep: %.3f us per bin of the longest segment (one work-group per segment: the longest one is the critical path), %.4f us per bin of the input"
               % (sweep * 1e3 / len(longest), sweep * 1e3 / bins))
    if exact:
        es.estep(*params)
        t = time.perf_counter(); es.estep(*params); ms = (time.perf_counter() - t) * 1e3
        out.append("exact-mode E-step, same build and input: %.1f ms = %.3f us per bin of the longest segment; the Viterbi sweep is %.2f x that"
                   % (ms, ms * 1e3 / len(longest), sweep / ms))
    es.close()
    us = reference_us_per_bin(params, longest[:ref_bins])
    if us is not None:
        out.append("reference hmm_Viterbi, one core, %d bins: %.2f us per bin -> %.1f s for this input; the device call (wall, default tile) is %.0f x faster"
                   % (min(ref_bins, len(longest)), us, us * bins * 1e-6, us * bins * 1e-3 / r[0] if r[0] else 0))
    print("\n".join(out[-12:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=30_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wide-bins", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viterbi.txt"))
    args = ap.parse_args()
    os.environ["PSMC_HIP_DEBUG_TIMES"] = "1"
    from psmc_amd import hip, sim
    import wide_fast_timing as wt
    err = Stderr()
    g = np.load(os.path.join(ROOT, "tests", "golden", "hmm_params.npz"))
    p64 = (g["n64_curve.a"], g["n64_curve.e"], g["n64_curve.a0"])
    g8 = np.load(os.path.join(ROOT, "tests", "golden", "estep_n128.npz"))
    p128 = (g8["n128_curve.a"], g8["n128_curve.e"], g8["n128_curve.a0"])
    out = ["# psmc_hip_viterbi on an MI355X (scripts/viterbi_timing.py): device times from the call's own events, wall = the whole call",
           "# (host log tables, allocation of the table, uploads, kernels, copy-out, release)"]
    lens = sim.human_like_lengths(args.bins, n_seg=90)
    segs = sim.simulate_genome(*p64, lens, seed=43)   # bench.py's genome
    case(hip, "genome", 64, p64, segs, out, err, args.reps, 200000)
    case(hip, "genome", 128, p128, segs, out, err, args.reps, 100000)
    del segs
    stress = wt.stress_segs()
    case(hip, "stress fixture", 200, wt.params_seq(200, 1)[0], stress, out, err, args.reps, 50000, tiles=[1024, 2048, 4096])
    cut = [s[:args.wide_bins] for s in stress]
    case(hip, "stress fixture, segments cut to %d bins" % args.wide_bins, 1024, wt.params_seq(1024, 1)[0], cut, out, err, args.reps, 4000,
         tiles=[1024, 2048, 4096])
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
