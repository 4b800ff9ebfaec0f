#!/usr/bin/env python3
"""What psmc_hip_sample_paths costs on an MI355X (profiles/sample_paths.txt):

  cases     the 30 M-bin genome bench.py builds (psmc_amd/sim.py) at 64 states; the stress fixture (tests/golden/stress, 2.2 M bins in
            six segments) at 200 states, and at 1024 states its segments cut to --wide-bins bins each
  per case  n_samp = 1 and n_samp = 8 in one group ("samp_group" auto): seconds per call, split into the sweeps and the backtraces
            from the events the library records under PSMC_HIP_DEBUG_TIMES=1 (one line per call on stderr); the marginal cost of a
            sample inside a group = (sweep of the group of 8 - sweep of one sample) / 7
  against   psmc_hip_viterbi on the same input in the same session (its sweep and its backtrace)

One process, one session; the code objects are loaded by a call on a small input first, then every figure is ONE call (--reps for more:
the median).

    python scripts/sample_timing.py [--bins 30000000] [--out profiles/sample_paths.txt]
"""
import argparse
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from viterbi_timing import LINE as VIT_LINE, Stderr  # noqa: E402

LINE = re.compile(r"sample_paths: .* in (\d+) groups of (\d+), .*: sweeps ([\d.]+) ms, backtraces ([\d.]+) ms")


def timed(call, err, line, reps):
    """medians: wall (ms) and the groups of the library's line"""
    rows = []
    for _ in range(reps):
        err.new_lines()
        t = time.perf_counter()
        call()
        wall = (time.perf_counter() - t) * 1e3
        m = [line.search(l) for l in err.new_lines()]
        rows.append([wall] + [float(v) for v in [x for x in m if x][-1].groups()])
    return [statistics.median(c) for c in zip(*rows)]


def case(hip, name, n, params, segs, out, err, reps):
    bins = sum(len(s) for s in segs)
    longest = max(len(s) for s in segs)
    first = len(out)
    out.append("\n== %s: %d states, %d bins in %d segments, the longest %d bins" % (name, n, bins, len(segs), longest))
    es = hip.HipEStep(n, mode=hip.MODE_EXACT)
    es.load_segments(segs)
    out.append("%-28s %10s %10s %12s %8s   (ms; %d call%s each)" % ("call", "wall", "sweeps", "backtraces", "groups", reps, "" if reps == 1 else "s, medians"))
    res = {}
    for label, n_samp in (("n_samp 1", 1), ("n_samp 8, one group", 8)):
        r = timed(lambda: es.sample_paths(*params, 1, n_samp), err, LINE, reps)
        res[label] = r
        out.append("%-28s %10.1f %10.1f %12.2f %5d x %d" % (label, r[0], r[3], r[4], r[1], r[2]))
    one, grp = res["n_samp 1"], res["n_samp 8, one group"]
    if grp[2] == 8:
        out.append("sweep of one sample: %.3f us per bin of the longest segment (one work-group per segment: the longest is the critical path); of a group of 8: %.3f us,"
                   % (one[3] * 1e3 / longest, grp[3] * 1e3 / longest))
        out.append("i.e. %.3f us per sample; marginal cost of a sample inside the group: %.3f us per bin = %.2f of the one-sample sweep (8 one-sample calls: %.2f x the group's sweep)"
                   % (grp[3] * 1e3 / longest / 8, (grp[3] - one[3]) * 1e3 / longest / 7, (grp[3] - one[3]) / 7 / one[3], 8 * one[3] / grp[3]))
    else:
        out.append("(the device's free memory held groups of %d, not 8)" % grp[2])
    out.append("backtrace per sample: %.2f ms = %.2f %% of a one-sample sweep" % (grp[4] / 8, 100 * grp[4] / 8 / one[3]))
    v = timed(lambda: es.viterbi(*params), err, VIT_LINE, reps)
    out.append("psmc_hip_viterbi, same input and session: wall %.1f ms, sweep %.1f ms (%.3f us per bin of the longest segment), backtrace A+B+C %.2f ms; the one-sample sampling sweep is %.2f x the Viterbi sweep"
               % (v[0], v[1], v[1] * 1e3 / longest, sum(v[2:5]), one[3] / v[1]))
    es.close()
    print("\n".join(out[first:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=30_000_000)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--wide-bins", type=int, default=20000)
    ap.add_argument("--cases", default="64,200,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_paths.txt"))
    args = ap.parse_args()
    os.environ["PSMC_HIP_DEBUG_TIMES"] = "1"
    from psmc_amd import hip, sim
    import wide_fast_timing as wt
    err = Stderr()
    g = np.load(os.path.join(ROOT, "tests", "golden", "hmm_params.npz"))
    p64 = (g["n64_curve.a"], g["n64_curve.e"], g["n64_curve.a0"])
    out = ["# psmc_hip_sample_paths on an MI355X (python scripts/sample_timing.py): device times from the call's own events, wall = the whole call",
           "# (allocation of the map tables, uploads, kernels, copy-out of n_samp x bins path entries, release)"]
    cases = [int(x) for x in args.cases.split(",")]
    warm = hip.HipEStep(64, mode=hip.MODE_EXACT)   # loads the code objects
    warm.load_segments([np.zeros(1000, dtype=np.uint8)])
    warm.sample_paths(*p64, 1, 1)
    warm.viterbi(*p64)
    warm.close()
    if 64 in cases:
        lens = sim.human_like_lengths(args.bins, n_seg=90)
        segs = sim.simulate_genome(*p64, lens, seed=43)   # bench.py's genome
        case(hip, "genome", 64, p64, segs, out, err, args.reps)
        del segs
    stress = wt.stress_segs()
    if 200 in cases:
        case(hip, "stress fixture", 200, wt.params_seq(200, 1)[0], stress, out, err, args.reps)
    if 1024 in cases:
        cut = [s[:args.wide_bins] for s in stress]
        case(hip, "stress fixture, segments cut to %d bins" % args.wide_bins, 1024, wt.params_seq(1024, 1)[0], cut, out, err, args.reps)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
