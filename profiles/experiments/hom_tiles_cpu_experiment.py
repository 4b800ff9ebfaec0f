#!/usr/bin/env python3
"""The CPU experiment behind the "hom_tiles" rule: how far is a speculated start vector from the true one when
the warm-up before a tile lies in a run of homozygous bins?  Dense normalised forward recursion in numpy, no GPU.

Input: the long segment of tests/test_gpu_hom_tiles.py -- 120 000 bins from psmc_amd/sim.py, bins 40 000-85 000 set to 0 -- under
n64_curve and n64_flat of tests/golden/hmm_params.npz.  A speculation starts W = 3072 bins before the tile from the stationary vector;
the figure is max |speculated - true| / max true at the tile's first bin, both vectors normalised to sum 1."""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from psmc_amd import sim

W, RUN = 3072, (40000, 85000)


def forward(a, e, x, obs, keep=False):
    """x_p = e[o_p] . (x_{p-1} a), normalised; returns the last vector, or all of them"""
    out = np.empty((len(obs), len(x))) if keep else None
    for i, o in enumerate(obs):
        x = (x @ a) * e[o]
        x /= x.sum()
        if keep: out[i] = x
    return out if keep else x


def main():
    raw = dict(np.load(os.path.join(ROOT, "tests", "golden", "hmm_params.npz")))
    rows = []
    for key in ("n64_curve", "n64_flat"):
        a, e, a0 = raw[key + ".a"], raw[key + ".e"], raw[key + ".a0"]
        rng = np.random.default_rng(20234)
        sim.simulate_segment(a, e, a0, 2761, rng)
        s = sim.simulate_segment(a, e, a0, 120000, rng)
        s[RUN[0]:RUN[1]] = 0
        true = forward(a, e, a0.copy(), s, keep=True)            # true[p] = the vector after bin p (0-based)
        def mismatch(lo, w=W):                                    # tile starting at bin lo, warm-up over bins lo - w .. lo - 1
            x = forward(a, e, a0.copy(), s[lo - w:lo])
            t = true[lo - 1]
            return float(np.abs(x - t).max() / t.max())
        col = [("ordinary data tile", mismatch(20000))]
        col += [("tile starting %d bins into the run" % k, mismatch(RUN[0] + k)) for k in (512, 1024, 2048, 3072, 6144, 20000)]
        col += [("tile starting %d bins after the run's end" % k, mismatch(RUN[1] + k)) for k in (256, 512, 1024, 2048)]
        col += [("warm-up of %d bins entirely inside the run" % w, mismatch(RUN[1], w)) for w in (3072, 12288, 40000)]
        rows.append(col)
    print("%-52s %10s %10s" % ("case", "n64_curve", "n64_flat"))
    for (name, x), (_, y) in zip(*rows):
        print("%-52s %10.1e %10.1e" % (name, x, y))


if __name__ == "__main__":
    main()
