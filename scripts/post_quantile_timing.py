#!/usr/bin/env python3
"""What psmc_hip_post_quantile costs (three columns: q = 0.025, 0.5, 0.975; all segments) beside the two routes to the same band
on the same context and tables:

  post_mean_2col      psmc_hip_post_mean with two columns (the PSMC_TMRCA track: 16 bytes per bin off the device)
  rows                psmc_hip_posterior's rows alone (8 n bytes per bin off the device)
  rows_host_loop      the rows plus the host's count over them (numpy: running sums in state order, q times the total, the count) --
                      the route psmc_hip_post_quantile replaces

  (a) the 30 M-bin genome bench.py builds (psmc_amd/sim.py), 64 states: exact tables, and the fast tables (unfused back half)
  (b) the stress fixture (tests/golden/stress, 2.2 M bins) on the wide fast path at 200 and 1024 states, from the full X table and
      from checkpoints ("wide_ckpt" + "wide_decode_ckpt")

The library calls are synchronous; every call is warmed once, then the best of three passes over all segments is taken (the rows:
one pass after the warm-up; the rows plus the host loop: one pass).  One JSON object per case on stderr as it is measured, all of them on stdout.

    python scripts/post_quantile_timing.py [--bins 30000000] [--states 200,1024] [--skip-genome] [--skip-stress]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

Q = np.array([0.025, 0.5, 0.975])


def best_of(fn, k=3, warm=True):
    if warm:
        fn()   # (allocations, code objects)
    ts = []
    for _ in range(k):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    return min(ts) * 1e3


def host_count(post):
    """the exact-tables rule of include/psmc_hip.h over one segment's rows"""
    c = np.cumsum(post, axis=1)   # sequential along a row: one rounded addition per state
    out = np.empty((post.shape[0], len(Q)), dtype=np.int32)
    for j, qj in enumerate(Q):
        out[:, j] = np.minimum((c < (qj * c[:, -1])[:, None]).sum(1), post.shape[1] - 1)
    return out


def measure(es, nseg, n, bins):
    w = np.stack([np.linspace(0.01, 15.0, n), np.linspace(0.01, 15.0, n) ** 2])
    r = {"bins": bins, "states": n}
    r["post_quantile_3col_ms"] = best_of(lambda: [es.post_quantile(i, Q) for i in range(nseg)])
    r["post_mean_2col_ms"] = best_of(lambda: [es.post_mean(i, w) for i in range(nseg)])
    r["rows_ms"] = best_of(lambda: [es.posterior(i, want_recomb=False) for i in range(nseg)], k=1)
    r["rows_host_loop_ms"] = best_of(lambda: [host_count(es.posterior(i, want_recomb=False)[0]) for i in range(nseg)], k=1, warm=False)
    r["post_quantile_d2h_bytes"], r["rows_d2h_bytes"] = 4 * len(Q) * bins, 8 * n * bins
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=30_000_000)
    ap.add_argument("--states", default="200,1024")
    ap.add_argument("--skip-genome", action="store_true")
    ap.add_argument("--skip-stress", action="store_true")
    args = ap.parse_args()
    from psmc_amd import hip, sim
    out = {}

    def done(key, r):
        out[key] = r
        print(json.dumps({key: r}), file=sys.stderr, flush=True)

    if not args.skip_genome:
        g = np.load(os.path.join(ROOT, "tests", "golden", "hmm_params.npz"))
        p64 = (g["n64_curve.a"], g["n64_curve.e"], g["n64_curve.a0"])
        segs = sim.simulate_genome(*p64, sim.human_like_lengths(args.bins, n_seg=90), seed=43)   # bench.py's genome
        bins = int(sum(len(s) for s in segs))
        for kind in ("exact", "fast"):
            es = hip.HipEStep(64, mode=hip.MODE_EXACT) if kind == "exact" else hip.HipEStep(64, mode=hip.MODE_FAST, fuse=0)
            es.load_segments(segs)
            es.estep(*p64)
            done("genome_n64_" + kind, measure(es, len(segs), 64, bins))
            es.close()
    if not args.skip_stress:
        from wide_fast_timing import params_seq, stress_segs
        segs = stress_segs()
        bins = int(sum(len(s) for s in segs))
        for n in [int(x) for x in args.states.split(",") if x]:
            a, e, a0 = params_seq(n, 1)[0]
            for ckpt in (False, True):
                es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=2 if n > 256 else 1, wide_decode=1)
                if ckpt:
                    es.set_option("wide_ckpt", 1)
                    es.set_option("wide_decode_ckpt", 1)
                es.load_segments(segs)
                es.estep_factored(a, e[:2], a0)
                done("stress_n%d_%s" % (n, "ckpt" if ckpt else "full"), measure(es, len(segs), n, bins))
                es.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
