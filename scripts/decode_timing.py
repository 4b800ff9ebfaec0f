#!/usr/bin/env python3
"""What decoding costs in fast mode (PSMC_HIP_DECODE=fast, estep_post_fast.hip) against the exact path, on the 30 M-bin genome
bench.py builds (psmc_amd/sim.py), at 64 states and at 128 (-p "64*2"):

  (a) the fused fast E-step (the default back half) and the unfused one (fuse=0 / fuse128=0: keeps bt, what decoding reads)
  (b) psmc_hip_decode over every segment after (a) -- and posterior (-D), scales (-s), post_counts (-c) beside it
  (c) the exact E-step plus the exact psmc_hip_decode over every segment
  (d) wall clock of `psmc -N25 -d` (64 states): fast mode falling back to exact (no PSMC_HIP_DECODE), PSMC_HIP_DECODE=fast,
      and plain fast without -d; and of `psmc -N0 -D` on the first 1 M bins (to /dev/null) against the device time of -D alone

Device times: the library calls are synchronous (hipStreamSynchronize before they return); every shape is warmed first and
the best of three is reported.  D2H bytes: what the call copies back.  Writes one JSON object to stdout.

    python scripts/decode_timing.py [--bins 30000000] [--skip-cli]
    python scripts/decode_timing.py --mean      (psmc_hip_post_mean beside the other decoding calls: profiles/post_mean.txt)
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best_of(fn, k=3):
    fn()   # warm (allocations, code objects)
    ts = []
    for _ in range(k):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    return min(ts) * 1e3


def write_psmcfa(path, segs):
    conv = np.frombuffer(b"TKN", dtype=np.uint8)
    with open(path, "wb") as fh:
        for i, s in enumerate(segs):
            fh.write(b">%d\n" % (i + 1))
            c = conv[s]
            for j in range(0, len(c), 60):
                fh.write(c[j:j + 60].tobytes() + b"\n")


def library_part(hip, segs, n, params, out):
    a, e, a0 = params
    L = np.array([len(s) for s in segs], dtype=np.int64)
    bins = int(L.sum())
    r = {}
    fused = hip.HipEStep(n, mode=hip.MODE_FAST)
    fused.load_segments(segs)
    r["a_fused_estep_ms"] = best_of(lambda: fused.estep(a, e, a0))
    fused.close()
    fast = hip.HipEStep(n, mode=hip.MODE_FAST, **({"fuse": 0} if n == 64 else {"fuse128": 0}))
    fast.load_segments(segs)
    r["a_unfused_estep_ms"] = best_of(lambda: fast.estep(a, e, a0))
    fast.estep(a, e, a0)
    nseg = len(segs)
    r["b_fast_decode_ms"] = best_of(lambda: [fast.decode(i) for i in range(nseg)])
    r["b_fast_decode_d2h_bytes"] = 12 * bins
    r["b_fast_scales_ms"] = best_of(lambda: [fast.scales(i) for i in range(nseg)])
    r["b_fast_scales_d2h_bytes"] = 8 * bins
    cnt1 = [np.ones((len(s), 2), np.int32) for s in segs]
    cnt = np.zeros((n, 2))
    r["b_fast_post_counts_ms"] = best_of(lambda: [fast.post_counts(i, cnt1[i], cnt) for i in range(nseg)])
    big = int(np.argmax(L))
    r["b_fast_posterior_longest_segment_ms"] = best_of(lambda: fast.posterior(big))
    r["b_fast_posterior_longest_segment_bins"] = int(L[big])
    r["b_fast_posterior_d2h_bytes_per_bin"] = 8 * (n + 1)
    fast.close()
    ex = hip.HipEStep(n, mode=hip.MODE_EXACT)
    ex.load_segments(segs)
    t = time.perf_counter(); ex.estep(a, e, a0); r["c_exact_estep_first_ms"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter(); ex.estep(a, e, a0); r["c_exact_estep_ms"] = (time.perf_counter() - t) * 1e3
    r["c_exact_decode_ms"] = best_of(lambda: [ex.decode(i) for i in range(nseg)])
    r["c_exact_posterior_longest_segment_ms"] = best_of(lambda: ex.posterior(big))
    ex.close()
    r["fast_pass_ms"] = r["a_unfused_estep_ms"] + r["b_fast_decode_ms"]
    r["exact_pass_ms"] = r["c_exact_estep_ms"] + r["c_exact_decode_ms"]
    r["exact_over_fast"] = r["exact_pass_ms"] / r["fast_pass_ms"]
    out["n%d" % n] = r
    print(json.dumps({"n%d" % n: r}), file=sys.stderr, flush=True)


def mean_part(hip, segs, n, params, out):
    """--mean: psmc_hip_post_mean (two columns: t_k and t_k^2, all segments) beside psmc_hip_posterior (rows only) and the four
    older decoding calls, on the same tables: exact, and fast with the unfused back half.  A library without post_mean (the
    parent commit's, through PSMC_HIP_LIB) gives the other columns alone."""
    a, e, a0 = params
    nseg, bins = len(segs), int(sum(len(s) for s in segs))
    w = np.stack([np.linspace(0.01, 15.0, n), np.linspace(0.01, 15.0, n) ** 2])
    cnt1 = [np.ones((len(s), 2), np.int32) for s in segs]
    cnt = np.zeros((n, 2))
    have = hasattr(hip.load_library(), "psmc_hip_post_mean")
    for kind in ("exact", "fast"):
        es = hip.HipEStep(n, mode=hip.MODE_EXACT) if kind == "exact" else hip.HipEStep(n, mode=hip.MODE_FAST, **({"fuse": 0} if n <= 64 else {"fuse128": 0}))
        es.load_segments(segs)
        es.estep(a, e, a0)
        r = {"bins": bins}
        if have:
            r["post_mean_2col_ms"] = best_of(lambda: [es.post_mean(i, w) for i in range(nseg)])
            r["post_mean_d2h_bytes"] = 16 * bins
        r["posterior_rows_ms"] = best_of(lambda: [es.posterior(i, want_recomb=False) for i in range(nseg)], k=1)
        r["posterior_d2h_bytes"] = 8 * n * bins
        r["decode_ms"] = best_of(lambda: [es.decode(i) for i in range(nseg)])
        r["scales_ms"] = best_of(lambda: [es.scales(i) for i in range(nseg)])
        r["post_counts_2col_ms"] = best_of(lambda: [es.post_counts(i, cnt1[i], cnt) for i in range(nseg)])
        r["recomb_only_ms"] = best_of(lambda: [es.posterior(i, want_post=False) for i in range(nseg)])
        es.close()
        out["mean_n%d_%s" % (n, kind)] = r
        print(json.dumps({"mean_n%d_%s" % (n, kind): r}), file=sys.stderr, flush=True)


def cli_part(segs, out):
    psmc = os.path.join(ROOT, "psmc_amd", "host", "psmc")
    r = {}
    with tempfile.TemporaryDirectory() as td:
        fa = os.path.join(td, "genome.psmcfa")
        write_psmcfa(fa, segs)

        def wall(args, env, dest):
            e = dict(os.environ); [e.pop(k, None) for k in ("PSMC_HIP_MODE", "PSMC_HIP_DECODE", "PSMC_HIP_OPTIONS")]
            e.update(env)
            t = time.perf_counter()
            with open(dest, "w") as fo:
                p = subprocess.run([psmc] + args, stdout=fo, stderr=subprocess.PIPE, text=True, env=e, timeout=900)
            dt = time.perf_counter() - t
            if p.returncode != 0:
                raise RuntimeError(p.stderr[-400:])
            return dt, p.stderr

        base = ["-N25", "-t15", "-r5", "-p", "4+25*2+4+6"]
        r["d_plain_fast_N25_s"], _ = wall(base + [fa], dict(PSMC_HIP_MODE="fast"), os.devnull)
        r["d_fast_decode_N25_d_s"], err = wall(base + ["-d", fa], dict(PSMC_HIP_MODE="fast", PSMC_HIP_DECODE="fast"), os.devnull)
        r["d_fast_decode_stderr"] = err.strip().splitlines()[:3]
        r["d_exact_fallback_N25_d_s"], err = wall(base + ["-d", fa], dict(PSMC_HIP_MODE="fast"), os.devnull)
        # -D: 8(n+1) B per bin off the device and a printf line of n + 2 fields per bin -- on the first 1 M bins
        sub, left = [], 1_000_000
        for s in segs:
            if left <= 0: break
            sub.append(s[:left]); left -= len(sub[-1])
        fa1 = os.path.join(td, "sub.psmcfa")
        write_psmcfa(fa1, sub)
        d1 = ["-N0", "-t15", "-r5", "-p", "4+25*2+4+6", "-D", fa1]
        r["D_bins"] = int(sum(len(s) for s in sub))
        r["D_fast_decode_N0_s"], _ = wall(d1, dict(PSMC_HIP_MODE="fast", PSMC_HIP_DECODE="fast"), os.devnull)
        r["D_exact_N0_s"], _ = wall(d1, dict(), os.devnull)
        r["D_plain_fast_N0_no_decoding_s"], _ = wall(["-N0", "-t15", "-r5", "-p", "4+25*2+4+6", fa1], dict(PSMC_HIP_MODE="fast"), os.devnull)
    out["cli"] = r
    print(json.dumps({"cli": r}), file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=30_000_000)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--mean", action="store_true", help="time psmc_hip_post_mean beside psmc_hip_posterior and the other decoding calls (64 states, exact and fast) and nothing else")
    args = ap.parse_args()
    from psmc_amd import hip, sim
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    g = np.load(os.path.join(ROOT, "tests", "golden", "hmm_params.npz"))
    p64 = (g["n64_curve.a"], g["n64_curve.e"], g["n64_curve.a0"])
    g8 = np.load(os.path.join(ROOT, "tests", "golden", "estep_n128.npz"))
    p128 = (g8["n128_curve.a"], g8["n128_curve.e"], g8["n128_curve.a0"])
    lens = sim.human_like_lengths(args.bins, n_seg=90)
    t = time.perf_counter()
    segs = sim.simulate_genome(*p64, lens, seed=43)   # bench.py's genome
    out = {"bins": int(lens.sum()), "segments": len(segs), "simulate_s": time.perf_counter() - t}
    if args.mean:
        mean_part(hip, segs, 64, p64, out)
        print(json.dumps(out))
        return
    library_part(hip, segs, 64, p64, out)
    library_part(hip, segs, 128, p128, out)
    if not args.skip_cli:
        cli_part(segs, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
