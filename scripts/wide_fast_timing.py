#!/usr/bin/env python3
"""What the factored E-step of the wide fast path ("wide_fast", estep_wide_fast.hip) costs against the wide exact kernels, on the
30 M-bin genome bench.py builds (psmc_amd/sim.py), at 149, 200 and 256 states (patterns "1+74*2", "100*2", "128*2"), and
-- beyond 256 states with "wide_fast" = 2, the same kernels at 2..4 waves per tile -- at 300, 512, 768 and 1024 states
("150*2", "128*4", "128*6", "128*8"); --stress takes the stress fixture (tests/golden/stress, 2.2 M bins) instead of the genome:

  (a) ms per factored E-step on the wide fast path, parameters moving every step (the host model of psmc_amd.hostlib with
      lambdas scaled by a few per cent per step): the first E-step of a context and the mean of the later ones, with the
      verify / repair rounds and repaired head tiles of every step
  (b) ms per E-step of the wide exact kernels (psmc_hip_estep) on the same input and the first parameters (one step after a
      warm-up of the allocations)
  (c) with --cli: wall clock of `psmc -N5 -p "100*2"` on the genome in exact mode and with PSMC_HIP_MODE=fast PSMC_HIP_WIDE=fast
  (d) with --decode: decoding from the wide fast tables ("wide_decode", estep_wide_post.hip; beyond 256 states "wide_fast" = 2: the
      same kernels at 2..4 waves per tile) -- after a warm-up pass, --repeats
      passes of each decoding call over ALL segments (decode = -d, recombination only and posterior rows + recombination = -D,
      post_counts with three columns = -c, scales = -s; the posterior rows of the longest segment only unless --full-post: all
      of them are 8 n bytes per bin to the host), min | median | max in ms; and what the same request costs without the option:
      one exact E-step (full counts) + the same calls on the exact tables, once

  (e) with --batch R: the bootstrap batch on the wide fast path ("wide_batch") -- R replicates, each a seeded multiset of the input's
      segments (as many draws as segments, with replacement) with parameters of its own (the moving parameters of (a)):
      seconds per replicate of psmc_hip_estep_batch with "wide_batch" = 1 (after one warm-up call: allocations), every replicate's
      own time from the progress callback, one single wide E-step over ALL segments in the same process, and -- --batch-leg exact,
      a process of its own so that a job can give each leg its time limit -- the same batch with "wide_batch" = 0: the exact
      launch groups, what such a context ran before the option existed

  (f) with --counts: the full count matrix from the wide fast path ("wide_counts", estep_wide_counts.hip) -- ms per psmc_hip_estep of a
      context with "wide_fast" + "wide_counts" (parameters moving as in (a); the first step and the later ones, and of the later ones
      what the library's events give to the factored part and to the counts pass), ms per factored wide E-step of the same build
      and parameters, and -- unless --exact-steps 0 -- ms per psmc_hip_estep on the wide exact kernels, what that call ran before the
      option existed; --counts-slab sets "wide_counts_slab".  With --ckpt it sets "wide_ckpt" = 1 and "wide_counts_ckpt" = 1 on that
      context: the counts E-steps keep checkpoints and the counts pass recomputes the rows between them.  Either way it prints the X
      table's bytes and interval beside each time, and the device memory in use before the context exists and after its E-steps
      (hipMemGetInfo: the context keeps every buffer, so the difference is what the run needs)

  --gap-tiles sets "wide_gap_tiles" = 1 on the wide contexts of every leg (the exact-kernel contexts are what they are).

  --hom-tiles sets "wide_hom_tiles" = 1 on the same contexts: runs of homozygosity are crossed by the chain with the matrix of a
  homozygous tile.  --plant-hom LEN[,LEN...] plants such runs in the chosen input first: stretch k of m (k = 1 .. m) starts at bin
  k total / (m + 1) of the input, counted over its segments in order, and ends after LEN bins or at its segment's end; its het bins
  become symbol 0 (missing bins stay).  No random draw: the same input at every call.

  --mix-tiles sets "wide_mix_tiles" = 1 beside --hom-tiles: het-free tiles that hold both symbol 0 and missing bins join the chain, each
  with two matrices of its own.

  --ckpt sets "wide_ckpt" = 1 on the wide contexts of (a) and (e): X at every 8th bin only, the rest recomputed in the accumulate
  sweep.  Beside every time, (a) and (e) print what psmc_hip_wide_table_info reports: the bytes of X the context holds.
  With --decode it sets "wide_ckpt" = 1 and "wide_decode_ckpt" = 1 on the wide context of (d): the decoding E-step keeps checkpoints
  and every decoding call recomputes the rows between them; (d) prints the X table's bytes beside the decode times either way.

Library calls are synchronous.  Writes one JSON object to stdout (progress on stderr).

    python scripts/wide_fast_timing.py [--bins 30000000] [--steps 6] [--states 149,200,256] [--cli]
    python scripts/wide_fast_timing.py --stress --states 300,512,768,1024 --steps 4 --exact-steps 1
    python scripts/wide_fast_timing.py --stress --states 200,300,1024 --steps 4 --exact-steps 0 [--ckpt] [--gap-tiles]
    python scripts/wide_fast_timing.py --states 200,300,1024 --steps 4 --exact-steps 0 --plant-hom 20000,20000,200000 [--hom-tiles [--mix-tiles]]
    python scripts/wide_fast_timing.py --decode --stress --states 300,1024
    python scripts/wide_fast_timing.py --decode --stress --states 200,300,1024 --exact-steps 0 [--ckpt]
    python scripts/wide_fast_timing.py --stress --batch 4 --states 200 --batch-leg wide    (then --batch-leg exact; the same at 300)
    python scripts/wide_fast_timing.py --counts [--stress] --states 200,300,1024 --steps 4 --exact-steps 1
    python scripts/wide_fast_timing.py --counts --stress --states 200,300,1024 --steps 4 --exact-steps 0 [--ckpt]
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

PATTERNS = {149: ("1+74*2", 75), 150: ("75*2", 75), 200: ("100*2", 100), 256: ("128*2", 128),
            300: ("150*2", 150), 512: ("128*4", 128), 768: ("128*6", 128), 1024: ("128*8", 128)}


def stress_segs():
    """tests/golden/stress: 2e5-bin runs of N, a 5e4-bin run of homozygosity, an all-gap segment; 2.2 M bins in six segments"""
    import gzip
    lut = np.full(256, 2, np.uint8); lut[ord("T")] = 0; lut[ord("K")] = 1
    segs, cur = [], []
    for line in gzip.open(os.path.join(ROOT, "tests", "golden", "stress", "stress.psmcfa.gz"), "rb"):
        if line.startswith(b">"):
            if cur: segs.append(np.concatenate(cur))
            cur = []
        else:
            cur.append(lut[np.frombuffer(line.rstrip(b"\n"), dtype=np.uint8)])
    segs.append(np.concatenate(cur))
    return segs


def params_seq(n, steps, seed=11):
    from psmc_amd import hostlib
    pat, k = PATTERNS[n]
    rng = np.random.default_rng(seed + n)
    lam = np.exp(rng.normal(0.0, 0.5, size=k))
    out = []
    for _ in range(steps):
        out.append(hostlib.hmm_params(pat, [0.0008, 0.0002, 15.0] + list(lam)))
        lam = lam * np.exp(rng.normal(0.0, 0.03, size=k))   # an EM round moves the parameters a little
    return out


GAP_OPTS = {}   # --gap-tiles: {"wide_gap_tiles": 1} on the wide contexts of every leg; --hom-tiles: "wide_hom_tiles" likewise


def plant_hom(segs, lens):
    """--plant-hom: stretch k of m = len(lens) starts at bin k total / (m + 1) of the input (k = 1 .. m) and holds lens[k - 1] bins or
    ends with its segment; its het bins become symbol 0.  Returns the segments and [(segment, first bin, bins, hets removed)]."""
    segs = [np.array(s, dtype=np.uint8) for s in segs]
    ends = np.cumsum([len(s) for s in segs])
    total, m, planted = int(ends[-1]), len(lens), []
    for k, ln in enumerate(lens, 1):
        at = k * total // (m + 1)
        i = int(np.searchsorted(ends, at, side="right"))
        lo = at - (int(ends[i - 1]) if i else 0)
        hi = min(len(segs[i]), lo + ln)
        hets = int((segs[i][lo:hi] == 1).sum())
        segs[i][lo:hi][segs[i][lo:hi] == 1] = 0
        planted.append((i, int(lo), int(hi - lo), hets))
    return segs, planted


def table_info(es):
    """psmc_hip_wide_table_info; None with a library from before the entry point existed (PSMC_HIP_LIB: A/B against an older build)"""
    try:
        return es.wide_table_info()
    except AttributeError:
        return None


def library_part(hip, segs, n, steps, exact_steps, ckpt=False):
    ps = params_seq(n, steps)
    r = {}
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=2 if n > 256 else 1, **GAP_OPTS)
    if ckpt:
        es.set_option("wide_ckpt", 1)
    es.load_segments(segs)
    ms, rounds = [], []
    for a, e, a0 in ps:
        t = time.perf_counter(); es.estep_factored(a, e[:2], a0); ms.append((time.perf_counter() - t) * 1e3)
        d = es.fast_diag()
        rounds.append(dict(fwd_rounds=d["fwd_rounds"], bwd_rounds=d["bwd_rounds"], fwd_tiles=d["fwd_tiles"], bwd_tiles=d["bwd_tiles"],
                           warm_err_fwd=d["warm_err_fwd"], warm_err_bwd=d["warm_err_bwd"]))
    d = es.fast_diag()
    ti = table_info(es)
    r.update(wide_gap_tiles=int(GAP_OPTS.get("wide_gap_tiles", 0)), wide_hom_tiles=int(GAP_OPTS.get("wide_hom_tiles", 0)), wide_mix_tiles=int(GAP_OPTS.get("wide_mix_tiles", 0)), wide_ckpt=int(ckpt), x_table=ti, x_table_bytes=ti["bytes"] if ti else None, fast_later_ms_median=float(np.median(ms[1:])))
    if GAP_OPTS:
        try:
            cls = es.wide_plan_tiles()["cls"]
            r.update(plan_classes=[int(x) for x in np.bincount(cls, minlength=7)], chains=[len(c) for c in es.wide_gap_chains()], rechained=es.wide_gap_rechained())
        except Exception as ex:   # (PSMC_HIP_LIB: an older build without the diagnostics)
            r.update(plan_classes=str(ex))
    r.update(tiles=d["n_chunks"], tile_len=d["tile_len"], warmup=d["warmup"], fast_ms=ms, fast_first_ms=ms[0],
             fast_later_ms_mean=float(np.mean(ms[1:])), fast_later_ms_min=float(np.min(ms[1:])), repairs=rounds)
    es.close()
    print(json.dumps({"n%d" % n: r}), file=sys.stderr, flush=True)
    if exact_steps > 0:
        ex = hip.HipEStep(n, mode=hip.MODE_EXACT)
        ex.load_segments(segs)
        a, e, a0 = ps[0]
        t = time.perf_counter(); ex.estep(a, e, a0); r["exact_first_ms"] = (time.perf_counter() - t) * 1e3
        xs = []
        for _ in range(exact_steps - 1):
            t = time.perf_counter(); ex.estep(a, e, a0); xs.append((time.perf_counter() - t) * 1e3)
        ex.close()
        r["exact_ms"] = float(np.min(xs)) if xs else r["exact_first_ms"]
        r["exact_over_fast"] = r["exact_ms"] / r["fast_later_ms_mean"]
        print(json.dumps({"n%d" % n: {k: r[k] for k in ("exact_first_ms", "exact_ms", "exact_over_fast")}}), file=sys.stderr, flush=True)
    return r


def device_bytes_in_use(hip):
    """total - free of hipMemGetInfo on the current device -- the runtime the library is linked against, found through the library's
    own handle; None when it cannot be asked"""
    import ctypes as C
    try:
        fn = hip.load_library().hipMemGetInfo
    except AttributeError:
        return None
    fn.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    fn.restype = C.c_int
    free, total = C.c_size_t(0), C.c_size_t(0)
    return int(total.value - free.value) if fn(C.byref(free), C.byref(total)) == 0 else None


def counts_part(hip, segs, n, steps, exact_steps, slab=0, ckpt=False):
    """(f)"""
    ps = params_seq(n, steps)
    r = {"wide_counts_slab": slab, "wide_counts_ckpt": int(ckpt)}
    hip.load_library().psmc_hip_device_count()   # (the runtime is up before the first reading)
    before = device_bytes_in_use(hip)
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=2 if n > 256 else 1, wide_counts=1, wide_counts_slab=slab, **GAP_OPTS)
    if ckpt:
        es.set_option("wide_ckpt", 1)
        es.set_option("wide_counts_ckpt", 1)
    es.load_segments(segs)
    ms, dev, tabs = [], [], []
    for a, e, a0 in ps:
        t = time.perf_counter(); es.estep(a, e, a0); ms.append((time.perf_counter() - t) * 1e3)
        tm = es.timing()
        dev.append(dict(total=float(tm["total"]), factored=float(tm["chains"]), counts=float(tm["expect"])))
        ti = table_info(es)
        tabs.append(dict(bytes=ti["bytes"], interval=ti["interval"]) if ti else None)
    after = device_bytes_in_use(hip)
    d = es.fast_diag()
    assert d["back_half"] == 4, d
    ti = table_info(es)
    assert ti is None or ti["interval"] == (8 if ckpt else 1), ti
    r.update(x_table=tabs, device_bytes_before=before, device_bytes_after_counts_esteps=after,
             device_bytes_of_the_context=after - before if before is not None and after is not None else None)
    r.update(tiles=d["n_chunks"], tile_len=d["tile_len"], x_table_bytes=ti["bytes"] if ti else None, counts_ms=ms, counts_first_ms=ms[0],
             counts_later_ms_mean=float(np.mean(ms[1:])), counts_later_ms_min=float(np.min(ms[1:])), device_ms=dev,
             device_counts_pass_ms_mean=float(np.mean([x["counts"] for x in dev[1:]])),
             device_factored_part_ms_mean=float(np.mean([x["factored"] for x in dev[1:]])))
    fm = []
    for a, e, a0 in ps:   # the factored wide E-step of the same build, on the same context (the first one sizes nothing anew)
        t = time.perf_counter(); es.estep_factored(a, e[:2], a0); fm.append((time.perf_counter() - t) * 1e3)
    r.update(factored_ms=fm, factored_later_ms_mean=float(np.mean(fm[1:])))
    r["counts_over_factored"] = r["counts_later_ms_mean"] / r["factored_later_ms_mean"]
    es.close()
    print(json.dumps({"n%d" % n: r}), file=sys.stderr, flush=True)
    if exact_steps > 0:
        ex = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=2 if n > 256 else 1)   # the same call without the option: the wide exact kernels
        ex.load_segments(segs)
        a, e, a0 = ps[0]
        xs = []
        for _ in range(exact_steps):
            t = time.perf_counter(); ex.estep(a, e, a0); xs.append((time.perf_counter() - t) * 1e3)
        ex.close()
        r.update(exact_ms_all=xs, exact_ms=float(np.min(xs)), exact_over_counts=float(np.min(xs)) / r["counts_later_ms_mean"])
        print(json.dumps({"n%d" % n: {k: r[k] for k in ("exact_ms_all", "exact_ms", "exact_over_counts")}}), file=sys.stderr, flush=True)
    return r


def batch_part(hip, segs, n, n_rep, leg, ckpt=False):
    """(e): the replicates are the same for both legs (seeded)"""
    ps = params_seq(n, n_rep)
    rng = np.random.default_rng(97 + n)
    sel = [[int(i) for i in rng.integers(0, len(segs), size=len(segs))] for _ in range(n_rep)]
    r = {"replicates": n_rep, "selections": sel,
         "unique_bins": [int(sum(len(segs[i]) for i in set(x))) for x in sel], "all_bins": int(sum(len(s) for s in segs))}
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=2 if n > 256 else 1, wide_batch=1 if leg == "wide" else 0, **GAP_OPTS)
    if ckpt:
        es.set_option("wide_ckpt", 1)
    es.load_segments(segs)
    if leg == "wide":
        es.estep_batch(ps[:1], sel[:1], want="sums")   # warm-up: the X table and the plan's buffers
        stamps = []
        t = time.perf_counter()
        es.estep_batch(ps, sel, want="sums", on_done=lambda reps, out: stamps.append(time.perf_counter()))
        wall = time.perf_counter() - t
        d = es.fast_diag()
        ti = table_info(es)
        r.update(wide_ckpt=int(ckpt), x_table_bytes=ti["bytes"] if ti else None)
        r.update(wide_batch_s=wall, wide_batch_s_per_replicate=wall / n_rep,
                 wide_replicate_s=[float(x) for x in np.diff([t] + stamps)],
                 last_replicate=dict(tiles=d["n_chunks"], tile_len=d["tile_len"], fwd_rounds=d["fwd_rounds"], bwd_rounds=d["bwd_rounds"],
                                     fwd_tiles=d["fwd_tiles"], bwd_tiles=d["bwd_tiles"]))
        a, e, a0 = ps[0]
        ms = []
        for _ in range(4):   # the single E-step over all segments; the first one re-plans and is left out
            t = time.perf_counter(); es.estep_factored(a, e[:2], a0); ms.append(time.perf_counter() - t)
        d = es.fast_diag()
        r.update(single_estep_s=float(np.mean(ms[1:])), single_estep_first_s=ms[0], single_tiles=d["n_chunks"], single_tile_len=d["tile_len"],
                 batch_over_single=wall / n_rep / float(np.mean(ms[1:])))
    else:
        t = time.perf_counter()
        es.estep_batch(ps, sel, want="sums")
        wall = time.perf_counter() - t
        r.update(exact_batch_s=wall, exact_batch_s_per_replicate=wall / n_rep, exact_launch_groups=es.batch_info()["groups"])
    es.close()
    print(json.dumps({"n%d" % n: r}), file=sys.stderr, flush=True)
    return r


def _spread(xs):
    return dict(min=float(np.min(xs)), median=float(np.median(xs)), max=float(np.max(xs)))


def decode_calls(es, segs, n, full_post, mean=False):
    """one pass of every decoding call over all segments: seconds per kind"""
    longest = int(np.argmax([len(s) for s in segs]))
    c1 = [np.ones((len(s), 3), np.int32) for s in segs]
    cnt = np.zeros((n, 3))
    out = {}
    for name, f in (("decode", lambda i: es.decode(i)), ("recomb", lambda i: es.posterior(i, want_post=False)),
                    ("scales", lambda i: es.scales(i)), ("post_counts", lambda i: es.post_counts(i, c1[i], cnt))):
        t = time.perf_counter()
        for i in range(len(segs)):
            f(i)
        out[name] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    for i in (range(len(segs)) if full_post else [longest]):
        es.posterior(i)
    out["posterior_all" if full_post else "posterior_longest"] = (time.perf_counter() - t) * 1e3
    if mean:   # --mean: psmc_hip_post_mean, two columns, beside psmc_hip_posterior's rows alone -- both over all segments
        w = np.stack([np.linspace(0.01, 15.0, n), np.linspace(0.01, 15.0, n) ** 2])
        for name, f in (("post_mean_2col", lambda i: es.post_mean(i, w)), ("posterior_rows_all", lambda i: es.posterior(i, want_recomb=False))):
            t = time.perf_counter()
            for i in range(len(segs)):
                f(i)
            out[name] = (time.perf_counter() - t) * 1e3
    return out


def decode_part(hip, segs, n, repeats, full_post, exact, ckpt=False, mean=False):
    a, e, a0 = params_seq(n, 1)[0]
    r = {"longest_segment_bins": int(max(len(s) for s in segs))}
    es = hip.HipEStep(n, mode=hip.MODE_FAST, wide_fast=2 if n > 256 else 1, wide_decode=1, **GAP_OPTS)
    if ckpt:
        es.set_option("wide_ckpt", 1)
        es.set_option("wide_decode_ckpt", 1)
    es.load_segments(segs)
    es.estep_factored(a, e[:2], a0)
    ms = []
    for _ in range(3):
        t = time.perf_counter(); es.estep_factored(a, e[:2], a0); ms.append((time.perf_counter() - t) * 1e3)
    r["wide_estep_ms"] = _spread(ms)
    ti = table_info(es)
    r.update(wide_gap_tiles=int(bool(GAP_OPTS)), wide_ckpt=int(ckpt), x_table=ti, x_table_bytes=ti["bytes"] if ti else None)
    decode_calls(es, segs, n, full_post, mean)   # warm-up
    passes = [decode_calls(es, segs, n, full_post, mean) for _ in range(repeats)]
    r["wide_decode_ms"] = {k: _spread([p[k] for p in passes]) for k in passes[0]}
    es.close()
    print(json.dumps({"n%d" % n: r}), file=sys.stderr, flush=True)
    if exact:
        ex = hip.HipEStep(n, mode=hip.MODE_EXACT)
        ex.load_segments(segs)
        t = time.perf_counter(); ex.estep(a, e, a0); r["exact_estep_ms"] = (time.perf_counter() - t) * 1e3
        r["exact_decode_ms"] = decode_calls(ex, segs, n, full_post, mean)
        ex.close()
        print(json.dumps({"n%d" % n: {k: r[k] for k in ("exact_estep_ms", "exact_decode_ms")}}), file=sys.stderr, flush=True)
    return r


def write_psmcfa(path, segs):
    conv = np.frombuffer(b"TKN", dtype=np.uint8)
    with open(path, "wb") as fh:
        for i, s in enumerate(segs):
            fh.write(b">%d\n" % (i + 1))
            c = conv[s]
            for j in range(0, len(c), 60):
                fh.write(c[j:j + 60].tobytes() + b"\n")


def cli_part(segs):
    psmc = os.path.join(ROOT, "psmc_amd", "host", "psmc")
    r = {}
    with tempfile.TemporaryDirectory() as td:
        fa = os.path.join(td, "genome.psmcfa")
        write_psmcfa(fa, segs)
        for name, env in (("fast_wide", dict(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast")), ("exact", dict())):
            e = dict(os.environ); [e.pop(k, None) for k in ("PSMC_HIP_MODE", "PSMC_HIP_WIDE", "PSMC_HIP_DECODE", "PSMC_HIP_OPTIONS")]
            e.update(env)
            t = time.perf_counter()
            p = subprocess.run([psmc, "-N5", "-t15", "-r5", "-p", "100*2", fa], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                               text=True, env=e, timeout=1100)
            r[name + "_N5_s"] = time.perf_counter() - t
            r[name + "_stderr"] = p.stderr.strip().splitlines()[:3]
            if p.returncode != 0:
                raise RuntimeError(p.stderr[-400:])
            print(json.dumps({"cli": {name + "_N5_s": r[name + "_N5_s"]}}), file=sys.stderr, flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=30_000_000)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--exact-steps", type=int, default=2)
    ap.add_argument("--states", default="149,200,256")
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--decode", action="store_true", help="time the decoding calls on the wide fast tables (and on the exact ones) instead of (a), (b)")
    ap.add_argument("--mean", action="store_true", help="with --decode: also psmc_hip_post_mean (two columns) and psmc_hip_posterior's rows alone, each over all segments (profiles/post_mean.txt)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--full-post", action="store_true")
    ap.add_argument("--batch", type=int, default=0, help="(e): the bootstrap batch of this many replicates on the wide fast path instead of (a), (b)")
    ap.add_argument("--batch-leg", choices=["wide", "exact"], default="wide", help="with --batch: \"wide_batch\" = 1 and the single E-step, or the exact launch groups")
    ap.add_argument("--ckpt", action="store_true", help="\"wide_ckpt\" = 1 on the wide contexts of (a) and (e): X at every 8th bin only; the table's bytes are printed beside each time.  With --decode: \"wide_ckpt\" = 1 and \"wide_decode_ckpt\" = 1 on the wide context of (d), decoding from checkpoints.  With --counts: \"wide_ckpt\" = 1 and \"wide_counts_ckpt\" = 1 on the wide-counts context of (f), counts from checkpoints")
    ap.add_argument("--counts", action="store_true", help="(f): psmc_hip_estep with \"wide_counts\" = 1 against the factored wide E-step and the exact kernels instead of (a), (b)")
    ap.add_argument("--counts-slab", type=int, default=0, help="with --counts: \"wide_counts_slab\" (0 = auto)")
    ap.add_argument("--stress", action="store_true", help="the stress fixture (tests/golden/stress, 2.2 M bins) instead of the simulated genome")
    ap.add_argument("--gap-tiles", action="store_true", help="\"wide_gap_tiles\" = 1 on the wide contexts of every leg: runs of missing data are crossed by the transfer-matrix chain (estep_wide_gap.hip); (a) prints the largest verify mismatch of every step beside its rounds")
    ap.add_argument("--hom-tiles", action="store_true", help="\"wide_hom_tiles\" = 1 on the wide contexts of every leg: runs of homozygosity are crossed by the transfer-matrix chain with the matrix of a homozygous tile")
    ap.add_argument("--plant-hom", default="", help="LEN[,LEN...]: turn the het bins of stretches of these lengths into symbol 0, at offsets k total / (m + 1) of the chosen input")
    ap.add_argument("--mix-tiles", action="store_true", help="\"wide_mix_tiles\" = 1 beside --hom-tiles: het-free tiles with both symbol 0 and missing bins join the chain with two matrices each")
    args = ap.parse_args()
    if args.mix_tiles:
        GAP_OPTS["wide_mix_tiles"] = 1
    if args.gap_tiles:
        GAP_OPTS["wide_gap_tiles"] = 1
    if args.hom_tiles:
        GAP_OPTS["wide_hom_tiles"] = 1
    from psmc_amd import hip, sim
    if args.stress:
        segs = stress_segs()
        out = {"input": "tests/golden/stress", "bins": int(sum(len(s) for s in segs)), "segments": len(segs)}
    else:
        g = np.load(os.path.join(ROOT, "tests", "golden", "hmm_params.npz"))
        p64 = (g["n64_curve.a"], g["n64_curve.e"], g["n64_curve.a0"])
        lens = sim.human_like_lengths(args.bins, n_seg=90)
        t = time.perf_counter()
        segs = sim.simulate_genome(*p64, lens, seed=43)   # bench.py's genome
        out = {"bins": int(lens.sum()), "segments": len(segs), "simulate_s": time.perf_counter() - t}
    if args.plant_hom:
        segs, planted = plant_hom(segs, [int(x) for x in args.plant_hom.split(",") if x])
        out["planted_hom"] = planted
    for n in [int(x) for x in args.states.split(",") if x]:
        if args.counts:
            out["n%d" % n] = counts_part(hip, segs, n, args.steps, args.exact_steps, args.counts_slab, args.ckpt)
        elif args.batch > 0:
            out["n%d" % n] = batch_part(hip, segs, n, args.batch, args.batch_leg, args.ckpt)
        elif args.decode:
            out["n%d" % n] = decode_part(hip, segs, n, args.repeats, args.full_post, args.exact_steps > 0, args.ckpt, args.mean)
        else:
            out["n%d" % n] = library_part(hip, segs, n, args.steps, args.exact_steps, args.ckpt)
    if args.cli:
        out["cli"] = cli_part(segs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
