"""Histories of API calls on one long-lived psmc_hip context, and the twin every call of one is checked against
(tests/test_gpu_ctx_history.py on the device, tests/test_ctx_history_model.py without one).  TEST INFRASTRUCTURE: nothing here needs a
device to be imported, to build a history or to interpret one on the oracle.

THE INVARIANT.  For every checked call of a history the return code and every output array equal, bit for bit, those of the same call
on a TWIN: a context created for that one check, given the options, the segments and the selection in force at the start of its
replay window, then the state operations of the window, then the call.  The window by context kind:

  exact  (exact mode, any state count)        an E-step, a batch, Viterbi, sampling: empty.  A decoding call: from the last single
                                              E-step on.
  wide   (fast mode, 129 .. 1024 states,      as exact: the path learns nothing between E-steps.
          "wide_fast" set)
  fast   (fast mode up to 128 states)         from the last event that makes the plan dirty (load, select, an option of PLAN_OPTIONS)
                                              at or before the current call -- for a decoding call: at or before the last single
                                              E-step.

State operations are load, load_device, select, option, reserve and the E-steps and batches; the decoding calls, Viterbi, sampling
and every refused `bad_call` are not replayed: they must leave nothing behind.  Three extensions of the rule, each decided from the
library's code and named here by the field that makes it necessary:
  * the window is replayed with ALL its state operations in order, the options that do not make the plan dirty included
    ("learn", "structured", "kc_min", "group_cap" ...: psmc_hip_opts decides what the E-steps of the window learn: glue_f, glue_b,
    the tiles' warm-ups);
  * psmc_hip_ctx::kids / sh_glue_*: the replicate contexts of a fast batch keep their plans and what they learned over a select
    (psmc_hip_select does not destroy them), so on a fast context a select ends the window only when no batch ran in it;
  * psmc_hip_ctx::tables_batch / tab_serial: a batch after the last single E-step owns the tables, so the window of a decoding
    call holds the batches that followed that E-step too (the twin refuses as the context does).

Exact-mode results are held to the CPU oracle as well (OracleBackend), Viterbi and sampling to tests/viterbi_model.py and
tests/sample_model.py, so a twin with the same defect cannot hide it.

A history is a list of Op.  Segments are named by pool, parameters by name (params()), so a history is plain data: the coverage
conditions of tests/test_ctx_history_model.py are computed from the histories alone."""
import hashlib
import os
import re
from collections import namedtuple

import numpy as np

import exact_extremes as xx
import path_extremes as px

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KINDS = ("exact", "fast", "wide")
SIZES = {"exact": (23, 64, 65, 128, 200, 300), "fast": (64, 128), "wide": (200, 300, 1024)}
GENERATED_SIZES = {"exact": (23, 64, 65, 128, 200, 300), "fast": (64, 128), "wide": (200, 300)}   # 1024: hand-written histories only
N_GENERATED, N_OPS = 12, 25
BASE_OPTIONS = {"exact": (), "fast": (), "wide": (("wide_fast", 2), ("wide_decode", 1))}

E_STEPS = ("estep", "estep_factored", "estep_segments")
DECODING = ("decode", "posterior", "scales", "post_counts", "post_mean", "post_quantile")
PATHS = ("viterbi", "sample")
STATE_OPS = ("load", "load_device", "select", "option", "reserve") + E_STEPS + ("batch",)
CHECKED = E_STEPS + ("batch",) + DECODING + PATHS + ("table_info", "bad_call")
VOCABULARY = STATE_OPS + DECODING + PATHS + ("table_info", "bad_call")
# what a kind has no use for: the operation is refused there by design whatever the state (it occurs as a `bad_call` instead)
NOT_APPLICABLE = {
    "exact": ("estep_factored", "table_info"),     # psmc_hip_estep_factored: fast mode only
    "fast": ("estep_segments", "reserve", "table_info"),  # exact mode only below 129 states; reserve moves tab_serial on: a table event of its own
    "wide": ("reserve",),
}

# psmc_hip_set_option (psmc_amd/csrc/api.hip): every key it accepts, and whether its branch sets plan_dirty.  Derived from the
# source once; tests/test_ctx_history_model.py holds it to the source text.
PLAN_OPTIONS = frozenset((
    "chunk", "warmup", "merge", "adapt", "prev_start", "warm_shift", "merge1", "gap_tiles", "hom_tiles", "hom_min", "coarse",
    "kc_sub", "two_phase", "fuse", "fuse128", "wide_ckpt", "wide_gap_tiles", "wide_gap_min", "wide_hom_tiles", "wide_hom_min",
    "wide_mix_tiles", "wide_mix_mb"))
OTHER_OPTIONS = frozenset((
    "batch_first", "vit_tile", "samp_group", "max_rounds", "structured", "learn", "phase1", "phase1_waves", "tail", "lanes8",
    "kc_min", "ckpt", "group_cap", "share_learn", "exact_refwd", "batch_sort", "batch_tailfill", "batch_major", "batch_bins",
    "overlap", "warm_tol", "wide_fast", "wide_decode", "wide_decode_ckpt", "wide_batch", "wide_counts", "wide_counts_ckpt",
    "wide_counts_slab", "rep_impl"))
# the plan options a history of each kind must change at least once (the rest of PLAN_OPTIONS is read by the other path only; of
# the fast path's, "merge" / "adapt" / "prev_start" / "warm_shift" / "merge1" / "coarse" / "kc_sub" / "two_phase" are covered by the
# generator's option draw)
PLAN_OPTIONS_OF = {
    "exact": (),
    "fast": ("chunk", "warmup", "merge", "adapt", "prev_start", "warm_shift", "merge1", "gap_tiles", "hom_tiles", "hom_min", "coarse",
             "kc_sub", "two_phase", "fuse", "fuse128"),
    "wide": ("chunk", "warmup", "wide_ckpt", "wide_gap_tiles", "wide_gap_min", "wide_hom_tiles", "wide_hom_min", "wide_mix_tiles",
             "wide_mix_mb"),
}


def options_in_source(text):
    """{key: sets plan_dirty} of every key psmc_hip_set_option accepts, from the text of api.hip"""
    body = text[text.index('extern "C" int psmc_hip_set_option'):]
    body = body[:body.index("\n}\n")]
    out = {}
    for line in body.splitlines():
        m = re.search(r'if \(k == "(\w+)"\)', line)
        if m:
            out[m.group(1)] = "plan_dirty = true" in line
    return out


Op = namedtuple("Op", "kind args expect")   # expect: None (whatever the twin does), "ok" or "refused"


def op(kind, *args, expect=None):
    assert kind in VOCABULARY, kind
    return Op(kind, tuple(args), expect)


# ---------------------------------------------------------------------------------------------------------------- data, parameters
PAR_NAMES = ("golden", "rho_1e-6", "lambda_ramp_down_1e2_1e-2")
POOLS = ("small", "medium", "large", "sandwich")
_POOLS, _PARAMS = {}, {}


def large_bins(n):
    return 600 if n >= 513 else 3000


def pools(golden, n):
    """small: 5 segments of 2, 65, 129, 32 and 1 bins; medium: the nine of path_extremes.short_segs, up to 700 bins; large: the
    thirteen of exact_extremes.segments with the longest grown to 3000 bins (600 from 513 states on); each with its single-bin
    segment LAST.  sandwich: wide_mix_model.mix_sandwich (gap, hom and het-free mixed tiles at tiles of 64 bins) and a short one."""
    key = large_bins(n)
    if key not in _POOLS:
        from wide_mix_model import mix_sandwich
        base = xx.segments(golden, n)
        med = px.short_segs(golden, 700)
        out = dict(small=[base[2], base[5], base[12], base[7], base[0]],
                   medium=med[1:] + [med[0]],
                   large=base[1:8] + [golden.segs_mid[3][:large_bins(n)]] + base[9:] + [base[0]],
                   sandwich=[mix_sandwich(golden.segs_mid[3]), golden.segs_small[7]])
        assert [len(s) for s in out["small"]] == [2, 65, 129, 32, 1]
        assert len(out["medium"]) == 9 and len(out["large"]) == 13 and max(len(s) for s in out["large"]) == large_bins(n)
        assert all(len(v[-1]) == 1 for k, v in out.items() if k != "sandwich")
        _POOLS[key] = {k: [np.ascontiguousarray(s, dtype=np.uint8) for s in v] for k, v in out.items()}
    return _POOLS[key]


N_SEG = dict(small=5, medium=9, large=13, sandwich=2)
# multisets over a pool in the style of exact_extremes.SEL / SEL2: one segment three times, one twice, one loaded segment left out,
# a non-monotonic order
SELECTIONS = {
    5: ((2, 0, 4, 2, 3, 2, 0), (3, 3, 1, 4, 0, 3, 1)),
    9: ((7, 2, 8, 7, 0, 4, 3, 4, 7, 5, 6), (1, 6, 6, 8, 0, 3, 5, 6, 2, 2, 7)),
    13: ((7, 2, 11, 7, 12, 4, 9, 0, 4, 7, 1, 3, 5, 8, 10), (10, 3, 3, 8, 12, 7, 11, 3, 1, 5, 5, 0, 2, 9, 6)),
    2: ((1, 0, 0), (0, 1, 1)),
}


def selection(pool, which):
    return SELECTIONS[N_SEG[pool]][which]


def params(golden, n, name):
    """(a, e (3, n), a0): "golden" is the golden set of the size where the fixtures hold one (23, 64, 128 states), par_of(n) of
    tests/test_gpu_post_mean.py at the sizes of the wide path, else the mild model of exact_extremes; the other two names are the
    extreme models of test_gpu_wide_fast_edges.MODELS.  Computed once, never changed."""
    key = (n, name)
    if key not in _PARAMS:
        if name != "golden":
            p = xx.params(n, name)
        elif n in (23, 64):
            g = golden.params("n%d_curve" % n)
            p = (g["a"], g["e"], g["a0"])
        elif n == 128:
            p = tuple(golden.n128["n128_curve." + k] for k in ("a", "e", "a0"))
        elif n > 128:
            from test_gpu_wide_fast_ckpt import par_of
            p = par_of(n)
        else:
            p = xx.params(n, xx.MILD)
        p = tuple(np.ascontiguousarray(x, dtype=np.float64) for x in p)
        assert p[0].shape == (n, n) and p[1].shape[1] == n and p[2].shape == (n,)
        e3 = np.ones((3, n))
        e3[:2] = p[1][:2]
        _PARAMS[key] = (p[0], e3, p[2])
    return _PARAMS[key]


def weights(n, cols):
    from test_gpu_post_mean import weights as w4
    return np.ascontiguousarray(w4(n)[:cols])


QUANTILES = (0.5, 0.025, 0.975, 1.0)


def count_matrix(L, cols):
    """cnt1 of psmc_hip_post_counts: (L, cols) int32, a fixed pattern with zeros"""
    u = np.arange(L)[:, None]
    j = np.arange(cols)[None, :]
    return np.ascontiguousarray(((u * 7 + j * 3) % 5).astype(np.int32))


# ---------------------------------------------------------------------------------------------------------------- the world
class World:
    """What a history has made of a context so far, from the history alone."""

    def __init__(self, kind, n):
        self.kind, self.n = kind, n
        self.opts = dict(BASE_OPTIONS[kind])
        self.pool, self.sel = None, None
        self.log = []          # (op, snapshot before it) of every state operation that was accepted
        self.last_estep = None    # index into log of the last single E-step; None after a load
        self.last_plan = 0        # index into log where the fast plan's window starts
        self.batch_in_window = False
        self.plan_starts = [0]
        self.last_estep_ok = False

    def snapshot(self):
        return (dict(self.opts), self.pool, self.sel)

    def record(self, o, rc="ok"):
        """a state operation was accepted (or an E-step or batch ran and failed: it is replayed as well)"""
        k = o.kind
        snap = self.snapshot()
        if k in ("load", "load_device"):
            self.pool, self.sel = o.args[0], tuple(range(N_SEG[o.args[0]]))
            self.last_estep = None
        elif k == "select":
            self.sel = tuple(o.args[0])
        elif k == "option":
            self.opts[o.args[0]] = o.args[1]
        self.log.append((o, snap))
        at = len(self.log)
        if k in E_STEPS:
            self.last_estep = at - 1
            self.last_estep_ok = rc == "ok"
        if k == "batch":
            self.batch_in_window = True
        plan_event = k in ("load", "load_device") or (k == "option" and o.args[0] in PLAN_OPTIONS) or (k == "select" and not self.batch_in_window)
        if plan_event:
            self.last_plan = at
            self.batch_in_window = False
            self.plan_starts.append(at)

    def window(self, o):
        """index into log where the twin's replay for operation o starts"""
        now = len(self.log)
        dec = o.kind in DECODING or o.kind == "table_info"
        if o.kind in PATHS:   # they read the observations and nothing else
            return now
        if self.kind != "fast":
            return self.last_estep if dec and self.last_estep is not None else now
        if dec and self.last_estep is not None:
            return max(s for s in self.plan_starts if s <= self.last_estep)
        return self.last_plan

    def last_plan_event(self):
        w = self.last_plan
        return "%d: %s" % (w - 1, describe(self.log[w - 1][0])) if w > 0 else "creation"

    # -- predictions the generator and the coverage conditions use (conservative: "ok" only where the code leaves no doubt)
    def decodable(self, seg):
        if self.last_estep is None:
            return False
        e, snap = self.log[self.last_estep]
        later = [x.kind for x, _ in self.log[self.last_estep + 1:]]
        if any(k in ("batch", "select", "reserve") or k in E_STEPS for k in later):
            return False
        if any(x.kind == "option" and (x.args[0] in PLAN_OPTIONS or x.args[0].startswith("wide_")) for x, _ in self.log[self.last_estep + 1:]):
            return False
        if seg % N_SEG[self.pool] not in snap[2]:
            return False
        if self.kind == "exact":
            return e.kind in ("estep", "estep_segments")
        if self.kind == "wide":
            return True
        o = snap[0]
        unfused = o.get("fuse", 1) == 0 if self.n <= 64 else o.get("fuse128", 2) == 0
        return e.kind == "estep" and unfused and not o.get("merge", 0)


def describe(o):
    def short(x):
        if isinstance(x, (tuple, list)) and len(x) > 6:
            return "(%d items)" % len(x)
        return repr(x)
    return "%s(%s)%s" % (o.kind, ", ".join(short(x) for x in o.args), " expect " + o.expect if o.expect else "")


# ---------------------------------------------------------------------------------------------------------------- backends
STRERROR = ("invalid argument", "out of memory", "HIP runtime error", "not supported in this build", "call order violated",
            "fast-mode tile boundaries did not converge")
BAD_CALLS = ("nan_quantile", "n_w_5", "segment_out_of_range", "decode_before_estep", "estep_device_wide", "factored_on_exact",
             "segments_on_fast")
BAD_CALLS_OF = {"exact": ("nan_quantile", "n_w_5", "segment_out_of_range", "factored_on_exact"),
                "fast": ("nan_quantile", "n_w_5", "segment_out_of_range", "segments_on_fast"),
                "wide": ("nan_quantile", "n_w_5", "segment_out_of_range", "estep_device_wide")}
BAD_RC = {"nan_quantile": "invalid argument", "n_w_5": "invalid argument", "segment_out_of_range": "invalid argument",
          "decode_before_estep": "call order violated", "estep_device_wide": "not supported in this build",
          "factored_on_exact": "not supported in this build", "segments_on_fast": "not supported in this build"}


def rc_of(err):
    msg = str(err)
    for s in STRERROR:
        if ": " + s + " (" in msg:
            return s
    raise AssertionError("no return code in %r" % msg)


class DeviceBackend:
    """One psmc_hip context; run(op) -> (rc, [(name, array)])"""

    def __init__(self, hip, golden, kind, n, opts=None):
        self.hip, self.golden, self.kind, self.n = hip, golden, kind, n
        self.es = hip.HipEStep(n, mode=hip.MODE_EXACT if kind == "exact" else hip.MODE_FAST)
        self.pool = None
        for k, v in (BASE_OPTIONS[kind] if opts is None else opts.items()):
            self.es.set_option(k, v)

    def close(self):
        self.es.close()

    def segs(self):
        return pools(self.golden, self.n)[self.pool]

    def par(self, name):
        return params(self.golden, self.n, name)

    def run(self, o):
        try:
            return "ok", self._run(o)
        except self.hip.HipError as err:
            return rc_of(err), []

    def _run(self, o):
        es, k, a = self.es, o.kind, o.args
        if k == "load":
            self.pool = a[0]
            es.load_segments(self.segs())
        elif k == "load_device":
            import torch
            self.pool = a[0]
            segs = self.segs()
            lens = np.array([len(s) for s in segs], dtype=np.int32)
            off = np.concatenate([[0], np.cumsum((lens.astype(np.int64) + 63) // 64 * 64)])
            host = np.full(int(off[-1]) + 256, 2, dtype=np.uint8)
            for s, at in zip(segs, off[:-1]):
                host[at:at + len(s)] = s
            d_obs = torch.from_numpy(host).cuda()
            es.load_segments_device(d_obs.data_ptr(), off[:-1], lens, keepalive=d_obs)
        elif k == "select":
            es.select(list(a[0]))
        elif k == "option":
            es.set_option(a[0], a[1])
        elif k == "reserve":
            if a:
                es.reserve_batch_tables(a[0])
            else:
                es.reserve_tables()
        elif k == "estep":
            r = es.estep(*self.par(a[0]))
            return [(x, r[x]) for x in ("A", "E", "A0", "LL", "chk")]
        elif k == "estep_factored":
            r = es.estep_factored(*self.par(a[0]))
            return [(x, r[x]) for x in ("sums", "E", "LL")]
        elif k == "estep_segments":
            r = es.estep_segments(*self.par(a[0]))
            return [(x, r[x]) for x in ("seg_A", "seg_E", "seg_A0", "seg_LL", "chk")]
        elif k == "batch":
            r = es.estep_batch([self.par(p) for p in a[0]], [list(s) for s in a[1]], want=a[2])
            return [(x, r[x]) for x in ("A", "sums", "E", "LL") if x in r]
        elif k == "decode":
            path, mp = es.decode(a[0] % es.n_seg)
            return [("path", path), ("maxp", mp)]
        elif k == "posterior":
            post, rec = es.posterior(a[0] % es.n_seg)
            return [("post", post), ("recomb", rec)]
        elif k == "scales":
            return [("s", es.scales(a[0] % es.n_seg))]
        elif k == "post_counts":
            seg = a[0] % es.n_seg
            cnt = np.zeros((self.n, a[1]))
            es.post_counts(seg, count_matrix(int(es.lens[seg]), a[1]), cnt)
            return [("cnt", cnt)]
        elif k == "post_mean":
            return [("mean", es.post_mean(a[0] % es.n_seg, weights(self.n, a[1])))]
        elif k == "post_quantile":
            return [("state", es.post_quantile(a[0] % es.n_seg, QUANTILES[:a[1]]))]
        elif k == "viterbi":
            paths, score = es.viterbi(*self.par(a[0]), want_path=a[1])
            return ([("paths", np.concatenate(paths))] if a[1] else []) + [("score", score)]
        elif k == "sample":
            paths = es.sample_paths(*self.par(a[0]), seed=a[2], n_samp=a[1])
            return [("paths", np.concatenate([np.concatenate(p) for p in paths]))]
        elif k == "table_info":
            return [("interval", np.array([es.wide_table_info()["interval"]], dtype=np.int64))]
        elif k == "bad_call":
            self._bad(a[0])
        return []

    def _bad(self, what):
        es = self.es
        if what == "nan_quantile":
            es.post_quantile(0, [0.5, float("nan")])
        elif what == "n_w_5":
            es.post_mean(0, np.ones((5, self.n)))
        elif what == "segment_out_of_range":
            import ctypes as C
            path = np.zeros(4, dtype=np.int32)
            es._chk(es.lib.psmc_hip_decode(es.h, es.n_seg, path.ctypes.data_as(C.POINTER(C.c_int32)), None), "decode")
        elif what == "decode_before_estep":
            es.decode(0)
        elif what == "estep_device_wide":
            import torch
            buf = torch.zeros(self.n * self.n + 2 * self.n + 1, dtype=torch.float64, device="cuda")
            es.estep_device(*self.par("golden"), buf.data_ptr())
        elif what == "factored_on_exact":
            es.estep_factored(*self.par("golden"))
        elif what == "segments_on_fast":
            es.estep_segments(*self.par("golden"))
        else:
            raise AssertionError(what)


class OracleBackend:
    """Exact mode on the CPU: the oracle (tests/orc.py) for the E-steps, the batch and the decoding calls, tests/viterbi_model.py and
    tests/sample_model.py for the paths, and the call order of an exact context (what a fresh context and the header promise): a
    decoding call needs a single E-step after the last load and the last batch."""

    def __init__(self, oracle, golden, n):
        self.oracle, self.golden, self.n, self.kind = oracle, golden, n, "exact"
        self.pool, self.sel, self.tables = None, None, None
        self.cache = {}

    def close(self):
        pass

    def segs(self):
        return pools(self.golden, self.n)[self.pool]

    def par(self, name):
        return params(self.golden, self.n, name)

    def _estep(self, par, sel):
        key = ("estep", par, self.pool, tuple(sel))
        if key not in self.cache:
            a, e, a0 = self.par(par)
            self.cache[key] = self.oracle.estep(a, e, a0, [self.segs()[i] for i in sel], per_seg=True)
        return self.cache[key]

    def _fb(self, par, seg):
        key = ("fb", par, self.pool, seg)
        if key not in self.cache:
            a, e, a0 = self.par(par)
            self.cache = {k: v for k, v in self.cache.items() if k[0] != "fb"}   # one segment's tables at a time
            self.cache[key] = self.oracle.fwd_bwd(a, e, a0, self.segs()[seg])
        return self.cache[key]

    def run(self, o):
        k, a, n = o.kind, o.args, self.n
        if k in ("load", "load_device"):
            self.pool, self.sel, self.tables = a[0], tuple(range(N_SEG[a[0]])), None
        elif k == "select":
            if any(i < 0 or i >= N_SEG[self.pool] for i in a[0]):
                return "invalid argument", []
            self.sel = tuple(a[0])
        elif k in ("option", "reserve"):
            pass
        elif k == "estep":
            r = self._estep(a[0], self.sel)
            self.tables = a[0]
            return "ok", [("A", r["A"]), ("E", r["E"]), ("A0", r["A0"]), ("LL", r["LL"]), ("chk", r["seg_chk"])]
        elif k == "estep_segments":
            r = self._estep(a[0], self.sel)
            self.tables = a[0]
            return "ok", [("seg_A", r["seg_A"]), ("seg_E", r["seg_E"]), ("seg_LL", r["seg_LL"]), ("chk", r["seg_chk"])]
        elif k == "estep_factored":
            return "not supported in this build", []
        elif k == "batch":
            self.tables = None
            rs = [self._estep(p, s) for p, s in zip(a[0], a[1])]
            out = []
            if a[2] in ("A", "both"):
                out.append(("A", np.stack([r["A"] for r in rs])))
            out += [("E", np.stack([r["E"] for r in rs])), ("LL", np.array([r["LL"] for r in rs]))]
            return "ok", out
        elif k in DECODING:
            if self.tables is None:
                return "call order violated", []
            seg = a[0] % N_SEG[self.pool]
            pa, pe, pa0 = self.par(self.tables)
            f, b, s, lk, chk = self._fb(self.tables, seg)
            if k == "decode":
                path, mp = self.oracle.post_decode(f, b, s)
                return "ok", [("path", path[1:]), ("maxp", mp[1:])]
            if k == "scales":
                return "ok", [("s", s[1:])]
            if k == "post_counts":
                cnt = np.zeros((n, a[1]))
                self.oracle.post_counts(f, b, s, count_matrix(len(self.segs()[seg]), a[1]), cnt)
                return "ok", [("cnt", cnt)]
            post, rec = self.oracle.post_full(pa, pe, self.segs()[seg], f, b, s)
            if k == "posterior":
                return "ok", [("post", post[1:]), ("recomb", rec[1:])]
            if k == "post_mean":
                from test_gpu_post_mean import loop_sum
                return "ok", [("mean", loop_sum(post[1:], weights(n, a[1])))]
            from test_gpu_post_quantile import loop_count
            return "ok", [("state", loop_count(post[1:], np.array(QUANTILES[:a[1]])))]
        elif k == "viterbi":
            import viterbi_model as vm
            key = ("vit", a[0], self.pool)
            if key not in self.cache:
                tabs = vm.log_tables(*self.par(a[0]))
                try:
                    self.cache[key] = [vm.viterbi(tabs, s) for s in self.segs()]
                except vm.NoFinitePath:
                    self.cache[key] = None
            if self.cache[key] is None:
                return "invalid argument", []
            got = self.cache[key]
            return "ok", ([("paths", np.concatenate([p for p, _ in got]))] if a[1] else []) + [("score", np.array([s for _, s in got]))]
        elif k == "sample":
            import sample_model as sm
            pa, pe, pa0 = self.par(a[0])
            paths = sm.sample_segments(pa, pe, pa0, self.segs(), a[2], a[1])
            return "ok", [("paths", np.concatenate([np.concatenate(p) for p in paths]))]
        elif k == "bad_call":
            return BAD_RC[a[0]], []
        return "ok", []


def same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype.kind == "f" or y.dtype.kind == "f":
        return x.shape == y.shape and np.array_equal(xx.bits(x).reshape(-1), xx.bits(y).reshape(-1))
    return x.shape == y.shape and np.array_equal(x, y)


ORACLE_OMITS = frozenset(("seg_A0",))   # tests/orc.py returns no per-segment A0: that output is held to the twin alone


def first_difference(got, want, omits=frozenset()):
    """(output name, flat index, got, wanted) of the first output that differs, or None; the two calls must return the same
    outputs by name (but for `omits`, which `want` may lack)"""
    names = dict(want)
    have = [name for name, _ in got]
    if set(have) - set(omits) != set(names) - set(omits) or len(have) != len(set(have)):
        return "(the names of the outputs)", -1, sorted(have), sorted(names)
    for name, x in got:
        if name not in names:
            continue
        y = names[name]
        if not same(x, y):
            x, y = np.atleast_1d(np.asarray(x)), np.atleast_1d(np.asarray(y))
            if x.shape != y.shape:
                return name, -1, x.shape, y.shape
            fx, fy = x.reshape(-1), y.reshape(-1)
            ne = xx.bits(fx) != xx.bits(fy) if fx.dtype.kind == "f" else fx != fy
            i = int(np.flatnonzero(ne)[0])
            return name, i, fx[i], fy[i]
    return None


def digest(rc, outs):
    return [rc] + ["%s:%s" % (name, hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]) for name, x in outs]


FINAL = op("estep", "golden")   # after the last operation of every history


def interpret(history, backend, kind, n, twin_of=None, reference=None):
    """Run the history on `backend`.  twin_of(world, op) -> a backend that has been through the replay (closed here);
    reference: a second backend run in step (the oracle, exact mode).  Returns the digest list of the checked calls; raises
    AssertionError naming the operation index, the operation, the first differing output and element and the last plan event."""
    world = World(kind, n)
    out = []
    ops = list(history) + [FINAL]
    for i, o in enumerate(ops):
        rc, got = backend.run(o)
        where = "operation %d %s on a %s context of %d states" % (i, describe(o), kind, n)
        moot = o.expect == "ok" and o.kind in DECODING and not world.last_estep_ok   # (the E-step it would read failed, here as on the twin)
        if o.expect is not None and not moot:
            assert (rc == "ok") == (o.expect == "ok"), "%s: returned %r" % (where, rc)
        if o.kind == "bad_call":
            assert rc == BAD_RC[o.args[0]], "%s: returned %r" % (where, rc)
        if o.kind not in CHECKED:
            assert rc == "ok", "%s: %r" % (where, rc)
        for what, other in (("the twin", twin_of), ("the reference", reference)):
            if other is None or (o.kind not in CHECKED and what == "the twin"):
                continue
            if what == "the twin":
                if o.kind == "bad_call":
                    continue
                tw = twin_of(world, o)
                try:
                    trc, want = tw.run(o)
                finally:
                    tw.close()
            else:
                trc, want = other.run(o)
                if o.kind == "table_info":
                    continue
            assert rc == trc, "%s: returned %r, %s %r; last plan event: %s" % (where, rc, what, trc, world.last_plan_event())
            d = first_difference(got, want, ORACLE_OMITS if what == "the reference" else frozenset())
            assert d is None, "%s: output %s differs from %s at element %d: %r against %r; last plan event: %s" % (
                where, d[0], what, d[1], d[2], d[3], world.last_plan_event())
        if o.kind == "table_info" and len(o.args):
            assert int(got[0][1][0]) == o.args[0], "%s: interval %d" % (where, int(got[0][1][0]))
        if o.kind in STATE_OPS and (rc == "ok" or o.kind in E_STEPS or o.kind == "batch"):
            world.record(o, rc)   # (an E-step that failed is replayed too: it fails on the twin as it did here, and leaves what it left)
        if o.kind in CHECKED:
            out.append(digest(rc, got))
    backend.close()
    return out


def device_twin(hip, golden, kind, n):
    def twin_of(world, o):
        start = world.window(o)
        opts, pool, sel = world.log[start][1] if start < len(world.log) else world.snapshot()
        tw = DeviceBackend(hip, golden, kind, n, opts)
        if pool is not None:
            tw.run(op("load", pool))
            if tuple(sel) != tuple(range(N_SEG[pool])):
                tw.run(op("select", tuple(sel)))
        for x, _ in world.log[start:]:
            tw.run(x)
        return tw
    return twin_of


# ---------------------------------------------------------------------------------------------------------------- hand-written histories
G, R6, RD = PAR_NAMES


def _decodes(seg):
    return [op("decode", seg), op("posterior", seg), op("scales", seg), op("post_counts", seg, 5), op("post_mean", seg, 4), op("post_quantile", seg, 4)]


def _unfuse(kind, n):
    """fast contexts: the back half that keeps the backward table, so that the decoding calls have something to read"""
    return [op("option", "fuse" if n <= 64 else "fuse128", 0)] if kind == "fast" else []


def s1_reload(kind, n):
    """large -> small -> large, medium -> large: the segment count shrinks and grows, a single-bin segment is last, the last and the
    longest segment are decoded after each reload"""
    return [("a", _reloads(kind, n, (("large", G), ("small", R6), ("large", RD)))), ("b", _reloads(kind, n, (("medium", G), ("large", R6), ("small", RD))))]


def _reloads(kind, n, loads):
    h = _unfuse(kind, n)
    for pool, par in loads:
        long_seg = {"large": 7, "small": 2, "medium": 7}[pool]
        h += [op("load", pool)]
        h += [op(d.kind, *d.args, expect="refused") for d in _decodes(-1)] if pool == "small" else [op("bad_call", "decode_before_estep")]   # nothing to decode after a reload
        h += [op("estep", par), op("decode", -1, expect="ok"), op("posterior", long_seg, expect="ok"), op("scales", -1, expect="ok"),
              op("post_counts", long_seg, 5, expect="ok"), op("post_mean", -1, 4, expect="ok"), op("post_quantile", long_seg, 4, expect="ok")]
        h += [              op("viterbi", par, True), op("sample", par, 1, 5)] if pool != "large" else [op("estep", par), op("scales", long_seg, expect="ok")]
    return h


def s2_select(kind, n):
    h = _unfuse(kind, n) + [op("load", "large"), op("estep", G)]
    h += [op("select", selection("large", 0))] + [op(d.kind, *d.args) for d in _decodes(7)]   # refused or the twin's: both are in order
    h += [op("estep", R6)] + [op(d.kind, *d.args, expect="ok") for d in _decodes(7)]
    h += [op("select", selection("large", 1)), op("estep_factored" if kind != "exact" else "estep_segments", RD), op("decode", 3)]
    h += [op("estep", G), op("decode", 3, expect="ok"), op("post_mean", -1, 1, expect="ok"), op("post_quantile", 3, 1, expect="ok")]
    return h


def s3_tables(kind, n):
    pool, big = ("medium", 7) if n < 513 else ("small", 2)   # (1024 states: the exact kernels' E-steps on the shorter pool)
    sels = [selection(pool, 0), selection(pool, 1), tuple(range(N_SEG[pool]))]
    h = _unfuse(kind, n) + [op("load", pool), op("estep", G), op("batch", (G, R6, RD), tuple(sels), "A")]
    h += [op(d.kind, *d.args, expect="refused") for d in _decodes(big)]
    h += [op("estep", R6)] + [op(d.kind, *d.args, expect="ok") for d in _decodes(big)]
    h += [op("viterbi", G, True), op("sample", G, 3, 21), op("estep_segments" if kind == "exact" else "estep", RD)] + [op(d.kind, *d.args, expect="ok") for d in _decodes(-1)]
    if kind != "wide":
        return h
    # wide tables, then the exact kernels' (newer), then wide again
    w = [op("load", pool), op("estep_factored", G), op("decode", big, expect="ok"), op("estep", RD), op("decode", big, expect="ok"), op("posterior", big, expect="ok"),
         op("estep_factored", R6)] + [op(d.kind, *d.args, expect="ok") for d in _decodes(big)] + [
         op("option", "wide_counts", 1), op("estep", G), op("decode", big, expect="ok"), op("option", "wide_counts", 0), op("estep", G), op("decode", big, expect="ok")]
    return [("a", h), ("b", w)]


def s4_ckpt(kind, n):
    """wide: "wide_ckpt" 0 -> 1 -> 0 -> 1 (with "wide_decode_ckpt" on, so that the interval follows it), "wide_decode_ckpt" the same
    under "wide_ckpt" = 1, "wide_counts" and "wide_counts_ckpt" toggled between factored and full-count E-steps"""
    assert kind == "wide"
    h = [op("load", "medium"), op("option", "wide_decode_ckpt", 1)]
    for v, par in ((0, G), (1, R6), (0, RD), (1, G)):
        h += [op("option", "wide_ckpt", v), op("estep_factored", par), op("table_info", 8 if v else 1), op("decode", 7, expect="ok"), op("post_mean", 7, 1, expect="ok")]
    for v, par in ((0, R6), (1, G), (0, RD), (1, R6)):
        h += [op("option", "wide_decode_ckpt", v), op("estep_factored", par), op("table_info", 8 if v else 1), op("posterior", 7, expect="ok"), op("scales", -1, expect="ok")]
    for v, par in ((1, G), (0, R6), (1, RD)):
        h += [op("option", "wide_counts", v), op("estep", par), op("decode", 7, expect="ok"), op("estep_factored", par), op("table_info", 8)]
    for v, par in ((1, G), (0, R6), (1, RD)):
        h += [op("option", "wide_counts_ckpt", v), op("estep", par), op("table_info", 8 if v else 1), op("post_quantile", 7, 4, expect="ok")]
    return h


def s5_tiles(kind, n):
    """the chain options in every order of switching on and off, on the sandwich at tiles of 64 bins"""
    h = _unfuse(kind, n) + [op("load", "sandwich"), op("option", "chunk", 64), op("option", "warmup", 512)]
    # wide: the exact kernels' tables, then the wide ones, which the decoding reads; fast: the full counts keep the backward table
    step = [op("estep", R6), op("estep_factored", G), op("decode", 0, expect="ok")] if kind == "wide" else [op("estep_factored", G), op("estep", G), op("decode", 0, expect="ok")]
    if kind == "wide":
        g, m, x = "wide_gap_tiles", "wide_hom_tiles", "wide_mix_tiles"
        order = [(g, 1), (m, 1), (x, 1), (g, 0), (x, 0), (m, 0), (x, 1), (m, 1), (g, 1), (m, 0), (m, 1), (x, 0), (g, 0), (m, 0)]
        h2 = list(h) + [op("option", g, 1), op("option", m, 1), op("option", x, 1)]
        for k, v in order:
            h += [op("option", k, v)] + step
        h, h1 = h2, h
        for k, v in (("wide_mix_mb", 1), ("wide_mix_mb", 2048), ("wide_gap_min", 129), ("wide_gap_min", 128), ("wide_hom_min", 4000), ("wide_hom_min", 64), ("wide_hom_min", 0)):
            h += [op("option", k, v)] + step
        return [("a", h1), ("b", h)]
    else:
        for k, v in (("hom_tiles", 1), ("gap_tiles", 0), ("hom_tiles", 0), ("gap_tiles", 1), ("hom_tiles", 1), ("hom_min", 129), ("hom_min", 128), ("hom_min", 5000), ("hom_min", 0)):
            h += [op("option", k, v)] + step
    return h


def s6_scratch(kind, n):
    """the users of the per-call scratch in three orders, on segments of different lengths, "vit_tile" changed in between; then an
    E-step whose bits are those of a context that made none of these calls"""
    h = _unfuse(kind, n) + [op("load", "large"), op("estep", G)]
    a = [op("viterbi", G, True), op("sample", G, 1, 11), op("decode", 7, expect="ok"), op("post_counts", 7, 1, expect="ok"), op("post_mean", 7, 1, expect="ok"),
         op("post_quantile", 7, 1, expect="ok"), op("sample", R6, 3, 12), op("viterbi", R6, False)]
    b = [op("option", "vit_tile", 16), op("option", "samp_group", 3), op("sample", G, 7, 13), op("post_counts", -1, 9, expect="ok"), op("viterbi", G, True),
         op("post_quantile", 3, 4, expect="ok"), op("decode", -1, expect="ok"), op("post_mean", 3, 4, expect="ok"), op("post_counts", 3, 5, expect="ok")]
    c = [op("option", "vit_tile", 4096), op("option", "samp_group", 0), op("post_mean", 0, 4, expect="ok"), op("viterbi", RD, False), op("post_quantile", -1, 1, expect="ok"),
         op("sample", RD, 3, 14), op("decode", 0, expect="ok"), op("viterbi", G, True), op("post_counts", 7, 9, expect="ok"), op("sample", G, 1, 15)]
    return [("a", h + a + b + [op("estep", R6)]),
            ("b", h + c + a[:4] + [op("estep", R6), op("load", "small"), op("viterbi", G, True), op("sample", G, 3, 16), op("estep", G), op("decode", 2, expect="ok")])]


def s7_tilings(kind, n):
    h = _unfuse(kind, n) + [op("load", "large")]
    step = [op("estep", G), op("decode", 7), op("estep_factored", R6)]
    for k, v in (("chunk", 1000), ("chunk", 37), ("chunk", 0), ("chunk", 64), ("warmup", 4096), ("warmup", 5), ("warmup", 3072)):
        h += [op("option", k, v)] + step
    if kind == "fast":
        for k, v in (("fuse", 1), ("fuse128", 2), ("fuse", 0), ("fuse128", 0), ("structured", 0), ("structured", 1), ("two_phase", 0), ("two_phase", -1),
                     ("coarse", 2), ("coarse", -1), ("warm_shift", 2), ("merge", 1), ("merge", 0)):
            h += [op("option", k, v)] + step
    else:
        for k, v in (("structured", 0), ("structured", 1)):
            h += [op("option", k, v), op("estep", G), op("decode", 7)]
    return h


def s8_batches(kind, n):
    s0, s1, al = selection("large", 0), selection("large", 1), tuple(range(13))
    h = _unfuse(kind, n) + [op("load", "large")]
    if kind == "exact":
        h += [op("option", "exact_refwd", 1), op("reserve", 20000), op("batch", (G, R6, RD), (s0, s1, al), "A"), op("estep", G), op("decode", 7, expect="ok"),
              op("option", "exact_refwd", -1), op("batch", (R6, G), (s1, s0), "A"), op("reserve"), op("estep", RD), op("posterior", -1, expect="ok")]
        return h
    want = "sums" if kind == "wide" else "A"
    if kind == "wide":
        h += [op("option", "wide_batch", 1)]
    h += [op("batch", (G, R6, RD), (s0, s1, al), want), op("estep", G), op("decode", 7, expect="ok"), op("batch", (RD, G), (s1, al), want),
          op("estep_factored", R6), op("batch", (G, G, R6, RD), (al, s0, s1, s0), "both" if kind == "fast" else want), op("estep", G), op("decode", -1, expect="ok")]
    if kind == "wide":
        h += [op("option", "wide_batch", 0), op("batch", (G, R6), (s0, s1), "A"), op("decode", 7, expect="refused"), op("estep_factored", G), op("decode", 7, expect="ok")]
    return h


def s9_refusals(kind, n):
    h = _unfuse(kind, n) + [op("load", "medium"), op("bad_call", "decode_before_estep"), op("estep", G)]
    for bad in BAD_CALLS_OF[kind]:
        h += [op("bad_call", bad), op("decode", 7, expect="ok"), op("estep", R6 if bad != "n_w_5" else G), op("post_mean", 7, 4, expect="ok"), op("scales", 7, expect="ok")]
    h += [op("load", "small"), op("bad_call", "decode_before_estep"), op("estep_factored" if kind != "exact" else "estep", G), op("bad_call", "nan_quantile"), op("estep", G),
          op("post_quantile", 2, 4, expect="ok")]
    return h


HAZARDS = {"S1_reload": (s1_reload, KINDS), "S2_select": (s2_select, KINDS), "S3_tables": (s3_tables, KINDS), "S4_ckpt": (s4_ckpt, ("wide",)),
           "S5_tiles": (s5_tiles, ("fast", "wide")), "S6_scratch": (s6_scratch, KINDS), "S7_tilings": (s7_tilings, ("fast", "wide")),
           "S8_batches": (s8_batches, KINDS), "S9_refusals": (s9_refusals, KINDS)}
# the sizes each hazard runs at (every size of the kind takes part in some hazard; 1024 states: the reload, the tables and the scratch)
HAZARD_SIZES = {
    "exact": {"S1_reload": (64, 300), "S2_select": (23, 200), "S3_tables": (65, 128), "S6_scratch": (64, 200), "S8_batches": (64, 128, 300), "S9_refusals": (23, 65)},
    "fast": {k: (64, 128) for k in HAZARDS},
    "wide": dict({k: (200, 300) for k in HAZARDS}, S1_reload=(200, 1024), S3_tables=(300, 1024), S6_scratch=(200, 1024), S4_ckpt=(200, 300)),
}
# on the device these hazards refuse exactly what they expect to be refused: every E-step and batch of theirs returns ok (S2 and S7
# hold decodes and factored E-steps that an option in force refuses by design: "fuse", "merge", "structured" = 0)
EXACT_REFUSALS = ("S1_reload", "S3_tables", "S4_ckpt", "S5_tiles", "S6_scratch", "S8_batches", "S9_refusals")
POISONED = (("exact", 64, "S6_scratcha"), ("exact", 64, "S6_scratchb"), ("fast", 64, "S6_scratcha"), ("fast", 64, "S6_scratchb"),
            ("wide", 200, "S6_scratcha"), ("wide", 200, "S6_scratchb"), ("wide", 200, "S4_ckpt"))


# ---------------------------------------------------------------------------------------------------------------- the generator
GEN_MIX = ("load", "load_device", "select", "option", "reserve", "estep", "estep", "estep", "estep_factored", "estep_segments", "batch",
           "decode", "posterior", "scales", "post_counts", "post_mean", "post_quantile", "viterbi", "sample", "bad_call")
GEN_OPTIONS = {
    "exact": (("exact_refwd", (-1, 0, 1)), ("batch_sort", (0, 1)), ("vit_tile", (16, 100, 2048)), ("samp_group", (0, 1, 3)), ("batch_bins", (0, 4096))),
    "fast": (("chunk", (0, 37, 256, 512, 1001, 2048)), ("warmup", (128, 512, 3072)), ("fuse", (0, 1)), ("fuse128", (0, 2)), ("gap_tiles", (0, 1)), ("merge", (0, 1)),
             ("adapt", (0, 1)), ("prev_start", (0, 1)), ("warm_shift", (0, 2)), ("merge1", (-1, 0, 1)), ("coarse", (-1, 2)), ("kc_sub", (2, 4)), ("two_phase", (-1, 0, 2)),
             ("hom_tiles", (0, 1)), ("hom_min", (0, 64)), ("learn", (0, 1)), ("vit_tile", (16, 2048))),
    "wide": (("chunk", (0, 37, 64, 500)), ("warmup", (40, 512, 4096)), ("wide_ckpt", (0, 1)), ("wide_decode_ckpt", (0, 1)), ("wide_counts", (0, 1)), ("wide_counts_ckpt", (0, 1)),
             ("wide_gap_tiles", (0, 1)), ("wide_hom_tiles", (0, 1)), ("wide_mix_tiles", (0, 1)), ("wide_mix_mb", (1, 2048)), ("wide_gap_min", (0, 64)), ("wide_hom_min", (0, 64)),
             ("wide_batch", (0, 1)), ("wide_counts_slab", (0, 64)), ("samp_group", (0, 3))),
}


def generated(kind, n, seed):
    """25 operations drawn with a fixed seed in the mix of scripts/fuzz_gpu_state.py, extended to the calls and options that came
    after it.  A decoding call is drawn only where World.decodable says it must succeed (else an E-step takes its place), so it is
    asserted to."""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    world = World(kind, n)
    h = []

    def emit(o):
        h.append(o)
        if o.kind in STATE_OPS:
            world.record(o)
    for o in _unfuse(kind, n):
        emit(o)
    pool_cycle = [str(x) for x in rng.permutation(["small", "medium", "large"])]
    emit(op("load", pool_cycle[0]))
    n_load = 1
    while len(h) < N_OPS:
        k = str(rng.choice(GEN_MIX))
        if k in NOT_APPLICABLE[kind]:
            k = "estep"
        nseg = N_SEG[world.pool]
        par = PAR_NAMES[int(rng.integers(3))] if rng.random() < 0.5 else PAR_NAMES[len(h) % 3]
        if k in ("load", "load_device"):
            emit(op(k, pool_cycle[n_load % 3] if rng.random() < 0.7 else str(rng.choice(pool_cycle))))
            n_load += 1
        elif k == "select":
            emit(op("select", selection(world.pool, int(rng.integers(2))) if rng.random() < 0.6 else tuple(int(x) for x in rng.integers(0, nseg, size=int(rng.integers(1, nseg + 3))))))
        elif k == "option":
            key, vals = GEN_OPTIONS[kind][int(rng.integers(len(GEN_OPTIONS[kind])))]
            emit(op("option", key, vals[int(rng.integers(len(vals)))]))
        elif k == "reserve":
            emit(op("reserve") if rng.random() < 0.5 else op("reserve", 20000))
        elif k in E_STEPS:
            emit(op(k, par))
        elif k == "batch":
            R = int(rng.integers(2, 5))
            sels = tuple(tuple(int(x) for x in rng.integers(0, nseg, size=int(rng.integers(1, nseg + 2)))) for _ in range(R))
            want = "A" if kind != "wide" or not world.opts.get("wide_batch") else ("sums", "A")[int(rng.integers(2))]
            emit(op("batch", tuple(PAR_NAMES[int(rng.integers(3))] for _ in range(R)), sels, want))
        elif k in DECODING:
            cand = [s for s in range(nseg) if world.decodable(s)]
            if not cand:
                emit(op("estep", par))
                continue
            seg = cand[int(rng.integers(len(cand)))]
            cols = {"post_counts": (1, 5, 9), "post_mean": (1, 4), "post_quantile": (1, 4)}.get(k)
            emit(op(k, seg, *([cols[int(rng.integers(len(cols)))]] if cols else []), expect="ok"))
        elif k == "viterbi":
            emit(op("viterbi", par, bool(rng.integers(2))))
        elif k == "sample":
            emit(op("sample", par, (1, 3, 7)[int(rng.integers(3))], int(rng.integers(1, 1000))))
        elif k == "bad_call":
            emit(op("bad_call", BAD_CALLS_OF[kind][int(rng.integers(len(BAD_CALLS_OF[kind])))]))
    return h


def all_histories():
    """[(id, kind, n, history)]: the hand-written ones at their sizes, then 12 generated ones per kind"""
    out = []
    for kind in KINDS:
        for name, (fn, kinds) in HAZARDS.items():
            if kind in kinds:
                for n in HAZARD_SIZES[kind][name]:
                    parts = fn(kind, n)
                    for part, h in ([("", parts)] if isinstance(parts[0], Op) else parts):   # (a hazard in parts: one history each, a few seconds each)
                        out.append(("%s%s-%s-%d" % (name, part, kind, n), kind, n, h))
        sizes = GENERATED_SIZES[kind]
        for seed in range(N_GENERATED):
            n = sizes[seed % len(sizes)]
            out.append(("gen%02d-%s-%d" % (seed, kind, n), kind, n, generated(kind, n, seed)))
    return out


def history_by_id(hid):
    for h in all_histories():
        if h[0] == hid:
            return h
    raise KeyError(hid)


def expected_refusals(history):
    return sum(1 for o in history if o.kind == "bad_call" or o.expect == "refused")


def child_code(hid, tag):
    """the program of a poisoned child: the history on one long-lived context, no twins; prints its digest list behind `tag`"""
    return ("import sys, json\nsys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import conftest, ctx_history as ch\nfrom psmc_amd import hip\n"
            "hid, kind, n, h = ch.history_by_id(%r)\n"
            "print(%r + json.dumps(ch.interpret(h, ch.DeviceBackend(hip, conftest.Golden(), kind, n), kind, n)))\n") % (
                ROOT, os.path.join(ROOT, "tests"), hid, tag)
