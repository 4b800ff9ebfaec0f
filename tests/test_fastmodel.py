"""The numpy specification of the fast-mode algorithm (tests/fastmodel.py)
against the oracle: checks the algebra (lagged normalisation, shared divisors,
per-tile posterior normalisation, a .* C factorisation) and documents how the
error depends on the warm-up length W."""
import numpy as np
import pytest
import fastmodel


def relmax(x, y):
    return float(np.abs(x - y).max() / np.abs(y).max())


def test_untiled_matches_oracle(golden, oracle):
    p = golden.params("n64_curve")
    segs = golden.segs_small
    ref = oracle.estep(p["a"], p["e"], p["a0"], segs)
    m = fastmodel.estep_fast_model(p["a"], p["e"], p["a0"], segs, T=1 << 30, W=0)
    assert relmax(m["A"], ref["A"]) < 1e-12 and relmax(m["E"], ref["E"]) < 1e-12
    assert abs(m["LL"] - ref["LL"]) < 1e-12 * abs(ref["LL"])


@pytest.mark.parametrize("T,W,tol", [(1024, 4096, 1e-11), (4096, 4096, 1e-11), (512, 8192, 1e-12)])
def test_tiled_matches_oracle(golden, oracle, T, W, tol):
    p = golden.params("n64_curve")
    segs = golden.segs_mid[2:]   # 20000, 12000, 5000, 800 bins
    ref = oracle.estep(p["a"], p["e"], p["a0"], segs)
    m = fastmodel.estep_fast_model(p["a"], p["e"], p["a0"], segs, T=T, W=W)
    assert relmax(m["A"], ref["A"]) < tol and relmax(m["E"], ref["E"]) < tol
    assert abs(m["LL"] - ref["LL"]) < tol * abs(ref["LL"])


def test_short_overlap_alone_is_wrong_and_repair_fixes_it(golden, oracle):
    """An overlap far below the forgetting length must NOT pass by itself (this is what the
    verify kernel of the HIP path detects); with verify + repair it is right again, at a
    fraction of the work a long fixed overlap would cost."""
    p = golden.params("n64_curve")
    segs = golden.segs_mid[2:4]
    ref = oracle.estep(p["a"], p["e"], p["a0"], segs)
    m = fastmodel.estep_fast_model(p["a"], p["e"], p["a0"], segs, T=1024, W=128)
    assert relmax(m["A"], ref["A"]) > 1e-6
    st = {}
    m = fastmodel.estep_fast_model(p["a"], p["e"], p["a0"], segs, T=1024, W=128, tol=1e-12, stats=st)
    assert relmax(m["A"], ref["A"]) < 1e-11 and relmax(m["E"], ref["E"]) < 1e-11
    assert abs(m["LL"] - ref["LL"]) < 1e-12 * abs(ref["LL"])
    assert st["fwd_rounds"] >= 1 and st["fwd_steps"] < 4 * st["bins"]


def test_no_overlap_with_repair(golden, oracle):
    p = golden.params("n64_flat")
    segs = golden.segs_small
    ref = oracle.estep(p["a"], p["e"], p["a0"], segs)
    m = fastmodel.estep_fast_model(p["a"], p["e"], p["a0"], segs, T=500, W=0, tol=1e-12)
    assert relmax(m["A"], ref["A"]) < 1e-11 and relmax(m["E"], ref["E"]) < 1e-11


def test_structured_factorisation(golden):
    """The O(N) sweeps rest on a[k][l] = P_k qa_l below and R_k c_l above the diagonal (core.c:112-122):
    every golden transition matrix factors to 64 ulp with dd >= 0, the two-scan step equals the dense
    product, and a capped matrix (aux.c:115-127) or a generic one is rejected (dense fallback)."""
    rng = np.random.default_rng(3)
    for key in golden.param_keys() + ["n128"]:
        a = golden.n128["n128_curve.a"] if key == "n128" else golden.params(key)["a"]
        f = fastmodel.factor_structure(a)
        assert f is not None, key
        x = rng.random(a.shape[0]) ** 3
        assert relmax(fastmodel.struct_step_forward(f, x), a.T @ x) < 1e-13
        assert relmax(fastmodel.struct_step_backward(f, x), a @ x) < 1e-13
    a = golden.params("n64_curve")["a"].copy()
    a[:, 40] = a[:, 40:].sum(1); a[:, 41:] = 0.0
    assert fastmodel.factor_structure(a) is None
    b = rng.random((64, 64)); b /= b.sum(1, keepdims=True)
    assert fastmodel.factor_structure(b) is None


def test_struct_option_of_the_model(golden, oracle):
    """estep_fast_model(struct=True): both sweeps through the two-scan steps.  Not the dense model's bits (the factorisation is good to 64 ulp
    per entry, not exact), the oracle's numbers per cell; and the dense model's bits where the criterion refuses the matrix."""
    p = golden.params("n64_curve")
    segs = golden.segs_small[:9]
    ref = oracle.estep(p["a"], p["e"], p["a0"], segs)
    dense = fastmodel.estep_fast_model(p["a"], p["e"], p["a0"], segs, T=1 << 30, W=0)
    st = fastmodel.estep_fast_model(p["a"], p["e"], p["a0"], segs, T=1 << 30, W=0, struct=True)
    assert not np.array_equal(st["A"], dense["A"])
    for m in (dense, st):
        assert fastmodel.cell_error(m["A"], ref["A"])[0] <= 1e-12 and fastmodel.cell_error(m["E"], ref["E"])[0] <= 1e-12
        assert abs(m["LL"] - ref["LL"]) <= 1e-14 * abs(ref["LL"])
    a = p["a"].copy()   # capped: not of the form
    a[:, 40] = a[:, 40:].sum(1); a[:, 41:] = 0.0
    assert fastmodel.factor_structure(a) is None
    d2 = fastmodel.estep_fast_model(a, p["e"], p["a0"], segs, T=64, W=4096)
    s2 = fastmodel.estep_fast_model(a, p["e"], p["a0"], segs, T=64, W=4096, struct=True)
    assert np.array_equal(d2["A"], s2["A"]) and np.array_equal(d2["E"], s2["E"]) and d2["LL"] == s2["LL"]
    # cell_error: no floor relative to the largest cell, and the index of the worst
    x = np.array([[1.0, 1e-200], [0.0, 3.0]])
    assert fastmodel.cell_error(x * np.array([[1.0, 1.0 + 1e-9], [1.0, 1.0]]), x) == (pytest.approx(1e-9, rel=1e-6), (0, 1))
    assert fastmodel.cell_error(np.zeros(3), np.zeros(3)) == (0.0, None)
    assert fastmodel.cell_bound(3e-15) == 32 * 64 * 2.0 ** -53 and fastmodel.cell_bound(1e-13) == 32e-13


# ---------------------------------------------------------------------------------------------
# The CPU side of tests/test_gpu_fast_cells.py (the fast E-step up to 128 states, cell by cell in the anchored regime).
def test_fast_cells_case_table():
    """The literal tables of the GPU file against the host model: which (model, n) pairs are HMMs at all -- the four drop-outs, no others --
    and which of the cases the factorisation criterion refuses (what the GPU file asserts against fast_diag()["structured"])."""
    import test_gpu_fast_cells as cells
    import test_gpu_wide_fast_edges as edges
    assert cells.MODELS is edges.MODELS and len(cells.MODELS) == 13
    assert cells.SIZES == (2, 3, 63, 64, 65, 127, 128) and set(cells.NOT_HMM) <= set(cells.MODELS)
    table = [(n, name) for n in cells.SIZES for name in cells.MODELS if cells.is_hmm(cells.host_model(name, n))]
    assert table == cells.CASES and len(table) == 70
    assert cells.STRUCT_REFUSED <= set(cells.CASES)
    for n, name in cells.CASES:
        a, e, a0 = cells.host_model(name, n)
        assert a.shape == (n, n) and e.shape == (3, n) and a0.shape == (n,)
        assert (fastmodel.factor_structure(a) is None) == ((n, name) in cells.STRUCT_REFUSED), (n, name)
    assert not any(n > 64 for n, _ in cells.STRUCT_REFUSED)   # (the exact fallback beyond 64 states has no case here)


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 127, 128])
def test_fast_cells_reference_error(golden, oracle, n):
    """A condition on the inputs of tests/test_gpu_fast_cells.py, not a measurement of the device: on every case the oracle's A, E and LL
    are finite and non-negative, and E_ref -- the untiled numpy model, dense and structured, against the oracle over EVERY cell above
    2^-900 -- is at most 1e-12, over the five triangular sums as well.  Observed: <= 4.4e-13 (rho0 = 1e-6 at 128 states, structured;
    dense <= 2.1e-13, theta0 = 0.3 at 128 states), typically 2e-14 .. 1e-13; LL within 6e-16 relative."""
    import test_gpu_fast_cells as cells
    segs = cells.cells_segs(golden)
    for m, name in cells.CASES:
        if m != n:
            continue
        par, o, r = cells.reference(oracle, golden, n, name)
        assert cells.is_hmm(par)
        assert np.isfinite(o["A"]).all() and np.isfinite(o["E"]).all() and np.isfinite(o["LL"]) and (o["A"] >= 0).all() and (o["E"] >= 0).all()
        print("E_ref n %3d %-26s cell %.2e (dense %.2e struct %.2e) sums %.2e LL %.1e; B %.2e" % (
            n, name, r["cell"], r["dense"][0], r["struct"][0], r["tri"], r["LL"], fastmodel.cell_bound(r["cell"])))
        assert r["cell"] <= 1e-12 and r["tri"] <= 1e-12 and r["LL"] <= 1e-14, (n, name, r)
        assert (o["A"] > fastmodel.CELL_FLOOR).all() and (o["E"] > fastmodel.CELL_FLOOR).all()   # the gate covers all n^2 + 2n cells
    assert sum(len(s) for s in segs) == 4827


# ---------------------------------------------------------------------------------------------
# The CPU side of tests/test_gpu_wide_fast_edges.py (the wide fast E-step, 129 .. 256 states).
def test_factorisation_criterion_on_the_extreme_models():
    """api.hip factor_structure restated in numpy (fastmodel.factor_structure: every off-diagonal entry to 64 ulp, both corner
    entries above 1e-280, dd >= 0) on the models of part B at the four sizes and at 200 states: it refuses exactly the models
    the GPU test lists as REFUSED -- at most a quarter of the list -- and for the reason the list gives; the others must run
    on the device.  The same answer at every size."""
    import test_gpu_wide_fast_edges as edges
    assert 4 * len(edges.REFUSED) <= len(edges.MODELS) and set(edges.REFUSED) <= set(edges.MODELS)
    assert not set(edges.HARSH) & set(edges.REFUSED)
    for name in edges.MODELS:
        for n in list(edges.SIZES) + [200]:
            a, e, a0 = edges.model(name, n)
            f = fastmodel.factor_structure(a)
            assert (f is None) == (name in edges.REFUSED), (name, n)
            if f is not None:
                assert np.isfinite(a).all() and np.isfinite(e).all() and (a >= 0).all() and (a0 >= 0).all()
                x = np.linspace(0.1, 1.0, n) ** 3
                assert relmax(fastmodel.struct_step_forward(f, x), a.T @ x) < 1e-13
                assert relmax(fastmodel.struct_step_backward(f, x), a @ x) < 1e-13
            else:
                _refused_for_the_listed_reason(edges, name, a)


def _refused_for_the_listed_reason(edges, name, a):
    """a, which the criterion refuses, is refused for the reason edges.REFUSED[name] gives"""
    n = a.shape[0]
    assert fastmodel.factor_structure(a) is None, (name, n)
    if "corner" in edges.REFUSED[name]:
        assert a[0, n - 1] == 0.0 and not a[n - 1, 0] > 1e-280, (name, n)
    else:   # the off-diagonal entries do factor; the remainder of the diagonal is negative
        assert fastmodel.factor_structure(a, ulps=1e30) is None and a.min() < 0, (name, n)
        P, qa, R, c = a[:, 0].copy(), a[n - 1] / a[n - 1, 0], a[:, n - 1].copy(), a[0] / a[0, n - 1]
        P[0] = R[n - 1] = 0.0; qa[n - 1] = c[0] = 0.0
        assert (np.diag(a) - P * qa - R * c).min() < 0, (name, n)


# ---------------------------------------------------------------------------------------------
# The CPU side of tests/test_gpu_wide_cells.py (the wide fast path at 129 .. 1024 states, cell by cell in the anchored regime).
def test_wide_cells_case_table():
    """The literal table of the GPU file against the host model and the criterion, at all ten sizes and all thirteen models: a pair is either an
    HMM (a, e, a0 finite, a >= 0) that factor_structure accepts, or it is in REFUSED -- no HMM, refused, and refused for the reason
    tests/test_gpu_wide_fast_edges.py lists.  The four models of the sizes beyond 256 states are accepted everywhere."""
    import test_gpu_wide_cells as wc
    import test_gpu_wide_fast_edges as edges
    assert wc.MODELS is edges.MODELS and len(wc.MODELS) == 13 and set(wc.REFUSED) == set(edges.REFUSED)
    assert wc.SIZES == (129, 192, 193, 256, 257, 512, 513, 768, 769, 1024)
    assert len(wc.CASES) == 4 * 13 + 6 * 4 and not set(wc.LARGE_MODELS) & set(wc.REFUSED)
    assert all(name in wc.LARGE_MODELS for n, name in wc.CASES if n > 256)
    for n in wc.SIZES:
        for name in wc.MODELS:
            a, e, a0 = wc.host_model(name, n)
            assert a.shape == (n, n) and e.shape == (3, n) and a0.shape == (n,)
            refused = n in wc.REFUSED.get(name, ())
            assert wc.is_hmm((a, e, a0)) == (not refused), (n, name)
            assert (fastmodel.factor_structure(a) is None) == refused, (n, name)
            if refused:
                _refused_for_the_listed_reason(edges, name, a)


@pytest.mark.parametrize("n", [129, 257, 1024])
def test_wide_cells_criterion_refuses_what_it_must(n):
    """Around the accepted models of the large sizes: one off-diagonal entry off by 1e-13 relative (450 ulp: beyond the 64 the criterion admits),
    a capped matrix (aux.c:115-127), a corner at zero and a diagonal entry below P.qa + R.c are all refused; 32 ulp on one entry is not."""
    import test_gpu_wide_cells as wc
    for name in wc.LARGE_MODELS:
        a = wc.host_model(name, n)[0]
        assert fastmodel.factor_structure(a) is not None
        k, l = 4 + int(np.argmax(a[4:n - 1, 3])), 3   # an entry inside the lower triangle, off the rows and columns the factors are read from
        assert a[k, l] > 1e-200
        b = a.copy(); b[k, l] *= 1.0 + 1e-13
        assert fastmodel.factor_structure(b) is None, (name, n)
        b = a.copy(); b[k, l] *= 1.0 + 32 * 2.0 ** -52
        assert fastmodel.factor_structure(b) is not None, (name, n)
        b = a.copy(); b[:, 40] = b[:, 40:].sum(1); b[:, 41:] = 0.0
        assert fastmodel.factor_structure(b) is None, (name, n)
        b = a.copy(); b[0, n - 1] = 0.0
        assert fastmodel.factor_structure(b) is None, (name, n)
        b = a.copy(); b[n // 2, n // 2] = 0.0
        assert fastmodel.factor_structure(b) is None, (name, n)


@pytest.mark.parametrize("n", [129, 256, 257, 1024])
def test_wide_cells_reference_error(golden, oracle, n):
    """A condition on the inputs of tests/test_gpu_wide_cells.py, not a measurement of the device: for the four models of the large sizes on the
    small input (1127 bins) the oracle's A, E and LL are finite and non-negative, and E_ref -- the untiled numpy model, dense and structured,
    against the oracle over EVERY cell above 2^-900 -- is at most 1e-12, over the five triangular sums as well.  Observed: <= 2.1e-13 (1024
    states), so B = 32 max(E_ref, 64 ulp) stays below 7e-12."""
    import test_gpu_wide_cells as wc
    segs = wc.small_segs(golden)
    assert sum(len(s) for s in segs) == 1127
    for name in wc.LARGE_MODELS:
        a, e, a0 = wc.host_model(name, n)
        o = oracle.estep(a, e, a0, segs)
        assert np.isfinite(o["A"]).all() and np.isfinite(o["E"]).all() and np.isfinite(o["LL"]) and (o["A"] >= 0).all() and (o["E"] >= 0).all()
        r = fastmodel.reference_error(a, e, a0, segs, o)
        print("E_ref n %4d %-26s cell %.2e (dense %.2e struct %.2e) sums %.2e LL %.1e; B %.2e; cells above 2^-900: %d of %d" % (
            n, name, r["cell"], r["dense"][0], r["struct"][0], r["tri"], r["LL"], fastmodel.cell_bound(r["cell"]),
            int((o["A"] > fastmodel.CELL_FLOOR).sum()), n * n))
        assert r["cell"] <= 1e-12 and r["tri"] <= 1e-12 and r["LL"] <= 1e-14, (n, name, r)


# ---------------------------------------------------------------------------------------------
# The CPU side of tests/test_gpu_decode_cells.py (decoding from the fast tables, entry by entry in the anchored regime).
def test_decode_cells_case_table():
    """The case tables of the GPU file are those of the two cell files: every pair it runs is an HMM (NOT_HMM / REFUSED list the others, and
    none of those is run), the pairs that run the dense sweeps are STRUCT_REFUSED -- which the numpy criterion refuses, and no other -- and the
    paths of a size are the ones its kernels have."""
    import test_gpu_decode_cells as dc
    import test_gpu_fast_cells as cells
    import test_gpu_wide_cells as wc
    small = [c for c in dc.CASES if c[0] <= 128]
    wide = [c for c in dc.CASES if c[0] > 128]
    assert small == cells.CASES and len(small) == 70 and len(wide) == 10 * 4 + 4 * 6 and len(set(dc.CASES)) == len(dc.CASES)
    assert {n for n, _ in small} == set(cells.SIZES) and {n for n, _ in wide} == set(wc.SIZES)
    assert not any(n in cells.NOT_HMM.get(name, ()) for n, name in small) and not any(n in wc.REFUSED.get(name, ()) for n, name in wide)
    assert set(wide) == {(n, name) for n, name in wc.CASES if n not in wc.REFUSED.get(name, ())}
    assert {name for n, name in wide if n > 256} == set(wc.LARGE_MODELS)
    for n, name in dc.CASES:
        par = dc.host_model(name, n)
        assert cells.is_hmm(par) and par[0].shape == (n, n), (n, name)
        refused = fastmodel.factor_structure(par[0]) is None
        assert refused == ((n, name) in cells.STRUCT_REFUSED), (n, name)
        tags = [p[0] for p in dc.paths(n, refused)]
        assert tags == (["D1", "D2"] if n <= 64 else ["D1"] if n <= 128 else ["D3", "D4"]), (n, tags)
        assert [p[4] for p in dc.paths(n, refused)] == ([not refused, False] if n <= 64 else [True] * len(tags)), (n, name)
    assert dc.D0_CASES <= set(dc.CASES) and len(dc.D0_CASES) == 8
    assert all(-n % 64 for n in dc.D0_SIZES)           # sizes that leave padded states


def _decode_cpu_cases(n):
    import test_gpu_decode_cells as dc
    return [name for m, name in dc.CASES if m == n]


@pytest.mark.parametrize("n", [3, 65, 129])
def test_decode_model_reference_error(golden, oracle, n):
    """decode_model, dense and structured, against the oracle on small_segs (1127 bins) over every HMM model of the size: a condition on the
    formulas and on the inputs of tests/test_gpu_decode_cells.py, not a measurement of the device.  Every E_ref below 1e-12 (so every B of the
    GPU file stays below 3.2e-11), rows sum to 1 within 1e-13, the model's path is the oracle's at every position, nothing the oracle puts at or
    below 2^-900 is above 2^-899 in the model.  Observed: post <= 1.3e-13, maxp <= 7.6e-14, recomb <= 1.6e-14 absolute, scales <= 1.4e-14,
    counts <= 7.9e-14, mean <= 3.0e-14; the smallest relative top-two gap 1.5e-7 (129 states, rho0 = 0.1).  On the longer input of the GPU file
    up to 256 states (cells_segs, 4827 bins) and at the sizes beyond, every E_ref stays below 7.2e-13 (post, rho0 = 1e-6 at 256 states)."""
    import test_gpu_decode_cells as dc
    import test_gpu_wide_cells as wc
    segs = wc.small_segs(golden)
    names = _decode_cpu_cases(n)
    assert len(names) == 10
    for name in names:
        a, e, a0 = dc.host_model(name, n)
        w = fastmodel.decode_weights(n, dc.MODELS[name](4)[2])
        assert w.shape == (4, n) and (w >= 0).all() and (w[3] == 1).all() and w[2].sum() == n - n // 2 and w[0, 0] == 0 and (np.diff(w[0]) > 0).all()
        r = fastmodel.decode_reference_error(a, e, a0, segs, oracle, w=w)
        print("E_ref n %3d %-26s %s ties %d gap %.1e rowsum %.1e" % (
            n, name, " ".join("%s %.1e" % (k, r[k]) for k in fastmodel.DECODE_OUTPUTS), r["ties"], r["gap"], r["rowsum"]))
        assert ("struct" in r) == ((n, name) not in dc.cells.STRUCT_REFUSED)
        assert all(r[k] < 1e-12 for k in fastmodel.DECODE_OUTPUTS), (n, name, r)
        assert r["rowsum"] <= 1e-13 and r["ties"] == 0 and r["below"] <= 2.0 ** -899, (n, name, r)
        assert r["gap"] > 2 * fastmodel.cell_bound(r["post"]), (n, name, r)   # no position of the case is excused from the path gate


class _ModelContext:
    """The decoding calls of HipEStep answered by decode_model: what decode_all of the GPU file is driven with on the CPU.  wrong: {output: a
    function that spoils it in place}."""

    def __init__(self, par, segs, wrong=None):
        self.n, self.wrong = par[0].shape[0], wrong or {}
        self.m = [fastmodel.decode_model(par[0], par[1], par[2], s) for s in segs]

    def _out(self, k, s, x):
        x = x.copy()
        if k in self.wrong:
            self.wrong[k](s, x)
        return x

    def posterior(self, s, want_post=True, want_recomb=True):
        return (self._out("post", s, self.m[s]["post"]) if want_post else None, self._out("recomb", s, self.m[s]["recomb"]) if want_recomb else None)

    def decode(self, s):
        return self._out("path", s, self.m[s]["path"]), self._out("maxp", s, self.m[s]["maxp"])

    def scales(self, s):
        return self._out("scales", s, self.m[s]["scales"])

    def post_counts(self, s, cnt1, cnt):
        add = fastmodel.add_counts(np.zeros_like(cnt), self.m[s]["post"], cnt1)
        cnt += self._out("counts", s, add)
        return cnt

    def post_mean(self, s, w):
        return self._out("mean", s, self.m[s]["post"] @ np.atleast_2d(w).T)


def test_decode_cells_gates_refuse_what_the_old_tolerances_accept(golden, oracle):
    """Errors injected into the outputs, not into a kernel: decode_all of tests/test_gpu_decode_cells.py, driven by the numpy model, passes every
    gate as it is, and names the gate when one small posterior entry is off by 1e-9 relative (1e-9 absolute accepts anything there), when a
    row, maxp, recomb, a scale, one segment's counts or a mean is off by 1e-10, when recomb at position L is not exactly 0, when the all-ones mean is
    not 1, and when the path leaves the oracle's at one position."""
    import test_gpu_decode_cells as dc
    n, name = 3, "rho_1e-6"
    segs = dc.data(golden, n)
    R = dc.reference(oracle, golden, n, name)
    assert max(R["B"].values()) < 1e-11 and all(c.all() for c in R["clear"])
    out, bad = dc.Outputs(), []
    assert dc.decode_all(_ModelContext(R["par"], segs), segs, R, out, bad, "model") == 0 and bad == [], bad[:3]
    assert all(out.err[k][0] <= R["eref"][k] for k in dc.OUTPUTS)

    def small_entry(s, x):
        if s == 9:
            k = int(np.argmin(x[1500]))
            assert x[1500, k] < 0.5
            x[1500, k] *= 1.0 + 1e-9

    def at(seg, i, f):
        def spoil(s, x):
            if s == seg:
                x[i] = f(x[i])
        return spoil

    cases = [("post", small_entry, "(P1) post"),
             ("post", at(7, 5, lambda r: r * (1.0 + 1e-10)), "(P1) a row sums"),
             ("maxp", at(8, 17, lambda v: v * (1.0 + 1e-10)), "(P2) maxp"),
             ("recomb", at(8, 400, lambda v: v + 1e-10), "(P3) recomb:"),
             ("recomb", at(3, -1, lambda v: 2.0 ** -1000), "(P3) recomb at position L"),
             ("scales", at(9, 2048, lambda v: v * (1.0 + 1e-10)), "(P4) scales"),
             ("path", at(12, 150, lambda v: (v + 1) % 3), "(P5) path"),
             ("counts", at(9, slice(None), lambda v: v * (1.0 + 1e-10)), "(P6) post_counts, 9 columns, running totals"),
             ("counts", at(0, slice(None), lambda v: v * (1.0 + 1e-10)), "segment 0 (P6) post_counts"),      # one bin of 4827: no total sees it
             ("counts", at(1, (0, 0), lambda v: 1e-300), "segment 1 (P6) post_counts, 1 columns: a cell the oracle leaves at 0"),
             ("mean", at(4, (10, 0), lambda v: v * (1.0 + 1e-10)), "(P6) post_mean")]
    for k, spoil, gate in cases:
        bad = []
        dc.decode_all(_ModelContext(R["par"], segs, {k: spoil}), segs, R, dc.Outputs(), bad, "spoiled")
        assert any(gate in b for b in bad), (k, gate, bad[:3])
    bad = []
    ones = lambda s, x: x.__setitem__((slice(None), 3), 1.0 + 1e-10) if x.shape[1] == 4 else None
    dc.decode_all(_ModelContext(R["par"], segs, dict(mean=ones)), segs, R, dc.Outputs(), bad, "spoiled")
    assert any("all-ones column" in b for b in bad) and any("(P7) post_mean" in b for b in bad), bad[:3]


def test_decode_model_pieces(golden, oracle):
    """decode_model's conventions on one segment: position L on its own formula, recomb 0 there, the scales are the oracle's s, the first
    maximum wins a tie; count_tables has records shorter and longer than their segments; and the gates' yardstick sees one entry of 1e-200
    that is off by 1e-9 relative -- which 1e-9 absolute does not."""
    p = golden.params("n64_curve")
    seg = golden.segs_small[7]
    m = fastmodel.decode_model(p["a"], p["e"], p["a0"], seg)
    ms = fastmodel.decode_model(p["a"], p["e"], p["a0"], seg, struct=True)
    f, b, s, lk, chk = oracle.fwd_bwd(p["a"], p["e"], p["a0"], seg)
    post, rec = oracle.post_full(p["a"], p["e"], seg, f, b, s)
    for x in (m, ms):
        assert x["post"].shape == (len(seg), 64) and x["recomb"][-1] == 0.0 and np.array_equal(x["path"], x["post"].argmax(1))
        assert fastmodel.cell_error(x["post"], post[1:])[0] < 1e-12 and fastmodel.cell_error(x["scales"], s[1:])[0] < 1e-13
        assert np.abs(x["recomb"] - rec[1:]).max() < 1e-13 and fastmodel.cell_error(x["post"][-1], f[-1] / f[-1].sum())[0] < 1e-13
    assert not np.array_equal(m["post"], ms["post"])
    capped = p["a"].copy(); capped[:, 40] = capped[:, 40:].sum(1); capped[:, 41:] = 0.0
    assert fastmodel.decode_model(capped, p["e"], p["a0"], seg, struct=True) is None
    one = fastmodel.decode_model(p["a"], p["e"], p["a0"], seg[:1])
    assert one["post"].shape == (1, 64) and one["recomb"][0] == 0.0 and one["scales"][0] == (p["a0"] * p["e"][seg[0]]).sum()
    segs = golden.segs_small[:4]
    t = fastmodel.count_tables(segs)
    assert sorted(t) == [1, 5, 9] and [len(x) for x in t[9]] == [1, 0, 8, 63] and all(x.dtype == np.int32 and x.shape[1] == 9 for x in t[9])
    import test_gpu_fast_cells as cells
    import test_gpu_wide_cells as wc
    # the records of the GPU file's two inputs: shorter and longer than a segment of several tiles, ending inside a tile and a block of eight rows
    assert fastmodel.count_lengths(cells.cells_segs(golden)) == [1, 0, 8, 63, 64, 65, 127, 126, 1005, 2051, 3, 70, 151]
    assert fastmodel.count_lengths(wc.small_segs(golden)) == [1, 0, 8, 63, 64, 65, 127, 126, 305, 3, 70, 151]
    assert all(l % T > 1 and l % 8 > 1 for l in (126, 151) for T in (37, 64, 256))   # neither the last nor the first row of a tile or block
    assert 2051 - 2048 == 3 and 129 % 64 == 1                      # into the second block of PCNT_BLK; position L alone in a tile at chunk 64
    assert all(np.array_equal(x, y) for x, y in zip(t[5], fastmodel.count_tables(segs)[5]))
    cnt = fastmodel.add_counts(np.zeros((64, 9)), m["post"][:3], t[9][2])      # a record longer than its segment: the first L rows count
    assert np.allclose(cnt, m["post"][:3].T @ t[9][2][:3].astype(float), rtol=1e-15, atol=0)
    assert fastmodel.top_two_gap(np.array([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25 + 2.0 ** -30]])).tolist() == [0.5, 0.5 - 2.0 ** -29]
    x = np.array([[1.0 - 1e-200, 1e-200]])
    y = x * np.array([[1.0, 1.0 + 1e-9]])
    assert np.abs(y - x).max() < 1e-9 and fastmodel.cell_error(y, x) == (pytest.approx(1e-9, rel=1e-6), (0, 1))
    assert fastmodel.long_mean(np.array([[0.25, 0.75]]), np.array([[1.0, 1.0], [0.0, 2.0]])).tolist() == [[1.0, 1.5]]


def test_untiled_matches_oracle_per_cell_at_200_states(golden, oracle):
    """Before the per-vector gates of the wide fast path (tests/test_gpu_wide_fast.py gate_factored, FAST_TOL_CELL = 1e-9) are
    relied on: the algorithm itself -- this file's numpy model, untiled, in double -- agrees with the oracle on every gated cell
    of each of the seven vectors at least ten times tighter, on the inputs the GPU tests use: the golden parameters at 200 states
    on the ragged segments and on the sets of the call sequence, and every accepted extreme model (at 200 states) on the data
    of part B.  Observed: <= 4.2e-13 (rho0 = 1e-6, DG); an input that missed this would not be fit for the gate."""
    import os
    from conftest import GOLD
    from psmc_amd.parity import factored_error_metrics, tri_sums, FACTORED_NAMES
    import test_gpu_wide_fast_edges as edges
    from test_gpu_wide_fast import FAST_TOL_CELL
    w = dict(np.load(os.path.join(GOLD, "estep_wide.npz")))
    gold = (w["n200.a"], w["n200.e"], w["n200.a0"])
    cases = [("golden n200, ragged", gold, edges.ragged_segs(golden)), ("golden n200, sequence", gold, golden.segs_small + golden.segs_mid[4:])]
    cases += [(name, edges.model(name, 200), edges.extremes_segs(golden)) for name in edges.MODELS if name not in edges.REFUSED]
    worst = 0.0
    for what, (a, e, a0), segs in cases:
        o = oracle.estep(a, e, a0, segs)
        m = fastmodel.estep_fast_model(a, e, a0, segs, T=1 << 30, W=0)
        x = factored_error_metrics(dict(sums=tri_sums(m["A"]), E=m["E"], LL=m["LL"]), dict(sums=tri_sums(o["A"]), E=o["E"], LL=o["LL"]), a, e)
        cell = max(x[v + "_cell"] for v in FACTORED_NAMES)
        worst = max(worst, cell)
        assert cell <= FAST_TOL_CELL / 10, (what, x)
        assert max(x[v + "_l1"] for v in FACTORED_NAMES) <= 1e-11 and x["QA"] <= 1e-11 and x["QE"] <= 1e-11 and x["LL"] <= 1e-13, (what, x)
    print("fastmodel vs oracle, worst gated cell: %.2e" % worst)


def test_per_vector_gate_refuses_what_the_block_gate_accepts():
    """An error injected into the reference, not the kernel: one cell of weight 1e-5 of its vector's largest, off by 1e-6
    relative.  The block gate of tests/test_gpu_wide_fast.py before the per-vector gates (max |x - ref| / max |ref| < 1e-10 over
    the whole of SL | SU | DG | CL | CU) accepts it; gate_factored must not -- in whichever of the seven vectors it sits."""
    import conftest
    from test_gpu_wide_fast import check, gate_factored, relmax as block, FAST_TOL_STATS, WORST
    seen, worst = len(conftest.FAST_METRICS), dict(WORST)
    try:
        _inject_and_gate(check, gate_factored, block, FAST_TOL_STATS)
    finally:   # the injected errors are not measurements: keep them out of the session's summary
        del conftest.FAST_METRICS[seen:]
        WORST.clear(); WORST.update(worst)


def _inject_and_gate(check, gate_factored, block, FAST_TOL_STATS):
    rng = np.random.default_rng(5)
    n = 193
    sums = np.exp(rng.normal(0.0, 2.0, size=(5, n))) * 1e3
    sums[2] *= 50.0                                  # the diagonal counts dominate the block
    E = np.exp(rng.normal(0.0, 2.0, size=(2, n))) * 1e3
    r = dict(sums=sums.copy(), E=E.copy(), LL=-12345.678)
    gate_factored(r, sums, E, r["LL"], "unperturbed")
    for v in range(7):
        rs, rE = sums.copy(), E.copy()
        vec = rs[v] if v < 5 else rE[v - 5]
        k = (0, n - 1, n // 2, 63 * 3, 64 * 3, 1, n - 2)[v]   # first, last, lane 63's first state, the state after it ...
        vec[k] = 1e-5 * np.delete(vec, k).max()
        ref = dict(sums=rs.copy(), E=rE.copy())
        vec[k] *= 1.0 + 1e-6
        bad = dict(sums=rs, E=rE, LL=r["LL"])
        assert block(bad["sums"], ref["sums"]) < FAST_TOL_STATS and block(bad["E"], ref["E"]) < FAST_TOL_STATS   # the old gate: passes
        with pytest.raises(AssertionError):
            gate_factored(bad, ref["sums"], ref["E"], r["LL"], "perturbed cell %d of vector %d" % (k, v))
        with pytest.raises(AssertionError):
            check(bad, ref["sums"], ref["E"], r["LL"], "perturbed cell %d of vector %d" % (k, v))
