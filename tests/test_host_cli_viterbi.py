"""PSMC_VITERBI=<path>: after the EM rounds `psmc` writes the Viterbi path under the final parameters -- per sequence a line
`VS name L score` (%.6f) and one `VC name start end k t_k` per run of equal states (1-based inclusive bins, t_k = avg_t[k] * theta
as a DC line prints it; psmc_amd/host/run.c).  It needs no decoding option, and the -o / stdout stream stays byte for byte what it
is without the variable.

On the CPU the E-step backend is the oracle (tests/host_oracle_main.c, built as tests/test_host_cli_tmrca.py builds it), which has
no `viterbi` member: the host's own dense recursion (psmc_viterbi_host) runs.  On the GPU `psmc` calls psmc_hip_viterbi: exact mode
must write the oracle-backed binary's bytes, one context or two shards.

What the file is compared with: the numpy restatement (tests/viterbi_model.py) under the parameters of the last RD block, rebuilt
through psmc_amd.hostlib from the PA line.  A PA line holds nine decimals, so the rebuilt model is the run's to within 5e-10 per
parameter, not to the bit, and a score over thousands of bins feels that in its sixth decimal (measured on the restatement alone:
moving every parameter by 5e-10 moves the score of small.psmcfa's second sequence by 1e-6).  So: runs and states are compared
exactly; t_k within 1e-6 (six printed decimals) + 1e-7; the score within 5e-7 (six printed decimals) + 1.5 x 5e-10 x
sum_i |d score / d parameter_i|, the derivative taken along the path by central differences on the model (first order, half as
much again for the rest).  Bit-exactness of the device against the host recursion and the reference is the business of the GPU
tests here (the same bytes as the oracle-backed binary) and of tests/test_gpu_viterbi.py."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import viterbi_model as vm
from test_host_cli_tmrca import BUILD, CLI, HOST, ROOT, args_of, golden_text, input_segments, oracle_psmc, psmc  # noqa: F401 (fixtures)

ENV_KEYS = ("PSMC_HIP_MODE", "PSMC_HIP_DECODE", "PSMC_HIP_WIDE", "PSMC_HIP_OPTIONS", "PSMC_HIP_DEVICES", "PSMC_TMRCA", "PSMC_VITERBI")


def run(exe, args, track, **env):
    """(stdout, stderr, the file's text or None when none was written)"""
    e = dict(os.environ)
    for k in ENV_KEYS:
        e.pop(k, None)
    e.update(env)
    if track:
        e["PSMC_VITERBI"] = str(track)
    r = subprocess.run([exe] + args, cwd=CLI, capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stderr[-800:]
    return r.stdout, r.stderr, open(track).read() if track and os.path.exists(track) else None


def parse(text):
    """[(name, L, score text, [(start, end, k, t_k)])]; asserts the layout: a VS line per sequence, then its runs, which tile 1 .. L
    without gaps and change state at every boundary"""
    segs = []
    for line in text.splitlines():
        f = line.split("\t")
        if f[0] == "VS":
            assert len(f) == 4 and len(f[3].split(".")[1]) == 6, line
            segs.append((f[1], int(f[2]), f[3], []))
        else:
            assert f[0] == "VC" and len(f) == 6 and segs and f[1] == segs[-1][0], line
            segs[-1][3].append((int(f[2]), int(f[3]), int(f[4]), float(f[5])))
    for name, L, _, runs in segs:
        assert runs and runs[0][0] == 1 and runs[-1][1] == L, name
        for (s0, e0, k0, _), (s1, e1, k1, _) in zip(runs, runs[1:]):
            assert s1 == e0 + 1 and k1 != k0 and s0 <= e0, (name, s0, e0, s1)
    return segs


def read_input(path):
    """[(name, symbols uint8)] of a .psmcfa file as psmc reads it (cli.c:103-138): a called base -> 0, an IUPAC het -> 1, anything else -> 2"""
    sym = {c: 0 for c in "TACGtacg0"}
    sym.update({c: 1 for c in "KMRSWYkmrswy1"})
    out = []
    with open(os.path.join(CLI, path)) as fh:
        for line in fh:
            if line.startswith(">"):
                out.append([line[1:].split()[0], []])
            elif out:
                out[-1][1].append(line.strip())
    return [(nm, np.array([sym.get(c, 2) for c in "".join(rows)], dtype=np.uint8)) for nm, rows in out]


def last_pa(stdout):
    line = [l for l in stdout.splitlines() if l.startswith("PA\t")][-1]
    f = line[3:].split()
    return f[0], [float(x) for x in f[1:]]


def model_of(pattern, params):
    """(a, e, a0, t_k = avg_t[k] * theta) through the host library"""
    from psmc_amd import hostlib
    a, e, a0 = hostlib.hmm_params(pattern, params)
    lib = hostlib.load()
    pat = hostlib._Pattern()
    assert lib.psmc_pattern_parse(pattern.encode(), C.byref(pat)) == 0
    m = lib.psmc_model_new(C.byref(pat), pattern.encode(), 0.1, 0)
    for i, x in enumerate(params):
        m.contents.params[i] = float(x)
    lib.psmc_model_update(m)
    avg = np.zeros(pat.n_states)
    lib.psmc_model_avg_t.argtypes = [C.POINTER(hostlib._Model), C.POINTER(C.c_double)]
    lib.psmc_model_avg_t(m, avg.ctypes.data_as(C.POINTER(C.c_double)))
    lib.psmc_model_free(m)
    lib.psmc_pattern_free(C.byref(pat))
    return a, e, a0, avg * params[0]


def path_score(tables, seq, path):
    """log probability of one given path (a plain sum: what the gradient below needs, not the recursion's bits)"""
    la, le, l0 = tables
    return float(l0[path[0]] + le[seq, path].sum() + la[path[1:], path[:-1]].sum())


def check_against_restatement(stdout, text, fa):
    """runs and states exactly; t_k and the score within the bounds of the module's docstring.  Returns the number of runs."""
    pattern, params = last_pa(stdout)
    a, e, a0, tk = model_of(pattern, params)
    tables = vm.log_tables(a, e, a0)
    segs = parse(text)
    data = read_input(fa)
    assert [(nm, L) for nm, L, _, _ in segs] == [(nm, len(s)) for nm, s in data]
    paths = []
    for (name, L, score, runs), (_, seq) in zip(segs, data):
        path, want = vm.viterbi(tables, seq)
        assert [(s + 1, t + 1, k) for s, t, k in vm.runs(path)] == [r[:3] for r in runs], name
        for _, _, k, t in runs:
            assert abs(t - tk[k]) <= 1e-6 + 1e-7, (name, k, t, tk[k])
        paths.append((path, want))
    # d score / d parameter along the path, by central differences on the model
    h = 1e-6
    grad = np.zeros((len(params), len(segs)))
    for i in range(len(params)):
        side = []
        for sgn in (1.0, -1.0):
            moved = list(params)
            moved[i] += sgn * h
            am, em, a0m, _ = model_of(pattern, moved)
            tb = vm.log_tables(am, em, a0m)
            side.append([path_score(tb, seq, path) for (path, _), (_, seq) in zip(paths, data)])
        grad[i] = (np.array(side[0]) - np.array(side[1])) / (2 * h)
    for j, ((name, L, score, runs), (path, want)) in enumerate(zip(segs, paths)):
        tol = 5e-7 + 1.5 * 5e-10 * np.abs(grad[:, j]).sum()
        print("%s: score %s, restatement %.9f, bound %.3e" % (name, score, want, tol))
        assert abs(float(score) - want) <= tol, (name, score, want, tol)
        assert tol <= 1e-4  # the bound itself stays a statement about the sixth decimal's neighbourhood
    return sum(len(r) for _, _, _, r in segs)


# ------------------------------------------------------------------ CPU: the oracle-backed binary, the host's own recursion
@pytest.mark.parametrize("name,fa", [("small_decode_d", "small.psmcfa"), ("t10k_n64_N3", "t10k.psmcfa")], ids=["23", "64"])
def test_viterbi_file_beside_the_golden_output(oracle_psmc, tmp_path, name, fa):
    out, err, text = run(oracle_psmc, args_of(name), tmp_path / "v.txt")
    assert out == golden_text(name)                       # the stream does not change
    assert text is not None
    n_runs = check_against_restatement(out, text, fa)
    if name == "small_decode_d":
        assert n_runs > 3                                 # more runs than sequences: a path that moves (t10k's stays in one state)
        # t_k is the text of the TC line's middle column
        tc = {int(l.split("\t")[1]): l.split("\t")[3] for l in out.splitlines() if l.startswith("TC\t")}
        for line in text.splitlines():
            f = line.split("\t")
            if f[0] == "VC":
                assert f[5] == tc[int(f[4])], line
    out2, err2, none = run(oracle_psmc, args_of(name), None)  # without the variable: no file, the same stream
    assert none is None and out2 == out


# ------------------------------------------------------------------ GPU: the product binary
EXACT_CASES = {23: args_of("small_decode_d"), 64: ["-N1", "-t15", "-r5", "-p", "4+25*2+4+6", "small.psmcfa"],
               128: args_of("small_n128_N2"), 200: ["-N1", "-p", "100*2", "small.psmcfa"]}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(EXACT_CASES), ids=[str(k) for k in EXACT_CASES])
def test_viterbi_exact_mode_writes_the_oracle_bytes(oracle_psmc, psmc, tmp_path, case):
    args = EXACT_CASES[case]
    o_out, _, o_text = run(oracle_psmc, args, tmp_path / "o.txt")
    g_out, _, g_text = run(psmc, args, tmp_path / "g.txt")
    assert g_out == o_out
    assert g_text is not None and g_text == o_text
    assert [(nm, L) for nm, L, _, _ in parse(g_text)] == input_segments("small.psmcfa")


@pytest.mark.gpu
def test_viterbi_two_shards_write_the_oracle_bytes(oracle_psmc, psmc, tmp_path):
    args = EXACT_CASES[23]
    o_out, _, o_text = run(oracle_psmc, args, tmp_path / "o.txt")
    g_out, _, g_text = run(psmc, args, tmp_path / "g.txt", PSMC_HIP_DEVICES="0,0")
    assert g_out == o_out and g_text == o_text


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["4+5*3+4", "4+25*2+4+6"], ids=["23", "64"])
def test_viterbi_fast_mode(psmc, tmp_path, pattern):
    """the stream is what it is without the variable; the file parses, tiles every sequence, and its runs and scores are the
    restatement's on that run's final parameters"""
    args = ["-N2", "-p", pattern, "small.psmcfa"]
    out0, err0, _ = run(psmc, args, None, PSMC_HIP_MODE="fast")
    out, err, text = run(psmc, args, tmp_path / "f.txt", PSMC_HIP_MODE="fast")
    assert "using PSMC_HIP_MODE=exact" not in err
    assert out == out0 and text is not None
    check_against_restatement(out, text, "small.psmcfa")
