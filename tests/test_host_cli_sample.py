"""PSMC_SAMPLE=<path>: after the EM rounds `psmc` writes state paths drawn from the posterior under the final parameters (forward
filtering, backward sampling; the definition include/psmc_hip.h pins) -- per sample j and sequence a line `PS j name L` and one
`PC j name start end k t_k` per run of equal states (fields as on the VC lines of PSMC_VITERBI; psmc_amd/host/run.c).
PSMC_SAMPLE_N=<J> sets the number of samples (default 1), PSMC_SAMPLE_SEED=<s> the seed (default 1); the stream id of a sequence is
its index in the input.  It needs no decoding option, and the -o / stdout stream stays byte for byte what it is without the variable.

On the CPU the E-step backend is the oracle (tests/host_oracle_main.c), which has no `sample_paths` member: the host's own plain C
statement (psmc_sample_host) runs.  On the GPU `psmc` calls psmc_hip_sample_paths: it must write the oracle-backed binary's bytes in
exact mode, one context or two shards.

What the file is compared with: the numpy restatement (tests/sample_model.py) under the parameters of the last RD block, rebuilt
through psmc_amd.hostlib from the PA line as tests/test_host_cli_viterbi.py does.  Runs and states are compared exactly, t_k within
1e-6 (six printed decimals) + 1e-7."""
import os
import subprocess
import numpy as np
import pytest

import sample_model as sm
from test_host_cli_tmrca import BUILD, CLI, HOST, ROOT, args_of, input_segments, oracle_psmc, psmc  # noqa: F401 (fixtures)
from test_host_cli_viterbi import last_pa, model_of, read_input

ENV_KEYS = ("PSMC_HIP_MODE", "PSMC_HIP_DECODE", "PSMC_HIP_WIDE", "PSMC_HIP_OPTIONS", "PSMC_HIP_DEVICES", "PSMC_TMRCA", "PSMC_VITERBI",
            "PSMC_SAMPLE", "PSMC_SAMPLE_N", "PSMC_SAMPLE_SEED")
ARGS = ["-N2", "-p", "4+5*3+4", "small.psmcfa"]


def run(exe, args, track, status=0, **env):
    """(stdout, stderr, the file's text or None when none was written)"""
    e = dict(os.environ)
    for k in ENV_KEYS:
        e.pop(k, None)
    e.update(env)
    if track:
        e["PSMC_SAMPLE"] = str(track)
    r = subprocess.run([exe] + args, cwd=CLI, capture_output=True, text=True, env=e)
    assert r.returncode == status, (r.returncode, r.stderr[-800:])
    return r.stdout, r.stderr, open(track).read() if track and os.path.exists(track) else None


def parse(text):
    """[[(name, L, [(start, end, k, t_k)])] per sample]; asserts the layout: samples 0, 1, .. in order, per sample a PS line per
    sequence followed by its runs, which tile 1 .. L without gaps and change state at every boundary"""
    samples = []
    for line in text.splitlines():
        f = line.split("\t")
        if f[0] == "PS":
            assert len(f) == 4, line
            j = int(f[1])
            assert j in (len(samples) - 1, len(samples)), line
            if j == len(samples):
                samples.append([])
            samples[j].append((f[2], int(f[3]), []))
        else:
            assert f[0] == "PC" and len(f) == 7 and samples and int(f[1]) == len(samples) - 1 and f[2] == samples[-1][-1][0], line
            assert len(f[6].split(".")[1]) == 6, line
            samples[-1][-1][2].append((int(f[3]), int(f[4]), int(f[5]), float(f[6])))
    for segs in samples:
        for name, L, runs in segs:
            assert runs and runs[0][0] == 1 and runs[-1][1] == L, name
            for (s0, e0, k0, _), (s1, e1, k1, _) in zip(runs, runs[1:]):
                assert s1 == e0 + 1 and k1 != k0 and s0 <= e0, (name, s0, e0, s1)
    return samples


def check_against_restatement(stdout, text, fa, seed, n_samp):
    """every run of every sample is the restatement's under the run's final parameters.  Returns the number of runs."""
    pattern, params = last_pa(stdout)
    a, e, a0, tk = model_of(pattern, params)
    samples = parse(text)
    data = read_input(fa)
    assert len(samples) == n_samp
    want = sm.sample_segments(a, e, a0, [s for _, s in data], seed, n_samp)
    n_runs = 0
    for j, segs in enumerate(samples):
        assert [(nm, L) for nm, L, _ in segs] == [(nm, len(s)) for nm, s in data]
        for i, (name, L, runs) in enumerate(segs):
            assert [(s + 1, t + 1, k) for s, t, k in sm.runs(want[j][i])] == [r[:3] for r in runs], (j, name)
            for _, _, k, t in runs:
                assert abs(t - tk[k]) <= 1e-6 + 1e-7, (name, k, t, tk[k])
            n_runs += len(runs)
    return n_runs


# ------------------------------------------------------------------ CPU: the oracle-backed binary, the host's own sampler
def test_sample_file_beside_an_unchanged_stream(oracle_psmc, tmp_path):
    out0, _, none = run(oracle_psmc, ARGS, None)
    out, _, text = run(oracle_psmc, ARGS, tmp_path / "s.txt")
    assert none is None and out == out0                   # the stream does not change
    assert text is not None
    n_seq = len(input_segments("small.psmcfa"))
    n_runs = check_against_restatement(out, text, "small.psmcfa", 1, 1)
    assert n_runs > 3 * n_seq                             # paths that move
    # t_k is the text of the TC line's middle column when the run decodes as well
    out_d, _, text_d = run(oracle_psmc, ["-d"] + ARGS, tmp_path / "d.txt")
    assert text_d == text
    tc = {int(l.split("\t")[1]): l.split("\t")[3] for l in out_d.splitlines() if l.startswith("TC\t")}
    assert all(l.split("\t")[6] == tc[int(l.split("\t")[5])] for l in text.splitlines() if l.startswith("PC\t"))


def test_sample_n_and_seed(oracle_psmc, tmp_path):
    out, _, one = run(oracle_psmc, ARGS, tmp_path / "1.txt")
    out3, _, three = run(oracle_psmc, ARGS, tmp_path / "3.txt", PSMC_SAMPLE_N="3")
    assert out3 == out
    n_seq = len(input_segments("small.psmcfa"))
    s1, s3 = parse(one), parse(three)
    assert len(s1) == 1 and len(s3) == 3 and all(len(s) == n_seq for s in s3)   # three PS blocks per sequence
    assert sum(l.startswith("PS\t") for l in three.splitlines()) == 3 * n_seq
    assert s3[0] == s1[0] and s3[1] != s3[0] and s3[2] != s3[1]
    assert three.startswith(one)
    check_against_restatement(out3, three, "small.psmcfa", 1, 3)
    _, _, other = run(oracle_psmc, ARGS, tmp_path / "o.txt", PSMC_SAMPLE_SEED="18446744073709551615")
    assert parse(other)[0] != s1[0]
    check_against_restatement(out, other, "small.psmcfa", 2 ** 64 - 1, 1)


@pytest.mark.parametrize("bad", ["0", "-2", "x", "2x", "1.5"])
def test_bad_sample_n_is_status_2(oracle_psmc, tmp_path, bad):
    out, err, text = run(oracle_psmc, ARGS, tmp_path / "b.txt", status=2, PSMC_SAMPLE_N=bad)
    assert "PSMC_SAMPLE_N" in err and text is None and out == ""


def test_usage_names_the_variables(oracle_psmc):
    r = subprocess.run([oracle_psmc], cwd=CLI, capture_output=True, text=True)
    assert all(k in r.stderr for k in ("PSMC_SAMPLE=<path>", "PSMC_SAMPLE_N=<J>", "PSMC_SAMPLE_SEED=<s>"))


# ------------------------------------------------------------------ GPU: the product binary
EXACT_CASES = {23: ARGS, 64: ["-N1", "-t15", "-r5", "-p", "4+25*2+4+6", "small.psmcfa"], 200: ["-N1", "-p", "100*2", "small.psmcfa"]}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(EXACT_CASES), ids=[str(k) for k in EXACT_CASES])
def test_sample_exact_mode_writes_the_oracle_bytes(oracle_psmc, psmc, tmp_path, case):
    args = EXACT_CASES[case]
    o_out, _, o_text = run(oracle_psmc, args, tmp_path / "o.txt", PSMC_SAMPLE_N="2", PSMC_SAMPLE_SEED="7")
    g_out, _, g_text = run(psmc, args, tmp_path / "g.txt", PSMC_SAMPLE_N="2", PSMC_SAMPLE_SEED="7")
    assert g_out == o_out
    assert g_text is not None and g_text == o_text
    assert [(nm, L) for nm, L, _ in parse(g_text)[1]] == input_segments("small.psmcfa")


@pytest.mark.gpu
def test_sample_two_shards_write_the_oracle_bytes(oracle_psmc, psmc, tmp_path):
    o_out, _, o_text = run(oracle_psmc, ARGS, tmp_path / "o.txt", PSMC_SAMPLE_N="3")
    g_out, _, g_text = run(psmc, ARGS, tmp_path / "g.txt", PSMC_SAMPLE_N="3", PSMC_HIP_DEVICES="0,0")
    assert g_out == o_out and g_text == o_text


@pytest.mark.gpu
def test_sample_fast_mode(psmc, tmp_path):
    """the stream is what it is without the variable; the file is the restatement's on that run's final parameters"""
    out0, _, _ = run(psmc, ARGS, None, PSMC_HIP_MODE="fast")
    out, err, text = run(psmc, ARGS, tmp_path / "f.txt", PSMC_HIP_MODE="fast", PSMC_SAMPLE_N="2")
    assert out == out0 and text is not None
    check_against_restatement(out, text, "small.psmcfa", 1, 2)


@pytest.mark.gpu
def test_bad_sample_n_is_status_2_on_the_product_binary(psmc, tmp_path):
    out, err, text = run(psmc, ARGS, tmp_path / "b.txt", status=2, PSMC_SAMPLE_N="none")
    assert "PSMC_SAMPLE_N" in err and text is None
