"""PSMC_TMRCA=<path>: a decoding run of `psmc` (-d, -D, -s or -c) also writes the local TMRCA track -- per sequence a line
`TS name L` and L lines `TM bin mean sd`, the posterior mean and standard deviation of the coalescence time of every bin in the
units of the TC lines (w0[k] = the middle column of TC line k, w1 = w0^2; psmc_amd/host/run.c).  The -o / stdout stream stays byte
for byte what it is without the variable.

On the CPU the E-step backend is the oracle (tests/host_oracle_main.c, built as tests/test_host_cli.py builds it), which has no
post_mean: the two sums are formed on the host, in state order over f * b * s.  On the GPU `psmc` forms them on the device
(psmc_hip_post_mean): exact mode must write the oracle-backed binary's bytes; the fast sources are held to the header's posterior
tolerance: every value of a TM line, mean and sd alike, within 1e-9 sum_k w[k] + 1e-6 of the exact run's (1e-6: both files print six
decimals).  A second test main, tests/host_oracle_post_main.c, gives the oracle backend a `posterior` member and no `post_mean`: the
host's middle branch (sums over the backend's posterior rows) must write the bytes of the other two.

The margin of the -D cross-check, |mean - sum_k DF[k] TC[k]| <= 5e-5 sum_k w0[k] + 1e-5, is derived, not measured: a DF column is
printed with %.4f (off by at most 5e-5 each, so 5e-5 sum_k w0[k] in the sum), a TC column with %lf (off by at most 5e-7, times
posteriors that sum to one) and the mean with %.6f (5e-7): the last two together stay below 1e-5."""
import atexit
import gzip
import os
import shutil
import subprocess
import tempfile
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "psmc_amd", "host")
CLI = os.path.join(ROOT, "tests", "golden", "cli")
BUILD = tempfile.mkdtemp(prefix="psmc_test_tmrca_")
atexit.register(shutil.rmtree, BUILD, True)
IGNORED = "PSMC_TMRCA is ignored"


@pytest.fixture(scope="module")
def oracle_psmc():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "all"], check=True)
    subprocess.run(["make", "-s", "-C", HOST, "libpsmc_host.so"], check=True)
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "psmc_oracle_backend")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "host_oracle_main.c"),
                    "-I" + HOST, "-I" + os.path.join(ROOT, "oracle"), "-L" + HOST, "-lpsmc_host",
                    "-L" + os.path.join(ROOT, "oracle"), "-lpsmc_oracle",
                    "-Wl,-rpath," + HOST, "-Wl,-rpath," + os.path.join(ROOT, "oracle"), "-lz", "-lm"], check=True)
    return exe


@pytest.fixture(scope="module")
def psmc():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    return os.path.join(HOST, "psmc")


def run(exe, args, track, **env):
    """(stdout, stderr, the track's text or None when no file was written)"""
    e = dict(os.environ)
    for k in ("PSMC_HIP_MODE", "PSMC_HIP_DECODE", "PSMC_HIP_WIDE", "PSMC_HIP_OPTIONS", "PSMC_HIP_DEVICES", "PSMC_TMRCA"):
        e.pop(k, None)
    e.update(env)
    if track:
        e["PSMC_TMRCA"] = str(track)
    r = subprocess.run([exe] + args, cwd=CLI, capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stderr[-800:]
    return r.stdout, r.stderr, open(track).read() if track and os.path.exists(track) else None


def args_of(name):
    return open(os.path.join(CLI, name + ".args")).read().split()


def golden_text(name):
    p = os.path.join(CLI, name + ".psmc")
    return open(p).read() if os.path.exists(p) else gzip.open(p + ".gz", "rt").read()


def input_segments(path):
    """(name, L) of every sequence of a .psmcfa file"""
    out = []
    for line in open(os.path.join(CLI, path)):
        if line.startswith(">"):
            out.append([line[1:].split()[0], 0])
        elif out:
            out[-1][1] += len(line.strip())
    return [tuple(s) for s in out]


def parse_track(text):
    """[(name, L, [(mean, sd)] * L)]; asserts the layout: one TS line per segment and its L TM lines, bins 1 .. L"""
    segs = []
    for line in text.splitlines():
        f = line.split("\t")
        if f[0] == "TS":
            assert len(f) == 3
            segs.append((f[1], int(f[2]), []))
        else:
            assert f[0] == "TM" and len(f) == 4 and segs, line
            assert int(f[1]) == len(segs[-1][2]) + 1, line
            assert all(len(x.split(".")[1]) == 6 for x in f[2:]), line   # %.6f
            segs[-1][2].append((float(f[2]), float(f[3])))
    for name, L, rows in segs:
        assert len(rows) == L, name
    return segs


def tc_times(stdout):
    return [float(l.split("\t")[3]) for l in stdout.splitlines() if l.startswith("TC\t")]   # TC k t_k avg_t_k t_{k+1}


# ------------------------------------------------------------------ CPU: the oracle-backed binary
@pytest.mark.parametrize("name", ["small_decode_d", "small_decode_D"])
def test_tmrca_track_beside_the_golden_output(oracle_psmc, tmp_path, name):
    out, err, track = run(oracle_psmc, args_of(name), tmp_path / "t.txt")
    assert out == golden_text(name)                      # the stream does not change
    assert IGNORED not in err and track is not None
    segs = parse_track(track)
    assert [(nm, L) for nm, L, _ in segs] == input_segments("small.psmcfa")
    w0 = tc_times(out)
    assert len(w0) == 23
    for nm, L, rows in segs:
        for u, (mean, sd) in enumerate(rows):
            assert min(w0) <= mean <= max(w0) and 0.0 <= sd <= max(w0), (nm, u + 1, mean, sd)
    if name == "small_decode_D":                          # the rows of -D give the same means
        df = [l.split("\t") for l in out.splitlines() if l.startswith("DF\t")]
        assert len(df) == sum(L for _, L, _ in segs)
        margin = 5e-5 * sum(w0) + 1e-5
        i = 0
        for nm, L, rows in segs:
            for u, (mean, _) in enumerate(rows):
                f = df[i]; i += 1
                assert int(f[1]) == u + 1 and len(f) == 3 + len(w0)
                want = sum(float(p) * t for p, t in zip(f[3:], w0))
                assert abs(mean - want) <= margin, (nm, u + 1, mean, want, margin)


def test_tmrca_needs_a_decoding_run(oracle_psmc, tmp_path):
    out, err, track = run(oracle_psmc, args_of("small_T"), tmp_path / "t.txt")
    assert track is None and err.count(IGNORED) == 1
    assert out == golden_text("small_T")
    out, err, _ = run(oracle_psmc, args_of("small_decode_d"), None)   # and without the variable: no word about it
    assert IGNORED not in err and out == golden_text("small_decode_d")


@pytest.mark.parametrize("name", ["small_decode_d", "small_decode_D"])
def test_tmrca_from_a_backend_with_posterior_rows_only(oracle_psmc, tmp_path, name):
    """a backend that has `posterior` and no `post_mean`: the host sums over its rows, in the same order -- the same bytes"""
    exe = os.path.join(BUILD, "psmc_oracle_posterior_backend")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "host_oracle_post_main.c"),
                    "-I" + HOST, "-I" + os.path.join(ROOT, "oracle"), "-I" + os.path.join(ROOT, "tests"), "-L" + HOST, "-lpsmc_host",
                    "-L" + os.path.join(ROOT, "oracle"), "-lpsmc_oracle",
                    "-Wl,-rpath," + HOST, "-Wl,-rpath," + os.path.join(ROOT, "oracle"), "-lz", "-lm"], check=True)
    out, err, track = run(exe, args_of(name), tmp_path / "p.txt")
    assert out == golden_text(name)      # (-D prints this backend's rows: they are the reference's)
    assert track is not None and track == run(oracle_psmc, args_of(name), tmp_path / "o.txt")[2]


@pytest.mark.parametrize("name", ["small_decode_d", "small_decode_s"])
def test_tmrca_host_path_asan_ubsan_clean(oracle_psmc, tmp_path, name):
    """the host's own sums and the writer under AddressSanitizer + UBSan (the stand-alone build of tests/test_host_sanitizers.py):
    no report, and the plain build's bytes"""
    from test_host_sanitizers import build
    exe = build("psmc_oracle_asan_tmrca", "host_oracle_main.c", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    out, err, track = run(exe, args_of(name), tmp_path / "a.txt", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
                          UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err and "LeakSanitizer" not in err, err[-3000:]
    assert out == golden_text(name)
    assert track == run(oracle_psmc, args_of(name), tmp_path / "p.txt")[2] and track.count("TS\t") == len(input_segments("small.psmcfa"))


# ------------------------------------------------------------------ GPU: the product binary
EXACT_CASES = {23: args_of("small_decode_d"), "23-D": args_of("small_decode_D"), "23-s": args_of("small_decode_s"),
               64: ["-N1", "-d", "-t15", "-r5", "-p", "4+25*2+4+6", "small.psmcfa"], 128: args_of("small_n128_d"),
               149: args_of("small_n149_d"), 200: ["-N1", "-d", "-p", "100*2", "small.psmcfa"]}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(EXACT_CASES), ids=[str(k) for k in EXACT_CASES])
def test_tmrca_exact_mode_writes_the_oracle_bytes(oracle_psmc, psmc, tmp_path, case):
    """psmc_hip_post_mean on the exact tables is bit for bit the host's state-order sum: the same file, at every kernel width"""
    args = EXACT_CASES[case]
    o_out, _, o_track = run(oracle_psmc, args, tmp_path / "o.txt")
    g_out, _, g_track = run(psmc, args, tmp_path / "g.txt")
    assert g_out == o_out
    assert g_track is not None and g_track == o_track
    assert [(nm, L) for nm, L, _ in parse_track(g_track)] == input_segments("small.psmcfa")


def close_tracks(got, want, w0):
    tol = 1e-9 * sum(w0) + 1e-6
    a, b = parse_track(got), parse_track(want)
    assert [(nm, L) for nm, L, _ in a] == [(nm, L) for nm, L, _ in b]
    worst, worst_sd = 0.0, 0.0
    for (nm, L, ra), (_, _, rb) in zip(a, b):
        for u in range(L):
            worst = max(worst, abs(ra[u][0] - rb[u][0])); worst_sd = max(worst_sd, abs(ra[u][1] - rb[u][1]))
            assert abs(ra[u][0] - rb[u][0]) <= tol and abs(ra[u][1] - rb[u][1]) <= tol, (nm, u + 1, ra[u], rb[u], tol)   # every value
    print("TMRCA track against the exact run: mean worst %.3e, sd worst %.3e, bound %.3e" % (worst, worst_sd, tol))
    return worst, worst_sd


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["4+5*3+4", "4+25*2+4+6", "64*2"], ids=["23", "64", "128"])
def test_tmrca_fast_mode_close_to_exact(psmc, tmp_path, pattern):
    """-N0 decodes the starting parameters, so the fast and the exact run decode the same model"""
    args = ["-N0", "-d", "-p", pattern, "small.psmcfa"]
    x_out, _, x_track = run(psmc, args, tmp_path / "x.txt")
    f_out, err, f_track = run(psmc, args, tmp_path / "f.txt", PSMC_HIP_MODE="fast", PSMC_HIP_DECODE="fast")
    assert "using PSMC_HIP_MODE=exact" not in err
    close_tracks(f_track, x_track, tc_times(x_out))


@pytest.mark.gpu
def test_tmrca_wide_fast_close_to_exact_and_checkpoints_alike(psmc, tmp_path):
    args = ["-N0", "-d", "-p", "100*2", "small.psmcfa"]
    wide = dict(PSMC_HIP_MODE="fast", PSMC_HIP_DECODE="fast", PSMC_HIP_WIDE="fast")
    x_out, _, x_track = run(psmc, args, tmp_path / "x.txt")
    f_out, err, f_track = run(psmc, args, tmp_path / "f.txt", **wide)
    assert "using PSMC_HIP_MODE=exact" not in err
    close_tracks(f_track, x_track, tc_times(x_out))
    c_out, err, c_track = run(psmc, args, tmp_path / "c.txt", PSMC_HIP_OPTIONS="wide_ckpt=1,wide_decode_ckpt=1", **wide)
    assert "checkpoints" in err
    assert c_track == f_track and c_out == f_out
