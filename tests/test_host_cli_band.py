"""PSMC_TMRCA_BAND=<path>: a decoding run of `psmc` (-d, -D, -s or -c) also writes the quantile band of the local TMRCA -- per
sequence a line `QS name L q_1 .. q_m` and L lines `QM bin k_1 .. k_m t_1 .. t_m`: k_j the 0-based state at the posterior quantile
q_j of the bin (include/psmc_hip.h, psmc_hip_post_quantile), t_j = the time a DC line prints for that state, `%.6f`.
PSMC_TMRCA_Q=<q_1,..,q_m> [0.025,0.5,0.975] takes 1 to 4 values in [0, 1]; anything else ends the run with status 2 before any
work.  The -o / stdout stream and the PSMC_TMRCA file stay byte for byte what they are without the variable.

On the CPU the E-step backend is the oracle (tests/host_oracle_main.c), which has neither post_quantile nor posterior: the host
counts over f * b * s.  tests/host_oracle_quant_main.c adds a `posterior` member: the host's middle branch must write the same
bytes.  On the GPU `psmc` counts on the device: exact mode must write the oracle-backed binary's bytes; the fast sources are held
to (Q3) of the header against the exact run's -D rows.

Margins, derived and not measured.  A DF column is printed with %.4f, off by at most 5e-5, so the cdf of a printed row of n states
is off by at most n * 5e-5 at every state (DMARG).
  * the -D cross-check on one run: where every printed cdf value is MORE than DMARG away from q, the count #{k : P_k < q} over the
    printed cdf P is the count over the true one (the total of a row is 1 within a few ulp: far inside the gap), so k_j must
    equal it; elsewhere nothing is asserted.  The share of (bin, q) pairs that are checked is printed and must be most of them.
  * (Q3) against the exact run's printed rows: state i is acceptable when (i == 0 or P_{i-1} < q + d) and (i == n-1 or
    P_i >= q - d) with d = 1e-9 n + DMARG: the header's d for the true rows, widened by what the printing can move P."""
import os
import subprocess
import pytest
from test_host_cli_tmrca import BUILD, CLI, HOST, ROOT, args_of, golden_text, input_segments, tc_times, oracle_psmc, psmc  # noqa: F401 (fixtures)

IGNORED = "PSMC_TMRCA_BAND is ignored"
ENV_KEYS = ("PSMC_HIP_MODE", "PSMC_HIP_DECODE", "PSMC_HIP_WIDE", "PSMC_HIP_OPTIONS", "PSMC_HIP_DEVICES", "PSMC_TMRCA", "PSMC_TMRCA_BAND", "PSMC_TMRCA_Q")
Q_DEFAULT = (0.025, 0.5, 0.975)


def run(exe, args, band=None, track=None, status=0, **env):
    """(stdout, stderr, the band file's text or None, the PSMC_TMRCA file's text or None)"""
    e = dict(os.environ)
    for k in ENV_KEYS:
        e.pop(k, None)
    e.update(env)
    if band:
        e["PSMC_TMRCA_BAND"] = str(band)
    if track:
        e["PSMC_TMRCA"] = str(track)
    r = subprocess.run([exe] + args, cwd=CLI, capture_output=True, text=True, env=e)
    assert r.returncode == status, (r.returncode, r.stderr[-800:])
    text = lambda p: open(p).read() if p and os.path.exists(p) else None
    return r.stdout, r.stderr, text(band), text(track)


def parse_band(text, w0):
    """[(name, L, q, [k_1 .. k_m] * L)]; asserts the layout: one QS line per segment and its L QM lines, bins 1 .. L, every
    state within 0 .. n-1 and every time the %.6f print of the TC line's time of that state"""
    segs = []
    for line in text.splitlines():
        f = line.split("\t")
        if f[0] == "QS":
            assert len(f) >= 4, line
            segs.append((f[1], int(f[2]), tuple(float(x) for x in f[3:]), []))
        else:
            assert f[0] == "QM" and segs, line
            m = len(segs[-1][2])
            assert len(f) == 2 + 2 * m, line
            assert int(f[1]) == len(segs[-1][3]) + 1, line
            ks = [int(x) for x in f[2:2 + m]]
            assert all(0 <= k < len(w0) for k in ks), line
            for k, t in zip(ks, f[2 + m:]):
                assert len(t.split(".")[1]) == 6 and abs(float(t) - w0[k]) <= 1e-6, line   # %.6f of a time TC prints with %lf
            segs[-1][3].append(ks)
    for name, L, q, rows in segs:
        assert len(rows) == L, name
    return segs


def df_cdfs(stdout, n):
    """the printed posterior rows of a -D run as running sums, one list per bin, in output order"""
    out = []
    for l in stdout.splitlines():
        if l.startswith("DF\t"):
            f = l.split("\t")
            assert len(f) == 3 + n
            c, row = 0.0, []
            for p in f[3:]:
                c += float(p)
                row.append(c)
            out.append(row)
    return out


def acceptable(i, P, q, d):
    n = len(P)
    return (i == 0 or P[i - 1] < q + d) and (i == n - 1 or P[i] >= q - d)


# ------------------------------------------------------------------ CPU: the oracle-backed binary
@pytest.mark.parametrize("name", ["small_decode_d", "small_decode_D"])
def test_band_beside_the_golden_output(oracle_psmc, tmp_path, name):
    out, err, band, _ = run(oracle_psmc, args_of(name), tmp_path / "b.txt")
    assert out == golden_text(name)                      # the stream does not change
    assert IGNORED not in err and band is not None
    w0 = tc_times(out)
    n = len(w0)
    assert n == 23
    segs = parse_band(band, w0)
    assert [(nm, L) for nm, L, _, _ in segs] == input_segments("small.psmcfa")
    assert all(q == Q_DEFAULT for _, _, q, _ in segs)
    assert band.splitlines()[0] == "QS\ta\t%d\t0.025\t0.5\t0.975" % segs[0][1]
    for _, _, _, rows in segs:
        assert all(ks[0] <= ks[1] <= ks[2] for ks in rows)   # q ascending, and the running sums of one row are shared
    # with PSMC_TMRCA as well: both files, each what it is alone
    out2, _, band2, track2 = run(oracle_psmc, args_of(name), tmp_path / "b2.txt", tmp_path / "t2.txt")
    _, _, _, track = run(oracle_psmc, args_of(name), None, tmp_path / "t.txt")
    assert out2 == out and band2 == band and track2 is not None and track2 == track
    if name == "small_decode_D":                          # the rows of -D give the same states away from the printing's reach
        cdfs = df_cdfs(out, n)
        assert len(cdfs) == sum(L for _, L, _, _ in segs)
        dmarg = n * 5e-5
        i, checked, total = 0, 0, 0
        for nm, L, q, rows in segs:
            for u, ks in enumerate(rows):
                P = cdfs[i]; i += 1
                for qj, kj in zip(q, ks):
                    total += 1
                    if min(abs(p - qj) for p in P) > dmarg:
                        checked += 1
                        assert kj == min(n - 1, sum(p < qj for p in P)), (nm, u + 1, qj, kj)
        print("-D cross-check: %d of %d (bin, q) pairs lie outside the printing margin and were compared" % (checked, total))
        assert 2 * checked > total


def test_band_custom_quantiles(oracle_psmc, tmp_path):
    """PSMC_TMRCA_Q: one to four columns; q = 0 gives state 0; a column does not depend on the others"""
    args = args_of("small_decode_d")
    out, _, b4, _ = run(oracle_psmc, args, tmp_path / "b4.txt", PSMC_TMRCA_Q="0,0.5,0.25,1")
    w0 = tc_times(out)
    s4 = parse_band(b4, w0)
    assert all(q == (0.0, 0.5, 0.25, 1.0) for _, _, q, _ in s4)
    assert all(ks[0] == 0 and ks[2] <= ks[1] <= ks[3] for _, _, _, rows in s4 for ks in rows)
    _, _, b1, _ = run(oracle_psmc, args, tmp_path / "b1.txt", PSMC_TMRCA_Q="0.5")
    s1 = parse_band(b1, w0)
    assert [[ks[1]] for _, _, _, rows in s4 for ks in rows] == [ks for _, _, _, rows in s1 for ks in rows]
    _, _, b3, _ = run(oracle_psmc, args, tmp_path / "b3.txt")
    assert [ks[1] for _, _, _, rows in parse_band(b3, w0) for ks in rows] == [ks[0] for _, _, _, rows in s1 for ks in rows]   # the default's median


def test_band_needs_a_decoding_run(oracle_psmc, tmp_path):
    out, err, band, _ = run(oracle_psmc, args_of("small_T"), tmp_path / "b.txt")
    assert band is None and err.count(IGNORED) == 1
    assert out == golden_text("small_T")
    out, err, _, _ = run(oracle_psmc, args_of("small_decode_d"))   # and without the variable: no word about it
    assert IGNORED not in err and out == golden_text("small_decode_d")


@pytest.mark.parametrize("bad", ["x", "0.5,", ",0.5", "0.5;0.6", "1.5", "-0.1", "nan", "0.1,0.2,0.3,0.4,0.5", "0.5 0.6"])
def test_band_bad_quantiles_end_the_run_with_status_2(oracle_psmc, tmp_path, bad):
    out, err, band, _ = run(oracle_psmc, args_of("small_decode_d"), tmp_path / "b.txt", status=2, PSMC_TMRCA_Q=bad)
    assert "PSMC_TMRCA_Q" in err and band is None
    assert out == ""                                      # before any work: not even the header


@pytest.mark.parametrize("name", ["small_decode_d", "small_decode_D"])
def test_band_from_a_backend_with_posterior_rows_only(oracle_psmc, tmp_path, name):
    """a backend that has `posterior` and no `post_quantile`: the host counts over its rows, by the same rule -- the same bytes"""
    exe = os.path.join(BUILD, "psmc_oracle_quant_backend")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "host_oracle_quant_main.c"),
                    "-I" + HOST, "-I" + os.path.join(ROOT, "oracle"), "-I" + os.path.join(ROOT, "tests"), "-L" + HOST, "-lpsmc_host",
                    "-L" + os.path.join(ROOT, "oracle"), "-lpsmc_oracle",
                    "-Wl,-rpath," + HOST, "-Wl,-rpath," + os.path.join(ROOT, "oracle"), "-lz", "-lm"], check=True)
    out, err, band, _ = run(exe, args_of(name), tmp_path / "p.txt", PSMC_TMRCA_Q="0,0.025,0.5,1")
    assert out == golden_text(name)      # (-D prints this backend's rows: they are the reference's)
    assert band is not None and band == run(oracle_psmc, args_of(name), tmp_path / "o.txt", PSMC_TMRCA_Q="0,0.025,0.5,1")[2]


@pytest.mark.parametrize("main_c", ["host_oracle_main.c", "host_oracle_quant_main.c"])
def test_band_host_path_asan_ubsan_clean(oracle_psmc, tmp_path, main_c):
    """the host's own counts (over the tables, and over a backend's rows), the parser of PSMC_TMRCA_Q and the writer under
    AddressSanitizer + UBSan (the stand-alone build of tests/test_host_sanitizers.py): no report, and the plain build's bytes"""
    from test_host_sanitizers import build
    exe = build("psmc_asan_band_" + main_c[:-2], main_c, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], ["-I" + os.path.join(ROOT, "tests")])
    san = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    q = "0,0.025,0.5,1"
    out, err, band, _ = run(exe, args_of("small_decode_d"), tmp_path / "a.txt", PSMC_TMRCA_Q=q, **san)
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err and "LeakSanitizer" not in err, err[-3000:]
    assert out == golden_text("small_decode_d")
    assert band == run(oracle_psmc, args_of("small_decode_d"), tmp_path / "p.txt", PSMC_TMRCA_Q=q)[2] and band.count("QS\t") == len(input_segments("small.psmcfa"))
    _, err, _, _ = run(exe, args_of("small_decode_d"), tmp_path / "b.txt", status=2, PSMC_TMRCA_Q="0.1,0.2,0.3,0.4,0.5,", **san)
    assert "PSMC_TMRCA_Q" in err and "ERROR: AddressSanitizer" not in err and "runtime error" not in err and "LeakSanitizer" not in err, err[-3000:]


# ------------------------------------------------------------------ GPU: the product binary
EXACT_CASES = {23: args_of("small_decode_d"), "23-D": args_of("small_decode_D"), "23-s": args_of("small_decode_s"),
               64: ["-N1", "-d", "-t15", "-r5", "-p", "4+25*2+4+6", "small.psmcfa"], 128: args_of("small_n128_d"),
               149: ["-N0", "-d", "-p", "1+74*2", "small.psmcfa"]}   # (-N0: the oracle's E-step at 149 states is what this case costs)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(EXACT_CASES), ids=[str(k) for k in EXACT_CASES])
def test_band_exact_mode_writes_the_oracle_bytes(oracle_psmc, psmc, tmp_path, case):
    """psmc_hip_post_quantile on the exact tables is bit for bit the host's count: the same file, at every kernel width"""
    args = EXACT_CASES[case]
    q = "0,0.025,0.5,1"                                   # both ends pinned
    o_out, _, o_band, _ = run(oracle_psmc, args, tmp_path / "o.txt", PSMC_TMRCA_Q=q)
    g_out, _, g_band, _ = run(psmc, args, tmp_path / "g.txt", PSMC_TMRCA_Q=q)
    assert g_out == o_out
    assert g_band is not None and g_band == o_band
    assert [(nm, L) for nm, L, _, _ in parse_band(g_band, tc_times(g_out))] == input_segments("small.psmcfa")


FAST64 = dict(PSMC_HIP_MODE="fast", PSMC_HIP_DECODE="fast")
WIDE300 = dict(PSMC_HIP_MODE="fast", PSMC_HIP_WIDE="fast-all", PSMC_HIP_DECODE="fast-all")
FAST_RUNS = {"fast64": ("4+25*2+4+6", FAST64), "wide300": ("150*2", WIDE300),
             "wide300-ckpt": ("150*2", dict(WIDE300, PSMC_HIP_OPTIONS="wide_ckpt=1,wide_decode_ckpt=1"))}
_EXACT_D = {}


def exact_rows(psmc, pattern, tmp_path):
    """the exact run's -D rows as cdfs and its band, once per pattern (-N0 decodes the starting parameters: every run decodes one model)"""
    if pattern not in _EXACT_D:
        out, _, band, _ = run(psmc, ["-N0", "-D", "-p", pattern, "small.psmcfa"], tmp_path / "x.txt")
        w0 = tc_times(out)
        _EXACT_D[pattern] = (w0, df_cdfs(out, len(w0)), parse_band(band, w0))
    return _EXACT_D[pattern]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(FAST_RUNS))
def test_band_fast_sources_acceptable_against_the_exact_rows(psmc, tmp_path, case):
    pattern, env = FAST_RUNS[case]
    w0, cdfs, x_segs = exact_rows(psmc, pattern, tmp_path)
    n = len(w0)
    out, err, band, _ = run(psmc, ["-N0", "-d", "-p", pattern, "small.psmcfa"], tmp_path / "f.txt", **env)
    assert "using PSMC_HIP_MODE=exact" not in err
    if "ckpt" in case:
        assert "checkpoints" in err
    segs = parse_band(band, w0)
    assert [(nm, L, q) for nm, L, q, _ in segs] == [(nm, L, q) for nm, L, q, _ in x_segs]
    d = 1e-9 * n + n * 5e-5
    i, differ, total = 0, 0, 0
    for (nm, L, q, rows), (_, _, _, x_rows) in zip(segs, x_segs):
        for u, (ks, xs) in enumerate(zip(rows, x_rows)):
            P = cdfs[i]; i += 1
            for qj, kj, xj in zip(q, ks, xs):
                total += 1; differ += kj != xj
                assert acceptable(kj, P, qj, d), (nm, u + 1, qj, kj, xj)
    print("%s: %d of %d states differ from the exact run's" % (case, differ, total))
    if case == "wide300-ckpt":   # the bits of the full table
        assert band == run(psmc, ["-N0", "-d", "-p", pattern, "small.psmcfa"], tmp_path / "w.txt", **WIDE300)[2]
