"""`psmc` with PSMC_HIP_MODE=fast PSMC_HIP_DECODE=fast: the run stays in fast mode and -d / -D / -c / -s decode from the fast
E-step's tables (include/psmc_hip.h).  -N0 decodes the starting parameters, so the fast and the exact run decode the same
model: same lines, numbers within the library's tolerances (to the last printed digit), DC runs identical except at
near-ties, which the exact run's own -D output shows to be ties.  Without PSMC_HIP_DECODE nothing changes."""
import os
import subprocess
import numpy as np
import pytest
from conftest import GOLD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "psmc_amd", "host")
CLI = os.path.join(GOLD, "cli")
FALLBACK = "decoding needs the exact forward/backward tables; using PSMC_HIP_MODE=exact"
FAST_DEC = dict(PSMC_HIP_MODE="fast", PSMC_HIP_DECODE="fast")


@pytest.fixture(scope="module")
def psmc():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    return os.path.join(HOST, "psmc")


def run(psmc, args, **env):
    e = dict(os.environ)
    for k in ("PSMC_HIP_MODE", "PSMC_HIP_DECODE", "PSMC_HIP_OPTIONS", "PSMC_HIP_DEVICES"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([psmc] + args, cwd=CLI, capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stderr[-800:]
    return r.stdout, r.stderr


def _unit(field):
    """one unit of the last printed digit of a %f-style field"""
    return 10.0 ** -(len(field) - field.index(".") - 1) if "." in field else 1.0


def _close(x, y, rel):
    """two printed numbers whose true values are within `rel` relative (1e-9 absolute for probabilities): at most one printed unit apart"""
    if x == y:
        return True
    a, b = float(x), float(y)
    return abs(a - b) <= _unit(y) * 1.0001 + rel * abs(b)


def _path(lines, L_of):
    """per-position states of the DC lines of each segment"""
    out = {}
    for l in lines:
        f = l.split("\t")
        name, s, t, k = f[1], int(f[2]), int(f[3]), int(f[4])
        out.setdefault(name, np.full(L_of[name] + 1, -1))[s:t + 1] = k
    return out


def compare(fast, exact, exact_D=None):
    fl, xl = fast.splitlines(), exact.splitlines()
    fdc = [l for l in fl if l.startswith("DC")]
    xdc = [l for l in xl if l.startswith("DC")]
    fo = [l for l in fl if not l.startswith("DC")]
    xo = [l for l in xl if not l.startswith("DC")]
    assert len(fo) == len(xo)
    for a, b in zip(fo, xo):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[0] == fb[0] and len(fa) == len(fb), (a[:80], b[:80])
        tag = fa[0]
        if tag in ("DF", "CT", "PR"):
            rel = {"DF": 1e-9, "CT": 1e-9, "PR": 1e-11}[tag]
            start = 3 if tag == "PR" else 2
            assert fa[:start] == fb[:start], (a[:80], b[:80])
            bad = [(x, y) for x, y in zip(fa[start:], fb[start:]) if not _close(x, y, rel)]
            assert not bad, (tag, bad[:5])
        else:
            assert a == b   # header, rounds, TC
    if fdc == xdc:
        return 0
    # DC runs that differ: only at positions where the exact posterior has a tie to the printed precision (its -D output)
    assert exact_D is not None, "DC lines differ and no -D output to check them against"
    L_of = {}
    for l in xl:
        if l.startswith("DC"):
            f = l.split("\t"); L_of[f[1]] = max(L_of.get(f[1], 0), int(f[3]))
    pf, px = _path(fdc, L_of), _path(xdc, L_of)
    df = [l.split("\t") for l in exact_D.splitlines() if l.startswith("DF")]
    rows, seg_rows, names = [], {}, list(L_of)
    i = 0
    for nm in names:   # DF lines carry no segment name: they follow the segments in input order
        seg_rows[nm] = df[i:i + L_of[nm]]; i += L_of[nm]
    n_diff = 0
    for nm in names:
        for u in np.nonzero(pf[nm][1:] != px[nm][1:])[0] + 1:
            post = sorted(float(v) for v in seg_rows[nm][u - 1][3:])
            assert post[-1] - post[-2] <= 1e-4 + 1e-12, (nm, u, post[-2:])
            n_diff += 1
    return n_diff


SMALL = ["small.psmcfa"]
T10K = ["-i", "t10k_restart.par", "t10k.psmcfa"]
CNT = ["-c", "small.cnt"]   # (a cntcpg record per segment of small.psmcfa)
CASES = [("small", ["-d"]), ("small", ["-D"]), ("small", CNT), ("small", ["-s"]), ("small", ["-d"] + CNT),
         ("t10k", ["-d"]), ("t10k", ["-D"]), ("t10k", ["-s"])]


@pytest.mark.parametrize("inp,flags", CASES, ids=["%s%s" % (i, "".join(x for x in f if x.startswith("-"))) for i, f in CASES])
def test_fast_decode_cli_matches_exact(psmc, inp, flags):
    tail = SMALL if inp == "small" else T10K
    args = ["-N0"] + flags + tail
    fast, err = run(psmc, args, **FAST_DEC)
    assert FALLBACK not in err and "PSMC_HIP_DECODE=fast" in err, err
    exact, _ = run(psmc, args)
    exact_D = run(psmc, ["-N0", "-D"] + tail)[0] if "-d" in flags else None
    compare(fast, exact, exact_D)


def test_fast_decode_cli_em_rounds_unchanged(psmc):
    """-N4 -d: the EM rounds are the plain fast run's byte for byte (only MM is_decoding differs), then the decoding."""
    with_d, _ = run(psmc, ["-N4", "-d"] + SMALL, **FAST_DEC)
    plain, _ = run(psmc, ["-N4"] + SMALL, PSMC_HIP_MODE="fast")
    head = with_d[:with_d.index("TC\t")]
    assert head.replace("MM\tis_decoding:1\n", "MM\tis_decoding:0\n") == plain
    assert "DC\t" in with_d


def test_without_the_switch_nothing_changes(psmc):
    """PSMC_HIP_MODE=fast with -d and no PSMC_HIP_DECODE: the fallback message and an exact run, byte for byte the reference's."""
    args = open(os.path.join(CLI, "small_decode_d.args")).read().split()
    out, err = run(psmc, args, PSMC_HIP_MODE="fast")
    assert FALLBACK in err
    assert out == open(os.path.join(CLI, "small_decode_d.psmc")).read()


@pytest.mark.parametrize("flags", [["-d"], ["-D"]])
def test_fast_decode_cli_capped_matrix(psmc, flags):
    """-C: a matrix without the PSMC form -> the dense fast sweeps, decoded from their tables."""
    args = ["-N0", "-C", "12"] + flags + SMALL
    fast, err = run(psmc, args, **FAST_DEC)
    exact, _ = run(psmc, args)
    compare(fast, exact, run(psmc, ["-N0", "-C", "12", "-D"] + SMALL)[0] if "-d" in flags else None)


def test_fast_decode_cli_device_list(psmc):
    """PSMC_HIP_DEVICES=0,0: the decoding entry points reach each segment's shard through psmc_hip_group_route."""
    args = ["-N0", "-D", "-c", "small.cnt"] + SMALL
    fast, err = run(psmc, args, PSMC_HIP_DEVICES="0,0", **FAST_DEC)
    exact, _ = run(psmc, args)
    compare(fast, exact)


def test_fast_decode_cli_exact_fallback(psmc):
    """A decoding E-step whose tile boundaries cannot converge (64-bin warm-ups, no repair round): it is repeated by the exact
    twin, and the decoding reads the twin's tables -- the exact decoding of the same parameters, byte for byte."""
    for flag in ("-d", "-s"):
        a = ["-N0", "-t15", "-r5", "-p", "4+25*2+4+6", flag, "mid.psmcfa.gz"]
        fast, err = run(psmc, a, PSMC_HIP_OPTIONS="warmup=64,chunk=512,max_rounds=0,learn=0", **FAST_DEC)
        assert err.count("repeating this E-step with the exact kernels") == 1, err[-600:]
        exact, _ = run(psmc, a)
        assert fast == exact
