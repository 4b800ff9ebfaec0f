"""The gate of long-lived contexts: every call of a history on ONE context returns the return code and the bits of the same call on
a twin -- a context made for that one check and given the minimal replay of its kind (tests/ctx_history.py states the invariant and
the replay rule, DESIGN.md promises both under "Long-lived contexts").  Exact-mode histories are held to the CPU oracle call by call as well, Viterbi and sampling
to their numpy models, so a twin with the same defect cannot hide it.  No tolerance anywhere: bits and return codes.

One test per (history, context kind, state count): nine hand-written hazards (S1 reloads that shrink and grow, S2 multiset selections,
S3 table ownership, S4 the checkpoint options of the wide path, S5 the chain options in every order, S6 the users of the per-call
scratch interleaved, S7 tilings, S8 batches, S9 refusals in the middle) and twelve generated histories of 25 operations per kind.
A failure names the operation index, the operation, the first differing output and element, and the last event that made the plan
dirty.  After the last operation of every history a final E-step is compared with a twin and the context is closed.

test_poisoned_children runs one history per kind (S6; S4 as well on the wide path) in fresh child processes under
PSMC_HIP_POISON=vary and =1 -- every allocation of the contexts and every block of the per-call scratch filled with garbage -- and holds
the children's digests to the parent's unpoisoned ones: garbage never reaches a result."""
import json
import os
import subprocess
import sys
import time

import pytest

import ctx_history as ch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ch.all_histories()
CALLS = {k: 0 for k in ch.KINDS}
REFUSED = {k: 0 for k in ch.KINDS}
LINES = []
SECONDS = {}


@pytest.fixture(scope="module")
def hip():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "psmc_amd", "csrc")], check=True)
    from psmc_amd import hip as h
    assert h.load_library().psmc_hip_device_count() > 0, "GPU tests need a visible HIP device"
    return h


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if SECONDS:
        slow = max(SECONDS, key=SECONDS.get)
        LINES.append("ctx history gate: %.1f s in all, slowest %s %.1f s; checked calls (of them refused) %s" % (
            sum(SECONDS.values()), slow, SECONDS[slow], ", ".join("%s %d (%d)" % (k, CALLS[k], REFUSED[k]) for k in ch.KINDS)))
        print("\n" + LINES[-1])
        if os.environ.get("PSMC_CTX_HISTORY_REPORT"):   # one line per history and the totals (profiles/ctx_history_tests.txt)
            with open(os.environ["PSMC_CTX_HISTORY_REPORT"], "w") as f:
                f.write("\n".join(LINES) + "\n")


@pytest.mark.parametrize("hid", [h[0] for h in ALL])
def test_history(hip, golden, oracle, hid):
    _, kind, n, h = ch.history_by_id(hid)
    t0 = time.time()
    ref = ch.OracleBackend(oracle, golden, n) if kind == "exact" else None
    d = ch.interpret(h, ch.DeviceBackend(hip, golden, kind, n), kind, n, twin_of=ch.device_twin(hip, golden, kind, n), reference=ref)
    SECONDS[hid] = time.time() - t0
    CALLS[kind] += len(d)
    refused = sum(1 for x in d if x[0] != "ok")
    assert 4 * refused <= len(d) or not hid.startswith("S"), (hid, refused, len(d))   # the hand-written ones hold (C5) on the device too
    if hid.startswith(ch.EXACT_REFUSALS):
        assert refused == ch.expected_refusals(h), (hid, refused, ch.expected_refusals(h))   # every E-step and batch returned ok
    REFUSED[kind] += refused
    LINES.append("%-24s %3d checked calls, %2d refused (%2d expected), %4.1f s" % (hid, len(d), refused, ch.expected_refusals(h), SECONDS[hid]))
    print(LINES[-1])


@pytest.mark.parametrize("kind, n, name", ch.POISONED, ids=lambda v: str(v))
def test_poisoned_children(hip, golden, kind, n, name):
    hid = "%s-%s-%d" % (name, kind, n)
    _, _, _, h = ch.history_by_id(hid)
    want = ch.interpret(h, ch.DeviceBackend(hip, golden, kind, n), kind, n)
    assert sum(1 for x in want if x[0] == "ok") >= len(want) * 3 // 4
    tag = "DIGESTS "
    for poison in ("vary", "1"):   # one after the other, each under its own time limit
        r = subprocess.run([sys.executable, "-c", ch.child_code(hid, tag)], capture_output=True, text=True,
                           env=dict(os.environ, PSMC_HIP_POISON=poison), timeout=300)
        lines = [x for x in r.stdout.splitlines() if x.startswith(tag)]
        assert r.returncode == 0 and len(lines) == 1, (poison, r.stdout[-500:], r.stderr[-1500:])
        got = json.loads(lines[0][len(tag):])
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "PSMC_HIP_POISON=%s, checked call %d of %s: %s against the unpoisoned %s" % (poison, i, hid, g, w)
