"""The CPU side of the gate of long-lived contexts (tests/ctx_history.py, tests/test_gpu_ctx_history.py): the histories cover what
they claim to, the table of plan options is the source's, and every exact-mode history runs end to end on the oracle, so the
references exist and the histories are valid before a device sees them.

The coverage conditions are computed from the histories alone, so a later edit cannot hollow the gate:
  (C1) every operation kind that applies to a context kind (ctx_history.NOT_APPLICABLE names the others and why) occurs at least ten
       times over the hand-written and the generated histories of that kind;
  (C2) every plan option that the kind's path reads (PLAN_OPTIONS_OF) is changed at least once;
  (C3) every ordered pair of the three data pools occurs as consecutive loads;
  (C4) every decoding call follows, as the last state operation before it, each of: a single E-step, a batch, a select, a reload --
       and a factored E-step on the wide kind, whose factored E-step leaves tables to decode (up to 128 states it keeps no backward
       table: there one refused decode after it, in S2; an exact context has none);
  (C5) at most a quarter of the checked calls of any history are refusals by construction (`bad_call`, expect "refused").
"""
import os
import time

import pytest

import ctx_history as ch
import exact_extremes as xx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ch.all_histories()


def of_kind(kind):
    return [h for h in ALL if h[1] == kind]


def test_option_table_is_the_source():
    """every key psmc_hip_set_option accepts is classified, and as the source has it"""
    with open(os.path.join(ROOT, "psmc_amd", "csrc", "api.hip")) as f:
        src = ch.options_in_source(f.read())
    assert len(src) > 50, len(src)
    assert not (ch.PLAN_OPTIONS & ch.OTHER_OPTIONS)
    assert set(src) == ch.PLAN_OPTIONS | ch.OTHER_OPTIONS, set(src) ^ (ch.PLAN_OPTIONS | ch.OTHER_OPTIONS)
    assert {k for k, dirty in src.items() if dirty} == ch.PLAN_OPTIONS
    for kind in ch.KINDS:
        assert set(ch.PLAN_OPTIONS_OF[kind]) <= ch.PLAN_OPTIONS
    assert set(ch.PLAN_OPTIONS_OF["fast"]) | set(ch.PLAN_OPTIONS_OF["wide"]) == ch.PLAN_OPTIONS


def test_histories_are_what_the_gate_claims():
    ids = [h[0] for h in ALL]
    assert len(set(ids)) == len(ids)
    for kind in ch.KINDS:
        gen = [h for h in of_kind(kind) if h[0].startswith("gen")]
        assert len(gen) == ch.N_GENERATED and all(len(h[3]) == ch.N_OPS for h in gen)
        assert {h[2] for h in of_kind(kind)} == set(ch.SIZES[kind]), kind
        assert all(h[2] != 1024 for h in gen)
    for name, (fn, kinds) in ch.HAZARDS.items():
        for kind in kinds:
            assert ch.HAZARD_SIZES[kind][name], (name, kind)
    for n_seg in (5, 9, 13):
        for sel in ch.SELECTIONS[n_seg]:
            xx.assert_selection(sel, n_seg)
    assert ch.generated("fast", 64, 3) == ch.generated("fast", 64, 3)   # fixed seeds


@pytest.mark.parametrize("kind", ch.KINDS)
def test_coverage(kind):
    hs = of_kind(kind)
    count = {}
    for _, _, _, h in hs:
        for o in h:
            count[o.kind] = count.get(o.kind, 0) + 1
    for k in ch.VOCABULARY:      # (C1)
        if k not in ch.NOT_APPLICABLE[kind]:
            assert count.get(k, 0) >= 10, (kind, k, count.get(k, 0))
    changed = {o.args[0] for _, _, _, h in hs for o in h if o.kind == "option"}      # (C2)
    assert set(ch.PLAN_OPTIONS_OF[kind]) <= changed, set(ch.PLAN_OPTIONS_OF[kind]) - changed
    pairs = set()      # (C3)
    for _, _, _, h in hs:
        loads = [o.args[0] for o in h if o.kind in ("load", "load_device")]
        pairs |= set(zip(loads, loads[1:]))
    want = {(x, y) for x in ("small", "medium", "large") for y in ("small", "medium", "large") if x != y}
    assert want <= pairs, want - pairs
    after = {d: set() for d in ch.DECODING}      # (C4)
    for _, _, _, h in hs:
        last = None
        for o in h:
            if o.kind in ch.DECODING:
                after[o.kind].add(last)
            elif o.kind in ch.STATE_OPS and o.kind not in ("option", "reserve"):
                last = "reload" if o.kind in ("load", "load_device") else o.kind
    need = {"estep", "batch", "select", "reload"} | ({"estep_factored"} if kind == "wide" else set())
    for d in ch.DECODING:
        assert need <= after[d], (kind, d, need - after[d])
    if kind == "fast":
        assert "estep_factored" in after["decode"]
    for hid, _, _, h in hs:      # (C5)
        checked = sum(1 for o in h if o.kind in ch.CHECKED) + 1    # (and the final E-step)
        assert 4 * ch.expected_refusals(h) <= checked, (hid, ch.expected_refusals(h), checked)


EXACT = [h for h in ALL if h[1] == "exact"]
SECONDS = {}


@pytest.mark.parametrize("hid", [h[0] for h in EXACT])
def test_exact_history_on_the_oracle(golden, oracle, hid):
    """the history is valid and its references exist: every call returns what the history expects of it, and the digests are the
    same the second time (the references are functions of the history)"""
    _, kind, n, h = ch.history_by_id(hid)
    t0 = time.time()
    d1 = ch.interpret(h, ch.OracleBackend(oracle, golden, n), kind, n)
    SECONDS[hid] = time.time() - t0
    assert len(d1) == sum(1 for o in h if o.kind in ch.CHECKED) + 1
    if len(h) <= ch.N_OPS + 2:
        assert d1 == ch.interpret(h, ch.OracleBackend(oracle, golden, n), kind, n)
    print("%s: %d checked calls, %.1f s on the oracle" % (hid, len(d1), SECONDS[hid]))
