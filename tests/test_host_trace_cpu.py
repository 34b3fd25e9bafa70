"""CPU: the host layer of the sampler, the table arenas and the multi-stream decoder does what it did before it was restructured.
tests/golden/gen_host_trace.py runs a fixed script -- every set_* of a Sampler, load / unload of the four arenas, every refusal
of admit / admit_n / load / extend / fork / score / admit_guided that precedes device work, and well-formed admissions up to their
first kernel -- and records the row tensors byte for byte, the host notes, the handles and each refusal's type and full text.
tests/golden/host_trace.json is that record as the commit before the restructuring produced it; here the same script runs on the
working tree and every entry must be equal, exactly."""
import json
import os
import sys

import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import gen_host_trace  # noqa: E402


@pytest.fixture(scope="module")
def traces():
    with open(os.path.join(GOLDEN, "host_trace.json")) as fh:
        want = json.load(fh)
    return want, json.loads(json.dumps(gen_host_trace.trace()))


def test_the_script_makes_the_recorded_calls_in_the_recorded_order(traces):
    want, got = traces
    assert [e["call"] for e in got] == [e["call"] for e in want]


def test_every_entry_equals_its_record(traces):
    want, got = traces
    for w, g in zip(want, got):
        assert g.get("raised") == w.get("raised"), w["call"]
        assert g.get("returned") == w.get("returned"), w["call"]
        assert g["state"].keys() == w["state"].keys(), w["call"]
        for k in w["state"]:
            assert g["state"][k] == w["state"][k], (w["call"], k)
        assert g == w, w["call"]


def test_the_record_covers_what_it_is_meant_to(traces):
    want, _ = traces
    calls = {e["call"]: e for e in want}
    raised = {e["call"]: e["raised"] for e in want if "raised" in e}
    assert sum(r[0] == "RuntimeError" and "no CPU fallback" in r[1] for r in raised.values()) >= 7      # the well-formed admissions
    assert sum(r[0] == "ValueError" for r in raised.values()) >= 120
    for space in ("Sampler(plain)", "Sampler(full)", "BiasTables", "BanTables", "FsmTables", "LoraTable", "full", "ring", "plain", "none"):
        assert f"{space}.new" in calls, space
    for arena in ("BiasTables", "BanTables", "FsmTables", "LoraTable"):
        assert "are taken" in raised[f"{arena}.load 2"][1] or "arena is full" in raised[f"{arena}.load 2"][1]
        for what in ("unload 0 again (stale)", "unload the stale handle of a place that is taken again", "unload a foreign handle"):
            assert raised[f"{arena}.{what}"][1].endswith("is not loaded here"), (arena, what)
        assert "raised" not in calls[f"{arena}.reload into the freed place"]
    # the row setup of a well-formed admission reached the sampler's rows before the first kernel
    assert {"row.temperature", "row.fsm_state", "row.bias_idx", "row.ban_idx"} <= set(
        calls["full.admit(3, every option, no prompt_ids): stops at the prefill"]["state"])
    assert "row.ctx" in calls["ring.admit(1, sampling, bad_words, prompt_ids): stops at the prefill"]["state"]
