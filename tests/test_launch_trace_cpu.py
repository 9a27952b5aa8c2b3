"""Every engine against its recorded launch trace (tests/launch_trace.py, tests/golden/launch_traces.json): the same libmmrca calls in
the same order with the same arguments, on buffers of the same size, dtype and sharing pattern.  No GPU, no libmmrca.so.  What a trace
does not see are torch-side copies between launches (index_select, copy_, zero_, index_copy_); the engines' GPU suites cover those."""
import json
import os

import pytest

from tests import launch_trace as LT

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_traces.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_lists_exactly_the_configurations():
    assert list(GOLDEN) == list(LT.CONFIGS)
    assert all(g["count"] == len(g["calls"]) > 0 for g in GOLDEN.values())


@pytest.mark.parametrize("name", list(LT.CONFIGS))
def test_engine_issues_the_recorded_launches(name, monkeypatch):
    lines = LT.trace(name, monkeypatch)
    want = GOLDEN[name]["calls"]
    for idx, (line, rec) in enumerate(zip(lines, want)):
        assert LT.entry(line) == rec, (f"{name}: launch {idx} differs from the recorded {rec.split()[0]}; it is now\n  {line}\n"
                                       f"(make_launch_traces.py --dump DIR writes the whole trace)")
    assert len(lines) == GOLDEN[name]["count"], (f"{name}: {len(lines)} launches, {GOLDEN[name]['count']} recorded; the first "
                                                 f"{min(len(lines), len(want))} agree" + (f", then comes\n  {lines[len(want)]}" if len(lines) > len(want) else ""))


def test_a_changed_launch_is_named_with_its_index(monkeypatch):
    """the comparison itself: one argument of one launch changed -> its digest changes; an unresolvable pointer is an error"""
    lines = LT.trace("blip2-tiny-bf16-eval", monkeypatch)
    want = GOLDEN["blip2-tiny-bf16-eval"]["calls"]
    changed = lines[7].replace("(", "(None, ", 1)
    assert LT.entry(lines[7]) == want[7] and LT.entry(changed) != want[7] and LT.entry(changed).split()[0] == want[7].split()[0]
    with pytest.raises(LT.TraceError, match="resolves to no known allocation"):
        LT.canonical([("mmrca_split_f32", (0x1000, None, None, 4, 0))], [])
    with pytest.raises(LT.TraceError, match="takes 5 arguments"):
        LT.canonical([("mmrca_split_f32", (None, None, None, 4))], [])
