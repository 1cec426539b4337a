"""tools/ab.py, the measuring protocol the tools/*_bench.py scripts share, on the CPU with a fake event pair: the order
of warm-up and timed calls, the restore of a toggled flag (also when the timed callable raises), the summary's rounding,
the three verdict rules at their edges, and that every tool built on it imports without touching a device."""
import functools
import importlib
import math
import os
import sys
import types

import pytest
import torch

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
for p in (TOOLS, os.path.join(TOOLS, "probes")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ab  # noqa: E402


class FakeCuda:
    """Stands in for torch.cuda in ab.time_us: events that count what was recorded between them."""

    def __init__(self):
        self.log = []
        outer = self

        class Event:
            def __init__(self, enable_timing):
                assert enable_timing

            def record(self):
                outer.log.append(self)
                self.at = len(outer.log)

            def synchronize(self):
                pass

            def elapsed_time(self, stop):  # ms: one per entry logged between the two records
                return float(stop.at - self.at - 1)

        self.Event = Event

    def synchronize(self):
        self.log.append("sync")

    def calls(self):
        return [e for e in self.log if isinstance(e, str)]


def test_time_us_counts_calls_between_the_events():
    cuda = FakeCuda()
    us = ab.time_us(lambda: cuda.log.append("f"), 4, cuda=cuda)
    assert us == 4 * 1e3 / 4 and cuda.calls() == ["f"] * 4
    cuda = FakeCuda()
    ab.time_us(lambda: cuda.log.append("f"), 2, warmup=3, cuda=cuda)
    assert cuda.calls() == ["f"] * 3 + ["sync"] + ["f"] * 2 and not isinstance(cuda.log[4], str)  # start after the sync
    cuda = FakeCuda()
    ab.time_us(lambda: cuda.log.append("f"), 2, warmup=3, sync=False, cuda=cuda)
    assert cuda.calls() == ["f"] * 5


@pytest.mark.parametrize("warm,warm_calls", [("call", 1), (1, 1), (2, 2)])
def test_alternate_order(warm, warm_calls):
    cuda = FakeCuda()
    arms = {"A": lambda: cuda.log.append("A"), "B": lambda: cuda.log.append("B")}
    times = ab.alternate(arms, 3, 4, warm=warm, time=functools.partial(ab.time_us, cuda=cuda))
    assert cuda.calls() == ["A"] * warm_calls + ["B"] * warm_calls + (["A"] * 4 + ["B"] * 4) * 3
    assert list(times) == ["A", "B"] and all(len(t) == 3 for t in times.values())
    assert times["A"] == [1e3] * 3  # 4 calls between the events of every timed round, over iters = 4


def test_alternate_custom_warm_gets_name_and_callable():
    seen = []
    ab.alternate({"A": lambda: seen.append("a"), "B": lambda: seen.append("b")}, 0, 1,
                 warm=lambda name, run: (seen.append(name), run()))
    assert seen == ["A", "a", "B", "b"]


def test_setting_arm_applies_and_restores():
    cuda, mod, during = FakeCuda(), types.SimpleNamespace(FLAG="before"), []

    def fn():
        during.append(mod.FLAG)
        cuda.log.append("f")

    times = ab.alternate({True: (mod, "FLAG", True), False: (mod, "FLAG", False)}, 2, 3, fn=fn, warm=1,
                         time=functools.partial(ab.time_us, cuda=cuda))
    assert during == [True, False] + ([True] * 3 + [False] * 3) * 2
    assert mod.FLAG == "before" and [len(t) for t in times.values()] == [2, 2]
    assert ab.switch_arms(mod, "FLAG") == {True: (mod, "FLAG", True), False: (mod, "FLAG", False)}


def test_setting_arm_restores_when_the_timed_callable_raises():
    cuda, mod, during = FakeCuda(), types.SimpleNamespace(FLAG=True), []

    def fn():
        during.append(mod.FLAG)
        if len(during) == 4:  # warm native, warm off, timed native, then the timed call with the flag off
            raise RuntimeError("step failed")

    with pytest.raises(RuntimeError, match="step failed"):
        ab.alternate(ab.switch_arms(mod, "FLAG"), 2, 1, fn=fn, time=functools.partial(ab.time_us, cuda=cuda))
    assert during == [True, False, True, False] and mod.FLAG is True


def test_summary():
    assert ab.summary([10.04, 10.06, 30.0]) == {"median_us": 10.1, "min_us": 10.0, "max_us": 30.0}


def _s(median, lo, hi):
    return {"median_us": median, "min_us": lo, "max_us": hi}


def test_tie_rule_edge():
    other = _s(100.0, 99.0, 101.5)  # spread 2.5
    assert ab.larger_spread(_s(0.0, 102.0, 103.0), other) == 2.5 and ab.larger_spread(other, _s(0.0, 1.0, 5.0)) == 4.0
    edge = other["median_us"] + 2.5
    assert ab.tie_within_spread(_s(edge, 102.0, 103.0), other) == "tie"
    assert ab.tie_within_spread(_s(math.nextafter(edge, math.inf), 102.0, 103.0), other) == "native slower"


def test_below_median_and_below_fastest_disagree_between_min_and_median():
    native, other = _s(95.0, 94.0, 96.0), _s(100.0, 90.0, 110.0)
    assert ab.median_below_median(native, other) and not ab.median_below_fastest(native, other)
    assert ab.median_below_fastest(_s(89.9, 89.0, 91.0), other)
    assert not ab.median_below_median(_s(100.0, 99.0, 101.0), other)  # strictly below, as the tools had it


def test_tie_report_fields():
    rep = ab.tie_report({True: [10.0, 12.0, 11.0], False: [9.0, 9.5, 9.2]}, "step", other="switch_off")
    assert rep == {"native_step": _s(11.0, 10.0, 12.0), "switch_off_step": _s(9.2, 9.0, 9.5), "larger_spread_us": 2.0,
                   "native_over_switch_off_median": 1.196, "verdict": "tie"}
    assert list(ab.tie_report({True: [1.0], False: [1.0]}, "fwd_bwd")) == [
        "native_fwd_bwd", "framework_fwd_bwd", "larger_spread_us", "native_over_framework_median", "verdict"]


def test_lines_and_parser(tmp_path, capsys):
    a = ab.parser(iters=5).parse_args(["--quick", "--out", str(tmp_path / "sub" / "o.jsonl")])
    assert (a.rounds, a.iters, a.quick) == (7, 5, True)
    assert ab.parser().parse_args([]).iters == 10 and ab.parser().parse_args([]).out is None
    lines = ab.Lines(a.out)
    lines.emit({"b": 1, "a": {"median_us": 1.5}})
    lines.emit({"c": True})
    lines.write()
    text = '{"b": 1, "a": {"median_us": 1.5}}\n{"c": true}\n'
    assert capsys.readouterr().out == text and open(a.out).read() == text


@pytest.mark.parametrize("name", [
    "attn_backward_bench", "layernorm_backward_bench", "merge_backward_bench", "mlp_backward_bench",
    "vivit_backward_bench", "motionformer_backward_bench", "timesformer_backward_bench", "autocast_bench",
    "attn_bench", "attn_short_bench", "temporal_attn_bench", "merge_exp", "tubelet_rows_bench"])
def test_tool_imports_without_a_device(name):
    mod = importlib.import_module(name)
    assert callable(mod.main)
    assert os.path.dirname(os.path.abspath(mod.__file__)).startswith(TOOLS)
    assert not torch.cuda.is_initialized()
    assert not any(hasattr(mod, gone) for gone in ("_time", "_stats", "_compare", "_verdict", "_alternate", "timeit",
                                                   "timed"))
