"""Host-only logic of the native backward: which call takes the native Functions and which keeps the framework path
(the predicate alone, no device), and the argument checks of the new entry points that need no GPU."""
import ctypes

import pytest
import torch


def _covers(kind, **facts):
    from tome import merge as M
    base = dict(even_odd=True, hybrid=False, distill_token=False, on_device=True, dtype=torch.float32, mode=None,
                size_requires_grad=False, enabled=True)
    base.update(facts)
    if kind == "merge" and "mode" not in facts:
        base["mode"] = "mean"
    return M.native_backward_covers(kind, **base)


def test_covered_cases_take_the_native_functions():
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        assert _covers("merge", mode="sum", dtype=dtype)
        assert _covers("merge", mode="mean", dtype=dtype)
        assert _covers("merge_wavg", dtype=dtype)
        assert _covers("drop", dtype=dtype)
        assert _covers("unmerge", dtype=dtype)
    # a distillation token is covered by the merge forms, not by unmerge
    assert _covers("merge", mode="sum", distill_token=True)
    assert _covers("merge_wavg", distill_token=True)
    assert _covers("drop", distill_token=True)
    assert not _covers("unmerge", distill_token=True)


@pytest.mark.parametrize("kind", ["merge", "merge_wavg", "drop", "unmerge"])
def test_not_covered_cases_keep_the_framework_path(kind):
    assert _covers(kind)
    assert not _covers(kind, even_odd=False)            # kth_ / random_ partition plans
    assert not _covers(kind, hybrid=True)               # threshold flags
    assert not _covers(kind, on_device=False)           # CPU tensors
    assert not _covers(kind, dtype=torch.float64)
    assert not _covers(kind, enabled=False)             # the A/B flag
    if kind == "merge":
        for mode in ("max", "amax", "min", "amin", "prod", "median"):
            assert not _covers(kind, mode=mode)
    assert _covers(kind, size_requires_grad=True) == (kind != "merge_wavg")


def test_flag_is_a_module_attribute_and_is_read_per_call(monkeypatch):
    from tome import merge as M
    assert M.NATIVE_BACKWARD is True
    assert M.native_backward_covers("drop", even_odd=True)
    monkeypatch.setattr(M, "NATIVE_BACKWARD", False)
    assert not M.native_backward_covers("drop", even_odd=True)
    assert M.native_backward_covers("drop", even_odd=True, enabled=True)
    with pytest.raises(ValueError):
        M.native_backward_covers("merge_source", even_odd=True)


def test_plan_facts_feed_the_predicate():
    """`_covers` reads the facts off a plan and a tensor: a CPU tensor is never covered, whatever the plan."""
    from tome import _abi, merge as M
    plan = _abi.MatchPlan(1, 8, 2, False, False, None, None, None, None, None, torch.device("cuda", 0))
    assert plan.count is None
    x = torch.zeros(1, 8, 4, requires_grad=True)
    assert not M._covers("merge", plan, x, mode="sum")
    assert not M._covers("merge", object(), x, mode="sum")


def test_backward_entry_points_validate_on_the_host():
    from tome import _abi
    L = _abi.lib()
    assert L.tome_abi_version() == 11 == _abi.ABI_VERSION
    assert {"tome_merge_backward", "tome_merge_backward_regrouped"} <= set(_abi.SYMBOLS)
    buf = ctypes.create_string_buffer(64)
    rc = L.tome_merge_backward(None, 0, None, None, 0, 2, 16, 8, 4, buf, 0, 0, buf, None)
    assert rc == 1 and b"tome_merge_backward" in L.tome_last_error()
    rc = L.tome_merge_backward(buf, 0, None, None, 0, 1, 8, 4, 9, buf, 0, 0, buf, None)
    assert rc == 1  # r outside (0, T/2]
    rc = L.tome_merge_backward(buf, 0, None, None, 0, 1, 8, 4, 2, None, 0, 0, buf, None)
    assert rc == 1 and b"row_map" in L.tome_last_error()
    rc = L.tome_merge_backward(buf, 0, buf, None, 0, 1, 8, 4, 2, buf, 0, 1, buf, None)
    assert rc == 1 and b"drop" in L.tome_last_error()
    rc = L.tome_merge_backward(buf, 1, buf, None, 2, 1, 8, 4, 2, buf, 0, 0, buf, None)
    assert rc == 1 and b"dtypes" in L.tome_last_error()  # bf16 tokens with fp16 sizes
    rc = L.tome_merge_backward_regrouped(buf, 0, None, None, 0, 0, 4, 8, 4, 2, 1, buf, 0, buf, None)
    assert rc == 1 and b"tome_merge_backward_regrouped" in L.tome_last_error()
    with pytest.raises(_abi.TomeHipError, match="no CPU path"):
        _abi.merge_backward(_abi.MatchPlan(1, 8, 2, False, False, None, None, None, None, None, torch.device("cuda", 0)),
                            torch.zeros(1, 6, 4))
