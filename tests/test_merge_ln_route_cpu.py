"""Which route `merge_then_norm` (tome/patch/_common.py) takes with the switch TRAIN_FUSED_LN, on CPU tensors with the
launch seams of tests/test_modes_route_cpu.py (its recorder class is reused) plus recorders in place of the two public
calls the trained route goes through, tome.merge.merge_wavg_ln and tome.merge.drop_ln.  A literal table holds (mode, who
requires grad, token dtype, switch, trace_source) against the route; 'hybrid' is the mode column's third value.  With
the switch off the table is today's.  `_abi.merge_ln_trainable` asks `x.is_cuda` itself, so CPU tensors never take the
Function; the table rows that show the Function's route put a copy of the predicate without that clause in its place."""
import pytest
import torch

import test_modes_route_cpu as base

BF, HF, F32 = base.BF, base.HF, base.F32
MERGE_LN, DROP_LN, UNFUSED = base.MERGE_LN, base.DROP_LN, base.UNFUSED
FUNCTION = "function"  # the public call, which takes _MergeLnFunction on a device

# mode, who requires grad, dtype, TRAIN_FUSED_LN, trace_source -> route
TABLE = [
    # switch off: today's table -- the fused launch without grad, the three steps with it
    ("merge", None, BF, False, False, MERGE_LN),
    ("merge", "x", BF, False, False, UNFUSED),
    ("merge", "residual", BF, False, False, UNFUSED),
    ("merge", "norm", BF, False, False, UNFUSED),
    ("drop", None, BF, False, False, DROP_LN),
    ("drop", "x", BF, False, False, UNFUSED),
    ("hybrid", None, BF, False, False, MERGE_LN),
    ("hybrid", "x", BF, False, False, UNFUSED),
    ("random_merge", "norm", BF, False, False, UNFUSED),
    # switch on, nobody wants a gradient: nothing changes
    ("merge", None, BF, True, False, MERGE_LN),
    ("drop", None, HF, True, False, DROP_LN),
    ("hybrid", None, BF, True, False, MERGE_LN),
    # switch on, a participant wants one: the Function for the kinds "merge" and "drop"
    ("merge", "x", BF, True, False, FUNCTION),
    ("merge", "residual", BF, True, False, FUNCTION),
    ("merge", "norm", BF, True, False, FUNCTION),
    ("merge", "x", HF, True, False, FUNCTION),
    ("random_merge", "x", BF, True, False, FUNCTION),
    ("drop", "x", BF, True, False, FUNCTION),
    ("drop", "residual", HF, True, False, FUNCTION),
    ("random_drop", "norm", BF, True, False, FUNCTION),
    # ... and what it does not cover keeps the three steps
    ("hybrid", "x", BF, True, False, UNFUSED),
    ("hybrid", "norm", BF, True, False, UNFUSED),
    ("merge", "x", F32, True, False, UNFUSED),
    ("drop", "residual", F32, True, False, UNFUSED),
    ("merge", "x", BF, True, True, UNFUSED),
    ("drop", "norm", BF, True, True, UNFUSED),
]


def _ids(table):
    return ["-".join(str(v).replace("torch.", "") for v in row[:5]) for row in table]


def _run(monkeypatch, row, device_free_predicate=True, size=None, norm_cls=torch.nn.LayerNorm):
    mode, who, dtype, switch, trace, _ = row
    from tome import _abi
    from tome import merge as M
    seams, C, _ = base._setup(monkeypatch, (mode, False, dtype, False, trace, True, True, True, False))
    monkeypatch.setattr(C, "TRAIN_FUSED_LN", switch)
    if device_free_predicate:
        def trainable(x, norm, addend, merge=None):  # _abi.merge_ln_trainable without `x.is_cuda` and the plan's class
            return (x.dim() == 3 and _abi.ln_trainable(x, norm)
                    and (addend is None or (addend.shape == x.shape and addend.dtype == x.dtype)))
        monkeypatch.setattr(_abi, "merge_ln_trainable", trainable)

    def public_merge(merge, x, size, norm, residual=None, log_size=False):
        seams.calls.append((FUNCTION, "merge", residual is not None))
        return x[:, 2:] * 1, x[:, 2:] * 1, torch.ones(x.shape[0], x.shape[1] - 2, 1)

    def public_drop(drop, x, norm, residual=None):
        seams.calls.append((FUNCTION, "drop", residual is not None))
        return x[:, 2:] * 1, x[:, 2:] * 1

    monkeypatch.setattr(M, "merge_wavg_ln", public_merge)
    monkeypatch.setattr(M, "drop_ln", public_drop)
    norm = norm_cls(base.C_).to(dtype).requires_grad_(who == "norm")
    merge_fn, drop_fn, hybrid_fn = base._reducers(seams, False)
    fn = C.pick_reduction(mode, merge_fn, drop_fn, hybrid_fn)
    info = base._info(mode, trace, 2)
    info["size"] = size
    x = torch.randn(2, 8, base.C_).to(dtype).requires_grad_(who == "x")
    res = torch.randn(2, 8, base.C_).to(dtype).requires_grad_(who == "residual")
    xo, y = C.merge_then_norm(None, x, info, norm, fn, merge_fn, residual=res, fold=base._fc2(dtype), drop_fn=drop_fn,
                              hybrid_fn=hybrid_fn)
    assert info["r"] == [2], "exactly one r is consumed"
    return seams, info, [c for c in seams.calls if c[0] in (MERGE_LN, DROP_LN, UNFUSED, FUNCTION)]


@pytest.mark.parametrize("row", TABLE, ids=_ids(TABLE))
def test_switch_route(row, monkeypatch):
    mode, who, dtype, switch, trace, want = row
    seams, info, got = _run(monkeypatch, row)
    assert len(got) == 1 and got[0][0] == want, got
    if want == FUNCTION:
        assert got[0][1] == ("drop" if mode in ("drop", "random_drop") else "merge")
        assert got[0][2] is True, "the residual goes into the launch as its addend"
        assert "_folded" not in info, "no bias is folded into the stream under grad"
        which = "drop" if mode in ("drop", "random_drop") else "merge"
        assert [c for c in seams.calls if c[0] == "match"] == [("match", which, 2, mode, None)]
        if which == "drop":
            assert tuple(info["size"].shape) == (2, 6, 1) and bool((info["size"] == 1).all())
    if who is not None and want != FUNCTION:
        assert "_folded" not in info


@pytest.mark.parametrize("row", [r for r in TABLE if r[5] == FUNCTION], ids=_ids([r for r in TABLE if r[5] == FUNCTION]))
def test_cpu_tensors_never_take_the_function(row, monkeypatch):
    """The real predicate: the same rows on CPU tensors run the three steps, switch on or not."""
    _, _, got = _run(monkeypatch, row, device_free_predicate=False)
    assert len(got) == 1 and got[0][0] == UNFUSED, got


def test_a_size_that_requires_grad_and_a_layernorm_subclass_keep_the_three_steps(monkeypatch):
    class Sub(torch.nn.LayerNorm):
        pass

    row = ("merge", "x", BF, True, False, UNFUSED)
    size = torch.ones(2, 8, 1, dtype=BF).requires_grad_(True)
    assert _run(monkeypatch, row, size=size)[2][0][0] == UNFUSED
    assert _run(monkeypatch, row, norm_cls=Sub)[2][0][0] == UNFUSED
    assert _run(monkeypatch, row)[2][0][0] == FUNCTION


def test_switch_is_off_by_default_and_the_entries_exist():
    from tome import _abi, _ln
    from tome import merge as M
    from tome.patch import _common as C
    assert C.TRAIN_FUSED_LN is False
    assert callable(M.merge_wavg_ln) and callable(M.drop_ln)
    assert "tome_merge_ln_backward" in _abi.SYMBOLS and "tome_merge_ln_backward_workspace_bytes" in _abi.SYMBOLS
    assert callable(_abi.merge_ln_backward) and callable(_abi.merge_ln_trainable)
    assert issubclass(_ln._MergeLnFunction, torch.autograd.Function)


def test_public_calls_answer_on_cpu_tensors_with_the_three_steps():
    """No plan, CPU tensors: `x + residual`, merge_wavg / drop, norm(x) -- with a gradient for everyone."""
    from tome import merge as M
    norm = torch.nn.LayerNorm(16)
    x, res = torch.randn(2, 8, 16, requires_grad=True), torch.randn(2, 8, 16, requires_grad=True)
    xo, y, size = M.merge_wavg_ln(M.do_nothing, x, None, norm, residual=res)
    assert torch.equal(xo, x + res) and torch.equal(y, norm(x + res)) and tuple(size.shape) == (2, 8, 1)
    assert type(xo.grad_fn).__name__ != "_MergeLnFunctionBackward"
    (xo.sum() + y.square().sum()).backward()
    assert torch.equal(x.grad, res.grad) and norm.weight.grad is not None
    xd, yd = M.drop_ln(M.do_nothing, x.detach(), norm)
    assert torch.equal(xd, x.detach()) and torch.equal(yd, norm(x.detach()))
