"""Which route the add + reduction + LayerNorm step takes under autocast, held to literal tables on the CPU:
`tome.merge._ln_route` (the public calls merge_wavg_ln / drop_ln) on stand-in tensors that say they live on the device,
and `merge_then_norm` (tome/patch/_common.py) with the launch seams of tests/test_modes_route_cpu.py plus recorders for the
two mixed-precision bindings.  Axes: autocast, stream / residual / parameter dtype, who wants a gradient, trace_source,
hybrid / partition plan, AUTOCAST_FUSED_LN, NATIVE_LN_AUTOCAST, TOME_FUSE_MODES (and TOME_FUSE_LN, TOME_FUSE_ADD).
Autocast off gives today's answer in every row; the attribute off leaves merge_then_norm on its present path.  And the
header declares both entries with the argument order the bindings use."""
import contextlib
import os
import re
import types

import pytest
import torch

import test_modes_route_cpu as base

BF, HF, F32 = base.BF, base.HF, base.F32
MERGE_LN, DROP_LN, UNFUSED = base.MERGE_LN, base.DROP_LN, base.UNFUSED
MERGE_AMP, DROP_AMP = "merge_wavg_ln_amp", "drop_ln_amp"
FUNCTION = "function"  # the public call, which takes _MergeLnFunction on a device
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUDA = torch.device("cuda", 0)


class T:
    """What _ln_route asks of a tensor, without a device behind it."""

    def __init__(self, dtype, requires_grad=False, shape=(2, 8, 16), device=CUDA):
        self.dtype, self.requires_grad, self.shape, self.device = dtype, requires_grad, torch.Size(shape), device
        self.is_cuda = device.type == "cuda"

    def dim(self):
        return len(self.shape)


def _norm(dtype, grad=False, cls=torch.nn.LayerNorm):
    return cls(16).to(dtype).requires_grad_(grad)


def _plan(kind):
    from tome import _abi
    if kind == "none":
        return None
    if kind == "partition":
        return object.__new__(_abi.PartitionPlan)
    plan = _abi.MatchPlan(2, 8, 2, False, False, None, None, None, None, None, CUDA)
    plan.edge_keep = "flags" if kind == "hybrid" else None
    return plan


# autocast dtype (None: off), x, residual (None: absent), parameters, who wants a gradient, plan, NATIVE_LN_AUTOCAST -> answer
ROUTE = [
    # autocast off: today's answers
    (None, BF, BF, BF, None, "even_odd", True, "direct"),
    (None, BF, None, BF, None, "hybrid", True, "direct"),
    (None, BF, BF, F32, None, "even_odd", True, None),
    (None, F32, BF, F32, None, "even_odd", True, None),
    (None, F32, F32, F32, None, "even_odd", True, None),
    (None, BF, HF, BF, None, "even_odd", True, None),
    (None, BF, BF, BF, "x", "even_odd", True, "function"),
    (None, BF, BF, BF, "x", "hybrid", True, None),
    (None, BF, BF, BF, None, "partition", True, None),
    (None, BF, BF, BF, None, "none", True, None),
    # autocast on, fp32 parameters, nobody wants a gradient: the mixed-precision launch for every legal dtype pair
    (BF, BF, BF, F32, None, "even_odd", True, "amp_direct"),
    (BF, BF, None, F32, None, "even_odd", True, "amp_direct"),
    (BF, F32, BF, F32, None, "even_odd", True, "amp_direct"),
    (BF, F32, F32, F32, None, "even_odd", True, "amp_direct"),
    (BF, F32, None, F32, None, "even_odd", True, "amp_direct"),
    (HF, HF, HF, F32, None, "even_odd", True, "amp_direct"),
    (HF, F32, HF, F32, None, "hybrid", True, "amp_direct"),
    (BF, BF, BF, F32, None, "hybrid", True, "amp_direct"),
    # ... not for the pairs the entry refuses
    (BF, BF, F32, F32, None, "even_odd", True, None),
    (BF, HF, HF, F32, None, "even_odd", True, None),
    (BF, F32, HF, F32, None, "even_odd", True, None),
    (HF, BF, BF, F32, None, "even_odd", True, None),
    # ... not with a gradient wanted, a partition plan, a foreign callable, or the switch off
    (BF, BF, BF, F32, "x", "even_odd", True, None),
    (BF, F32, BF, F32, "residual", "even_odd", True, None),
    (BF, F32, BF, F32, "norm", "even_odd", True, None),
    (BF, F32, BF, F32, "size", "even_odd", True, None),
    (BF, F32, BF, F32, None, "partition", True, None),
    (BF, F32, BF, F32, None, "none", True, None),
    (BF, BF, BF, F32, None, "even_odd", False, None),
    (BF, F32, BF, F32, None, "hybrid", False, None),
    # autocast on with 16-bit parameters (a model cast as a whole): the 16-bit launch keeps its place
    (BF, BF, BF, BF, None, "even_odd", True, "direct"),
    (BF, BF, BF, BF, None, "even_odd", False, "direct"),
    (BF, BF, BF, BF, "x", "even_odd", True, "function"),
]


def _route_ids():
    return ["-".join(str(v).replace("torch.", "") for v in row[:7]) for row in ROUTE]


@pytest.mark.parametrize("row", ROUTE, ids=_route_ids())
def test_ln_route(row, monkeypatch):
    autocast, xd, rd, pd, who, plan_kind, native, want = row
    from tome import _abi, _ln
    from tome import merge as M
    monkeypatch.setattr(_abi, "autocast_dtype", lambda device: autocast)
    monkeypatch.setattr(_ln, "NATIVE_LN_AUTOCAST", native)
    x = T(xd, who == "x")
    res = None if rd is None else T(rd, who == "residual")
    size = T(F32, who == "size", shape=(2, 8, 1))
    norm = _norm(pd, who == "norm")
    plan = _plan(plan_kind)
    merge = types.SimpleNamespace(plan=plan) if plan is not None else (lambda t, mode=None: t)
    assert M._ln_route(merge, x, norm, res, size) == want


def test_ln_route_other_refusals(monkeypatch):
    """A LayerNorm without bias or of another width, a residual of another shape or device, a plan of another device."""
    from tome import _abi
    from tome import merge as M
    monkeypatch.setattr(_abi, "autocast_dtype", lambda device: BF)
    merge = types.SimpleNamespace(plan=_plan("even_odd"))
    x, res = T(F32), T(BF)
    assert M._ln_route(merge, x, _norm(F32), res) == "amp_direct"
    assert M._ln_route(merge, x, torch.nn.LayerNorm(16, bias=False), res) is None
    assert M._ln_route(merge, x, torch.nn.LayerNorm(8), res) is None
    assert M._ln_route(merge, x, torch.nn.GroupNorm(1, 16), res) is None
    assert M._ln_route(merge, x, _norm(F32), T(BF, shape=(2, 7, 16))) is None
    assert M._ln_route(merge, x, _norm(F32), T(BF, device=torch.device("cpu"))) is None
    assert M._ln_route(merge, T(F32, device=torch.device("cuda", 1)), _norm(F32), None) is None
    assert M._ln_route(merge, T(F32, device=torch.device("cpu")), _norm(F32), None) is None
    assert M._ln_route(merge, T(F32, shape=(2, 8, 12)), torch.nn.LayerNorm(12), None) is None      # C % 8
    assert M._ln_route(merge, T(F32, shape=(2, 8, 1032)), torch.nn.LayerNorm(1032), None) is None  # C > 1024


WITH_PLAN = [r for r in ROUTE if r[5] in ("even_odd", "hybrid")]


@pytest.mark.parametrize("row", WITH_PLAN, ids=[i for i, r in zip(_route_ids(), ROUTE) if r in WITH_PLAN])
def test_one_rule_before_and_behind_the_matching(row, monkeypatch):
    """`_ln_route` asked without a matching (merge=None) answers as with one on the same tensors -- but for what only
    the plan can say: its threshold flags refuse the Function.  And the patched blocks' route (both switches on) gives the
    same "function" / "amp_direct" answers, with its kind standing in for the flags."""
    autocast, xd, rd, pd, who, plan_kind, native, want = row
    from tome import _abi, _ln
    from tome import merge as M
    from tome.patch import _common as C
    monkeypatch.setattr(_abi, "autocast_dtype", lambda device: autocast)
    monkeypatch.setattr(_ln, "NATIVE_LN_AUTOCAST", native)
    monkeypatch.setattr(C, "TRAIN_FUSED_LN", True)
    monkeypatch.setattr(C, "AUTOCAST_FUSED_LN", True)
    x = T(xd, who == "x")
    res = None if rd is None else T(rd, who == "residual")
    size = T(F32, who == "size", shape=(2, 8, 1))
    norm = _norm(pd, who == "norm")
    behind = M._ln_route(types.SimpleNamespace(plan=_plan(plan_kind)), x, norm, res, size)
    before = M._ln_route(None, x, norm, res, size)
    assert behind == want
    if plan_kind == "hybrid" and before == "function":
        assert behind is None
    else:
        assert before == behind
    mode = "hybrid" if plan_kind == "hybrid" else "merge"
    info = base._info(mode, False, 2)
    info["size"] = size
    got = C.fused_route(mode, x, norm, res, info)
    switched = ("function", "amp_direct")
    assert (got if got in switched else None) == (behind if behind in switched else None)


# ---------------------------------------------------------------------------------------------------------------------
# merge_then_norm
# ---------------------------------------------------------------------------------------------------------------------
# mode, autocast, stream, residual, parameters, who wants grad, trace, AUTOCAST_FUSED_LN, NATIVE_LN_AUTOCAST, FUSE_MODES,
# FUSE_LN, FUSE_ADD -> launch, residual fused as addend
BLOCK = [
    # the attribute off: the present path, under autocast and without
    ("merge", True, BF, BF, F32, None, False, False, True, True, True, True, UNFUSED, False),
    ("merge", True, F32, BF, F32, None, False, False, True, True, True, True, UNFUSED, False),
    ("drop", True, F32, BF, F32, None, False, False, True, True, True, True, UNFUSED, False),
    ("hybrid", True, BF, BF, F32, None, False, False, True, True, True, True, UNFUSED, False),
    ("merge", False, BF, BF, BF, None, False, False, True, True, True, True, MERGE_LN, True),
    ("drop", False, BF, BF, BF, None, False, False, True, True, True, True, DROP_LN, True),
    ("merge", False, F32, F32, F32, None, False, False, True, True, True, True, UNFUSED, False),
    # the attribute on, autocast off: nothing changes
    ("merge", False, BF, BF, BF, None, False, True, True, True, True, True, MERGE_LN, True),
    ("hybrid", False, BF, BF, BF, None, False, True, True, True, True, True, MERGE_LN, True),
    ("drop", False, HF, HF, HF, None, False, True, True, True, True, True, DROP_LN, True),
    ("merge", False, F32, F32, F32, None, False, True, True, True, True, True, UNFUSED, False),
    ("merge", False, BF, BF, F32, None, False, True, True, True, True, True, UNFUSED, False),
    # the attribute on under autocast: the new launch, for both streams and the three kinds
    ("merge", True, BF, BF, F32, None, False, True, True, True, True, True, MERGE_AMP, True),
    ("merge", True, F32, BF, F32, None, False, True, True, True, True, True, MERGE_AMP, True),
    ("merge", True, F32, F32, F32, None, False, True, True, True, True, True, MERGE_AMP, True),
    ("random_merge", True, F32, BF, F32, None, False, True, True, True, True, True, MERGE_AMP, True),
    ("hybrid", True, BF, BF, F32, None, False, True, True, True, True, True, MERGE_AMP, True),
    ("hybrid", True, F32, BF, F32, None, False, True, True, True, True, True, MERGE_AMP, True),
    ("drop", True, BF, BF, F32, None, False, True, True, True, True, True, DROP_AMP, True),
    ("drop", True, F32, BF, F32, None, False, True, True, True, True, True, DROP_AMP, True),
    ("random_drop", True, F32, BF, F32, None, False, True, True, True, True, True, DROP_AMP, True),
    # ... with TOME_FUSE_ADD off the add stays the framework's and the launch takes the sum
    ("merge", True, F32, BF, F32, None, False, True, True, True, True, False, MERGE_AMP, False),
    ("drop", True, BF, BF, F32, None, False, True, True, True, True, False, DROP_AMP, False),
    # ... and it yields: a gradient wanted, trace_source, NATIVE_LN_AUTOCAST, TOME_FUSE_LN, TOME_FUSE_MODES, a dtype pair
    # the entry refuses
    ("merge", True, F32, BF, F32, "x", False, True, True, True, True, True, UNFUSED, False),
    ("merge", True, F32, BF, F32, "residual", False, True, True, True, True, True, UNFUSED, False),
    ("drop", True, BF, BF, F32, "norm", False, True, True, True, True, True, UNFUSED, False),
    ("merge", True, F32, BF, F32, None, True, True, True, True, True, True, UNFUSED, False),
    ("hybrid", True, BF, BF, F32, None, True, True, True, True, True, True, UNFUSED, False),
    ("merge", True, F32, BF, F32, None, False, True, False, True, True, True, UNFUSED, False),
    ("drop", True, BF, BF, F32, None, False, True, False, True, True, True, UNFUSED, False),
    ("merge", True, F32, BF, F32, None, False, True, True, True, False, True, UNFUSED, False),
    ("merge", True, F32, BF, F32, None, False, True, True, False, True, True, MERGE_AMP, True),
    ("random_merge", True, F32, BF, F32, None, False, True, True, False, True, True, UNFUSED, False),
    ("hybrid", True, F32, BF, F32, None, False, True, True, False, True, True, UNFUSED, False),
    ("drop", True, F32, BF, F32, None, False, True, True, False, True, True, UNFUSED, False),
    ("merge", True, BF, F32, F32, None, False, True, True, True, True, True, UNFUSED, False),
    ("merge", True, HF, HF, F32, None, False, True, True, True, True, True, UNFUSED, False),
    # 16-bit parameters under autocast: the 16-bit launch, attribute or not
    ("merge", True, BF, BF, BF, None, False, True, True, True, True, True, MERGE_LN, True),
]


def _block_ids():
    return ["-".join(str(v).replace("torch.", "") for v in row[:12]) for row in BLOCK]


def _train_seams(monkeypatch, seams, C):
    """TRAIN_FUSED_LN on, with the Function route's seams of tests/test_merge_ln_route_cpu.py: the device-free copy of
    `_abi.merge_ln_trainable` and recorders in place of the two public calls."""
    from tome import _abi
    from tome import merge as M
    monkeypatch.setattr(C, "TRAIN_FUSED_LN", True)

    def trainable(x, norm, addend, merge=None):
        return (x.dim() == 3 and _abi.ln_trainable(x, norm)
                and (addend is None or (addend.shape == x.shape and addend.dtype == x.dtype)))

    def public_merge(merge, x, size, norm, residual=None, log_size=False):
        seams.calls.append((FUNCTION, "merge", residual is not None))
        return x[:, 2:] * 1, x[:, 2:] * 1, torch.ones(x.shape[0], x.shape[1] - 2, 1)

    def public_drop(drop, x, norm, residual=None):
        seams.calls.append((FUNCTION, "drop", residual is not None))
        return x[:, 2:] * 1, x[:, 2:] * 1

    monkeypatch.setattr(_abi, "merge_ln_trainable", trainable)
    monkeypatch.setattr(M, "merge_wavg_ln", public_merge)
    monkeypatch.setattr(M, "drop_ln", public_drop)


def _run_block(monkeypatch, row, train=False):
    mode, autocast, xd, rd, pd, who, trace, attr, native, fuse_modes, fuse_ln, fuse_add = row[:12]
    from tome import _abi, _ln
    seams, C, _ = base._setup(monkeypatch, (mode, False, xd, autocast, trace, fuse_ln, fuse_add, fuse_modes, False))
    monkeypatch.setattr(C, "AUTOCAST_FUSED_LN", attr)
    monkeypatch.setattr(_ln, "NATIVE_LN_AUTOCAST", native)
    if train:
        _train_seams(monkeypatch, seams, C)

    def ln_amp_fusable(x, norm, *others):  # _abi.ln_amp_fusable without `x.is_cuda`
        return (isinstance(norm, torch.nn.LayerNorm) and _abi._ln_amp_of(x, norm, others[0] if others else None)
                and not (torch.is_grad_enabled() and _abi.needs_grad(x, norm.weight, norm.bias, *others)))

    monkeypatch.setattr(_abi, "ln_amp_fusable", ln_amp_fusable)

    def merge_wavg_ln_amp(plan, x, size, w, b, eps, y_dtype, addend=None, log_size=False):
        seams.calls.append((MERGE_AMP, addend is not None, y_dtype, x.dtype, None if addend is None else addend.dtype))
        return x[:, 2:].clone(), x[:, 2:].to(y_dtype), torch.ones(x.shape[0], x.shape[1] - 2, 1)

    def drop_ln_amp(plan, x, w, b, eps, y_dtype, addend=None):
        seams.calls.append((DROP_AMP, addend is not None, y_dtype, x.dtype, None if addend is None else addend.dtype))
        return x[:, 2:].clone(), x[:, 2:].to(y_dtype)

    monkeypatch.setattr(_abi, "merge_wavg_ln_amp", merge_wavg_ln_amp)
    monkeypatch.setattr(_abi, "drop_ln_amp", drop_ln_amp)
    norm = torch.nn.LayerNorm(base.C_).to(pd).requires_grad_(who == "norm")
    merge_fn, drop_fn, hybrid_fn = base._reducers(seams, False)
    fn = C.pick_reduction(mode, merge_fn, drop_fn, hybrid_fn)
    info = base._info(mode, trace, 2)
    x = torch.randn(2, 8, base.C_).to(xd).requires_grad_(who == "x")
    res = torch.randn(2, 8, base.C_).to(rd).requires_grad_(who == "residual")
    # (autocast is stood in for by the patched predicate, so the framework's own layer_norm would see mixed dtypes)
    monkeypatch.setattr(torch.nn.LayerNorm, "forward", lambda self, t: t.clone())
    with torch.set_grad_enabled(who is not None):
        xo, y = C.merge_then_norm(None, x, info, norm, fn, merge_fn, residual=res, fold=base._fc2(xd), drop_fn=drop_fn,
                                  hybrid_fn=hybrid_fn)
    assert info["r"] == [2], "exactly one r is consumed"
    return seams, info, xo, y, [c for c in seams.calls if c[0] in (MERGE_LN, DROP_LN, UNFUSED, MERGE_AMP, DROP_AMP, FUNCTION)]


@pytest.mark.parametrize("row", BLOCK, ids=_block_ids())
def test_merge_then_norm_route(row, monkeypatch):
    mode, autocast, xd, rd = row[:4]
    want, want_add = row[12:]
    seams, info, xo, y, got = _run_block(monkeypatch, row)
    assert len(got) == 1 and got[0][0] == want, got
    if want in (MERGE_AMP, DROP_AMP):
        _, added, y_dtype, x_dtype, a_dtype = got[0]
        assert added is want_add and y_dtype == BF and y.dtype == BF
        # the stream the launch is given: x itself with the residual beside it, or the framework's sum
        assert x_dtype == (xd if want_add else torch.promote_types(xd, rd)) and a_dtype == (rd if want_add else None)
        assert "_folded" not in info, "no bias is folded into the stream under autocast"
        which = {"random_merge": "merge", "random_drop": "drop"}.get(mode, mode)
        assert [c[:2] for c in seams.calls if c[0] == "match"] == [("match", which)]
        assert not [c for c in seams.calls if c[0] == "trailing_ln_kernel"], "the launch holds the LayerNorm"
        if which == "drop":
            assert tuple(info["size"].shape) == (2, 6, 1) and bool((info["size"] == 1).all())
    elif want in (MERGE_LN, DROP_LN):
        assert got[0][1] is want_add


@pytest.mark.parametrize("row", [r for r in BLOCK if not r[7]], ids=[i for i, r in zip(_block_ids(), BLOCK) if not r[7]])
def test_attribute_off_is_the_present_path(row, monkeypatch):
    """The rows with the attribute off once more: neither mixed-precision binding is called, and under autocast the
    trailing LayerNorm is the mixed-precision add + LayerNorm kernel as before."""
    seams, info, xo, y, got = _run_block(monkeypatch, row)
    assert not [c for c in got if c[0] in (MERGE_AMP, DROP_AMP)]
    if row[1]:
        assert [c for c in seams.calls if c[0] == "trailing_ln_kernel"] == [("trailing_ln_kernel", "amp_direct")]


# TRAIN_FUSED_LN and AUTOCAST_FUSED_LN on together: the Function first, then the mixed-precision launch, then the 16-bit one
# mode, autocast, stream, residual, parameters, who wants grad, trace, FUSE_ADD -> launch, residual fused as addend
PRECEDENCE = [
    # no-grad without autocast: the 16-bit launch
    ("merge", False, BF, BF, BF, None, False, True, MERGE_LN, True),
    ("hybrid", False, BF, BF, BF, None, False, True, MERGE_LN, True),
    ("drop", False, HF, HF, HF, None, False, True, DROP_LN, True),
    # no-grad under autocast with an fp32 norm: the mixed-precision launch
    ("merge", True, F32, BF, F32, None, False, True, MERGE_AMP, True),
    ("hybrid", True, BF, BF, F32, None, False, True, MERGE_AMP, True),
    ("drop", True, BF, BF, F32, None, False, True, DROP_AMP, True),
    # grad without autocast, kinds merge and drop: the Function; hybrid: three steps
    ("merge", False, BF, BF, BF, "x", False, True, FUNCTION, True),
    ("random_merge", False, BF, BF, BF, "residual", False, True, FUNCTION, True),
    ("drop", False, BF, BF, BF, "norm", False, True, FUNCTION, True),
    ("hybrid", False, BF, BF, BF, "x", False, True, UNFUSED, False),
    # grad under autocast with an fp32 norm: three steps, then the trailing mixed-precision LayerNorm
    ("merge", True, F32, BF, F32, "x", False, True, UNFUSED, False),
    ("drop", True, BF, BF, F32, "x", False, True, UNFUSED, False),
    # trace_source: the 16-bit launch in no-grad (the add stays the framework's), three steps under grad
    ("merge", False, BF, BF, BF, None, True, True, MERGE_LN, False),
    ("drop", False, BF, BF, BF, None, True, True, DROP_LN, False),
    ("merge", False, BF, BF, BF, "x", True, True, UNFUSED, False),
    ("merge", True, F32, BF, F32, None, True, True, UNFUSED, False),
    # TOME_FUSE_ADD off under autocast: the framework's add, then the mixed-precision launch without addend
    ("merge", True, F32, BF, F32, None, False, False, MERGE_AMP, False),
    ("drop", True, BF, BF, F32, None, False, False, DROP_AMP, False),
]


@pytest.mark.parametrize("row", PRECEDENCE, ids=["-".join(str(v).replace("torch.", "") for v in r[:8]) for r in PRECEDENCE])
def test_both_switches_on_precedence(row, monkeypatch):
    mode, autocast, xd, rd, pd, who, trace, fuse_add, want, want_add = row
    seams, info, xo, y, got = _run_block(
        monkeypatch, (mode, autocast, xd, rd, pd, who, trace, True, True, True, True, fuse_add), train=True)
    assert len(got) == 1 and got[0][0] == want, got
    trailing = [c for c in seams.calls if c[0] == "trailing_ln_kernel"]
    if want == UNFUSED:
        if autocast:
            assert trailing == [("trailing_ln_kernel", "amp_function" if who else "amp_direct")]
    else:
        assert not trailing, "the launch holds the LayerNorm"
        which = "drop" if mode in ("drop", "random_drop") else "hybrid" if mode == "hybrid" else "merge"
        assert [c[:2] for c in seams.calls if c[0] == "match"] == [("match", which)]
        tracked = [c[0] for c in seams.calls if c[0].endswith("_source")]
        assert tracked == ([] if not trace else ["drop_source" if which == "drop" else "merge_source"])
    if want == FUNCTION:
        assert got[0][1:] == ("drop" if mode in ("drop", "random_drop") else "merge", True), got
        assert "_folded" not in info
    elif want in (MERGE_AMP, DROP_AMP):
        _, added, y_dtype, x_dtype, a_dtype = got[0]
        assert added is want_add and y_dtype == BF
        assert x_dtype == (xd if want_add else torch.promote_types(xd, rd)) and a_dtype == (rd if want_add else None)
        assert "_folded" not in info
    elif want in (MERGE_LN, DROP_LN):
        assert got[0][1] is want_add
        assert got[0][2] is (mode == "merge") and ("_folded" in info) is (mode == "merge"), got


def test_the_attribute_is_off_by_default_and_the_entries_exist():
    from tome import _abi
    from tome import merge as M
    from tome.patch import _common as C
    assert C.AUTOCAST_FUSED_LN is False
    assert "tome_merge_wavg_ln_amp" in _abi.SYMBOLS and "tome_drop_ln_amp" in _abi.SYMBOLS
    assert _abi.SIGNATURES["tome_merge_wavg_ln_amp"][2] and _abi.SIGNATURES["tome_drop_ln_amp"][2]  # additions to v11
    assert callable(_abi.merge_wavg_ln_amp) and callable(_abi.drop_ln_amp) and callable(_abi.ln_amp_fusable)
    assert "amp_direct" in M._ln_route.__doc__ and "tome_merge_wavg_ln_amp" in M.merge_wavg_ln.__doc__
    assert "tome_drop_ln_amp" in M.drop_ln.__doc__
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "AUTOCAST_FUSED_LN" in readme and "tome_merge_wavg_ln_amp" in readme


# ---------------------------------------------------------------------------------------------------------------------
# the header and the bindings' argument order
# ---------------------------------------------------------------------------------------------------------------------
def _header_params(name):
    text = open(os.path.join(ROOT, "include", "tome_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m is not None, f"{name} is not declared in include/tome_hip.h"
    return [re.split(r"[\s\*]+", p.strip())[-1] for p in m.group(1).split(",")]


def _recorded_call(monkeypatch, which, x_dtype, a_dtype, size):
    """The positional arguments a binding hands the library for CPU tensors, with the device checks stood down."""
    from tome import _abi
    seen = {}

    def entry(*args):
        seen["args"] = args
        return 0

    monkeypatch.setattr(_abi, "lib", lambda: types.SimpleNamespace())
    monkeypatch.setattr(_abi, "require_symbol", lambda L, name: seen.setdefault("name", name) and entry)
    monkeypatch.setattr(_abi, "require_device", lambda t, what: None)
    monkeypatch.setattr(_abi, "_stream", lambda device: 4242)
    monkeypatch.setattr(_abi, "_on_device", lambda device: contextlib.nullcontext())
    cpu = torch.device("cpu")
    idx = [torch.zeros((2, k, 1), dtype=torch.int64) for k in (2, 2, 2)]
    plan = _abi.MatchPlan(2, 8, 2, False, True, idx[0], idx[1], idx[2], None, None, cpu)
    plan.edge_keep = torch.ones((2, 2), dtype=torch.uint8)
    t = {"x": torch.zeros((2, 8, 16), dtype=x_dtype), "addend": torch.zeros((2, 8, 16), dtype=a_dtype),
         "weight_f32": torch.ones(16), "bias_f32": torch.zeros(16), "size": size}
    if which == "merge":
        out = _abi.merge_wavg_ln_amp(plan, t["x"], size, t["weight_f32"], t["bias_f32"], 1e-5, torch.float16,
                                     addend=t["addend"], log_size=True)
    else:
        out = _abi.drop_ln_amp(plan, t["x"], t["weight_f32"], t["bias_f32"], 1e-5, torch.float16, addend=t["addend"])
    return seen, plan, t, out


@pytest.mark.parametrize("which", ["merge", "drop"])
def test_binding_argument_order_is_the_headers(which, monkeypatch):
    from tome import _abi
    name = "tome_merge_wavg_ln_amp" if which == "merge" else "tome_drop_ln_amp"
    params = _header_params(name)
    assert len(params) == len(_abi.SIGNATURES[name][1])
    size = torch.ones((2, 8, 1), dtype=torch.float32) if which == "merge" else None
    seen, plan, t, out = _recorded_call(monkeypatch, which, torch.float32, torch.float16, size)
    assert seen["name"] == name and len(seen["args"]) == len(params)
    got = dict(zip(params, seen["args"]))
    code = _abi.DTYPES
    want = {"x": t["x"].data_ptr(), "x_dtype": code[torch.float32], "addend": t["addend"].data_ptr(),
            "addend_dtype": code[torch.float16], "n": 2, "T": 8, "C": 16, "r": 2, "distill_token": 1,
            "weight_f32": t["weight_f32"].data_ptr(), "bias_f32": t["bias_f32"].data_ptr(), "x_out": out[0].data_ptr(),
            "y_out": out[1].data_ptr(), "y_dtype": code[torch.float16], "stream": 4242}
    if which == "merge":
        want.update({"size": size.data_ptr(), "size_dtype": code[torch.float32], "src_idx": plan.src_idx.data_ptr(),
                     "dst_idx": plan.dst_idx.data_ptr(), "unm_idx": plan.unm_idx.data_ptr(),
                     "edge_keep": plan.edge_keep.data_ptr(), "size_out": out[2].data_ptr(),
                     "log_size_out": out[2]._tome_log.data_ptr()})
    else:
        want["und_idx"] = plan.unm_idx.data_ptr()
    assert set(want) | {"eps"} == set(params), sorted(set(params) ^ (set(want) | {"eps"}))
    for key, value in want.items():
        assert got[key] == value, (key, got[key], value)
    assert abs(got["eps"] - 1e-5) < 1e-12
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.float16 and tuple(out[1].shape) == (2, 6, 16)


def test_refusals_are_made_on_the_host_before_any_launch():
    """The entries' own checks need no device: with host buffers (never dereferenced) every illegal call comes back with
    TOME_EINVAL and a text of its own.  (tests/test_merge_ln_amp_gpu.py repeats them on the device and shows that
    nothing was written.)"""
    from tome import _abi
    L = _abi.lib()
    code = _abi.DTYPES
    n, T, r = 2, 8, 2
    idx = torch.zeros((n, r), dtype=torch.int64)
    w = torch.ones(1032, dtype=torch.float32)

    def merge(x, a, y, C, so_dtype=torch.float32, weight=w):
        xo, so = torch.empty_like(x[:, : T - r]), torch.empty((n, T - r, 1), dtype=so_dtype)
        return L.tome_merge_wavg_ln_amp(x.data_ptr(), code[x.dtype], _abi._ptr(a), 0 if a is None else code[a.dtype], None,
                                        code[so_dtype], n, T, C, r, idx.data_ptr(), idx.data_ptr(), idx.data_ptr(), 0, None,
                                        weight.data_ptr(), w.data_ptr(), 1e-6, xo.data_ptr(), y.data_ptr(), code[y.dtype],
                                        so.data_ptr(), None, None)

    def drop(x, a, y, C):
        xo = torch.empty_like(x[:, : T - r])
        return L.tome_drop_ln_amp(x.data_ptr(), code[x.dtype], _abi._ptr(a), 0 if a is None else code[a.dtype], n, T, C, r,
                                  idx.data_ptr(), 0, w.data_ptr(), w.data_ptr(), 1e-6, xo.data_ptr(), y.data_ptr(),
                                  code[y.dtype], None)

    def mk(dtype, C=64):
        return torch.zeros((n, T, C), dtype=dtype)

    for call, name in ((merge, b"tome_merge_wavg_ln_amp"), (drop, b"tome_drop_ln_amp")):
        for xd, ad, yd in ((BF, HF, BF), (BF, F32, BF), (F32, BF, HF), (F32, None, F32), (BF, None, HF)):
            assert call(mk(xd), None if ad is None else mk(ad), mk(yd), 64) != 0
            assert name in L.tome_last_error() and b"unsupported dtypes" in L.tome_last_error()
        assert call(mk(F32, 12), None, mk(BF, 12), 12) != 0 and b"C=12 must be a multiple of 8" in L.tome_last_error()
        assert call(mk(F32, 1032), None, mk(BF, 1032), 1032) != 0 and b"C=1032" in L.tome_last_error()
        off = torch.zeros(n * T * 64 + 8, dtype=BF)[4:4 + n * T * 64].view(n, T, 64)
        assert off.data_ptr() % 16 == 8
        assert call(off, None, mk(BF), 64) != 0 and b"x / x_out not 16-byte aligned" in L.tome_last_error()
        assert call(mk(BF), off, mk(BF), 64) != 0 and b"addend not 16-byte aligned" in L.tome_last_error()
    assert merge(mk(BF), None, mk(BF), 64, so_dtype=HF) != 0 and b"sizes must be of x's dtype or fp32" in L.tome_last_error()
    assert merge(mk(BF), None, mk(BF), 64, weight=w[2:]) != 0 and b"weight_f32 / bias_f32 not 16-byte" in L.tome_last_error()
