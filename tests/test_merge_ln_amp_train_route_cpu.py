"""Which route the add + reduction + LayerNorm step takes under autocast WITH a gradient wanted, held to literal tables
on the CPU: `tome.merge._ln_route` on the stand-in tensors of tests/test_merge_ln_amp_route_cpu.py, and `merge_then_norm`
(tome/patch/_common.py) with that file's launch seams plus recorders for the two public calls and for fused_route's
answer.  Axes: tome._ln.NATIVE_MERGE_LN_AUTOCAST_BACKWARD off and on, autocast, stream / residual / parameter dtype, who
wants a gradient, hybrid / partition / no plan, trace_source, NATIVE_LN_AUTOCAST, tome.merge.NATIVE_BACKWARD (and
NATIVE_LN_BACKWARD, TRAIN_FUSED_LN, AUTOCAST_FUSED_LN).  With the switch off every row gives the answer it gave before the
switch existed.  And the header declares the entry with the argument order the binding uses, and the entry's refusals are
made on the host."""
import contextlib
import types

import pytest
import torch

import test_merge_ln_amp_route_cpu as amp
import test_modes_route_cpu as base

BF, HF, F32 = base.BF, base.HF, base.F32
UNFUSED, FUNCTION = base.UNFUSED, amp.FUNCTION
AMP_FN = "amp_function"

# autocast dtype (None: off), x, residual (None: absent), parameters, who wants a gradient, plan, NATIVE_LN_AUTOCAST,
# merge.NATIVE_BACKWARD -> answer with the switch off (the answer before it existed), answer with it on
ROUTE = [
    # a gradient wanted under autocast with fp32 parameters: every legal dtype pair, whoever wants it
    (BF, BF, BF, F32, "x", "even_odd", True, True, None, AMP_FN),
    (BF, BF, None, F32, "x", "even_odd", True, True, None, AMP_FN),
    (BF, F32, BF, F32, "x", "even_odd", True, True, None, AMP_FN),
    (BF, F32, BF, F32, "residual", "even_odd", True, True, None, AMP_FN),
    (BF, F32, BF, F32, "norm", "even_odd", True, True, None, AMP_FN),
    (BF, F32, F32, F32, "residual", "even_odd", True, True, None, AMP_FN),
    (BF, F32, None, F32, "norm", "even_odd", True, True, None, AMP_FN),
    (HF, HF, HF, F32, "x", "even_odd", True, True, None, AMP_FN),
    (HF, F32, HF, F32, "residual", "even_odd", True, True, None, AMP_FN),
    # ... not when the sizes want one, for a hybrid or partition plan or a foreign callable, for a pair the entries
    # refuse, or with either of the switches it stands on off
    (BF, F32, BF, F32, "size", "even_odd", True, True, None, None),
    (BF, F32, BF, F32, "x", "hybrid", True, True, None, None),
    (BF, BF, BF, F32, "x", "partition", True, True, None, None),
    (BF, BF, BF, F32, "x", "none", True, True, None, None),
    (BF, BF, F32, F32, "x", "even_odd", True, True, None, None),
    (BF, HF, HF, F32, "x", "even_odd", True, True, None, None),
    (BF, F32, HF, F32, "residual", "even_odd", True, True, None, None),
    (HF, BF, BF, F32, "norm", "even_odd", True, True, None, None),
    (BF, F32, BF, F32, "x", "even_odd", False, True, None, None),
    (BF, F32, BF, F32, "x", "even_odd", True, False, None, None),
    # nobody wants a gradient: the launch itself, hybrid included, whatever the switch says
    (BF, BF, BF, F32, None, "even_odd", True, True, "amp_direct", "amp_direct"),
    (BF, F32, BF, F32, None, "hybrid", True, True, "amp_direct", "amp_direct"),
    (BF, F32, BF, F32, None, "even_odd", True, False, "amp_direct", "amp_direct"),
    (BF, F32, BF, F32, None, "even_odd", False, True, None, None),
    # autocast off, and 16-bit parameters under autocast: the 16-bit answers keep their place
    (None, BF, BF, BF, "x", "even_odd", True, True, "function", "function"),
    (None, BF, BF, BF, "x", "even_odd", True, False, None, None),
    (None, BF, BF, BF, None, "even_odd", True, True, "direct", "direct"),
    (None, F32, BF, F32, "x", "even_odd", True, True, None, None),
    (None, BF, BF, F32, "x", "even_odd", True, True, None, None),
    (BF, BF, BF, BF, "x", "even_odd", True, True, "function", "function"),
    (BF, BF, BF, BF, "x", "hybrid", True, True, None, None),
    (BF, BF, BF, BF, None, "even_odd", True, True, "direct", "direct"),
]


def _ids(table, k):
    return ["-".join(str(v).replace("torch.", "") for v in row[:k]) for row in table]


def _ask(monkeypatch, row, switch, without_matching=False):
    autocast, xd, rd, pd, who, plan_kind, native, merge_native = row[:8]
    from tome import _abi, _ln
    from tome import merge as M
    monkeypatch.setattr(_abi, "autocast_dtype", lambda device: autocast)
    monkeypatch.setattr(_ln, "NATIVE_LN_AUTOCAST", native)
    monkeypatch.setattr(M, "NATIVE_BACKWARD", merge_native)
    monkeypatch.setattr(_ln, "NATIVE_MERGE_LN_AUTOCAST_BACKWARD", switch)
    x = amp.T(xd, who == "x")
    res = None if rd is None else amp.T(rd, who == "residual")
    size = amp.T(F32, who == "size", shape=(2, 8, 1))
    norm = amp._norm(pd, who == "norm")
    plan = amp._plan(plan_kind)
    merge = types.SimpleNamespace(plan=plan) if plan is not None else (lambda t, mode=None: t)
    return M._ln_route(None if without_matching else merge, x, norm, res, size)


@pytest.mark.parametrize("switch", [False, True], ids=["off", "on"])
@pytest.mark.parametrize("row", ROUTE, ids=_ids(ROUTE, 8))
def test_ln_route(row, switch, monkeypatch):
    assert _ask(monkeypatch, row, switch) == row[9 if switch else 8]


@pytest.mark.parametrize("row", amp.ROUTE, ids=amp._route_ids())
def test_the_existing_table_with_the_switch_off_and_on(row, monkeypatch):
    """tests/test_merge_ln_amp_route_cpu.py's own rows: the switch off gives each its answer; on, an answer moves only
    where that table says "three steps" for a gradient wanted under autocast on tensors the Function takes."""
    wide = row[:6] + (row[6], True)
    assert _ask(monkeypatch, wide, False) == row[7]
    got = _ask(monkeypatch, wide, True)
    moved = (row[0] is not None and row[4] in ("x", "residual", "norm") and row[5] == "even_odd" and row[6]
             and row[3] == F32 and row[7] is None)
    assert got == (AMP_FN if moved else row[7])


def test_ln_route_other_refusals(monkeypatch):
    """With the switch on and a gradient wanted: a LayerNorm subclass, one without bias or of another width, a residual of
    another shape or device, a plan of another device or with r = 0, tokens off the device, NATIVE_LN_BACKWARD off."""
    from tome import _abi, _ln
    from tome import merge as M
    monkeypatch.setattr(_abi, "autocast_dtype", lambda device: BF)
    monkeypatch.setattr(_ln, "NATIVE_MERGE_LN_AUTOCAST_BACKWARD", True)

    class Sub(torch.nn.LayerNorm):
        pass

    merge = types.SimpleNamespace(plan=amp._plan("even_odd"))
    x, res = amp.T(F32, True), amp.T(BF)
    assert M._ln_route(merge, x, amp._norm(F32), res) == AMP_FN
    assert M._ln_route(merge, x, amp._norm(F32, cls=Sub), res) is None
    assert M._ln_route(merge, x, torch.nn.LayerNorm(16, bias=False), res) is None
    assert M._ln_route(merge, x, torch.nn.LayerNorm(8), res) is None
    assert M._ln_route(merge, x, amp._norm(F32), amp.T(BF, shape=(2, 7, 16))) is None
    assert M._ln_route(merge, x, amp._norm(F32), amp.T(BF, device=torch.device("cpu"))) is None
    assert M._ln_route(merge, amp.T(F32, True, device=torch.device("cuda", 1)), amp._norm(F32), None) is None
    assert M._ln_route(merge, amp.T(F32, True, device=torch.device("cpu")), amp._norm(F32), None) is None
    assert M._ln_route(merge, amp.T(F32, True, shape=(2, 8, 12)), torch.nn.LayerNorm(12), None) is None      # C % 8
    assert M._ln_route(merge, amp.T(F32, True, shape=(2, 8, 1032)), torch.nn.LayerNorm(1032), None) is None  # C > 1024
    zero = amp._plan("even_odd")
    zero.r = 0
    assert M._ln_route(types.SimpleNamespace(plan=zero), x, amp._norm(F32), res) is None
    with torch.no_grad():
        assert M._ln_route(merge, x, amp._norm(F32), res) == "amp_direct"
    monkeypatch.setattr(_ln, "NATIVE_LN_BACKWARD", False)
    assert M._ln_route(merge, x, amp._norm(F32), res) is None


@pytest.mark.parametrize("row", [r for r in ROUTE if r[5] in ("even_odd", "hybrid")],
                         ids=[i for i, r in zip(_ids(ROUTE, 8), ROUTE) if r[5] in ("even_odd", "hybrid")])
def test_one_rule_before_and_behind_the_matching(row, monkeypatch):
    """`_ln_route` asked without a matching answers as with one on the same tensors -- but for what only the plan can say
    (its threshold flags refuse both Functions) -- and the patched blocks' route gives the same "amp_function" answers,
    with its kind standing in for the flags, whatever its own two switches say."""
    from tome.patch import _common as C
    who, plan_kind = row[4], row[5]
    behind = _ask(monkeypatch, row, True)
    before = _ask(monkeypatch, row, True, without_matching=True)
    assert behind == row[9]
    if plan_kind == "hybrid" and before in ("function", AMP_FN):
        assert behind is None
    else:
        assert before == behind
    mode = "hybrid" if plan_kind == "hybrid" else "merge"
    for train, direct in ((False, False), (True, True)):
        monkeypatch.setattr(C, "TRAIN_FUSED_LN", train)
        monkeypatch.setattr(C, "AUTOCAST_FUSED_LN", direct)
        info = base._info(mode, False, 2)
        x = amp.T(row[1], who == "x")
        res = None if row[2] is None else amp.T(row[2], who == "residual")
        info["size"] = amp.T(F32, who == "size", shape=(2, 8, 1))
        got = C.fused_route(mode, x, amp._norm(row[3], who == "norm"), res, info)
        assert (got == AMP_FN) == (behind == AMP_FN), (train, got, behind)


# ---------------------------------------------------------------------------------------------------------------------
# merge_then_norm
# ---------------------------------------------------------------------------------------------------------------------
MERGE_AMP, DROP_AMP, MERGE_LN = amp.MERGE_AMP, amp.DROP_AMP, base.MERGE_LN
# mode, autocast, stream, residual, parameters, who wants grad, trace, NATIVE_LN_AUTOCAST, merge.NATIVE_BACKWARD,
# TRAIN_FUSED_LN, FUSE_ADD -> launch with the switch off, launch with it on (FUNCTION: a public call of tome.merge)
BLOCK = [
    # a gradient wanted under autocast: the Function for the kinds merge and drop, whatever TRAIN_FUSED_LN / TOME_FUSE_ADD say
    ("merge", True, BF, BF, F32, "x", False, True, True, False, True, UNFUSED, AMP_FN),
    ("merge", True, F32, BF, F32, "x", False, True, True, False, True, UNFUSED, AMP_FN),
    ("merge", True, F32, BF, F32, "residual", False, True, True, True, True, UNFUSED, AMP_FN),
    ("merge", True, F32, F32, F32, "norm", False, True, True, False, True, UNFUSED, AMP_FN),
    ("random_merge", True, F32, BF, F32, "x", False, True, True, False, True, UNFUSED, AMP_FN),
    ("drop", True, BF, BF, F32, "x", False, True, True, False, True, UNFUSED, AMP_FN),
    ("drop", True, F32, BF, F32, "norm", False, True, True, True, True, UNFUSED, AMP_FN),
    ("random_drop", True, F32, BF, F32, "residual", False, True, True, False, True, UNFUSED, AMP_FN),
    ("merge", True, F32, BF, F32, "x", False, True, True, False, False, UNFUSED, AMP_FN),
    # ... not for hybrid, with trace_source, for a pair the entries refuse, or with a switch it stands on off
    ("hybrid", True, F32, BF, F32, "x", False, True, True, True, True, UNFUSED, UNFUSED),
    ("merge", True, F32, BF, F32, "x", True, True, True, True, True, UNFUSED, UNFUSED),
    ("drop", True, BF, BF, F32, "residual", True, True, True, False, True, UNFUSED, UNFUSED),
    ("merge", True, BF, F32, F32, "x", False, True, True, False, True, UNFUSED, UNFUSED),
    ("merge", True, F32, BF, F32, "x", False, False, True, False, True, UNFUSED, UNFUSED),
    ("merge", True, F32, BF, F32, "x", False, True, False, False, True, UNFUSED, UNFUSED),
    # nobody wants a gradient (AUTOCAST_FUSED_LN on in every row): the mixed-precision launch as before
    ("merge", True, F32, BF, F32, None, False, True, True, False, True, MERGE_AMP, MERGE_AMP),
    ("drop", True, BF, BF, F32, None, False, True, True, True, True, DROP_AMP, DROP_AMP),
    # autocast off, and 16-bit parameters under autocast: the 16-bit launches and their Function keep their place
    ("merge", False, BF, BF, BF, "x", False, True, True, True, True, FUNCTION, FUNCTION),
    ("merge", False, BF, BF, BF, "x", False, True, True, False, True, UNFUSED, UNFUSED),
    ("merge", False, BF, BF, BF, None, False, True, True, False, True, MERGE_LN, MERGE_LN),
    ("merge", True, BF, BF, BF, "x", False, True, True, True, True, FUNCTION, FUNCTION),
    ("merge", False, F32, F32, F32, "x", False, True, True, True, True, UNFUSED, UNFUSED),
]


def _run_block(monkeypatch, row, switch):
    mode, autocast, xd, rd, pd, who, trace, native, merge_native, train, fuse_add = row[:11]
    from tome import _abi, _ln
    from tome import merge as M
    from tome.patch import _common as C
    routes = []
    monkeypatch.setattr(_ln, "NATIVE_MERGE_LN_AUTOCAST_BACKWARD", switch)
    monkeypatch.setattr(M, "NATIVE_BACKWARD", merge_native)

    def amp_trainable(x, norm, addend, merge=None):  # _abi.merge_ln_amp_trainable without `x.is_cuda` and the plan
        return x.dim() == 3 and type(norm) is torch.nn.LayerNorm and _abi._ln_amp_of(x, norm, addend)

    monkeypatch.setattr(_abi, "merge_ln_amp_trainable", amp_trainable)
    real_route = C.fused_route
    monkeypatch.setattr(C, "fused_route", lambda *a: routes.append(real_route(*a)) or routes[-1])
    real_seams = amp._train_seams

    def train_seams(mp, seams, Cmod):  # the recorders of the two public calls; TRAIN_FUSED_LN as the row says
        real_seams(mp, seams, Cmod)
        mp.setattr(Cmod, "TRAIN_FUSED_LN", train)

    monkeypatch.setattr(amp, "_train_seams", train_seams)
    seams, info, xo, y, got = amp._run_block(
        monkeypatch, (mode, autocast, xd, rd, pd, who, trace, True, native, True, True, fuse_add), train=True)
    return seams, info, xo, y, got, routes


@pytest.mark.parametrize("switch", [False, True], ids=["off", "on"])
@pytest.mark.parametrize("row", BLOCK, ids=_ids(BLOCK, 11))
def test_merge_then_norm_route(row, switch, monkeypatch):
    mode = row[0]
    want = row[12 if switch else 11]
    seams, info, xo, y, got, routes = _run_block(monkeypatch, row, switch)
    assert len(got) == 1, got
    launch = got[0][0]
    if want == AMP_FN:
        assert routes[0] == AMP_FN and launch == FUNCTION, (routes, got)
        which = "drop" if mode in ("drop", "random_drop") else "merge"
        assert got[0][1:] == (which, True), "the Function reads the residual itself, whatever TOME_FUSE_ADD says"
        assert "_folded" not in info and not [c for c in seams.calls if c[0] == "trailing_ln_kernel"]
        assert [c[:2] for c in seams.calls if c[0] == "match"] == [("match", which)]
        if which == "drop":
            assert tuple(info["size"].shape) == (2, 6, 1) and bool((info["size"] == 1).all())
    else:
        assert AMP_FN not in routes and launch == want, (routes, got)


def test_the_switch_is_off_by_default_and_the_entry_exists():
    import os
    from tome import _abi, _ln
    from tome import merge as M
    from tome.patch import _common as C
    assert _ln.NATIVE_MERGE_LN_AUTOCAST_BACKWARD is False and _ln.AMP_FUNCTION == AMP_FN
    for name in ("tome_merge_ln_backward_amp", "tome_merge_ln_backward_amp_workspace_bytes"):
        assert name in _abi.SYMBOLS and _abi.SIGNATURES[name][2]  # additions to v11
    assert _abi.ABI_VERSION == 11
    assert callable(_abi.merge_ln_backward_amp) and callable(_abi.merge_ln_amp_trainable)
    assert callable(_ln.merge_ln_backward_amp) and callable(_ln.merge_ln_amp_native)
    assert (AMP_FN, False) in C._LAUNCH and (AMP_FN, True) in C._LAUNCH
    assert "amp_function" in M._ln_route.__doc__ and "tome_merge_ln_backward_amp" in M.merge_wavg_ln.__doc__
    assert "tome_merge_ln_backward_amp" in M.drop_ln.__doc__
    readme = open(os.path.join(amp.ROOT, "README.md")).read()
    assert "NATIVE_MERGE_LN_AUTOCAST_BACKWARD" in readme and "tome_merge_ln_backward_amp" in readme


# ---------------------------------------------------------------------------------------------------------------------
# the Function on the CPU, through its seams
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_dtype,a_dtype,needs", [(BF, BF, (True, True)), (F32, BF, (True, True)), (F32, BF, (True, False)),
                                                   (F32, F32, (False, True)), (F32, None, (True, False))])
def test_function_saves_and_returns_what_the_issue_says(x_dtype, a_dtype, needs, monkeypatch):
    """_MergeLnAmpFunction with its launches stood in for on the CPU: it saves x_out, weight, size and size_out and
    nothing else, asks gx16 only for a 16-bit addend of an fp32 stream that needs a gradient, hands x gx and the addend
    gx or gx16, and -- when nothing read y -- runs the merge alone and gives the parameters zeros."""
    from tome import _abi, _ln
    n, T, r, C = 2, 8, 2, 16
    plan = types.SimpleNamespace(n=n, T=T, r=r)
    seen = {}
    monkeypatch.setattr(_abi, "plan_row_map", lambda p: None)

    def fwd(plan_, x, size, w, b, eps, y_dtype, addend=None, log_size=False):
        assert not any(t.requires_grad for t in (x, w, b) + ((addend,) if addend is not None else ()))
        seen["fwd"] = (x.dtype, None if addend is None else addend.dtype, y_dtype)
        return x[:, r:].clone(), x[:, r:].to(y_dtype), torch.ones(n, T - r, 1)

    def bwd(plan_, gy, gx_out, xs, out_div, in_mul, weight, eps, drop, want_w, want_b, want_gx16):
        seen["bwd"] = (gy.dtype, None if gx_out is None else gx_out.dtype, xs.dtype, want_w, want_b, want_gx16, drop)
        gx = torch.full((n, T, C), 3.0, dtype=xs.dtype)
        return (gx, torch.full((n, T, C), 5.0, dtype=gy.dtype) if want_gx16 else None,
                torch.ones(C) if want_w else None, torch.ones(C) if want_b else None)

    def merge_bwd(plan_, g, out_div=None, in_mul=None, drop=False):
        seen["merge_bwd"] = (g.dtype, out_div is not None, in_mul is not None, drop)
        return torch.full((n, T, C), 7.0, dtype=g.dtype)

    monkeypatch.setattr(_abi, "merge_wavg_ln_amp", fwd)
    monkeypatch.setattr(_ln, "merge_ln_backward_amp", bwd)
    monkeypatch.setattr(_abi, "merge_backward", merge_bwd)
    monkeypatch.setattr(_abi, "autocast_dtype", lambda device: BF)
    norm = torch.nn.LayerNorm(C)
    x = torch.randn(n, T, C).to(x_dtype).requires_grad_(needs[0])
    a = None if a_dtype is None else torch.randn(n, T, C).to(a_dtype).requires_grad_(needs[1])
    size = torch.ones(n, T, 1)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        x_out, y, s_out = _ln.merge_ln_amp_native(plan, x, a, size, norm)
    assert seen["fwd"] == (x_dtype, a_dtype, BF) and y.dtype == BF and not s_out.requires_grad
    assert len(saved) == 4 and [tuple(t.shape) for t in saved] == [(n, T - r, C), (C,), (n, T, 1), (n, T - r, 1)]
    (x_out.float().sum() + y.float().sum()).backward()
    addend16 = a is not None and a_dtype != x_dtype
    assert seen["bwd"] == (BF, x_dtype, x_dtype, True, True, bool(addend16 and needs[1]), False)
    if needs[0]:
        assert x.grad.dtype == x_dtype and float(x.grad[0, 0, 0]) == 3.0
    if a is not None and needs[1]:
        assert a.grad.dtype == a_dtype and float(a.grad[0, 0, 0]) == (5.0 if addend16 else 3.0)
    assert norm.weight.grad is not None and norm.bias.grad is not None
    # nothing read y
    norm.zero_grad(set_to_none=True)
    x2 = x.detach().clone().requires_grad_(True)
    x_out, y, _ = _ln.merge_ln_amp_native(plan, x2, None if a is None else a.detach(), size, norm)
    seen.clear()
    x_out.float().sum().backward()
    assert "bwd" not in seen and seen["merge_bwd"] == (x_dtype, True, True, False)
    assert float(x2.grad[0, 0, 0]) == 7.0 and float(norm.weight.grad.abs().max()) == 0.0
    assert float(norm.bias.grad.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the header, the binding's argument order and the refusals on the host
# ---------------------------------------------------------------------------------------------------------------------
def test_binding_argument_order_is_the_headers(monkeypatch):
    from tome import _abi
    name = "tome_merge_ln_backward_amp"
    params = amp._header_params(name)
    assert len(params) == len(_abi.SIGNATURES[name][1])
    seen = {}

    def entry(*args):
        seen["args"] = args
        return 0

    monkeypatch.setattr(_abi, "lib", lambda: types.SimpleNamespace())
    monkeypatch.setattr(_abi, "require_symbol", lambda L, nm: (lambda *a: 512) if nm.endswith("_bytes") else entry)
    monkeypatch.setattr(_abi, "require_device", lambda t, what: None)
    monkeypatch.setattr(_abi, "_stream", lambda device: 4242)
    monkeypatch.setattr(_abi, "_on_device", lambda device: contextlib.nullcontext())
    made = []
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: made.append(real_empty(*a, **k)) or made[-1])
    cpu = torch.device("cpu")
    plan = _abi.MatchPlan(2, 8, 2, False, True, None, None, None, None, torch.zeros((2, 4), dtype=torch.int32), cpu)
    gy, xs, gi = torch.zeros((2, 6, 16), dtype=HF), torch.zeros((2, 6, 16)), torch.ones((2, 6, 16))
    s_out, size, w = torch.ones((2, 6, 1)), torch.ones((2, 8, 1)), torch.ones(16)
    gx, gx16, dw, db = _abi.merge_ln_backward_amp(plan, gy, gi, xs, s_out, size, w, 1e-5, want_gx16=True)
    got = dict(zip(params, seen["args"]))
    code = _abi.DTYPES
    ws = [t for t in made if t.dtype == torch.uint8][-1]
    want = {"gy": gy.data_ptr(), "gy_dtype": code[HF], "gx_out": gi.data_ptr(), "xs": xs.data_ptr(), "x_dtype": code[F32],
            "out_div": s_out.data_ptr(), "in_mul": size.data_ptr(), "size_dtype": code[F32], "n": 2, "T": 8, "C": 16,
            "r": 2, "row_map": plan.row_map.data_ptr(), "distill_token": 1, "drop": 0, "weight_f32": w.data_ptr(),
            "gx": gx.data_ptr(), "gx16": gx16.data_ptr(), "dweight_f32": dw.data_ptr(), "dbias_f32": db.data_ptr(),
            "workspace": ws.data_ptr(), "stream": 4242}
    assert set(want) | {"eps"} == set(params), sorted(set(params) ^ (set(want) | {"eps"}))
    for key, value in want.items():
        assert got[key] == value, (key, got[key], value)
    assert abs(got["eps"] - 1e-5) < 1e-12
    assert gx.dtype == F32 and tuple(gx.shape) == (2, 8, 16) and gx16.dtype == HF and dw.dtype == F32 and db.dtype == F32


def test_refusals_are_made_on_the_host_before_any_launch():
    """The entry's own checks need no device: with host buffers (never dereferenced) every illegal call comes back with
    status 1 and a text of its own.  (tests/test_merge_ln_backward_amp_gpu.py repeats them on the device and shows that
    nothing was written.)"""
    from tome import _abi
    L = _abi.lib()
    code = _abi.DTYPES
    n, T, r = 2, 8, 2
    rm = torch.zeros((n, 4), dtype=torch.int32)
    w = torch.ones(1032)
    ws = torch.zeros(1 << 16, dtype=torch.uint8)

    def call(gy, xs, C=64, gi=None, so=None, si=None, size_dtype=F32, r_=r, row_map=rm, drop=0, gx16=None, dw=None,
             workspace=ws, weight=w, gy_code=None):
        gx = torch.empty((n, T, xs.shape[-1]), dtype=xs.dtype)
        return L.tome_merge_ln_backward_amp(gy.data_ptr(), code[gy.dtype] if gy_code is None else gy_code, _abi._ptr(gi),
                                            xs.data_ptr(), code[xs.dtype], _abi._ptr(so), _abi._ptr(si), code[size_dtype], n,
                                            T, C, r_, _abi._ptr(row_map), 0, drop, _abi._ptr(weight), 1e-6, gx.data_ptr(),
                                            _abi._ptr(gx16), _abi._ptr(dw), None, _abi._ptr(workspace), None)

    def mk(dtype, C=64, rows=T - r):
        return torch.zeros((n, rows, C), dtype=dtype)

    def refused(rc, text):
        msg = L.tome_last_error()
        assert rc == 1 and b"tome_merge_ln_backward_amp" in msg and text in msg, (rc, msg)

    for gd, xd in ((F32, F32), (BF, HF), (HF, BF)):
        refused(call(mk(gd), mk(xd)), b"unsupported dtypes")
    refused(call(mk(BF), mk(F32), gy_code=7), b"unsupported dtypes")
    refused(call(mk(BF, 12), mk(F32, 12), C=12), b"C % 8 == 0 and C <= 1024 required (C=12)")
    refused(call(mk(BF, 1032), mk(F32, 1032), C=1032), b"(C=1032)")
    refused(call(mk(BF), mk(F32), r_=0), b"r=0")
    refused(call(mk(BF), mk(F32), r_=5), b"r=5")
    refused(call(mk(BF), mk(F32), row_map=None), b"null row_map")
    refused(call(mk(BF), mk(F32), weight=None), b"null buffer")
    refused(call(mk(BF), mk(BF), gx16=mk(BF, rows=T)), b"gx16 belongs to an fp32 stream")
    refused(call(mk(BF), mk(F32), so=torch.ones(n, T - r), drop=1), b"drop takes no scales")
    refused(call(mk(BF), mk(F32), so=torch.ones(n, T - r), size_dtype=BF), b"sizes must be of x's dtype or fp32")
    refused(call(mk(HF), mk(HF), si=torch.ones(n, T), size_dtype=BF), b"sizes must be of x's dtype or fp32")
    refused(call(mk(BF), mk(F32), dw=torch.zeros(64), workspace=None), b"need a workspace")
    off = torch.zeros(n * (T - r) * 64 + 8, dtype=BF)[4:4 + n * (T - r) * 64].view(n, T - r, 64)
    assert off.data_ptr() % 16 == 8
    refused(call(off, mk(F32)), b"16-byte aligned buffers required")
    refused(call(mk(BF), mk(BF), gi=off), b"16-byte aligned buffers required")
    refused(call(mk(BF), mk(F32), weight=w[2:]), b"16-byte aligned buffers required")
    for C, dt in ((1032, BF), (100, F32), (96, None)):
        assert L.tome_merge_ln_backward_amp_workspace_bytes(n, T, C, 7 if dt is None else code[dt]) == 0
    assert L.tome_merge_ln_backward_amp_workspace_bytes(n, T, 96, code[F32]) >= 2 * 96 * 4
    assert (L.tome_merge_ln_backward_amp_workspace_bytes(n, T, 96, code[F32])
            == L.tome_merge_ln_backward_amp_workspace_bytes(n, T, 96, code[BF]))
