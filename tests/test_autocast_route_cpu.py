"""`tome._ln.route` under autocast, on CPU tensors, no launch.  The one seam `_abi.autocast_dtype` is replaced by a given
answer: None (autocast off) must leave every row of tests/test_route_cpu.py's table, and fp32 tensors, as they are;
a 16-bit answer brings the mixed answers "amp_direct" / "amp_function" for the tensors a model under autocast has (fp32
LayerNorm parameters, tokens of the autocast dtype or fp32), per participant that wants a gradient; the module switch
`_ln.NATIVE_LN_AUTOCAST` turns every mixed answer into None."""
import itertools

import pytest
import torch

from test_route_cpu import SWITCH, TABLE, _route
from test_route_cpu import mods  # noqa: F401  (the fixture: the tensor-kind predicates answer what the test says)

D, F_, AD, AF = "direct", "function", "amp_direct", "amp_function"
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.fixture
def seam(monkeypatch):
    from tome import _abi
    state = {"dtype": None, "asked": 0}

    def autocast_dtype(device):
        state["asked"] += 1
        return state["dtype"]

    monkeypatch.setattr(_abi, "autocast_dtype", autocast_dtype)
    return state


def _ln_mods():
    from tome import _abi, _ln, merge
    from tome.patch import _common
    return _abi, _ln, merge, _common


@pytest.mark.parametrize("row", TABLE, ids=[f"{r[0]}-{r[1]}" for r in TABLE])
def test_autocast_off_answers_as_today(row, mods, seam, monkeypatch):  # noqa: F811
    """The table of tests/test_route_cpu.py with the seam saying "off": the same answers in every grad mode, tensor kind
    and switch setting -- and the switch of the mixed forms changes nothing."""
    op, who, _, _, want_on, want_off, _ = row
    module, attr = SWITCH[op]
    for grad, kind, flag, amp in itertools.product((True, False), (True, False), (True, False), (True, False)):
        mods["kind"]["value"] = kind
        monkeypatch.setattr(mods[module], attr, flag)
        monkeypatch.setattr(mods["_ln"], "NATIVE_LN_AUTOCAST", amp)
        with torch.set_grad_enabled(grad):
            got = _route(mods, op, who)
            nobody = _route(mods, op, None)
        no_grad = D if kind else None
        want = no_grad if not grad else None if not kind else want_on if flag else want_off
        assert got == want, (op, who, dict(grad=grad, kind=kind, flag=flag, amp=amp), got, want)
        assert nobody == no_grad, (op, dict(grad=grad, kind=kind, flag=flag), nobody)
        monkeypatch.setattr(mods[module], attr, True)


def _parts(x_dtype=F32, a_dtype=None, C=8, norm_dtype=F32, cls=torch.nn.LayerNorm):
    norm = cls(C).requires_grad_(False).to(norm_dtype)
    x = torch.zeros(2, 5, C, dtype=x_dtype)
    a = None if a_dtype is None else torch.zeros(2, 5, C, dtype=a_dtype)
    return {"x": x, "addend": a, "weight": norm.weight, "bias": norm.bias, "norm": norm}


def _ask(_ln, p, **kw):
    return _ln.route(p["x"], p["norm"], p["addend"], **kw)


def test_fp32_tensors_without_autocast_take_the_framework(seam):
    """The real predicates: an fp32 model without autocast answers None, in both grad modes, whoever wants a gradient."""
    _abi, _ln, _, _ = _ln_mods()
    for a_dtype, who, grad in itertools.product((None, F32), (None, "x", "weight"), (True, False)):
        p = _parts(F32, a_dtype)
        if who:
            p[who].requires_grad_(True)
        with torch.set_grad_enabled(grad):
            assert _ask(_ln, p) is None
            assert not _abi._ln_amp_of(p["x"], p["norm"], p["addend"])


@pytest.mark.parametrize("half", [BF, HF], ids=["bf16", "fp16"])
def test_autocast_on_brings_the_mixed_answers(half, seam):
    _abi, _ln, _, _ = _ln_mods()
    seam["dtype"] = half
    other = HF if half is BF else BF
    legal = [(F32, None), (F32, half), (F32, F32), (half, None), (half, half)]
    for x_dtype, a_dtype in legal:
        who_all = ["x", "weight", "bias"] + (["addend"] if a_dtype is not None else [])
        p = _parts(x_dtype, a_dtype)
        assert _abi._ln_amp_of(p["x"], p["norm"], p["addend"])
        assert _ask(_ln, p) == AD, (x_dtype, a_dtype)                       # grad mode on, nobody wants a gradient
        for who in who_all:                                                  # ... per participant that wants one
            p = _parts(x_dtype, a_dtype)
            p[who].requires_grad_(True)
            assert _ask(_ln, p) == AF, (x_dtype, a_dtype, who)
            with torch.no_grad():
                assert _ask(_ln, p) == AD, (x_dtype, a_dtype, who)
            assert _ask(_ln, p, regrouped=True) is None                      # the regrouped mid-block norm stays as it is
    illegal = [(half, F32), (half, other), (F32, other), (other, None), (other, other), (torch.float64, None), (F32, torch.float64)]
    for x_dtype, a_dtype in illegal:
        p = _parts(x_dtype, a_dtype)
        assert _ask(_ln, p) is None, (x_dtype, a_dtype)
        with torch.no_grad():
            assert _ask(_ln, p) is None, (x_dtype, a_dtype)
    # the norm: fp32 master weights over C % 8 == 0, C <= 1024 channels of x; an addend of x's shape
    assert _ask(_ln, _parts(F32, None, norm_dtype=half)) is None
    assert _ask(_ln, _parts(half, None, norm_dtype=half)) is None              # (a CPU tensor: not _ln_of's kind either)
    assert _ask(_ln, _parts(F32, None, C=12)) is None and _ask(_ln, _parts(F32, None, C=1032)) is None
    assert _ask(_ln, _parts(F32, None, C=1024)) == AD
    p = _parts(F32, half)
    p["addend"] = p["addend"][:, 1:]
    assert _ask(_ln, p) is None
    p = _parts(F32, None)
    assert _ln.route(p["x"], torch.nn.Identity()) is None
    assert _ln.route(p["x"], torch.nn.LayerNorm(8, elementwise_affine=False)) is None
    assert _ln.route(p["x"], torch.nn.LayerNorm(8, bias=False)) is None

    class Sub(torch.nn.LayerNorm):
        pass

    p = _parts(F32, None, cls=Sub)  # a subclass may carry a forward of its own: direct without grad, never a Function
    assert _ask(_ln, p) == AD
    p["weight"].requires_grad_(True)
    assert _ask(_ln, p) is None


def test_a_model_cast_to_16_bit_keeps_its_routes_under_autocast(mods, seam):  # noqa: F811
    """Tensors of the 16-bit kernels' kind (`_ln_of` true) never reach the seam: "direct" / "function" as without autocast."""
    seam["dtype"] = BF
    for op in ("ln", "ln_add", "ln_regrouped"):
        assert _route(mods, op, None) == D and _route(mods, op, "x") == F_
    assert seam["asked"] == 0


def test_the_switches(seam, monkeypatch):
    _abi, _ln, merge, _ = _ln_mods()
    seam["dtype"] = BF
    cases = [(F32, BF, None), (F32, BF, "addend"), (F32, F32, "weight"), (BF, BF, "x"), (F32, None, "bias"), (BF, None, None)]

    def answers():
        out = []
        for x_dtype, a_dtype, who in cases:
            p = _parts(x_dtype, a_dtype)
            if who:
                p[who].requires_grad_(True)
            out.append(_ask(_ln, p))
            with torch.no_grad():
                out.append(_ask(_ln, p))
        return out

    on = answers()
    assert on == [AD, AD, AF, AD, AF, AD, AF, AD, AF, AD, AD, AD]
    monkeypatch.setattr(_ln, "NATIVE_LN_AUTOCAST", False)                   # gates both forms
    assert answers() == [None] * len(on)
    monkeypatch.setattr(_ln, "NATIVE_LN_AUTOCAST", True)
    for module, attr in ((_ln, "NATIVE_LN_BACKWARD"), (merge, "NATIVE_BACKWARD")):  # the backward's switches: the Function
        monkeypatch.setattr(module, attr, False)
        assert answers() == [None if a == AF else a for a in on], attr
        monkeypatch.setattr(module, attr, True)
    assert answers() == on


def test_the_seam_itself_is_off_on_the_cpu():
    from tome import _abi
    assert _abi.autocast_dtype(torch.device("cpu")) is None
    assert _abi.autocast_dtype(torch.device("cuda", 0)) is None            # autocast is off
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert _abi.autocast_dtype(torch.device("cpu")) is None            # not the kernels' device
        x = torch.zeros(2, 5, 8, dtype=torch.bfloat16)
        assert not _abi._ln_amp_of(x, torch.nn.LayerNorm(8))


def test_trailing_norm_takes_the_mixed_form_in_both_grad_modes(seam, monkeypatch):
    """Autocast off: the no-grad layer never asks the route (as always) and grad mode with nothing to differentiate takes
    the framework's norm.  Autocast on: whatever mixed form the route offers is taken, with and without grad."""
    _abi, _ln, _, _common = _ln_mods()
    taken = []
    monkeypatch.setattr(_ln, "add_layernorm", lambda x, a, norm, how=False: taken.append(how) or (x, "native", False))
    asked = []
    route = _ln.route
    monkeypatch.setattr(_ln, "route", lambda *a, **kw: asked.append(1) or route(*a, **kw))
    p = _parts(F32, None)
    want = p["norm"](p["x"])
    with torch.no_grad():
        assert torch.equal(_common._trailing_norm(p["x"], p["norm"]), want) and not asked and not taken
    assert torch.equal(_common._trailing_norm(p["x"], p["norm"]), want) and not taken
    seam["dtype"] = BF
    with torch.no_grad():
        assert _common._trailing_norm(p["x"], p["norm"]) == "native"
    assert _common._trailing_norm(p["x"], p["norm"]) == "native"
    p["x"].requires_grad_(True)
    assert _common._trailing_norm(p["x"], p["norm"]) == "native"
    assert taken == [AD, AD, AF]
    monkeypatch.setattr(_ln, "NATIVE_LN_AUTOCAST", False)
    got = _common._trailing_norm(p["x"], p["norm"])
    assert torch.equal(got, want) and got.grad_fn is not None and len(taken) == 3
