"""The routing decisions of the patch layer (`route` of tome/_ln.py, _attn.py and _mlp.py) on CPU tensors, no launch:
the tensor-kind predicates of tome/_abi.py are replaced by a given bool, so what is left is the logic -- grad mode, who
requires grad, the module's switch.

TABLE is written by hand from the conditions of the commit before the routes existed (`_abi.*_ok` / `ln_fusable`, then
`_ln.wants` / `_attn.wants` / `_mlp.wants` and the inline checks of the model patches), for grad mode on and tensors of
the kind the kernels take: (operation, the one participant that requires grad, parent's answer with the module's switch
on / off, this commit's answer with the switch on / off, mark).  Marks:
    "hole"   the parent launched directly although a participant it did not look at wanted a gradient (the residual or
             addend, the LayerNorm's bias, the trajectory mix's val): the gradient was dropped without an error
    "subset" the parent's two questions looked at different subsets the other way round: a LayerNorm whose weight alone
             requires grad took the framework's ops; asking every participant once gives it the Function form
Every other row is the parent's answer.  With grad mode off, or nothing requiring grad, both commits answer "direct";
with tensors of another kind both answer None: asserted for every row below."""
import itertools

import pytest
import torch

D, F_, N = "direct", "function", None

TABLE = [
    # operation          who        parent on/off   now on/off   mark
    ("ln",               "x",       F_, N,          F_, N,       ""),
    ("ln",               "weight",  N, N,           F_, N,       "subset"),
    ("ln",               "bias",    D, D,           F_, N,       "hole"),
    ("ln_add",           "x",       F_, N,          F_, N,       ""),
    ("ln_add",           "addend",  D, D,           F_, N,       "hole"),
    ("ln_add",           "weight",  N, N,           F_, N,       "subset"),
    ("ln_add",           "bias",    D, D,           F_, N,       "hole"),
    ("ln_regrouped",     "x",       F_, N,          F_, N,       ""),
    ("ln_regrouped",     "addend",  D, D,           F_, N,       "hole"),
    ("ln_regrouped",     "weight",  F_, N,          F_, N,       ""),
    ("ln_regrouped",     "bias",    D, D,           F_, N,       "hole"),
    ("attention",        "q",       F_, N,          F_, N,       ""),
    ("attention",        "k",       F_, N,          F_, N,       ""),
    ("attention",        "v",       F_, N,          F_, N,       ""),
    ("short",            "q",       F_, N,          F_, N,       ""),
    ("short",            "k",       F_, N,          F_, N,       ""),
    ("short",            "v",       F_, N,          F_, N,       ""),
    ("short_aliased",    "q",       N, N,           N, N,        ""),
    ("trajectory",       "heads",   F_, N,          F_, N,       ""),
    ("trajectory_mix",   "q2p",     F_, N,          F_, N,       ""),
    ("trajectory_mix",   "k2",      F_, N,          F_, N,       ""),
    ("trajectory_mix",   "val",     D, D,           F_, N,       "hole"),
    ("mlp",              "y",       F_, N,          F_, N,       ""),
    ("mlp",              "fc1.weight", F_, N,       F_, N,       ""),
    ("mlp",              "fc1.bias",   F_, N,       F_, N,       ""),
    ("mlp",              "fc2.weight", F_, N,       F_, N,       ""),
    ("mlp",              "fc2.bias",   F_, N,       F_, N,       ""),
]
# the module switch of each operation: (module name, attribute)
SWITCH = {"ln": ("_ln", "NATIVE_LN_BACKWARD"), "ln_add": ("_ln", "NATIVE_LN_BACKWARD"),
          "ln_regrouped": ("_ln", "NATIVE_LN_REGROUPED_BACKWARD"), "attention": ("_attn", "NATIVE_ATTN_BACKWARD"),
          "short": ("_attn", "NATIVE_SHORT_ATTN_BACKWARD"), "short_aliased": ("_attn", "NATIVE_SHORT_ATTN_BACKWARD"),
          "trajectory": ("_attn", "NATIVE_TRAJECTORY_BACKWARD"), "trajectory_mix": ("_attn", "NATIVE_TRAJECTORY_BACKWARD"),
          "mlp": ("_mlp", "NATIVE_MLP_BACKWARD")}


class _Mlp(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1, self.act, self.fc2 = torch.nn.Linear(8, 16), torch.nn.GELU(), torch.nn.Linear(16, 8)


def _route(mods, op, who):
    """`route` of `op` on fresh CPU tensors of which `who` alone (or nothing: None) requires grad."""
    _ln, _attn, _mlp = mods["_ln"], mods["_attn"], mods["_mlp"]
    t = lambda *shape: torch.zeros(*shape)  # noqa: E731
    if op.startswith("ln"):
        norm = torch.nn.LayerNorm(8).requires_grad_(False)
        parts = {"x": t(2, 5, 8), "addend": None if op == "ln" else t(2, 4 if op == "ln_regrouped" else 5, 8),
                 "weight": norm.weight, "bias": norm.bias}
        call = lambda: _ln.route(parts["x"], norm, parts["addend"], regrouped=op == "ln_regrouped")  # noqa: E731
    elif op == "attention":
        parts = {"q": t(1, 1, 4, 64), "k": t(1, 1, 4, 64), "v": t(1, 1, 4, 64)}
        call = lambda: _attn.route(parts["q"], parts["k"], parts["v"])  # noqa: E731
    elif op.startswith("short"):
        parts = {"q": t(1, 1, 4, 64), "k": t(1, 1, 4, 64), "v": t(1, 1, 4, 64)}
        qkv5 = None if op == "short_aliased" else t(1, 4, 3, 1, 64)
        call = lambda: _attn.short_route(parts["q"], parts["k"], parts["v"], False, qkv5)  # noqa: E731
    elif op == "trajectory":
        parts = {"heads": t(3, 1, 1, 5, 64)}
        call = lambda: _attn.trajectory_route(parts["heads"], 2)  # noqa: E731
    elif op == "trajectory_mix":
        parts = {"q2p": t(1, 4, 64), "k2": t(1, 4, 2, 64), "val": t(1, 4, 2, 64)}
        call = lambda: _attn.trajectory_mix_route(parts["q2p"], parts["k2"], parts["val"], 1)  # noqa: E731
    else:
        mlp = _Mlp().eval().requires_grad_(False)
        if not mods["kind"]["value"]:
            mlp.act = torch.nn.ReLU()  # (the MLP's kind is a module kind as well: _plain_mlp)
        parts = {"y": t(2, 8), "fc1.weight": mlp.fc1.weight, "fc1.bias": mlp.fc1.bias, "fc2.weight": mlp.fc2.weight,
                 "fc2.bias": mlp.fc2.bias}
        call = lambda: _mlp.route(mlp, parts["y"])  # noqa: E731
    if who is not None:
        parts[who].requires_grad_(True)
    return call()


@pytest.fixture
def mods(monkeypatch):
    from tome import _abi, _attn, _ln, _mlp
    kind = {"value": True}
    # the tensor-kind predicates answer what the test says (the MLP's has the device and the dtype in it, like the rest)
    for name in ("_ln_of", "_head_view", "_short_heads", "_trajectory_rows", "mlp_trainable"):
        monkeypatch.setattr(_abi, name, lambda *a, **kw: kind["value"])
    return {"_abi": _abi, "_ln": _ln, "_attn": _attn, "_mlp": _mlp, "kind": kind}


def test_table_is_complete():
    ops = {op: {who for o, who, *_ in TABLE if o == op} for op in SWITCH}
    assert ops["ln_add"] == ops["ln_regrouped"] == {"x", "addend", "weight", "bias"} and ops["ln"] == {"x", "weight", "bias"}
    assert ops["attention"] == ops["short"] == {"q", "k", "v"} and ops["trajectory_mix"] == {"q2p", "k2", "val"}
    assert ops["mlp"] == {"y", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"} and ops["trajectory"] == {"heads"}
    for op, who, p_on, p_off, on, off, mark in TABLE:
        # the rows that differ from the parent are exactly the marked ones, and no row where a participant other than
        # the first wants a gradient answers "direct"
        assert ((p_on, p_off) != (on, off)) == bool(mark), (op, who)
        assert (mark == "hole") == (D in (p_on, p_off)), (op, who)
        assert D not in (on, off), (op, who)


@pytest.mark.parametrize("row", TABLE, ids=[f"{r[0]}-{r[1]}" for r in TABLE])
def test_route_against_the_table(row, mods, monkeypatch):
    op, who, _, _, want_on, want_off, _ = row
    module, attr = SWITCH[op]
    for grad, kind, flag in itertools.product((True, False), (True, False), (True, False)):
        mods["kind"]["value"] = kind
        monkeypatch.setattr(mods[module], attr, flag)
        with torch.set_grad_enabled(grad):
            got = _route(mods, op, who)
            nobody = _route(mods, op, None)
        no_grad = D if kind else None
        want = no_grad if not grad else None if not kind else want_on if flag else want_off
        assert got == want, (op, who, dict(grad=grad, kind=kind, flag=flag), got, want)
        assert nobody == no_grad, (op, dict(grad=grad, kind=kind, flag=flag), nobody)
        monkeypatch.setattr(mods[module], attr, True)


def test_the_outer_switches_and_the_refusals(mods, monkeypatch):
    """merge.NATIVE_BACKWARD and the older switch of each family gate the Function form too; dropout, an attention map
    wanted under grad, a LayerNorm subclass and a live dropout in the MLP take the framework's ops under grad and change
    nothing without."""
    from tome import merge
    _ln, _attn, _mlp = mods["_ln"], mods["_attn"], mods["_mlp"]
    rows = {merge: [(op, who) for op, who, *_ in TABLE], _ln: [("ln_regrouped", "addend")],
            _attn: [("short", "q"), ("trajectory", "heads"), ("trajectory_mix", "val")]}
    for module, attr in ((merge, "NATIVE_BACKWARD"), (_ln, "NATIVE_LN_BACKWARD"), (_attn, "NATIVE_ATTN_BACKWARD")):
        monkeypatch.setattr(module, attr, False)
        for op, who in rows[module]:
            assert _route(mods, op, who) is None, (attr, op, who)
        monkeypatch.setattr(module, attr, True)
    q = torch.zeros(1, 1, 4, 64)
    g = torch.zeros(1, 1, 4, 64, requires_grad=True)
    assert _attn.route(q, q, q, 0.1) is None and _attn.route(g, q, q, 0.1) is None
    assert _attn.short_route(q, q, q, True) is None and _attn.short_route(q, q, g, True, torch.zeros(1, 4, 3, 1, 64)) is None
    heads = torch.zeros(3, 1, 1, 5, 64)
    assert _attn.trajectory_route(heads, 2, True) is None and _attn.trajectory_route(heads, 2, False, True) == D
    assert _attn.trajectory_route(heads.clone().requires_grad_(True), 2, False, True) is None
    q2p, k2, val = torch.zeros(1, 4, 64), torch.zeros(1, 4, 2, 64), torch.zeros(1, 4, 2, 64, requires_grad=True)
    assert _attn.trajectory_mix_route(q2p, k2, val.detach(), 1, True) == D
    assert _attn.trajectory_mix_route(q2p, k2, val, 1, True) is None

    class Sub(torch.nn.LayerNorm):
        pass

    x = torch.zeros(2, 5, 8)
    assert _ln.route(x, Sub(8).requires_grad_(False)) == D and _ln.route(x, Sub(8)) is None  # (ln_trainable: the stock class)
    assert _ln.route(x, torch.nn.LayerNorm(8).requires_grad_(False), torch.zeros(2, 5, 8, dtype=torch.float64)) is None
    assert _ln.route(x, torch.nn.Identity()) is None

    class Twice(torch.nn.Module):
        def forward(self, w):
            return 2 * w

    # a parametrized weight: the trainable tensor lives in a child module, `norm.weight` is computed from it (and the
    # norm is a LayerNorm subclass made on the fly, which ln_fusable takes).  Bias frozen, x without grad: never "direct"
    norm = torch.nn.LayerNorm(8)
    norm.bias.requires_grad_(False)
    torch.nn.utils.parametrize.register_parametrization(norm, "weight", Twice())
    assert not any(p.requires_grad for p in norm.parameters(recurse=False)) and norm.weight.requires_grad
    assert _ln.route(x, norm) is None and _ln.route(x, norm, torch.zeros(2, 5, 8)) is None
    assert not mods["_abi"].ln_fusable(x, norm) and not mods["_abi"].ln_fusable(x, norm, None)
    with torch.no_grad():
        assert _ln.route(x, norm) == D and mods["_abi"].ln_fusable(x, norm)
    mlp = _Mlp().train()
    mlp.drop = torch.nn.Dropout(0.1)
    assert _mlp.route(mlp, x) is None and _mlp.route(mlp.eval(), x) == F_
    assert _mlp.route(mlp.requires_grad_(False), x) == D and _mlp.route(torch.nn.Identity(), x) is None
