"""ViViT's MLP on the kernels (tome_gelu_tanh, tome_gelu_tanh_backward: k_gelu_tanh, k_gelu_bwd with the tanh form;
tome/_mlp.py mlp_pair): op-level gradients at the widths around every change of the launch form against the fp64
reference and derived bounds of tests/gelu_tanh_oracle.py, bit-level properties, the forward against the bound and the
framework's kernel, the ABI's refusals, the Function on the host's VivitIntermediate / VivitOutput, routing, the memory
it saves, and a patched ViViT that trains through it."""
import copy

import pytest
import torch

import gelu_bwd_oracle as erf_oracle
import gelu_tanh_oracle as go

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
ROWS = (1, 2, 5, 37, 111, 1031)
WIDTHS = (8, 16, 64, 200, 2040, 2048, 2056, 3072, 4096, 4104, 8192)


def _mods():
    from tome import _abi, _mlp
    from tome import merge as M
    return _abi, _mlp, M


def _bits(t):
    return t.view(torch.int16)


def _all_four(_abi, h, ga, ref, dtype, label):
    """The four (want_act, want_bias) launches on one input: every element checked, gh the same bits in all of them, the
    activation the forward's bits, h untouched."""
    hd, gd = h.to(DEV), ga.to(DEV)
    h_before = hd.clone()
    want_a = _abi.gelu_tanh(hd, inplace=False)
    first = None
    worst = (0.0, 0.0)
    for want_act in (False, True):
        for want_bias in (False, True):
            gh, a, db = _abi.gelu_tanh_backward(hd, gd, want_act=want_act, want_bias=want_bias, inplace=False)
            assert (a is None) == (not want_act) and (db is None) == (not want_bias)
            if first is None:  # every element against the bound once; the other launches must give these very bits
                first = gh
                worst = go.check(f"{label} act={want_act} bias={want_bias}", gh, db, ref, dtype)
            else:
                assert torch.equal(_bits(gh), _bits(first)), f"{label}: gh depends on what else was asked for"
            if want_bias:
                badp, w = go.outside_db(db, gh, dtype)
                assert not bool(badp.any()), f"{label} act={want_act}: {int(badp.sum())} columns of db1 outside"
                worst = (worst[0], max(worst[1], w))
            if want_act:
                assert torch.equal(_bits(a), _bits(want_a)), f"{label}: the activation is not the forward's bits"
    assert torch.equal(_bits(hd), _bits(h_before)), f"{label}: h was written"
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_gradients_at_every_width(dtype):
    """Every M x Hd of the lists, all four (want_act, want_bias) combinations, every element of gh / a / db1; every third
    width has ga scaled by 1e-3.  The forms visited are the forms the mirror says exist."""
    _abi = _mods()[0]
    forms, worst = set(), (0.0, 0.0)
    for i, Hd in enumerate(WIDTHS):
        for rows in ROWS:
            S, _, RP, _, _ = go.form(rows, Hd)
            forms.add((S, RP > 1))
            h, ga = go.make_inputs(rows, Hd, dtype, 13 * Hd + rows, grad_scale=1e-3 if i % 3 == 2 else 1.0)
            w = _all_four(_abi, h, ga, go.reference(h, ga), dtype, f"M={rows} Hd={Hd} {dtype}")
            worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    print(f"tanh form, worst err/bound over all shapes {dtype}: gh {worst[0]:.3f} db1 {worst[1]:.3f}")
    assert forms == erf_oracle.forms_that_exist()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_gradients_on_launches_whose_workgroups_walk_several_steps(dtype):
    """2051 rows of 3072 (S = 2, two passes per step) and 1541 rows of 8192 (S = 4): more than 512 steps, so workgroups
    walk 3 and 4 steps and the last one runs out of rows part-way."""
    _abi = _mods()[0]
    for rows, Hd in ((2051, 3072), (1541, 8192)):
        S, Up, RP, spw, parts = go.form(rows, Hd)
        assert spw >= 3 and rows % (Up * RP * spw) != 0
        h, ga = go.make_inputs(rows, Hd, dtype, Hd + 1)
        _all_four(_abi, h, ga, go.reference(h, ga), dtype, f"long M={rows} Hd={Hd} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_every_value_is_finite_and_inside(dtype):
    """Every finite fp16 value / every bf16 value with |v| <= 2^20 through forward and backward (ga = -1e3)."""
    _abi = _mods()[0]
    h = go.every_value(dtype)
    ga = torch.full_like(h, -1e3)
    ref = go.reference(h, ga)
    gh, a, _ = _abi.gelu_tanh_backward(h.to(DEV), ga.to(DEV), want_act=True, want_bias=False, inplace=False)
    y = _abi.gelu_tanh(h.to(DEV))
    assert torch.isfinite(gh.float()).all() and torch.isfinite(a.float()).all()
    assert torch.equal(_bits(y), _bits(a))
    bad, worst = go.outside_gh(gh, ref, dtype)
    bad_a, worst_a = go.outside_a(y, ref, dtype)
    print(f"every value {dtype}: gh worst err/bound {worst:.3f}, a {worst_a:.3f}")
    assert not bool(bad.any()) and not bool(bad_a.any())


def test_bits_in_place_and_on_every_run():
    _abi = _mods()[0]
    for dtype in DTYPES:
        for rows, Hd in ((111, 200), (1031, 3072), (37, 4104)):
            h, ga = go.make_inputs(rows, Hd, dtype, rows + Hd)
            hd, gd = h.to(DEV), ga.to(DEV)
            out = [_abi.gelu_tanh_backward(hd, gd, want_act=True, want_bias=True, inplace=False) for _ in range(2)]
            for x, y in zip(*out):
                assert torch.equal(_bits(x), _bits(y)), "two runs differ"
            g2 = gd.clone()
            gh, a, db = _abi.gelu_tanh_backward(hd, g2, want_act=True, want_bias=True, inplace=True)
            assert gh.data_ptr() == g2.data_ptr()
            for x, y in zip((gh, a, db), out[0]):
                assert torch.equal(_bits(x), _bits(y)), "in place differs from out of place"
            g3 = gd.clone()
            gh3, a3, db3 = _abi.gelu_tanh_backward(hd, g3, want_act=False, want_bias=False, inplace=True)
            assert a3 is None and db3 is None and torch.equal(_bits(gh3), _bits(out[0][0]))
            assert torch.equal(_bits(hd), _bits(h.to(DEV)))
            # the forward: in place and out of place, the bits the backward rebuilds
            y = _abi.gelu_tanh(hd, inplace=False)
            y2 = _abi.gelu_tanh(hd.clone(), inplace=True)
            assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(y), _bits(a))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_forward_against_the_bound_and_the_framework(dtype):
    """tome_gelu_tanh within the bound for a; against F.gelu(h, approximate="tanh") on the GPU the share of differing
    elements and the largest difference are printed and gated only by the sum of the two forms'
    bounds."""
    _abi = _mods()[0]
    worst_a = share = top = 0.0
    n = 0
    for rows, Hd in ((37, 64), (111, 200), (1031, 3072), (5, 8192)):
        h, _ = go.make_inputs(rows, Hd, dtype, rows + 7 * Hd)
        ref = go.reference(h)
        y = _abi.gelu_tanh(h.to(DEV))
        bad, w = go.outside_a(y, ref, dtype)
        assert not bool(bad.any()), (rows, Hd, int(bad.sum()))
        worst_a = max(worst_a, w)
        fw = torch.nn.functional.gelu(h.to(DEV), approximate="tanh")
        diff = (y.double() - fw.double()).abs().cpu().reshape(ref["a"].shape)
        assert bool((diff <= go.bound_a(ref, dtype) + go.bound_a_framework(ref, dtype)).all())
        share += float((_bits(y) != _bits(fw)).sum())
        n += y.numel()
        top = max(top, float(diff.max()))
    print(f"tome_gelu_tanh {dtype}: worst err/bound {worst_a:.3f}; against the framework's kernel "
          f"{100 * share / n:.3f} % of {n} elements differ, largest difference {top:.3e}")


def test_abi_refusals():
    """Every TOME_EINVAL / TOME_EWORKSPACE case of the entry (the erf entry's list); none of them launches."""
    _abi = _mods()[0]
    L = _abi.lib()
    rows, Hd = 5, 64
    h, ga = (t.to(DEV) for t in go.make_inputs(rows, Hd, torch.bfloat16, 1))
    gh = torch.full_like(h, 7.0)
    act = torch.full_like(h, 7.0)
    db = torch.full((Hd,), 7.0, dtype=h.dtype, device=DEV)
    need = L.tome_gelu_erf_backward_workspace_bytes(rows, Hd)  # the one size function
    assert need > 0 and not hasattr(L, "tome_gelu_tanh_backward_workspace_bytes")
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def call(h_=h, ga_=ga, dtype=1, rows_=rows, Hd_=Hd, gh_=gh, act_=act, db_=db, ws_=ws.data_ptr(), nbytes=need):
        ptr = lambda t: t if (t is None or isinstance(t, int)) else p(t)  # noqa: E731
        return L.tome_gelu_tanh_backward(ptr(h_), ptr(ga_), dtype, rows_, Hd_, ptr(gh_), ptr(act_), ptr(db_), ws_, nbytes, stream)

    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((gh == 7.0).all())
    gh.fill_(7.0), act.fill_(7.0), db.fill_(7.0)
    bad = [call(h_=None), call(ga_=None), call(gh_=None),
           call(h_=h.data_ptr() + 2), call(ga_=ga.data_ptr() + 2), call(gh_=gh.data_ptr() + 2),
           call(act_=act.data_ptr() + 2), call(ws_=ws.data_ptr() + 4),
           call(dtype=0), call(Hd_=12), call(Hd_=60), call(Hd_=8200), call(Hd_=0), call(rows_=0), call(rows_=-3),
           call(act_=h), call(act_=ga), call(act_=gh), call(gh_=h)]
    einval = bad[0]
    assert einval != 0 and all(rc == einval for rc in bad), bad
    assert b"tome_gelu_tanh_backward" in L.tome_last_error()
    short = [call(ws_=None), call(nbytes=need - 1), call(nbytes=0)]
    assert all(rc != 0 and rc != einval for rc in short) and len(set(short)) == 1, short
    assert b"workspace" in L.tome_last_error()
    assert call(db_=None, ws_=None, nbytes=0) == 0  # without dbias no workspace is needed
    assert call(gh_=ga) == 0                        # gh may lie over ga
    torch.cuda.synchronize()
    ga.copy_(go.make_inputs(rows, Hd, torch.bfloat16, 1)[1])
    gh.fill_(7.0), act.fill_(7.0), db.fill_(7.0)
    for rc in (call(h_=None), call(Hd_=12), call(ws_=None), call(act_=h), call(gh_=h)):
        assert rc != 0
    torch.cuda.synchronize()
    assert bool((gh == 7.0).all()) and bool((act == 7.0).all()) and bool((db == 7.0).all()), "a refused call launched"
    # the forward's refusals
    y = torch.empty_like(h)
    f = lambda x, dt, n, out: L.tome_gelu_tanh(x, dt, n, out, stream)  # noqa: E731
    assert f(h.data_ptr(), 1, h.numel(), y.data_ptr()) == 0
    for rc in (f(None, 1, 8, y.data_ptr()), f(h.data_ptr(), 0, 8, y.data_ptr()), f(h.data_ptr(), 1, 12, y.data_ptr()),
               f(h.data_ptr() + 2, 1, 8, y.data_ptr()), f(h.data_ptr(), 1, 0, y.data_ptr())):
        assert rc == einval
    with pytest.raises(_abi.TomeHipError):
        _abi.gelu_tanh_backward(h.float(), ga.float(), want_act=False, want_bias=False)
    with pytest.raises(_abi.TomeHipError):
        _abi.gelu_tanh(h.float())


# ---------------------------------------------------------------------------------------------------------------------
# the Function, through mlp_pair on the host's modules
# ---------------------------------------------------------------------------------------------------------------------
def _pair(C=64, Hd=256, dtype=torch.bfloat16, seed=0, drop1=0.0, drop2=0.0, bias=True):
    from hosts import vivit
    torch.manual_seed(seed)
    cfg = vivit.VivitConfig(hidden_size=C, intermediate_size=Hd)
    inter, outp = vivit.VivitIntermediate(cfg), vivit.VivitOutput(cfg)
    if not bias:
        inter.dense = torch.nn.Linear(C, Hd, bias=False)
    inter.dropout.p, outp.dropout.p = drop1, drop2
    inter, outp = inter.to(DEV).to(dtype).eval(), outp.to(DEV).to(dtype).eval()
    with torch.no_grad():
        for prm in list(inter.parameters()) + list(outp.parameters()):
            prm.copy_(torch.randn_like(prm.float()).mul_(0.3 if prm.dim() == 2 else 0.5).to(dtype))
    return inter, outp


def _tokens(M=74, C=64, dtype=torch.bfloat16, seed=1, grad=True):
    y = torch.randn(M, C, generator=torch.Generator().manual_seed(seed)).to(DEV).to(dtype)
    return y.requires_grad_(grad)


def _framework(inter, outp, y):
    return outp.dense(inter(y))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_function_forward_bits_and_gradients(dtype):
    """C = 64, Hd = 256, M = 2 x 37.  Forward bit-equal to output.dense(gelu_tanh(intermediate.dense(y))); gradients of
    y, W1, b1, W2, b2 against the fp64 gradient: native error <= 2 x the framework path's error + 2^-20 of the largest
    gradient (the acceptance of tests/test_mlp_backward_gpu.py)."""
    _abi, _mlp_mod, _ = _mods()
    inter, outp = _pair(dtype=dtype)
    y = _tokens(dtype=dtype)
    gout = torch.randn(74, 64, generator=torch.Generator().manual_seed(2)).to(DEV).to(dtype)
    with torch.no_grad():
        want = outp.dense(_abi.gelu_tanh(inter.dense(y)))
    out = _mlp_mod.mlp_pair(inter, outp, y)
    assert out is not None and type(out.grad_fn).__name__ == "_MlpFunctionBackward"
    assert torch.equal(_bits(out), _bits(want))
    prms = [y, inter.dense.weight, inter.dense.bias, outp.dense.weight, outp.dense.bias]
    g_nat = torch.autograd.grad(out, prms, gout)
    g_fw = torch.autograd.grad(_framework(inter, outp, y), prms, gout)
    i64, o64 = copy.deepcopy(inter).double(), copy.deepcopy(outp).double()
    y64 = y.detach().double().requires_grad_()
    p64 = [y64, i64.dense.weight, i64.dense.bias, o64.dense.weight, o64.dense.bias]
    g_ref = torch.autograd.grad(_framework(i64, o64, y64), p64, gout.double())
    for name, a, b, r in zip(("y", "W1", "b1", "W2", "b2"), g_nat, g_fw, g_ref):
        ea, eb = float((a.double() - r).abs().max()), float((b.double() - r).abs().max())
        top = float(r.abs().max())
        print(f"{name} {dtype}: native err {ea:.3e} framework err {eb:.3e} largest gradient {top:.3e}")
        assert ea <= 2 * eb + 2.0 ** -20 * top, (name, ea, eb, top)


def test_function_asks_for_what_is_needed_retains_and_refuses_double_backward(monkeypatch):
    _abi, _mlp_mod, _ = _mods()
    asked = []
    orig_seam = _mlp_mod.gelu_backward
    monkeypatch.setattr(_mlp_mod, "gelu_backward", lambda *a: asked.append(a[2:]) or orig_seam(*a))
    sizes = []
    orig_ws = _abi._workspace
    monkeypatch.setattr(_abi, "_workspace", lambda dev, st, n: sizes.append(n) or orig_ws(dev, st, n))
    # frozen fc2 weight: no activation is asked for
    inter, outp = _pair()
    outp.dense.weight.requires_grad_(False)
    _mlp_mod.mlp_pair(inter, outp, _tokens()).float().square().sum().backward()
    assert asked == [(False, True, "tanh")] and len(sizes) == 1
    assert outp.dense.weight.grad is None and outp.dense.bias.grad is not None
    # fc1 without bias: no workspace
    asked.clear(), sizes.clear()
    inter, outp = _pair(bias=False)
    _mlp_mod.mlp_pair(inter, outp, _tokens()).float().square().sum().backward()
    assert asked == [(True, False, "tanh")] and sizes == []
    # retain_graph: the saved h survives, the second backward gives the same gradients
    inter, outp = _pair()
    y = _tokens()
    out = _mlp_mod.mlp_pair(inter, outp, y)
    prms = [y] + list(inter.parameters()) + list(outp.parameters())
    gout = torch.randn_like(out)
    g1 = torch.autograd.grad(out, prms, gout, retain_graph=True)
    g2 = torch.autograd.grad(out, prms, gout)
    for a, b in zip(g1, g2):
        assert torch.equal(_bits(a), _bits(b))
    # double backward raises
    out = _mlp_mod.mlp_pair(inter, outp, y)
    (gy,) = torch.autograd.grad(out, [y], gout, create_graph=True)
    with pytest.raises(RuntimeError):
        gy.float().sum().backward()


def test_routing(monkeypatch):
    _abi, _mlp_mod, Mg = _mods()
    calls = []
    orig = _mlp_mod.gelu_backward
    monkeypatch.setattr(_mlp_mod, "gelu_backward", lambda *a: calls.append(a[4:]) or orig(*a))

    def goes(pair, y):
        before = len(calls)
        inter, outp = pair
        out = _mlp_mod.mlp_pair(inter, outp, y)
        assert (out is not None) == (_mlp_mod.route_pair(inter, outp, y) == "function")
        if out is None:
            return False
        assert type(out.grad_fn).__name__ == "_MlpFunctionBackward"
        out.float().square().sum().backward()
        assert calls[before:] == [("tanh",)]
        return True

    def train(pair):
        return pair[0].train(), pair[1].train()

    assert goes(_pair(), _tokens())                                          # .eval() under grad
    assert goes(train(_pair()), _tokens())                                   # .train(), dropout 0
    assert goes(_pair(), _tokens(grad=False))                                # parameters alone require grad
    assert goes(_pair(dtype=torch.float16), _tokens(dtype=torch.float16))
    assert not goes(train(_pair(drop1=0.1)), _tokens())                      # live dropout in intermediate
    assert not goes(train(_pair(drop2=0.1)), _tokens())                      # ... in output
    assert goes(_pair(drop1=0.1, drop2=0.1), _tokens())                      # which .eval() switches off
    for which in (0, 1):
        child = _pair(drop1=0.1, drop2=0.1)
        child[which].dropout.train()  # the module in .eval(), its dropout alone in .train(): live all the same
        assert not goes(child, _tokens())
        child = train(_pair(drop1=0.1 if which == 0 else 0.0, drop2=0.1 if which == 1 else 0.0))
        child[which].dropout.eval()   # and the other way round: the identity
        assert goes(child, _tokens())
    erf = _pair()
    erf[0].intermediate_act_fn = torch.nn.GELU()
    assert not goes(erf, _tokens())                                          # the exact-erf form is not this pair's
    relu = _pair()
    relu[0].intermediate_act_fn = torch.nn.ReLU()
    assert not goes(relu, _tokens())
    assert not goes(_pair(dtype=torch.float32), _tokens(dtype=torch.float32))
    for which in (0, 1):
        hooked = _pair()
        hooked[which].dense.register_forward_hook(lambda m, i, o: None)
        assert not goes(hooked, _tokens())
        hooked = _pair()
        hooked[which].register_forward_hook(lambda m, i, o: None)
        assert not goes(hooked, _tokens())
        own = _pair()
        own[which].forward = lambda *a: None  # a forward put on the instance
        assert not goes(own, _tokens())

        class MyLinear(torch.nn.Linear):
            pass

        sub = _pair()
        sub[which].dense.__class__ = MyLinear
        assert not goes(sub, _tokens())
        extra = _pair()
        extra[which].adapter = torch.nn.Identity()  # a child the pair does not have
        assert not goes(extra, _tokens())

    class Renamed(type(_pair()[0])):
        pass

    other = _pair()
    other[0].__class__ = Renamed
    assert not goes(other, _tokens())                                        # a class not named VivitIntermediate
    monkeypatch.setattr(_mlp_mod, "NATIVE_MLP_BACKWARD", False)
    assert not goes(_pair(), _tokens())
    monkeypatch.setattr(_mlp_mod, "NATIVE_MLP_BACKWARD", True)
    monkeypatch.setattr(Mg, "NATIVE_BACKWARD", False)
    assert not goes(_pair(), _tokens())
    monkeypatch.setattr(Mg, "NATIVE_BACKWARD", True)
    # HF's activation classes are recognised by module and name, without transformers
    for name in ("FastGELUActivation", "NewGELUActivation", "PytorchGELUTanh", "GELUTanh"):
        cls = type(name, (torch.nn.Module,), {"forward": lambda self, x: torch.nn.functional.gelu(x, approximate="tanh"),
                                              "__module__": "transformers.activations"})
        hf = _pair()
        hf[0].intermediate_act_fn = cls()
        assert goes(hf, _tokens())
    stranger = _pair()
    stranger[0].intermediate_act_fn = type("FastGELUActivation", (torch.nn.Module,), {"__module__": "elsewhere"})()
    assert not goes(stranger, _tokens())
    # a plain fc1 / act / fc2 MLP with a tanh act stays the framework's (tome/_mlp.py route is not widened)
    plain = torch.nn.Module()
    plain.fc1, plain.act, plain.fc2 = torch.nn.Linear(64, 256), torch.nn.GELU(approximate="tanh"), torch.nn.Linear(256, 64)
    plain = plain.to(DEV).to(torch.bfloat16).eval()
    assert _mlp_mod.route(plain, _tokens()) is None


def _tiny_vivit(dtype=torch.bfloat16, layers=3):
    from hosts import vivit
    torch.manual_seed(0)
    model = vivit.ViViT(num_classes=9, image_size=64, num_frames=8, hidden_size=64, num_hidden_layers=layers,
                        num_attention_heads=1, intermediate_size=256).to(DEV)
    with torch.no_grad():  # (the host initialises some parameters with zeros: every parameter gets a value)
        for prm in model.parameters():
            if float(prm.abs().max()) == 0.0:
                prm.normal_(0.0, 0.02)
    return model


def test_no_grad_runs_nothing_of_the_function_and_keeps_the_bits(monkeypatch):
    """Under no_grad the patched layer looks nothing up and its output has the bits of the path with the switch off."""
    import tome
    _, _mlp_mod, _ = _mods()
    model = _tiny_vivit().to(torch.bfloat16).eval()
    tome.patch.vivit(model, prop_attn=True)
    model.r = 6
    clip = torch.rand(2, 3, 8, 64, 64, generator=torch.Generator().manual_seed(3)).to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        monkeypatch.setattr(_mlp_mod, "NATIVE_MLP_BACKWARD", False)
        want = model([clip])
        monkeypatch.setattr(_mlp_mod, "NATIVE_MLP_BACKWARD", True)
        for name in ("mlp_pair", "route_pair", "pair_trainable"):
            monkeypatch.setattr(_mlp_mod, name, lambda *a, name=name: pytest.fail(f"{name} under no_grad"))
        got = model([clip])
    assert got.grad_fn is None and torch.equal(_bits(got), _bits(want))


def test_memory_between_forward_and_backward(monkeypatch):
    """L = 4 pairs in a row, M = 1024, C = 64, Hd = 256, bf16: with the graph alive the native path holds one hidden
    tensor per pair less than the framework's -- at least 0.9 x L x M x Hd x 2 bytes (0.9: allocator rounding)."""
    _, _mlp_mod, _ = _mods()
    L, M, C, Hd = 4, 1024, 64, 256
    pairs = [_pair(C, Hd, seed=i) for i in range(L)]
    y = _tokens(M, C)

    def held(native):
        monkeypatch.setattr(_mlp_mod, "NATIVE_MLP_BACKWARD", native)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        x = y
        for inter, outp in pairs:
            out = _mlp_mod.mlp_pair(inter, outp, x)
            assert (out is not None) == native
            x = _framework(inter, outp, x) if out is None else out
        torch.cuda.synchronize()
        got = torch.cuda.memory_allocated() - base
        x.float().sum().backward()
        del x, out
        return got

    held(False), held(True)  # (first use: the library's own workspaces are allocated once and stay)
    fw, nat = held(False), held(True)
    print(f"bytes held between forward and backward: framework {fw}, native {nat}, one hidden tensor {M * Hd * 2}")
    assert nat <= fw - 0.9 * L * M * Hd * 2, (nat, fw)


# ---------------------------------------------------------------------------------------------------------------------
# a patched ViViT
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_patched_vivit_gradients_native_framework_fp32(mode, monkeypatch):
    """Reduced-width host, bf16, r = 6 in every layer, `.eval()` with grad and `.train()`; three runs on the same
    weights: (a) native, (b) the switch off (the parent commit's behaviour), (c) the framework in fp32.  Exactly 3
    launches through the seam for 3 layers and none with the switch off.  Worst per-parameter gradient error against (c),
    scaled by that parameter's largest gradient in (c): native <= 2 x framework.  Parameters whose largest fp32 gradient
    is below 1e-6 of the model's largest (ViViT's key bias: zero in exact arithmetic) are held to the absolute floor of
    tests/test_attention_backward_gpu.py (2^-6 of the model's largest gradient) in both 16-bit runs instead.  The pairs
    are printed; the ones measured on an MI355X are in DESIGN.md section 2."""
    import tome
    _, _mlp_mod, _ = _mods()
    model32 = _tiny_vivit()
    model16 = copy.deepcopy(model32).to(torch.bfloat16)
    with torch.no_grad():  # the fp32 run starts from the bf16 weights
        for p32, p16 in zip(model32.parameters(), model16.parameters()):
            p32.copy_(p16.float())
    tome.patch.vivit(model16, prop_attn=True)
    tome.patch.vivit(model32, prop_attn=True)
    for m in (model16, model32):
        m.train() if mode == "train" else m.eval()
    clip = torch.rand(2, 3, 8, 64, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
    launches = []
    orig = _mlp_mod.gelu_backward
    monkeypatch.setattr(_mlp_mod, "gelu_backward", lambda *a: launches.append(a[4:]) or orig(*a))

    def run(model, x):
        model.zero_grad(set_to_none=True)
        model.r = 6
        out = model([x])
        out.float().square().sum().backward()
        return {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}

    ga = run(model16, clip.to(torch.bfloat16))
    assert launches == [("tanh",)] * 3, f"{len(launches)} native MLP backward launches for 3 layers"
    monkeypatch.setattr(_mlp_mod, "NATIVE_MLP_BACKWARD", False)
    gb = run(model16, clip.to(torch.bfloat16))
    assert len(launches) == 3
    gc = run(model32, clip)
    assert ga.keys() == gb.keys() == gc.keys()
    worst_a = worst_b = 0.0
    top = max(g.abs().max().item() for g in gc.values())
    for k in gc:
        scale = gc[k].abs().max().item()
        assert torch.isfinite(ga[k]).all(), k
        if scale < 1e-6 * top:  # zero in exact arithmetic: noise in every run, no scale to divide by
            assert ga[k].abs().max().item() <= 2.0 ** -6 * top and gb[k].abs().max().item() <= 2.0 ** -6 * top, k
            continue
        worst_a = max(worst_a, (ga[k] - gc[k]).abs().max().item() / scale)
        worst_b = max(worst_b, (gb[k] - gc[k]).abs().max().item() / scale)
    print(f"vivit {mode}: worst scaled gradient error native vs fp32 {worst_a:.3e}, framework vs fp32 {worst_b:.3e}")
    assert worst_a <= 2 * worst_b, (mode, worst_a, worst_b)


def test_a_folded_bias_is_left_to_finish_linear(monkeypatch):
    """`.eval()` with grad where `intermediate.dense` alone trains: in the first layer nothing the merge or `output.dense`
    touches wants a gradient, so the fused merge launch has folded `output.dense`'s bias into the residual stream -- that
    layer's MLP stays on the former path (finish_linear finishes the fold), the later layers (their tokens require grad)
    take the Function; the gradients are those of the run with the switch off up to the 16-bit runs' own noise."""
    import tome
    _, _mlp_mod, _ = _mods()
    model = _tiny_vivit().to(torch.bfloat16).eval()
    tome.patch.vivit(model, prop_attn=True)
    for name, prm in model.named_parameters():
        prm.requires_grad_(".intermediate.dense." in name)
    clip = torch.rand(2, 3, 8, 64, 64, generator=torch.Generator().manual_seed(3)).to(DEV).to(torch.bfloat16)
    launches = []
    orig = _mlp_mod.gelu_backward
    monkeypatch.setattr(_mlp_mod, "gelu_backward", lambda *a: launches.append(a[4:]) or orig(*a))

    def run():
        model.zero_grad(set_to_none=True)
        model.r = 6
        model([clip]).float().square().sum().backward()
        return {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}

    got = run()
    assert launches == [("tanh",)] * 2, launches
    monkeypatch.setattr(_mlp_mod, "NATIVE_MLP_BACKWARD", False)
    want = run()
    assert len(launches) == 2 and got.keys() == want.keys() and len(got) == 6
    top = max(g.abs().max().item() for g in want.values())
    for k in want:
        assert torch.isfinite(got[k]).all() and (got[k] - want[k]).abs().max().item() <= 2.0 ** -6 * top, k
