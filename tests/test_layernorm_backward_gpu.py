"""Native backward of the add + LayerNorm kernels (tome_layernorm_backward, k_ln_rows_bwd / k_ln_param_grad) on the
GPU: op-level gradients at every width against the fp64 reference and derived bound of tests/ln_bwd_oracle.py, bit-level
properties, routing of the Functions of tome/_ln.py, and patched models that train through them."""
import pytest
import torch

import ln_bwd_oracle as bo
import ln_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
EPS = 1e-5


def _mods():
    from tome import _abi, _ln
    from tome import merge as M
    from tome.patch import _common
    return _abi, _ln, M, _common


def _run(_abi, gy, xs, gi, w, skip, params):
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    gx, dw, db = _abi.layernorm_backward(dev(gy), dev(xs), dev(gi), dev(w), EPS, skip_first=skip, want_weight=params,
                                         want_bias=params)
    assert (dw is None) == (not params) and (db is None) == (not params)
    return gx, dw, db


def _class_rows_pass_through(gx, gi, label):
    want = torch.zeros_like(gx[:, 0]) if gi is None else gi[:, 0].to(gx.device)
    assert torch.equal(gx[:, 0].view(torch.int16), want.view(torch.int16)), f"{label}: class rows of gx are not gx_in's bits"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_gradients_at_every_width(dtype):
    """Every C = 8 .. 1024 (all (NIT, R) forms of the packing), 3 x 37 = 111 rows (no multiple of R = 2, 3, 4 nor of
    the 4 R rows of a workgroup), with and without gx_in, with and without parameter gradients, plain and skip_first:
    8 launches per width, every element of gx / dweight / dbias inside the oracle's bound, no case left out.  Three
    widths in four have their rows 30 standard deviations from zero."""
    _abi = _mods()[0]
    forms = set()
    for C in lo.WIDTHS:
        forms.add((3, bo.form(111, C)[0]))
        for skip in (False, True):
            for with_in in (False, True):
                gy, xs, gi, w = bo.make_inputs((3, 37, C), dtype, 7 * C + 2 * skip + with_in, far=(C // 8) % 4 != 0,
                                               grad_scale=1e-3 if (C // 8) % 3 == 0 else 1.0, skip_first=skip,
                                               with_in=with_in)
                ref = bo.reference(gy, xs, gi, w, EPS, skip_first=skip)
                for params in (False, True):
                    gx, dw, db = _run(_abi, gy, xs, gi, w, skip, params)
                    label = f"C={C} skip={skip} gx_in={with_in} params={params} {dtype}"
                    bo.check(label, gx, dw, db, ref, dtype)
                    if skip:
                        _class_rows_pass_through(gx, gi, label)
    assert forms == {(3, 1), (3, 2), (3, 3), (3, 4)} == {f for f in lo.forms_that_exist("add_layernorm")}


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_gradients_on_launches_whose_workgroups_walk_several_slabs(dtype):
    """11 x 1499 = 16489 rows: more than 512 workgroups' worth at every width, so every wave walks 2 .. 17 slabs and the
    last workgroups run out of rows part-way."""
    _abi = _mods()[0]
    for C in (8, 64, 96, 200, 384, 392, 768, 1024):
        assert bo.form(11 * 1499, C)[1] >= 2
        for skip, with_in in ((False, True), (True, False), (True, True)):
            gy, xs, gi, w = bo.make_inputs((11, 1499, C), dtype, 31 * C + skip, far=True, skip_first=skip, with_in=with_in)
            ref = bo.reference(gy, xs, gi, w, EPS, skip_first=skip)
            for params in (False, True):
                gx, dw, db = _run(_abi, gy, xs, gi, w, skip, params)
                bo.check(f"long C={C} skip={skip} gx_in={with_in} params={params} {dtype}", gx, dw, db, ref, dtype)
                if skip:
                    _class_rows_pass_through(gx, gi, f"long C={C}")


def test_bits_are_the_same_on_every_run_and_frozen_norms_need_no_workspace(monkeypatch):
    _abi = _mods()[0]
    for C, shape in ((96, (5, 77)), (768, (9, 1201)), (1024, (2, 333))):
        gy, xs, gi, w = bo.make_inputs((*shape, C), torch.bfloat16, C, skip_first=True)
        a = _run(_abi, gy, xs, gi, w, True, True)
        b = _run(_abi, gy, xs, gi, w, True, True)
        for ta, tb in zip(a, b):
            assert torch.equal(ta.view(torch.int16), tb.view(torch.int16))
        asked = []
        orig = _abi._workspace
        monkeypatch.setattr(_abi, "_workspace", lambda *args: asked.append(args) or orig(*args))
        gx, dw, db = _run(_abi, gy, xs, gi, w, True, False)
        monkeypatch.setattr(_abi, "_workspace", orig)
        assert not asked and dw is None and db is None
        assert torch.equal(gx.view(torch.int16), a[0].view(torch.int16)), "gx must not depend on the parameter work"


def _norm(C, dtype, bias=True, cls=torch.nn.LayerNorm):
    torch.manual_seed(C)
    n = cls(C, eps=EPS, bias=bias) if not bias else cls(C, eps=EPS)
    with torch.no_grad():
        n.weight.add_(0.1 * torch.randn(C))
        if bias:
            n.bias.add_(0.1 * torch.randn(C))
    return n.to(DEV).to(dtype)


def test_functions_give_both_inputs_one_gradient_and_refuse_double_backward():
    _abi, _ln, _, _ = _mods()
    C = 96
    norm = _norm(C, torch.bfloat16)
    gy, xs, gi, _ = bo.make_inputs((3, 37, C), torch.bfloat16, 5)
    x = xs.to(DEV).requires_grad_(True)
    a = (0.5 * gi).to(DEV).requires_grad_(True)
    x_out, y = _ln.add_layernorm_native(x, a, norm)
    assert type(x_out.grad_fn).__name__ == "_AddLayerNormFunctionBackward" and y.grad_fn is x_out.grad_fn
    fx, fy = _abi.add_layernorm(x.detach(), a.detach(), norm.weight, norm.bias, norm.eps)
    assert torch.equal(x_out, fx) and torch.equal(y, fy), "forward = the inference kernel"
    (x_out * gi.to(DEV)).sum().backward(retain_graph=False, inputs=[x, a], create_graph=False)
    only_stream = x.grad.clone()
    assert torch.equal(only_stream, gi.to(DEV)) and torch.equal(a.grad, only_stream)  # y unused: the stream's gradient
    x.grad = a.grad = None
    x_out, y = _ln.add_layernorm_native(x, a, norm)
    ((x_out * gi.to(DEV)).sum() + (y * gy.to(DEV)).sum()).backward()
    assert torch.equal(x.grad, a.grad)
    ref = bo.reference(gy, x_out.detach(), gi, norm.weight, EPS)
    bo.check("add_layernorm_native", x.grad, norm.weight.grad, norm.bias.grad, ref, torch.bfloat16)
    # direct calls of the inference entry on tensors that require grad: as before, no graph
    assert _abi.add_layernorm(x, a, norm.weight, norm.bias, norm.eps)[1].grad_fn is None
    x2 = xs.to(DEV).requires_grad_(True)
    y2 = _ln.layernorm_native(x2, norm)
    (g,) = torch.autograd.grad(y2.square().sum(), x2, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_routing(monkeypatch):
    """The helpers of tome/patch/_common.py take the native Functions exactly when ln_trainable holds, the flags are on
    and the tokens require grad; everything else takes the framework's ops and still has a finite gradient."""
    _abi, _ln, M, common = _mods()

    class Sub(torch.nn.LayerNorm):
        pass

    class Blk:
        training = True
    bf = torch.bfloat16

    def grads(x, norm, expect_native, residual=False):
        blk = Blk()
        object.__setattr__(blk, "_tome_next_norm", norm)
        x = x.clone().requires_grad_(True)
        info = {}
        if residual:
            out = common.finish_block(blk, x, torch.ones_like(x), info)
            y = common.first_norm(blk, out, info, norm)
            fn = type(out.grad_fn).__name__
            want = "_AddLayerNormFunctionBackward"
        else:
            y = common.first_norm(blk, x, info, norm)
            fn = type(y.grad_fn).__name__
            want = "_LayerNormFunctionBackward"
        assert (fn == want) == expect_native, (fn, expect_native)
        y.float().square().sum().backward()
        assert torch.isfinite(x.grad).all() and norm.weight.grad is not None
        norm.weight.grad = None
        t = common._trailing_norm(x, norm)
        assert (type(t.grad_fn).__name__ == "_LayerNormFunctionBackward") == expect_native

    x96 = torch.randn(2, 9, 96, device=DEV)
    for residual in (False, True):
        grads(x96.to(bf), _norm(96, bf), True, residual)
        grads(x96.to(torch.float16), _norm(96, torch.float16), True, residual)
        grads(x96, _norm(96, torch.float32), False, residual)                                   # fp32 tokens
        grads(torch.randn(2, 9, 100, device=DEV).to(bf), _norm(100, bf), False, residual)       # C % 8 != 0
        grads(torch.randn(2, 9, 1032, device=DEV).to(bf), _norm(1032, bf), False, residual)     # C > 1024
        grads(x96.to(bf), _norm(96, bf, cls=Sub), False, residual)                              # a LayerNorm subclass
        grads(x96.to(bf), _norm(96, bf, bias=False), False, residual)                           # no bias
        monkeypatch.setattr(_ln, "NATIVE_LN_BACKWARD", False)
        grads(x96.to(bf), _norm(96, bf), False, residual)                                       # the flag off
        monkeypatch.setattr(_ln, "NATIVE_LN_BACKWARD", True)
        monkeypatch.setattr(M, "NATIVE_BACKWARD", False)
        grads(x96.to(bf), _norm(96, bf), False, residual)                                       # the merge flag off
        monkeypatch.setattr(M, "NATIVE_BACKWARD", True)
    monkeypatch.setattr(common, "_FUSE_NEXT", False)                                            # TOME_FUSE_NEXT=0
    blk = Blk()
    norm = _norm(96, bf)
    object.__setattr__(blk, "_tome_next_norm", norm)
    x = x96.to(bf).requires_grad_(True)
    out = common.finish_block(blk, x, torch.ones_like(x), {})
    y = common.first_norm(blk, out, {}, norm)
    assert "LayerNormFunction" not in type(out.grad_fn).__name__ + type(y.grad_fn).__name__
    y.float().sum().backward()
    assert torch.isfinite(x.grad).all()
    # tokens without grad: the inference launch, no graph
    monkeypatch.setattr(common, "_FUSE_NEXT", True)
    with torch.no_grad():
        assert common.first_norm(blk, x96.to(bf), {}, norm).grad_fn is None


def test_finish_block_keeps_the_gradient_of_a_residual_that_alone_requires_grad():
    _, _, _, common = _mods()
    bf = torch.bfloat16
    norm = _norm(96, bf).requires_grad_(False)

    class Blk:
        training = True
    blk = Blk()
    object.__setattr__(blk, "_tome_next_norm", norm)

    def run(x, residual):
        info = {}
        out = common.finish_block(blk, x, residual, info)
        return out, common.first_norm(blk, out, info, norm)

    gen = torch.Generator().manual_seed(5)
    bo.residual_gradient_survives(run, torch.randn(2, 9, 96, generator=gen).to(bf).to(DEV),
                                  torch.randn(2, 9, 96, generator=gen).to(bf).to(DEV), DEV)


def test_merge_then_norm_keeps_the_gradient_of_a_residual_that_alone_requires_grad():
    """[2, 8, 96], r = 2, the VideoMAE patch's merge function: the fused merge + LayerNorm launch is inference-only, a
    residual that requires grad takes the unfused steps (add, merge_wavg as a Function, the trailing norm)."""
    _, _, _, common = _mods()
    from tome.patch.videomae import videomae_merge
    bf = torch.bfloat16
    norm = _norm(96, bf).requires_grad_(False)
    gen = torch.Generator().manual_seed(6)
    metric = torch.randn(2, 8, 32, generator=gen).to(DEV)

    def run(x, residual):
        info = common.new_tome_info(False, True, "merge", "mean", 0.0, False, False)
        info["r"] = [2]
        out, y = common.merge_then_norm(metric, x, info, norm, videomae_merge, videomae_merge, residual=residual)
        assert out.shape == (2, 6, 96) and not info["r"]
        return out, y

    bo.residual_gradient_survives(run, torch.randn(2, 8, 96, generator=gen).to(bf).to(DEV),
                                  torch.randn(2, 8, 96, generator=gen).to(bf).to(DEV), DEV)


def test_a_bias_that_alone_requires_grad_gets_its_gradient():
    """x without grad, the weight frozen, norm.bias alone requires grad (bias-only fine-tuning): first_norm takes the
    Function, and dbias is inside the bound ln_bwd_oracle.check applies to it."""
    _, _, _, common = _mods()
    bf = torch.bfloat16
    gy, xs, _, _ = bo.make_inputs((2, 9, 96), bf, 17, with_in=False)
    norm = _norm(96, bf)
    norm.weight.requires_grad_(False)
    y = common.first_norm(None, xs.to(DEV), {}, norm)
    assert type(y.grad_fn).__name__ == "_LayerNormFunctionBackward", y.grad_fn
    y.backward(gy.to(DEV))
    assert norm.bias.grad is not None and norm.weight.grad is None
    ref = bo.reference(gy, xs, None, norm.weight, EPS)
    bad, worst = bo.outside_param(norm.bias.grad, ref, "db", bf)
    print(f"bias alone: dbias worst err/bound {worst:.3f}")
    assert not bool(bad.any()), (int(bad.sum()), worst)


def test_a_weight_that_alone_requires_grad_gets_its_gradient():
    """The twin: x without grad, the bias frozen, norm.weight alone requires grad.  The parent took the framework's
    LayerNorm here; asking every participant once gives the Function, and dweight is inside ln_bwd_oracle's bound."""
    _, _, _, common = _mods()
    bf = torch.bfloat16
    gy, xs, _, _ = bo.make_inputs((2, 9, 96), bf, 19, with_in=False)
    norm = _norm(96, bf)
    norm.bias.requires_grad_(False)
    y = common.first_norm(None, xs.to(DEV), {}, norm)
    assert type(y.grad_fn).__name__ == "_LayerNormFunctionBackward", y.grad_fn
    y.backward(gy.to(DEV))
    assert norm.weight.grad is not None and norm.bias.grad is None
    ref = bo.reference(gy, xs, None, norm.weight, EPS)
    bad, worst = bo.outside_param(norm.weight.grad, ref, "dw", bf)
    print(f"weight alone: dweight worst err/bound {worst:.3f}")
    assert not bool(bad.any()), (int(bad.sum()), worst)


def _train_hosts():
    import tome
    from hosts import timesformer, videomae
    return (
        ("videomae", lambda: videomae.VideoMAE(num_frames=8, img_size=64, patch_size=16, embed_dim=64, depth=3,
                                               num_heads=1, num_classes=9), (2, 3, 8, 64, 64), tome.patch.videomae),
        ("timesformer", lambda: timesformer.TimeSformer(num_frames=4, img_size=64, patch_size=8, embed_dim=64, depth=3,
                                                        num_heads=1, num_classes=9), (2, 3, 4, 64, 64),
         tome.patch.timesformer))


def _model(which):
    name, make, clip_shape, patch = _train_hosts()[which]
    torch.manual_seed(0)
    model = make().to(DEV).to(torch.bfloat16).train()
    patch(model)
    clip = torch.rand(*clip_shape, generator=torch.Generator().manual_seed(3)).to(DEV).to(torch.bfloat16)
    return name, model, clip


@pytest.mark.parametrize("which", [0, 1], ids=["videomae", "timesformer"])
def test_patched_model_trains_through_the_layernorm_kernels(which, monkeypatch):
    """bf16, .train(), model.r = 6: one tome_layernorm_backward launch per LayerNorm the wiring covers -- VideoMAE:
    norm1 and norm2 of each of the 3 blocks = 6; TimeSformer: temporal_norm1 and norm2 of each block = 6 (norm1 sits
    behind add_layernorm_regrouped, which keeps the reference's ops under grad) -- finite gradients everywhere, every
    qkv / mlp / norm parameter of the blocks has one."""
    _abi, _ln, M, _ = _mods()
    name, model, clip = _model(which)
    calls = []
    orig = _abi.layernorm_backward
    monkeypatch.setattr(_abi, "layernorm_backward", lambda *a, **kw: calls.append(kw.get("skip_first")) or orig(*a, **kw))
    model.r = 6
    out = model([clip])
    out.float().square().sum().backward()
    assert len(calls) == 6, (name, calls)
    if name == "timesformer":
        assert sum(bool(c) for c in calls) == 3, calls  # temporal_norm1 reads the patch rows only
    grads = {k: q.grad for k, q in model.named_parameters()}
    assert not [k for k, q in grads.items() if q is not None and not torch.isfinite(q).all()]
    assert not [k for k, q in grads.items() if q is None and "blocks" in k and ("qkv" in k or "mlp" in k or "norm" in k)]
    calls.clear()
    monkeypatch.setattr(_ln, "NATIVE_LN_BACKWARD", False)
    model.zero_grad(set_to_none=True)
    model([clip]).float().square().sum().backward()
    assert not calls, "the framework path must not launch the backward kernel"


def _framework_backward(gy, xs, gx_in, weight, eps, skip_first, want_weight, want_bias):
    """The framework's LayerNorm backward on the same saved tensors, and its separate add for the residual stream."""
    C = xs.shape[-1]
    if skip_first:
        full = torch.zeros_like(xs)
        full[:, 1:] = gy
        gy = full
    _, mean, rstd = torch.native_layer_norm(xs, [C], weight, torch.zeros_like(weight), eps)
    gx, dw, db = torch.ops.aten.native_layer_norm_backward(gy.contiguous(), xs, [C], mean, rstd, weight,
                                                           torch.zeros_like(weight), [True, want_weight, want_bias])
    if gx_in is not None:
        gx = gx + gx_in
    return gx, (dw if want_weight else None), (db if want_bias else None)


def _oracle_backward(gy, xs, gx_in, weight, eps, skip_first, want_weight, want_bias):
    """The fp64 reference, cast once to the token dtype."""
    ref = bo.reference(gy, xs, gx_in, weight, eps, skip_first=skip_first)
    cast = lambda t: t.to(xs.dtype).to(xs.device)  # noqa: E731
    return (cast(ref["gx"]).reshape(xs.shape), cast(ref["dw"]) if want_weight else None,
            cast(ref["db"]) if want_bias else None)


@pytest.mark.parametrize("which", [0, 1], ids=["videomae", "timesformer"])
def test_model_gradients_against_the_framework_and_the_oracle(which, monkeypatch):
    """model.r = [6, 0, 0], three runs with the same native forward (logits and matchings bit-identical, asserted) and
    three evaluations of the LayerNorm backward on the same saved tensors: (a) the kernel, (b) the framework's
    native_layer_norm_backward, (c) the fp64 reference cast once to bf16.  Per parameter, scaled by its largest
    gradient in (c): err(a, c) <= 2 err(b, c) + 2^-8 -- (a) and (b) are two single-precision evaluations of one
    formula with one 16-bit rounding each, the floor is one such rounding, the bound comes from (c)."""
    _abi, _ln, M, _ = _mods()
    name, model, clip = _model(which)
    plans = []
    make_pair = M._make_merge_pair
    monkeypatch.setattr(M, "_make_merge_pair", lambda plan: plans.append(plan) or make_pair(plan))
    native = _ln.ln_backward
    used = []

    def run(fn):
        monkeypatch.setattr(_ln, "ln_backward", lambda *a: used.append(fn) or fn(*a))
        plans.clear()
        model.zero_grad(set_to_none=True)
        model.r = [6, 0, 0]
        torch.manual_seed(1)
        out = model([clip])
        out.float().square().sum().backward()
        idx = [(p.src_idx.clone(), p.dst_idx.clone(), p.unm_idx.clone()) for p in plans]
        return out.detach().clone(), idx, {k: q.grad.detach().double().cpu() for k, q in model.named_parameters()
                                           if q.grad is not None}

    oa, ia, ga = run(native)
    ob, ib, gb = run(_framework_backward)
    oc, ic, gc = run(_oracle_backward)
    assert len(used) == 18 and used.count(native) == 6, len(used)
    assert torch.equal(oa, ob) and torch.equal(oa, oc), "the three runs must share one forward"
    assert len(ia) >= 1 and len(ia) == len(ib) == len(ic)
    for pa, pb, pc in zip(ia, ib, ic):
        for ta, tb, tc in zip(pa, pb, pc):
            assert torch.equal(ta, tb) and torch.equal(ta, tc), "the three runs must merge the same tokens"
    assert ga.keys() == gb.keys() == gc.keys()
    bad, worst_a, worst_b = [], 0.0, 0.0
    for k in ga:
        scale = gc[k].abs().max().item()
        if scale == 0.0:
            assert ga[k].abs().max().item() == 0.0, k
            continue
        ea = (ga[k] - gc[k]).abs().max().item() / scale
        eb = (gb[k] - gc[k]).abs().max().item() / scale
        worst_a, worst_b = max(worst_a, ea), max(worst_b, eb)
        if not ea <= 2 * eb + 2.0 ** -8:
            bad.append((k, ea, eb))
    print(f"{name}: worst scaled gradient error kernel vs oracle {worst_a:.3e}, framework vs oracle {worst_b:.3e}")
    assert not bad, bad
