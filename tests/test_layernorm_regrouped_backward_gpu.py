"""Native backward of the regrouped add + LayerNorm (tome_layernorm_backward_regrouped, k_ln_rows_bwd<.., REGROUP>) on
the GPU: every element of gx / dweight / dbias against the fp64 reference and derived bound of
tests/ln_regrouped_bwd_oracle.py at every width and at the shapes where the row map can go wrong, bit-level properties,
the Function of tome/_ln.py and the routing in tome/patch/timesformer.py.  The model-level test of both new entries is
in tests/test_short_attention_backward_gpu.py."""
import pytest
import torch

import ln_bwd_oracle as bo
import ln_oracle as lo
import ln_regrouped_bwd_oracle as ro

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
EPS = 1e-5


def _mods():
    from tome import _abi, _ln
    from tome import merge as M
    from tome.patch import _common
    return _abi, _ln, M, _common


def _run(_abi, gy, xs, gi, w, F, params):
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    gx, dw, db = _abi.layernorm_backward_regrouped(dev(gy), dev(xs), dev(gi), F, dev(w), EPS, want_weight=params,
                                                   want_bias=params)
    assert (dw is None) == (not params) and (db is None) == (not params)
    return gx, dw, db


def _sweep(shape, C, dtype, seed):
    """With and without gx_in, with and without parameter gradients: four launches, each inside the bound, each twice
    with the same bits."""
    _abi = _mods()[0]
    B, F, P = shape
    for with_in in (False, True):
        gy, xs, gi, w = ro.make_inputs(B, F, P, C, dtype, seed + with_in, with_in=with_in, far=(C // 8) % 4 != 0,
                                       grad_scale=1e-3 if (C // 8) % 3 == 0 else 1.0)
        ref = ro.reference(gy, xs, gi, w, EPS, F)
        for params in (False, True):
            got = _run(_abi, gy, xs, gi, w, F, params)
            ro.check(f"{shape} C={C} gx_in={with_in} params={params} {dtype}", *got, ref, dtype)
            again = _run(_abi, gy, xs, gi, w, F, params)
            for a, b in zip(got, again):
                assert a is None or torch.equal(a, b), "bits differ between two runs"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_gradients_at_every_width(dtype):
    """Every C = 8 .. 1024 in steps of 8 at (B, F, P) = (2, 3, 5): 32 rows, every (NIT, R) form of the packing."""
    for C in lo.WIDTHS:
        _sweep((2, 3, 5), C, dtype, 13 * C)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C", [64, 768, 1024])
def test_gradients_at_the_shapes_of_the_row_map(C, dtype):
    """F in {1, 2, 8} x P in {1, 3, 14, 49} x B in {1, 3}, and (4, 8, 128): 4100 rows -- 513 workgroups' worth at
    C = 768 (two rows per wave) and 1025 at C = 1024 (one), against at most 512 partial rows: the waves walk two and
    three slabs."""
    for B in (1, 3):
        for F in (1, 2, 8):
            for P in (1, 3, 14, 49):
                _sweep((B, F, P), C, dtype, 1000 * B + 100 * F + P)
    _sweep((4, 8, 128), C, dtype, 5)


def test_frozen_layernorm_needs_no_workspace_and_bad_shapes_none():
    L = _mods()[0].lib()
    assert L.tome_layernorm_backward_regrouped_workspace_bytes(2, 8, 196, 768) > 0
    for bad in ((0, 8, 196, 768), (2, 0, 196, 768), (2, 8, 0, 768), (2, 8, 196, 12), (2, 8, 196, 1032)):
        assert L.tome_layernorm_backward_regrouped_workspace_bytes(*bad) == 0, bad
    gy, xs, gi, w = (t.to(DEV) for t in ro.make_inputs(2, 3, 5, 64, torch.bfloat16, 1))
    gx = torch.empty_like(xs)
    # frozen: both parameter gradients NULL, workspace NULL -- accepted; wanted without a workspace -- refused
    rc = L.tome_layernorm_backward_regrouped(gy.data_ptr(), xs.data_ptr(), gi.data_ptr(), 1, 2, 3, 5, 64, w.data_ptr(), EPS,
                                             gx.data_ptr(), None, None, None, None)
    assert rc == 0
    dw = torch.empty_like(w)
    rc = L.tome_layernorm_backward_regrouped(gy.data_ptr(), xs.data_ptr(), gi.data_ptr(), 1, 2, 3, 5, 64, w.data_ptr(), EPS,
                                             gx.data_ptr(), dw.data_ptr(), None, None, None)
    assert rc != 0 and L.tome_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_class_rows_without_a_gradient_pass_gx_in_through(dtype):
    """gy = 0 on every class row of every frame, gx_in given: the class rows of gx are gx_in's bits."""
    _abi = _mods()[0]
    B, F, P, C = 3, 8, 14, 768
    gy, xs, gi, w = ro.make_inputs(B, F, P, C, dtype, 31)
    gy[:, 0] = 0
    gx, _, _ = _run(_abi, gy, xs, gi, w, F, True)
    assert torch.equal(gx[:, 0].view(torch.int16), gi[:, 0].to(DEV).view(torch.int16))
    ro.check("zero class gy", gx, None, None, ro.reference(gy, xs, gi, w, EPS, F), dtype)


def _norm(C, dtype, cls=torch.nn.LayerNorm):
    torch.manual_seed(1)
    n = cls(C, eps=EPS).to(DEV).to(dtype)
    with torch.no_grad():
        n.weight.normal_(1.0, 0.1)
        n.bias.normal_(0.0, 0.1)
    return n


def test_function(monkeypatch):
    """x's gradient is gx, the addend's is the view gx[:, 1:]; g_y None passes the stream's gradient through; double
    backward raises."""
    _abi, _ln, _, _ = _mods()
    B, F, P, C = 2, 4, 6, 64
    dtype = torch.bfloat16
    norm = _norm(C, dtype)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, 1 + P * F, C, generator=g).to(dtype).to(DEV).requires_grad_(True)
    rt = torch.randn(B, P * F, C, generator=g).to(dtype).to(DEV).requires_grad_(True)
    g1 = torch.randn(B, 1 + P * F, C, generator=g).to(dtype).to(DEV)
    gy = torch.randn(B * F, 1 + P, C, generator=g).to(dtype).to(DEV)
    x1, y = _ln.add_layernorm_regrouped_native(x, rt, F, norm)
    assert type(x1.grad_fn).__name__ == type(y.grad_fn).__name__ == "_AddLayerNormRegroupedFunctionBackward"
    want1, wanty = _abi.add_layernorm_regrouped(x.detach(), rt.detach(), F, norm.weight, norm.bias, norm.eps)
    assert torch.equal(x1, want1) and torch.equal(y, wanty)
    torch.autograd.backward((x1, y), (g1, gy))
    gx, dw, db = _abi.layernorm_backward_regrouped(gy, want1, g1, F, norm.weight, EPS)
    assert torch.equal(x.grad, gx) and torch.equal(rt.grad, gx[:, 1:])
    assert torch.equal(norm.weight.grad, dw) and torch.equal(norm.bias.grad, db)
    ro.check("function", x.grad, norm.weight.grad, norm.bias.grad,
             ro.reference(gy, want1, g1, norm.weight, EPS, F), dtype)
    # nothing read the LayerNorm: the stream's gradient passes through, no launch
    calls = []
    orig = _ln.ln_backward_regrouped
    monkeypatch.setattr(_ln, "ln_backward_regrouped", lambda *a, **kw: calls.append(1) or orig(*a, **kw))
    x.grad = rt.grad = None
    norm.zero_grad(set_to_none=True)
    x1, y = _ln.add_layernorm_regrouped_native(x, rt, F, norm)
    x1.backward(g1)
    assert not calls and torch.equal(x.grad, g1) and torch.equal(rt.grad, g1[:, 1:])
    assert float(norm.weight.grad.abs().max()) == 0.0 and float(norm.bias.grad.abs().max()) == 0.0
    x1, y = _ln.add_layernorm_regrouped_native(x, rt, F, norm)
    (gg,) = torch.autograd.grad(y.float().sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gg.float().sum().backward()


def test_routing_in_the_block(monkeypatch):
    """_block_forward takes the Function under grad; the reference's ops with each switch off, with TOME_FUSE_NEXT off,
    with fp32 tokens and with a LayerNorm subclass; the inference launch without grad."""
    import tome
    from hosts import timesformer
    _abi, _ln, M, common = _mods()
    seen = []
    orig = _ln.add_layernorm_regrouped_native
    monkeypatch.setattr(_ln, "add_layernorm_regrouped_native",
                        lambda *a, **kw: seen.append(type((r := orig(*a, **kw))[1].grad_fn).__name__) or r)

    def model(dtype=torch.bfloat16):
        torch.manual_seed(0)
        m = timesformer.TimeSformer(num_frames=4, img_size=64, patch_size=8, embed_dim=64, depth=2, num_heads=1,
                                    num_classes=9).to(DEV).to(dtype).train()
        tome.patch.timesformer(m)
        m.r = 6
        return m

    clip = torch.rand(2, 3, 4, 64, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
    m = model()
    m([clip.to(torch.bfloat16)]).float().sum().backward()
    assert seen == ["_AddLayerNormRegroupedFunctionBackward"] * 2
    assert all(torch.isfinite(b.norm1.weight.grad).all() for b in m.model.blocks)
    seen.clear()
    with torch.no_grad():
        m([clip.to(torch.bfloat16)])
    assert not seen
    for mod, attr in ((_ln, "NATIVE_LN_REGROUPED_BACKWARD"), (_ln, "NATIVE_LN_BACKWARD"), (M, "NATIVE_BACKWARD"),
                      (common, "_FUSE_NEXT")):
        monkeypatch.setattr(mod, attr, False)
        m.zero_grad(set_to_none=True)
        m([clip.to(torch.bfloat16)]).float().sum().backward()
        assert not seen, attr
        assert all(torch.isfinite(b.norm1.weight.grad).all() for b in m.model.blocks), attr
        monkeypatch.setattr(mod, attr, True)
    m32 = model(torch.float32)
    m32([clip]).float().sum().backward()
    assert not seen, "fp32 tokens"

    class MyNorm(torch.nn.LayerNorm):
        pass

    for b in m.model.blocks:
        b.norm1.__class__ = MyNorm
    m.zero_grad(set_to_none=True)
    m([clip.to(torch.bfloat16)]).float().sum().backward()
    assert not seen, "a LayerNorm subclass keeps its own forward"


def test_merge_then_norm_regrouped_keeps_the_gradient_of_a_residual_that_alone_requires_grad():
    """B = 2, F = 2, P = 4, r = 1, TimeSformer's merge function: the fused regrouped merge + LayerNorm launch is
    inference-only, a residual that requires grad takes the unfused steps."""
    _, _, _, common = _mods()
    from tome.patch.timesformer import timesformer_merge
    B, F, P, C = 2, 2, 4, 96
    dtype = torch.bfloat16
    norm = _norm(C, dtype).requires_grad_(False)
    gen = torch.Generator().manual_seed(7)
    metric = torch.randn(B * F, P, 32, generator=gen).to(DEV)

    def run(x, residual):
        info = common.new_tome_info(False, True, "merge", "mean", 0.0, False, False)
        info["r"] = [1]
        out, y = common.merge_then_norm_regrouped(metric, x, info, norm,
                                                  lambda z: timesformer_merge(metric, z, info, B, F, P), True, F,
                                                  residual=residual)
        assert out.shape == (B, 1 + (P - 1) * F, C) and not info["r"]
        return out, y

    bo.residual_gradient_survives(run, torch.randn(B, 1 + P * F, C, generator=gen).to(dtype).to(DEV),
                                  torch.randn(B, 1 + P * F, C, generator=gen).to(dtype).to(DEV), DEV)


def test_mid_block_step_keeps_the_gradient_of_an_addend_that_alone_requires_grad():
    """TimeSformer's mid-block step as the patched block calls it (tome/patch/timesformer.py::_block_forward, r = 1):
    the tokens without grad, every parameter frozen, and a tensor that requires grad added to temporal_fc's output -- so
    the temporal residual alone requires grad where the block adds it."""
    import tome
    from hosts import timesformer
    B, F, P, C = 2, 2, 4, 96
    torch.manual_seed(0)
    model = timesformer.TimeSformer(num_frames=F, img_size=16, patch_size=8, embed_dim=C, depth=1, num_heads=1,
                                    num_classes=3).to(DEV).to(torch.bfloat16).eval()
    tome.patch.timesformer(model)
    block = model.model.blocks[0]
    model.requires_grad_(False)

    def run(x, rt_offset):
        model._tome_info.update(r=[1], size=None, source=None)
        model._tome_info.pop("_prenorm", None)
        model._tome_info.pop("_folded", None)
        hook = block.temporal_fc.register_forward_hook(lambda m, i, o: o + rt_offset.reshape(B, P * F, C))
        try:
            return (block(x, B, F, 2),)
        finally:
            hook.remove()

    gen = torch.Generator().manual_seed(8)
    bo.residual_gradient_survives(run, torch.randn(B, 1 + P * F, C, generator=gen).to(torch.bfloat16).to(DEV),
                                  torch.zeros(B, P * F, C, dtype=torch.bfloat16, device=DEV), DEV)
