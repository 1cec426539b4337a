"""tome_prop_attention_backward on the GPU: every element of dq, dk, dv inside the component-wise bound of
attn_bwd_oracle.py (fp64 reference of the reference's op sequence), the kernels' properties (same bits on every run,
strided targets, workspace), the routing of tome/patch/_common.py:attention, and the gradients of patched models
against the framework path and an fp32 run."""
import copy

import pytest
import torch

import attn_bwd_oracle as ao

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]


def _mods():
    import tome
    from tome import _abi, _attn, merge as M
    from tome.patch import _common as common
    return tome, _abi, _attn, M, common


def _to_dev(inp: ao.Inputs) -> ao.Inputs:
    if inp.qkv is not None:
        qkv = inp.qkv.to(DEV)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    else:
        qkv, q, k, v = None, inp.q.to(DEV), inp.k.to(DEV), inp.v.to(DEV)
    lb = None if inp.log_bias is None else inp.log_bias.to(DEV)
    return ao.Inputs(q, k, v, inp.dout.to(DEV), lb, inp.skip, inp.scale, qkv)


def _native(_abi, d: ao.Inputs, **kw):
    """Forward launch + backward launch on the device inputs -> dict of [B, H, *, 64] gradients."""
    out = _abi.prop_attention(d.q, d.k, d.v, None, d.scale, bias_skip=d.skip, log_bias=d.log_bias)
    dq, dk, dv = _abi.prop_attention_backward(d.q, d.k, d.v, out, d.dout, d.log_bias, d.scale, bias_skip=d.skip, **kw)
    return dict(dq=dq, dk=dk, dv=dv)


def _case(_abi, label, B, H, N, Nk, dtype, bias, layout, seed=1, **kw):
    inp = ao.make_inputs(B, H, N, Nk, dtype, seed, bias=bias, layout=layout, **kw)
    got = _native(_abi, _to_dev(inp))
    torch.cuda.synchronize()
    ref = ao.reference(inp)
    return ao.check(f"{label} {B}x{H}x{N}x{Nk} {bias} {layout} {dtype}", got, ref, ao.bounds(ref, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N", [8, 63, 64, 65, 197, 392, 1472, 1568, 3137])
def test_gradients_inside_the_bound_at_every_length(N, dtype):
    """N = Nk; q/k/v as slices of a qkv buffer and as separate tensors; with bias, without, skip form.  Every element."""
    _, _abi, _, _, _ = _mods()
    B, H = (2, 3) if N <= 392 else ((1, 2) if N < 3137 else (1, 1))
    combos = [("bias", "qkv"), ("none", "separate"), ("skip", "qkv")]
    if N <= 392:
        combos += [("bias", "separate"), ("none", "qkv"), ("skip", "separate")]
    for bias, layout in combos:
        _case(_abi, "length", B, H, N, N, dtype, bias, layout, seed=N)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(1, 197), (1568, 784)], ids=["1x197", "1568x784"])
def test_gradients_with_other_numbers_of_keys_than_queries(shape, dtype):
    _, _abi, _, _, _ = _mods()
    N, Nk = shape
    for bias in ("bias", "none"):
        _case(_abi, "N != Nk", 1, 2, N, Nk, dtype, bias, "separate", seed=7)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_gradients_where_the_row_maximum_matters(dtype):
    """Logits 8x larger, sizes up to 64; and the family with a common mean in v and dout (delta large)."""
    _, _abi, _, _, _ = _mods()
    for N in (197, 392):
        _case(_abi, "gain 8", 1, 2, N, N, dtype, "bias", "qkv", seed=3, logit_gain=8.0, max_size=64)
        _case(_abi, "gain 8", 1, 2, N, N, dtype, "skip", "separate", seed=4, logit_gain=8.0, max_size=64)
    _case(_abi, "offset", 1, 2, 197, 197, dtype, "bias", "qkv", seed=5, offset=2.0)


def test_bits_strides_and_workspace():
    _, _abi, _, _, _ = _mods()
    inp = ao.make_inputs(2, 3, 197, 197, torch.bfloat16, 21, bias="skip", layout="qkv")
    d = _to_dev(inp)
    a = _native(_abi, d)
    b = _native(_abi, d)
    for n in a:
        assert torch.equal(a[n], b[n]), f"{n}: bits differ between two runs"
    # gradients through strides: the three slices of one [B, N, 3, H, 80] buffer -- only the 64 channels are written
    B, H, N = 2, 3, 197
    buf = torch.full((B, N, 3, H, 80), 7.0, dtype=torch.bfloat16, device=DEV)
    g = buf.permute(2, 0, 3, 1, 4)[..., :64]
    c = _native(_abi, d, grads=(g[0], g[1], g[2]))
    torch.cuda.synchronize()
    for i, n in enumerate(("dq", "dk", "dv")):
        assert c[n].data_ptr() == g[i].data_ptr()
        assert torch.equal(g[i], a[n]), f"{n}: strided target differs"
    assert bool((buf[..., 64:] == 7.0).all()), "bytes between the slices were touched"
    # workspace: the stated size is enough, anything smaller is refused before a launch
    L = _abi.lib()
    need = L.tome_prop_attention_backward_workspace_bytes(B, H, N, N)
    assert need >= 2 * 4 * B * H * N and need % 256 == 0
    assert L.tome_prop_attention_backward_workspace_bytes(0, H, N, N) == 0
    guard = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    e = _native(_abi, d, workspace=guard[:need])
    torch.cuda.synchronize()
    assert bool((guard[need:] == 0x5A).all()), "wrote past workspace_bytes"
    for n in a:
        assert torch.equal(a[n], e[n])
    with pytest.raises(_abi.TomeHipError, match="status 2"):
        _native(_abi, d, workspace=guard[:need - 256])


def test_routing(monkeypatch):
    _, _abi, _attn, M, common = _mods()
    bf = torch.bfloat16

    def heads(dtype=bf, hd=64, grad=True):
        qkv = torch.randn(2, 70, 3, 2, hd, device=DEV).to(dtype).requires_grad_(grad)
        return qkv, qkv.permute(2, 0, 3, 1, 4)

    size = torch.randint(1, 5, (2, 70, 1), device=DEV).to(bf)
    qkv, p = heads()
    out = common.attention(p[0], p[1], p[2], size, 0.125)
    assert type(out.grad_fn).__name__ == "_AttentionFunctionBackward", out.grad_fn
    out.float().square().sum().backward()
    g_native = qkv.grad.clone()
    assert torch.isfinite(g_native).all() and float(g_native.abs().max()) > 0
    # the qkv form: one input, one gradient buffer, same bits as three slices
    qkv2, p2 = heads()
    with torch.no_grad():
        qkv2.copy_(qkv)
    out2 = common.attention_qkv(p2, size, 0.125)
    assert type(out2.grad_fn).__name__ == "_AttentionQKVFunctionBackward", out2.grad_fn
    assert torch.equal(out2, out)
    out2.float().square().sum().backward()
    assert torch.equal(qkv2.grad, g_native)
    # double backward raises
    qkv3, p3 = heads()
    o3 = common.attention(p3[0], p3[1], p3[2], None, 0.125)
    (g3,) = torch.autograd.grad(o3.float().sum(), qkv3, create_graph=True)
    with pytest.raises(RuntimeError):
        g3.sum().backward()

    def falls_back(*args, **kw):
        q4, p4 = kw.pop("hp", None) or heads()
        o = common.attention(p4[0], p4[1], p4[2], *args, **kw)
        assert o.grad_fn is not None and type(o.grad_fn).__name__ not in (
            "_AttentionFunctionBackward", "_AttentionQKVFunctionBackward"), o.grad_fn
        o.float().square().sum().backward()
        assert q4.grad is not None and torch.isfinite(q4.grad).all()
        return q4.grad

    # the switches
    monkeypatch.setattr(_attn, "NATIVE_ATTN_BACKWARD", False)
    qkv5, p5 = heads()
    with torch.no_grad():
        qkv5.copy_(qkv)
    g_fw = falls_back(size, 0.125, hp=(qkv5, p5))
    monkeypatch.setattr(_attn, "NATIVE_ATTN_BACKWARD", True)
    monkeypatch.setattr(M, "NATIVE_BACKWARD", False)
    falls_back(size, 0.125)
    monkeypatch.setattr(M, "NATIVE_BACKWARD", True)
    # native and framework gradients agree to 16-bit accuracy
    scale = float(g_fw.float().abs().max())
    assert float((g_native.float() - g_fw.float()).abs().max()) <= 0.05 * scale
    # each excluded case
    falls_back(size, 0.125, 0.1)                                   # dropout
    falls_back(size.float(), 0.125, hp=heads(torch.float32))       # fp32 heads
    falls_back(size, 0.125, hp=heads(hd=32))                       # head dim
    # no_grad: the inference launch, no Function, no backward launch
    calls = []
    orig = _abi.prop_attention
    monkeypatch.setattr(_abi, "prop_attention", lambda *a, **kw: calls.append(kw) or orig(*a, **kw))
    monkeypatch.setattr(_abi, "prop_attention_backward", lambda *a, **kw: pytest.fail("backward launch under no_grad"))
    with torch.no_grad():
        qn, pn = heads()
        o = common.attention(pn[0], pn[1], pn[2], size, 0.125)
        o2 = common.attention_qkv(pn, size, 0.125)
    assert o.grad_fn is None and o2.grad_fn is None and len(calls) == 2
    assert all(kw.get("checked") and kw.get("log_bias") is None for kw in calls), calls
    assert torch.equal(o, o2)
    # heads that do not require grad, grad enabled: the same inference launch
    qf, pf = heads(grad=False)
    o = common.attention(pf[0], pf[1], pf[2], size, 0.125)
    assert o.grad_fn is None and len(calls) == 3


def _train_hosts():
    import tome
    from hosts import timesformer, videomae, vivit
    return dict(
        videomae=(lambda: videomae.VideoMAE(num_frames=8, img_size=64, patch_size=16, embed_dim=64, depth=3,
                                            num_heads=1, num_classes=9), (2, 3, 8, 64, 64), tome.patch.videomae, 6),
        vivit=(lambda: vivit.ViViT(num_classes=9, image_size=64, num_frames=8, hidden_size=64, num_hidden_layers=3,
                                   num_attention_heads=1, intermediate_size=256), (2, 3, 8, 64, 64), tome.patch.vivit, 6),
        timesformer=(lambda: timesformer.TimeSformer(num_frames=4, img_size=64, patch_size=8, embed_dim=64, depth=3,
                                                     num_heads=1, num_classes=9), (2, 3, 4, 64, 64),
                     tome.patch.timesformer, 6))


@pytest.mark.parametrize("name", ["videomae", "vivit", "timesformer", "videomae/attention only", "vivit/attention only",
                                  "timesformer/attention only"])
def test_patched_model_gradients_native_framework_fp32(name, monkeypatch):
    """Reduced-width model, bf16, prop_attn=True, merging in every block (r = 6), three runs on the same weights:
    (a) native attention backward, (b) the framework path (switch off: the parent commit's behaviour), (c) the framework
    in fp32.  Worst per-parameter gradient error against (c), scaled by that parameter's largest gradient in (c):
    native <= 2 x framework -- both make the same kind and number of 16-bit roundings in a different order.
    A parameter whose largest fp32 gradient is below 1e-6 of the model's largest is left out of the ratio: its gradient
    is zero in exact arithmetic (ViViT's key bias: the softmax does not see a shift common to a row's logits, so dS sums
    to zero over the keys), the fp32 value is rounding noise and would set a scale of ~1e4 under which any attention
    gradient passes; for such a parameter both 16-bit runs must stay below 2^-6 of the model's largest gradient instead
    (the rounding noise of 16-bit sums, not a gradient).  The measured pairs are in DESIGN.md section 2.  What this test
    can and cannot see: the bf16 and fp32 runs may merge different tokens, an error both 16-bit runs share -- VideoMAE's
    pair is equal to four digits for that reason -- so the op-level tests above, not this one, are what holds the
    kernels to their arithmetic.
    ".../attention only": embedding, LayerNorms, MLPs and head frozen, the attention projections alone train (LoRA-style
    fine-tuning) -- block 0 then reads tokens without grad and adds a residual that requires grad to them; every trainable
    parameter of block 0 must get a gradient, under the same bound."""
    _, _abi, _attn, M, _ = _mods()
    name, _, freeze = name.partition("/")
    make, clip_shape, patch, r = _train_hosts()[name]
    torch.manual_seed(0)
    model32 = make().to(DEV).train()
    with torch.no_grad():  # (the hosts initialise some parameters with zeros: every parameter gets a value)
        for prm in model32.parameters():
            if float(prm.abs().max()) == 0.0:
                prm.normal_(0.0, 0.02)
    model16 = copy.deepcopy(model32).to(torch.bfloat16)
    with torch.no_grad():  # the fp32 run starts from the bf16 weights
        for p32, p16 in zip(model32.parameters(), model16.parameters()):
            p32.copy_(p16.float())
    if freeze:
        for model in (model32, model16):
            for k, prm in model.named_parameters():
                prm.requires_grad_("attn." in k or ".attention." in k)
    patch(model16, prop_attn=True)
    patch(model32, prop_attn=True)
    clip = torch.rand(*clip_shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    launches = []
    orig = _abi.prop_attention_backward
    monkeypatch.setattr(_abi, "prop_attention_backward", lambda *a, **kw: launches.append(1) or orig(*a, **kw))

    def run(model, x):
        model.zero_grad(set_to_none=True)
        model.r = r
        out = model([x])
        out.float().square().sum().backward()
        return {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}

    ga = run(model16, clip.to(torch.bfloat16))
    assert len(launches) == 3, f"{name}: {len(launches)} backward launches for 3 blocks"
    monkeypatch.setattr(_attn, "NATIVE_ATTN_BACKWARD", False)
    gb = run(model16, clip.to(torch.bfloat16))
    assert len(launches) == 3
    gc = run(model32, clip)
    assert ga.keys() == gb.keys() == gc.keys()
    if freeze:
        first = [k for k, prm in model16.named_parameters() if prm.requires_grad and (".blocks.0." in k or ".layer.0." in k)]
        assert len(first) >= 4 and not [k for k in first if k not in ga], [k for k in first if k not in ga]
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
    print(f"{name} {freeze}: worst scaled gradient error native vs fp32 {worst_a:.3e}, framework vs fp32 {worst_b:.3e}")
    assert worst_a <= 2 * worst_b, (name, worst_a, worst_b)
