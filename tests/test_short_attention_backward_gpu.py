"""Native backward of the short attention (tome_short_attention_backward, k_short_attention_bwd) on the GPU: every
element of dq, dk, dv against the fp64 reference and derived bound of tests/short_attn_bwd_oracle.py, what the launch
writes and leaves alone, refusals, the Function of tome/_attn.py, the routing in hosts/timesformer.py, and a patched
TimeSformer that trains through both new backward entries."""
import copy
import ctypes

import pytest
import torch

import short_attn_bwd_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]


def _mods():
    from tome import _abi, _attn, _ln
    from tome import merge as M
    return _abi, _attn, _ln, M


def _targets(inp, how):
    """dq, dk, dv head views: the slices of one NaN-filled [B, N, 3, H, 64] buffer, or three NaN-filled tensors."""
    B, H, N, D = inp.q.shape
    if how == "one":
        buf = torch.full((B, N, 3, H, D), float("nan"), dtype=inp.q.dtype, device=DEV)
        return tuple(buf[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    return tuple(torch.full((B, N, H, D), float("nan"), dtype=inp.q.dtype, device=DEV).permute(0, 2, 1, 3) for _ in range(3))


def _launch(_abi, inp, how):
    dq, dk, dv = _abi.short_attention_backward(inp.q, inp.k, inp.v, inp.dout, inp.scale, grads=_targets(inp, how))
    return dict(dq=dq, dk=dk, dv=dv)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_every_element_inside_the_bound(dtype):
    """Every N in 1..8, H in {1, 3, 12}, B*H in {1, 31, 33, 65} units (one below and above a workgroup's 32, above two),
    sources as slices of one qkv buffer and as separate tensors, targets in one buffer and in three, pre-filled with NaN:
    every element finite afterwards and inside the bound, two runs the same bits."""
    _abi = _mods()[0]
    units = set()
    shapes = [(1, 1), (31, 1), (33, 1), (65, 1), (11, 3), (3, 12)]
    for N in range(1, 9):
        for B, H in shapes:
            units.add(B * H)
            layout, how = (("qkv", "one"), ("separate", "three"), ("qkv", "three"), ("separate", "one"))[(N + B) % 4]
            inp = so.make_inputs(B, H, N, dtype, 1000 * N + 10 * B + H, layout=layout, device=DEV)
            got = _launch(_abi, inp, how)
            for n, t in got.items():
                assert torch.isfinite(t).all(), f"N={N} B={B} H={H} {n}: an element was not written"
            so.check(f"N={N} B={B} H={H} {layout}->{how} {dtype}", got, so.reference(inp), dtype)
            again = _launch(_abi, inp, how)
            for n in got:
                assert torch.equal(got[n], again[n]), f"{n}: bits differ between two runs"
    assert {1, 31, 33, 65} <= units


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rows_whose_maximum_matters(dtype):
    """q scaled by 8: logits of +-30, a softmax that is nearly one-hot; without the row maximum exp2 overflows."""
    _abi = _mods()[0]
    for N in (3, 8):
        inp = so.make_inputs(7, 3, N, dtype, 50 + N, layout="qkv", logit_gain=8.0, device=DEV)
        so.check(f"gain 8 N={N} {dtype}", _launch(_abi, inp, "one"), so.reference(inp), dtype)


def test_memory_beside_the_channels_stays_untouched():
    """Targets whose token rows are 3 * H * 64 + 16 apart inside a buffer of a sentinel value: the 64 channels of every
    head of every row are written, the 16 elements behind each token and everything else keep the sentinel."""
    _abi = _mods()[0]
    B, H, N = 5, 3, 7
    inp = so.make_inputs(B, H, N, torch.bfloat16, 9, layout="separate", device=DEV)
    row = 3 * H * 64 + 16
    buf = torch.full((B, N, row), 7.0, dtype=torch.bfloat16, device=DEV)
    grads = tuple(buf[:, :, i * H * 64:(i + 1) * H * 64].unflatten(2, (H, 64)).permute(0, 2, 1, 3) for i in range(3))
    _abi.short_attention_backward(inp.q, inp.k, inp.v, inp.dout, inp.scale, grads=grads)
    assert (buf[:, :, 3 * H * 64:] == 7.0).all(), "elements behind the channels were written"
    so.check("strided target", dict(zip(("dq", "dk", "dv"), grads)), so.reference(inp), torch.bfloat16)


def test_refusals_launch_nothing():
    """N = 9, D = 32, fp32, head stride != 64, a misaligned pointer, a NULL target: a non-zero status, a message, and
    the NaN-filled targets still all NaN."""
    _abi = _mods()[0]
    L = _abi.lib()
    B, H, N = 2, 3, 8
    inp = so.make_inputs(B, H, N, torch.bfloat16, 1, layout="qkv", device=DEV)
    dq, dk, dv = _targets(inp, "one")
    st = lambda t: (ctypes.c_int64 * 3)(*t.stride()[:3])  # noqa: E731
    bad_head = (ctypes.c_int64 * 3)(inp.q.stride(0), 128, inp.q.stride(2))

    def call(q=inp.q.data_ptr(), dtype=1, N=N, D=64, qs=st(inp.q), dq_ptr=dq.data_ptr()):
        return L.tome_short_attention_backward(q, inp.k.data_ptr(), inp.v.data_ptr(), inp.dout.data_ptr(), dtype, B, H, N,
                                               D, qs, st(inp.k), st(inp.v), 0.125, dq_ptr, dk.data_ptr(), dv.data_ptr(),
                                               st(dq), st(dk), st(dv), None)

    for label, kw in (("N=9", dict(N=9)), ("D=32", dict(D=32)), ("fp32", dict(dtype=0)), ("head stride", dict(qs=bad_head)),
                      ("misaligned", dict(q=inp.q.data_ptr() + 2)), ("NULL target", dict(dq_ptr=None))):
        assert call(**kw) != 0, label
        assert L.tome_last_error(), label
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (dq, dk, dv)), "a refused call wrote something"
    assert not _abi.short_attention_trainable(inp.q, inp.q, inp.q)  # aliases: the gradients would have to be summed
    assert not _abi.short_attention_trainable(inp.q.float(), inp.k.float(), inp.v.float())


def test_function():
    """grad_fn name, gradient equal to the raw launch bit for bit, retain_graph, double backward raises."""
    _abi, _attn, _, _ = _mods()
    inp = so.make_inputs(6, 3, 8, torch.bfloat16, 21, layout="qkv", device=DEV)
    qkv = inp.qkv.clone().requires_grad_(True)
    out = _attn.short_attention_native(qkv, inp.scale)
    assert type(out.grad_fn).__name__ == "_ShortAttentionFunctionBackward"
    assert torch.equal(out, _abi.short_attention(inp.q, inp.k, inp.v, inp.scale))
    out.backward(inp.dout, retain_graph=True)
    raw = _launch(_abi, inp, "one")
    for i, n in enumerate(("dq", "dk", "dv")):
        assert torch.equal(qkv.grad[:, :, i].permute(0, 2, 1, 3), raw[n]), n
    first = qkv.grad.clone()
    qkv.grad = None
    out.backward(inp.dout)
    assert torch.equal(qkv.grad, first)
    out2 = _attn.short_attention_native(qkv, inp.scale)
    (g,) = torch.autograd.grad(out2.float().sum(), qkv, create_graph=True)
    with pytest.raises(RuntimeError):
        g.float().sum().backward()


def test_routing_in_the_host_attention(monkeypatch):
    _abi, _attn, _, M = _mods()
    from hosts import timesformer
    calls = []
    orig = _abi.short_attention_backward
    monkeypatch.setattr(_abi, "short_attention_backward", lambda *a, **kw: calls.append(1) or orig(*a, **kw))
    torch.manual_seed(0)
    att = timesformer.Attention(192, num_heads=3, qkv_bias=True).to(DEV).to(torch.bfloat16).train()
    x = torch.randn(10, 8, 192, device=DEV, dtype=torch.bfloat16)

    def name_of(mod, inp):
        """The grad_fn that produced the input of proj (or of the result when there is no proj)."""
        seen = []
        if mod.with_qkv:
            h = mod.proj.register_forward_hook(lambda m, a, o: seen.append(a[0]))
            out = mod(inp)
            h.remove()
            return out, type(seen[0].grad_fn).__name__
        out = mod(inp)
        return out, type(out.grad_fn).__name__

    out, name = name_of(att, x)                                                     # under grad
    assert name == "_ShortAttentionFunctionBackward"
    out.float().sum().backward()
    assert len(calls) == 1 and torch.isfinite(att.qkv.weight.grad).all()
    with torch.no_grad():                                                           # no_grad: the inference launch
        o2 = att(x)
    assert o2.grad_fn is None and torch.equal(o2, out)
    for mod, attr in ((_attn, "NATIVE_SHORT_ATTN_BACKWARD"), (_attn, "NATIVE_ATTN_BACKWARD"), (M, "NATIVE_BACKWARD")):
        monkeypatch.setattr(mod, attr, False)                                       # each switch off
        assert "ShortAttention" not in name_of(att, x)[1], attr
        monkeypatch.setattr(mod, attr, True)
    plain = timesformer.Attention(192, num_heads=3, with_qkv=False).to(DEV).train()  # with_qkv=False: q = k = v
    assert "ShortAttention" not in name_of(plain, x.clone().requires_grad_(True))[1]
    att32 = copy.deepcopy(att).float()                                              # fp32
    assert "ShortAttention" not in name_of(att32, x.float())[1]
    x9 = torch.randn(10, 9, 192, device=DEV, dtype=torch.bfloat16)                  # N = 9
    assert "ShortAttention" not in name_of(att, x9)[1]
    wet = copy.deepcopy(att)
    wet.attn_drop.p = 0.1                                                           # live dropout
    assert "ShortAttention" not in name_of(wet, x)[1]
    name_of(att, x)[0].float().sum().backward()
    assert len(calls) == 2, "only the routed cases launch the backward kernel"


def test_patched_timesformer_trains_through_both_new_entries(monkeypatch):
    """The reduced TimeSformer (frames 4, image 64, patch 8, width 64, depth 3, one head, bf16, .train(), r = 6): exactly
    3 tome_short_attention_backward and 3 tome_layernorm_backward_regrouped launches, none with the new switches off;
    every block parameter has a finite gradient; and per parameter, scaled by its largest fp32 gradient, the native
    run's error against an fp32 run is at most 2 x that of the run with the new switches off -- both make the same kind
    and number of 16-bit roundings (a parameter whose exact gradient is zero is treated as
    test_attention_backward_gpu.py treats it).  Measured pair: DESIGN.md section 2."""
    import tome
    from hosts import timesformer
    _abi, _attn, _ln, M = _mods()
    make = lambda: timesformer.TimeSformer(num_frames=4, img_size=64, patch_size=8, embed_dim=64, depth=3,  # noqa: E731
                                           num_heads=1, num_classes=9)
    torch.manual_seed(0)
    model32 = make().to(DEV).train()
    with torch.no_grad():
        for prm in model32.parameters():
            if float(prm.abs().max()) == 0.0:
                prm.normal_(0.0, 0.02)
    model16 = copy.deepcopy(model32).to(torch.bfloat16)
    with torch.no_grad():
        for p32, p16 in zip(model32.parameters(), model16.parameters()):
            p32.copy_(p16.float())
    tome.patch.timesformer(model16, prop_attn=True)
    tome.patch.timesformer(model32, prop_attn=True)
    clip = torch.rand(2, 3, 4, 64, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
    short, regrouped = [], []
    o1, o2 = _abi.short_attention_backward, _abi.layernorm_backward_regrouped
    monkeypatch.setattr(_abi, "short_attention_backward", lambda *a, **kw: short.append(1) or o1(*a, **kw))
    monkeypatch.setattr(_abi, "layernorm_backward_regrouped", lambda *a, **kw: regrouped.append(1) or o2(*a, **kw))

    def run(model, x):
        model.zero_grad(set_to_none=True)
        model.r = 6
        model([x]).float().square().sum().backward()
        return {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}

    ga = run(model16, clip.to(torch.bfloat16))
    assert (len(short), len(regrouped)) == (3, 3), (len(short), len(regrouped))
    missing = [k for k, p in model16.named_parameters() if "blocks" in k and p.grad is None]
    assert not missing, missing
    assert not [k for k, g in ga.items() if not torch.isfinite(g).all()]
    monkeypatch.setattr(_attn, "NATIVE_SHORT_ATTN_BACKWARD", False)
    monkeypatch.setattr(_ln, "NATIVE_LN_REGROUPED_BACKWARD", False)
    gb = run(model16, clip.to(torch.bfloat16))
    assert (len(short), len(regrouped)) == (3, 3), "the framework path must not launch the new kernels"
    gc = run(model32, clip)
    assert ga.keys() == gb.keys() == gc.keys()
    worst_a = worst_b = 0.0
    top = max(g.abs().max().item() for g in gc.values())
    for k in gc:
        scale = gc[k].abs().max().item()
        if scale < 1e-6 * top:
            assert ga[k].abs().max().item() <= 2.0 ** -6 * top and gb[k].abs().max().item() <= 2.0 ** -6 * top, k
            continue
        worst_a = max(worst_a, (ga[k] - gc[k]).abs().max().item() / scale)
        worst_b = max(worst_b, (gb[k] - gc[k]).abs().max().item() / scale)
    print(f"timesformer: worst scaled gradient error native vs fp32 {worst_a:.3e}, new switches off vs fp32 {worst_b:.3e}")
    assert worst_a <= 2 * worst_b, (worst_a, worst_b)
