"""The pooled tail of a mean-pooling ViT's last block (tome/patch/_common.py::pooled_tail, armed by the wrapped model
forward through tome/patch/videomae.py::pooled_tail_block): `mean_t(x' + b2 + W2 a_t) = mean_t(x') + b2 + W2 mean_t(a_t)`.

Tail alone: against the float64 value of the right-hand side computed from the SAME fc1 output bits, within half a 16-bit
ulp of the result (the one rounding at the end: 2^-8 relative for bf16, 2^-11 for fp16) plus the fp32 summation bound of
the two means, T 2^-24 (mean|x'| + |W2| mean|a|); and no farther from that reference than the parent path (fc2 as a 16-bit
GEMM accumulating onto the stream, then the 16-bit `mean`) by more than that half ulp.
Small model: every block but the last is bit-equal with the tail on and off, the row fed to fc_norm obeys the bound,
logits repeat bit for bit, a captured HIP graph replays to the eager bits.
Fallbacks: whatever fails the predicate takes the parent path bit for bit (and never calls the tail)."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
U = 2.0 ** -24


def _mods():
    import tome
    from hosts import videomae
    from tome import _abi
    from tome.patch import _common as C
    return tome, videomae, _abi, C


def _tail_reference(abi, mlp, x, y):
    """(ref, allowance without the half ulp) in float64 from the bits of fc1(y) and of tome_gelu_erf of them."""
    T = x.shape[1]
    a = abi.gelu_erf(mlp.fc1(y), inplace=False).double()
    W2, b2 = mlp.fc2.weight.double(), mlp.fc2.bias.double()
    ref = x.double().mean(1) + b2 + a.mean(1) @ W2.t()
    summation = T * U * (x.double().abs().mean(1) + a.abs().mean(1) @ W2.abs().t())
    return ref, summation


def _random_biases(module, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_tail_alone_against_float64_and_the_parent_path(dtype):
    _, videomae, abi, C = _mods()
    B, T, Cw, Hd = 2, 33, 64, 256
    torch.manual_seed(3)
    mlp = videomae.Mlp(Cw, Hd)
    torch.nn.init.normal_(mlp.fc1.weight, std=0.2)
    torch.nn.init.normal_(mlp.fc2.weight, std=0.2)
    _random_biases(mlp, 4)
    mlp = mlp.to(DEV).to(dtype).eval()
    x = torch.randn(B, T, Cw).to(dtype).to(DEV)
    y = torch.randn(B, T, Cw).to(dtype).to(DEV)
    with torch.no_grad():
        ref, summation = _tail_reference(abi, mlp, x, y)
        out = C.pooled_tail(mlp, x, y)
        assert tuple(out.shape) == (B, 1, Cw) and out.dtype == dtype
        # the parent path, by the project's own code: fc2's bias folded into the stream, the GEMM accumulating onto it
        # (finish_linear), then the host's 16-bit mean
        stream = x + mlp.fc2.bias
        block = types.SimpleNamespace(training=False, _tome_next_norm=None)
        full = C.mlp_residual(block, mlp, stream, y, {"_folded": (stream, mlp.fc2)})
        assert tuple(full.shape) == (B, T, Cw)
        parent = full.mean(1)
    half = HALF_ULP[dtype] * ref.abs()
    err = (out[:, 0].double() - ref).abs()
    err_parent = (parent.double() - ref).abs()
    print(f"tail alone {dtype}: max err {float(err.max()):.3e} (allowed at that place "
          f"{float((half + summation).flatten()[err.argmax()]):.3e}), parent max err {float(err_parent.max()):.3e}")
    assert bool((err <= half + summation).all())
    assert bool((err <= err_parent + half).all())


def _model(dtype=torch.bfloat16, **kw):
    tome, videomae, _, _ = _mods()
    torch.manual_seed(0)
    m = videomae.VideoMAE(num_frames=8, img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=9,
                          **kw)
    _random_biases(m, 1)
    torch.nn.init.normal_(m.model.head.weight, std=0.2)  # (the host's 0.001 scale would hide the tokens behind the bias)
    m = m.to(DEV).to(dtype).eval()
    tome.patch.videomae(m, prop_attn=True)
    m.r = 2
    return m


def _clips(dtype=torch.bfloat16, B=3):
    gen = torch.Generator().manual_seed(2)
    return [torch.rand(B, 3, 8, 64, 64, generator=gen).to(dtype).to(DEV)]


class _Spy:
    """Counts the calls of C.pooled_tail and keeps the arguments of the last one."""

    def __init__(self, monkeypatch, C):
        self.calls, self.args, real = 0, None, C.pooled_tail

        def spy(mlp, x, y):
            self.calls += 1
            self.args = (mlp, x, y)
            return real(mlp, x, y)

        monkeypatch.setattr(C, "pooled_tail", spy)


def _run(model, clips, C, switch, grad=False):
    """(logits, first block's output, the row fed to fc_norm or None) of one forward with the switch set."""
    seen = {}
    hooks = [model.model.blocks[0].register_forward_hook(lambda m, i, o: seen.__setitem__("first", o.clone()))]
    if model.model.fc_norm is not None:
        hooks.append(model.model.fc_norm.register_forward_pre_hook(lambda m, i: seen.__setitem__("row", i[0].clone())))
    was = C._POOL_TAIL
    C._POOL_TAIL = switch
    try:
        with torch.set_grad_enabled(grad):
            logits = model(clips)
    finally:
        C._POOL_TAIL = was
        for h in hooks:
            h.remove()
    torch.cuda.synchronize()
    return logits.detach(), seen["first"].detach(), seen.get("row")


def test_small_model_armed(monkeypatch):
    _, _, abi, C = _mods()
    model, clips = _model(), _clips()
    spy = _Spy(monkeypatch, C)
    off = _run(model, clips, C, False)
    assert spy.calls == 0
    on = _run(model, clips, C, True)
    assert spy.calls == 1 and "_pool_tail" not in model._tome_info
    assert torch.equal(on[1], off[1])  # every block but the last: the same bits
    mlp, x, y = spy.args
    assert tuple(x.shape) == (3, 64 - 2 * 2, 128)
    with torch.no_grad():
        ref, summation = _tail_reference(abi, mlp, x, y)
    allowed = HALF_ULP[torch.bfloat16] * ref.abs() + summation
    err = (on[2].double() - ref).abs()
    print(f"small model: max err of the pooled row {float(err.max()):.3e}, allowed there "
          f"{float(allowed.flatten()[err.argmax()]):.3e}; max |logit on - off| {float((on[0] - off[0]).abs().max()):.3e}")
    assert bool((err <= allowed).all())
    again = _run(model, clips, C, True)
    assert spy.calls == 2 and torch.equal(again[0], on[0])  # run to run: the same bits


def test_captured_graph_of_the_armed_forward_replays_to_the_eager_bits(monkeypatch):
    _, _, _, C = _mods()
    from hosts.graphed import GraphedForward
    model, clips = _model(), _clips()
    spy = _Spy(monkeypatch, C)
    with torch.no_grad():
        eager = model(clips).clone()
    assert spy.calls == 1
    fwd = GraphedForward(model, clips, warmup=1)
    assert spy.calls == 3  # the warm-up and the captured forward were armed too
    other = [torch.rand_like(clips[0])]
    assert not torch.equal(fwd(other), eager)
    replayed = fwd(clips).clone()
    torch.cuda.synchronize()
    assert torch.equal(replayed, eager)


FALLBACKS = ["hook", "train", "grad", "gamma_2", "no_mean_pooling", "fp32", "mlp_hook", "norm_hook"]


@pytest.mark.parametrize("case", FALLBACKS)
def test_fallbacks_take_the_parent_path_bit_for_bit(case, monkeypatch):
    _, _, _, C = _mods()
    kw, dtype, grad = {}, torch.bfloat16, False
    if case == "gamma_2":
        kw["init_values"] = 0.1
    elif case == "no_mean_pooling":
        kw["use_mean_pooling"] = False
    elif case == "fp32":
        dtype = torch.float32
    model, clips = _model(dtype, **kw), _clips(dtype)
    last, full = model.model.blocks[-1], {}
    if case == "hook":
        last.register_forward_hook(lambda m, i, o: full.__setitem__("out", o.clone()))
    elif case == "mlp_hook":
        last.mlp.fc2.register_forward_hook(lambda m, i, o: None)
    elif case == "norm_hook":
        model.model.norm.register_forward_hook(lambda m, i, o: full.__setitem__("out", o.clone()))
    elif case == "train":
        model.train()
    elif case == "grad":
        grad = True
    spy = _Spy(monkeypatch, C)
    on = _run(model, clips, C, True, grad)
    seen = full.get("out")
    off = _run(model, clips, C, False, grad)
    assert spy.calls == 0
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    if seen is not None:  # whoever observes the block's output gets the full tensor, with the parent's bits
        assert tuple(seen.shape) == (3, 64 - 2 * 2, 128) and torch.equal(seen, full["out"])


def test_the_last_block_called_directly_returns_every_token(monkeypatch):
    _, _, _, C = _mods()
    model = _model()
    spy = _Spy(monkeypatch, C)
    last = model.model.blocks[-1]
    tokens = torch.randn(3, 40, 128).to(torch.bfloat16).to(DEV)
    outs = []
    for switch in (True, False):
        monkeypatch.setattr(C, "_POOL_TAIL", switch)
        model._tome_info.update(r=[2], size=None, source=None)
        with torch.no_grad():
            outs.append(last(tokens))
    assert spy.calls == 0 and tuple(outs[0].shape) == (3, 38, 128) and torch.equal(outs[0], outs[1])
    # ... and the armed model forward is not vacuous here: the same model pools when called as a model
    monkeypatch.setattr(C, "_POOL_TAIL", True)
    with torch.no_grad():
        model(_clips())
    assert spy.calls == 1
