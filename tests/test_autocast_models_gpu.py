"""Patched models under torch.autocast with fp32 master weights -- how the reference trains (tools/train_net.py:123, with
a GradScaler at :680) and benchmarks (tome/utils.py:54): the LayerNorms of the patched blocks run on
tome_add_layernorm_amp / tome_layernorm_backward_amp, in no_grad and in .train(), for all four families; logits and
gradients against the same weights run in fp32 without autocast."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCK_TAGS = ("ToMeBlock", "ToMeVivitLayer")


def _hosts():
    import tome
    from hosts import motionformer, timesformer, videomae, vivit
    return dict(
        videomae=(lambda: videomae.VideoMAE(num_frames=8, img_size=64, patch_size=16, embed_dim=64, depth=3, num_heads=1,
                                            num_classes=9), (2, 3, 8, 64, 64), tome.patch.videomae),
        timesformer=(lambda: timesformer.TimeSformer(num_frames=4, img_size=64, patch_size=8, embed_dim=64, depth=3,
                                                     num_heads=1, num_classes=9), (2, 3, 4, 64, 64),
                     tome.patch.timesformer),
        motionformer=(lambda: motionformer.Motionformer(img_size=64, patch_size=16, temporal_resolution=4, embed_dim=64,
                                                        depth=3, num_heads=1, num_classes=9), (2, 3, 8, 64, 64),
                      tome.patch.motionformer),
        vivit=(lambda: vivit.ViViT(num_classes=9, image_size=64, num_frames=8, hidden_size=64, num_hidden_layers=3,
                                   num_attention_heads=1, intermediate_size=256), (2, 3, 8, 64, 64), tome.patch.vivit))


FAMILIES = ["videomae", "timesformer", "motionformer", "vivit"]


def _model(name):
    """A reduced-width fp32 host on the device, every parameter with a value, patched; and its clip."""
    make, clip_shape, patch = _hosts()[name]
    torch.manual_seed(0)
    model = make().to(DEV)
    with torch.no_grad():  # (the hosts initialise some parameters with zeros: every parameter gets a value)
        for prm in model.parameters():
            if float(prm.abs().max()) == 0.0:
                prm.normal_(0.0, 0.02)
    patch(model, prop_attn=True)
    clip = torch.rand(*clip_shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    return model, clip


class _Watch:
    """Counts the launches of the two mixed entries and the calls of F.layer_norm made while a patched block's forward
    is on the stack (forward hooks on the tagged blocks keep the depth)."""

    def __init__(self, monkeypatch, model):
        from tome import _abi
        self.forward, self.backward, self.layer_norms, self.depth = 0, 0, [], 0
        fwd, bwd, ln = _abi.add_layernorm_amp, _abi.layernorm_backward_amp, torch.nn.functional.layer_norm

        def fwd_w(*a, **kw):
            self.forward += 1
            return fwd(*a, **kw)

        def bwd_w(*a, **kw):
            self.backward += 1
            return bwd(*a, **kw)

        def ln_w(inp, *a, **kw):
            if self.depth > 0:
                self.layer_norms.append(tuple(inp.shape))
            return ln(inp, *a, **kw)

        monkeypatch.setattr(_abi, "add_layernorm_amp", fwd_w)
        monkeypatch.setattr(_abi, "layernorm_backward_amp", bwd_w)
        monkeypatch.setattr(torch.nn.functional, "layer_norm", ln_w)
        self.blocks = [m for m in model.modules() if getattr(type(m), "_tome_tag", None) in BLOCK_TAGS]
        assert len(self.blocks) == 3
        for m in self.blocks:
            m.register_forward_pre_hook(lambda *_: setattr(self, "depth", self.depth + 1))
            m.register_forward_hook(lambda *_: setattr(self, "depth", self.depth - 1))

    def reset(self):
        self.forward, self.backward, self.layer_norms = 0, 0, []


def _only_the_regrouped_norm(name, watch, clip):
    """F.layer_norm inside a patched block: never -- but for TimeSformer's mid-block norm of the regrouped tokens
    [B*T, 1 + P, C], once per block."""
    if name != "timesformer":
        assert not watch.layer_norms, (name, watch.layer_norms)
        return
    B, T = clip.shape[0], clip.shape[2]
    assert len(watch.layer_norms) == 3 and all(s[0] == B * T for s in watch.layer_norms), watch.layer_norms


def _grads(model):
    return {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}


def _step(model, clip, dtype):
    """One forward + backward in .train(): under autocast of `dtype`, or plain fp32 (dtype None)."""
    model.zero_grad(set_to_none=True)
    model.r = 6
    with torch.autocast("cuda", dtype=dtype, enabled=dtype is not None):
        out = model([clip])
    out.float().square().sum().backward()
    return out.detach().double().cpu(), _grads(model)


@pytest.mark.parametrize("name", FAMILIES)
def test_no_grad_forward_runs_the_mixed_entry(name, monkeypatch):
    from tome import _ln
    model, clip = _model(name)
    model.eval()
    watch = _Watch(monkeypatch, model)
    model.r = 6
    with torch.no_grad():
        want = model([clip]).double()
        assert watch.forward == 0 and watch.backward == 0, "an fp32 model without autocast launches neither entry"
        watch.reset()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            model.r = 6
            got = model([clip]).double()
        launched = watch.forward
        assert launched >= 6 and watch.backward == 0, (name, launched)  # two LayerNorms in each of three blocks
        _only_the_regrouped_norm(name, watch, clip)
        watch.reset()
        monkeypatch.setattr(_ln, "NATIVE_LN_AUTOCAST", False)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            model.r = 6
            off = model([clip]).double()
        assert watch.forward == 0 and len(watch.layer_norms) >= 6, "with the switch off the entries are not launched"
    scale = float(want.abs().max())
    err_on, err_off = float((got - want).abs().max()) / scale, float((off - want).abs().max()) / scale
    print(f"{name} no_grad bf16 autocast: logits error vs fp32 native {err_on:.3e}, switch off {err_off:.3e} "
          f"({launched} launches)")
    assert err_on <= 2 * err_off + 2.0 ** -8, (name, err_on, err_off)


@pytest.mark.parametrize("name", FAMILIES)
def test_training_step_under_autocast(name, monkeypatch):
    """.train(), bf16 autocast, fp32 parameters, r = 6 in every block.  Three runs on the same weights: (a) native, (b)
    the switch off (the framework's add, fp32 layer_norm and casts), (c) fp32 without autocast.  Logits, and the worst
    per-parameter gradient error scaled by that parameter's largest gradient in (c): native <= 2 x switch-off + 2^-8.
    Parameters whose largest fp32 gradient is below 1e-6 of the model's largest are zero in exact arithmetic and held to
    the absolute floor of tests/test_attention_backward_gpu.py (2^-6 of the model's largest gradient) in both runs."""
    from tome import _ln
    model, clip = _model(name)
    model.train()
    watch = _Watch(monkeypatch, model)
    out_c, gc = _step(model, clip, None)
    assert watch.forward == 0 and watch.backward == 0, "an fp32 model without autocast launches neither entry"
    watch.reset()
    out_a, ga = _step(model, clip, torch.bfloat16)
    assert watch.forward >= 6 and watch.backward == watch.forward, (name, watch.forward, watch.backward)
    _only_the_regrouped_norm(name, watch, clip)
    launches = watch.forward
    for k, p in model.named_parameters():
        if "blocks" in k or "encoder.layer" in k:
            assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), k
    watch.reset()
    monkeypatch.setattr(_ln, "NATIVE_LN_AUTOCAST", False)
    out_b, gb = _step(model, clip, torch.bfloat16)
    assert watch.forward == 0 and watch.backward == 0, "with the switch off the entries are not launched"
    assert ga.keys() == gb.keys() == gc.keys()
    scale = float(out_c.abs().max())
    log_a, log_b = float((out_a - out_c).abs().max()) / scale, float((out_b - out_c).abs().max()) / scale
    worst_a = worst_b = 0.0
    top = max(g.abs().max().item() for g in gc.values())
    for k in gc:
        s = gc[k].abs().max().item()
        if s < 1e-6 * top:
            assert ga[k].abs().max().item() <= 2.0 ** -6 * top and gb[k].abs().max().item() <= 2.0 ** -6 * top, k
            continue
        worst_a = max(worst_a, (ga[k] - gc[k]).abs().max().item() / s)
        worst_b = max(worst_b, (gb[k] - gc[k]).abs().max().item() / s)
    print(f"{name} train bf16 autocast ({launches} forward and backward launches): logits error vs fp32 native {log_a:.3e}, "
          f"switch off {log_b:.3e}; worst scaled gradient error native {worst_a:.3e}, switch off {worst_b:.3e}")
    assert log_a <= 2 * log_b + 2.0 ** -8, (name, log_a, log_b)
    assert worst_a <= 2 * worst_b + 2.0 ** -8, (name, worst_a, worst_b)


def test_fp16_autocast_with_a_grad_scaler_step(monkeypatch):
    """VideoMAE (the 16-bit stream) under fp16 autocast: scaled loss, unscale, optimizer step -- finite gradients, the
    step is taken, the parameters of the blocks change."""
    model, clip = _model("videomae")
    model.train()
    watch = _Watch(monkeypatch, model)
    opt = torch.optim.SGD(model.parameters(), lr=1.0)  # (one step: large enough to move fp32 weights near 1)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    model.r = 6
    with torch.autocast("cuda", dtype=torch.float16):
        loss = model([clip]).float().square().sum()
    scaler.scale(loss).backward()
    assert watch.forward >= 6 and watch.backward == watch.forward
    scaler.unscale_(opt)
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == 2.0 ** 10, "the step was skipped: a non-finite gradient"
    changed = [k for k, p in model.named_parameters() if not torch.equal(p.detach(), before[k])]
    for kind in ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "qkv"):
        grads = [float(p.grad.abs().max()) for k, p in model.named_parameters() if kind in k]
        print(f"fp16 GradScaler step: {kind} largest gradients {grads}")
        assert any(kind in k for k in changed), kind
    assert bool(torch.isfinite(loss))


def test_benchmark_with_use_fp16_launches_the_forward_entry(monkeypatch):
    """tome.utils.benchmark(model, use_fp16=True) -- the reference's public throughput function, tome/utils.py:54 -- on
    a reduced host: its forward under autocast runs the LayerNorms on the mixed entry."""
    import tome
    from hosts import videomae

    class Clips(torch.nn.Module):  # benchmark hands the model a tensor; the hosts take the list of pathways
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x):
            return self.inner([x])

    torch.manual_seed(0)
    inner = videomae.VideoMAE(num_frames=8, img_size=64, patch_size=16, embed_dim=64, depth=3, num_heads=1, num_classes=9)
    tome.patch.videomae(inner, prop_attn=True)
    inner.r = 6
    watch = _Watch(monkeypatch, inner)
    rate = tome.utils.benchmark(Clips(inner), device=torch.device(DEV), input_size=(3, 8, 64, 64), batch_size=2, runs=4,
                                use_fp16=True)
    assert rate > 0 and watch.forward >= 4 * 6 and watch.backward == 0
    assert not watch.layer_norms
