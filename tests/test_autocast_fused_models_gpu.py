"""Patched models under torch.autocast with tome.patch._common.AUTOCAST_FUSED_LN on: the flat-layout blocks (VideoMAE,
ViViT) take the residual add, the reduction and the second LayerNorm as one launch (tome_merge_wavg_ln_amp /
tome_drop_ln_amp) in the modes merge, drop and hybrid; the interleaved layouts (TimeSformer, Motionformer) are out of its
reach and keep their bits.  Reduced-width fp32 hosts as in tests/test_autocast_models_gpu.py, .eval(), bf16 autocast,
r = 6; logits against the same weights in fp32 without autocast."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCK_TAGS = ("ToMeBlock", "ToMeVivitLayer")
MODES = ["merge", "drop", "hybrid"]


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


def _model(name, mode):
    """A reduced-width fp32 host on the device, every parameter with a value, patched in `mode`; and its clip."""
    make, clip_shape, patch = _hosts()[name]
    torch.manual_seed(0)
    model = make().to(DEV)
    with torch.no_grad():  # (the hosts initialise some parameters with zeros: every parameter gets a value)
        for prm in model.parameters():
            if float(prm.abs().max()) == 0.0:
                prm.normal_(0.0, 0.02)
    patch(model, prop_attn=True, mode=mode, threshold=0.5 if mode == "hybrid" else 0.0)
    clip = torch.rand(*clip_shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    return model.eval(), clip


class _Watch:
    """Counts the launches of the two new entries and of tome_add_layernorm_amp, and keeps every block's token count."""

    def __init__(self, monkeypatch, model):
        from tome import _abi
        self.counts = {"merge_wavg_ln_amp": 0, "drop_ln_amp": 0, "add_layernorm_amp": 0}
        self.tokens = []
        for name in self.counts:
            monkeypatch.setattr(_abi, name, self._counted(name, getattr(_abi, name)))
        blocks = [m for m in model.modules() if getattr(type(m), "_tome_tag", None) in BLOCK_TAGS]
        assert len(blocks) == 3
        for m in blocks:
            m.register_forward_hook(lambda mod, args, out: self.tokens.append(
                tuple((out[0] if isinstance(out, (tuple, list)) else out).shape)))

    def _counted(self, name, real):
        def call(*a, **kw):
            self.counts[name] += 1
            return real(*a, **kw)
        return call

    def take(self):
        got = dict(self.counts), list(self.tokens)
        self.counts = {k: 0 for k in self.counts}
        self.tokens = []
        return got


def _forward(model, clip, autocast=True):
    model.r = 6
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        return model([clip]).double()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["videomae", "vivit"])
def test_flat_blocks_take_the_fused_launch(name, mode, monkeypatch):
    from tome.patch import _common as C
    model, clip = _model(name, mode)
    watch = _Watch(monkeypatch, model)
    want = _forward(model, clip, autocast=False)
    assert not any(watch.take()[0].values()), "an fp32 model without autocast launches none of the entries"
    assert C.AUTOCAST_FUSED_LN is False
    off = _forward(model, clip)
    counts_off, tokens_off = watch.take()
    assert counts_off["merge_wavg_ln_amp"] == 0 and counts_off["drop_ln_amp"] == 0 and counts_off["add_layernorm_amp"] >= 6
    monkeypatch.setattr(C, "AUTOCAST_FUSED_LN", True)
    on = _forward(model, clip)
    counts_on, tokens_on = watch.take()
    entry, other = ("drop_ln_amp", "merge_wavg_ln_amp") if mode == "drop" else ("merge_wavg_ln_amp", "drop_ln_amp")
    assert counts_on[entry] == 3 and counts_on[other] == 0, counts_on           # once per reducing block
    assert counts_on["add_layernorm_amp"] == counts_off["add_layernorm_amp"] - 3, (counts_on, counts_off)
    assert tokens_on == tokens_off and len(tokens_on) == 3, (tokens_on, tokens_off)
    scale = float(want.abs().max())
    err_on, err_off = float((on - want).abs().max()) / scale, float((off - want).abs().max()) / scale
    print(f"{name} {mode} no_grad bf16 autocast: logits error vs fp32 with AUTOCAST_FUSED_LN on {err_on:.3e}, off "
          f"{err_off:.3e}; tokens per block {[t[1] for t in tokens_on]}")
    assert err_on <= 2 * err_off + 2.0 ** -8, (name, mode, err_on, err_off)


@pytest.mark.parametrize("name", ["timesformer", "motionformer"])
def test_interleaved_layouts_are_out_of_reach(name, monkeypatch):
    from tome.patch import _common as C
    model, clip = _model(name, "merge")
    watch = _Watch(monkeypatch, model)
    off = _forward(model, clip)
    counts_off, tokens_off = watch.take()
    monkeypatch.setattr(C, "AUTOCAST_FUSED_LN", True)
    on = _forward(model, clip)
    counts_on, tokens_on = watch.take()
    assert counts_on["merge_wavg_ln_amp"] == 0 and counts_on["drop_ln_amp"] == 0
    assert counts_on == counts_off and tokens_on == tokens_off
    assert torch.equal(on, off), "the attribute changed a model it does not cover"
