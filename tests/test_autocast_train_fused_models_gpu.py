"""Patched models that TRAIN under torch.autocast with tome._ln.NATIVE_MERGE_LN_AUTOCAST_BACKWARD on: the flat-layout
blocks (VideoMAE, ViViT) take the residual add, the reduction and the second LayerNorm as one launch forward
(tome_merge_wavg_ln_amp / tome_drop_ln_amp) and one launch backward (tome_merge_ln_backward_amp) in the modes merge and
drop; mode hybrid and the interleaved layouts (TimeSformer, Motionformer) are out of its reach.  Reduced-width fp32 hosts
as in tests/test_autocast_fused_models_gpu.py, .train(), bf16 autocast, r = 6, gradients on; the loss and every
parameter's gradient against the same weights in fp32 without autocast."""
import pytest
import torch

import test_autocast_fused_models_gpu as fused

pytestmark = pytest.mark.gpu
COUNTED = ("merge_wavg_ln_amp", "drop_ln_amp", "merge_ln_backward_amp", "add_layernorm_amp", "layernorm_backward_amp")


class _Watch(fused._Watch):
    """Counts the launches of the forward and backward entries, and keeps every block's token count."""

    def __init__(self, monkeypatch, model):
        from tome import _abi
        self.counts = {name: 0 for name in COUNTED}
        self.tokens = []
        for name in self.counts:
            monkeypatch.setattr(_abi, name, self._counted(name, getattr(_abi, name)))
        blocks = [m for m in model.modules() if getattr(type(m), "_tome_tag", None) in fused.BLOCK_TAGS]
        assert len(blocks) == 3
        for m in blocks:
            m.register_forward_hook(lambda mod, args, out: self.tokens.append(
                tuple((out[0] if isinstance(out, (tuple, list)) else out).shape)))


def _step(model, clip, autocast=True):
    """One training step's loss and gradients (float64 on the CPU) on the same weights."""
    model.zero_grad(set_to_none=True)
    model.r = 6
    torch.manual_seed(1)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = model([clip])
    loss = out.float().square().mean()
    loss.backward()
    grads = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}
    return loss.detach().double().cpu(), grads


def _train_model(name, mode):
    model, clip = fused._model(name, mode)
    return model.train(), clip


@pytest.mark.parametrize("mode", ["merge", "drop"])
@pytest.mark.parametrize("name", ["videomae", "vivit"])
def test_flat_blocks_train_through_the_fused_launches(name, mode, monkeypatch):
    from tome import _ln
    model, clip = _train_model(name, mode)
    watch = _Watch(monkeypatch, model)
    loss_ref, g_ref = _step(model, clip, autocast=False)
    assert not any(watch.take()[0].values()), "an fp32 model without autocast launches none of the entries"
    assert _ln.NATIVE_MERGE_LN_AUTOCAST_BACKWARD is False
    loss_off, g_off = _step(model, clip)
    counts_off, tokens_off = watch.take()
    assert counts_off["merge_wavg_ln_amp"] == 0 and counts_off["drop_ln_amp"] == 0
    assert counts_off["merge_ln_backward_amp"] == 0
    assert counts_off["add_layernorm_amp"] >= 6 and counts_off["layernorm_backward_amp"] >= 6
    monkeypatch.setattr(_ln, "NATIVE_MERGE_LN_AUTOCAST_BACKWARD", True)
    loss_on, g_on = _step(model, clip)
    counts_on, tokens_on = watch.take()
    entry, other = ("drop_ln_amp", "merge_wavg_ln_amp") if mode == "drop" else ("merge_wavg_ln_amp", "drop_ln_amp")
    assert counts_on[entry] == 3 and counts_on[other] == 0, counts_on               # once per reducing block
    assert counts_on["merge_ln_backward_amp"] == 3, counts_on
    assert counts_on["add_layernorm_amp"] == counts_off["add_layernorm_amp"] - 3, (counts_on, counts_off)
    assert counts_on["layernorm_backward_amp"] == counts_off["layernorm_backward_amp"] - 3, (counts_on, counts_off)
    assert tokens_on == tokens_off and len(tokens_on) == 3, (tokens_on, tokens_off)
    assert g_on.keys() == g_off.keys() == g_ref.keys() and len(g_ref) > 0
    named = dict(g_ref, loss=loss_ref)
    on, off = dict(g_on, loss=loss_on), dict(g_off, loss=loss_off)
    worst_on = worst_off = 0.0
    bad = []
    for k, want in named.items():
        scale = float(want.abs().max())
        if scale == 0.0:
            assert float(on[k].abs().max()) == 0.0, k
            continue
        e_on, e_off = float((on[k] - want).abs().max()) / scale, float((off[k] - want).abs().max()) / scale
        worst_on, worst_off = max(worst_on, e_on), max(worst_off, e_off)
        if not (torch.isfinite(on[k]).all() and e_on <= 2 * e_off + 2.0 ** -8):
            bad.append((k, e_on, e_off))
    print(f"{name} {mode} train bf16 autocast: worst scaled error vs fp32 (loss and {len(g_ref)} gradients) with the switch "
          f"on {worst_on:.3e}, off {worst_off:.3e}; tokens per block {[t[1] for t in tokens_on]}")
    assert not bad, bad


@pytest.mark.parametrize("name,mode", [("videomae", "hybrid"), ("vivit", "hybrid"), ("timesformer", "merge"),
                                       ("motionformer", "merge")])
def test_what_the_switch_does_not_cover_keeps_its_launches(name, mode, monkeypatch):
    from tome import _ln
    model, clip = _train_model(name, mode)
    watch = _Watch(monkeypatch, model)
    loss_off, g_off = _step(model, clip)
    counts_off, tokens_off = watch.take()
    monkeypatch.setattr(_ln, "NATIVE_MERGE_LN_AUTOCAST_BACKWARD", True)
    loss_on, g_on = _step(model, clip)
    counts_on, tokens_on = watch.take()
    assert counts_on["merge_wavg_ln_amp"] == 0 and counts_on["drop_ln_amp"] == 0 and counts_on["merge_ln_backward_amp"] == 0
    assert counts_on == counts_off and tokens_on == tokens_off
    assert g_on.keys() == g_off.keys() and bool(torch.isfinite(loss_on)) and bool(torch.isfinite(loss_off))
