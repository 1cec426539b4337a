"""The four reduced hosts of test_models_gpu.test_fused_block_equals_unfused_block_bf16 in the modes beside plain merge
(drop, hybrid, random_merge, random_drop), bf16, `.eval()`, no grad: with `_FUSE_MODES` on every merging block takes ONE
reduction + LayerNorm launch (no framework LayerNorm on norm2's input, no reduction on its own); with the switch off the
launch sequence is the three steps it was before.  Between the two arms: the same token schedule, the same index tensors in
every layer, the same final sizes, logits within that test's bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HOSTS = ["videomae", "vivit", "timesformer", "motionformer"]
MODES = ["drop", "hybrid", "random_merge", "random_drop"]
R = 5
FLAT = ("videomae", "vivit")


def _model(host_name, **patch_kw):
    import tome
    from hosts import motionformer, timesformer, videomae, vivit
    torch.manual_seed(0)
    if host_name == "videomae":
        model = videomae.VideoMAE(num_frames=8, img_size=64, patch_size=16, embed_dim=64, depth=4, num_heads=1,
                                  num_classes=9)
        patch, frames, blocks, norm2 = tome.patch.videomae, 8, lambda m: m.model.blocks, "norm2"
    elif host_name == "vivit":
        model = vivit.ViViT(num_classes=9, image_size=64, num_frames=8, hidden_size=64, num_hidden_layers=4,
                            num_attention_heads=1, intermediate_size=128)
        patch, frames, blocks, norm2 = tome.patch.vivit, 8, lambda m: m.vivit.encoder.layer, "layernorm_after"
    elif host_name == "timesformer":
        model = timesformer.TimeSformer(num_frames=4, img_size=64, patch_size=8, embed_dim=64, depth=4, num_heads=1,
                                        num_classes=9)
        patch, frames, blocks, norm2 = tome.patch.timesformer, 4, lambda m: m.model.blocks, "norm2"
    else:
        model = motionformer.Motionformer(img_size=64, patch_size=8, patch_size_temp=2, temporal_resolution=4,
                                          embed_dim=64, depth=3, num_heads=1, num_classes=9)
        patch, frames, blocks, norm2 = tome.patch.motionformer, 8, lambda m: m.blocks, "norm2"
    model = model.to(DEV).to(torch.bfloat16).eval()
    patch(model, **patch_kw)
    torch.manual_seed(1)
    clip = torch.rand(3, 3, frames, 64, 64, device=DEV).to(torch.bfloat16)
    return model, clip, [getattr(b, norm2) for b in blocks(model)]


class Counters:
    """Wrappers around the reduction entries of tome._abi and around F.layer_norm, for one forward."""
    ABI = ("drop_ln", "drop_regrouped", "merge_wavg_ln", "merge_wavg_regrouped", "drop", "merge_wavg")
    MATCH = ("bipartite_soft_matching", "bipartite_soft_matching_drop", "bipartite_soft_matching_hybrid")

    def __init__(self, monkeypatch, norm2s):
        from tome import _abi
        from tome.patch import _common
        self.n = {"fused": 0, "fused_with_addend": 0, "alone": 0, "drop": 0, "norm2_layer_norm": 0}
        self.plans = []
        weights = {id(n.weight) for n in norm2s}

        def wrap(name, orig):
            def call(*a, **kw):
                if name in ("drop_ln", "merge_wavg_ln") or kw.get("ln") is not None:
                    self.n["fused"] += 1
                    self.n["fused_with_addend"] += int(kw.get("addend") is not None or kw.get("addend_grouped") is not None)
                else:
                    self.n["alone"] += 1
                    self.n["drop"] += int(name == "drop")
                return orig(*a, **kw)
            return call

        for name in self.ABI:
            monkeypatch.setattr(_abi, name, wrap(name, getattr(_abi, name)))

        def spy_of(orig):
            def spy(metric, *a, **kw):
                got = orig(metric, *a, **kw)
                fn = got[0] if isinstance(got, tuple) else got
                if hasattr(fn, "plan"):
                    self.plans.append(fn.plan)
                return got
            return spy

        for name in self.MATCH:
            monkeypatch.setattr(_common, name, spy_of(getattr(_common, name)))
        layer_norm = torch.nn.functional.layer_norm

        def counted(x, shape, weight=None, bias=None, eps=1e-5):
            self.n["norm2_layer_norm"] += int(id(weight) in weights)
            return layer_norm(x, shape, weight, bias, eps)

        monkeypatch.setattr(torch.nn.functional, "layer_norm", counted)


def _forward(model, clip, norm2s, fuse_modes, r=R):
    """One forward under fresh counters (its own monkeypatch context: the wrappers do not stack)."""
    from tome.patch import _common
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_common, "_FUSE_MODES", fuse_modes)
        c = Counters(mp, norm2s)
        model.r = r
        torch.manual_seed(1234)
        with torch.no_grad():
            out = model([clip])
        torch.cuda.synchronize()
    info = model._tome_info
    return dict(out=out.float(), plans=c.plans, n=c.n, size=info["size"].float().clone(),
                source=None if info["source"] is None else info["source"].clone())


def _first_layer_threshold(model, clip, norm2s):
    """A threshold inside the first layer's edge scores: the median score of its selected edges."""
    model._tome_info["threshold"] = 0.0
    plan = _forward(model, clip, norm2s, False)["plans"][0]
    picked = plan.node_max.reshape(plan.n, -1).gather(1, plan.src_idx.reshape(plan.n, -1)).reshape(-1).float().sort().values
    lo_, hi_ = float(picked[0]), float(picked[-1])
    thr = float(picked[picked.numel() // 2])
    assert lo_ < thr <= hi_, (lo_, thr, hi_)
    return thr


def _same_schedule(p1, p0):
    assert [(p.n, p.T, p.r) for p in p1] == [(p.n, p.T, p.r) for p in p0], "token schedule"


def _differing(a, b):
    """Entries of a plan's index tensors (and threshold flags) that differ between the two arms."""
    names = ("src_idx", "dst_idx", "unm_idx") + (("edge_keep",) if a.edge_keep is not None else ())
    return {name: int((getattr(a, name) != getattr(b, name)).sum()) for name in names}


_ARMS = {}


def _arms(host_name, mode, trace=False, r=R):
    """(layers, switch-on forward, switch-off forward) of one host in one mode: computed once, shared by the tests."""
    key = (host_name, mode, trace, str(r))
    if key not in _ARMS:
        model, clip, norm2s = _model(host_name, mode=mode, trace_source=trace)
        if mode == "hybrid":
            model._tome_info["threshold"] = _first_layer_threshold(model, clip, norm2s)
        _ARMS[key] = (len(norm2s), _forward(model, clip, norm2s, True, r), _forward(model, clip, norm2s, False, r))
    return _ARMS[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("host_name", HOSTS)
def test_one_fused_launch_per_merging_block(host_name, mode):
    layers, on, off = _arms(host_name, mode)
    assert len(on["plans"]) == len(off["plans"]) == layers  # every block reduces at r = 5
    if mode == "hybrid":
        keep = on["plans"][0].edge_keep
        assert 0 < int(keep.sum()) < keep.numel()
    # switch on: one launch per merging block carries add + reduction + LayerNorm
    assert on["n"] == dict(fused=layers, fused_with_addend=layers, alone=0, drop=0, norm2_layer_norm=0), on["n"]
    # switch off: the reduction on its own and the framework's LayerNorm behind it, as before
    assert off["n"] == dict(fused=0, fused_with_addend=0, alone=layers, drop=layers if (mode.endswith("drop")
                            and host_name in FLAT) else 0, norm2_layer_norm=layers), off["n"]
    _same_schedule(on["plans"], off["plans"])
    assert not any(_differing(on["plans"][0], off["plans"][0]).values())  # the first layer sees the same bits
    assert on["size"].shape == off["size"].shape and on["size"].dtype == off["size"].dtype
    if mode.endswith("drop"):
        assert on["size"].dtype == torch.float32 and bool((on["size"] == 1).all())
    assert float((on["out"] - off["out"]).abs().max()) <= 0.05 * max(1.0, float(off["out"].abs().max()))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("host_name", HOSTS)
def test_every_layer_selects_the_same_tokens(host_name, mode, capsys):
    """Between the two arms: every layer's index tensors (and threshold flags) and the final sizes are equal.

    This holds because the fused launch of these modes stores the stream of the three steps bit for bit
    (tests/test_modes_ln_gpu.py) and does NOT fold fc2's bias into it (tome/patch/_common.py::_fold_for: plain 'merge'
    alone).  With the fold, round(round(x' + b) + h W) stands for round(x' + round(h W + b)): measured on these hosts, 7 of
    the 16 cases then part from the second layer on (timesformer-drop: 2 / 3 / 24 entries of src / dst / unm_idx at layer
    1, 36 / 33 / 165 at layer 3), as plain 'merge' does between _FUSE_LN on and off -- which is why test_models_gpu.py
    compares first-layer indices only for it."""
    layers, on, off = _arms(host_name, mode)
    _same_schedule(on["plans"], off["plans"])
    diffs = [_differing(a, b) for a, b in zip(on["plans"], off["plans"])]
    capsys.readouterr()
    print(f"{host_name} {mode}: differing index entries per layer {diffs}; sizes equal "
          f"{on['size'].shape == off['size'].shape and bool(torch.equal(on['size'], off['size']))}")
    assert not any(v for d in diffs for v in d.values()), diffs
    assert torch.equal(on["size"], off["size"])


@pytest.mark.parametrize("mode", ["drop", "hybrid"])
@pytest.mark.parametrize("host_name", HOSTS)
def test_trace_source_keeps_the_add_unfused(host_name, mode):
    """trace_source=True with a residual: the plain layouts fuse reduction + LayerNorm but add the residual first (as
    plain merge does while tracing); the interleaved layouts do not fuse at all while tracing.  info["source"] is the same
    matrix in both arms.  Only the first block reduces here (r = [5]): its matching sees the same bits in both arms, so
    the comparison is about the source tracking and not about near-tied scores in later layers (see above)."""
    layers, on, off = _arms(host_name, mode, trace=True, r=[R])
    if host_name in FLAT:
        assert on["n"]["fused"] == 1 and on["n"]["fused_with_addend"] == 0 and on["n"]["norm2_layer_norm"] == layers - 1
    else:
        assert on["n"]["fused"] == 0 and on["n"]["norm2_layer_norm"] == layers
    assert off["n"]["fused"] == 0 and off["n"]["norm2_layer_norm"] == layers
    assert len(on["plans"]) == len(off["plans"]) == 1
    _same_schedule(on["plans"], off["plans"])
    assert not any(_differing(on["plans"][0], off["plans"][0]).values())
    assert on["source"] is not None and on["source"].shape == off["source"].shape
    assert torch.equal(on["source"], off["source"])
    assert float((on["out"] - off["out"]).abs().max()) <= 0.05 * max(1.0, float(off["out"].abs().max()))
