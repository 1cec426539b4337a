"""The arming predicate of the pooled tail (tome/patch/videomae.py::pooled_tail_block, tome/patch/_common.py::
pool_tail_modules_ok / pool_tail_armed), which involves modules only: no GPU, no launch.  A stock mean-pooling host model
in `.eval()` mode under no_grad names its last block; every entry of the fallback list names none."""
import pytest
import torch


def _model(dtype=torch.bfloat16, patch=True, **kw):
    import tome
    from hosts import videomae
    torch.manual_seed(0)
    m = videomae.VideoMAE(num_frames=4, img_size=32, patch_size=16, embed_dim=64, depth=2, num_heads=1, num_classes=5,
                          **kw).to(dtype).eval()
    if patch:
        tome.patch.videomae(m)
        m.r = 2
    return m


def _block_of(model):
    from tome.patch.videomae import pooled_tail_block
    with torch.no_grad():
        return pooled_tail_block(model)


def test_stock_model_names_its_last_block():
    model = _model()
    assert _block_of(model) is model.model.blocks[-1]
    assert _block_of(_model(torch.float16)) is not None
    assert "_pool_tail" not in model._tome_info  # the predicate itself arms nothing


def _append_duplicate(m):
    """A ToMeDuplicateBlock (attend for the metric, merge, no MLP) behind the last block."""
    import copy
    import sys
    from tome.patch import _common as C
    V = sys.modules["tome.patch.videomae"]
    dup = copy.deepcopy(m.model.blocks[-1])
    C.swizzle(dup, "ToMeDuplicateBlock", {"forward": V._duplicate_block_forward})
    dup._tome_info = m._tome_info
    m.model.blocks.append(dup)


FALLBACKS = {
    "train": lambda m: m.train(),
    "last block in train mode": lambda m: m.model.blocks[-1].train(),
    "hook on the last block": lambda m: m.model.blocks[-1].register_forward_hook(lambda *a: None),
    "pre-hook on the last block": lambda m: m.model.blocks[-1].register_forward_pre_hook(lambda *a: None),
    "hook on its mlp": lambda m: m.model.blocks[-1].mlp.register_forward_hook(lambda *a: None),
    "hook on its act": lambda m: m.model.blocks[-1].mlp.act.register_forward_hook(lambda *a: None),
    "hook on its fc2": lambda m: m.model.blocks[-1].mlp.fc2.register_forward_hook(lambda *a: None),
    "hook on the norm": lambda m: m.model.norm.register_forward_hook(lambda *a: None),
    "hook on the ViT": lambda m: m.model.register_forward_hook(lambda *a: None),
    "pre-hook on the ViT": lambda m: m.model.register_forward_pre_hook(lambda *a: None),
    "gamma_2": lambda m: setattr(m.model.blocks[-1], "gamma_2", torch.nn.Parameter(torch.ones(64, dtype=torch.bfloat16))),
    "drop_path": lambda m: setattr(m.model.blocks[-1], "drop_path", torch.nn.Dropout(0.0)),
    "fc2 without bias": lambda m: setattr(m.model.blocks[-1].mlp, "fc2", torch.nn.Linear(256, 64, bias=False).bfloat16()),
    "tanh GELU": lambda m: setattr(m.model.blocks[-1].mlp, "act", torch.nn.GELU(approximate="tanh")),
    "a weighted norm in front of the mean": lambda m: setattr(m.model, "norm", torch.nn.LayerNorm(64).bfloat16()),
    "forward put on the ViT instance": lambda m: setattr(m.model, "forward_features", lambda x: x),
    "duplicate block last": lambda m: _append_duplicate(m),
    "the last block also earlier in the list": lambda m: m.model.blocks.insert(0, m.model.blocks[-1]),
}


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_fallbacks_name_no_block(case):
    model = _model()
    assert _block_of(model) is not None
    FALLBACKS[case](model)
    assert _block_of(model) is None


def test_models_that_never_arm():
    from tome.patch.videomae import pooled_tail_block
    model = _model()
    with torch.enable_grad():
        assert pooled_tail_block(model) is None  # grad enabled
    assert _block_of(_model(torch.float32)) is None  # fp32 parameters: fp32 tokens
    assert _block_of(_model(use_mean_pooling=False)) is None  # the head reads x[:, 0] behind a LayerNorm
    assert _block_of(_model(init_values=0.1)) is None  # layer scale
    unpatched = _model(patch=False)
    unpatched._tome_info = {}
    assert _block_of(unpatched) is None  # not the patched wrapper class, no ToMeBlock

    from hosts import videomae

    class OtherViT(videomae.VisionTransformer):  # a subclass may read the tokens another way
        pass

    sub = _model(patch=False)
    sub.model.__class__ = OtherViT
    import tome
    tome.patch.videomae(sub)
    assert _block_of(sub) is None


def test_a_hook_registered_for_all_modules_disarms():
    model = _model()
    handle = torch.nn.modules.module.register_module_forward_hook(lambda *a: None)
    try:
        assert _block_of(model) is None
    finally:
        handle.remove()
    assert _block_of(model) is not None


def test_the_flag_is_popped_by_the_named_block_only_and_needs_device_tokens():
    from tome.patch import _common as C
    model = _model()
    first, last = model.model.blocks
    info = model._tome_info
    x = torch.zeros(1, 4, 64, dtype=torch.bfloat16)
    with torch.no_grad():
        assert not C.pool_tail_armed(last, x, info)  # never armed: a block called on its own
        info["_pool_tail"] = last
        assert not C.pool_tail_armed(first, x, info) and info["_pool_tail"] is last
        assert not C.pool_tail_armed(last, x, info)  # host tokens: the parent path ...
        assert "_pool_tail" not in info              # ... and the flag is gone all the same
