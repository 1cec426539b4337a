"""tests/golden/vivit_tree.py IS ViViT: the stand-in module tree that the golden generator hands to the reference's
ViViT patch (which is written against transformers 4.x class names the installed 5.x no longer has) gives, with the
same weights, the logits of the installed `VivitForVideoClassification` -- the check of test_vivit_host_vs_hf.py, its
rename map, its two shapes and its tolerances, on the tree.  And the tree's parameter names are those of
`hosts.vivit.ViViT` for the fixtures' configuration: the fixtures fill weights by NAME on both sides.  CPU only."""
import importlib.util
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "video-how-do-your-tokens-merge_amd")]

try:
    from transformers import VivitConfig as HFConfig
    from transformers import VivitForVideoClassification as HFViViT
except Exception:  # pragma: no cover - transformers without ViViT
    HFViViT = None

from test_vivit_host_vs_hf import _rename  # noqa: E402


def _tree():
    spec = importlib.util.spec_from_file_location(
        "vivit_tree", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vivit_tree.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tree_imports_nothing_of_the_package_under_test():
    before = {m for m in sys.modules if m == "hosts" or m.startswith("hosts.") or m == "tome" or m.startswith("tome.")}
    _tree()
    after = {m for m in sys.modules if m == "hosts" or m.startswith("hosts.") or m == "tome" or m.startswith("tome.")}
    assert after == before
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vivit_tree.py")).read()
    assert "import hosts" not in text and "from hosts" not in text and "import tome" not in text and "from tome" not in text


@pytest.mark.skipif(HFViViT is None, reason="installed transformers has no ViViT")
@pytest.mark.parametrize("frames,size,tubelet,hidden,layers,heads", [(8, 32, (2, 8, 8), 32, 2, 2), (4, 48, (2, 16, 16), 48, 3, 4)])
def test_tree_equals_hf_vivit(frames, size, tubelet, hidden, layers, heads):
    T = _tree()
    torch.manual_seed(0)
    hf = HFViViT(HFConfig(image_size=size, num_frames=frames, tubelet_size=list(tubelet), hidden_size=hidden,
                          num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=2 * hidden,
                          num_labels=5, hidden_act="gelu_fast", layer_norm_eps=1e-6, qkv_bias=True,
                          attn_implementation="eager")).eval()
    with torch.no_grad():  # HF initialises biases / cls token to zero: randomise everything so each term counts
        for p in hf.parameters():
            p.copy_(torch.randn_like(p) * 0.1)
    tree = T.ViViT(T.VivitConfig(image_size=size, num_frames=frames, tubelet_size=tubelet, hidden_size=hidden,
                                 num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=2 * hidden,
                                 layer_norm_eps=1e-6, qkv_bias=True), num_classes=5).eval()
    sd = {_rename(k): v for k, v in hf.state_dict().items()}
    missing, unexpected = tree.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    clip = torch.rand(2, 3, frames, size, size)
    with torch.no_grad():
        want = hf(pixel_values=clip.permute(0, 2, 1, 3, 4)).logits
        got = tree([clip])
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("embed", [32, 128])
def test_tree_parameter_names_are_the_host_models(embed):
    """The fixture configuration of tests/golden/generate_models.py (reduced_families: vivit)."""
    from hosts.vivit import ViViT, VivitConfig
    T = _tree()
    kw = dict(image_size=32, num_frames=8, tubelet_size=(2, 8, 8), hidden_size=embed, num_hidden_layers=4,
              num_attention_heads=2, intermediate_size=4 * embed, layer_norm_eps=1e-6, qkv_bias=True)
    tree = T.ViViT(T.VivitConfig(**kw), num_classes=10)
    host = ViViT(VivitConfig(**kw), num_classes=10)
    want = {n: tuple(p.shape) for n, p in host.named_parameters()}
    got = {n: tuple(p.shape) for n, p in tree.named_parameters()}
    assert got == want
    tokens = 1 + (8 // 2) * (32 // 8) ** 2
    assert got["vivit.embeddings.position_embeddings"] == (1, tokens, embed) and tokens == 65
