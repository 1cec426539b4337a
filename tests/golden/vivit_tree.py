"""ViViT as transformers 4.x laid it out, in plain PyTorch: the module tree that a ToMe patch for ViViT written
against 4.x expects (`VivitLayer` / `VivitAttention` / `VivitSelfAttention` with `query`, `key`, `value`,
`transpose_for_scores`), which transformers 5.x no longer has (it keeps `VivitAttention` with q_proj / k_proj / v_proj
and a `VivitMLP`).  Stand-in for the golden generator (tests/golden/generate_models.py registers these classes under
the module names the reference's patch imports from) and pinned to the installed `VivitForVideoClassification` by
tests/test_vivit_tree_cpu.py: same weights, same logits.

Framework ops only.  Imports nothing of this repository's package (`hosts`, `tome`): the generator puts the
reference's `tome` into sys.modules, and a fixture made by the code under test would pin nothing.  The activation is
the installed transformers' own `gelu_fast` where there is one."""
from __future__ import annotations

import math

import torch
from torch import nn

try:
    from transformers.activations import ACT2FN
    _gelu_fast = ACT2FN["gelu_fast"]
except Exception:  # pragma: no cover - no transformers: the same formula, spelled out
    class _GeluFast(nn.Module):
        def forward(self, x):
            return 0.5 * x * (1.0 + torch.tanh(x * 0.7978845608 * (1.0 + 0.044715 * x * x)))
    _gelu_fast = _GeluFast()


class VivitConfig:
    def __init__(self, image_size=224, num_frames=32, tubelet_size=(2, 16, 16), num_channels=3, hidden_size=768,
                 num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, layer_norm_eps=1e-6,
                 qkv_bias=True):
        self.image_size, self.num_frames, self.tubelet_size = image_size, num_frames, tuple(tubelet_size)
        self.num_channels, self.hidden_size = num_channels, hidden_size
        self.num_hidden_layers, self.num_attention_heads = num_hidden_layers, num_attention_heads
        self.intermediate_size, self.layer_norm_eps, self.qkv_bias = intermediate_size, layer_norm_eps, qkv_bias


class VivitTubeletEmbeddings(nn.Module):
    def __init__(self, config):
        super().__init__()
        t, h, w = config.tubelet_size
        self.num_patches = (config.image_size // h) * (config.image_size // w) * (config.num_frames // t)
        self.projection = nn.Conv3d(config.num_channels, config.hidden_size, kernel_size=config.tubelet_size,
                                    stride=config.tubelet_size)

    def forward(self, pixel_values):  # [B, T, C, H, W]
        x = self.projection(pixel_values.permute(0, 2, 1, 3, 4))
        return x.flatten(2).transpose(1, 2)


class VivitEmbeddings(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.cls_token = nn.Parameter(torch.zeros(1, 1, config.hidden_size))
        self.patch_embeddings = VivitTubeletEmbeddings(config)
        self.position_embeddings = nn.Parameter(torch.zeros(1, self.patch_embeddings.num_patches + 1, config.hidden_size))
        self.dropout = nn.Dropout(0.0)

    def forward(self, pixel_values):
        x = self.patch_embeddings(pixel_values)
        x = torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1)
        return self.dropout(x + self.position_embeddings)


class VivitSelfAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.num_attention_heads = config.num_attention_heads
        self.attention_head_size = config.hidden_size // config.num_attention_heads
        self.all_head_size = self.num_attention_heads * self.attention_head_size
        self.query = nn.Linear(config.hidden_size, self.all_head_size, bias=config.qkv_bias)
        self.key = nn.Linear(config.hidden_size, self.all_head_size, bias=config.qkv_bias)
        self.value = nn.Linear(config.hidden_size, self.all_head_size, bias=config.qkv_bias)
        self.dropout = nn.Dropout(0.0)

    def transpose_for_scores(self, x):  # [B, N, H * hd] -> [B, H, N, hd]
        return x.view(x.shape[0], x.shape[1], self.num_attention_heads, self.attention_head_size).permute(0, 2, 1, 3)

    def forward(self, hidden_states, head_mask=None, output_attentions=False):
        q = self.transpose_for_scores(self.query(hidden_states))
        k = self.transpose_for_scores(self.key(hidden_states))
        v = self.transpose_for_scores(self.value(hidden_states))
        probs = self.dropout(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(self.attention_head_size), dim=-1))
        if head_mask is not None:
            probs = probs * head_mask
        ctx = (probs @ v).permute(0, 2, 1, 3).reshape(hidden_states.shape[0], -1, self.all_head_size)
        return (ctx, probs) if output_attentions else (ctx,)


class VivitSelfOutput(nn.Module):
    """The projection behind the attention; the residual is added by the layer."""

    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.dropout = nn.Dropout(0.0)

    def forward(self, hidden_states, input_tensor):
        return self.dropout(self.dense(hidden_states))


class VivitAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.attention = VivitSelfAttention(config)
        self.output = VivitSelfOutput(config)

    def forward(self, hidden_states, head_mask=None, output_attentions=False):
        outs = self.attention(hidden_states, head_mask, output_attentions)
        return (self.output(outs[0], hidden_states),) + outs[1:]


class VivitIntermediate(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.intermediate_size)
        self.dropout = nn.Dropout(0.0)
        self.intermediate_act_fn = _gelu_fast

    def forward(self, hidden_states):
        return self.dropout(self.intermediate_act_fn(self.dense(hidden_states)))


class VivitOutput(nn.Module):
    """The second projection of the MLP; this one adds its residual itself."""

    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.intermediate_size, config.hidden_size)
        self.dropout = nn.Dropout(0.0)

    def forward(self, hidden_states, input_tensor):
        return self.dropout(self.dense(hidden_states)) + input_tensor


class VivitLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.attention = VivitAttention(config)
        self.intermediate = VivitIntermediate(config)
        self.output = VivitOutput(config)
        self.layernorm_before = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.layernorm_after = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)

    def forward(self, hidden_states, head_mask=None, output_attentions=False):
        outs = self.attention(self.layernorm_before(hidden_states), head_mask, output_attentions)
        hidden_states = outs[0] + hidden_states
        return (self.output(self.intermediate(self.layernorm_after(hidden_states)), hidden_states),) + outs[1:]


class VivitEncoder(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.layer = nn.ModuleList([VivitLayer(config) for _ in range(config.num_hidden_layers)])

    def forward(self, hidden_states, head_mask=None, output_attentions=False):
        for i, layer in enumerate(self.layer):
            hidden_states = layer(hidden_states, None if head_mask is None else head_mask[i], output_attentions)[0]
        return hidden_states


class VivitModel(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.embeddings = VivitEmbeddings(config)
        self.encoder = VivitEncoder(config)
        self.layernorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)

    def forward(self, pixel_values):
        return (self.layernorm(self.encoder(self.embeddings(pixel_values))),)


class ViViT(nn.Module):
    """The video-classification wrapper: `.vivit`, `.classifier`; takes the list of pathways with one [B, C, T, H, W]
    clip and answers the logits of token 0."""

    def __init__(self, config: VivitConfig, num_classes=400):
        super().__init__()
        self.config = config
        self.num_labels = num_classes
        self.vivit = VivitModel(config)
        self.classifier = nn.Linear(config.hidden_size, num_classes)

    def forward(self, pixel_values):
        seq = self.vivit(pixel_values[0].permute(0, 2, 1, 3, 4))[0]
        return self.classifier(seq[:, 0, :])
