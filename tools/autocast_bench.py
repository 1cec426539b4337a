#!/usr/bin/env python3
"""add + LayerNorm under torch.autocast with fp32 master weights (how the reference trains and benchmarks:
tools/train_net.py:123, tome/utils.py:54): the mixed-precision kernels (tome_add_layernorm_amp,
tome_layernorm_backward_amp) against the path with tome._ln.NATIVE_LN_AUTOCAST off -- the framework's `x + a`, its fp32
layer_norm and the cast the consuming Linear makes.  One process, alternated rounds, device events, medians with
min-max.

Op level, C = 768, bf16 autocast: forward (no_grad) and forward + backward (x, addend, weight and bias require grad) at
    8 x 1568 rows, 16-bit stream (VideoMAE: `pos_embed.type_as(x)` keeps the patch embedding's dtype)
    8 x (1 + 196 * 8) rows, fp32 stream with a 16-bit addend (TimeSformer, Motionformer, ViViT: `x + self.pos_embed`)
Stack level: one forward + backward of a two-block patched stack of every family, full width, `.train()`, r = 16.

One JSON line per case; `native_slower_beyond_spread` says whether the native median is above the switch-off median by
more than the larger of the two min-max spreads (the project's rule for excluding a shape from a default-on switch).
The exit status is always 0: this tool reports, it does not judge.
`--out` (default profiles/r07_autocast_bench.jsonl) also receives the lines.  `--quick`: op level only."""
import os
import sys

import torch

import ab
from tome import _ln

DEV = ab.DEV
HALF = torch.bfloat16
SWITCH = (_ln, "NATIVE_LN_AUTOCAST")


def report(times):
    a, b = ab.summary(times[True]), ab.summary(times[False])
    return {"native": a, "switch_off": b, "speedup_median": round(b["median_us"] / a["median_us"], 3),
            "native_slower_beyond_spread": ab.tie_within_spread(a, b) != "tie"}


def op_case(n, N, stream, rounds, iters, C=768):
    gen = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(n, N, C, device=DEV, generator=gen).to(stream)
    a = torch.randn(n, N, C, device=DEV, generator=gen).to(HALF)
    norm = torch.nn.LayerNorm(C).to(DEV)  # fp32 master weights
    g_sum = torch.randn(n, N, C, device=DEV, generator=gen).to(stream)
    g_y = torch.randn(n, N, C, device=DEV, generator=gen).to(HALF)

    def op(xi, ai):
        out = _ln.add_layernorm(xi, ai, norm)
        if out is not None:
            return out[0], out[1]
        s = xi + ai
        return s, norm(s).to(HALF)  # the framework's fp32 layer_norm, then the cast the consuming Linear makes

    def forward():
        with torch.no_grad(), torch.autocast("cuda", dtype=HALF):
            op(x, a)

    xg, ag = x.clone().requires_grad_(True), a.clone().requires_grad_(True)

    def step():
        xg.grad = ag.grad = norm.weight.grad = norm.bias.grad = None
        with torch.autocast("cuda", dtype=HALF):
            s, y = op(xg, ag)
        torch.autograd.backward((s, y), (g_sum, g_y))

    with torch.autocast("cuda", dtype=HALF):
        assert _ln.route(xg, norm, ag) == _ln.AMP_FUNCTION and _ln.route(x.detach(), norm, a) in (_ln.AMP_DIRECT, _ln.AMP_FUNCTION)
    out = {"level": "op", "rows": n * N, "n": n, "rows_per_clip": N, "C": C, "stream": str(stream).replace("torch.", ""),
           "autocast": "bfloat16"}
    for label, fn in (("forward", forward), ("forward_backward", step)):
        out[label] = report(ab.alternate(ab.switch_arms(*SWITCH), rounds, iters, fn=fn, warm=2))
    return out


def _stacks():
    import tome
    from hosts import motionformer, timesformer, videomae, vivit
    return (
        ("videomae", lambda: videomae.VideoMAE(depth=2), (3, 16, 224, 224), tome.patch.videomae),
        ("timesformer", lambda: timesformer.TimeSformer(depth=2), (3, 8, 224, 224), tome.patch.timesformer),
        ("motionformer", lambda: motionformer.Motionformer(depth=2), (3, 16, 224, 224), tome.patch.motionformer),
        ("vivit", lambda: vivit.ViViT(num_hidden_layers=2), (3, 32, 224, 224), tome.patch.vivit))


def stack_case(name, make, clip_shape, patch, rounds, iters, batch):
    times = ab.model_train_step(make, patch, clip_shape, batch, 16, SWITCH, rounds, iters, warm=2, autocast=HALF,
                                prop_attn=True)
    return dict({"level": "stack", "family": name, "blocks": 2, "batch": batch, "mode": "train", "r": 16,
                 "autocast": "bfloat16"}, forward_backward=report(times))


def main():
    ap = ab.parser(out=os.path.join(ab.ROOT, "profiles", "r07_autocast_bench.jsonl"))
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    lines = ab.Lines(a.out)
    lines.emit(op_case(8, 1568, HALF, a.rounds, a.iters))
    lines.emit(op_case(8, 1 + 196 * 8, torch.float32, a.rounds, a.iters))
    if not a.quick:
        for name, make, clip_shape, patch in _stacks():
            torch.cuda.empty_cache()
            lines.emit(stack_case(name, make, clip_shape, patch, a.rounds, max(1, a.iters // 3), a.batch))
    lines.write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
