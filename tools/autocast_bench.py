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
`--out` (default profiles/r07_autocast_bench.jsonl) also receives the lines.  `--quick`: op level only."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-how-do-your-tokens-merge_amd"))

from tome import _ln  # noqa: E402

DEV = "cuda:0"
HALF = torch.bfloat16


def _time(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters  # us


def _stats(xs):
    return {"median_us": round(statistics.median(xs), 1), "min_us": round(min(xs), 1), "max_us": round(max(xs), 1)}


def _compare(native, off):
    a, b = _stats(native), _stats(off)
    spread = max(a["max_us"] - a["min_us"], b["max_us"] - b["min_us"])
    return {"native": a, "switch_off": b, "speedup_median": round(b["median_us"] / a["median_us"], 3),
            "native_slower_beyond_spread": a["median_us"] - b["median_us"] > spread}


def _alternate(fn, rounds, iters):
    """fn() timed with the switch on and off in alternated rounds; ({True: [...], False: [...]})."""
    times = {True: [], False: []}
    for flag in (True, False):
        _ln.NATIVE_LN_AUTOCAST = flag
        _time(fn, 2)
    for _ in range(rounds):
        for flag in (True, False):
            _ln.NATIVE_LN_AUTOCAST = flag
            times[flag].append(_time(fn, iters))
    _ln.NATIVE_LN_AUTOCAST = True
    return times


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
        t = _alternate(fn, rounds, iters)
        out[label] = _compare(t[True], t[False])
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
    torch.manual_seed(0)
    model = make().to(DEV).train()
    patch(model, prop_attn=True)
    clip = torch.rand(batch, *clip_shape, device=DEV)

    def step():
        model.zero_grad(set_to_none=True)
        model.r = 16
        with torch.autocast("cuda", dtype=HALF):
            out = model([clip])
        out.float().square().sum().backward()

    t = _alternate(step, rounds, iters)
    return dict({"level": "stack", "family": name, "blocks": 2, "batch": batch, "mode": "train", "r": 16,
                 "autocast": "bfloat16"}, forward_backward=_compare(t[True], t[False]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_autocast_bench.jsonl"))
    a = ap.parse_args()
    lines = []

    def emit(res):
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)

    emit(op_case(8, 1568, HALF, a.rounds, a.iters))
    emit(op_case(8, 1 + 196 * 8, torch.float32, a.rounds, a.iters))
    if not a.quick:
        for name, make, clip_shape, patch in _stacks():
            torch.cuda.empty_cache()
            emit(stack_case(name, make, clip_shape, patch, a.rounds, max(1, a.iters // 3), a.batch))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
