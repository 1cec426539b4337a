#!/usr/bin/env python3
"""Forward + backward of the patched blocks' proportional attention on heads that require grad: the native Function of
tome/_attn.py (tome_prop_attention forward, k_attn_bwd_dq + k_attn_bwd_dkv backward) against the framework path of
tome/patch/_common.py:attention under grad (scaled_dot_product_attention with the bias tensor the reference builds, and
autograd), in one process, alternated rounds in the same order, device events, medians; peak memory of one step of each
path; and one forward + backward step of the patched bf16 VideoMAE-B host with tome._attn.NATIVE_ATTN_BACKWARD on and off.

Shapes (B x H x N, head dim 64, bf16, q/k/v = the slices of one qkv buffer): 8 x 12 x 1568, 128 x 12 x 1568,
8 x 12 x 3137, TimeSformer's (8*8) x 12 x 197 in the skip form; each with and without the size bias.  Prints one JSON
line per case; exit status 1 when a native median is not below the framework's at some shape.  `--quick` runs the
smallest case only, `--no-model` leaves the model step out."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-how-do-your-tokens-merge_amd"))

from tome import _attn  # noqa: E402
from tome.patch import _common as common  # noqa: E402

DEV = "cuda:0"


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


def case(B, H, N, bias, skip, dtype, rounds, iters):
    gen = torch.Generator(device=DEV).manual_seed(7)
    qkv = torch.randn(B, N, 3, H, 64, device=DEV, generator=gen).to(dtype).requires_grad_(True)
    heads = qkv.permute(2, 0, 3, 1, 4)
    g = torch.randn(B, N, H * 64, device=DEV, generator=gen).to(dtype)
    size = None
    if bias:
        size = torch.randint(1, 9, (B, N - int(skip), 1), device=DEV, generator=gen).to(dtype)

    def step(native):
        _attn.NATIVE_ATTN_BACKWARD = native
        qkv.grad = None
        out = common.attention_qkv(heads, size, 0.125, 0.0, bias_skip=skip)
        out.backward(g)

    peak = {}
    for native in (True, False):
        step(native)  # warm-up (and the framework's kernel selection)
        qkv.grad = None  # (the warm-up's gradient buffer is not part of the inputs)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(native)
        torch.cuda.synchronize()
        peak[native] = torch.cuda.max_memory_allocated() - base
        _time(lambda: step(native), iters)
    times = {True: [], False: []}
    for _ in range(rounds):
        for native in (True, False):
            times[native].append(_time(lambda: step(native), iters))
    _attn.NATIVE_ATTN_BACKWARD = True
    flops = 4.0 * B * H * N * N * 64  # the forward's two tile products; the backward recomputes and adds eight
    out = {"B": B, "H": H, "N": N, "bias": bool(bias), "skip": bool(skip), "dtype": str(dtype).replace("torch.", ""),
           "native_fwd_bwd": _stats(times[True]), "framework_fwd_bwd": _stats(times[False]),
           "native_peak_bytes_above_inputs": int(peak[True]), "framework_peak_bytes_above_inputs": int(peak[False])}
    out["speedup_median"] = round(out["framework_fwd_bwd"]["median_us"] / out["native_fwd_bwd"]["median_us"], 2)
    out["native_tflops_fwd_plus_bwd_products"] = round(5.0 * flops / out["native_fwd_bwd"]["median_us"] / 1e6, 1)
    out["native_median_below_framework_median"] = (out["native_fwd_bwd"]["median_us"]
                                                   < out["framework_fwd_bwd"]["median_us"])
    return out


def model_step(rounds, iters, batch):
    """One forward + backward of the patched bf16 VideoMAE-B host (r = 16, prop_attn, .train()) with the flag on and off."""
    import tome
    from hosts import videomae
    torch.manual_seed(0)
    model = videomae.VideoMAE().to(DEV).to(torch.bfloat16).train()
    tome.patch.videomae(model, prop_attn=True)
    model.r = 16
    clip = torch.rand(batch, 3, 16, 224, 224, device=DEV).to(torch.bfloat16)

    def step():
        model.zero_grad(set_to_none=True)
        model([clip]).float().square().sum().backward()

    times = {True: [], False: []}
    for flag in (True, False):
        _attn.NATIVE_ATTN_BACKWARD = flag
        _time(step, 1)
    for _ in range(rounds):
        for flag in (True, False):
            _attn.NATIVE_ATTN_BACKWARD = flag
            times[flag].append(_time(step, iters))
    _attn.NATIVE_ATTN_BACKWARD = True
    on, off = _stats(times[True]), _stats(times[False])
    return {"model": "VideoMAE-B 16x224 bf16 r=16 prop_attn train step", "batch": batch, "native_attn_backward": on,
            "framework_attn_backward": off, "speedup_median": round(off["median_us"] / on["median_us"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    shapes = [(8, 12, 1568, False), (128, 12, 1568, False), (8, 12, 3137, False), (64, 12, 197, True)]
    if a.quick:
        shapes = shapes[:1]
    lines, ok = [], True
    for B, H, N, skip in shapes:
        for bias in (True, False):
            res = case(B, H, N, bias, skip, torch.bfloat16, a.rounds, a.iters)
            ok = ok and res["native_median_below_framework_median"]
            torch.cuda.empty_cache()
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    if not a.no_model:
        lines.append(json.dumps(model_step(max(3, a.rounds // 2), 2, a.model_batch)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
