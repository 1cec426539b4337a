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
import sys

import torch

import ab
from tome import _attn
from tome.patch import _common as common

DEV = ab.DEV
SWITCH = (_attn, "NATIVE_ATTN_BACKWARD")


def case(B, H, N, bias, skip, dtype, rounds, iters):
    gen = torch.Generator(device=DEV).manual_seed(7)
    qkv = torch.randn(B, N, 3, H, 64, device=DEV, generator=gen).to(dtype).requires_grad_(True)
    heads = qkv.permute(2, 0, 3, 1, 4)
    g = torch.randn(B, N, H * 64, device=DEV, generator=gen).to(dtype)
    size = None
    if bias:
        size = torch.randint(1, 9, (B, N - int(skip), 1), device=DEV, generator=gen).to(dtype)

    def step():
        qkv.grad = None
        out = common.attention_qkv(heads, size, 0.125, 0.0, bias_skip=skip)
        out.backward(g)

    peak = {}

    def warm(native, run):
        run()  # warm-up (and the framework's kernel selection)
        qkv.grad = None  # (the warm-up's gradient buffer is not part of the inputs)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run()
        torch.cuda.synchronize()
        peak[native] = torch.cuda.max_memory_allocated() - base
        ab.time_us(run, iters)

    times = ab.alternate(ab.switch_arms(*SWITCH), rounds, iters, fn=step, warm=warm)
    flops = 4.0 * B * H * N * N * 64  # the forward's two tile products; the backward recomputes and adds eight
    nat, fw = ab.summary(times[True]), ab.summary(times[False])
    return {"B": B, "H": H, "N": N, "bias": bool(bias), "skip": bool(skip), "dtype": str(dtype).replace("torch.", ""),
            "native_fwd_bwd": nat, "framework_fwd_bwd": fw,
            "native_peak_bytes_above_inputs": int(peak[True]), "framework_peak_bytes_above_inputs": int(peak[False]),
            "speedup_median": round(fw["median_us"] / nat["median_us"], 2),
            "native_tflops_fwd_plus_bwd_products": round(5.0 * flops / nat["median_us"] / 1e6, 1),
            "native_median_below_framework_median": ab.median_below_median(nat, fw)}


def model_step(rounds, iters, batch):
    """One forward + backward of the patched bf16 VideoMAE-B host (r = 16, prop_attn, .train()) with the flag on and off."""
    import tome
    from hosts import videomae
    times = ab.model_train_step(videomae.VideoMAE, tome.patch.videomae, (3, 16, 224, 224), batch, 16, SWITCH, rounds,
                                iters, warm=1, dtype=torch.bfloat16, prop_attn=True)
    on, off = ab.summary(times[True]), ab.summary(times[False])
    return {"model": "VideoMAE-B 16x224 bf16 r=16 prop_attn train step", "batch": batch, "native_attn_backward": on,
            "framework_attn_backward": off, "speedup_median": round(off["median_us"] / on["median_us"], 3)}


def main():
    ap = ab.parser(iters=5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=8)
    a = ap.parse_args()
    shapes = [(8, 12, 1568, False), (128, 12, 1568, False), (8, 12, 3137, False), (64, 12, 197, True)]
    if a.quick:
        shapes = shapes[:1]
    lines, ok = ab.Lines(a.out), True
    for B, H, N, skip in shapes:
        for bias in (True, False):
            res = case(B, H, N, bias, skip, torch.bfloat16, a.rounds, a.iters)
            ok = ok and res["native_median_below_framework_median"]
            torch.cuda.empty_cache()
            lines.emit(res)
    if not a.no_model:
        lines.emit(model_step(max(3, a.rounds // 2), 2, a.model_batch))
    lines.write()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
