#!/usr/bin/env python3
"""Forward + backward of add + LayerNorm on tokens that require grad: the native Functions of tome/_ln.py (inference
kernel forward, k_ln_rows_bwd + k_ln_param_grad backward) against the framework chain (`x + a`, `F.layer_norm`,
autograd), in one process, alternated rounds, device events; the backward launch alone as bytes over time (4 x rows x C
x 2 bytes with gx_in, 3 x without; parameter gradients included); and one forward + backward step of the patched bf16
VideoMAE-B host with tome._ln.NATIVE_LN_BACKWARD on and off.

Shapes: C = 768, rows of the benchmark's models: VideoMAE [n, 1568] at n = 64 and 384, TimeSformer [64, 1 + 196*8]
(skip_first).  Prints one JSON line per case; exit status 1 when a native median is not below the framework's.
`--quick` runs the smallest case only, `--no-model` leaves the model step out."""
import sys

import torch

import ab
from tome import _abi, _ln

DEV = ab.DEV


def case(n, N, skip_first, dtype, rounds, iters, C=768):
    gen = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(n, N, C, device=DEV, generator=gen).to(dtype).requires_grad_(True)
    a = torch.randn(n, N, C, device=DEV, generator=gen).to(dtype).requires_grad_(True)
    norm = torch.nn.LayerNorm(C).to(DEV).to(dtype)
    g_sum = torch.randn(n, N, C, device=DEV, generator=gen).to(dtype)
    g_y = torch.randn(n, N - 1 if skip_first else N, C, device=DEV, generator=gen).to(dtype)

    def native():
        return _ln.add_layernorm_native(x, a, norm, skip_first=skip_first)

    def framework():
        s = x + a
        y = torch.nn.functional.layer_norm(s, (C,), norm.weight, norm.bias, norm.eps)
        return s, (y[:, 1:] if skip_first else y)

    def step(fwd):
        x.grad = a.grad = norm.weight.grad = norm.bias.grad = None
        s, y = fwd()
        torch.autograd.backward((s, y), (g_sum, g_y))

    times = ab.alternate({"native": lambda: step(native), "framework": lambda: step(framework)}, rounds, iters,
                         warm=iters)
    nat, fw = ab.summary(times["native"]), ab.summary(times["framework"])
    out = {"n": n, "rows_per_clip": N, "C": C, "skip_first": skip_first, "dtype": str(dtype).replace("torch.", ""),
           "native_fwd_bwd": nat, "framework_fwd_bwd": fw,
           "speedup_median": round(fw["median_us"] / nat["median_us"], 2),
           "native_median_below_framework_median": ab.median_below_median(nat, fw)}
    with torch.no_grad():
        xs = (x + a).detach()
        for label, gi, params, passes in (("backward_launch", g_sum, True, 4), ("backward_launch_no_gx_in", None, True, 3),
                                          ("backward_launch_frozen", g_sum, False, 4)):
            bwd = lambda: _abi.layernorm_backward(g_y, xs, gi, norm.weight, norm.eps, skip_first=skip_first,  # noqa: E731
                                                  want_weight=params, want_bias=params)
            out[label] = ab.bandwidth(ab.launch_alone(bwd, rounds, iters), passes * n * N * C * x.element_size())
    return out


def model_step(rounds, iters, batch):
    """One forward + backward of the patched bf16 VideoMAE-B host (r = 16, .train()) with the flag on and off."""
    import tome
    from hosts import videomae
    times = ab.model_train_step(videomae.VideoMAE, tome.patch.videomae, (3, 16, 224, 224), batch, 16,
                                (_ln, "NATIVE_LN_BACKWARD"), rounds, iters, warm=1, dtype=torch.bfloat16)
    on, off = ab.summary(times[True]), ab.summary(times[False])
    return {"model": "VideoMAE-B 16x224 bf16 r=16 train step", "batch": batch, "native_ln_backward": on,
            "framework_ln_backward": off, "speedup_median": round(off["median_us"] / on["median_us"], 3)}


def main():
    ap = ab.parser()
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=16)
    a = ap.parse_args()
    cases = [(64, 1568, False), (384, 1568, False), (64, 1 + 196 * 8, True)]
    if a.quick:
        cases = cases[:1]
    lines, ok = ab.Lines(a.out), True
    for n, N, skip in cases:
        res = case(n, N, skip, torch.bfloat16, a.rounds, a.iters)
        ok = ok and res["native_median_below_framework_median"]
        torch.cuda.empty_cache()
        lines.emit(res)
    if not a.no_model:
        lines.emit(model_step(max(3, a.rounds // 2), 2, a.model_batch))
    lines.write()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
