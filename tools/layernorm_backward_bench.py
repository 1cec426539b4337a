#!/usr/bin/env python3
"""Forward + backward of add + LayerNorm on tokens that require grad: the native Functions of tome/_ln.py (inference
kernel forward, k_ln_rows_bwd + k_ln_param_grad backward) against the framework chain (`x + a`, `F.layer_norm`,
autograd), in one process, alternated rounds, device events; the backward launch alone as bytes over time (4 x rows x C
x 2 bytes with gx_in, 3 x without; parameter gradients included); and one forward + backward step of the patched bf16
VideoMAE-B host with tome._ln.NATIVE_LN_BACKWARD on and off.

Shapes: C = 768, rows of the benchmark's models: VideoMAE [n, 1568] at n = 64 and 384, TimeSformer [64, 1 + 196*8]
(skip_first).  Prints one JSON line per case; exit status 1 when a native median is not below the framework's.
`--quick` runs the smallest case only, `--no-model` leaves the model step out."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-how-do-your-tokens-merge_amd"))

from tome import _abi, _ln  # noqa: E402

DEV = "cuda:0"
PEAK_TBS = 8.0


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

    for fwd in (native, framework):
        _time(lambda: step(fwd), iters)
    times = {native: [], framework: []}
    for _ in range(rounds):
        for fwd in (native, framework):
            times[fwd].append(_time(lambda: step(fwd), iters))
    out = {"n": n, "rows_per_clip": N, "C": C, "skip_first": skip_first, "dtype": str(dtype).replace("torch.", ""),
           "native_fwd_bwd": _stats(times[native]), "framework_fwd_bwd": _stats(times[framework])}
    out["speedup_median"] = round(out["framework_fwd_bwd"]["median_us"] / out["native_fwd_bwd"]["median_us"], 2)
    out["native_median_below_framework_median"] = (out["native_fwd_bwd"]["median_us"]
                                                   < out["framework_fwd_bwd"]["median_us"])
    with torch.no_grad():
        xs = (x + a).detach()
        for label, gi, params, passes in (("backward_launch", g_sum, True, 4), ("backward_launch_no_gx_in", None, True, 3),
                                          ("backward_launch_frozen", g_sum, False, 4)):
            bwd = lambda: _abi.layernorm_backward(g_y, xs, gi, norm.weight, norm.eps, skip_first=skip_first,  # noqa: E731
                                                  want_weight=params, want_bias=params)
            bwd()
            launch = [_time(bwd, iters) for _ in range(rounds)]
            nbytes = passes * n * N * C * x.element_size()
            med = statistics.median(launch)
            out[label] = dict(_stats(launch), bytes=nbytes, TBps=round(nbytes / med / 1e6, 2),
                              share_of_8TBps=round(nbytes / med / 1e6 / PEAK_TBS, 3))
    return out


def model_step(rounds, iters, batch):
    """One forward + backward of the patched bf16 VideoMAE-B host (r = 16, .train()) with the flag on and off."""
    import tome
    from hosts import videomae
    torch.manual_seed(0)
    model = videomae.VideoMAE().to(DEV).to(torch.bfloat16).train()
    tome.patch.videomae(model)
    model.r = 16
    clip = torch.rand(batch, 3, 16, 224, 224, device=DEV).to(torch.bfloat16)

    def step():
        model.zero_grad(set_to_none=True)
        model([clip]).float().square().sum().backward()

    times = {True: [], False: []}
    for flag in (True, False):
        _ln.NATIVE_LN_BACKWARD = flag
        _time(step, 1)
    for _ in range(rounds):
        for flag in (True, False):
            _ln.NATIVE_LN_BACKWARD = flag
            times[flag].append(_time(step, iters))
    _ln.NATIVE_LN_BACKWARD = True
    on, off = _stats(times[True]), _stats(times[False])
    return {"model": "VideoMAE-B 16x224 bf16 r=16 train step", "batch": batch, "native_ln_backward": on,
            "framework_ln_backward": off, "speedup_median": round(off["median_us"] / on["median_us"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    cases = [(64, 1568, False), (384, 1568, False), (64, 1 + 196 * 8, True)]
    if a.quick:
        cases = cases[:1]
    lines, ok = [], True
    for n, N, skip in cases:
        res = case(n, N, skip, torch.bfloat16, a.rounds, a.iters)
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
