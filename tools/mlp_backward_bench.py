#!/usr/bin/env python3
"""The MLP `fc2(gelu(fc1(y)))` on tokens that require grad: the native Function of tome/_mlp.py (library GEMMs,
tome_gelu_erf forward, k_gelu_bwd between the backward's GEMMs) against the framework's modules and autograd.  Four
figures per case, one JSON line each:
  1. the backward launch alone as bytes over time: (4 with the activation, 3 without) x M x Hd x 2 bytes plus the fp32
     partial rows of the bias gradient;
  2. forward + backward of the MLP, native against framework, in one process, alternated rounds, device events, medians
     with min-max;
  3. bytes allocated between forward and backward on both paths;
  4. (once) one forward + backward step of the patched bf16 VideoMAE-B host with tome._mlp.NATIVE_MLP_BACKWARD on and off.
Shapes: C = 768, Hd = 3072, M = 8 x 1568, 64 x 1568 and 64 x 1569 (TimeSformer's row count); fc2 trainable and frozen.
`verdict`: "tie" when the native median is not above the framework's by more than the larger of the two paths' own
min-max spreads, "native slower" otherwise -- what DESIGN.md section 1 says about the default rests on it.
`--quick` runs the smallest shape only, `--no-model` leaves the model step out."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-how-do-your-tokens-merge_amd"))

from tome import _abi, _mlp  # noqa: E402

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


class Mlp(torch.nn.Module):
    def __init__(self, C, Hd):
        super().__init__()
        self.fc1, self.act, self.fc2 = torch.nn.Linear(C, Hd), torch.nn.GELU(), torch.nn.Linear(Hd, C)
        self.drop = torch.nn.Dropout(0.0)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


def case(M, fc2_trainable, dtype, rounds, iters, C=768, Hd=3072):
    gen = torch.Generator(device=DEV).manual_seed(7)
    torch.manual_seed(0)
    mlp = Mlp(C, Hd).to(DEV).to(dtype).train()
    mlp.fc2.weight.requires_grad_(fc2_trainable)
    y = torch.randn(M, C, device=DEV, generator=gen).to(dtype).requires_grad_(True)
    g = torch.randn(M, C, device=DEV, generator=gen).to(dtype)
    paths = {"native": lambda: _mlp.mlp_native(mlp, y), "framework": lambda: mlp(y)}

    def step(fwd):
        y.grad = None
        mlp.zero_grad(set_to_none=True)
        fwd().backward(g)

    held = {}
    for name, fwd in paths.items():
        step(fwd)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        out = fwd()
        torch.cuda.synchronize()
        held[name] = torch.cuda.memory_allocated() - base - out.numel() * out.element_size()
        out.backward(g)
        del out
    times = {name: [] for name in paths}
    for _ in range(rounds):
        for name, fwd in paths.items():
            times[name].append(_time(lambda: step(fwd), iters))
    nat, fw = _stats(times["native"]), _stats(times["framework"])
    spread = max(nat["max_us"] - nat["min_us"], fw["max_us"] - fw["min_us"])
    out = {"M": M, "C": C, "Hd": Hd, "fc2_trainable": fc2_trainable, "dtype": str(dtype).replace("torch.", ""),
           "native_fwd_bwd": nat, "framework_fwd_bwd": fw, "larger_spread_us": round(spread, 1),
           "native_over_framework_median": round(nat["median_us"] / fw["median_us"], 3),
           "verdict": "tie" if nat["median_us"] <= fw["median_us"] + spread else "native slower",
           "held_between_fwd_and_bwd_bytes": held, "one_hidden_tensor_bytes": M * Hd * y.element_size()}
    with torch.no_grad():
        h = mlp.fc1(y)
        ga = torch.randn(M, Hd, device=DEV, generator=gen).to(dtype)
        bwd = lambda: _abi.gelu_erf_backward(h, ga, want_act=fc2_trainable, want_bias=True, inplace=True)  # noqa: E731
        bwd()
        launch = [_time(bwd, iters) for _ in range(rounds)]
        parts = _abi.lib().tome_gelu_erf_backward_workspace_bytes(M, Hd)
        nbytes = (4 if fc2_trainable else 3) * M * Hd * y.element_size() + parts
        med = statistics.median(launch)
        out["backward_launch"] = dict(_stats(launch), bytes=nbytes, TBps=round(nbytes / med / 1e6, 2),
                                      share_of_8TBps=round(nbytes / med / 1e6 / PEAK_TBS, 3))
    return out


def model_step(rounds, iters, batch):
    """One forward + backward of the patched bf16 VideoMAE-B host (r = 16, .train()) with the switch on and off."""
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

    times, peak = {True: [], False: []}, {}
    for flag in (True, False):
        _mlp.NATIVE_MLP_BACKWARD = flag
        _time(step, 1)
        torch.cuda.reset_peak_memory_stats()
        _time(step, 1)
        peak[flag] = torch.cuda.max_memory_allocated()
    for _ in range(rounds):
        for flag in (True, False):
            _mlp.NATIVE_MLP_BACKWARD = flag
            times[flag].append(_time(step, iters))
    _mlp.NATIVE_MLP_BACKWARD = True
    on, off = _stats(times[True]), _stats(times[False])
    return {"model": "VideoMAE-B 16x224 bf16 r=16 train step", "batch": batch, "native_mlp_backward": on,
            "framework_mlp_backward": off, "native_over_framework_median": round(on["median_us"] / off["median_us"], 3),
            "peak_bytes_native": peak[True], "peak_bytes_framework": peak[False]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    rows = [8 * 1568, 64 * 1568, 64 * 1569]
    if a.quick:
        rows = rows[:1]
    lines, ok = [], True
    for M in rows:
        for fc2_trainable in (True, False):
            res = case(M, fc2_trainable, torch.bfloat16, a.rounds, a.iters)
            ok = ok and res["verdict"] == "tie"
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
