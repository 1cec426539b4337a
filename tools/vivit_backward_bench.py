#!/usr/bin/env python3
"""ViViT's MLP pair `output.dense(gelu_fast(intermediate.dense(y)))` on tokens that require grad: the native Function of
tome/_mlp.py with the tanh form (library GEMMs, tome_gelu_tanh forward, k_gelu_bwd<.., GELU_TANH> between the backward's
GEMMs) against the path with tome._mlp.NATIVE_MLP_BACKWARD off (the framework's modules and autograd).  One process,
alternated rounds, device events, medians with min-max; one JSON line per figure:
  1. the backward launch alone as bytes over time: (4 with the activation, 3 without) x M x Hd x 2 bytes plus the fp32
     partial rows of the bias gradient;
  2. forward + backward of the pair, native against the switch off, and the bytes held between forward and backward;
  3. (once) a two-layer patched bf16 ViViT stack at full width (768 / 3072, 32 x 224 x 224 clips: 3137 tokens), one
     forward + backward step with the switch on and off: step time and peak memory.
Shapes: C = 768, Hd = 3072, M = 2 x 3137 and 8 x 3137; fc2 trainable and frozen.
`verdict`: "tie" when the native median is not above the other path's by more than the larger of the two paths' own
min-max spreads, "native slower" otherwise -- a shape with that verdict is excluded in tome/_mlp.py pair_trainable
(_PAIR_EXCLUDED), and DESIGN.md section 1 says what the default rests on.
`--quick` runs the smallest shape only, `--no-model` leaves the stack out."""
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


def _verdict(nat, fw):
    spread = max(nat["max_us"] - nat["min_us"], fw["max_us"] - fw["min_us"])
    return round(spread, 1), "tie" if nat["median_us"] <= fw["median_us"] + spread else "native slower"


def case(M, fc2_trainable, dtype, rounds, iters, C=768, Hd=3072):
    from hosts import vivit
    gen = torch.Generator(device=DEV).manual_seed(7)
    torch.manual_seed(0)
    cfg = vivit.VivitConfig(hidden_size=C, intermediate_size=Hd)
    inter = vivit.VivitIntermediate(cfg).to(DEV).to(dtype).train()
    outp = vivit.VivitOutput(cfg).to(DEV).to(dtype).train()
    outp.dense.weight.requires_grad_(fc2_trainable)
    y = torch.randn(M, C, device=DEV, generator=gen).to(dtype).requires_grad_(True)
    g = torch.randn(M, C, device=DEV, generator=gen).to(dtype)

    routed = _mlp.route_pair(inter, outp, y) == "function"  # (False: a shape pair_trainable excludes; measured anyway)

    def native():
        return _mlp._MlpFunction.apply(y, inter.dense.weight, inter.dense.bias, outp.dense.weight, outp.dense.bias, "tanh")

    paths = {"native": native, "framework": lambda: outp.dropout(outp.dense(inter(y)))}

    def step(fwd):
        y.grad = None
        inter.zero_grad(set_to_none=True)
        outp.zero_grad(set_to_none=True)
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
    spread, verdict = _verdict(nat, fw)
    out = {"M": M, "C": C, "Hd": Hd, "fc2_trainable": fc2_trainable, "dtype": str(dtype).replace("torch.", ""),
           "routed_to_native": routed, "native_fwd_bwd": nat, "framework_fwd_bwd": fw, "larger_spread_us": spread,
           "native_over_framework_median": round(nat["median_us"] / fw["median_us"], 3), "verdict": verdict,
           "held_between_fwd_and_bwd_bytes": held, "one_hidden_tensor_bytes": M * Hd * y.element_size()}
    with torch.no_grad():
        h = inter.dense(y)
        ga = torch.randn(M, Hd, device=DEV, generator=gen).to(dtype)
        bwd = lambda: _abi.gelu_tanh_backward(h, ga, want_act=fc2_trainable, want_bias=True, inplace=True)  # noqa: E731
        bwd()
        launch = [_time(bwd, iters) for _ in range(rounds)]
        parts = _abi.lib().tome_gelu_erf_backward_workspace_bytes(M, Hd)
        nbytes = (4 if fc2_trainable else 3) * M * Hd * y.element_size() + parts
        med = statistics.median(launch)
        out["backward_launch"] = dict(_stats(launch), bytes=nbytes, TBps=round(nbytes / med / 1e6, 2),
                                      share_of_8TBps=round(nbytes / med / 1e6 / PEAK_TBS, 3))
    return out


def model_step(rounds, iters, batch, layers=2):
    """One forward + backward of a `layers`-deep patched bf16 ViViT stack at ViViT-B's width (r = 64, .train()) with the
    switch on and off."""
    import tome
    from hosts import vivit
    torch.manual_seed(0)
    model = vivit.vivit_base(num_hidden_layers=layers).to(DEV).to(torch.bfloat16).train()
    tome.patch.vivit(model)
    model.r = 64
    clip = torch.rand(batch, 3, 32, 224, 224, device=DEV).to(torch.bfloat16)
    seen = []
    orig = _mlp.gelu_backward
    _mlp.gelu_backward = lambda *a: seen.append(1) or orig(*a)

    def step():
        model.zero_grad(set_to_none=True)
        model([clip]).float().square().sum().backward()

    times, peak, launches = {True: [], False: []}, {}, {}
    for flag in (True, False):
        _mlp.NATIVE_MLP_BACKWARD = flag
        _time(step, 1)
        torch.cuda.reset_peak_memory_stats()
        seen.clear()
        _time(step, 1)
        peak[flag], launches[flag] = torch.cuda.max_memory_allocated(), len(seen)
    for _ in range(rounds):
        for flag in (True, False):
            _mlp.NATIVE_MLP_BACKWARD = flag
            times[flag].append(_time(step, iters))
    _mlp.NATIVE_MLP_BACKWARD = True
    _mlp.gelu_backward = orig
    on, off = _stats(times[True]), _stats(times[False])
    spread, verdict = _verdict(on, off)
    return {"model": f"ViViT-B width, {layers} layers, 32x224 bf16 r=64 train step", "batch": batch,
            "native_mlp_backward": on, "framework_mlp_backward": off, "larger_spread_us": spread, "verdict": verdict,
            "native_over_framework_median": round(on["median_us"] / off["median_us"], 3),
            "native_launches_per_step": launches[True], "launches_per_step_switch_off": launches[False],
            "peak_bytes_native": peak[True], "peak_bytes_framework": peak[False]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=4)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    rows = [2 * 3137, 8 * 3137]
    if a.quick:
        rows = rows[:1]
    lines, ok = [], True
    for M in rows:
        for fc2_trainable in (True, False):
            res = case(M, fc2_trainable, torch.bfloat16, a.rounds, a.iters)
            ok = ok and (res["verdict"] == "tie" or not res["routed_to_native"])  # (an excluded shape may lose)
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
