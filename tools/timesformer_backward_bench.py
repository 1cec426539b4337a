#!/usr/bin/env python3
"""The two stages of TimeSformer's divided space-time block that tome_short_attention_backward and
tome_layernorm_backward_regrouped put on the kernels under grad, native against the framework branch.  One process,
alternated rounds, device events, medians with min-max, one JSON line per case:
  1. the temporal attention (hosts/timesformer.py::Attention, T = 8, H = 12, bf16) forward + backward at
     B * P = 8 x 196, 64 x 196 and 64 x 180 sequences, and the backward launch alone as bytes over time (7 streams of
     B P x 8 x 768 16-bit values);
  2. the regrouped add + LayerNorm (tome/_ln.py::add_layernorm_regrouped_native against the reference's op sequence of
     tome/patch/timesformer.py) at B = 8 and 64, F = 8, P = 196 and 180, C = 768, parameters trainable and frozen, and
     the backward launch alone (gy, xs, gx_in in, gx out, plus the fp32 partial rows);
  3. (once) one training step of the patched bf16 TimeSformer-B 8 x 224 host, r = 16, batch 8, with each new switch on
     and off.
`verdict` (the rule of tools/mlp_backward_bench.py): "tie" when the native median is not above the framework's by more
than the larger of the two paths' own min-max spreads, "native slower" otherwise.  A shape that loses has to be excluded
in the matching `_abi.*_trainable` predicate; if it is the TimeSformer-B shape itself the switch's default goes to off.
`--quick` runs the smallest shape only, `--no-model` leaves the model step out."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-how-do-your-tokens-merge_amd"))

from tome import _abi, _attn, _ln  # noqa: E402

DEV = "cuda:0"
PEAK_TBS = 8.0
BF = torch.bfloat16


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


def _compare(times, what):
    nat, fw = _stats(times[True]), _stats(times[False])
    spread = max(nat["max_us"] - nat["min_us"], fw["max_us"] - fw["min_us"])
    return {"native_" + what: nat, "framework_" + what: fw, "larger_spread_us": round(spread, 1),
            "native_over_framework_median": round(nat["median_us"] / fw["median_us"], 3),
            "verdict": "tie" if nat["median_us"] <= fw["median_us"] + spread else "native slower"}


def _alternate(step, switch, rounds, iters):
    mod, attr = switch
    times = {True: [], False: []}
    for flag in (True, False):
        setattr(mod, attr, flag)
        step()
    for _ in range(rounds):
        for flag in (True, False):
            setattr(mod, attr, flag)
            times[flag].append(_time(step, iters))
    setattr(mod, attr, True)
    return times


def attention_case(seqs, rounds, iters, T=8, H=12):
    from hosts import timesformer
    C = H * 64
    torch.manual_seed(0)
    att = timesformer.Attention(C, num_heads=H, qkv_bias=True).to(DEV).to(BF).train()
    gen = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(seqs, T, C, device=DEV, generator=gen).to(BF).requires_grad_(True)
    g = torch.randn(seqs, T, C, device=DEV, generator=gen).to(BF)

    def step():
        x.grad = None
        att.zero_grad(set_to_none=True)
        att(x).backward(g)

    out = {"stage": "temporal attention", "sequences": seqs, "T": T, "H": H, "dtype": "bfloat16"}
    out.update(_compare(_alternate(step, (_attn, "NATIVE_SHORT_ATTN_BACKWARD"), rounds, iters), "fwd_bwd"))
    with torch.no_grad():
        qkv = torch.randn(seqs, T, 3, H, 64, device=DEV, generator=gen).to(BF)
        q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
        grads = tuple(torch.empty_like(qkv).permute(2, 0, 3, 1, 4).unbind(0))
        bwd = lambda: _abi.short_attention_backward(q, k, v, g, att.scale, grads=grads)  # noqa: E731
        bwd()
        launch = [_time(bwd, iters) for _ in range(rounds)]
        nbytes = 7 * seqs * T * C * 2
        med = statistics.median(launch)
        out["backward_launch"] = dict(_stats(launch), bytes=nbytes, TBps=round(nbytes / med / 1e6, 2),
                                      share_of_8TBps=round(nbytes / med / 1e6 / PEAK_TBS, 3))
    return out


def _reference_ops(x, rt, T, norm):
    """The branch tome/patch/timesformer.py::_block_forward keeps under grad with the switch off."""
    B, N, m = x.shape
    P = (N - 1) // T
    cls0 = x[:, :1, :]
    xt = x[:, 1:, :] + rt
    x1 = torch.cat((cls0, xt), 1)
    xs_in = torch.cat((cls0.expand(B, T, m).reshape(B * T, 1, m),
                       xt.reshape(B, P, T, m).transpose(1, 2).reshape(B * T, P, m)), 1)
    return x1, norm(xs_in)


def layernorm_case(B, P, trainable, rounds, iters, F=8, C=768):
    torch.manual_seed(0)
    norm = torch.nn.LayerNorm(C, eps=1e-6).to(DEV).to(BF)
    norm.weight.requires_grad_(trainable)
    norm.bias.requires_grad_(trainable)
    gen = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(B, 1 + P * F, C, device=DEV, generator=gen).to(BF).requires_grad_(True)
    rt = torch.randn(B, P * F, C, device=DEV, generator=gen).to(BF).requires_grad_(True)
    g1 = torch.randn(B, 1 + P * F, C, device=DEV, generator=gen).to(BF)
    gy = torch.randn(B * F, 1 + P, C, device=DEV, generator=gen).to(BF)

    def step():
        x.grad = rt.grad = None
        norm.zero_grad(set_to_none=True)
        if _ln.regrouped_enabled():
            outs = _ln.add_layernorm_regrouped_native(x, rt, F, norm)
        else:
            outs = _reference_ops(x, rt, F, norm)
        torch.autograd.backward(outs, (g1, gy))

    out = {"stage": "regrouped add + LayerNorm", "B": B, "F": F, "P": P, "C": C, "trainable": trainable,
           "dtype": "bfloat16"}
    out.update(_compare(_alternate(step, (_ln, "NATIVE_LN_REGROUPED_BACKWARD"), rounds, iters), "fwd_bwd"))
    with torch.no_grad():
        xs = x.detach()
        bwd = lambda: _abi.layernorm_backward_regrouped(gy, xs, g1, F, norm.weight, norm.eps,  # noqa: E731
                                                        want_weight=trainable, want_bias=trainable)
        bwd()
        launch = [_time(bwd, iters) for _ in range(rounds)]
        parts = _abi.lib().tome_layernorm_backward_regrouped_workspace_bytes(B, F, P, C) if trainable else 0
        nbytes = (3 * xs.numel() + gy.numel()) * 2 + parts
        med = statistics.median(launch)
        out["backward_launch"] = dict(_stats(launch), bytes=nbytes, TBps=round(nbytes / med / 1e6, 2),
                                      share_of_8TBps=round(nbytes / med / 1e6 / PEAK_TBS, 3))
    return out


def model_step(switch, rounds, iters, batch):
    """One forward + backward of the patched bf16 TimeSformer-B host (8 x 224, r = 16, .train()), one switch on / off."""
    import tome
    from hosts import timesformer
    torch.manual_seed(0)
    model = timesformer.timesformer_base(num_frames=8).to(DEV).to(BF).train()
    tome.patch.timesformer(model)
    model.r = 16
    clip = torch.rand(batch, 3, 8, 224, 224, device=DEV).to(BF)

    def step():
        model.zero_grad(set_to_none=True)
        model([clip]).float().square().sum().backward()

    out = {"model": "TimeSformer-B 8x224 bf16 r=16 train step", "batch": batch, "switch": switch[1]}
    out.update(_compare(_alternate(step, switch, rounds, iters), "step"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    shapes = [(8, 196), (64, 196), (64, 180)]
    if a.quick:
        shapes = shapes[:1]
    lines, ok = [], True

    def emit(res):
        nonlocal ok
        ok = ok and res["verdict"] == "tie"
        torch.cuda.empty_cache()
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)

    for B, P in shapes:
        emit(attention_case(B * P, a.rounds, a.iters))
    for B, P in shapes:
        for trainable in (True, False):
            emit(layernorm_case(B, P, trainable, a.rounds, a.iters))
    if not a.no_model:
        for switch in ((_attn, "NATIVE_SHORT_ATTN_BACKWARD"), (_ln, "NATIVE_LN_REGROUPED_BACKWARD")):
            emit(model_step(switch, max(3, a.rounds // 2), 2, a.model_batch))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
