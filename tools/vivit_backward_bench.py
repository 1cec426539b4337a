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
(_PAIR_EXCLUDED), and DESIGN.md section 1 says what the default rests on; exit status 1 when a shape that is routed to
the native Function is not a tie.
`--quick` runs the smallest shape only, `--no-model` leaves the stack out."""
import sys

import torch

import ab
from tome import _abi, _mlp

DEV = ab.DEV


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

    held, warm = ab.held_between(paths, g)
    times = ab.alternate({name: (lambda fwd=fwd: step(fwd)) for name, fwd in paths.items()}, rounds, iters, warm=warm)
    nat, fw = ab.summary(times["native"]), ab.summary(times["framework"])
    out = {"M": M, "C": C, "Hd": Hd, "fc2_trainable": fc2_trainable, "dtype": str(dtype).replace("torch.", ""),
           "routed_to_native": routed, "native_fwd_bwd": nat, "framework_fwd_bwd": fw,
           "larger_spread_us": round(ab.larger_spread(nat, fw), 1),
           "native_over_framework_median": round(nat["median_us"] / fw["median_us"], 3),
           "verdict": ab.tie_within_spread(nat, fw),
           "held_between_fwd_and_bwd_bytes": held, "one_hidden_tensor_bytes": M * Hd * y.element_size()}
    with torch.no_grad():
        h = inter.dense(y)
        ga = torch.randn(M, Hd, device=DEV, generator=gen).to(dtype)
        bwd = lambda: _abi.gelu_tanh_backward(h, ga, want_act=fc2_trainable, want_bias=True, inplace=True)  # noqa: E731
        parts = _abi.lib().tome_gelu_erf_backward_workspace_bytes(M, Hd)
        nbytes = (4 if fc2_trainable else 3) * M * Hd * y.element_size() + parts
        out["backward_launch"] = ab.bandwidth(ab.launch_alone(bwd, rounds, iters), nbytes)
    return out


def model_step(rounds, iters, batch, layers=2):
    """One forward + backward of a `layers`-deep patched bf16 ViViT stack at ViViT-B's width (r = 64, .train()) with the
    switch on and off."""
    import tome
    from hosts import vivit
    seen, peak, launches = [], {}, {}

    def warm(flag, run):  # warm-up, then the peak memory and the native launches of one step
        ab.time_us(run, 1)
        torch.cuda.reset_peak_memory_stats()
        seen.clear()
        ab.time_us(run, 1)
        peak[flag], launches[flag] = torch.cuda.max_memory_allocated(), len(seen)

    orig = _mlp.gelu_backward
    _mlp.gelu_backward = lambda *a: seen.append(1) or orig(*a)
    try:
        times = ab.model_train_step(lambda: vivit.vivit_base(num_hidden_layers=layers), tome.patch.vivit,
                                    (3, 32, 224, 224), batch, 64, (_mlp, "NATIVE_MLP_BACKWARD"), rounds, iters,
                                    warm=warm, dtype=torch.bfloat16)
    finally:
        _mlp.gelu_backward = orig
    on, off = ab.summary(times[True]), ab.summary(times[False])
    return {"model": f"ViViT-B width, {layers} layers, 32x224 bf16 r=64 train step", "batch": batch,
            "native_mlp_backward": on, "framework_mlp_backward": off,
            "larger_spread_us": round(ab.larger_spread(on, off), 1), "verdict": ab.tie_within_spread(on, off),
            "native_over_framework_median": round(on["median_us"] / off["median_us"], 3),
            "native_launches_per_step": launches[True], "launches_per_step_switch_off": launches[False],
            "peak_bytes_native": peak[True], "peak_bytes_framework": peak[False]}


def main():
    ap = ab.parser()
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=4)
    a = ap.parse_args()
    rows = [2 * 3137, 8 * 3137]
    if a.quick:
        rows = rows[:1]
    lines, ok = ab.Lines(a.out), True
    for M in rows:
        for fc2_trainable in (True, False):
            res = case(M, fc2_trainable, torch.bfloat16, a.rounds, a.iters)
            ok = ok and (res["verdict"] == "tie" or not res["routed_to_native"])  # (an excluded shape may lose)
            torch.cuda.empty_cache()
            lines.emit(res)
    if not a.no_model:
        lines.emit(model_step(max(3, a.rounds // 2), 2, a.model_batch))
    lines.write()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
