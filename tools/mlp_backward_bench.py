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
min-max spreads, "native slower" otherwise -- what DESIGN.md section 1 says about the default rests on it; exit status 1
when an op-level case is not a tie.
`--quick` runs the smallest shape only, `--no-model` leaves the model step out."""
import sys

import torch

import ab
from tome import _abi, _mlp

DEV = ab.DEV


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

    held, warm = ab.held_between(paths, g)
    times = ab.alternate({name: (lambda fwd=fwd: step(fwd)) for name, fwd in paths.items()}, rounds, iters, warm=warm)
    nat, fw = ab.summary(times["native"]), ab.summary(times["framework"])
    out = {"M": M, "C": C, "Hd": Hd, "fc2_trainable": fc2_trainable, "dtype": str(dtype).replace("torch.", ""),
           "native_fwd_bwd": nat, "framework_fwd_bwd": fw, "larger_spread_us": round(ab.larger_spread(nat, fw), 1),
           "native_over_framework_median": round(nat["median_us"] / fw["median_us"], 3),
           "verdict": ab.tie_within_spread(nat, fw),
           "held_between_fwd_and_bwd_bytes": held, "one_hidden_tensor_bytes": M * Hd * y.element_size()}
    with torch.no_grad():
        h = mlp.fc1(y)
        ga = torch.randn(M, Hd, device=DEV, generator=gen).to(dtype)
        bwd = lambda: _abi.gelu_erf_backward(h, ga, want_act=fc2_trainable, want_bias=True, inplace=True)  # noqa: E731
        parts = _abi.lib().tome_gelu_erf_backward_workspace_bytes(M, Hd)
        nbytes = (4 if fc2_trainable else 3) * M * Hd * y.element_size() + parts
        out["backward_launch"] = ab.bandwidth(ab.launch_alone(bwd, rounds, iters), nbytes)
    return out


def model_step(rounds, iters, batch):
    """One forward + backward of the patched bf16 VideoMAE-B host (r = 16, .train()) with the switch on and off."""
    import tome
    from hosts import videomae
    peak = {}

    def warm(flag, run):  # warm-up, then the peak memory of one step
        ab.time_us(run, 1)
        torch.cuda.reset_peak_memory_stats()
        ab.time_us(run, 1)
        peak[flag] = torch.cuda.max_memory_allocated()

    times = ab.model_train_step(videomae.VideoMAE, tome.patch.videomae, (3, 16, 224, 224), batch, 16,
                                (_mlp, "NATIVE_MLP_BACKWARD"), rounds, iters, warm=warm, dtype=torch.bfloat16)
    on, off = ab.summary(times[True]), ab.summary(times[False])
    return {"model": "VideoMAE-B 16x224 bf16 r=16 train step", "batch": batch, "native_mlp_backward": on,
            "framework_mlp_backward": off, "native_over_framework_median": round(on["median_us"] / off["median_us"], 3),
            "peak_bytes_native": peak[True], "peak_bytes_framework": peak[False]}


def main():
    ap = ab.parser()
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=16)
    a = ap.parse_args()
    rows = [8 * 1568, 64 * 1568, 64 * 1569]
    if a.quick:
        rows = rows[:1]
    lines, ok = ab.Lines(a.out), True
    for M in rows:
        for fc2_trainable in (True, False):
            res = case(M, fc2_trainable, torch.bfloat16, a.rounds, a.iters)
            ok = ok and res["verdict"] == "tie"
            torch.cuda.empty_cache()
            lines.emit(res)
    if not a.no_model:
        lines.emit(model_step(max(3, a.rounds // 2), 2, a.model_batch))
    lines.write()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
