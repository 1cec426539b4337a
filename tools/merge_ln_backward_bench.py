#!/usr/bin/env python3
"""Forward + backward of `x + residual -> merge_wavg -> LayerNorm` on tokens that require grad: the fused Function
(tome/_ln.py::_MergeLnFunction: tome_merge_wavg_ln forward, tome_merge_ln_backward backward, what
tome.merge.merge_wavg_ln takes) against the three steps of the training path as it stands (`x + residual`,
_MergeWavgFunction, _LayerNormFunction), in one process, alternated rounds, device events; the backward launch alone as
bytes over time (4 x n x T x C x 2 bytes: x', gy and gx_out read at the merged row of every token, gx written;
parameter gradients included); and one forward + backward step of the patched bf16 VideoMAE-B host (batch 8, r = 16)
with tome.patch._common.TRAIN_FUSED_LN on and off -- off is the default and the parent's route.

Shapes: VideoMAE-B's first merging layer, [n, 1568, 768] r = 16 at n = 8 and 64, bf16.  One JSON line per case; exit
status 1 when a fused median is not below the three steps' median.  `--quick` runs the smallest case only, `--no-model`
leaves the model step out."""
import sys

import torch

import ab
from tome import _abi, _ln
from tome import merge as M
from tome.patch import _common

DEV = ab.DEV


def case(n, T, r, dtype, rounds, iters, C=768):
    gen = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(n, T, C, device=DEV, generator=gen).to(dtype).requires_grad_(True)
    res = torch.randn(n, T, C, device=DEV, generator=gen).to(dtype).requires_grad_(True)
    size = torch.randint(1, 4, (n, T, 1), device=DEV, generator=gen).to(dtype)
    norm = torch.nn.LayerNorm(C).to(DEV).to(dtype)
    merge, _ = M.bipartite_soft_matching(torch.randn(n, T, 64, device=DEV, generator=gen).to(dtype), r)
    g_x = torch.randn(n, T - r, C, device=DEV, generator=gen).to(dtype)
    g_y = torch.randn(n, T - r, C, device=DEV, generator=gen).to(dtype)

    def fused():
        return M.merge_wavg_ln(merge, x, size, norm, residual=res)[:2]

    def three_steps():
        xo, _ = M.merge_wavg(merge, x + res, size)
        return xo, _ln.layernorm_native(xo, norm)

    def step(fwd):
        x.grad = res.grad = norm.weight.grad = norm.bias.grad = None
        torch.autograd.backward(fwd(), (g_x, g_y))

    assert type(fused()[0].grad_fn).__name__ == "_MergeLnFunctionBackward"
    assert type(three_steps()[0].grad_fn).__name__ == "_MergeWavgFunctionBackward"
    times = ab.alternate({"fused": lambda: step(fused), "three_steps": lambda: step(three_steps)}, rounds, iters,
                         warm=iters)
    one, three = ab.summary(times["fused"]), ab.summary(times["three_steps"])
    out = {"n": n, "T": T, "r": r, "C": C, "dtype": str(dtype).replace("torch.", ""), "fused_fwd_bwd": one,
           "three_steps_fwd_bwd": three, "speedup_median": round(three["median_us"] / one["median_us"], 2),
           "fused_median_below_three_steps_median": ab.median_below_median(one, three)}
    with torch.no_grad():
        xs, _, s_out = _abi.merge_wavg_ln(merge.plan, x.detach(), size, norm.weight, norm.bias, norm.eps,
                                          addend=res.detach())
        nbytes = 4 * n * T * C * x.element_size()
        for label, params in (("backward_launch", True), ("backward_launch_frozen", False)):
            bwd = lambda: _abi.merge_ln_backward(merge.plan, g_y, g_x, xs, s_out, size, norm.weight, norm.eps,  # noqa: E731
                                                 want_weight=params, want_bias=params)
            out[label] = ab.bandwidth(ab.launch_alone(bwd, rounds, iters), nbytes)
    return out


def model_step(rounds, iters, batch):
    """One forward + backward of the patched bf16 VideoMAE-B host (r = 16, .train()) with the switch on and off."""
    import tome
    from hosts import videomae
    times = ab.model_train_step(videomae.VideoMAE, tome.patch.videomae, (3, 16, 224, 224), batch, 16,
                                (_common, "TRAIN_FUSED_LN"), rounds, iters, warm=1, dtype=torch.bfloat16)
    on, off = ab.summary(times[True]), ab.summary(times[False])
    return {"model": "VideoMAE-B 16x224 bf16 r=16 train step", "batch": batch, "train_fused_ln_on": on,
            "train_fused_ln_off": off, "speedup_median": round(off["median_us"] / on["median_us"], 3)}


def main():
    ap = ab.parser()
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=8)
    a = ap.parse_args()
    cases = [(8, 1568, 16), (64, 1568, 16)]
    if a.quick:
        cases = cases[:1]
    lines, ok = ab.Lines(a.out), True
    for n, T, r in cases:
        res = case(n, T, r, torch.bfloat16, a.rounds, a.iters)
        ok = ok and res["fused_median_below_three_steps_median"]
        torch.cuda.empty_cache()
        lines.emit(res)
    if not a.no_model:
        lines.emit(model_step(max(3, a.rounds // 2), 2, a.model_batch))
    lines.write()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
