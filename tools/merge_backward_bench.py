#!/usr/bin/env python3
"""Forward + backward of merge_wavg on tokens that require grad: the native Functions (inference kernel forward,
k_merge_rows_bwd backward) against the framework's gather / scatter_reduce chain (tome.merge.NATIVE_BACKWARD = False),
in one process, alternated rounds, device events; and the backward launch alone as bytes over time.

Shapes: VideoMAE's [n, 1568, 768] at n = 64 and 384, r = 16, and TimeSformer's regrouped [64, 1 + 196*8, 768], r = 16;
bf16 and fp32; sizes given (random integers 1..4, so every row is scaled: the kernel's slowest case).
Prints one JSON line per case; exit status 1 when a native median is not below the framework's fastest round.
`--quick` runs the smallest case only."""
import statistics
import sys

import torch

import ab
from tome import _abi
from tome import merge as M
from tome.patch import _common

DEV = ab.DEV


def case(kind, n, dtype, rounds, iters, r=16, C=768):
    gen = torch.Generator(device=DEV).manual_seed(7)
    if kind == "plain":
        T, F = 1568, 1
        x = torch.randn(n, T, C, device=DEV, generator=gen).to(dtype).requires_grad_(True)
        metric = torch.randn(n, T, 64, device=DEV, generator=gen)
    else:
        T, F = 196, 8
        x = torch.randn(n, 1 + T * F, C, device=DEV, generator=gen).to(dtype).requires_grad_(True)
        metric = torch.randn(n * F, T, 64, device=DEV, generator=gen)
    groups = n * F
    size = torch.randint(1, 5, (groups, T, 1), device=DEV, generator=gen).to(dtype)
    merge, _ = M.bipartite_soft_matching(metric, r)
    plan = merge.plan
    info = {"size": None}

    def fwd():
        if kind == "plain":
            return M.merge_wavg(merge, x, size)[0]
        if M.NATIVE_BACKWARD:
            return M.merge_wavg_regrouped_native(plan, x, size, F, has_cls=True)[0]
        # the parent commit's training path for the regrouped models: split, '(p t) -> (b t) p', merge, back, cat
        info["size"] = size
        return _common._regrouped_by_views(lambda m, body, i, rr: M.merge_wavg(merge, body, i["size"])[0], None, x, info,
                                           r, F)

    g = torch.randn_like(fwd().detach())

    def step():
        x.grad = None
        fwd().backward(g)

    times = ab.alternate(ab.switch_arms(M, "NATIVE_BACKWARD"), rounds, iters, fn=step, warm=iters)
    # the backward launch alone
    with torch.no_grad():
        s_out = (M.merge_wavg(merge, x.detach(), size)[1] if kind == "plain"
                 else _abi.merge_wavg_regrouped(plan, x.detach(), size, F, has_cls=True)[1])
        if kind == "plain":
            bwd = lambda: _abi.merge_backward(plan, g, out_div=s_out, in_mul=size)  # noqa: E731
        else:
            bwd = lambda: _abi.merge_backward_regrouped(plan, g, F, has_cls=True, out_div=s_out, in_mul=size)  # noqa: E731
        launch = ab.launch_alone(bwd, rounds, iters)
    e = x.element_size()
    nbytes = (g.numel() + x.numel()) * e + (s_out.numel() + size.numel()) * size.element_size()
    med = statistics.median(launch)
    nat, frm = ab.summary(times[True]), ab.summary(times[False])
    return {
        "case": kind, "n": n, "T": T, "frames": F, "C": C, "r": r, "dtype": str(dtype).replace("torch.", ""),
        "native_fwd_bwd": nat, "framework_fwd_bwd": frm,
        "speedup_median": round(frm["median_us"] / nat["median_us"], 2),
        "native_median_below_framework_fastest": ab.median_below_fastest(nat, frm),
        "backward_launch": ab.summary(launch), "backward_bytes": nbytes,
        "backward_TBps": round(nbytes / med / 1e6, 2), "share_of_8TBps": round(nbytes / med / 1e6 / ab.PEAK_TBS, 3),
    }


def main():
    a = ab.parser().parse_args()
    cases = [("plain", 64), ("plain", 384), ("regrouped", 64)]
    if a.quick:
        cases = cases[:1]
    lines, ok = ab.Lines(a.out), True
    for kind, n in cases:
        for dtype in (torch.bfloat16, torch.float32):
            res = case(kind, n, dtype, a.rounds, a.iters)
            ok = ok and res["native_median_below_framework_fastest"]
            torch.cuda.empty_cache()
            lines.emit(res)
    lines.write()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
