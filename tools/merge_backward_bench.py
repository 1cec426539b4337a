#!/usr/bin/env python3
"""Forward + backward of merge_wavg on tokens that require grad: the native Functions (inference kernel forward,
k_merge_rows_bwd backward) against the framework's gather / scatter_reduce chain (tome.merge.NATIVE_BACKWARD = False),
in one process, alternated rounds, device events; and the backward launch alone as bytes over time.

Shapes: VideoMAE's [n, 1568, 768] at n = 64 and 384, r = 16, and TimeSformer's regrouped [64, 1 + 196*8, 768], r = 16;
bf16 and fp32; sizes given (random integers 1..4, so every row is scaled: the kernel's slowest case).
Prints one JSON line per case.  `--quick` runs the smallest case only."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-how-do-your-tokens-merge_amd"))

from tome import _abi  # noqa: E402
from tome import merge as M  # noqa: E402
from tome.patch import _common  # noqa: E402

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

    def run(native):
        M.NATIVE_BACKWARD = native
        return _time(step, iters)

    for native in (True, False):  # warm-up of both paths
        run(native)
    times = {True: [], False: []}
    for _ in range(rounds):
        for native in (True, False):
            times[native].append(run(native))
    M.NATIVE_BACKWARD = True
    # the backward launch alone
    with torch.no_grad():
        s_out = (M.merge_wavg(merge, x.detach(), size)[1] if kind == "plain"
                 else _abi.merge_wavg_regrouped(plan, x.detach(), size, F, has_cls=True)[1])
        if kind == "plain":
            bwd = lambda: _abi.merge_backward(plan, g, out_div=s_out, in_mul=size)  # noqa: E731
        else:
            bwd = lambda: _abi.merge_backward_regrouped(plan, g, F, has_cls=True, out_div=s_out, in_mul=size)  # noqa: E731
        bwd()
        launch = [_time(bwd, iters) for _ in range(rounds)]
    e = x.element_size()
    nbytes = (g.numel() + x.numel()) * e + (s_out.numel() + size.numel()) * size.element_size()
    med = statistics.median(launch)
    nat, frm = _stats(times[True]), _stats(times[False])
    return {
        "case": kind, "n": n, "T": T, "frames": F, "C": C, "r": r, "dtype": str(dtype).replace("torch.", ""),
        "native_fwd_bwd": nat, "framework_fwd_bwd": frm,
        "speedup_median": round(frm["median_us"] / nat["median_us"], 2),
        "native_median_below_framework_fastest": nat["median_us"] < frm["min_us"],
        "backward_launch": _stats(launch), "backward_bytes": nbytes,
        "backward_TBps": round(nbytes / med / 1e6, 2), "share_of_8TBps": round(nbytes / med / 1e6 / PEAK_TBS, 3),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    cases = [("plain", 64), ("plain", 384), ("regrouped", 64)]
    if a.quick:
        cases = cases[:1]
    lines = []
    for kind, n in cases:
        for dtype in (torch.bfloat16, torch.float32):
            res = case(kind, n, dtype, a.rounds, a.iters)
            torch.cuda.empty_cache()
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(json.loads(line)["native_median_below_framework_fastest"] for line in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
