#!/usr/bin/env python3
"""The reduction + LayerNorm launch in the modes beside plain merge (drop, hybrid), bf16, no grad.  One process, alternated
rounds, device events, medians with min-max (tools/ab.py).

(a) op level, C = 768, r = 16: the one launch (tome_drop_ln / tome_merge_wavg_ln with the threshold flags, and their
    regrouped forms) against the three steps it replaces -- the framework's `x + residual`, the reduction kernel on its own,
    the framework's layer_norm -- at
        [64, 1568, 768]              the benchmark's VideoMAE tokens
        [8, 1 + 196 * 8, 768]        TimeSformer's, the residual where the spatial attention left it (GroupedResidual: the
                                     three-step arm also pays the strided copy that materialises it)
(b) model level: the no-grad forward of the four full-width hosts at batch 8 (tools/autocast_bench.py's), r = 16, modes
    drop and hybrid, tome.patch._common._FUSE_MODES on and off.  On a tree without that switch both arms run the same code:
    the line says `switch_present: false`, and (a) is left out (the entries do not exist there).

One JSON line per case; `native_slower_beyond_spread` says whether the native median is above the switch-off median by more
than the larger of the two min-max spreads (the project's rule for excluding a shape from a default-on switch).  The exit
status is always 0: this tool reports, it does not judge.  `--out` (default profiles/r08_modes_bench.jsonl) also receives
the lines.  `--quick`: op level only.  `--models-only`: model level only, `--families a,b`: of these hosts."""
import os
import sys

import torch

import ab
from tome import _abi
from tome import merge as tm
from tome.patch import _common

DEV = ab.DEV
HALF = torch.bfloat16
EPS = 1e-6
SWITCH = (_common, "_FUSE_MODES")
SWITCH_PRESENT = hasattr(_common, "_FUSE_MODES")


def report(times):
    a, b = ab.summary(times[True]), ab.summary(times[False])
    return {"native": a, "switch_off": b, "speedup_median": round(b["median_us"] / a["median_us"], 3),
            "native_slower_beyond_spread": ab.tie_within_spread(a, b) != "tie"}


def _matching(mode, n, T, r, gen):
    """(callable with .plan, size or None) of one matching on random keys; hybrid: the threshold is the median score of
    the selected edges, so about half of the destinations lose their own term."""
    metric = torch.randn(n, T, 64, device=DEV, generator=gen)
    if mode == "drop":
        return tm.bipartite_soft_matching_drop(metric, r)
    probe, _ = tm.bipartite_soft_matching_hybrid(metric, r, False, False, "hybrid", 0.0)
    p = probe.plan
    picked = p.node_max.reshape(n, -1).gather(1, p.src_idx.reshape(n, -1)).reshape(-1).float()
    merge, _ = tm.bipartite_soft_matching_hybrid(metric, r, False, False, "hybrid", float(picked.median()))
    return merge


def op_flat(mode, n, T, r, rounds, iters, C=768):
    gen = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(n, T, C, device=DEV, generator=gen).to(HALF)
    a = torch.randn(n, T, C, device=DEV, generator=gen).to(HALF)
    norm = torch.nn.LayerNorm(C, eps=EPS).to(DEV).to(HALF)
    w, b = norm.weight.detach(), norm.bias.detach()
    plan = _matching(mode, n, T, r, gen).plan

    if mode == "drop":
        def native():
            _abi.drop_ln(plan, x, w, b, EPS, addend=a)

        def steps():
            torch.nn.functional.layer_norm(_abi.drop(plan, x + a), (C,), w, b, EPS)
    else:
        def native():
            _abi.merge_wavg_ln(plan, x, None, w, b, EPS, addend=a)

        def steps():
            torch.nn.functional.layer_norm(_abi.merge_wavg(plan, x + a, None)[0], (C,), w, b, EPS)

    with torch.no_grad():
        times = ab.alternate({True: native, False: steps}, rounds, iters, warm=2)
    nbytes = (2 * T + 2 * (T - r)) * n * C * 2  # x and the residual in, x' and y out
    return dict({"level": "op", "layout": "flat", "mode": mode, "shape": [n, T, C], "r": r, "dtype": "bfloat16",
                 "native_bandwidth": ab.bandwidth(times[True], nbytes)}, **report(times))


def op_regrouped(mode, B, F, P, r, rounds, iters, C=768):
    gen = torch.Generator(device=DEV).manual_seed(9)
    x = torch.randn(B, 1 + P * F, C, device=DEV, generator=gen).to(HALF)
    rs = torch.randn(B * F, 1 + P, C, device=DEV, generator=gen).to(HALF)
    cls_new = torch.randn(B, 1, C, device=DEV, generator=gen).to(HALF)
    res = _common.GroupedResidual(rs, cls_new, B, F, P)
    norm = torch.nn.LayerNorm(C, eps=EPS).to(DEV).to(HALF)
    w, b = norm.weight.detach(), norm.bias.detach()
    plan = _matching(mode, B * F, P, r, gen).plan

    if mode == "drop":
        def native():
            _abi.drop_regrouped(plan, x, F, has_cls=True, ln=(w, b, EPS), addend_grouped=rs, cls_addend=cls_new)

        def steps():
            torch.nn.functional.layer_norm(_abi.drop_regrouped(plan, x + res.materialize(), F, has_cls=True), (C,), w, b, EPS)
    else:
        def native():
            _abi.merge_wavg_regrouped(plan, x, None, F, has_cls=True, ln=(w, b, EPS), addend_grouped=rs, cls_addend=cls_new)

        def steps():
            s = _abi.merge_wavg_regrouped(plan, x + res.materialize(), None, F, has_cls=True)[0]
            torch.nn.functional.layer_norm(s, (C,), w, b, EPS)

    with torch.no_grad():
        times = ab.alternate({True: native, False: steps}, rounds, iters, warm=2)
    N, No = 1 + P * F, 1 + (P - r) * F
    nbytes = (2 * N + 2 * No) * B * C * 2
    return dict({"level": "op", "layout": "regrouped", "mode": mode, "shape": [B, N, C], "frames": F, "r": r,
                 "dtype": "bfloat16", "residual": "grouped", "native_bandwidth": ab.bandwidth(times[True], nbytes)},
                **report(times))


def _hosts():
    import tome
    from hosts import motionformer, timesformer, videomae, vivit
    return (("videomae", videomae.VideoMAE, (3, 16, 224, 224), tome.patch.videomae),
            ("timesformer", timesformer.TimeSformer, (3, 8, 224, 224), tome.patch.timesformer),
            ("motionformer", motionformer.Motionformer, (3, 16, 224, 224), tome.patch.motionformer),
            ("vivit", vivit.ViViT, (3, 32, 224, 224), tome.patch.vivit))


def model_case(name, make, clip_shape, patch, mode, rounds, iters, batch, r=16):
    torch.manual_seed(0)
    model = make().to(DEV).to(HALF).eval()
    patch(model, mode=mode, threshold=0.0)
    model.r = r
    clip = torch.rand(batch, *clip_shape, device=DEV).to(HALF)
    info = model._tome_info
    if mode == "hybrid":  # a threshold inside the first layer's edge scores: their median
        seen = []
        orig = _common.bipartite_soft_matching_hybrid

        def spy(*a, **kw):
            got = orig(*a, **kw)
            seen.append(got[0].plan)
            return got

        _common.bipartite_soft_matching_hybrid = spy
        try:
            with torch.no_grad():
                model([clip])
        finally:
            _common.bipartite_soft_matching_hybrid = orig
        p = seen[0]
        picked = p.node_max.reshape(p.n, -1).gather(1, p.src_idx.reshape(p.n, -1)).reshape(-1).float()
        info["threshold"] = float(picked.median())

    def forward():
        with torch.no_grad():
            model([clip])

    if not SWITCH_PRESENT:
        _common._FUSE_MODES = True  # (nobody reads it on such a tree: both arms are the same code)
    try:
        times = ab.alternate(ab.switch_arms(*SWITCH), rounds, iters, fn=forward, warm=2)
    finally:
        if not SWITCH_PRESENT:
            del _common._FUSE_MODES
    return dict({"level": "model", "family": name, "mode": mode, "batch": batch, "r": r, "dtype": "bfloat16",
                 "grad": False, "switch_present": SWITCH_PRESENT, "threshold": info["threshold"]}, **report(times))


def main():
    ap = ab.parser(out=os.path.join(ab.ROOT, "profiles", "r08_modes_bench.jsonl"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--models-only", action="store_true")
    ap.add_argument("--families", default="", help="comma-separated subset of the hosts for the model level")
    a = ap.parse_args()
    lines = ab.Lines(a.out)
    if SWITCH_PRESENT and not a.models_only:
        for mode in ("drop", "hybrid"):
            lines.emit(op_flat(mode, 64, 1568, 16, a.rounds, a.iters))
            torch.cuda.empty_cache()
            lines.emit(op_regrouped(mode, 8, 8, 196, 16, a.rounds, a.iters))
    if not a.quick:
        wanted = [f for f in a.families.split(",") if f]
        for name, make, clip_shape, patch in _hosts():
            if wanted and name not in wanted:
                continue
            for mode in ("drop", "hybrid"):
                torch.cuda.empty_cache()
                lines.emit(model_case(name, make, clip_shape, patch, mode, a.rounds, max(1, a.iters // 2), a.batch))
    lines.write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
