#!/usr/bin/env python3
"""The residual add + merge + LayerNorm of a patched block under torch.autocast with fp32 master weights (how the
reference benchmarks and trains: tome/utils.py:54, tools/train_net.py:123): ONE launch (tome_merge_wavg_ln_amp) against the
three steps of the route before it -- the framework's `x + residual`, tome_merge_wavg on the sum, tome_add_layernorm_amp
without an addend.  One process, alternated rounds (7 of 50 calls by default; a third of that for the models), device
events, medians with min-max.

Op level, C = 768, bf16 autocast, r = 16, batch 8 and batch 64:
    1568 rows per clip, 16-bit stream with a 16-bit residual (VideoMAE: `pos_embed.type_as(x)`)
    3137 rows per clip, fp32 stream with a 16-bit residual (ViViT: `x + self.pos_embed` has promoted the stream)
with the achieved TB/s of the new launch over its own algorithmic bytes (x and the residual read once, x_out and y_out
written once, the sizes in and out).
Model level: the no-grad forward of VideoMAE-B and ViViT at batch 8 as tome.utils.benchmark(use_fp16=True) runs it (a
half clip under torch.autocast's default dtype), with tome.patch._common.AUTOCAST_FUSED_LN on and off, r = 16.

One JSON line per case; `native_slower_beyond_spread` says whether the new launch's median is above the three steps' by
more than the larger of the two min-max spreads (ab.tie_within_spread).  The exit status is always 0: this tool reports,
it does not judge.  `--out` (default profiles/r10_autocast_merge_ln_bench.jsonl) also receives the lines.  `--quick`: op
level only."""
import os
import sys

import torch

import ab
from tome import _abi
from tome import merge as tm
from tome.patch import _common as C

DEV = ab.DEV
HALF = torch.bfloat16
R = 16


def report(times):
    a, b = ab.summary(times[True]), ab.summary(times[False])
    return {"native": a, "three_steps": b, "speedup_median": round(b["median_us"] / a["median_us"], 3),
            "native_slower_beyond_spread": ab.tie_within_spread(a, b) != "tie"}


def op_case(n, T, stream, rounds, iters, width=768):
    gen = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(n, T, width, device=DEV, generator=gen).to(stream)
    res = torch.randn(n, T, width, device=DEV, generator=gen).to(HALF)
    size = torch.ones(n, T, 1, device=DEV, dtype=stream)
    norm = torch.nn.LayerNorm(width).to(DEV)  # fp32 master weights
    metric = torch.randn(n, T, 64, device=DEV, generator=gen).to(HALF)
    merge, _ = tm.bipartite_soft_matching(metric, R)
    plan = merge.plan
    w, b = norm.weight.detach(), norm.bias.detach()

    def fused():
        return _abi.merge_wavg_ln_amp(plan, x, size, w, b, norm.eps, HALF, addend=res, log_size=True)

    def three_steps():
        s = x + res
        xo, so = _abi.merge_wavg(plan, s, size, log_size=True)
        return xo, _abi.add_layernorm_amp(xo, None, w, b, norm.eps, HALF)[1], so

    with torch.no_grad():
        a, c = fused(), three_steps()
        assert torch.equal(a[0], c[0]) and torch.equal(a[2], c[2]), "the two routes store different streams"
        with torch.autocast("cuda", dtype=HALF):
            assert tm._ln_route(merge, x, norm, res, size) == "amp_direct"
        times = ab.alternate({True: fused, False: three_steps}, rounds, iters, warm=2)
    To, sx = T - plan.r, x.element_size()
    nbytes = n * width * (T * (sx + 2) + To * (sx + 2)) + n * (T + 2 * To) * size.element_size()
    out = {"level": "op", "n": n, "rows_per_clip": T, "C": width, "r": plan.r, "autocast": "bfloat16",
           "stream": str(stream).replace("torch.", ""), "residual": "bfloat16"}
    out.update(report(times))
    out["native_launch"] = ab.bandwidth(times[True], nbytes)
    return out


def _models():
    import tome
    from hosts import videomae, vivit
    return (("videomae_b", lambda: videomae.VideoMAE(), (3, 16, 224, 224), tome.patch.videomae),
            ("vivit_b", lambda: vivit.ViViT(), (3, 32, 224, 224), tome.patch.vivit))


def model_case(name, make, clip_shape, patch, rounds, iters, batch):
    torch.manual_seed(0)
    model = make().to(DEV).eval()
    patch(model, prop_attn=True)
    clip = torch.rand(batch, *clip_shape, device=DEV).half()
    launches = []
    real = _abi.merge_wavg_ln_amp

    def counted(*a, **kw):
        launches.append(1)
        return real(*a, **kw)

    def forward():
        model.r = R
        with torch.autocast("cuda"), torch.no_grad():
            return model([clip])

    _abi.merge_wavg_ln_amp = counted
    try:
        C.AUTOCAST_FUSED_LN = True
        forward()
        per_forward = len(launches)
    finally:
        _abi.merge_wavg_ln_amp = real
        C.AUTOCAST_FUSED_LN = False
    times = ab.alternate(ab.switch_arms(C, "AUTOCAST_FUSED_LN"), rounds, iters, fn=forward, warm=2)
    out = {"level": "model", "model": name, "batch": batch, "mode": "eval no_grad", "r": R,
           "autocast": str(torch.get_autocast_dtype("cuda")).replace("torch.", ""), "fused_launches_per_forward": per_forward}
    out.update(report(times))
    return out


def main():
    ap = ab.parser(iters=50, out=os.path.join(ab.ROOT, "profiles", "r10_autocast_merge_ln_bench.jsonl"))
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    lines = ab.Lines(a.out)
    for n in (8, 64):
        lines.emit(op_case(n, 1568, HALF, a.rounds, a.iters))
        lines.emit(op_case(n, 3137, torch.float32, a.rounds, a.iters))
        torch.cuda.empty_cache()
    if not a.quick:
        for name, make, clip_shape, patch in _models():
            torch.cuda.empty_cache()
            lines.emit(model_case(name, make, clip_shape, patch, a.rounds, max(1, a.iters // 3), a.batch))
    lines.write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
