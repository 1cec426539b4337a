#!/usr/bin/env python3
"""Training through the residual add + merge + LayerNorm of a patched block under torch.autocast with fp32 master weights
(how the reference trains: tools/train_net.py:123, tome/utils.py:54): tome._ln.NATIVE_MERGE_LN_AUTOCAST_BACKWARD on -- ONE
launch forward (tome_merge_wavg_ln_amp) and ONE backward (tome_merge_ln_backward_amp) -- against the route with the switch
off: the framework's `x + residual`, the merge Function and the tome_add_layernorm_amp Function forward, and going back
tome_layernorm_backward_amp over the merged rows, tome_merge_backward over the token rows and the framework's cast of gx
for a 16-bit residual of an fp32 stream.

The two arms run in ALTERNATING PROCESSES: this script starts a fresh child per arm and round (on, off, on, off, ...; one
at a time), so neither arm inherits the other's allocator state, caches or clocks; every child times every case with
device events after a warm-up, and the parent reports medians with min-max over all of an arm's timings.

Op level, C = 768, bf16 autocast, r = 16, forward + backward of the step, for a 16-bit and an fp32 stream (16-bit residual):
    64 x 1568 rows (VideoMAE-B's tokens at batch 64) and 8 x 3137 rows (ViViT-B's at batch 8)
Model level: one training step (forward, loss, backward) of VideoMAE-B and ViViT-B at batch 8 under bf16 autocast, r = 16.

One JSON line per case; `on_slower_beyond_spread` says whether the switched-on median is above the other by more than the
larger of the two min-max spreads (ab.tie_within_spread).  The exit status is 0 unless a child fails: this tool reports,
it does not judge.  `--out` (default profiles/autocast_merge_ln_backward_bench.jsonl) also receives the lines.  `--quick`:
op level only."""
import json
import os
import subprocess
import sys

import ab

R = 16
OPS = [(64, 1568, "bfloat16"), (64, 1568, "float32"), (8, 3137, "bfloat16"), (8, 3137, "float32")]
MODELS = ("videomae_b", "vivit_b")


# ---------------------------------------------------------------------------------------------------------------------
# child: one arm, every case
# ---------------------------------------------------------------------------------------------------------------------
def op_step(n, T, stream, on, width=768):
    import torch
    from tome import _ln
    from tome import merge as tm
    half = torch.bfloat16
    gen = torch.Generator(device=ab.DEV).manual_seed(7)
    x = torch.randn(n, T, width, device=ab.DEV, generator=gen).to(stream).requires_grad_(True)
    res = torch.randn(n, T, width, device=ab.DEV, generator=gen).to(half).requires_grad_(True)
    size = torch.ones(n, T, 1, device=ab.DEV, dtype=stream)
    norm = torch.nn.LayerNorm(width).to(ab.DEV)  # fp32 master weights
    metric = torch.randn(n, T, 64, device=ab.DEV, generator=gen).to(half)
    merge, _ = tm.bipartite_soft_matching(metric, R)
    g_x = torch.randn(n, T - R, width, device=ab.DEV, generator=gen).to(stream)
    g_y = torch.randn(n, T - R, width, device=ab.DEV, generator=gen).to(half)

    def forward():
        if on:
            xo, y, _ = tm.merge_wavg_ln(merge, x, size, norm, residual=res, log_size=True)
        else:  # the block's three steps (tome/patch/_common.py::merge_then_norm without a fused route)
            xo, _ = tm.merge_wavg(merge, x + res, size, log_size=True)
            y = _ln.add_layernorm(xo, None, norm)[1]
        return xo, y

    def step():
        x.grad = res.grad = None
        norm.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=half):
            xo, y = forward()
        torch.autograd.backward([xo, y], [g_x, g_y])

    with torch.autocast("cuda", dtype=half):
        xo, y = forward()
        fn = type(xo.grad_fn).__name__
        assert (fn == "_MergeLnAmpFunctionBackward") == on, fn
        assert y.dtype == half and type(y.grad_fn).__name__ != "NativeLayerNormBackward0", "the LayerNorm left the kernels"
    return step


def model_step(name):
    import torch
    import tome
    from hosts import videomae, vivit
    make, clip_shape, patch = {"videomae_b": (videomae.VideoMAE, (3, 16, 224, 224), tome.patch.videomae),
                               "vivit_b": (vivit.ViViT, (3, 32, 224, 224), tome.patch.vivit)}[name]
    torch.manual_seed(0)
    model = make().to(ab.DEV).train()
    patch(model, prop_attn=True)
    clip = torch.rand(8, *clip_shape, device=ab.DEV)

    def step():
        model.zero_grad(set_to_none=True)
        model.r = R
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = model([clip])
        out.float().square().sum().backward()

    return step


def child(arm, iters, quick):
    import torch
    from tome import _abi, _ln
    on = arm == "on"
    _ln.NATIVE_MERGE_LN_AUTOCAST_BACKWARD = on
    launches = []
    real = _abi.merge_ln_backward_amp
    _abi.merge_ln_backward_amp = lambda *a, **kw: launches.append(1) or real(*a, **kw)

    def timed(case, step, iters, repeats=3):
        del launches[:]
        step()
        per_step = len(launches)
        us = [ab.time_us(step, iters, warmup=1) for _ in range(repeats)]
        print(json.dumps(dict(case, arm=arm, fused_backward_launches_per_step=per_step, us=us)), flush=True)

    for n, T, stream in OPS:
        timed({"level": "op", "n": n, "rows_per_clip": T, "C": 768, "r": R, "autocast": "bfloat16", "stream": stream,
               "residual": "bfloat16", "what": "forward + backward"}, op_step(n, T, getattr(torch, stream), on), iters)
        torch.cuda.empty_cache()
    if not quick:
        for name in MODELS:
            timed({"level": "model", "model": name, "batch": 8, "mode": "train step", "r": R, "autocast": "bfloat16"},
                  model_step(name), max(1, iters // 5))
            torch.cuda.empty_cache()
    return 0


# ---------------------------------------------------------------------------------------------------------------------
# parent: alternating processes, one at a time
# ---------------------------------------------------------------------------------------------------------------------
def main():
    ap = ab.parser(iters=20, out=os.path.join(ab.ROOT, "profiles", "autocast_merge_ln_backward_bench.jsonl"))
    ap.set_defaults(rounds=3)
    ap.add_argument("--child", choices=["on", "off"], help="(internal) run one arm in this process")
    ap.add_argument("--child-timeout", type=float, default=600.0, help="seconds a child may take")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.iters, a.quick)
    seen, order = {}, []
    for rnd in range(a.rounds):
        for arm in ("on", "off"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", arm, "--iters", str(a.iters)]
            try:
                done = subprocess.run(cmd + (["--quick"] if a.quick else []), stdout=subprocess.PIPE, text=True,
                                      timeout=a.child_timeout)
            except subprocess.TimeoutExpired:
                print(f"the {arm} child of round {rnd} was ended after {a.child_timeout} s", file=sys.stderr)
                return 1
            if done.returncode != 0:  # (nothing more is started behind a child that failed)
                print(f"the {arm} child of round {rnd} ended with status {done.returncode}", file=sys.stderr)
                return 1
            print(f"round {rnd}: the {arm} child is done", file=sys.stderr, flush=True)
            for line in done.stdout.splitlines():
                if not line.startswith("{"):
                    continue
                rec = json.loads(line)
                us, launches = rec.pop("us"), rec.pop("fused_backward_launches_per_step")
                key = json.dumps({k: v for k, v in rec.items() if k != "arm"}, sort_keys=True)
                if key not in seen:
                    seen[key] = {"on": [], "off": [], "launches": {}}
                    order.append(key)
                seen[key][arm] += us
                seen[key]["launches"][arm] = launches
    lines = ab.Lines(a.out)
    for key in order:
        got = seen[key]
        on, off = ab.summary(got["on"]), ab.summary(got["off"])
        out = json.loads(key)
        out.update({"switch_on": on, "switch_off": off, "speedup_median": round(off["median_us"] / on["median_us"], 3),
                    "on_slower_beyond_spread": ab.tie_within_spread(on, off) != "tie",
                    "fused_backward_launches_per_step": got["launches"], "processes_per_arm": a.rounds,
                    "timings_per_arm": len(got["on"])})
        lines.emit(out)
    lines.write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
