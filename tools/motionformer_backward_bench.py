#!/usr/bin/env python3
"""Training through the patched Motionformer block stack with the native trajectory backward
(tome_prop_attention_segments_backward + tome_trajectory_mix_backward) against the switch off
(tome/_attn.py::NATIVE_TRAJECTORY_BACKWARD = False: the reference's op sequence and autograd, the path before these
entries existed).  One process, alternated rounds, device events, medians with min-max, one JSON line per case:
  1. forward + backward of the block stack (the patched host's `blocks`, r tokens merged per frame and block, bf16,
     .train()) on a [B, 1 + F*P, C] token tensor, and the peak memory of one such step over what is allocated before it:
       reduced    embed 128, 2 heads, F = 8, P = 49,  depth 2, B = 8
       full size  embed 768, 12 heads, F = 8, P = 196, depth 2, B = 2 and 8       (Motionformer-B 224 16x4: 1569 tokens)
  2. the two backward entries alone at the full-size shape, with what they move or compute:
       trajectory mix   bytes over time: k2, val, q2, dout in, dk2, dval, dq2 out = (4 F + 3) B S C 16-bit values
       segments         10 B H N (F P) 64 FLOP over time (five tile products per (query, key) pair, forward's two recomputed
                        twice in the dq sweep: 14 executed, 10 counted as the algorithm's)
  3. (--glue) the framework glue this change leaves alone, at the full-size shape: `diagonal` + proj_q + the keys-only
     `linear`, whose backward sums three [B, S, F, C] gradients of y -- forward + backward time of that piece alone, for a
     later change to weigh.
`verdict` (the rule of tools/mlp_backward_bench.py): "tie" when the native median is not above the switch-off median by
more than the larger of the two paths' own min-max spreads, "native slower" otherwise; exit status 1 when a stack case
is not a tie.  `--quick` runs the reduced stack only."""
import statistics
import sys

import torch

import ab
from tome import _abi, _attn

DEV = ab.DEV
BF = torch.bfloat16
SWITCH = (_attn, "NATIVE_TRAJECTORY_BACKWARD")


def stack_case(label, embed, heads, F, P, depth, B, r, rounds, iters):
    import tome
    from hosts import motionformer
    torch.manual_seed(0)
    side = int(round(P ** 0.5)) * 16
    model = motionformer.Motionformer(img_size=side, patch_size=16, temporal_resolution=F, embed_dim=embed, depth=depth,
                                      num_heads=heads, num_classes=8).to(DEV).to(BF).train()
    tome.patch.motionformer(model, prop_attn=True)
    gen = torch.Generator(device=DEV).manual_seed(7)
    x0 = torch.randn(B, 1 + F * P, embed, device=DEV, generator=gen).to(BF)
    info = model._tome_info

    def step():
        model.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        # what the patched model's forward sets up per call (tome/patch/_common.py::wrap_model_forward)
        info["r"] = [r] * depth
        info["size"] = None
        info["source"] = None
        info.pop("_prenorm", None)
        info.pop("_folded", None)
        for blk in model.blocks:
            x = blk(x, seq_len=P, num_frames=F)
        x.float().square().sum().backward()

    peak = {}

    def warm(flag, run):  # warm-up of every path, then its peak memory
        run()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run()
        torch.cuda.synchronize()
        peak[flag] = torch.cuda.max_memory_allocated() - base

    out = {"stage": "block stack fwd + bwd", "shape": label, "embed": embed, "heads": heads, "F": F, "P": P,
           "depth": depth, "B": B, "r": r, "dtype": "bfloat16"}
    times = ab.alternate(ab.switch_arms(*SWITCH), rounds, iters, fn=step, warm=warm)
    out.update(ab.tie_report(times, "step", other="switch_off"))
    out["native_peak_bytes"], out["switch_off_peak_bytes"] = peak[True], peak[False]
    return out


def entries_case(B, H, F, P, rounds, iters):
    C, S = H * 64, F * P
    gen = torch.Generator(device=DEV).manual_seed(7)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen).to(BF)  # noqa: E731
    out = {"stage": "backward entries alone", "B": B, "H": H, "F": F, "P": P, "dtype": "bfloat16"}
    with torch.no_grad():
        q2, k2, val, g = rnd(B, S, C), rnd(B, S, F, C), rnd(B, S, F, C), rnd(B, S, C)
        mix = lambda: _abi.trajectory_mix_backward(q2, k2, val, g, H, 0.125)  # noqa: E731
        out["trajectory_mix_backward"] = ab.bandwidth(ab.launch_alone(mix, rounds, iters), (4 * F + 3) * B * S * C * 2)
        del k2, val
        qkv = rnd(B, 1 + S, 3, H, 64).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0][:, :, 1:], qkv[1][:, :, 1:], qkv[2][:, :, 1:]
        bias = torch.randint(1, 9, (B, S), device=DEV, generator=gen).float().log()
        y = _abi.prop_attention_segments(q, k, v, F, 0.125, log_bias=bias)
        gy = rnd(*y.shape)
        seg = lambda: _abi.prop_attention_segments_backward(q, k, v, y, gy, F, 0.125, log_bias=bias)  # noqa: E731
        t = ab.launch_alone(seg, rounds, iters)
        flop = 10 * B * H * S * S * 64
        out["segments_backward"] = dict(ab.summary(t), flop=flop, TFLOPs=round(flop / statistics.median(t) / 1e6, 1))
    return out


def glue_case(B, H, F, P, rounds, iters):
    from einops import rearrange
    C, S = H * 64, F * P
    torch.manual_seed(0)
    proj_q = torch.nn.Linear(C, C).to(DEV).to(BF)
    proj_k = torch.nn.Linear(C, C).to(DEV).to(BF)
    gen = torch.Generator(device=DEV).manual_seed(7)
    y0 = torch.randn(B, S, F, C, device=DEV, generator=gen).to(BF)
    gq, gk, gv = (torch.randn(*s, device=DEV, generator=gen).to(BF) for s in ((B, S, C), (B, S, F, C), (B, S, F, C)))

    def step():
        y = y0.clone().requires_grad_(True)
        y_diag = torch.diagonal(rearrange(y, "b (g n) f d -> b g n f d", g=F), dim1=-4, dim2=-2)
        q2 = proj_q(rearrange(y_diag, "b n d f -> b (f n) d", f=F))
        k2 = proj_k(y)
        torch.autograd.backward((q2, k2, y), (gq, gk, gv))  # y itself is the mix's `val`: three gradients of y are summed

    return {"stage": "framework glue fwd + bwd (diagonal, proj_q, keys-only linear)", "B": B, "H": H, "F": F, "P": P,
            "dtype": "bfloat16", **ab.summary(ab.launch_alone(step, rounds, iters))}


def main():
    ap = ab.parser(iters=5)
    ap.add_argument("--glue", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("motionformer_backward_bench: needs the GPU (no CPU path, no fallback)")
    lines, ok = ab.Lines(a.out), True

    def emit(res):
        nonlocal ok
        ok = ok and res.get("verdict", "tie") == "tie"
        torch.cuda.empty_cache()
        lines.emit(res)

    emit(stack_case("reduced", 128, 2, 8, 49, 2, 8, 3, a.rounds, a.iters))
    if not a.quick:
        for B in (2, 8):
            emit(stack_case("full size", 768, 12, 8, 196, 2, B, 16, a.rounds, a.iters))
        emit(entries_case(8, 12, 8, 196, a.rounds, a.iters))
        if a.glue:
            emit(glue_case(8, 12, 8, 196, a.rounds, a.iters))
    lines.write()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
