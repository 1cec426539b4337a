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
than the larger of the two paths' own min-max spreads, "native slower" otherwise; exit status 1 when a case is not a
tie.  A shape that loses has to be excluded in the matching `_abi.*_trainable` predicate; if it is the TimeSformer-B
shape itself the switch's default goes to off.
`--quick` runs the smallest shape only, `--no-model` leaves the model step out."""
import sys

import torch

import ab
from tome import _abi, _attn, _ln

DEV = ab.DEV
BF = torch.bfloat16
ATTN_SWITCH, LN_SWITCH = (_attn, "NATIVE_SHORT_ATTN_BACKWARD"), (_ln, "NATIVE_LN_REGROUPED_BACKWARD")


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
    out.update(ab.tie_report(ab.alternate(ab.switch_arms(*ATTN_SWITCH), rounds, iters, fn=step), "fwd_bwd"))
    with torch.no_grad():
        qkv = torch.randn(seqs, T, 3, H, 64, device=DEV, generator=gen).to(BF)
        q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
        grads = tuple(torch.empty_like(qkv).permute(2, 0, 3, 1, 4).unbind(0))
        bwd = lambda: _abi.short_attention_backward(q, k, v, g, att.scale, grads=grads)  # noqa: E731
        out["backward_launch"] = ab.bandwidth(ab.launch_alone(bwd, rounds, iters), 7 * seqs * T * C * 2)
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
    out.update(ab.tie_report(ab.alternate(ab.switch_arms(*LN_SWITCH), rounds, iters, fn=step), "fwd_bwd"))
    with torch.no_grad():
        xs = x.detach()
        bwd = lambda: _abi.layernorm_backward_regrouped(gy, xs, g1, F, norm.weight, norm.eps,  # noqa: E731
                                                        want_weight=trainable, want_bias=trainable)
        parts = _abi.lib().tome_layernorm_backward_regrouped_workspace_bytes(B, F, P, C) if trainable else 0
        nbytes = (3 * xs.numel() + gy.numel()) * 2 + parts
        out["backward_launch"] = ab.bandwidth(ab.launch_alone(bwd, rounds, iters), nbytes)
    return out


def model_step(switch, rounds, iters, batch):
    """One forward + backward of the patched bf16 TimeSformer-B host (8 x 224, r = 16, .train()), one switch on / off."""
    import tome
    from hosts import timesformer
    times = ab.model_train_step(lambda: timesformer.timesformer_base(num_frames=8), tome.patch.timesformer,
                                (3, 8, 224, 224), batch, 16, switch, rounds, iters, warm="call", dtype=BF)
    out = {"model": "TimeSformer-B 8x224 bf16 r=16 train step", "batch": batch, "switch": switch[1]}
    out.update(ab.tie_report(times, "step"))
    return out


def main():
    ap = ab.parser()
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=8)
    a = ap.parse_args()
    shapes = [(8, 196), (64, 196), (64, 180)]
    if a.quick:
        shapes = shapes[:1]
    lines, ok = ab.Lines(a.out), True

    def emit(res):
        nonlocal ok
        ok = ok and res["verdict"] == "tie"
        torch.cuda.empty_cache()
        lines.emit(res)

    for B, P in shapes:
        emit(attention_case(B * P, a.rounds, a.iters))
    for B, P in shapes:
        for trainable in (True, False):
            emit(layernorm_case(B, P, trainable, a.rounds, a.iters))
    if not a.no_model:
        for switch in (ATTN_SWITCH, LN_SWITCH):
            emit(model_step(switch, max(3, a.rounds // 2), 2, a.model_batch))
    lines.write()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
