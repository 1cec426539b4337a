"""Reference and component-wise error bound for the two small streaming attention forwards of csrc/tome_attn.h:
k_trajectory_mix (tome_trajectory_mix: per (batch, token, head) a softmax over the F <= 8 frames of (q2 * scale) . k2[f]
and the weighted sum of val[f], with the optional fp32 map tattn) and k_short_attention (tome_short_attention:
softmax(q k^T * scale) v over sequences of N <= 8 tokens).  No test functions; importable without a GPU (torch only).
tests/test_small_attn_fwd_oracle_cpu.py shows on the CPU that the bound accepts an fp32 evaluation of each kernel's
formula and rejects the slips such kernels can make; tests/test_small_attention_forward_gpu.py applies it to the kernels.

Inputs, make_inputs and the fp64 quantities are those of the two backward oracles (traj_mix_bwd_oracle.py,
short_attn_bwd_oracle.py): `reference` takes either kind of Inputs and adds the forward's own results.

Reference: fp64 on the 16-bit inputs (exact in fp64): P = softmax(scale * q . k), out = sum_j P_j v_j.

Bound (derived term by term; u = 2^-8 bf16 / 2^-11 fp16 for the one rounding of out, v = 2^-24 for fp32).  The kernels
round nothing but out: the inputs are used as stored, a product of two 16-bit values is exact in fp32, so every error
in front of that rounding is an fp32 one.  A sum of n fp32 terms in any order is off by at most (n + 2) v of the sum of
the magnitudes.  j runs over the keys of a row (the frames f of a token's trajectory in the mix):

  z      logit j = scale * sum_c q_c k_jc: 64 exact products and fp32 sums.  The mix adds them by fma and three
         xor-shuffle additions (8 + 3 roundings on any path); the short kernel by four v_dot2 per lane and the same
         shuffles -- a v_dot2 adds two exact products to its accumulator with at most two roundings, to nearest or
         towards zero (2 v each at worst): 4 * 2 * 2 + 3 = 19 v at most.  Both are inside the 66 v of a 64-term sum.
         Then, in an exponent: the product with scale (mix) or with the rounded constant scale * log2 e (short: 2 v for
         the constant, v for the product), the subtraction of the row maximum (v |z - m|) and, in the mix, __expf's own
         product with its rounded log2 e (2 v |z - m|).  With |z - m| <= |z| + max |z| each sum is at most
             E_j = 66 v scale sum_c |q_c k_jc| + 4 v (|z_j| + max_j |z_j|)                       (natural units)
  P      the log-sum-exp moves by at most Ebar = log sum_j P_j exp(E_j), so P~_j = P_j (1 + r) with
             |r| <= rho_j = expm1(E_j + Ebar) + 16 v
         (16 v: the v_exp_f32 results of numerator and denominator, 2 v each; the 8-term sum, 7 v; the reciprocal, 2 v;
         the product with it, v -- 14 v).  E, Ebar and rho are exactly those of the backward oracles.
  tattn  the mix stores P~ as it is, fp32:  |p~ - p|_j <= (rho_j + v) p_j.
  out    at most 8 fma steps on P~_j v_jc, then ONE rounding to the 16-bit format:
             |out~ - out|_c <= sum_j (rho_j + 10 v) P_j |v_jc| + u (1 + 2^-20) |out_c|
  fp16   results below 2^-14 are subnormal, spaced 2^-24: a correct rounding is off by up to 2^-25 whatever u says.

With one key (F = 1, N = 1) everything is exact: P~ = exp2(0) / 1 = 1, out~ = fma(1, v, 0) = v.

The output rounding dominates (rho is ~1e-5): the bound is within a few per cent of u |reference|, element by element --
no room for a second rounding, a weight rounded to 16 bits or a stray weight.  None of the constants is fitted to GPU
output.
"""
from __future__ import annotations

from typing import Optional

import torch

import short_attn_bwd_oracle as so
import traj_mix_bwd_oracle as to

LOG2E = so.LOG2E
U = so.U
V32 = so.V32
SCALE = so.SCALE


def _is_traj(inp) -> bool:
    return isinstance(inp, to.Inputs)


def reference(inp) -> dict:
    """fp64 forward on the 16-bit inputs (the backward oracle's own q, k, v, z, P) + the forward's results.
    to.Inputs: out [B, S, C], tattn [B, H, S, F];  so.Inputs: out [B, N, H*64]."""
    if _is_traj(inp):
        r = to.reference(inp)
        q, k, v, z, P = (r[n] for n in ("q", "k", "v", "z", "P"))  # q [B,S,H,64]; k, v [B,S,F,H,64]; z, P [B,S,H,F]
        absqk = torch.einsum("bshd,bsfhd->bshf", q.abs(), k.abs())
        out = torch.einsum("bshf,bsfhd->bshd", P, v).flatten(-2)
        return dict(kind="traj", out=out, tattn=P.permute(0, 2, 1, 3), P=P, z=z, v=v, absqk=absqk, scale=r["scale"])
    r = so.reference(inp)
    q, k, v, z, P = (r[n] for n in ("q", "k", "v", "z", "P"))      # q, k, v [B,H,N,64]; z, P [B,H,N,N]
    absqk = q.abs() @ k.abs().transpose(-2, -1)
    out = (P @ v).transpose(1, 2).flatten(-2)
    return dict(kind="short", out=out, P=P, z=z, v=v, absqk=absqk, scale=r["scale"])


def _rho(ref: dict) -> torch.Tensor:
    """rho of the top of this file (and of the two backward oracles), shaped like P."""
    P, z = ref["P"], ref["z"]
    E = 66 * V32 * ref["scale"] * ref["absqk"] + 4 * V32 * (z.abs() + z.abs().amax(-1, keepdim=True))
    Ebar = (P * E.exp()).sum(-1, keepdim=True).log()
    return torch.expm1(E + Ebar) + 16 * V32


def bounds(ref: dict, dtype) -> dict:
    """Component-wise bounds (see the top of this file) for out (and tattn of the trajectory mix)."""
    rho, P, v = _rho(ref), ref["P"], ref["v"]
    tiny = 2.0 ** -25 if dtype == torch.float16 else 0.0
    r16 = U[dtype] * (1 + 2.0 ** -20)
    w = (rho + 10 * V32) * P
    if ref["kind"] == "traj":
        e32 = torch.einsum("bshf,bsfhd->bshd", w, v.abs()).flatten(-2)
        return dict(out=e32 + r16 * ref["out"].abs() + tiny, tattn=((rho + V32) * P).permute(0, 2, 1, 3))
    e32 = (w @ v.abs()).transpose(1, 2).flatten(-2)
    return dict(out=e32 + r16 * ref["out"].abs() + tiny)


def outside(got: dict, ref: dict, dtype) -> dict:
    """Per output given ("out", "tattn"): (number of elements outside the bound or non-finite, worst err / bound;
    0 where the error is exactly 0)."""
    bnd = bounds(ref, dtype)
    res = {}
    for n in ("out", "tattn"):
        if got.get(n) is None:
            continue
        t = got[n].detach().cpu().double()
        assert t.shape == ref[n].shape, (n, t.shape, ref[n].shape)
        err = (t - ref[n]).abs()
        bad = ~torch.isfinite(t) | (err > bnd[n])
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd[n].clamp_min(1e-300))
        res[n] = (int(bad.sum()), float(ratio.nan_to_num(nan=1e30, posinf=1e30).max()))
    return res


def check(label, got: dict, ref: dict, dtype) -> dict:
    """Assert the bound on every element of the outputs given; prints each worst err / bound first."""
    res = outside(got, ref, dtype)
    print(f"small_attn_fwd_oracle {ref['kind']} {label}: " + " ".join(f"{n} worst err/bound {res[n][1]:.3f}" for n in res))
    assert res and not any(res[n][0] for n in res), (label, res)
    return {n: res[n][1] for n in res}


TRAJ_SLIPS = ("last_frame_twice", "no_scale", "neighbour_head_weights", "second_group_reads_first",
              "val_with_k_row_stride", "p_rounded_twice", "out_rounded_twice", "tattn_frames_of_next_token")
SHORT_SLIPS = ("masked_keys_counted", "no_scale", "heads_swapped", "query_row_dropped", "v_with_k_strides",
               "p_rounded_twice", "out_rounded_twice")


def _elements(t: torch.Tensor) -> torch.Tensor:
    """Every element of the buffer behind the view t, as the kernel's pointer arithmetic sees it."""
    return torch.as_strided(t, (t.untyped_storage().nbytes() // t.element_size(),), (1,), 0)


def emulate_traj_fp32(inp: to.Inputs, slip: Optional[str] = None) -> dict:
    """k_trajectory_mix's formula in fp32 on the CPU (sums by torch, i.e. in another order than the kernel's), one
    rounding of out to the 16-bit dtype; dict(out, tattn).  slip: None or one of TRAJ_SLIPS, the wrong answers the CPU
    tests must see rejected."""
    assert slip is None or slip in TRAJ_SLIPS, slip
    dtype, H = inp.q2.dtype, inp.heads
    q, k, v = to._split(inp.q2.float(), H), to._split(inp.k2.float(), H), to._split(inp.val.float(), H)
    B, S, F = k.shape[:3]
    C = H * 64
    if slip == "val_with_k_row_stride":  # val's rows walked with k2's row stride (wrapping inside val's buffer)
        flat = _elements(inp.val).float()
        row = torch.arange(B * S).view(B, S, 1, 1)
        idx = inp.val.storage_offset() + (row * F + torch.arange(F).view(1, 1, F, 1)) * inp.k2.stride(2) + torch.arange(C)
        v = to._split(flat[idx % flat.numel()], H)
    if slip == "last_frame_twice" and F < 8:  # the loads past the last frame repeat it: one frame too many, not masked
        k = torch.cat((k, k[:, :, -1:]), 2)
        v = torch.cat((v, v[:, :, -1:]), 2)
    sc = torch.tensor(1.0 if slip == "no_scale" else inp.scale, dtype=torch.float32)
    z = torch.einsum("bshd,bsfhd->bshf", q, k) * sc
    e = torch.exp(z - z.amax(-1, keepdim=True))
    inv = 1.0 / e.sum(-1, keepdim=True)
    P = e * inv
    if slip == "p_rounded_twice":  # the weights pass through the 16-bit format on their way to the weighted sum
        P = P.to(dtype).float()
    Pv = P
    if slip == "neighbour_head_weights":
        Pv = P.roll(1, dims=2)
    if slip == "second_group_reads_first":  # chunk group lane + 64 (heads >= 8) takes the weights of lane (head - 8)
        Pv = P.clone()
        Pv[:, :, 8:] = P[:, :, :max(H - 8, 0)]
    if slip == "out_rounded_twice":  # the sum is rounded to 16 bits before it is normalised, the quotient once more
        out = torch.einsum("bshf,bsfhd->bshd", e, v).to(dtype).float() * inv
    else:
        out = torch.einsum("bshf,bsfhd->bshd", Pv, v)
    tattn = P[..., :F].permute(0, 2, 1, 3)
    if slip == "tattn_frames_of_next_token":
        tattn = tattn.roll(-1, dims=2)
    return dict(out=out.flatten(-2).to(dtype), tattn=tattn.contiguous())


def emulate_short_fp32(inp: so.Inputs, slip: Optional[str] = None) -> dict:
    """k_short_attention's formula in fp32 on the CPU (sums by torch), one rounding of out to the 16-bit dtype;
    dict(out).  slip: None or one of SHORT_SLIPS."""
    assert slip is None or slip in SHORT_SLIPS, slip
    dtype = inp.q.dtype
    q, k, v = (t.detach().cpu().float() for t in (inp.q, inp.k, inp.v))
    B, H, N, _ = q.shape
    if slip == "v_with_k_strides":  # v's buffer walked with k's batch / token strides (wrapping inside v's buffer)
        flat = _elements(inp.v).float()
        b, h, n, c = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(N), torch.arange(64), indexing="ij")
        idx = inp.v.storage_offset() + b * inp.k.stride(0) + h * 64 + n * inp.k.stride(2) + c
        v = flat[idx % flat.numel()]
    if slip == "masked_keys_counted":  # the kernel's loads past the last token repeat it: eight keys, none masked
        k = torch.cat((k, k[:, :, -1:].expand(B, H, 8 - N, 64)), 2)
        v = torch.cat((v, v[:, :, -1:].expand(B, H, 8 - N, 64)), 2)
    sl = torch.tensor((1.0 if slip == "no_scale" else inp.scale) * LOG2E, dtype=torch.float32)
    z = (q @ k.transpose(-2, -1)) * sl
    e = torch.exp2(z - z.amax(-1, keepdim=True))
    inv = 1.0 / e.sum(-1, keepdim=True)
    P = e * inv
    if slip == "p_rounded_twice":
        P = P.to(dtype).float()
    if slip == "out_rounded_twice":
        out = (e @ v).to(dtype).float() * inv
    else:
        out = P @ v
    if slip == "heads_swapped":
        out = out.flip(1)
    if slip == "query_row_dropped":  # the last query row is never computed: its output is left as row 0's
        out = out.clone()
        out[:, :, -1] = out[:, :, 0]
    return dict(out=out.transpose(1, 2).flatten(-2).to(dtype))


def emulate_fp32(inp, slip: Optional[str] = None) -> dict:
    """emulate_traj_fp32 or emulate_short_fp32, by the kind of Inputs."""
    return emulate_traj_fp32(inp, slip) if _is_traj(inp) else emulate_short_fp32(inp, slip)
