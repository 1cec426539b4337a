"""Reference and component-wise error bound for tome_short_attention_backward (csrc/tome_short_attn_bwd.h): the
backward of softmax(q k^T * scale) v over sequences of N <= 8 tokens, head dim 64.  No test functions; importable
without a GPU (torch only).  tests/test_short_attn_bwd_oracle_cpu.py shows on the CPU that the bound accepts an fp32
evaluation of the kernel's formula and rejects the slips such a kernel can make; tests/test_short_attention_backward_gpu.py
applies it to the kernel.

Reference: autograd in fp64 of attn = (q * scale) @ k^T; softmax; @ v on the 16-bit inputs (exact in fp64), given dout.

Bound (derived term by term; u = 2^-8 bf16 / 2^-11 fp16 for the one rounding of an output, v = 2^-24 for fp32).  The
kernel rounds nothing but its outputs: the inputs are used as stored, products of two 16-bit values are exact in fp32,
so every error below is an fp32 one.  A sum of n fp32 terms in any order is off by at most (n + 2) v of the sum of the
magnitudes (n - 1 additions and a little room for the conversions around it).  With P the softmax, dP = dO V^T,
delta = rowsum(P o dP), dS = P o (dP - delta):

  z      logit (i, j) = scale * sum_c q_ic k_jc: 64 exact products, fp32 sums, then the products with scale * log2 e and
         the subtraction of the row maximum, which sit in an exponent:
             E_ij = (64 + 2) v scale sum_c |q_ic k_jc| + 4 v (|z_ij| + max_j |z_ij|)          (natural units)
  P      the row's log-sum-exp moves by at most Ebar_i = log sum_j P_ij exp(E_ij), so P~_ij = P_ij (1 + r) with
             |r| <= rho_ij = expm1(E_ij + Ebar_i) + 16 v
         (16 v: two v_exp_f32 results, the 8-term row sum, the reciprocal and the product with it).
  dP     64 exact products summed in fp32: |dP~ - dP|_ij <= 66 v A_ij,  A_ij = sum_c |dO_ic v_jc|
  delta  8 terms: |delta~ - delta|_i <= Ed_i = sum_j P_ij (rho_ij |dP_ij| + (1 + rho_ij) 66 v A_ij) + 10 v sum_j P_ij |dP_ij|
  dS     |dS~ - dS|_ij <= EdS_ij = (1 + rho_ij) P_ij (rho_ij |dP_ij - delta_i| + 66 v A_ij + Ed_i + 3 v (|dP_ij| + |delta_i|))
  dq     = scale sum_j dS_ij k_jc, at most 8 terms and the product with scale:
             |dq~ - dq| <= scale (sum_j EdS_ij |k_jc| + 11 v sum_j |dS_ij k_jc|) + u |dq| (1 + 2^-20)
  dk     the same over the query rows i with q in k's place.
  dv     = sum_i P_ij dO_ic:  |dv~ - dv| <= sum_i P_ij rho_ij |dO_ic| + 10 v sum_i P_ij |dO_ic| + u |dv| (1 + 2^-20)
  fp16   results below 2^-14 are subnormal, spaced 2^-24: a correct rounding is off by up to 2^-25 whatever u says.

The output rounding dominates (rho is ~1e-5): the bound is within a few per cent of u |reference|, element by element,
which is what makes a second 16-bit rounding anywhere inside visible.  None of the constants is fitted to GPU output.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

LOG2E = 1.4426950408889634
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
V32 = 2.0 ** -24
SCALE = 0.125


class Inputs(NamedTuple):
    q: torch.Tensor          # [B, H, N, 64] 16-bit (a slice of `qkv` in the "qkv" layout)
    k: torch.Tensor
    v: torch.Tensor
    dout: torch.Tensor       # [B, N, H*64] 16-bit
    scale: float
    qkv: Optional[torch.Tensor]  # the [B, N, 3, H, 64] buffer of the "qkv" layout, else None


def make_inputs(B, H, N, dtype, seed, layout="qkv", logit_gain=1.0, device="cpu") -> Inputs:
    """Random heads.  layout "qkv": the three slices of one [B, N, 3, H, 64] buffer; "separate": three tensors.
    logit_gain multiplies q (gain 8: rows whose maximum matters, logits of +-30)."""
    g = torch.Generator().manual_seed(seed)
    if layout == "qkv":
        buf = torch.randn(B, N, 3, H, 64, generator=g)
        buf[:, :, 0] *= logit_gain
        qkv = buf.to(dtype).to(device)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    else:
        qkv = None
        q, k, v = ((torch.randn(B, N, H, 64, generator=g) * (logit_gain if i == 0 else 1.0)).to(dtype).to(device)
                   .permute(0, 2, 1, 3) for i in range(3))
    dout = torch.randn(B, N, H * 64, generator=g).to(dtype).to(device)
    return Inputs(q, k, v, dout, SCALE, qkv)


def _heads(dout, B, H, N):
    return dout.detach().cpu().reshape(B, N, H, 64).permute(0, 2, 1, 3)


def reference(inp: Inputs) -> dict:
    """fp64 autograd on the 16-bit inputs + the quantities the bound needs."""
    q = inp.q.detach().cpu().double().requires_grad_(True)
    k = inp.k.detach().cpu().double().requires_grad_(True)
    v = inp.v.detach().cpu().double().requires_grad_(True)
    B, H, N, _ = q.shape
    g = _heads(inp.dout, B, H, N).double()
    z = (q * inp.scale) @ k.transpose(-2, -1)
    P = z.softmax(-1)
    dq, dk, dv = torch.autograd.grad(P @ v, (q, k, v), g)
    return dict(dq=dq, dk=dk, dv=dv, P=P.detach(), z=z.detach(), q=q.detach(), k=k.detach(), v=v.detach(), g=g,
                scale=inp.scale)


def bounds(ref: dict, dtype) -> dict:
    """Component-wise bounds (see the top of this file) for dq, dk, dv [B, H, N, 64]."""
    u, s = U[dtype], ref["scale"]
    q, k, v, g, P, z = (ref[n] for n in ("q", "k", "v", "g", "P", "z"))
    E = 66 * V32 * s * (q.abs() @ k.abs().transpose(-2, -1)) + 4 * V32 * (z.abs() + z.abs().amax(-1, keepdim=True))
    Ebar = (P * E.exp()).sum(-1, keepdim=True).log()
    rho = torch.expm1(E + Ebar) + 16 * V32
    dP = g @ v.transpose(-2, -1)
    A = g.abs() @ v.abs().transpose(-2, -1)
    delta = (P * dP).sum(-1, keepdim=True)
    Ed = (P * (rho * dP.abs() + (1 + rho) * 66 * V32 * A)).sum(-1, keepdim=True) \
        + 10 * V32 * (P * dP.abs()).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    EdS = (1 + rho) * P * (rho * (dP - delta).abs() + 66 * V32 * A + Ed + 3 * V32 * (dP.abs() + delta.abs()))
    tiny = 2.0 ** -25 if dtype == torch.float16 else 0.0
    r16 = u * (1 + 2.0 ** -20)
    bq = s * (EdS @ k.abs() + 11 * V32 * (dS.abs() @ k.abs())) + r16 * ref["dq"].abs() + tiny
    bk = s * (EdS.transpose(-2, -1) @ q.abs() + 11 * V32 * (dS.abs().transpose(-2, -1) @ q.abs())) \
        + r16 * ref["dk"].abs() + tiny
    bv = (P * rho).transpose(-2, -1) @ g.abs() + 10 * V32 * (P.transpose(-2, -1) @ g.abs()) + r16 * ref["dv"].abs() + tiny
    return dict(dq=bq, dk=bk, dv=bv)


def outside(got: dict, ref: dict, dtype) -> dict:
    """Per output: (number of elements outside the bound or non-finite, worst err / bound)."""
    bnd = bounds(ref, dtype)
    res = {}
    for n in ("dq", "dk", "dv"):
        t = got[n].detach().cpu().double()
        err = (t - ref[n]).abs()
        bad = ~torch.isfinite(t) | (err > bnd[n])
        res[n] = (int(bad.sum()), float((err / bnd[n].clamp_min(1e-300)).nan_to_num(posinf=1e30).max()))
    return res


def check(label, got: dict, ref: dict, dtype):
    """Assert the bound on every element of dq, dk, dv; prints each worst err / bound first."""
    res = outside(got, ref, dtype)
    print(f"short_attn_bwd_oracle {label}: " + " ".join(f"{n} worst err/bound {res[n][1]:.3f}" for n in res))
    assert not any(res[n][0] for n in res), (label, res)


SLIPS = ("no_delta", "no_scale", "masked_keys_counted", "query_row_dropped", "heads_swapped", "p_rounded_twice",
         "dout_with_q_strides")


def emulate_fp32(inp: Inputs, slip: Optional[str] = None) -> dict:
    """The kernel's formula in fp32 on the CPU (sums by torch, i.e. in another order than the kernel's), one rounding to
    the 16-bit dtype.  slip: None or one of SLIPS, the wrong answers the CPU tests must see rejected."""
    dtype = inp.q.dtype
    q, k, v = (t.detach().cpu().float() for t in (inp.q, inp.k, inp.v))
    B, H, N, _ = q.shape
    g = _heads(inp.dout, B, H, N).float()
    if slip == "heads_swapped":
        g = g.flip(1)
    if slip == "dout_with_q_strides":  # dout's buffer walked with the strides of q inside a [B, N, 3, H, 64] buffer
        flat = inp.dout.detach().cpu().float().reshape(-1)
        b, h, i, c = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(N), torch.arange(64), indexing="ij")
        g = flat[(b * N * 3 * H * 64 + i * 3 * H * 64 + h * 64 + c) % flat.numel()]
    if slip == "masked_keys_counted":  # the kernel's loads past the last token repeat it: eight keys, none masked
        pad = 8 - N
        k = torch.cat((k, k[:, :, -1:].expand(B, H, pad, 64)), 2)
        v = torch.cat((v, v[:, :, -1:].expand(B, H, pad, 64)), 2)
    z = (q @ k.transpose(-2, -1)) * torch.tensor(inp.scale * LOG2E, dtype=torch.float32)
    e = torch.exp2(z - z.amax(-1, keepdim=True))
    P = e * (1.0 / e.sum(-1, keepdim=True))
    if slip == "p_rounded_twice":
        P = P.to(dtype).float()
    dP = g @ v.transpose(-2, -1)
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - (0.0 if slip == "no_delta" else delta))
    Pk, dSk = P, dS
    if slip == "query_row_dropped":  # the last query row never reaches the dk / dv accumulators
        Pk, dSk = P.clone(), dS.clone()
        Pk[:, :, -1] = 0.0
        dSk[:, :, -1] = 0.0
    sc = 1.0 if slip == "no_scale" else inp.scale
    dq = (dS @ k) * sc
    dk = (dSk.transpose(-2, -1) @ q) * sc
    dv = Pk.transpose(-2, -1) @ g
    if slip == "masked_keys_counted":
        dk, dv = dk[:, :, :N], dv[:, :, :N]
    return dict(dq=dq.to(dtype), dk=dk.to(dtype), dv=dv.to(dtype))
