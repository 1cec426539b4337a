"""Reference and component-wise error bound for tome_trajectory_mix_backward (csrc/tome_traj_bwd.h): the backward of the
temporal stage of Motionformer's trajectory attention -- per (batch, token, head) a softmax over the F <= 8 frames of
(q2 * scale) . k2[f] and the weighted sum of val[f].  No test functions; importable without a GPU (torch only).
tests/test_traj_mix_bwd_oracle_cpu.py shows on the CPU that the bound accepts an fp32 evaluation of the kernel's formula
and rejects the slips such a kernel can make; tests/test_trajectory_mix_backward_gpu.py applies it to the kernel.

Reference: autograd in fp64 of the reference's op sequence (the `else` branch of the temporal stage in
tome/patch/motionformer.py::_trajectory_forward) on the 16-bit inputs, given dout:
    q2 = q2p * scale;  tattn = (k2 * q2.unsqueeze(-2)).sum(-1).softmax(-1);  out = (val * tattn.unsqueeze(-1)).sum(-2)

Bound (derived term by term, after short_attn_bwd_oracle.py; u = 2^-8 bf16 / 2^-11 fp16 for the one rounding of an
output, v = 2^-24 for fp32).  The kernel rounds nothing but its outputs: the inputs are used as stored, a product of two
16-bit values is exact in fp32, so every error below is an fp32 one.  A sum of n fp32 terms in any order is off by at
most (n + 2) v of the sum of the magnitudes.  With p the softmax, dp_f = dout . val[f], delta = sum_f p_f dp_f,
ds_f = p_f (dp_f - delta):

  z      logit f = scale * sum_c q_c k_fc: 64 exact products, fp32 sums, then the product with scale, the subtraction of
         the maximum and the product with log2 e inside __expf, which sit in an exponent:
             E_f = (64 + 2) v scale sum_c |q_c k_fc| + 4 v (|z_f| + max_f |z_f|)               (natural units)
  p      the log-sum-exp moves by at most Ebar = log sum_f p_f exp(E_f), so p~_f = p_f (1 + r) with
             |r| <= rho_f = expm1(E_f + Ebar) + 16 v
         (16 v: the v_exp_f32 results, the 8-term sum, the reciprocal and the product with it).
  dp     64 exact products summed in fp32: |dp~ - dp|_f <= 66 v A_f,  A_f = sum_c |dout_c val_fc|
  delta  8 terms: |delta~ - delta| <= Ed = sum_f p_f (rho_f |dp_f| + (1 + rho_f) 66 v A_f) + 10 v sum_f p_f |dp_f|
  ds     |ds~ - ds|_f <= Eds_f = (1 + rho_f) p_f (rho_f |dp_f - delta| + 66 v A_f + Ed + 3 v (|dp_f| + |delta|))
  dq2    = scale sum_f ds_f k_fc, at most 8 terms and the product with scale:
             |dq2~ - dq2|_c <= scale (sum_f Eds_f |k_fc| + 11 v sum_f |ds_f k_fc|) + u |dq2_c| (1 + 2^-20)
  dk2    = scale ds_f q_c, two products:
             |dk2~ - dk2|_fc <= scale (Eds_f + 3 v |ds_f|) |q_c| + u |dk2_fc| (1 + 2^-20)
  dval   = p_f dout_c:  |dval~ - dval|_fc <= (rho_f + 2 v) p_f |dout_c| + u |dval_fc| (1 + 2^-20)
  fp16   results below 2^-14 are subnormal, spaced 2^-24: a correct rounding is off by up to 2^-25 whatever u says.

The output rounding is the largest term (rho is ~1e-5; the 64-term sums behind dp add 66 v A against a ds of a few
tenths of A / 8), which is what makes a second 16-bit rounding, a missing factor or a neighbour's weight visible.  None of
the constants is fitted to GPU output.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
V32 = 2.0 ** -24
SCALE = 0.125
OUTPUTS = ("dq2", "dk2", "dval")


class Inputs(NamedTuple):
    q2: torch.Tensor     # [B, S, C] 16-bit, C = H * 64
    k2: torch.Tensor     # [B, S, F, C]
    val: torch.Tensor    # [B, S, F, C]
    dout: torch.Tensor   # [B, S, C]
    heads: int
    scale: float


def make_inputs(B, S, F, H, dtype, seed, logit_gain=1.0) -> Inputs:
    """Random tensors on the CPU (the GPU test lays them out).  logit_gain multiplies q2: gain 8 gives logits of +-30,
    rows whose maximum dominates."""
    g = torch.Generator().manual_seed(seed)
    C = H * 64
    q2 = (torch.randn(B, S, C, generator=g) * logit_gain).to(dtype)
    k2 = torch.randn(B, S, F, C, generator=g).to(dtype)
    val = torch.randn(B, S, F, C, generator=g).to(dtype)
    dout = torch.randn(B, S, C, generator=g).to(dtype)
    return Inputs(q2, k2, val, dout, H, SCALE)


def _split(t, H):
    """[..., H*64] -> [..., H, 64]"""
    return t.unflatten(-1, (H, 64))


def reference(inp: Inputs) -> dict:
    """fp64 autograd of the reference's op sequence on the 16-bit inputs + the quantities the bound needs
    (per-head layout: q, g [B, S, H, 64]; k, v [B, S, F, H, 64]; P, z, dP [B, S, H, F])."""
    H = inp.heads
    q2p = inp.q2.detach().cpu().double().requires_grad_(True)
    k2t = inp.k2.detach().cpu().double().requires_grad_(True)
    vt = inp.val.detach().cpu().double().requires_grad_(True)
    B, S, F, C = k2t.shape
    q2 = q2p.view(B, S, H, 64).permute(0, 2, 1, 3) * inp.scale                 # b h s d
    k2 = k2t.view(B, S, F, H, 64).permute(0, 3, 1, 2, 4)                       # b h s f d
    val = vt.view(B, S, F, H, 64).permute(0, 3, 1, 2, 4)
    tattn = (k2 * q2.unsqueeze(-2)).sum(dim=-1).softmax(dim=-1)
    out = (val * tattn.unsqueeze(-1)).sum(dim=-2).permute(0, 2, 1, 3).reshape(B, S, C)
    dq2, dk2, dval = torch.autograd.grad(out, (q2p, k2t, vt), inp.dout.detach().cpu().double())
    with torch.no_grad():
        q, g = _split(q2p.detach(), H), _split(inp.dout.detach().cpu().double(), H)
        k, v = _split(k2t.detach(), H), _split(vt.detach(), H)
        z = inp.scale * torch.einsum("bshd,bsfhd->bshf", q, k)
        return dict(dq2=dq2, dk2=dk2, dval=dval, q=q, g=g, k=k, v=v, z=z, P=tattn.detach().permute(0, 2, 1, 3),
                    scale=inp.scale)


def bounds(ref: dict, dtype) -> dict:
    """Component-wise bounds (see the top of this file) for dq2 [B, S, C], dk2 and dval [B, S, F, C]."""
    u, s = U[dtype], ref["scale"]
    q, g, k, v, z, P = (ref[n] for n in ("q", "g", "k", "v", "z", "P"))
    E = 66 * V32 * s * torch.einsum("bshd,bsfhd->bshf", q.abs(), k.abs()) \
        + 4 * V32 * (z.abs() + z.abs().amax(-1, keepdim=True))
    Ebar = (P * E.exp()).sum(-1, keepdim=True).log()
    rho = torch.expm1(E + Ebar) + 16 * V32
    dP = torch.einsum("bshd,bsfhd->bshf", g, v)
    A = torch.einsum("bshd,bsfhd->bshf", g.abs(), v.abs())
    delta = (P * dP).sum(-1, keepdim=True)
    Ed = (P * (rho * dP.abs() + (1 + rho) * 66 * V32 * A)).sum(-1, keepdim=True) \
        + 10 * V32 * (P * dP.abs()).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    EdS = (1 + rho) * P * (rho * (dP - delta).abs() + 66 * V32 * A + Ed + 3 * V32 * (dP.abs() + delta.abs()))
    tiny = 2.0 ** -25 if dtype == torch.float16 else 0.0
    r16 = u * (1 + 2.0 ** -20)
    bq = s * (torch.einsum("bshf,bsfhd->bshd", EdS, k.abs())
              + 11 * V32 * torch.einsum("bshf,bsfhd->bshd", dS.abs(), k.abs())).flatten(-2) \
        + r16 * ref["dq2"].abs() + tiny
    bk = s * torch.einsum("bshf,bshd->bsfhd", EdS + 3 * V32 * dS.abs(), q.abs()).flatten(-2) \
        + r16 * ref["dk2"].abs() + tiny
    bv = torch.einsum("bshf,bshd->bsfhd", (rho + 2 * V32) * P, g.abs()).flatten(-2) + r16 * ref["dval"].abs() + tiny
    return dict(dq2=bq, dk2=bk, dval=bv)


def outside(got: dict, ref: dict, dtype) -> dict:
    """Per output given: (number of elements outside the bound or non-finite, worst err / bound)."""
    bnd = bounds(ref, dtype)
    res = {}
    for n in OUTPUTS:
        if got.get(n) is None:
            continue
        t = got[n].detach().cpu().double()
        assert t.shape == ref[n].shape, (n, t.shape, ref[n].shape)
        err = (t - ref[n]).abs()
        bad = ~torch.isfinite(t) | (err > bnd[n])
        res[n] = (int(bad.sum()), float((err / bnd[n].clamp_min(1e-300)).nan_to_num(posinf=1e30).max()))
    return res


def check(label, got: dict, ref: dict, dtype) -> dict:
    """Assert the bound on every element of the outputs given; prints each worst err / bound first."""
    res = outside(got, ref, dtype)
    print(f"traj_mix_bwd_oracle {label}: " + " ".join(f"{n} worst err/bound {res[n][1]:.3f}" for n in res))
    assert not any(res[n][0] for n in res), (label, res)
    return {n: res[n][1] for n in res}


SLIPS = ("no_delta", "no_scale_dk2", "neighbour_head_weights", "last_frame_twice", "dval_rounded_twice")


def emulate_fp32(inp: Inputs, slip: Optional[str] = None) -> dict:
    """The kernel's formula in fp32 on the CPU (sums by torch, i.e. in another order than the kernel's), one rounding to
    the 16-bit dtype.  slip: None or one of SLIPS, the wrong answers the CPU tests must see rejected."""
    dtype, H = inp.q2.dtype, inp.heads
    q, g = _split(inp.q2.float(), H), _split(inp.dout.float(), H)
    k, v = _split(inp.k2.float(), H), _split(inp.val.float(), H)
    F = k.shape[2]
    if slip == "last_frame_twice":  # the kernel's loads past the last frame repeat it: one frame too many, not masked
        k = torch.cat((k, k[:, :, -1:]), 2)
        v = torch.cat((v, v[:, :, -1:]), 2)
    sc = torch.tensor(inp.scale, dtype=torch.float32)
    z = torch.einsum("bshd,bsfhd->bshf", q, k) * sc
    e = torch.exp(z - z.amax(-1, keepdim=True))
    P = e * (1.0 / e.sum(-1, keepdim=True))
    dP = torch.einsum("bshd,bsfhd->bshf", g, v)
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - (0.0 if slip == "no_delta" else delta))
    dq2 = torch.einsum("bshf,bsfhd->bshd", dS * sc, k)
    dk2 = torch.einsum("bshf,bshd->bsfhd", dS if slip == "no_scale_dk2" else dS * sc, q)
    Pv = P.roll(1, dims=2) if slip == "neighbour_head_weights" else P
    if slip == "dval_rounded_twice":
        Pv = Pv.to(dtype).float()
    dval = torch.einsum("bshf,bshd->bsfhd", Pv, g)
    return dict(dq2=dq2.flatten(-2).to(dtype), dk2=dk2[:, :, :F].flatten(-2).to(dtype),
                dval=dval[:, :, :F].flatten(-2).to(dtype))
