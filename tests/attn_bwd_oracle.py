"""Reference and component-wise error bound for tome_prop_attention_backward (csrc/tome_attn_bwd.h).

Reference: the gradient of the reference's op sequence (tome/patch/videomae.py:55-66; timesformer.py:66-78 for the
skip form) -- attn = (q * scale) @ k^T + log(size); softmax; @ v -- evaluated in fp64 on the 16-bit inputs, by autograd
on the CPU.  `size` gets no gradient.

Bound: every element of dq, dk and dv has its own bound, obtained by pushing absolute values through the same sums the
kernels form and counting the 16-bit roundings on each term's path (u = 2^-8 bf16, 2^-11 fp16).  With P the softmax,
dP = dO V^T, delta = rowsum(dO o O), dS = P o (dP - delta):

  q~     the kernels' logits come from q~ = round16(q * scale * log2 e): logit (i, j) moves by at most
         E_ij = u * scale * sum_c |q_ic k_jc| (natural units), the row's log-sum-exp by at most
         Ebar_i = log sum_j P_ij exp(E_ij), so P~_ij = P_ij (1 + r), |r| <= rho_ij = expm1(E_ij + Ebar_i) + eta_i.
         eta_i is the fp32 arithmetic behind a weight: the 64-term score sum started at bias - L ((64 + 8) 2^-24 of the
         magnitudes involved, times ln 2 as it sits in an exponent), the Nk-term row sum ((Nk + 8) 2^-24) and two
         v_exp_f32 / one v_log_f32 results (1 ulp each: 4 * 2^-24).                                       [1 rounding]
  P      enters dV = P^T dO as an MFMA operand in the 16-bit format: u per term.                          [1 rounding]
  O      delta is taken against the forward's STORED output: q~ (rho), its own P operand (u) and its output rounding
         (u, of the result) of O = P V, i.e. |O16 - O|_ic <= sum_j P_ij (rho_ij + u) |v_jc| + u |O_ic| (+ fp32 sums),
         then the 64-term fp32 dot product with dO.                                                [counted: rho + 2u]
  dS     = P~ (dP~ - delta~) carries rho on P, the fp32 sum of dP (64 terms) and delta's error, and enters
         dQ = scale dS K and dK = scale dS^T Q as an MFMA operand in the 16-bit format: u per term.      [1 rounding]
  out    one rounding of every output element: u |result| (the fp32 product with `scale` is inside the allowance).
  fp32   a sum of n terms accumulated in fp32 on the matrix pipe: (n + 8) 2^-24 of the sum of absolute values, the
         style of ln_bwd_oracle.py.

fp16 adds absolute terms where the format runs out of range (as test_backward_gpu.py found for the merge backward):
a P or dS operand below 2^-14 is subnormal, spaced 2^-24, so its rounding is off by up to 2^-25 ABSOLUTE (the same for
the stored O, q~ and the outputs), and the forward flushes weights below 2^-24 of its reference point (attn_oracle.py:
at most 2^-24 per key of the output).  bf16 has fp32's range and needs none.

How tight it is: a worst-case bound over signs.  In bf16 the q~ term dominates -- rho = expm1(E + Ebar) takes every
channel's rounding of q~ with the same sign, ~0.04 on unit-variance heads where the roundings really add like a random
walk over 64 channels -- so a correct kernel sits at ~0.01 of the dq / dk bounds and ~0.05-0.1 of dv's (fp16: the same
ratios, u being 8 x smaller on both sides).  What it catches is therefore a structural error (a term, a key tile, a
bias, a factor, a head: test_attn_bwd_oracle_cpu.py; a dropped 64-key tile of a 197-key row is caught in bf16 through dv
at 2.3 x, not through dq / dk at 0.8 / 0.5 x -- attn_bwd_accounting.py closes that gap: on inputs whose softmax is known
(q = 0 or k = 0) E vanishes, rho collapses to eta, and this same bound rejects a single key missing from dq or a single
query missing from dk), not a slip of a per cent in dq or dk alone.  `check` prints the RMS of
error / bound beside the worst element as a figure for that regime; no bound on it is derived here, so none is asserted.

None of the constants is fitted to GPU output.  CPU-importable (torch only).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

LOG2E = 1.4426950408889634
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
V32 = 2.0 ** -24


class Inputs(NamedTuple):
    q: torch.Tensor          # [B, H, N, 64] 16-bit (a slice of `qkv` in the "qkv" layout)
    k: torch.Tensor          # [B, H, Nk, 64]
    v: torch.Tensor
    dout: torch.Tensor       # [B, N, H*64] 16-bit
    log_bias: Optional[torch.Tensor]  # fp32 [B, Nk - skip] or None
    skip: bool
    scale: float
    qkv: Optional[torch.Tensor]       # the [B, N, 3, H, 64] buffer of the "qkv" layout (N == Nk), else None


def make_inputs(B, H, N, Nk, dtype, seed, bias="bias", layout="separate", logit_gain=1.0, max_size=8,
                grad_scale=1.0, offset=0.0, device="cpu") -> Inputs:
    """Random heads.  bias: "none" | "bias" | "skip" (TimeSformer's form: N == Nk, Nk - 1 sizes).  layout: "qkv" (the
    three slices of one [B, N, 3, H, 64] buffer, N == Nk) or "separate".  logit_gain multiplies q (gain 8 with sizes up
    to 64: rows whose maximum matters).  offset: a common mean of v (offset) and of dout (offset / 2): delta = rowsum(dO o O)
    is then large against dP - delta, the regime where an error in delta shows.  Sizes are integers in 1 .. max_size, as
    merging makes them."""
    g = torch.Generator().manual_seed(seed)
    skip = bias == "skip"
    assert not (skip and N != Nk) and not (layout == "qkv" and N != Nk)
    if layout == "qkv":
        buf = torch.randn(B, N, 3, H, 64, generator=g)
        buf[:, :, 0] *= logit_gain
        buf[:, :, 2] += offset
        qkv = buf.to(dtype).to(device)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    else:
        qkv = None
        q = (torch.randn(B, H, N, 64, generator=g) * logit_gain).to(dtype).to(device)
        k = torch.randn(B, H, Nk, 64, generator=g).to(dtype).to(device)
        v = (torch.randn(B, H, Nk, 64, generator=g) + offset).to(dtype).to(device)
    dout = ((torch.randn(B, N, H * 64, generator=g) + offset / 2) * grad_scale).to(dtype).to(device)
    log_bias = None
    if bias != "none":
        size = torch.randint(1, max_size + 1, (B, Nk - int(skip)), generator=g).float()
        log_bias = size.log().to(device)
    return Inputs(q, k, v, dout, log_bias, skip, 0.125, qkv)


def bias_matrix(log_bias, skip, N, Nk, dtype=torch.float64):
    """[B or 1, 1, N, Nk]: the additive bias of every (query, key) pair in natural units."""
    if log_bias is None:
        return torch.zeros(1, 1, N, Nk, dtype=dtype)
    lb = log_bias.to(dtype).cpu()
    beta = torch.zeros(lb.shape[0], 1, N, Nk, dtype=dtype)
    if skip:
        beta[:, :, 1:, 1:] = lb[:, None, None, :]
    else:
        beta[:, :, :, :] = lb[:, None, None, :]
    return beta


def reference(inp: Inputs, beta: Optional[torch.Tensor] = None) -> dict:
    """fp64 autograd of the reference's op sequence on the 16-bit inputs + the absolute-value sums the bound needs."""
    q = inp.q.detach().cpu().double().requires_grad_(True)
    k = inp.k.detach().cpu().double().requires_grad_(True)
    v = inp.v.detach().cpu().double().requires_grad_(True)
    B, H, N, D = q.shape
    Nk = k.shape[2]
    g = inp.dout.detach().cpu().double().view(B, N, H, D).permute(0, 2, 1, 3)   # [B, H, N, 64]
    if beta is None:
        beta = bias_matrix(inp.log_bias, inp.skip, N, Nk)
    attn = (q * inp.scale) @ k.transpose(-2, -1) + beta
    P = attn.softmax(dim=-1)
    out = P @ v
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), g)
    with torch.no_grad():
        P = P.detach()
        qd, kd, vd = q.detach(), k.detach(), v.detach()
        z = attn.detach()
        return dict(dq=dq, dk=dk, dv=dv, P=P, q=qd, k=kd, v=vd, g=g, z=z, out=out.detach(), scale=inp.scale)


def bounds(ref: dict, dtype) -> dict:
    """Component-wise bounds (see the top of this file) for dq [B, H, N, 64], dk and dv [B, H, Nk, 64]."""
    u = U[dtype]
    sub = 2.0 ** -25 if dtype == torch.float16 else 0.0          # absolute: one subnormal rounding
    flush = 2.0 ** -24 if dtype == torch.float16 else 0.0        # absolute per key: the forward's flushed weights
    P, q, k, v, g, z, scale = (ref[n] for n in ("P", "q", "k", "v", "g", "z", "scale"))
    N, Nk = P.shape[-2], P.shape[-1]
    aq, ak, av, ag = q.abs(), k.abs(), v.abs(), g.abs()
    # ---- rho: relative error of a recomputed weight
    E = u * scale * (aq @ ak.transpose(-2, -1)) + sub * math.log(2.0) * ak.sum(-1).unsqueeze(-2)   # natural units
    Ebar = (P * E.exp()).sum(-1, keepdim=True).log()
    lse = torch.logsumexp(z, dim=-1, keepdim=True)
    mag = (scale * (aq @ ak.transpose(-2, -1)) + (z - scale * (q @ k.transpose(-2, -1))).abs()).amax(-1, keepdim=True)
    eta = (64 + 8) * V32 * (mag + lse.abs()) + (Nk + 8) * V32 + 4 * V32
    rho = torch.expm1(E + Ebar) + eta                                                              # [B, H, N, Nk]
    f = lambda n: (n + 8) * V32  # noqa: E731
    # ---- dV = P^T dO
    Pw = P * (rho + u + f(N))
    e_dv = Pw.transpose(-2, -1) @ ag + sub * ag.sum(-2, keepdim=True) + u * ref["dv"].abs() + sub
    # ---- delta from the stored O
    PV = P @ av
    e_out = ((P * (rho + u + f(Nk))) @ av + u * ref["out"].abs() + sub
             + flush * av.sum(-2, keepdim=True))                                                   # |O16 - O|
    e_delta = (ag * e_out).sum(-1, keepdim=True) + f(64) * (ag * (PV + e_out)).sum(-1, keepdim=True)
    # ---- dS
    dP = g @ v.transpose(-2, -1)
    delta = (g * ref["out"]).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    adP = ag @ av.transpose(-2, -1)
    T = P * (1 + rho) * ((rho + u) * (dP - delta).abs() + f(64) * adP + e_delta) + sub             # operand error
    # ---- dQ = scale dS K, dK = scale dS^T Q
    e_dq = scale * ((T + f(Nk) * dS.abs()) @ ak) + u * ref["dq"].abs() + sub
    e_dk = scale * ((T + f(N) * dS.abs()).transpose(-2, -1) @ aq) + u * ref["dk"].abs() + sub
    return dict(dq=e_dq, dk=e_dk, dv=e_dv)


def worst(got: dict, ref: dict, bnd: dict) -> dict:
    """Largest |got - ref| / bound per output, over EVERY element (none exempt); non-finite values count as inf."""
    res = {}
    for n in ("dq", "dk", "dv"):
        x = got[n].detach().cpu().double()
        assert x.shape == ref[n].shape, (n, x.shape, ref[n].shape)
        ratio = (x - ref[n]).abs() / bnd[n]
        ratio = torch.where(torch.isfinite(x), ratio, torch.full_like(ratio, float("inf")))
        res[n] = float(ratio.max())
    return res


def check(label: str, got: dict, ref: dict, bnd: dict) -> dict:
    w = worst(got, ref, bnd)
    rms = {n: float(((got[n].detach().cpu().double() - ref[n]) / bnd[n]).square().mean().sqrt()) for n in w}
    print(f"{label}: worst error / bound  dq {w['dq']:.3f}  dk {w['dk']:.3f}  dv {w['dv']:.3f}"
          f"   (rms  dq {rms['dq']:.4f}  dk {rms['dk']:.4f}  dv {rms['dv']:.4f})")
    for n, r in w.items():
        assert r <= 1.0, f"{label}: {n} is {r:.3f}x its bound somewhere"
    return w


# ---- torch-CPU emulation of the kernels' arithmetic ---------------------------------------------------------------

def _r16(x, dtype):
    return x.to(dtype).double()


def emulate(inp: Inputs, slip: Optional[str] = None) -> dict:
    """The kernels' arithmetic with fp64 in place of fp32: q~, P and dS as operands, the stored O and the outputs are
    rounded to the format.  slip: one of the wrong answers the bound has to reject (test_attn_bwd_oracle_cpu.py)."""
    dt = inp.q.dtype
    q, k, v = inp.q.cpu(), inp.k.cpu(), inp.v.cpu()
    B, H, N, D = q.shape
    Nk = k.shape[2]
    g = inp.dout.cpu().double().view(B, N, H, D).permute(0, 2, 1, 3)
    sl = torch.tensor(inp.scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    qt = (q.float() * sl).to(dt).double()                                     # attn_oracle.kernel_q
    lb = inp.log_bias
    if slip == "bias_ignored":
        lb = None
    beta = bias_matrix(lb, inp.skip, N, Nk) * LOG2E
    if slip == "bias_shifted" and lb is not None:                            # the skip form applied to a plain bias
        beta = torch.zeros_like(beta)
        beta[..., 1:] = (lb.double().cpu() * LOG2E)[:, None, None, :Nk - 1]
    s = qt @ k.double().transpose(-2, -1) + beta                              # log2 units
    if slip == "tile_dropped":                                                # keys 64 .. 127 missing from row 0's sums
        keep = torch.ones(N, Nk)
        keep[0, 64:128] = 0
    else:
        keep = torch.ones(N, Nk)
    m = s.amax(-1, keepdim=True)
    L = m + torch.log2((torch.exp2(s - m) * keep).sum(-1, keepdim=True))
    P = torch.exp2(s - L) * keep
    o16 = _r16(_r16(P, dt) @ v.double(), dt)                                  # the forward's stored output
    delta = (g * o16).sum(-1, keepdim=True)
    if slip == "delta_omitted":
        delta = torch.zeros_like(delta)
    dP = g @ v.double().transpose(-2, -1)
    dS = P * (dP - delta)
    P16, dS16 = _r16(P, dt), _r16(dS, dt)
    if slip == "stale_rows":                                                  # the last partial query tile's rows past
        pad = (-N) % 64                                                       # the end repeat row N-1 and are added
        P16 = torch.cat([P16, P16[..., -1:, :].expand(B, H, pad, Nk)], -2)
        dS16 = torch.cat([dS16, dS16[..., -1:, :].expand(B, H, pad, Nk)], -2)
        gx = torch.cat([g, g[..., -1:, :].expand(B, H, pad, D)], -2)
        qx = torch.cat([q.double(), q.double()[..., -1:, :].expand(B, H, pad, D)], -2)
    else:
        gx, qx = g, q.double()
    dv = P16.transpose(-2, -1) @ gx
    dk = inp.scale * (dS16.transpose(-2, -1) @ qx)
    if slip == "scale_missing":
        dk = dS16.transpose(-2, -1) @ qx
    dq = inp.scale * (dS16[..., :N, :] @ k.double())
    if slip == "heads_exchanged" and H >= 2:
        dk = dk.clone()
        dv = dv.clone()
        dk[:, [0, 1]] = dk[:, [1, 0]]
        dv[:, [0, 1]] = dv[:, [1, 0]]
    return dict(dq=_r16(dq, dt), dk=_r16(dk, dt), dv=_r16(dv, dt))


SLIPS = ("delta_omitted", "bias_ignored", "bias_shifted", "tile_dropped", "stale_rows", "scale_missing",
         "heads_exchanged")
