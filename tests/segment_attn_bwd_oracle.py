"""Reference and component-wise error bound for tome_prop_attention_segments_backward (csrc/tome_attn_bwd.h, SEG form).
No test functions; CPU-importable (torch only).

Reference: the gradient of the reference's op sequence for the per-frame stage of the trajectory attention (the `else`
branch of tome/patch/motionformer.py::_trajectory_forward) -- q_dot_k = q @ k^T, viewed 'q (f n)', times scale, plus the
flat log(size) bias, softmax over the n keys of each frame f, einsum('b q f n, b f n d -> b q f d') with v -- evaluated
in fp64 on the 16-bit inputs by autograd on the CPU.  `size` gets no gradient.

Bound: the construction of attn_bwd_oracle.py, segment by segment.  Segment s is a plain proportional attention of the
N queries over its P keys with the gradient dO_s = dy[:, :, s], so dk_s and dv_s have exactly the roundings counted there
(one u per 16-bit rounding on a term's path -- q~, the P operand, the stored O, the dS operand, the output -- absolute
values pushed through the same sums, (n + 8) 2^-24 per fp32 sum of n terms) and take attn_bwd_oracle.bounds unchanged.
dq differs in one place: the kernel keeps the dQ accumulator across the segments and rounds once, so

    |dq~ - dq| <= sum_s T_s  +  (nseg + 8) 2^-24 sum_s |dq_s|_abs  +  u |dq|  (+ 2^-25 in fp16)

where T_s is segment s's bound WITHOUT its output rounding (attn_bwd_oracle's e_dq minus u |dq_s| and the subnormal
term: the errors of the operands and of the fp32 sum over the segment's keys), |dq_s|_abs = scale |dS_s| |K_s| the
absolute-value sum behind the partial result (the fp32 accumulator carries the partial sums of earlier segments while it
adds the next one's terms), and u |dq| the single rounding of the stored sum.

What the bound cannot see, and what holds it instead.  A kernel that rounded every partial dq_s before adding it would be
off by up to (u / 2) sum_s |dq_s|.  No term above allows for that, yet a worst-case bound of this construction can never
reject it: the dS operand alone is allowed u scale sum_j |dS_ij k_jc| per segment, which is at least u |dq_s| whatever
the inputs are.  That property is therefore held by a case in which every rounding the kernels make is exact
(`exact_inputs`): q = 0, two keys per segment (P = 1/2), values, keys and gradients chosen so that dS, every product
and every partial sum are short binary numbers.  Four segments contribute (1 + 2^-k) / 4 each and three contribute -1/4
with 2^-k a quarter of the format's spacing at 1: the exact dq, (1 + 2^-(k-2)) / 4, is a number of the format, so a
kernel that sums in fp32 and rounds once returns it bit for bit, and one that rounds per segment returns 1/4, one unit
in the last place away.  test_segment_attn_bwd_oracle_cpu.py shows both on the emulation, the GPU test holds the kernel
to the first.

None of the constants is fitted to GPU output.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

import attn_bwd_oracle as ao

LOG2E = ao.LOG2E
U = ao.U
V32 = ao.V32


class Inputs(NamedTuple):
    q: torch.Tensor          # [B, H, N, 64] 16-bit
    k: torch.Tensor          # [B, H, nseg*P, 64]: rows [s*P, (s+1)*P) are segment s
    v: torch.Tensor
    dy: torch.Tensor         # [B, N, nseg, H*64] 16-bit
    log_bias: Optional[torch.Tensor]  # fp32 [B, nseg*P] or None
    nseg: int
    scale: float
    qkv: Optional[torch.Tensor]       # "qkv" layout: the [B, 1 + N, 3, H, 64] buffer (N == nseg*P), class token in row 0


def make_inputs(B, H, N, P, nseg, dtype, seed, bias=True, layout="separate", logit_gain=1.0, max_size=8,
                offset=0.0, device="cpu") -> Inputs:
    """Random heads.  layout "qkv": q = rows 1.. of slice 0 and k / v = rows 1.. of slices 1 / 2 of one
    [B, 1 + N, 3, H, 64] buffer (needs N == nseg*P, Motionformer's case); "separate": three tensors, any N.
    logit_gain multiplies q (gain 8 with sizes up to 64: rows whose maximum matters); offset: a common mean of v and
    dy / 2 (delta large against dP - delta)."""
    g = torch.Generator().manual_seed(seed)
    K = nseg * P
    if layout == "qkv":
        assert N == K
        buf = torch.randn(B, 1 + N, 3, H, 64, generator=g)
        buf[:, :, 0] *= logit_gain
        buf[:, :, 2] += offset
        qkv = buf.to(dtype).to(device)
        q, k, v = (qkv[:, 1:, i].permute(0, 2, 1, 3) for i in range(3))
    else:
        qkv = None
        q = (torch.randn(B, N, H, 64, generator=g) * logit_gain).to(dtype).to(device).permute(0, 2, 1, 3)
        k = torch.randn(B, K, H, 64, generator=g).to(dtype).to(device).permute(0, 2, 1, 3)
        v = (torch.randn(B, K, H, 64, generator=g) + offset).to(dtype).to(device).permute(0, 2, 1, 3)
    dy = (torch.randn(B, N, nseg, H * 64, generator=g) + offset / 2).to(dtype).to(device)
    log_bias = None
    if bias:
        log_bias = torch.randint(1, max_size + 1, (B, K), generator=g).float().log().to(device)
    return Inputs(q, k, v, dy, log_bias, nseg, 0.125, qkv)


def exact_inputs(dtype, device="cpu") -> Inputs:
    """The case in which every rounding is exact (see the top of this file): B = H = 1, three queries, seven segments of
    two keys.  dq of every element is (1 + 4 eps) / 4 with eps a quarter of the format's spacing at 1, dk = 0."""
    eps = U[dtype] / 2
    nseg, N = 7, 3
    q = torch.zeros(1, 1, N, 64)
    k = torch.zeros(1, 1, nseg, 2, 64)
    v = torch.zeros(1, 1, nseg, 2, 64)
    dy = torch.zeros(1, N, nseg, 64)
    k[..., 0, :] = 1.0                      # k_1 - k_2 = 1 + eps in the first four segments, 1 in the other three
    k[:, :, :4, 1, :] = -eps
    v[..., 0, 0], v[..., 1, 0] = 1.0, -1.0  # dP = +-4 c_s, O = 0, delta = 0, dS = +-2 c_s
    dy[:, :, :4, 0], dy[:, :, 4:, 0] = 4.0, -4.0
    to = lambda t: t.to(dtype).to(device)  # noqa: E731
    return Inputs(to(q), to(k.flatten(2, 3)), to(v.flatten(2, 3)), to(dy), None, nseg, 0.125, None)


def segment(inp: Inputs, s: int, bias_from: Optional[int] = None) -> ao.Inputs:
    """Segment s as a plain attention problem of attn_bwd_oracle (CPU tensors)."""
    P = inp.k.shape[2] // inp.nseg
    sl = slice(s * P, (s + 1) * P)
    b = s if bias_from is None else bias_from
    lb = None if inp.log_bias is None else inp.log_bias.cpu()[:, b * P:(b + 1) * P]
    return ao.Inputs(inp.q.cpu(), inp.k.cpu()[:, :, sl], inp.v.cpu()[:, :, sl], inp.dy.cpu()[:, :, s], lb, False,
                     inp.scale, None)


def reference(inp: Inputs) -> dict:
    """fp64 autograd of the reference's op sequence on the 16-bit inputs, and every segment's attn_bwd_oracle
    reference (the quantities the bound needs)."""
    q = inp.q.detach().cpu().double().requires_grad_(True)
    k = inp.k.detach().cpu().double().requires_grad_(True)
    v = inp.v.detach().cpu().double().requires_grad_(True)
    B, H, N, D = q.shape
    F = inp.nseg
    P = k.shape[2] // F
    q_dot_k = (q @ k.transpose(-2, -1)).view(B, H, N, F, P) * inp.scale
    if inp.log_bias is not None:
        q_dot_k = q_dot_k + inp.log_bias.cpu().double().view(B, 1, 1, F, P)
    attn = q_dot_k.softmax(dim=-1)
    y = torch.einsum("b h q f n, b h f n d -> b h q f d", attn, v.view(B, H, F, P, D))
    g = inp.dy.detach().cpu().double().view(B, N, F, H, D).permute(0, 3, 1, 2, 4)
    dq, dk, dv = torch.autograd.grad(y, (q, k, v), g)
    return dict(dq=dq, dk=dk, dv=dv, segs=[ao.reference(segment(inp, s)) for s in range(F)])


def bounds(ref: dict, dtype) -> dict:
    """Component-wise bounds (see the top of this file): dq [B, H, N, 64], dk and dv [B, H, nseg*P, 64]."""
    u = U[dtype]
    sub = 2.0 ** -25 if dtype == torch.float16 else 0.0
    nseg = len(ref["segs"])
    e_dq = u * ref["dq"].abs() + sub
    e_dk, e_dv = [], []
    for r in ref["segs"]:
        b = ao.bounds(r, dtype)
        e_dk.append(b["dk"])
        e_dv.append(b["dv"])
        P, dP = r["P"], r["g"] @ r["v"].transpose(-2, -1)
        delta = (r["g"] * r["out"]).sum(-1, keepdim=True)
        abs_sum = r["scale"] * ((P * (dP - delta)).abs() @ r["k"].abs())
        e_dq = e_dq + (b["dq"] - u * r["dq"].abs() - sub) + (nseg + 8) * V32 * abs_sum
    return dict(dq=e_dq, dk=torch.cat(e_dk, dim=2), dv=torch.cat(e_dv, dim=2))


worst = ao.worst
check = ao.check


# ---- torch-CPU emulation of the kernels' arithmetic ---------------------------------------------------------------

SLIPS = ("dq_segment0_only", "dq_rounded_per_segment", "bias_of_next_segment", "last_partial_tile_dropped",
         "dkv_segments_exchanged", "delta_omitted")


def _r16(x, dtype):
    return x.to(dtype).double()


def emulate(inp: Inputs, slip: Optional[str] = None) -> dict:
    """The kernels' arithmetic with fp64 in place of fp32: q~, P and dS as operands, the stored O and the outputs are
    rounded to the format; dq is summed over the segments unrounded and rounded once.  slip: one of SLIPS, the wrong
    answers the bound has to reject (test_segment_attn_bwd_oracle_cpu.py)."""
    dt = inp.q.dtype
    F = inp.nseg
    q = inp.q.cpu()
    B, H, N, D = q.shape
    sl = torch.tensor(inp.scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    qt = (q.float() * sl).to(dt).double()
    dq = torch.zeros(B, H, N, D, dtype=torch.float64)
    dks, dvs = [], []
    for s in range(F):
        seg = segment(inp, s, bias_from=(s + 1) % F if slip == "bias_of_next_segment" else None)
        k, v = seg.k.double(), seg.v.double()
        P_ = k.shape[2]
        g = seg.dout.double().view(B, N, H, D).permute(0, 2, 1, 3)
        beta = ao.bias_matrix(seg.log_bias, False, N, P_) * LOG2E
        z = qt @ k.transpose(-2, -1) + beta
        keep = torch.ones(N, P_)
        if slip == "last_partial_tile_dropped" and P_ % 64:
            keep[:, P_ - P_ % 64:] = 0           # (P < 64: the only tile is the partial one -- nothing left)
        m = z.amax(-1, keepdim=True)
        L = m + torch.log2((torch.exp2(z - m)).sum(-1, keepdim=True))
        Pm = torch.exp2(z - L)
        o16 = _r16(_r16(Pm, dt) @ v, dt)          # the forward's stored output: every key counted
        Pm = Pm * keep
        delta = (g * o16).sum(-1, keepdim=True)
        if slip == "delta_omitted":
            delta = torch.zeros_like(delta)
        dS16 = _r16(Pm * (g @ v.transpose(-2, -1) - delta), dt)
        dvs.append(_r16(_r16(Pm, dt).transpose(-2, -1) @ g, dt))
        dks.append(_r16(inp.scale * (dS16.transpose(-2, -1) @ q.double()), dt))
        part = inp.scale * (dS16 @ k)
        if slip == "dq_rounded_per_segment":
            part = _r16(part, dt)
        if slip != "dq_segment0_only" or s == 0:
            dq = dq + part
    if slip == "dkv_segments_exchanged" and F >= 2:
        dks[0], dks[1] = dks[1], dks[0]
        dvs[0], dvs[1] = dvs[1], dvs[0]
    return dict(dq=_r16(dq, dt), dk=torch.cat(dks, dim=2), dv=torch.cat(dvs, dim=2))
