"""Accounting for tome_layernorm_backward_regrouped (csrc/tome_ln_bwd.h, k_ln_rows_bwd<.., REGROUP>), the backward of
tome_add_layernorm_regrouped: the row map of TimeSformer's mid-block regrouping in front of tests/ln_bwd_oracle.py.  No
test functions; importable without a GPU.

Reference
---------
xs [B, 1 + P*F, C]: the stored rows the forward normalised; gy [B*F, 1 + P, C]: the gradient of the regrouped,
normalised tensor.  Token row 1 + p*F + t of clip b takes row (b*F + t)(1 + P) + 1 + p of gy; a clip's class row takes
the sum over t of rows (b*F + t)(1 + P), formed in fp64.  The token-layout gradient then goes through
ln_bwd_oracle.reference unchanged (fp64 LayerNorm backward, dweight, dbias, the magnitudes its bounds need).

Bound
-----
ln_bwd_oracle.bound_gx / bound_param, plus what the class rows add.  The kernel forms a class row's gradient as an fp32
sum of F values that are exact in fp32: F - 1 additions, so channel c of that sum is off by at most
    e_c = (F - 1) v S_c,   S_c = sum_t |gy_t,c|,   v = 2^-24.
The LayerNorm backward is linear in gy, so pushing |e| through the formula term by term moves the class row's gx by at
most rstd (|e w| + mean|e w| + |xhat| mean|e w xhat|) = (F - 1) v M(S): ln_bwd_oracle's magnitude M evaluated on S in
gy's place (without gx_in).  The summed row enters dweight and dbias once, so they move by at most
(F - 1) v sum_class |S xhat| and (F - 1) v sum_class S.  Token rows get nothing extra.  F = 1 adds nothing at all.
The number of rows in ln_bwd_oracle's launch form is the number of token-layout rows, B (1 + P F): the kernel walks xs.
"""
import torch

import ln_bwd_oracle as L

V32 = L.V32


def to_token_layout(gy, B, F, P, slip=None, dtype=None):
    """gy [B*F, 1+P, C] (any float dtype) -> [B, 1 + P*F, C] in gy's dtype: the row map, class rows summed in frame
    order in gy's dtype.  slip: "transposed_map" | "cls_frame0" | "cls_rounded_per_frame" (needs `dtype`)."""
    C = gy.shape[-1]
    g = gy.reshape(B, F, 1 + P, C)
    tok = torch.zeros(B, 1 + P * F, C, dtype=gy.dtype)
    acc = g[:, 0, 0].clone()
    for t in range(1, F):
        if slip == "cls_frame0":
            break
        acc = acc + g[:, t, 0]
        if slip == "cls_rounded_per_frame":
            acc = acc.to(dtype).to(gy.dtype)
    tok[:, 0] = acc
    body = g[:, :, 1:]                                    # [B, F, P, C]
    if slip == "transposed_map":
        tok[:, 1:] = body.reshape(B, F * P, C)            # row 1 + t*P + p: frame and patch index the wrong way round
    else:
        tok[:, 1:] = body.permute(0, 2, 1, 3).reshape(B, P * F, C)
    return tok


def reference(gy, xs, gx_in, w, eps, F):
    """fp64 backward through the row map; ln_bwd_oracle.reference's dict plus the class rows' extra allowances."""
    B, N, C = xs.shape
    P = (N - 1) // F
    assert N == 1 + P * F and tuple(gy.shape) == (B * F, 1 + P, C)
    g64 = gy.detach().cpu().double()
    ref = L.reference(to_token_layout(g64, B, F, P), xs, gx_in, w, eps)
    S = torch.zeros(B, N, C, dtype=torch.float64)
    S[:, 0] = g64.reshape(B, F, 1 + P, C)[:, :, 0].abs().sum(1)
    mag = L.reference(S, xs, None, w, eps)
    ref["cls_gx"] = (F - 1) * V32 * mag["M"]
    ref["cls_dw"] = (F - 1) * V32 * mag["Tw"]
    ref["cls_db"] = (F - 1) * V32 * mag["Tb"]
    return ref


def bound_gx(ref, dtype):
    return L.bound_gx(ref, dtype) + ref["cls_gx"]


def bound_param(ref, which, dtype):
    return L.bound_param(ref, which, dtype) + ref["cls_" + which]


def outside_gx(gx, ref, dtype):
    got = gx.detach().cpu().double().reshape(ref["gx"].shape)
    err, bnd = (got - ref["gx"]).abs(), bound_gx(ref, dtype)
    bad = ~torch.isfinite(got) | (err > bnd)
    return bad.any(-1), float((err / bnd.clamp_min(1e-300)).max())


def outside_param(got, ref, which, dtype):
    got = got.detach().cpu().double().reshape(-1)
    err, bnd = (got - ref[which]).abs(), bound_param(ref, which, dtype)
    return ~torch.isfinite(got) | (err > bnd), float((err / bnd.clamp_min(1e-300)).max())


def check(label, gx, dw, db, ref, dtype):
    """Assert the bound on every element of gx and, where given, dweight and dbias; prints each worst err / bound."""
    bad, worst = outside_gx(gx, ref, dtype)
    line = f"ln_regrouped_bwd_oracle {label}: rows {ref['rows']} C {ref['gx'].shape[-1]} gx worst err/bound {worst:.3f}"
    fails = [] if not bool(bad.any()) else [f"gx: {int(bad.sum())} rows outside, first row {int(torch.nonzero(bad)[0])}"]
    for which, got in (("dw", dw), ("db", db)):
        if got is None:
            continue
        badp, worstp = outside_param(got, ref, which, dtype)
        line += f" {which} {worstp:.3f}"
        if bool(badp.any()):
            fails.append(f"{which}: {int(badp.sum())} channels outside, first {int(torch.nonzero(badp)[0])}")
    print(line)
    assert not fails, (label, fails)


def make_inputs(B, F, P, C, dtype, seed, with_in=True, grad_scale=1.0, far=True):
    """(gy [B*F, 1+P, C], xs [B, 1+P*F, C], gx_in or None, w): ln_bwd_oracle.make_inputs' rows, gy in the regrouped
    layout."""
    _, xs, gi, w = L.make_inputs((B, 1 + P * F, C), dtype, seed, far=far, grad_scale=grad_scale, with_in=with_in)
    gen = torch.Generator().manual_seed(seed + 7919)
    gy = (grad_scale * torch.randn(B * F, 1 + P, C, generator=gen, dtype=torch.float64)).to(dtype)
    return gy, xs, gi, w


SLIPS = ("transposed_map", "cls_frame0", "cls_rounded_per_frame", "cls_counted_per_frame", "neighbour_rstd")


def emulate_fp32(gy, xs, gx_in, w, eps, F, slip=None):
    """The kernel's arithmetic in fp32 on the CPU: the row map (class rows summed in frame order in fp32) in front of
    ln_bwd_oracle.emulate_fp32.  slip: None or one of SLIPS.  Returns (gx, dweight, dbias) in xs's dtype."""
    B, N, C = xs.shape
    P = (N - 1) // F
    tok = to_token_layout(gy.detach().cpu().float(), B, F, P, slip=slip, dtype=xs.dtype)
    gx, dw, db = L.emulate_fp32(tok, xs, gx_in, w, eps, slip="neighbour_rstd" if slip == "neighbour_rstd" else None)
    if slip == "cls_counted_per_frame":  # the class row enters dbias once per frame instead of once
        counted = tok.clone()
        counted[:, 0] *= F
        db = L.emulate_fp32(counted, xs, gx_in, w, eps)[2]
    return gx, dw, db
