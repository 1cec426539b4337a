"""Accounting for the backward of the add + LayerNorm kernels (tome_layernorm_backward, csrc/tome_ln_bwd.h): fp64
reference from the stored 16-bit tensors, acceptance bound, inputs, an fp32 emulation of the kernel's arithmetic and the
launch form.  No test functions; importable without a GPU.  tests/test_ln_bwd_oracle_cpu.py shows on the CPU that the
bound accepts the emulation and rejects the slips such a kernel can make; tests/test_layernorm_backward_gpu.py applies
it to the kernels.

Reference
---------
xs: the 16-bit rows the forward normalised; gy: gradient of y; gw = gy * w; mean, var (biased) of xs in fp64,
rstd = (var + eps)^-1/2, xhat = (xs - mean) rstd:
    gx = gx_in + rstd (gw - mean(gw) - xhat mean(gw xhat)),   dweight = sum_rows gy xhat,   dbias = sum_rows gy.
The 16-bit operands are exact in fp64.  skip_first: gy has no row for the first row of every group; that row has
gx = gx_in (0 without) exactly and no share in dweight / dbias.

Bound (derived, not tuned; v = 2^-24, u = 2^-8 bf16 / 2^-11 fp16)
-----
gx: one rounding of the result to the token dtype, taken on an fp32 value: u |ref| (1 + 2^-20); plus the fp32
evaluation: every term of the formula is a sum of at most C products in any order (g(C) ~ C v on the sum of the
magnitudes) and a handful of further roundings (reciprocal of C, rsq, the products and the fma: 8 v), all of them
relative to the magnitudes that are added up, M:
    |gx - ref| <= u |ref| (1 + 2^-20) + (C + 8) v M,    M = rstd (|gw| + mean|gw| + |xhat| mean|gw xhat|) + |gx_in|
fp16 adds 2^-25 absolute: results below 2^-14 are subnormal, spaced 2^-24, and a correct rounding is off by up to
half of that whatever u says.
dweight / dbias: one rounding of the stored value, u |ref| (1 + 2^-20) [+ 2^-25 fp16], plus
  a. the summation.  The kernel does not add `rows` terms in one chain: a workgroup owns 4 R spw consecutive rows and
     adds their terms in some order into ONE partial row, then the `parts` partial rows are added in some order
     (`form`).  Any order inside a workgroup and any order over the partial rows: no term passes through more than
     L = 4 R spw + parts additions (plus the rounding of its own product), so the sum is off by at most
     (L + 1) v sum_rows |term| -- against (rows - 1) v for one chain of all rows; rows = 4 R spw parts, so L is the sum
     where rows is the product.  A statement about the partition into workgroups, which is part of the entry's
     contract (the workspace holds `parts` rows).
  b. the terms.  dbias: gy is exact in fp32, nothing to add.  dweight: xhat^ = fl(d^ rstd^).  The mean is a sum that
     is scaled afterwards (tests/ln_oracle.py, step 1): exact-sum rows have |m - mu| <= dm = g(3) |mu|, other rows
     dm = g(C + 2) mean|x|; a shifted mean moves every d of the row by the same amount, so its first-order effect on
     the variance is sum(d) dm = 0 and the variance keeps a relative (C + 6) v (C - 1 additions, the squares, 1/C, eps,
     2 v from d^ = fl(x - m)); rstd^ by rsq to 1 ulp: (C + 6) v / 2 + 2 v; the rounding of d^ and of the product: 2 v.
     |xhat^ - xhat| <= rstd dm + (C / 2 + 7) v |xhat|:
         |dw - ref| <= u |ref| (1 + 2^-20) + sum_rows |gy| rstd dm + (C / 2 + 7 + L + 1) v sum_rows |gy xhat|
         |db - ref| <= u |ref| (1 + 2^-20) + L v sum_rows |gy|
  c. a + b is tighter than the form the bound started from, (rows + C + 8) v sum_rows |term|, at large row counts; at
     few rows and large C (rows around zero: dm ~ (C + 2) v mean|x|, so b alone is ~1.5 C v) it is not.  The fp32
     allowance is the element-wise MINIMUM of the two, for dweight and dbias: never above the starting form.
What no bound can show in bf16: one of P partial rows left out moves a channel by about |ref| / sqrt(P), the rounding
of the stored value alone allows u |ref|; the share of channels where the former stays below the latter is
(2 / pi) atan(u sqrt(P)) -- 1 % at P = 16, 5.6 % at P = 512 for u = 2^-8.  That is the format, not the allowance (and
in fp16 the any-order allowance (L + 1) v of 512 partial rows is of the size of one partial row's share); the CPU
tests therefore show the dropped partial row on launches of at most 64 partial rows, at every width, and the counted
class row where the class rows are one row in 16, at 512 and at 4096 rows (512 partial rows, several slabs per wave).
"""
import torch

import ln_oracle

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
V32 = 2.0 ** -24
WAVE = 64
MAX_PARTS = 512  # csrc/tome_kernels.hip: LN_BWD_MAX_PARTS


def _rows64(t, C):
    return t.detach().to("cpu").double().reshape(-1, C)


def expand_gy(gy, xs, skip_first):
    """gy as [rows, C] float64 with zero rows for the class rows, and the mask of the rows that have a gradient."""
    C = xs.shape[-1]
    rows = xs.numel() // C
    if not skip_first:
        return _rows64(gy, C), torch.ones(rows, dtype=torch.bool)
    B, N = xs.shape[0], xs.shape[1]
    full = torch.zeros(B, N, C, dtype=torch.float64)
    full[:, 1:] = gy.detach().cpu().double().reshape(B, N - 1, C)
    has = torch.ones(B, N, dtype=torch.bool)
    has[:, 0] = False
    return full.reshape(-1, C), has.reshape(-1)


def reference(gy, xs, gx_in, w, eps, skip_first=False):
    """fp64 backward; dict of float64 CPU tensors: gx, M [rows, C]; dw, db, Tw, Tb [C]; has [rows]."""
    C = xs.shape[-1]
    x = _rows64(xs, C)
    g, has = expand_gy(gy, xs, skip_first)
    gi = torch.zeros_like(x) if gx_in is None else _rows64(gx_in, C)
    w64 = w.detach().cpu().double()
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    rstd = ((d * d).mean(-1, keepdim=True) + eps) ** -0.5
    xhat = d * rstd
    gw = g * w64
    ln = rstd * (gw - gw.mean(-1, keepdim=True) - xhat * (gw * xhat).mean(-1, keepdim=True))
    ln = torch.where(has[:, None], ln, torch.zeros_like(ln))
    M = rstd * (gw.abs() + gw.abs().mean(-1, keepdim=True) + xhat.abs() * (gw * xhat).abs().mean(-1, keepdim=True))
    M = torch.where(has[:, None], M, torch.zeros_like(M)) + gi.abs()
    exact = ln_oracle.exact_sum_rows(xs.detach().reshape(-1, C))[:, None]
    dm = torch.where(exact, ln_oracle._g(3) * mu.abs(), ln_oracle._g(C + 2) * x.abs().mean(-1, keepdim=True))
    return {"gx": gi + ln, "M": M, "dw": (g * xhat).sum(0), "db": g.sum(0), "Tw": (g * xhat).abs().sum(0),
            "Tb": g.abs().sum(0), "Tm": (g.abs() * rstd * dm).sum(0), "has": has, "rows": x.shape[0]}


def bound_gx(ref, dtype):
    C = ref["gx"].shape[-1]
    return (U[dtype] * ref["gx"].abs() * (1 + 2.0 ** -20) + (C + 8) * V32 * ref["M"]
            + (2.0 ** -25 if dtype == torch.float16 else 0.0))


def bound_param(ref, which, dtype):
    C = ref["gx"].shape[-1]
    R, spw, parts = form(ref["rows"], C)
    L = 4 * R * spw + parts
    if which == "dw":
        val, terms, e32 = ref["dw"], ref["Tw"], ref["Tm"] + (C / 2 + 7 + L + 1) * V32 * ref["Tw"]
    else:
        val, terms, e32 = ref["db"], ref["Tb"], L * V32 * ref["Tb"]
    e32 = torch.minimum(e32, (ref["rows"] + C + 8) * V32 * terms)  # never above the form the bound started from
    return U[dtype] * val.abs() * (1 + 2.0 ** -20) + e32 + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def outside_gx(gx, ref, dtype):
    """[rows] bool: does the row hold an element outside the bound (or a non-finite one)?  Also the worst err / bound."""
    got = _rows64(gx, ref["gx"].shape[-1])
    err, bnd = (got - ref["gx"]).abs(), bound_gx(ref, dtype)
    bad = ~torch.isfinite(got) | (err > bnd)
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), (err > 0).double() * float("inf"))
    return bad.any(-1), float(ratio.max())


def outside_param(got, ref, which, dtype):
    """[C] bool and the worst err / bound for dweight ("dw") or dbias ("db")."""
    got = got.detach().cpu().double().reshape(-1)
    val = ref["dw"] if which == "dw" else ref["db"]
    err, bnd = (got - val).abs(), bound_param(ref, which, dtype)
    return ~torch.isfinite(got) | (err > bnd), float((err / bnd.clamp_min(1e-300)).max())


def check(label, gx, dw, db, ref, dtype):
    """Assert the bound on every element of gx and, where given, dweight and dbias; prints each worst err / bound."""
    bad, worst = outside_gx(gx, ref, dtype)
    line = f"ln_bwd_oracle {label}: rows {ref['rows']} C {ref['gx'].shape[-1]} gx worst err/bound {worst:.3f}"
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


def residual_gradient_survives(run, x, residual, dev):
    """`run(x, residual)` -> the tokens a block step returns, with x WITHOUT grad, its LayerNorm frozen and the residual
    alone requiring grad (the first block behind a frozen embedding when only the attention trains): every returned
    tensor has a grad_fn, and residual.grad after a backward with fixed cotangents is, bit for bit, the one of the same
    call with x requiring grad as well -- which takes the Functions whoever else requires grad (deterministic kernels)."""
    grads = []
    for x_grad in (False, True):
        xi, ri = x.clone().requires_grad_(x_grad), residual.clone().requires_grad_(True)
        tokens = run(xi, ri)
        assert all(t.grad_fn is not None for t in tokens), f"x.requires_grad={x_grad}: a returned tensor has no grad_fn"
        gen = torch.Generator().manual_seed(11)
        torch.autograd.backward(tokens, [torch.randn(t.shape, generator=gen).to(t.dtype).to(dev) for t in tokens])
        assert ri.grad is not None, f"x.requires_grad={x_grad}: grad is None"
        grads.append(ri.grad)
    assert torch.equal(grads[0], grads[1])


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_inputs(shape, dtype, seed, far=True, grad_scale=1.0, skip_first=False, with_in=True):
    """xs: row i = shift_i + scale_i N(0,1) with scale_i = 2^(i mod 5 - 2) (two rows that share a wave never share an
    rstd) and, far=True, shift_i = +-30 scale_i (rows 30 standard deviations from zero); gy, gx_in ~ grad_scale N(0,1);
    weight 1 + 0.1 N(0,1).  CPU tensors of `dtype`: (gy, xs, gx_in or None, w)."""
    gen = torch.Generator().manual_seed(seed)
    C = shape[-1]
    rows = 1
    for s in shape[:-1]:
        rows *= s
    i = torch.arange(rows, dtype=torch.float64)
    scale = torch.exp2(i % 5 - 2)[:, None]
    shift = (30.0 * scale * (1 - 2 * (i[:, None] % 2))) if far else 0.0
    xs = (shift + scale * torch.randn(rows, C, generator=gen, dtype=torch.float64)).to(dtype).reshape(shape)
    gshape = (shape[0], shape[1] - 1, C) if skip_first else tuple(shape)
    gy = (grad_scale * torch.randn(gshape, generator=gen, dtype=torch.float64)).to(dtype)
    gi = (grad_scale * torch.randn(shape, generator=gen, dtype=torch.float64)).to(dtype) if with_in else None
    w = (1.0 + 0.1 * torch.randn(C, generator=gen, dtype=torch.float64)).to(dtype)
    return gy, xs, gi, w


# ---------------------------------------------------------------------------------------------------------------------
# launch form and an fp32 emulation of the kernel's arithmetic (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def form(rows, C):
    """(R rows per wave, slabs per wave, parts) as csrc/tome_kernels.hip ln_bwd_form picks them."""
    cpr = C // 8
    R = min(4, 3 * WAVE // cpr)
    wgs = (-(-rows // R) + 3) // 4
    spw = -(-wgs // MAX_PARTS)
    return R, spw, -(-wgs // spw)


def rows_of_part(rows, C):
    """[rows] long: the workgroup (= partial row of the workspace) every row belongs to."""
    R, spw, _ = form(rows, C)
    return torch.arange(rows) // (R * 4 * spw)


def emulate_fp32(gy, xs, gx_in, w, eps, skip_first=False, slip=None):
    """The kernel's formula in fp32 on the CPU (sums by torch, i.e. in another order than the kernel's), one rounding to
    the token dtype; dweight / dbias through per-workgroup fp32 partials.  slip: None, or one of the wrong answers the
    CPU tests must see rejected: "no_xhat_term", "neighbour_rstd", "chunk_out_of_mean", "class_row_counted",
    "partial_dropped".  Returns (gx, dweight, dbias) in xs's dtype."""
    dtype, C = xs.dtype, xs.shape[-1]
    x = xs.detach().cpu().float().reshape(-1, C)
    g64, has = expand_gy(gy, xs, skip_first)
    g = g64.float()
    if slip == "class_row_counted":  # the class row takes the gradient of the row behind it
        g = torch.where(has[:, None], g, torch.roll(g, -1, 0))
    inv_c = torch.tensor(1.0 / C, dtype=torch.float32)
    m = x.sum(-1, keepdim=True) * inv_c
    d = x - m
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) * inv_c + torch.tensor(eps, dtype=torch.float32))
    gw = g * w.detach().cpu().float()
    sg = gw.sum(-1, keepdim=True)
    if slip == "chunk_out_of_mean":
        sg = sg - gw[:, :8].sum(-1, keepdim=True)
    mg = sg * inv_c
    rs = torch.roll(rstd, 1, 0) if slip == "neighbour_rstd" else rstd
    k = rs * (rs * ((gw * d).sum(-1, keepdim=True) * inv_c))
    t = gw - mg - (0.0 if slip == "no_xhat_term" else d * k)
    gi = torch.zeros_like(x) if gx_in is None else gx_in.detach().cpu().float().reshape(-1, C)
    gx = torch.where(has[:, None], gi + rs * t, gi).to(dtype)
    part = rows_of_part(x.shape[0], C)
    nparts = int(part.max()) + 1
    gp = g if slip == "class_row_counted" else torch.where(has[:, None], g, torch.zeros_like(g))
    pw = torch.zeros(nparts, C).index_add_(0, part, gp * (d * rstd))
    pb = torch.zeros(nparts, C).index_add_(0, part, gp)
    if slip == "partial_dropped":
        pw[nparts // 2] = 0.0
        pb[nparts // 2] = 0.0
    return gx.reshape(xs.shape), pw.sum(0).to(dtype), pb.sum(0).to(dtype)
