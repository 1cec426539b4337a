"""Accounting for the mixed-precision add + LayerNorm kernels (tome_add_layernorm_amp, tome_layernorm_backward_amp:
fp32 LayerNorm parameters, a 16-bit y / gy, a residual stream of that 16-bit dtype or fp32 -- a model under autocast).
Type combinations, inputs, bounds for fp32 outputs and fp32 emulations with the slips such kernels can make.  No test
functions; importable without a GPU.  tests/test_ln_amp_oracle_cpu.py shows on the CPU that the bounds accept the
emulations and reject the slips; tests/test_layernorm_amp_gpu.py applies them to the kernels.

Forward.  The stored row x' is compared bit for bit: `x + addend.float()` for an fp32 stream (one fp32 rounding),
`(x + addend)` in the 16-bit dtype for a 16-bit stream.  y is checked with ln_oracle.check on the STORED rows and the
fp32 parameters: its reference is fp64 of whatever it is given, its bound u |ref| + e32 has u of y's dtype and an e32
derived for any fp32 evaluation, so neither knows the byte width of the row.  Its input condition (>= 99 % exact-sum
rows, e32 <= u/8 |ref| + 2^-14 on them) is asserted by `check` itself; the inputs here are made for it:
  * a 16-bit stream or a 16-bit addend: ln_oracle.signature_rows and its grid noise, as for the 16-bit kernels;
  * an fp32 stream with an fp32 addend: the addend is `fine_addend`, multiples of s_k / 128 -- finer than bf16 AND fp16
    can hold next to M_k (fp16 spacing at M = 24 is 2^-6 = s / 64), so the stored fp32 row is NOT representable in 16
    bits and a kernel that takes its statistics from a 16-bit copy is seen; sum|x| / G <= 1024 * 500 * 128 / 8 < 2^24
    keeps every row an exact-sum row.
Backward.  ln_bwd_oracle.reference (fp64 of the stored tensors) and its bounds with the unit roundoff of the OUTPUT's
dtype: u = 2^-24 for the fp32 outputs (gx of an fp32 stream, dweight and dbias always), the 16-bit u for a 16-bit gx.
The fp16 subnormal term applies to fp16 outputs only.  gx16 must equal gx.to(dtype) bit for bit.
One term is added to ln_bwd_oracle's gx bound, which that module could leave to the 16-bit rounding it allows (u = 2^-8
or 2^-11 of |ref|) and an fp32 output cannot: the error of the row's MEAN.  ln_bwd_oracle accounts for it in dweight
(its step b: |m - mu| <= dm, with dm = g(3) |mu| on exact-sum rows and g(C + 2) mean|x| otherwise, from
tests/ln_oracle.py step 1) but not in gx.  A mean off by delta, |delta| <= dm, moves every d of the row by the same
delta: the variance keeps its first order (sum d = 0), xhat moves by rstd delta, mean(gw xhat) by rstd delta mean(gw),
so rstd xhat mean(gw xhat) moves by at most
    Em = rstd^2 dm (mean|gw xhat| + |xhat| mean|gw|) (1 + 2^-10)          (2^-10: the second order, dm rstd << 2^-10)
per element.  On rows 30 standard deviations from zero dm rstd is 30 (C + 2) v, well above the (C + 8) v of the other
roundings; any fp32 evaluation that sums the row has it.  `reference` below is ln_bwd_oracle.reference with Em added.
For the same reason dweight's allowance for the mean (Tm) is kept outside ln_bwd_oracle's closing minimum (bound_param).
"""
import torch

import ln_bwd_oracle as bo
import ln_oracle as lo

HALVES = (torch.bfloat16, torch.float16)
F32 = torch.float32
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
V32 = 2.0 ** -24


def combos(half):
    """Every legal (x dtype, addend dtype or None) for y of `half`."""
    return [(half, half), (half, None), (F32, half), (F32, F32), (F32, None)]


def illegal_combos():
    """(x, addend, y) dtype triples the forward entry must refuse."""
    b, h, f = torch.bfloat16, torch.float16, F32
    return [(b, h, b), (h, b, h), (b, f, b), (h, f, h), (b, b, h), (h, h, b), (f, b, h), (f, h, b), (f, f, f), (b, b, f),
            (f, None, f), (b, None, h)]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def fine_addend(shape, seed, klass=None):
    """fp32 addend s_k / 128 * round(64 z): a grid no 16-bit format holds next to the row's mean (module docstring)."""
    lead, C = tuple(shape[:-1]), shape[-1]
    nrows = 1
    for s in lead:
        nrows *= s
    k = (torch.arange(nrows) % len(lo.SIGNATURES)) if klass is None else klass.reshape(-1).cpu().long() % len(lo.SIGNATURES)
    s = torch.tensor(lo.SIGNATURES, dtype=torch.float64)[k, 1:2]
    z = torch.randn((nrows, C), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    a = s / 128.0 * (2.0 * torch.round(32.0 * z) + 1.0)  # odd multiples: never on the coarser 16-bit grids
    out = a.to(F32)
    assert torch.equal(out.double(), a)
    return out.reshape(*lead, C)


def forward_inputs(shape, x_dtype, a_dtype, seed, klass=None):
    """(x, addend or None) CPU tensors for one forward case; x' = x + addend is exact in x_dtype's arithmetic for fp32
    streams, and a signature row again for 16-bit ones."""
    x = lo.signature_rows(shape, x_dtype, seed, 1, klass)
    if a_dtype is None:
        if x_dtype == F32:  # a stream that is fp32 for a reason: not representable in 16 bits
            x = x + fine_addend(shape, seed + 2, klass)
        return x, None
    if a_dtype == F32:
        return x, fine_addend(shape, seed + 1, klass)
    return x, lo.signature_rows(shape, a_dtype, seed + 1, 1, klass, 0.5, offset=False)


def stored_sum(x, a):
    """The row the kernel must store, bit for bit: torch's own `x + a` (type promotion makes it x + a.float() for an fp32
    stream and the rounded 16-bit sum for a 16-bit one)."""
    return x if a is None else x + a


def affine(C, seed):
    """fp32 LayerNorm parameters with full fp32 mantissas (no 16-bit format holds them)."""
    return lo.affine(C, F32, seed)


def backward_inputs(shape, x_dtype, half, seed, skip_first=False, with_in=True, **kw):
    """ln_bwd_oracle.make_inputs in the mixed dtypes: gy `half`, xs / gx_in `x_dtype`, weight fp32."""
    gy, xs, gi, w = bo.make_inputs(shape, torch.float64, seed, skip_first=skip_first, with_in=with_in, **kw)
    return gy.to(half), xs.to(x_dtype), (None if gi is None else gi.to(x_dtype)), w.to(F32)


# ---------------------------------------------------------------------------------------------------------------------
# backward bounds: ln_bwd_oracle's formulas with the unit roundoff of the output's dtype
# ---------------------------------------------------------------------------------------------------------------------
def _floor(dtype):
    return 2.0 ** -25 if dtype == torch.float16 else 0.0


def reference(gy, xs, gx_in, w, eps, skip_first=False):
    """ln_bwd_oracle.reference (fp64 of the stored tensors) plus "Em" [rows, C], the allowance for the error of the mean
    (module docstring)."""
    ref = bo.reference(gy, xs, gx_in, w, eps, skip_first=skip_first)
    C = xs.shape[-1]
    x = xs.detach().cpu().double().reshape(-1, C)
    g, has = bo.expand_gy(gy, xs, skip_first)
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    rstd = ((d * d).mean(-1, keepdim=True) + eps) ** -0.5
    xhat = d * rstd
    gw = g * w.detach().cpu().double()
    exact = lo.exact_sum_rows(xs.detach().reshape(-1, C))[:, None]
    dm = torch.where(exact, lo._g(3) * mu.abs(), lo._g(C + 2) * x.abs().mean(-1, keepdim=True))
    Em = rstd * rstd * dm * ((gw * xhat).abs().mean(-1, keepdim=True) + xhat.abs() * gw.abs().mean(-1, keepdim=True))
    ref["Em"] = torch.where(has[:, None], Em * (1 + 2.0 ** -10), torch.zeros_like(Em))
    return ref


def bound_gx(ref, out_dtype):
    C = ref["gx"].shape[-1]
    return (U[out_dtype] * ref["gx"].abs() * (1 + 2.0 ** -20) + (C + 8) * V32 * ref["M"] + ref["Em"]
            + _floor(out_dtype))


def bound_param(ref, which):
    """dweight / dbias are fp32: u = 2^-24 on the stored value, the summation and term allowances of ln_bwd_oracle."""
    C = ref["gx"].shape[-1]
    R, spw, parts = bo.form(ref["rows"], C)
    L = 4 * R * spw + parts
    start = (ref["rows"] + C + 8) * V32  # ln_bwd_oracle's step c: the form its bound started from, per unit of the terms
    if which == "dw":
        # Tm, the share of the mean's error (ln_bwd_oracle step b), stays OUTSIDE the minimum of step c: the starting
        # form counts summation and rounding steps, the mean's error is a property of the row (30 (C + 2) v of a term
        # on rows 30 standard deviations from zero).  Behind a 16-bit rounding of the result that went unseen.
        val, e32 = ref["dw"], ref["Tm"] + torch.minimum((C / 2 + 7 + L + 1) * V32 * ref["Tw"], start * ref["Tw"])
    else:
        val, e32 = ref["db"], torch.minimum(L * V32 * ref["Tb"], start * ref["Tb"])
    return U[F32] * val.abs() * (1 + 2.0 ** -20) + e32


def outside_gx(gx, ref, out_dtype):
    got = gx.detach().cpu().double().reshape(ref["gx"].shape)
    err, bnd = (got - ref["gx"]).abs(), bound_gx(ref, out_dtype)
    bad = ~torch.isfinite(got) | (err > bnd)
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), (err > 0).double() * float("inf"))
    return bad.any(-1), float(ratio.max())


def outside_param(got, ref, which):
    got = got.detach().cpu().double().reshape(-1)
    val = ref["dw"] if which == "dw" else ref["db"]
    err, bnd = (got - val).abs(), bound_param(ref, which)
    return ~torch.isfinite(got) | (err > bnd), float((err / bnd.clamp_min(1e-300)).max())


def check_backward(label, gx, gx16, dw, db, ref, half):
    """Assert the bounds on gx (u of its own dtype), dweight, dbias (fp32), and gx16 == gx.to(half) bit for bit."""
    assert dw is None or dw.dtype == F32
    assert db is None or db.dtype == F32
    bad, worst = outside_gx(gx, ref, gx.dtype)
    line = f"ln_amp_oracle {label}: rows {ref['rows']} C {ref['gx'].shape[-1]} gx({gx.dtype}) worst err/bound {worst:.3f}"
    fails = [] if not bool(bad.any()) else [f"gx: {int(bad.sum())} rows outside, first row {int(torch.nonzero(bad)[0])}"]
    for which, got in (("dw", dw), ("db", db)):
        if got is None:
            continue
        badp, worstp = outside_param(got, ref, which)
        line += f" {which} {worstp:.3f}"
        if bool(badp.any()):
            fails.append(f"{which}: {int(badp.sum())} channels outside, first {int(torch.nonzero(badp)[0])}")
    if gx16 is not None:
        assert gx.dtype == F32 and gx16.dtype == half
        same = torch.equal(gx16.view(torch.int16), gx.to(half).view(torch.int16))
        line += f" gx16 {'=' if same else '!='} gx.to({half})"
        if not same:
            fails.append("gx16 is not gx.to(dtype) bit for bit")
    print(line)
    assert not fails, (label, fails)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulations (CPU), with the slips the CPU tests must see rejected
# ---------------------------------------------------------------------------------------------------------------------
FORWARD_SLIPS = ("weights_16bit", "stats_from_16bit_copy", "sum_rounded_16bit", "unit_out_of_row", "neighbour_stats")
BACKWARD_SLIPS = ("class_row_counted", "gx16_twice_rounded")


def emulate_forward(x, a, w, b, eps, half, slip=None):
    """(x', y) as an honest fp32 evaluation computes them (sums by torch: another order than the kernel's)."""
    assert slip is None or slip in FORWARD_SLIPS
    xs = stored_sum(x, a)
    if slip == "sum_rounded_16bit" and xs.dtype == F32:
        xs = xs.to(half).float()
    C = xs.shape[-1]
    v = xs.float().reshape(-1, C)
    src = v.to(half).float() if slip == "stats_from_16bit_copy" else v
    inv_c = torch.tensor(1.0 / C, dtype=F32)
    total = src.sum(-1, keepdim=True)
    if slip == "unit_out_of_row":
        total = total - src[:, :8].sum(-1, keepdim=True)
    m = total * inv_c
    ds = src - m
    rstd = torch.rsqrt((ds * ds).sum(-1, keepdim=True) * inv_c + torch.tensor(eps, dtype=F32))
    if slip == "neighbour_stats":
        m, rstd = torch.roll(m, 1, 0), torch.roll(rstd, 1, 0)
    wf, bf = w.float(), b.float()
    if slip == "weights_16bit":
        wf, bf = w.to(half).float(), b.to(half).float()
    y = ((v - m) * (wf * rstd) + bf).to(half)
    return xs, y.reshape(xs.shape)


def emulate_backward(gy, xs, gx_in, w, eps, skip_first=False, slip=None):
    """(gx, gx16 or None, dweight, dbias): the kernel's formula in fp32, gx in xs's dtype, parameters fp32 through
    per-workgroup partials (ln_bwd_oracle.emulate_fp32 with the mixed dtypes)."""
    assert slip is None or slip in BACKWARD_SLIPS
    half, C = gy.dtype, xs.shape[-1]
    x = xs.detach().float().reshape(-1, C)
    g64, has = bo.expand_gy(gy, xs, skip_first)
    g = g64.float()
    if slip == "class_row_counted":
        g = torch.where(has[:, None], g, torch.roll(g, -1, 0))
    inv_c = torch.tensor(1.0 / C, dtype=F32)
    m = x.sum(-1, keepdim=True) * inv_c
    d = x - m
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) * inv_c + torch.tensor(eps, dtype=F32))
    gw = g * w.float()
    mg = gw.sum(-1, keepdim=True) * inv_c
    k = rstd * (rstd * ((gw * d).sum(-1, keepdim=True) * inv_c))
    ln = rstd * (gw - mg - d * k)
    gi = torch.zeros_like(x) if gx_in is None else gx_in.detach().float().reshape(-1, C)
    gx = torch.where(has[:, None], gi + ln, gi).to(xs.dtype).reshape(xs.shape)
    gx16 = None
    if xs.dtype == F32:
        gx16 = gx.to(half)
        if slip == "gx16_twice_rounded":  # the LayerNorm's share rounded on its own, then the sum rounded again
            gx16 = torch.where(has[:, None], gi + ln.to(half).float(), gi).to(half).reshape(xs.shape)
    part = bo.rows_of_part(x.shape[0], C)
    nparts = int(part.max()) + 1
    gp = g if slip == "class_row_counted" else torch.where(has[:, None], g, torch.zeros_like(g))
    pw = torch.zeros(nparts, C).index_add_(0, part, gp * (d * rstd))
    pb = torch.zeros(nparts, C).index_add_(0, part, gp)
    return gx, gx16, pw.sum(0), pb.sum(0)
