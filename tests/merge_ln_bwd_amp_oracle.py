"""Accounting for tome_merge_ln_backward_amp (csrc/tome_merge_ln_bwd_amp.h), the backward of the fused residual add +
merge + LayerNorm launches under autocast: fp64 reference, acceptance bounds, inputs, and an fp32 emulation of the
contract with the slips such a kernel can make.  No test functions; importable without a GPU.
tests/test_merge_ln_bwd_amp_oracle_cpu.py shows on the CPU that the bounds accept the emulation and reject the slips;
tests/test_merge_ln_backward_amp_gpu.py applies them to the kernel.  Nothing is restated here that another oracle
already holds: the pieces are imported.

Reference
---------
xs [n, To, C]: the merged rows the forward stored and normalised, of the 16-bit dtype `half` or fp32; gy of `half`;
gx_out of xs's dtype or None; weight fp32.  merge_ln_bwd_oracle.reference does all of it in fp64 (the LayerNorm backward
of the stored rows by ln_bwd_oracle.reference, then its scale step gx[t] = gm[o(t)] in_mul[t] / out_div[o(t)], 0 for a
token without a row) with o(t) from merge_ln_bwd_oracle.rows_of_plan, i.e. from the matching's index tensors and not from
the row map the kernel reads.  fp32 operands are exact in fp64 like the 16-bit ones.
ln_amp_oracle.reference adds Em, the allowance for the error of the row's mean, which an fp32 output cannot hide behind
a 16-bit rounding (derived there); it rides on gm, so the scale multiplies it like the rest.
Input condition: ln_oracle's, at least 99 % exact-sum rows among xs (then dm = g(3) |mu| on them) -- asserted by
`reference` itself; `make_tensors` builds xs from ln_amp_oracle.forward_inputs, whose rows meet it by construction.

Bounds (derived, not tuned; v = 2^-24, u of the OUTPUT's dtype: 2^-24 for fp32, 2^-8 bf16, 2^-11 fp16;
s = |in_mul[t] / out_div[o(t)]|, g(k) = k v / (1 - k v))
------
gx: the kernel keeps gm in fp32 and does not round it.  The fp32 evaluation of the un-rounded LayerNorm term is allowed
(C + 8) v M[o] (ln_bwd_oracle) plus Em[o] (ln_amp_oracle); a scale multiplies an error like a value: both times s
(merge_ln_bwd_oracle's E, and Em s here).  Where scales are given, the division and the product are two correctly
rounded fp32 operations on that value: a factor (1 + d1)(1 + d2), |di| <= v, on the value AND its error, at most
g(2) (|ref| + E + Em s).  Without scales the kernel does neither and nothing is allowed for them.  One rounding to the
output's dtype of an fp32 value: u |ref| (1 + 2^-20) (for an fp32 output, the rounding of the last fp32 operation).
    |gx - ref| <= u |ref| (1 + 2^-20) + E + Em s + [scales] g(2) (|ref| + E + Em s)        [+ 2^-25 for an fp16 output]
A token without a row (drop) has ref = 0 and s = 0: only 0 is accepted.  A 16-bit gx has no room for a second rounding
(merge_ln_bwd_oracle.tie_row builds the row that shows it), an fp32 gx none for any 16-bit rounding at all.
gx16 must equal gx.to(half) bit for bit: it is compared, not bounded.
dweight / dbias (fp32): ln_amp_oracle.bound_param's formula -- u = 2^-24 on the stored value, the share of the mean's
error Tm kept outside the closing minimum -- with THIS launch's partition: a workgroup owns 4 R spw consecutive slabs of
INPUT tokens and adds the terms of the merged rows its tokens own into one partial row, `parts` partial rows are added
after that: L = 4 R spw + parts additions at most for any term (merge_ln_bwd_oracle.form; a token that owns nothing
adds an exact zero); never above (rows + C + 8) v sum |term| with rows = n To, one chain over the merged rows.
"""
import torch

import ln_amp_oracle as ao
import ln_oracle as lo
import merge_ln_bwd_oracle as mo

F32, HALVES, U, V32 = ao.F32, ao.HALVES, ao.U, ao.V32
form, FORM_WIDTHS, expected_form, rows_of_plan, hand_plan, size_out_of = (mo.form, mo.FORM_WIDTHS, mo.expected_form,
                                                                          mo.rows_of_plan, mo.hand_plan, mo.size_out_of)


def reference(gy, gx_out, xs, out_div, in_mul, w, eps, row_of):
    """merge_ln_bwd_oracle.reference (fp64: gx, E, gm, scale, row_of, the parameter fields over the merged rows) plus
    "Em" [n, T, C], ln_amp_oracle's allowance for the mean scaled like E, "scaled" (are there scales?) and
    "exact_share".  Asserts the input condition."""
    n, To, C = xs.shape
    T = row_of.shape[1]
    share = float(lo.exact_sum_rows(xs.detach().reshape(-1, C)).double().mean())
    assert share >= 0.99, f"only {100 * share:.1f} % of the stored rows are exact-sum rows"
    ref = mo.reference(gy, gx_out, xs, out_div, in_mul, w, eps, row_of)
    Em = ao.reference(gy, xs, gx_out, w, eps)["Em"].reshape(n, To, C)
    idx = row_of.clamp_min(0)[..., None].expand(n, T, C)
    ref.update(Em=Em.gather(1, idx) * ref["scale"].abs()[..., None], scaled=out_div is not None or in_mul is not None,
               exact_share=share)
    return ref


def bound_gx(ref, out_dtype):
    a = ref["gx"].abs()
    e32 = ref["E"] + ref["Em"]
    if ref["scaled"]:
        e32 = e32 + lo._g(2) * (a + e32)
    return U[out_dtype] * a * (1 + 2.0 ** -20) + e32 + (2.0 ** -25 if out_dtype == torch.float16 else 0.0)


def bound_param(ref, which):
    C = ref["gx"].shape[-1]
    R, spw, parts = mo.form(ref["n"], ref["T"], C)
    L = 4 * R * spw + parts
    start = (ref["rows"] + C + 8) * V32
    if which == "dw":
        val, e32 = ref["dw"], ref["Tm"] + torch.minimum((C / 2 + 7 + L + 1) * V32 * ref["Tw"], start * ref["Tw"])
    else:
        val, e32 = ref["db"], torch.minimum(L * V32 * ref["Tb"], start * ref["Tb"])
    return U[F32] * val.abs() * (1 + 2.0 ** -20) + e32


def outside_gx(gx, ref, out_dtype=None):
    """[n, T] bool: does the token's row hold an element outside the bound (or a non-finite one)?  And worst err / bound."""
    got = gx.detach().cpu().double().reshape(ref["gx"].shape)
    err, bnd = (got - ref["gx"]).abs(), bound_gx(ref, out_dtype or gx.dtype)
    bad = ~torch.isfinite(got) | (err > bnd)
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return bad.any(-1), float(ratio.max())


def outside_param(got, ref, which):
    got = got.detach().cpu().double().reshape(-1)
    val = ref["dw"] if which == "dw" else ref["db"]
    err, bnd = (got - val).abs(), bound_param(ref, which)
    return ~torch.isfinite(got) | (err > bnd), float((err / bnd.clamp_min(1e-300)).max())


def check(label, gx, gx16, dw, db, ref, half):
    """Assert the bounds on gx (u of its own dtype), dweight, dbias (fp32), and gx16 == gx.to(half) bit for bit; prints
    each worst err / bound."""
    assert gx.dtype in (half, F32) and (dw is None or dw.dtype == F32) and (db is None or db.dtype == F32)
    bad, worst = outside_gx(gx, ref)
    line = (f"merge_ln_bwd_amp_oracle {label}: n {ref['n']} T {ref['T']} C {ref['gx'].shape[-1]} gx({gx.dtype}) worst "
            f"err/bound {worst:.3f}")
    fails = []
    if bool(bad.any()):
        fails.append(f"gx: {int(bad.sum())} token rows outside, first {torch.nonzero(bad)[0].tolist()}")
    for which, got in (("dw", dw), ("db", db)):
        if got is None:
            continue
        badp, worstp = outside_param(got, ref, which)
        line += f" {which} {worstp:.3f}"
        if bool(badp.any()):
            fails.append(f"{which}: {int(badp.sum())} channels outside, first {int(torch.nonzero(badp)[0])}")
    if gx16 is not None:
        assert gx.dtype == F32 and gx16.dtype == half
        same = torch.equal(gx16.cpu().view(torch.int16), gx.cpu().to(half).view(torch.int16))
        line += f" gx16 {'=' if same else '!='} gx.to({half})"
        if not same:
            fails.append("gx16 is not gx.to(dtype) bit for bit")
    print(line)
    assert not fails, (label, fails)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_tensors(n, T, r, C, x_dtype, a_dtype, half, size_dtype, seed, with_mul=True, with_in=True, drop=False):
    """CPU tensors (gy, gx_out or None, xs, w, size or None) for the backward of a merge of [n, T, C] to [n, T - r, C]:
    xs = the row ln_amp_oracle.forward_inputs' (x, addend) pair of dtypes (x_dtype, a_dtype) stores (exact-sum rows; an
    fp32 stream with an fp32 or absent addend is not representable in 16 bits), gy ~ N(0, 1) of `half`, gx_out ~ N(0, 1)
    of x_dtype (full fp32 mantissas on an fp32 stream), weight fp32 with full mantissas, sizes 1..4 (exact in every
    dtype) of size_dtype; drop: no sizes."""
    To = T - r
    xs = ao.stored_sum(*ao.forward_inputs((n, To, C), x_dtype, a_dtype, seed))
    assert xs.dtype == x_dtype
    gen = torch.Generator().manual_seed(seed + 7)
    gy = torch.randn((n, To, C), generator=gen, dtype=torch.float64).to(half)
    gi = torch.randn((n, To, C), generator=gen, dtype=torch.float64).to(x_dtype) if with_in else None
    w, _ = ao.affine(C, seed + 3)
    size = None
    if not drop and with_mul:
        size = torch.randint(1, 5, (n, T, 1), generator=gen).to(size_dtype)
    return gy, gi, xs, w, size


# ---------------------------------------------------------------------------------------------------------------------
# an fp32 emulation of the contract (CPU), with the slips the CPU tests must see rejected
# ---------------------------------------------------------------------------------------------------------------------
SLIPS = ("gm_rounded_16bit", "stats_from_16bit_copy", "out_div_at_t", "dropped_token_gets_gm", "dest_counted_per_token",
         "gx16_twice_rounded")


def parts_of_tokens(n, T, C):
    """[n, T] long: the workgroup (= partial row of the workspace) every input token belongs to."""
    R, spw, _ = mo.form(n, T, C)
    wpg = -(-T // R)
    slab = torch.arange(n)[:, None] * wpg + torch.arange(T)[None, :] // R
    return slab // (4 * spw)


def emulate(gy, gx_out, xs, out_div, in_mul, w, eps, row_of, owns, slip=None):
    """(gx, gx16 or None, dweight, dbias) as an honest fp32 evaluation of the contract computes them (sums by torch:
    another order than the kernel's): gm in fp32 and not rounded, the division first and then the product, one rounding
    to xs's dtype, gx16 a cast of gx, the parameters through per-workgroup fp32 partials of the owners' terms."""
    assert slip is None or slip in SLIPS
    half = gy.dtype
    n, To, C = xs.shape
    T = row_of.shape[1]
    x = xs.detach().float().reshape(-1, C)
    src = x.to(half).float() if slip == "stats_from_16bit_copy" else x
    inv_c = torch.tensor(1.0 / C, dtype=F32)
    m = src.sum(-1, keepdim=True) * inv_c
    ds = src - m
    rstd = torch.rsqrt((ds * ds).sum(-1, keepdim=True) * inv_c + torch.tensor(eps, dtype=F32))
    d = x - m
    g = gy.detach().float().reshape(-1, C)
    gw = g * w.float()
    mg = gw.sum(-1, keepdim=True) * inv_c
    k = rstd * (rstd * ((gw * d).sum(-1, keepdim=True) * inv_c))
    gm = rstd * (gw - mg - d * k)
    if gx_out is not None:
        gm = gx_out.detach().float().reshape(-1, C) + gm
    gm = gm.reshape(n, To, C)
    has = row_of >= 0
    o = row_of.clamp_min(0)
    idx = o[..., None].expand(n, T, C)

    def scaled(v):
        if out_div is not None:
            at = torch.arange(T).clamp_max(To - 1).expand(n, T) if slip == "out_div_at_t" else o
            v = v / out_div.detach().float().reshape(n, To).gather(1, at)[..., None]
        if in_mul is not None:
            v = v * in_mul.detach().float().reshape(n, T, 1)
        return v

    keep = torch.ones_like(has) if slip == "dropped_token_gets_gm" else has
    zero = torch.zeros((), dtype=F32)
    once = gm.to(half).float() if slip == "gm_rounded_16bit" else gm
    gx = torch.where(keep[..., None], scaled(once.gather(1, idx)), zero).to(xs.dtype)
    gx16 = None
    if xs.dtype == F32:
        gx16 = gx.to(half)
        if slip == "gx16_twice_rounded":  # gm rounded on its own, then the scaled value rounded again
            gx16 = torch.where(keep[..., None], scaled(gm.to(half).float().gather(1, idx)), zero).to(half)
    counted = has if slip == "dest_counted_per_token" else owns
    gt = torch.where(counted[..., None], g.reshape(n, To, C).gather(1, idx), zero).reshape(-1, C)
    xhat = (d * rstd).reshape(n, To, C).gather(1, idx).reshape(-1, C)
    part = parts_of_tokens(n, T, C).reshape(-1)
    nparts = int(part.max()) + 1
    pw = torch.zeros(nparts, C).index_add_(0, part, gt * xhat)
    pb = torch.zeros(nparts, C).index_add_(0, part, gt)
    return gx, gx16, pw.sum(0), pb.sum(0)
