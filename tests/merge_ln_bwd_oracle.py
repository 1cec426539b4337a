"""Accounting for tome_merge_ln_backward (csrc/tome_merge_ln_bwd.h), the backward of the fused residual add + merge +
LayerNorm launches: fp64 reference, acceptance bound, inputs and the launch form.  No test functions; importable without
a GPU.  tests/test_merge_ln_bwd_oracle_cpu.py shows on the CPU that the bound accepts the rounded reference and rejects
the slips such a kernel can make; tests/test_merge_ln_backward_gpu.py applies it to the kernel.

Reference
---------
xs [n, To, C]: the 16-bit merged rows the forward stored and normalised; gy: gradient of y; gx_out: gradient that reaches
xs through the residual stream (or None).  The LayerNorm backward of the stored rows is ln_bwd_oracle.reference:
    gm[o] = gx_out[o] + rstd (gw - mean(gw) - xhat mean(gw xhat)),   dweight = sum_o gy xhat,   dbias = sum_o gy
with the parameter sums over the n To MERGED rows, each once.  Then the gather with the two scales, in fp64:
    gx[t] = gm[o(t)] in_mul[t] / out_div[o(t)]          (0 for a token without a row: drop)
o(t) comes from the matching's index tensors (rows_of_plan: the reference's output layout, merge.py:82-85), not from the
row map the kernel reads.  The 16-bit operands and the scales are exact in fp64.

Bound (derived, not tuned; v = 2^-24, u = 2^-8 bf16 / 2^-11 fp16, s = in_mul[t] / out_div[o(t)])
-----
gx: the kernel keeps gm in fp32 and does not round it.  ln_bwd_oracle allows the fp32 evaluation of the un-rounded
LayerNorm term (C + 8) v M[o] (its bound_gx without the rounding of the result); a scale multiplies an error like a
value: (C + 8) v M[o(t)] s.  The division and the product in fp32 are two correctly rounded operations, allowed 2 ulp
of fp32 on the value: 2 * 2^-23 |ref|.  One rounding to the token dtype of an fp32 value: u |ref| (1 + 2^-20).
    |gx - ref| <= (C + 8) v M[o(t)] s + u |ref| (1 + 2^-20) + 2^-22 |ref|        [+ 2^-25 fp16: subnormal results]
A token without a row has ref = 0, M s = 0: only 0 is accepted.  What the bound has no room for is a SECOND rounding to
the token dtype (gm rounded before the scales, what tome_layernorm_backward followed by tome_merge_backward do): at the
bottom of a binade u |ref| is half an ulp, and a first rounding that lands the product on a tie moves the result by a
whole ulp (tie_row builds such a row).
dweight / dbias: ln_bwd_oracle.bound_param's formula with this launch's partition: a workgroup owns 4 R spw consecutive
slabs of INPUT tokens and adds the terms of the merged rows its tokens own into one partial row, `parts` partial rows are
added after that: L = 4 R spw + parts additions at most for any term (terms of tokens that own nothing are zeros, exact);
never above (rows + C + 8) v sum |term| with rows = n To, the bound of one chain over the merged rows.
"""
import torch

import ln_bwd_oracle as bo

U, V32, WAVE, MAX_PARTS = bo.U, bo.V32, bo.WAVE, bo.MAX_PARTS


def form(n, T, C):
    """(R input-token rows per wave, slabs per wave, parts) as csrc/tome_kernels.hip merge_ln_bwd_form picks them."""
    cpr = C // 8
    R = min(4, 3 * WAVE // cpr)
    wpg = -(-T // R)
    wgs = (n * wpg + 3) // 4
    spw = -(-wgs // MAX_PARTS)
    return R, spw, -(-wgs // spw)


# one width for every (chunks per lane, rows per wave) form the dispatch instantiates: three chunks per lane always,
# R = min(4, 192 / (C / 8))
FORM_WIDTHS = {(3, 4): 384, (3, 3): 512, (3, 2): 768, (3, 1): 1024}


def expected_form(C):
    return 3, min(4, 3 * WAVE // (C // 8))


def rows_of_plan(src_idx, dst_idx, unm_idx, T, r, distill=False, drop=False):
    """(row_of [n, T] long, -1: no row; owns [n, T] bool) from the matching's index tensors ([n, r(,1)], [n, U(,1)]) in the
    reference's output layout: unmerged even tokens in unm_idx order, then the odd tokens; with a distillation token
    [unm 0, dst 0, unm 1.., dst 1..].  An odd token owns its row, an even token its own row unless it was merged away."""
    src = src_idx.detach().cpu().long().reshape(src_idx.shape[0], -1)
    dst = dst_idx.detach().cpu().long().reshape(src.shape[0], -1)
    unm = unm_idx.detach().cpu().long().reshape(src.shape[0], -1)
    n, T1 = src.shape[0], (T + 1) // 2
    Uu = T1 - r
    assert src.shape[1] == r and unm.shape[1] == Uu
    d_row = lambda j: torch.where(j == 0, torch.ones_like(j), Uu + j) if distill else Uu + j  # noqa: E731
    u_row = lambda k: torch.where(k >= 1, k + 1, k) if distill else k  # noqa: E731
    row_of = torch.full((n, T), -2, dtype=torch.long)
    owns = torch.zeros(n, T, dtype=torch.bool)
    row_of[:, 1::2] = d_row(torch.arange(T // 2))
    owns[:, 1::2] = True
    row_of.scatter_(1, 2 * unm, u_row(torch.arange(Uu)).expand(n, Uu))
    owns.scatter_(1, 2 * unm, torch.ones(n, Uu, dtype=torch.bool))
    row_of.scatter_(1, 2 * src, torch.full_like(src, -1) if drop else d_row(dst))
    assert int(row_of.min()) >= -1, "an even token is in neither set"
    return row_of, owns


def reference(gy, gx_out, xs, out_div, in_mul, w, eps, row_of):
    """fp64 backward; dict of float64 CPU tensors: gx, E (the scaled fp32 allowance) [n, T, C]; gm [n, To, C]; the
    parameter fields of ln_bwd_oracle.reference over the merged rows; n, T."""
    n, To, C = xs.shape
    T = row_of.shape[1]
    ln = bo.reference(gy, xs, gx_out, w, eps)
    gm, M = ln["gx"].reshape(n, To, C), ln["M"].reshape(n, To, C)
    o = row_of.clamp_min(0)
    s = torch.ones(n, T, dtype=torch.float64)
    if in_mul is not None:
        s = s * in_mul.detach().cpu().double().reshape(n, T)
    if out_div is not None:
        s = s / out_div.detach().cpu().double().reshape(n, To).gather(1, o)
    s = torch.where(row_of >= 0, s, torch.zeros_like(s))[..., None]
    idx = o[..., None].expand(n, T, C)
    ref = dict(ln)
    ref.update(gx=gm.gather(1, idx) * s, E=(C + 8) * V32 * M.gather(1, idx) * s.abs(), gm=gm, n=n, T=T, row_of=row_of,
               scale=s[..., 0])
    return ref


def bound_gx(ref, dtype):
    a = ref["gx"].abs()
    return ref["E"] + U[dtype] * a * (1 + 2.0 ** -20) + 2.0 ** -22 * a + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def bound_param(ref, which, dtype):
    C = ref["gx"].shape[-1]
    R, spw, parts = form(ref["n"], ref["T"], C)
    L = 4 * R * spw + parts
    if which == "dw":
        val, terms, e32 = ref["dw"], ref["Tw"], ref["Tm"] + (C / 2 + 7 + L + 1) * V32 * ref["Tw"]
    else:
        val, terms, e32 = ref["db"], ref["Tb"], L * V32 * ref["Tb"]
    e32 = torch.minimum(e32, (ref["rows"] + C + 8) * V32 * terms)  # never above one chain over the merged rows
    return U[dtype] * val.abs() * (1 + 2.0 ** -20) + e32 + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def outside_gx(gx, ref, dtype):
    """[n, T] bool: does the token's row hold an element outside the bound (or a non-finite one)?  And worst err / bound."""
    got = gx.detach().cpu().double().reshape(ref["gx"].shape)
    err, bnd = (got - ref["gx"]).abs(), bound_gx(ref, dtype)
    bad = ~torch.isfinite(got) | (err > bnd)
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
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
    line = f"merge_ln_bwd_oracle {label}: n {ref['n']} T {ref['T']} C {ref['gx'].shape[-1]} gx worst err/bound {worst:.3f}"
    fails = []
    if bool(bad.any()):
        fails.append(f"gx: {int(bad.sum())} token rows outside, first {torch.nonzero(bad)[0].tolist()}")
    for which, got in (("dw", dw), ("db", db)):
        if got is None:
            continue
        badp, worstp = outside_param(got, ref, which, dtype)
        line += f" {which} {worstp:.3f}"
        if bool(badp.any()):
            fails.append(f"{which}: {int(badp.sum())} channels outside, first {int(torch.nonzero(badp)[0])}")
    print(line)
    assert not fails, (label, fails)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_tensors(n, T, r, C, dtype, size_dtype, seed, with_mul=True, with_in=True, drop=False):
    """CPU tensors (gy, gx_out or None, xs, w, size or None) for a merge of [n, T, C] to [n, T - r, C]: the rows of
    ln_bwd_oracle.make_inputs, sizes 1..4 (exact in every dtype); drop: no sizes."""
    gy, xs, gi, w = bo.make_inputs((n, T - r, C), dtype, seed, with_in=with_in)
    gen = torch.Generator().manual_seed(seed + 1)
    size = None
    if not drop and with_mul:
        size = torch.randint(1, 5, (n, T, 1), generator=gen).to(size_dtype)
    return gy, gi, xs, w, size


def size_out_of(size, row_of, n, T, To, size_dtype):
    """size' [n, To, 1]: the sum of the sizes of the tokens of every merged row (ones without `size`), as the forward
    stores it (small integers: exact)."""
    s = torch.ones(n, T, dtype=torch.float64) if size is None else size.detach().cpu().double().reshape(n, T)
    out = torch.zeros(n, To, dtype=torch.float64)
    out.scatter_add_(1, row_of.clamp_min(0), torch.where(row_of >= 0, s, torch.zeros_like(s)))
    return out.to(size_dtype).reshape(n, To, 1)


def hand_plan(n, T, r, seed, class_token=False, distill=False, fan3=False):
    """A self-consistent even/odd matching made by hand on the CPU: (src_idx [n, r], dst_idx [n, r], unm_idx [n, U]).
    class_token: even token 0 is never a source; distill: odd token 0 never a destination.  fan3 (r >= 3): the first
    three sources of every group share one destination."""
    gen = torch.Generator().manual_seed(seed)
    T1, T2 = (T + 1) // 2, T // 2
    src, dst, unm = [], [], []
    for _ in range(n):
        cand = torch.arange(1 if class_token else 0, T1)
        pick = cand[torch.randperm(len(cand), generator=gen)[:r]]
        lo = 1 if distill else 0
        d = torch.randint(lo, T2, (r,), generator=gen)
        if fan3:
            d[:3] = d[0]
        rest = torch.tensor(sorted(set(range(T1)) - set(pick.tolist())), dtype=torch.long)
        src.append(pick)
        dst.append(d)
        unm.append(rest)
    return torch.stack(src), torch.stack(dst), torch.stack(unm)


def tie_row(ref_of, gx_out, xs, row, dtype):
    """Choose gx_out[0, row, :] (values of `dtype` in [1, 2)) channel by channel so that rounding gm to `dtype` BEFORE the
    scales lands the scaled value on a tie of the final rounding, as far as the grid of 16-bit values allows: per channel
    the candidate with the largest |chain - ref| / bound.  ref_of(gx_out) -> reference dict; token `tok` = the first
    token of group 0 that lands in `row` with a scale that is no power of two.  Returns (gx_out, tok)."""
    steps = 128 if dtype == torch.bfloat16 else 1024
    cands = (1.0 + torch.arange(steps, dtype=torch.float64) / steps).to(dtype)
    base = ref_of(gx_out)
    T = base["T"]
    tok = None
    for t in range(T):
        if base["row_of"][0, t] == row:
            s = float(base["scale"][0, t])
            if s > 0 and abs(torch.log2(torch.tensor(s)).item() % 1.0) > 1e-9:
                tok = t
                break
    assert tok is not None, "no token with a scale that is not a power of two lands in the row"
    best = torch.full((xs.shape[-1],), -1.0, dtype=torch.float64)
    choice = gx_out[0, row].clone()
    for c in cands:
        trial = gx_out.clone()
        trial[0, row, :] = c
        ref = ref_of(trial)
        chain = (ref["gm"][0, row].to(dtype).double() * ref["scale"][0, tok]).to(dtype).double()
        ratio = (chain - ref["gx"][0, tok]).abs() / bound_gx(ref, dtype)[0, tok]
        better = ratio > best
        best = torch.where(better, ratio, best)
        choice = torch.where(better, torch.full_like(choice, float(c)), choice)
    out = gx_out.clone()
    out[0, row, :] = choice
    return out, tok
