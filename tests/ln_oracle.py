"""Exact accounting for the fused LayerNorm kernels (tome_add_layernorm*, tome_merge_wavg*_ln): reference, bound,
inputs and launch forms.  No test functions; importable without a GPU.  tests/test_ln_oracle_cpu.py shows on the CPU
that `check` accepts honest fp32 evaluations and rejects the slips a rows-per-wave packing can make;
tests/test_layernorm_accounting_gpu.py applies it to the kernels.

Reference
---------
`reference(x_stored, w, b, eps)`: LayerNorm in fp64, biased variance, of the rows as they are STORED in the 16-bit
format (include/tome_hip.h: "computed in fp32 from the stored x_out and rounded once").  With x_out_bias the stored row
is the x_out of the same call without the bias.  The 16-bit operands are exact in fp64 and fp64 carries 29 more bits
than fp32, so the reference's own error is far below every term that follows.

Bound
-----
`bound(...)` = u * |ref| + e32 per element.  u is the format's unit roundoff (2^-8 bf16, 2^-11 fp16): what one
correct rounding of the exact value costs.  e32 allows for an fp32 evaluation; it is derived here from the data of
the row, holds for any summation order, and knows nothing of the kernel.  Notation: v = 2^-24 (fp32 unit roundoff),
g(k) = k v / (1 - k v) (k roundings compounded), row x_1..x_C with exact mean mu, exact biased variance var,
s2 = var + eps, rho = s2^-1/2, d_i = x_i - mu, ref_i = d_i rho w_i + b_i.

1. mean.  m = fl(S^ * fl(1/C)) (or fl(S^ / C), which is smaller).  A hardware reciprocal is good to 1 ulp = 2 v, the
   product adds v.
   a. exact-sum rows: if every x_i is a multiple of a power of two G and sum|x_i| / G < 2^24, every partial sum in
      every order is a multiple of G below 2^24 G, hence an fp32 number: S^ = S.  |m - mu| <= dm = g(3) |mu|.
      `exact_sum_rows` decides this per row from the data.
   b. otherwise: C - 1 additions in any order, |S^ - S| <= g(C-1) sum|x_i|, so
      dm = g(C+2) sum|x_i| / C  (>= g(C-1) sum|x|/C compounded with g(3), since |mu| <= sum|x|/C).
   c. 1a is a statement about evaluations that SUM the row and scale the sum, as the kernels' contract says and as
      any reduction over lanes does.  An evaluation that updates a running mean (the framework's CPU LayerNorm:
      Welford steps m += (x - m) / k per vector lane, then pairwise combination of partial means) rounds a number of
      the size of mu at every step and gains nothing from the grid; it is checked with branch 1b on every row
      (`sums=False`), which covers those roundings as it covers the additions of a sum.
2. centred values.  d^_i = fl(x_i - m): |d^_i - d_i| <= ed_i = dm + v (|d_i| + dm).
3. variance.  Sum of C non-negative terms fl(d^_i^2) (one rounding each, none when fused), any order, C - 1
   additions, then * fl(1/C) as in 1: relative g(C+3) on the exact sum of the d^_i^2.  That sum differs from C var by
   at most sum(2 |d_i| ed_i + ed_i^2) =: C A.  One more addition for eps:
       |s2^ - s2| <= E2 = A + g(C+3) (var + A) + v (s2 + A + g(C+3) (var + A)).
4. rstd.  rho^ = rsq(s2^) to 1 ulp (or 1 / sqrt: two correct roundings, the same 2 v):
       |rho^ / rho - 1| <= Rr = (1 - E2 / s2)^-1/2 (1 + g(2)) - 1      (first order: E2 / (2 s2) + 2 v).
5. output.  Products d^ * rho^ * w in either association are two roundings, the addition of b (or the fma) a third:
       |p^ - p| <= Ep = |rho w_i| ((|d_i| + ed_i) (1 + Rr) (1 + g(2)) - |d_i|),   p = d_i rho w_i
       |y32 - ref| <= E = Ep + v (|ref| + Ep).
6. the one rounding to 16 bits acts on y32, not on ref: u |y32| <= u |ref| + u E; and fp16 results below 2^-14 are
   subnormal, spaced 2^-24, so a correct rounding may be off by 2^-25 there whatever u says (bf16 shares fp32's
   range: no such term).
       e32 = E (1 + u) + (2^-25 for fp16, 0 for bf16).

Condition on the inputs (`check(signature=True)`): at least 99 % of the rows take branch 1a, and on those rows
e32 <= u / 8 |ref| + 2^-14 on every element -- so the allowance cannot hide a slip: the smallest one listed below
moves an element by 0.125 standard deviations.  This is a property of the inputs, asserted, not measured.

Inputs
------
`signature_rows`: row k = M_k + s_k * round(z), z ~ N(0,1), (|M|, s) one of SIGNATURES, every value exactly
representable in bf16 and fp16 (asserted); two channels per row, chosen by the class, hold M + s and M - s, so that
no row of 8 channels comes out constant.  All M of one tensor share a sign; |M| >= 16 s, so a row spans at most two
binades and stays an exact-sum row also after the merge has averaged it with rows of its own class; any two of four
consecutive classes differ in |M| by at least 12 max(s), so that the MEASURED means of such rows (M plus the mean of
the grid noise, up to about 2.4 s off over thousands of rows of 8 channels) still differ by 8 max(s), which is what
`assert_rows_in_a_wave_differ` asserts on the tensors the kernels return.  A chunk left out of a row's mean moves the row by
8 |M| / C >= 0.125 s; a chunk normalised with a neighbouring row's statistics by at least 8 s.
`plain_rows`: N(0,1) times a per-row power of two 2^-6 .. 2^6: zero mean, no grid, branch 1b; they keep the elements
near zero and the scale invariance honest and are exempt from the 99 % condition.
"""
import numpy as np
import torch

WAVE = 64
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
V32 = 2.0 ** -24
# (|M|, s): means and grid steps of the eight row classes
SIGNATURES = ((24, 1), (40, 1), (64, 2), (88, 2), (136, 4), (184, 4), (280, 8), (376, 8))
ENTRIES = ("add_layernorm", "add_layernorm_skip_first", "add_layernorm_regrouped", "merge_wavg_ln",
           "merge_wavg_regrouped_ln")
WIDTHS = tuple(range(8, 1025, 8))


def _g(k):
    return k * V32 / (1.0 - k * V32)


# ---------------------------------------------------------------------------------------------------------------------
# reference and bound
# ---------------------------------------------------------------------------------------------------------------------
def _rows64(t):
    return t.detach().to("cpu").double().reshape(-1, t.shape[-1])


def reference(x_stored, w, b, eps):
    """fp64 LayerNorm (biased variance) of the stored rows; returns [rows, C] float64 on the CPU."""
    x = _rows64(x_stored)
    w64, b64 = w.detach().cpu().double(), b.detach().cpu().double()
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).mean(-1, keepdim=True)
    return d / torch.sqrt(var + eps) * w64 + b64


def exact_sum_rows(x_stored):
    """Per row: are all elements multiples of one power of two G with sum|x| / G < 2^24 (branch 1a)?"""
    x = _rows64(x_stored).numpy()
    bits = np.ascontiguousarray(x).view(np.int64)
    expo = (bits >> 52) & 0x7FF
    mant = (bits & ((1 << 52) - 1)) | (1 << 52)  # 16-bit values are normal doubles (or zero)
    low = mant & -mant
    lowbit = expo - 1075 + np.log2(low.astype(np.float64)).astype(np.int64)  # exponent of the lowest set bit
    lowbit = np.where(x == 0.0, 4096, lowbit)
    gexp = lowbit.min(axis=1)
    allzero = gexp == 4096
    gexp = np.where(allzero, 0, gexp)
    ok = np.abs(x).sum(axis=1) / np.exp2(gexp.astype(np.float64)) < 2.0 ** 24
    return torch.from_numpy(ok | allzero)


def bound(x_stored, w, b, eps, dtype, return_parts=False, sums=True):
    """u * |ref| + e32 per element (module docstring, steps 1-6); [rows, C] float64.  sums=False: the evaluation's
    mean is not a sum that is scaled afterwards (see 1c): every row takes branch 1b."""
    u = U[dtype]
    x = _rows64(x_stored)
    C = x.shape[-1]
    w64, b64 = w.detach().cpu().double(), b.detach().cpu().double()
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).mean(-1, keepdim=True)
    s2 = var + eps
    rho = s2 ** -0.5
    ref = d * rho * w64 + b64
    exact = exact_sum_rows(x_stored) if sums else torch.zeros(x.shape[0], dtype=torch.bool)
    sabs = x.abs().sum(-1, keepdim=True)
    dm = torch.where(exact[:, None], _g(3) * mu.abs(), _g(C + 2) * sabs / C)                    # 1
    ed = dm + V32 * (d.abs() + dm)                                                                # 2
    A = (2 * d.abs() * ed + ed * ed).sum(-1, keepdim=True) / C                                    # 3
    E2 = A + _g(C + 3) * (var + A) + V32 * (s2 + A + _g(C + 3) * (var + A))
    q = E2 / s2                                                                                   # 4
    Rr = torch.where(q < 0.5, (1.0 - q.clamp(max=0.5)) ** -0.5 * (1.0 + _g(2)) - 1.0, torch.full_like(q, float("inf")))
    Ep = (rho * w64).abs() * ((d.abs() + ed) * (1.0 + Rr) * (1.0 + _g(2)) - d.abs())              # 5
    E = Ep + V32 * (ref.abs() + Ep)
    e32 = E * (1.0 + u) + (2.0 ** -25 if dtype == torch.float16 else 0.0)                         # 6
    total = u * ref.abs() + e32
    if return_parts:
        return total, ref, e32, exact
    return total


def check(y, x_stored, w, b, eps, dtype=None, R=1, out_index=None, label="", signature=True, rows=None, sums=True):
    """Assert |y - ref| <= bound on every element.  Prints the worst err / bound and the share of exact-sum rows.
    A failure names (row, 16-byte chunk column, lane slot it, row-in-wave rr) of the first bad element: R rows of
    cpr = C / 8 chunks are laid over the lanes of a wave, chunk q = rr * cpr + column sits in lane q % 64, slot q // 64.
    out_index: position of every row in its group's output order (default: the flat row number), rr = out_index % R.
    rows: optional boolean mask, only these rows are compared (and counted for the 99 % condition).
    signature=True also asserts the condition on the inputs (module docstring)."""
    dtype = dtype or y.dtype
    u = U[dtype]
    total, ref, e32, exact = bound(x_stored, w, b, eps, dtype, return_parts=True, sums=sums)
    got = _rows64(y)
    assert got.shape == ref.shape, (label, tuple(got.shape), tuple(ref.shape))
    nrows, C = ref.shape
    idx = torch.arange(nrows) if out_index is None else out_index.reshape(-1).cpu().long()
    sel = torch.ones(nrows, dtype=torch.bool) if rows is None else rows.reshape(-1).cpu().bool()
    assert int(sel.sum()) > 0, f"{label}: no rows to compare"
    err = (got - ref).abs()
    ratio = torch.where(sel[:, None], err / total, torch.zeros_like(err))
    share = float(exact[sel].double().mean())
    worst = float(ratio.max())
    print(f"ln_oracle {label}: rows {int(sel.sum())} C {C} worst err/bound {worst:.3f} exact-sum rows {100 * share:.1f} %")
    if signature:
        assert share >= 0.99, f"{label}: only {100 * share:.1f} % of the rows are exact-sum rows"
        tight = (e32 <= u / 8 * ref.abs() + 2.0 ** -14) | ~(exact & sel)[:, None]
        if not bool(tight.all()):
            rw, ch = [int(v) for v in torch.nonzero(~tight)[0]]
            raise AssertionError(f"{label}: e32 {float(e32[rw, ch]):.3e} above u/8 |ref| + 2^-14 at row {rw} channel "
                                 f"{ch} (|ref| {abs(float(ref[rw, ch])):.3e})")
    bad = (~torch.isfinite(got) | (err > total)) & sel[:, None]
    if bool(bad.any()):
        rw, ch = [int(v) for v in torch.nonzero(bad)[0]]
        cpr, rr = C // 8, int(idx[rw]) % R
        col = ch // 8
        it = (rr * cpr + col) // WAVE
        raise AssertionError(
            f"{label}: {int(bad.sum())} elements in {int(bad.any(-1).sum())} rows outside the bound; first at row {rw} "
            f"(output row {int(idx[rw])}) channel {ch}: chunk column {col}, lane slot it={it}, lane "
            f"{(rr * cpr + col) % WAVE}, row-in-wave rr={rr} of R={R}; got {float(got[rw, ch])!r} ref "
            f"{float(ref[rw, ch])!r} err {float(err[rw, ch]):.3e} bound {float(total[rw, ch]):.3e}")
    return {"worst": worst, "exact_share": share}


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _representable(t64, dtype):
    return bool(torch.equal(t64.to(dtype).double(), t64))


def signature_rows(shape, dtype, seed, sign=1, klass=None, noise_scale=1.0, offset=True):
    """Rows M_k + s_k * round(noise_scale * z); klass [*shape[:-1]] picks the class of every row (default: flat row
    number mod 8).  offset=False gives only the grid noise s_k * round(.) (an addend for such rows).  Asserts that
    every value is representable in bf16 and in fp16."""
    assert sign in (1, -1)
    lead, C = tuple(shape[:-1]), shape[-1]
    nrows = int(np.prod(lead)) if lead else 1
    k = (torch.arange(nrows) % len(SIGNATURES)) if klass is None else klass.reshape(-1).cpu().long() % len(SIGNATURES)
    sig = torch.tensor(SIGNATURES, dtype=torch.float64)
    M, s = sig[k, 0:1] * sign, sig[k, 1:2]
    z = torch.randn((nrows, C), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    noise = torch.round(noise_scale * z)
    # two channels of every row are fixed, by its class: +1 and -1 steps in the rows, 0 in an addend -- no row is
    # constant (a constant row has rstd = eps^-1/2 and fails the condition on the inputs), also after the merge has
    # averaged rows of one class
    at = torch.arange(nrows)
    noise[at, k % C] = 1.0 if offset else 0.0
    noise[at, (k + C // 2) % C] = -1.0 if offset else 0.0
    rows = s * noise + (M if offset else 0.0)
    for fmt in (torch.bfloat16, torch.float16):
        assert _representable(rows, fmt), f"signature rows not representable in {fmt}"
    return rows.to(dtype).reshape(*lead, C)


def row_class(x_stored):
    """The class 0..7 whose |M| is nearest to the row's mean (fp64), and the sign of the mean; [rows] each."""
    mu = _rows64(x_stored).mean(-1)
    Ms = torch.tensor([m for m, _ in SIGNATURES], dtype=torch.float64)
    return (mu.abs()[:, None] - Ms[None, :]).abs().argmin(-1), torch.sign(mu)


def assert_rows_in_a_wave_differ(x_stored, group_rows, label=""):
    """Any two of four consecutive rows of one group (rows that can share a wave) differ in their mean by at least
    8 * max(s) of the two rows' classes.  x_stored [groups * group_rows, C] in output order."""
    mu = _rows64(x_stored).mean(-1).reshape(-1, group_rows)
    k, _ = row_class(x_stored)
    s = torch.tensor([sv for _, sv in SIGNATURES], dtype=torch.float64)[k].reshape(-1, group_rows)
    for off in (1, 2, 3):
        if group_rows <= off:
            break
        gap = (mu[:, off:] - mu[:, :-off]).abs()
        need = 8.0 * torch.maximum(s[:, off:], s[:, :-off])
        assert bool((gap >= need).all()), f"{label}: rows {off} apart have means closer than 8 s"


def plain_rows(shape, dtype, seed):
    """N(0,1) rows times a per-row power of two 2^-6 .. 2^6."""
    lead, C = tuple(shape[:-1]), shape[-1]
    nrows = int(np.prod(lead)) if lead else 1
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn((nrows, C), generator=gen, dtype=torch.float64)
    e = torch.randint(-6, 7, (nrows, 1), generator=gen).double()
    return (z * torch.exp2(e)).to(dtype).reshape(*lead, C)


def affine(C, dtype, seed):
    """LayerNorm weight 1 + 0.1 N(0,1) and bias 0.1 N(0,1), distinct in every channel."""
    gen = torch.Generator().manual_seed(seed)
    w = (1.0 + 0.1 * torch.randn(C, generator=gen, dtype=torch.float64)).to(dtype)
    b = (0.1 * torch.randn(C, generator=gen, dtype=torch.float64)).to(dtype)
    return w, b


def merged_row_of_token(src_idx, dst_idx, unm_idx, T):
    """Output row of every input token of a bipartite merge without distillation token ([unmerged even tokens, odd
    tokens] per group), from the plan's index tensors [n, r, 1] / [n, T1 - r, 1]; returns ([n, T] rows, [n, T - r]
    mask of the output rows that receive sources)."""
    src, dst, unm = (t.cpu().long().reshape(t.shape[0], -1) for t in (src_idx, dst_idx, unm_idx))
    n, r = src.shape
    Uu = unm.shape[1]
    row = torch.full((n, T), -1, dtype=torch.long)
    g = torch.arange(n)[:, None]
    row[:, 1::2] = Uu + torch.arange(T // 2)[None, :]
    row[g, 2 * unm] = torch.arange(Uu)[None, :].expand(n, Uu)
    row[g, 2 * src] = Uu + dst
    assert int(row.min()) >= 0
    recv = torch.zeros((n, T - r), dtype=torch.bool)
    recv[g, Uu + dst] = True
    return row, recv


# ---------------------------------------------------------------------------------------------------------------------
# launch forms
# ---------------------------------------------------------------------------------------------------------------------
def expected_form(entry, C, addend=False, T=0, r=0):
    """(NIT, R, EAGER) the dispatcher picks (csrc/tome_kernels.hip: launch_merge_rows, add_layernorm_impl,
    tome_add_layernorm_regrouped): NIT 16-byte chunks per lane, R rows per wave, EAGER streaming waves."""
    assert entry in ENTRIES and C % 8 == 0 and 8 <= C <= 1024
    cpr = C // 8
    if entry.startswith("add_layernorm"):
        nit, eager = 3, False  # (cpr <= 128 <= 3 * 64: the six-chunk form of k_add_ln_rows is out of reach)
    else:
        nit = 3 if (addend and cpr <= 3 * WAVE) else 6
        eager = r <= 64 and 8 * r >= T
    return nit, min(4, nit * WAVE // cpr), eager


def boundary_inside_iteration(C, R):
    """Does some row of the wave start in the middle of a lane iteration (rr * cpr not a multiple of 64)?  None when
    the wave holds a single row."""
    cpr = C // 8
    if R < 2:
        return None
    return any((rr * cpr) % WAVE for rr in range(1, R))


def forms_that_exist(entry):
    """Every (NIT, R) the dispatcher can produce for `entry` over the legal widths, both addend settings."""
    return {expected_form(entry, C, addend)[:2] for C in WIDTHS for addend in (False, True)}
