"""Accounting for the MLP's native backward launch (tome_gelu_erf_backward, csrc/tome_gelu_bwd.h): fp64 reference,
acceptance bounds, inputs, an fp32 emulation of the kernel's arithmetic and a mirror of the launch form.  No test
functions; importable without a GPU.  tests/test_gelu_bwd_oracle_cpu.py shows on the CPU that the bounds accept the
emulation and reject the slips such a kernel can make; tests/test_mlp_backward_gpu.py applies them to the kernel.

Reference
---------
h: the stored 16-bit pre-activation, ga: the 16-bit gradient of the activation; both exact in fp64.  v = h,
    Phi(v) = 0.5 (1 + erf(v / sqrt 2)) = 0.5 erfc(-v / sqrt 2)   (the erfc form: no cancellation for v < 0)
    phi(v) = exp(-v^2 / 2) / sqrt(2 pi),   d = Phi(v) + v phi(v),   gh = ga d,   a = v Phi(v)
    db1[c] = sum over rows of the STORED gh[:, c]   (what fc1's weight-gradient GEMM reads)

Bound for gh (derived; u = 2^-8 bf16 / 2^-11 fp16, v32 = 2^-24 the fp32 unit roundoff)
------------
    |gh - ref| <= |ga| (u |d| (1 + 2^-20) + 2^-22 (|Phi| + |v phi| + K)) [+ 2^-25 fp16],   K = 1/2
1. One rounding of the result to the format, taken on an fp32 value: u |ga d| (1 + 2^-20).
2. The fp32 evaluation of the two terms, each on its own.  What is relative to a term: the product with 0.5, the sum of
   the two terms, the product with ga, the constant 1 / sqrt(2 pi) and the two products of v phi -- at most 4 v32 =
   2^-22 on |Phi| and on |v phi|.  What is NOT relative to the (possibly tiny) result goes into K, in units of 2^-22:
   a. Phi, v < 0: 1 + erf cancels.  erff near -1 has ulp 2^-24; the device erff is taken as accurate to 2 ulp (the
      figure the vendor math libraries publish for erff), the addition 1 + erf is then exact (Sterbenz), the product
      with 0.5 is exact: |Phi^ - Phi| <= 0.5 * 2 * 2^-24 = 2^-24 = 1/4 * 2^-22.  The rounding of the argument v / sqrt 2
      moves erf by at most max x erf'(x) v32 = 0.48 v32 -> 0.06 * 2^-22 on Phi.  For v > 0 the same absolute figures
      hold and the addition's rounding, 2^-24 on 1 + erf < 2, is relative to Phi >= 1/2.
   b. v phi: expf to 1 ulp and the rounding of v^2 (relative error v^2 / 2 * v32 on the exponential) beyond the 2^-22
      |v phi| of item 2: (1/2 + v^2 / 4) 2^-23 |v phi|, at most 0.12 * 2^-22 over all v (|v|^3 phi(v) <= 0.47).
   a + b <= 0.43 < K = 1/2.  (With erff to 1 ulp the sum is 0.31; the form this bound started from had K = 1/4.)
3. fp16: results below 2^-14 are subnormal, spaced 2^-24: a correct rounding is off by up to 2^-25 whatever u says.
The activation a is not bounded here: it must be BIT-equal to tome_gelu_erf(h), which the forward's tests hold to the
framework's kernel.

Bound for db1
-------------
ref = the fp64 sum of the stored gh column; T = the column's absolute sum.  One rounding of the parameter format,
u |ref| (1 + 2^-20) [+ 2^-25 fp16], plus the fp32 summation: a thread adds the U spw rows it owns of a column in one
chain, the RP rows-in-pass are combined through LDS in one chain, and the `parts` partial rows are added in some order
-- no term passes through more than L = U spw + RP + parts additions: L v32 T.  The terms themselves are exact in fp32
(16-bit values).  `form` mirrors csrc/tome_kernels.hip gelu_bwd_form.
"""
import math

import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
V32 = 2.0 ** -24
K_ABS = 0.5
MAX_PARTS = 512    # csrc/tome_kernels.hip: GELU_BWD_MAX_PARTS
MAX_WIDTH = 8192   # csrc/tome_kernels.hip: GELU_BWD_MAX_WIDTH
THREADS = 256


def _rows64(t, Hd):
    return t.detach().to("cpu").double().reshape(-1, Hd)


def reference(h, ga):
    """fp64 reference; dict of float64 CPU tensors [rows, Hd]: gh, a, Phi, vphi, d, ga."""
    Hd = h.shape[-1]
    v, g = _rows64(h, Hd), _rows64(ga, Hd)
    Phi = 0.5 * torch.special.erfc(-v / math.sqrt(2.0))
    vphi = v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)
    d = Phi + vphi
    return {"gh": g * d, "a": v * Phi, "Phi": Phi, "vphi": vphi, "d": d, "ga": g, "rows": v.shape[0], "Hd": Hd}


def bound_gh(ref, dtype):
    return (ref["ga"].abs() * (U[dtype] * ref["d"].abs() * (1 + 2.0 ** -20)
                               + 2.0 ** -22 * (ref["Phi"].abs() + ref["vphi"].abs() + K_ABS))
            + (2.0 ** -25 if dtype == torch.float16 else 0.0))


def outside_gh(gh, ref, dtype):
    """[rows, Hd] bool: outside the bound (or non-finite); and the worst err / bound."""
    got = _rows64(gh, ref["Hd"])
    err, bnd = (got - ref["gh"]).abs(), bound_gh(ref, dtype)
    bad = ~torch.isfinite(got) | (err > bnd)
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), (err > 0).double() * float("inf"))
    return bad, float(ratio.max())


def form(rows, Hd):
    """(S column slots per thread, U passes per step, RP rows per pass, spw steps per workgroup, parts) of the launch
    with the bias gradient, as csrc/tome_kernels.hip gelu_bwd_form picks them."""
    cpr = Hd // 8
    S = -(-cpr // THREADS)
    Up = 4 if S == 1 else (2 if S <= 3 else 1)
    RP = THREADS // cpr if S == 1 else 1
    steps = -(-(-(-rows // RP)) // Up)
    spw = -(-steps // MAX_PARTS)
    return S, Up, RP, spw, -(-steps // spw)


def forms_that_exist():
    """Every (S, rows-per-pass > 1) the packing can take: S = 1 with several rows per pass, S = 1 .. 4 with one."""
    return {(1, True), (1, False), (2, False), (3, False), (4, False)}


def rows_of_part(rows, Hd):
    """[rows] long: the workgroup (= partial row of the workspace) every row belongs to."""
    _, Up, RP, spw, _ = form(rows, Hd)
    return torch.arange(rows) // (Up * RP * spw)


def bound_db(gh_stored, dtype):
    """(ref, bound) [Hd] for db1 from the STORED gh [rows, Hd]."""
    Hd = gh_stored.shape[-1]
    g = _rows64(gh_stored, Hd)
    _, Up, RP, spw, parts = form(g.shape[0], Hd)
    L = Up * spw + RP + parts
    ref, T = g.sum(0), g.abs().sum(0)
    return ref, U[dtype] * ref.abs() * (1 + 2.0 ** -20) + L * V32 * T + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def outside_db(db, gh_stored, dtype):
    got = db.detach().cpu().double().reshape(-1)
    ref, bnd = bound_db(gh_stored, dtype)
    err = (got - ref).abs()
    return ~torch.isfinite(got) | (err > bnd), float((err / bnd.clamp_min(1e-300)).max())


def check(label, gh, db, ref, dtype):
    """Assert the bounds on every element of gh and, where given, db1 (against the gh that was stored); prints the worst
    err / bound of each."""
    bad, worst = outside_gh(gh, ref, dtype)
    line = f"gelu_bwd_oracle {label}: rows {ref['rows']} Hd {ref['Hd']} gh worst err/bound {worst:.3f}"
    fails = [] if not bool(bad.any()) else [f"gh: {int(bad.sum())} elements outside, first {torch.nonzero(bad)[0].tolist()}"]
    worst_db = 0.0
    if db is not None:
        badp, worst_db = outside_db(db, gh, dtype)
        line += f" db1 {worst_db:.3f}"
        if bool(badp.any()):
            fails.append(f"db1: {int(badp.sum())} columns outside, first {int(torch.nonzero(badp)[0])}")
    print(line)
    assert not fails, (label, fails)
    return worst, worst_db


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
SPECIAL_H = (0.0, -0.0, -0.7517915725708008, -0.75, 9.0, -9.0, 5.5, -5.5, -3.5, 1.0)


def make_inputs(rows, Hd, dtype, seed, grad_scale=1.0):
    """h ~ 3 N(0, 1) clamped to |v| <= 9, with +-0, the zero of the derivative near -0.75 and +-9 written over the first
    elements of every row that has room; ga = grad_scale * +-exp(N(0, 1) * 2.3) clamped to six orders of magnitude
    (1e-3 .. 1e3).  All finite.  CPU tensors of `dtype`."""
    gen = torch.Generator().manual_seed(seed)
    h = (3.0 * torch.randn(rows, Hd, generator=gen, dtype=torch.float64)).clamp_(-9.0, 9.0)
    n = min(len(SPECIAL_H), Hd)
    turn = (torch.arange(n)[None, :] + torch.arange(rows)[:, None] + seed) % n  # another order in every row
    h[:, :n] = torch.tensor(SPECIAL_H[:n], dtype=torch.float64)[turn]
    mag = torch.exp(2.3 * torch.randn(rows, Hd, generator=gen, dtype=torch.float64)).clamp_(1e-3, 1e3)
    sign = torch.where(torch.rand(rows, Hd, generator=gen) < 0.5, -1.0, 1.0).double()
    ga = grad_scale * sign * mag
    return h.to(dtype), ga.to(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# an fp32 emulation of the kernel's arithmetic (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def emulate_fp32(h, ga, slip=None):
    """The kernel's formula in fp32 on the CPU, one rounding to the format; db1 through per-workgroup fp32 partial rows.
    slip: None, or one of the wrong answers the CPU tests must see rejected: "no_vphi", "no_ga", "neighbour_chunk",
    "last_pass_dropped", "row_twice", "db_unrounded", "tanh_act".  Returns (gh, a, db1) in h's dtype."""
    dtype, Hd = h.dtype, h.shape[-1]
    v = h.detach().cpu().float().reshape(-1, Hd)
    g = ga.detach().cpu().float().reshape(-1, Hd)
    rows = v.shape[0]
    vg = v
    if slip == "neighbour_chunk":  # one 16-byte chunk of gh is computed from the neighbouring chunk's h
        vg = v.clone()
        c = (Hd // 8) // 2
        if Hd == 8:  # a row is one chunk: the neighbouring chunk is the next row
            vg = torch.roll(v, -1, 0)
        else:
            src = c + 1 if c + 1 < Hd // 8 else c - 1
            vg[:, 8 * c:8 * c + 8] = v[:, 8 * src:8 * src + 8]
    e1 = 1.0 + torch.erf(vg * torch.tensor(0.70710678118654752440, dtype=torch.float32))
    pdf = torch.exp(-0.5 * (vg * vg)) * torch.tensor(0.39894228040143267794, dtype=torch.float32)
    d = 0.5 * e1 + (0.0 if slip == "no_vphi" else vg * pdf)
    gh32 = d if slip == "no_ga" else g * d
    gh = gh32.to(dtype)
    if slip == "tanh_act":
        a = torch.nn.functional.gelu(v, approximate="tanh").to(dtype)
    else:
        a = (v * 0.5 * (1.0 + torch.erf(v * torch.tensor(0.70710678118654752440, dtype=torch.float32)))).to(dtype)
    terms = gh32 if slip == "db_unrounded" else gh.float()
    part = rows_of_part(rows, Hd)
    nparts = int(part.max()) + 1
    _, Up, RP, _, _ = form(rows, Hd)
    if slip == "last_pass_dropped":  # the rows of a partial last pass never reach the sums
        keep = torch.arange(rows) < (rows // RP) * RP if rows % RP else torch.arange(rows) < rows - RP
        terms = torch.where(keep[:, None], terms, torch.zeros_like(terms))
    pb = torch.zeros(nparts, Hd).index_add_(0, part, terms)
    if slip == "row_twice":
        pb[part[rows // 2]] += terms[rows // 2]
    return gh.reshape(h.shape), a.reshape(h.shape), pb.sum(0).to(dtype)
