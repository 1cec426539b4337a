"""Accounting for the tanh-form GELU launches (tome_gelu_tanh, tome_gelu_tanh_backward; csrc/tome_gelu_bwd.h with
FORM = GELU_TANH): fp64 reference of the contract in include/tome_hip.h, derived acceptance bounds, an fp32 emulation of
the kernel's arithmetic with the slips such a kernel can make.  No test functions; importable without a GPU.  The launch
form, the bias-gradient bound and the inputs are the erf oracle's (tests/gelu_bwd_oracle.py) and are imported from it.
tests/test_gelu_tanh_oracle_cpu.py holds the bounds against the emulation on the CPU, tests/test_gelu_tanh_backward_gpu.py
applies them to the kernels.

Reference (exact arithmetic on the contract's constants, which are fp32 numbers: beta = fl32(0.7978845608028654),
kappa = fl32(0.044715))
---------
v = the stored 16-bit pre-activation, ga = the 16-bit gradient of the activation; both exact in fp64.
    u = beta (v + kappa v^3),  s = sigma(2u),  c = 1 - s = sigma(-2u)   (two sigmoids: neither cancels)
    p = 2 beta (1 + 3 kappa v^2),  w = v s c p,  d = s + w,  gh = ga d,  a = v s
    db1[c] = sum over rows of the STORED gh[:, c]

The kernel's evaluation (v32 = 2^-24, the fp32 unit roundoff; first order)
-----------------------
    u^: v*v, kappa*., .*v, v + ., beta*.            5 roundings, no cancellation (both terms have v's sign): 5 v32 |u|
    e^ = exp2(fl(-2 log2(e)) * |u^|)                the constant and the product add 2 v32 to the exponent's 5, and the
                                                    exponent's relative error is amplified by 2|u| on e: 14 |u| v32; the
                                                    hardware exp2 (v_exp_f32) is accurate to 1 ulp, <= 2 v32 relative:
                                                    eps_e = (14 |u| + 2) v32
    big = rcp(1 + e^), small = e^ * big             one addition and the hardware reciprocal (v_rcp_f32, 1 ulp: 2 v32) on
                                                    big, one more product on small: 3 and 4 v32, and e eps_e / (1 + e) on
                                                    big, eps_e / (1 + e) on small
    p^: 3 kappa (one constant), .*v^2 (v^2 has one), 1 + ., 2 beta * .       5 v32 |p|
(An evaluation with the math library's expf and two IEEE divisions would need less: 10 |u| + 2 and 2 / 2 v32.  The
kernel does not use them: with them the pass was bound by the vector ALU.)

Bound for gh (u_f = 2^-8 bf16 / 2^-11 fp16)
------------
    |gh - ref| <= |ga| (u_f |d| (1 + 2^-20) + 2^-22 (|s| + |w| + K)) [+ 2^-25 fp16],        K = 9/4
1. One rounding of the result to the format, taken on an fp32 value: u_f |ga d| (1 + 2^-20).
2. 2^-22 = 4 v32 relative to each of the two terms |s| and |w|: the sum s + w (|d| <= |s| + |w|), the product with ga,
   and two of the term's own roundings.
3. K, in units of 2^-22, collects what is not relative to the (possibly tiny) result:
   a. s beyond item 2: one more v32 on big (u >= 0), two more on small (u < 0), and the error of e -- the exp2 and the
      roundings of u amplified by 2|u| -- passed through the reciprocal: e eps_e / (1 + e) |s| for u >= 0,
      eps_e / (1 + e) |s| for u < 0; both equal eps_e s c:
          K_s(v) = (1/4 [u >= 0] + 1/2 [u < 0]) s + (3.5 |u| + 0.5) s c
   b. w beyond item 2: the third product (1), p (5), big and small in s c (7), and the error of e, which moves big and
      small in opposite directions: eps_e (1 - e) / (1 + e) = eps_e tanh|u|; (13 + (14 |u| + 2) tanh|u|) v32 |w|:
          K_w(v) = (3.25 + (3.5 |u| + 0.5) tanh|u|) |w|
   sup over v of K_s + K_w (`k_needed`, evaluated on a grid by the CPU test) = 2.14 <= K = 9/4.  This is a worst-case
   sum of absolute values; the fp32 emulation below uses a fraction of it (the issue's K = 1/2 was read off a CPU
   emulation with the library's exp and divisions: the derived figure is the one that holds for the kernel's operations).
   Where e is below fp32's normal range (|u| > 43.6; the hardware exp2 flushes there) s, c and w carry absolute errors
   of at most 2^-126 |v p| < 2^-68 for |v| <= 2^20, far below 2^-22 K.
4. fp16: results below 2^-14 are subnormal, spaced 2^-24: a correct rounding is off by up to 2^-25 whatever u_f says.

Bound for a  (the forward, and the activation the backward rebuilds -- which must in addition be BIT-equal to the
-----------   forward's)
    |a - ref| <= u_f |a| (1 + 2^-20) + v32 |a| (7 + 14 |u| [v < 0]) [+ 2^-25 fp16] + floor
v >= 0: s = big, (3 + e eps_e / (1 + e)) v32 <= 5.5 v32, and the product v s: 7 v32.  v < 0: s = small carries the whole
error of e, 4 + eps_e / (1 + e) <= (14 |u| + 6) v32, and the product: the allowance grows with |u| there -- that is the
price of having digits at all where 1 + tanh(u) has none.  floor = 2^-126 (1 + |v|) where s or |a| is below 2^-125: e, s
or the product are subnormal fp32 numbers there (the hardware exp2 flushes them to zero, and bf16's own spacing is 2^-133
whatever u_f says).

The framework's form 0.5 v (1 + tanh(u)) is given one rounding and 0.5 |v| 2^-23 for its cancellation (`bound_a_framework`).
"""
import math

import torch

from gelu_bwd_oracle import U, V32, bound_db, form, make_inputs, outside_db, rows_of_part  # noqa: F401

BETA = float(torch.tensor(0.7978845608028654, dtype=torch.float32))
KAPPA = float(torch.tensor(0.044715, dtype=torch.float32))
K_ABS = 2.25


def _rows64(t, Hd):
    return t.detach().to("cpu").double().reshape(-1, Hd)


def reference(h, ga=None):
    """fp64 reference; dict of float64 CPU tensors [rows, Hd]: gh, a, s, c, w, d, u, v, ga."""
    Hd = h.shape[-1]
    v = _rows64(h, Hd)
    g = torch.ones_like(v) if ga is None else _rows64(ga, Hd)
    u = BETA * (v + KAPPA * v ** 3)
    s, c = torch.sigmoid(2 * u), torch.sigmoid(-2 * u)
    w = v * s * c * (2 * BETA * (1 + 3 * KAPPA * v * v))
    d = s + w
    return {"gh": g * d, "a": v * s, "s": s, "c": c, "w": w, "d": d, "u": u, "v": v, "ga": g, "rows": v.shape[0],
            "Hd": Hd}


def k_needed(v):
    """K_s + K_w of the docstring at the fp64 values v."""
    ref = reference(v.reshape(1, -1))
    au = ref["u"].abs()
    ks = torch.where(ref["u"] >= 0, 0.25, 0.5) * ref["s"] + (3.5 * au + 0.5) * ref["s"] * ref["c"]
    kw = (3.25 + (3.5 * au + 0.5) * torch.tanh(au)) * ref["w"].abs()
    return ks + kw


def bound_gh(ref, dtype):
    return (ref["ga"].abs() * (U[dtype] * ref["d"].abs() * (1 + 2.0 ** -20)
                               + 2.0 ** -22 * (ref["s"].abs() + ref["w"].abs() + K_ABS))
            + (2.0 ** -25 if dtype == torch.float16 else 0.0))


def bound_a(ref, dtype):
    v, a, au = ref["v"], ref["a"].abs(), ref["u"].abs()
    fp32 = V32 * a * (7.0 + torch.where(v < 0, 14.0 * au, torch.zeros_like(au)))
    floor = torch.where((ref["s"] < 2.0 ** -125) | (a < 2.0 ** -125), 2.0 ** -126 * (1 + v.abs()), torch.zeros_like(v))
    return U[dtype] * a * (1 + 2.0 ** -20) + fp32 + floor + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def bound_a_framework(ref, dtype):
    """What 0.5 v (1 + tanh(u)) in fp32, rounded once, may differ from the reference by."""
    return (U[dtype] * ref["a"].abs() * (1 + 2.0 ** -20) + 0.5 * ref["v"].abs() * 2.0 ** -23
            + (2.0 ** -25 if dtype == torch.float16 else 0.0))


def _outside(got, want, bnd):
    err = (got - want).abs()
    bad = ~torch.isfinite(got) | (err > bnd)
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return bad, float(ratio.max())


def outside_gh(gh, ref, dtype):
    """[rows, Hd] bool: outside the bound (or non-finite); and the worst err / bound."""
    return _outside(_rows64(gh, ref["Hd"]), ref["gh"], bound_gh(ref, dtype))


def outside_a(a, ref, dtype):
    return _outside(_rows64(a, ref["Hd"]), ref["a"], bound_a(ref, dtype))


def check(label, gh, db, ref, dtype):
    """Assert the bounds on every element of gh and, where given, db1 (against the gh that was stored); prints the worst
    err / bound of each."""
    bad, worst = outside_gh(gh, ref, dtype)
    line = f"gelu_tanh_oracle {label}: rows {ref['rows']} Hd {ref['Hd']} gh worst err/bound {worst:.3f}"
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


def every_value(dtype):
    """Every finite fp16 value / every bf16 value with |v| <= 2^20 (the contract's range), padded with zeros to whole
    rows of 64: [rows, 64] of `dtype`."""
    bits = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(dtype)
    v = bits[torch.isfinite(bits.float()) & (bits.float().abs() <= 2.0 ** 20)]
    pad = (-v.numel()) % 64
    return torch.cat([v, torch.zeros(pad, dtype=dtype)]).reshape(-1, 64)


# ---------------------------------------------------------------------------------------------------------------------
# an fp32 emulation of the kernel's arithmetic (CPU)
# ---------------------------------------------------------------------------------------------------------------------
GH_SLIPS = ("erf", "kappa_once", "kappa_dropped", "no_ga", "neighbour_chunk")
DB_SLIPS = ("last_pass_dropped", "row_twice", "db_unrounded")


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def emulate_fp32(h, ga, slip=None):
    """The kernel's formula in fp32 on the CPU, one rounding to the format; db1 through per-workgroup fp32 partial rows.
    slip: None, or one of the wrong answers the CPU tests must see rejected -- GH_SLIPS ("erf": the exact-erf GELU's
    derivative and activation; "kappa_once" / "kappa_dropped": 1 + kappa v^2 / 1 in place of 1 + 3 kappa v^2), DB_SLIPS,
    "cancelling_act" (the framework's 0.5 v (1 + tanh u) for the activation).  Returns (gh, a, db1) in h's dtype."""
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
    beta, kappa = _f32(BETA), _f32(KAPPA)

    def sigmoids(x):
        x2 = x * x
        u = beta * (x + kappa * x2 * x)
        e = torch.exp2(_f32(-2.8853900817779268) * u.abs())
        big = 1.0 / (1.0 + e)
        small = e * big
        return torch.where(u >= 0, big, small), torch.where(u >= 0, small, big), x2, u

    s, c1, x2, _ = sigmoids(vg)
    k3 = {"kappa_once": kappa, "kappa_dropped": _f32(0.0)}.get(slip, _f32(3.0) * kappa)
    d = s + vg * (s * c1) * (2.0 * beta * (1.0 + k3 * x2))
    sa, _, _, ua = sigmoids(v)
    a32 = v * sa
    if slip == "erf":
        e1 = 1.0 + torch.erf(vg * _f32(0.70710678118654752440))
        d = 0.5 * e1 + vg * (torch.exp(-0.5 * (vg * vg)) * _f32(0.39894228040143267794))
        a32 = v * 0.5 * (1.0 + torch.erf(v * _f32(0.70710678118654752440)))
    if slip == "cancelling_act":
        a32 = 0.5 * v * (1.0 + torch.tanh(ua))
    gh32 = d if slip == "no_ga" else g * d
    gh = gh32.to(dtype)
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
    return gh.reshape(h.shape), a32.to(dtype).reshape(h.shape), pb.sum(0).to(dtype)


assert math.isclose(BETA, 0.7978845608028654, rel_tol=1e-7) and math.isclose(KAPPA, 0.044715, rel_tol=1e-7)
