"""tests/ln_regrouped_bwd_oracle.py on the CPU: the row map agrees with autograd of the reference's op sequence, the
bound accepts the fp32 emulation and rejects the slips a regrouped LayerNorm backward can make."""
import pytest
import torch

import ln_regrouped_bwd_oracle as ro

DTYPES = [torch.bfloat16, torch.float16]
EPS = 1e-5


def test_reference_is_autograd_of_the_reference_ops():
    """x1 = cat(cls, x[:, 1:] + rt); xs = cat(cls per frame, 'b (p t) m -> (b t) p m'); y = norm1(xs) in fp64."""
    B, F, P, C = 2, 3, 5, 16
    gy, xs, gi, w = ro.make_inputs(B, F, P, C, torch.bfloat16, 3, far=False)
    x1 = xs.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    cls0, xt = x1[:, :1], x1[:, 1:]
    xs_in = torch.cat((cls0.expand(B, F, C).reshape(B * F, 1, C),
                       xt.reshape(B, P, F, C).transpose(1, 2).reshape(B * F, P, C)), 1)
    y = torch.nn.functional.layer_norm(xs_in, (C,), w64, b64, EPS)
    torch.autograd.backward((y, x1), (gy.double(), gi.double()))
    ref = ro.reference(gy, xs, gi, w, EPS, F)
    assert torch.allclose(ref["gx"].reshape(B, -1, C), x1.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(ref["dw"], w64.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(ref["db"], b64.grad, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_fp32_emulation_is_inside_the_bound(dtype):
    for (B, F, P, C) in ((2, 3, 5, 64), (1, 1, 3, 8), (3, 8, 14, 768), (2, 2, 49, 1024), (4, 8, 128, 64)):
        for with_in in (False, True):
            gy, xs, gi, w = ro.make_inputs(B, F, P, C, dtype, B * 1000 + F * 100 + P + with_in, with_in=with_in)
            ref = ro.reference(gy, xs, gi, w, EPS, F)
            gx, dw, db = ro.emulate_fp32(gy, xs, gi, w, EPS, F)
            ro.check(f"{(B, F, P, C)} gx_in={with_in} {dtype}", gx, dw, db, ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("slip", ro.SLIPS)
def test_slips_are_outside_the_bound(slip, dtype):
    """Many clips of few tokens (the class rows are one row in 17, so their share of dbias shows), F = 8, no gx_in
    (a class row's gx is then the LayerNorm term alone, and a rounding per frame of its gradient is not hidden behind
    the rounding of a larger sum)."""
    B, F, P, C = 16, 8, 2, 64
    gy, xs, gi, w = ro.make_inputs(B, F, P, C, dtype, 77, with_in=False)
    ref = ro.reference(gy, xs, gi, w, EPS, F)
    gx, dw, db = ro.emulate_fp32(gy, xs, gi, w, EPS, F, slip=slip)
    bad_rows, worst = ro.outside_gx(gx, ref, dtype)
    bad_db, worst_db = ro.outside_param(db, ref, "db", dtype)
    cls = torch.zeros(B * (1 + P * F), dtype=torch.bool)
    cls[:: 1 + P * F] = True
    print(slip, dtype, "gx rows outside", int(bad_rows.sum()), "worst", worst, "db channels outside", int(bad_db.sum()))
    if slip == "cls_counted_per_frame":
        assert not bad_rows.any() and bad_db.any()
    elif slip in ("cls_frame0", "cls_rounded_per_frame"):
        assert bad_rows[cls].any() and not bad_rows[~cls].any()
    else:
        assert bad_rows[~cls].any()
