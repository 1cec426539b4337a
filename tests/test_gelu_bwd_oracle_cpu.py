"""The acceptance bounds of tests/gelu_bwd_oracle.py on the CPU: an fp32 evaluation of the kernel's arithmetic lies inside
them in both formats, and each wrong answer such a kernel can give falls outside.  No GPU, no library."""
import math

import pytest
import torch

import gelu_bwd_oracle as go

DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(37, 64), (111, 200), (5, 2056), (300, 8)]


def _sweep(dtype, rows=64, Hd=512):
    """h swept over [-9, 9], log-normal ga."""
    gen = torch.Generator().manual_seed(5)
    h = torch.linspace(-9.0, 9.0, rows * Hd, dtype=torch.float64).reshape(rows, Hd)
    ga = torch.exp(2.0 * torch.randn(rows, Hd, generator=gen, dtype=torch.float64))
    return h.to(dtype), ga.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_the_fp32_emulation_lies_inside_the_bounds(dtype):
    cases = [go.make_inputs(r, Hd, dtype, 11 * r + Hd, grad_scale=1e-3 if i % 3 == 2 else 1.0)
             for i, (r, Hd) in enumerate(SHAPES)] + [_sweep(dtype)]
    for h, ga in cases:
        assert torch.isfinite(h.float()).all() and torch.isfinite(ga.float()).all()
        ref = go.reference(h, ga)
        gh, a, db = go.emulate_fp32(h, ga)
        worst, worst_db = go.check(f"emulation {tuple(h.shape)} {dtype}", gh, db, ref, dtype)
        assert worst <= 1.0 and worst_db <= 1.0
        # the activation of the emulation is the exact-erf GELU to one rounding of the format
        err = (a.double().reshape(ref["a"].shape) - ref["a"]).abs()
        assert bool((err <= go.U[dtype] * ref["a"].abs() * (1 + 2.0 ** -20) + 2.0 ** -22 * h.double().abs().reshape(err.shape)
                     + 2.0 ** -25).all())


def test_reference_is_the_derivative_of_the_exact_gelu():
    h = torch.linspace(-9, 9, 4001, dtype=torch.float64).reshape(1, -1)[:, :4000].requires_grad_()
    torch.nn.functional.gelu(h).sum().backward()
    ref = go.reference(h.detach(), torch.ones_like(h))
    assert float((ref["gh"] - h.grad).abs().max()) < 1e-14
    assert float((ref["a"] - torch.nn.functional.gelu(h.detach())).abs().max()) < 1e-14
    z = torch.tensor([[go.SPECIAL_H[2]] * 8], dtype=torch.float64)
    assert abs(float(go.reference(z, torch.ones_like(z))["d"][0, 0])) < 1e-6  # the zero of the derivative


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("slip", ["no_vphi", "no_ga", "neighbour_chunk"])
def test_wrong_gradients_fall_outside(dtype, slip):
    for r, Hd in SHAPES:
        h, ga = go.make_inputs(r, Hd, dtype, 3 * r + Hd)
        ref = go.reference(h, ga)
        gh, _, _ = go.emulate_fp32(h, ga, slip=slip)
        bad, _ = go.outside_gh(gh, ref, dtype)
        share = float(bad.double().mean())
        print(f"{slip} {(r, Hd)} {dtype}: {100 * share:.1f} % of the elements outside")
        if slip == "neighbour_chunk":
            assert bool(bad.any()) and bool(bad[:, 8 * ((Hd // 8) // 2):8 * ((Hd // 8) // 2) + 8].any())
        else:
            assert share > 0.25, (slip, r, Hd, share)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("slip", ["last_pass_dropped", "row_twice", "db_unrounded"])
def test_wrong_bias_gradients_fall_outside(dtype, slip):
    """db1 is judged against the gh that was stored.  A dropped partial last pass and a row counted twice move a column
    by whole terms: outside wherever those are not small against the column's sum (log-normal ga: not in every column).  Sums of the UNROUNDED values differ from the sums of the stored ones by the accumulated
    roundings, about u rms sqrt(rows) / 3.5 per column, against an allowance of u |sum| + L v32 T: outside wherever the
    column's sum is small against its terms -- shown at 1031 rows, where a share of the columns always is."""
    shapes = [(1031, 64), (1031, 200)] if slip == "db_unrounded" else [(37, 64), (111, 200), (5, 2056), (301, 8)]
    for r, Hd in shapes:
        h, ga = go.make_inputs(r, Hd, dtype, 3 * r + Hd)
        gh, _, db = go.emulate_fp32(h, ga, slip=slip)
        good = go.emulate_fp32(h, ga)[2]
        assert not bool(go.outside_db(good, gh, dtype)[0].any())
        bad, worst = go.outside_db(db, gh, dtype)
        print(f"{slip} {(r, Hd)} {dtype}: {int(bad.sum())} of {Hd} columns outside, worst {worst:.2f}")
        assert bool(bad.any()), (slip, r, Hd)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_tanh_form_activation_is_not_the_forwards_bits(dtype):
    h, ga = go.make_inputs(111, 200, dtype, 4)
    want = go.emulate_fp32(h, ga)[1]
    got = go.emulate_fp32(h, ga, slip="tanh_act")[1]
    assert not torch.equal(got, want)
    assert float((got != want).double().mean()) > 0.05


def test_form_mirror():
    """The packing at the widths around every change of form; parts never above the limit; every row has a part."""
    seen = set()
    for Hd in (8, 16, 64, 200, 2040, 2048, 2056, 3072, 4096, 4104, 6144, 6152, 8192):
        for rows in (1, 2, 5, 37, 111, 1031, 16489, 100352):
            S, Up, RP, spw, parts = go.form(rows, Hd)
            cpr = Hd // 8
            assert S * go.THREADS >= cpr and (S - 1) * go.THREADS < cpr and 1 <= parts <= go.MAX_PARTS
            assert (RP == 1 and Up * S >= 4) if S > 1 else (RP * cpr <= go.THREADS < (RP + 1) * cpr and Up == 4)
            assert parts * spw * Up * RP >= rows > (parts - 1) * spw * Up * RP
            part = go.rows_of_part(rows, Hd)
            assert int(part.max()) == parts - 1
            seen.add((S, RP > 1))
    assert seen == go.forms_that_exist()
    assert math.isclose(go.K_ABS, 0.5)
