"""The acceptance bounds of tests/gelu_tanh_oracle.py on the CPU: an fp32 evaluation of the kernel's arithmetic lies
inside them in both formats, at every launch form and on every value of the contract's range, and each wrong answer such
a kernel can give falls outside -- by the bound, never by a special case.  No GPU, no library."""
import pytest
import torch

import gelu_bwd_oracle as erf_oracle
import gelu_tanh_oracle as go

DTYPES = [torch.bfloat16, torch.float16]
# one shape per launch form: (S, several rows per pass)
FORM_SHAPES = {(1, True): (37, 64), (1, False): (5, 2040), (2, False): (5, 2056), (3, False): (3, 4104), (4, False): (2, 8192)}
SHAPES = [(37, 64), (111, 200), (5, 2056), (300, 8)]


def test_k_is_the_derived_one():
    """sup over v of K_s + K_w (the docstring's worst-case sum) on a fine grid, the 16-bit values included."""
    v = torch.cat([torch.linspace(-12.0, 12.0, 240001, dtype=torch.float64),
                   go.every_value(torch.float16).double().reshape(-1), go.every_value(torch.bfloat16).double().reshape(-1)])
    need = go.k_needed(v)
    top = float(need.max())
    print(f"sup K_s + K_w = {top:.3f} at v = {float(v[need.reshape(-1).argmax()]):.3f}; K = {go.K_ABS}")
    assert go.K_ABS - 0.25 < top <= go.K_ABS  # (the next quarter above the supremum)


def test_reference_is_the_derivative_of_the_tanh_gelu():
    h = torch.linspace(-9, 9, 4001, dtype=torch.float64).reshape(1, -1)[:, :4000].requires_grad_()
    torch.nn.functional.gelu(h, approximate="tanh").sum().backward()
    ref = go.reference(h.detach())
    # (the framework's constant is sqrt(2 / pi) in fp64, the contract's its fp32 rounding: 3e-8 relative on u)
    assert float((ref["gh"] - h.grad).abs().max()) < 2e-7
    assert float((ref["a"] - torch.nn.functional.gelu(h.detach(), approximate="tanh")).abs().max()) < 2e-7
    assert float((ref["s"] + ref["c"] - 1).abs().max()) < 1e-15
    # no cancellation on the negative side: s keeps its relative accuracy where 1 + tanh(u) has lost it
    far = go.reference(torch.tensor([[-9.0] * 8], dtype=torch.float64))
    assert 0 < float(far["s"][0, 0]) < 1e-28 and float(far["a"][0, 0]) < 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_the_fp32_emulation_lies_inside_the_bounds_at_every_form(dtype):
    assert set(FORM_SHAPES) == erf_oracle.forms_that_exist()
    cases = list(FORM_SHAPES.items()) + [(None, s) for s in SHAPES]
    for i, (want_form, (r, Hd)) in enumerate(cases):
        if want_form is not None:
            S, _, RP, _, _ = go.form(r, Hd)
            assert (S, RP > 1) == want_form
        h, ga = go.make_inputs(r, Hd, dtype, 11 * r + Hd, grad_scale=1e-3 if i % 3 == 2 else 1.0)
        ref = go.reference(h, ga)
        gh, a, db = go.emulate_fp32(h, ga)
        worst, worst_db = go.check(f"emulation {tuple(h.shape)} {dtype}", gh, db, ref, dtype)
        assert worst <= 1.0 and worst_db <= 1.0
        bad, worst_a = go.outside_a(a, ref, dtype)
        assert not bool(bad.any()), (r, Hd, worst_a)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_the_fp32_emulation_lies_inside_the_bounds_on_every_value(dtype):
    """Every finite fp16 value, every bf16 value with |v| <= 2^20; ga = 1 and ga = -1e3.  Everything finite."""
    h = go.every_value(dtype)
    for scale in (1.0, -1e3):
        ga = torch.full_like(h, scale)
        ref = go.reference(h, ga)
        gh, a, _ = go.emulate_fp32(h, ga)
        assert torch.isfinite(gh.float()).all() and torch.isfinite(a.float()).all()
        bad, worst = go.outside_gh(gh, ref, dtype)
        bad_a, worst_a = go.outside_a(a, ref, dtype)
        print(f"every value {dtype} ga {scale}: gh worst err/bound {worst:.3f}, a {worst_a:.3f}")
        assert not bool(bad.any()) and not bool(bad_a.any())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("slip", go.GH_SLIPS)
def test_wrong_gradients_fall_outside(dtype, slip):
    for r, Hd in SHAPES:
        h, ga = go.make_inputs(r, Hd, dtype, 3 * r + Hd)
        ref = go.reference(h, ga)
        gh, a, _ = go.emulate_fp32(h, ga, slip=slip)
        bad, _ = go.outside_gh(gh, ref, dtype)
        share = float(bad.double().mean())
        print(f"{slip} {(r, Hd)} {dtype}: {100 * share:.1f} % of the elements outside")
        # Hd = 8: the rows are the first eight special values, and the zero of the derivative and -0.75 are the two of
        # them at which the form or the factor 1 + 3 kappa v^2 matters (0, +-9 and +-5.5 are saturated): a quarter
        floor_share = 0.25 if Hd == 8 else 0.3
        if slip == "neighbour_chunk":
            assert bool(bad.any()) and bool(bad[:, 8 * ((Hd // 8) // 2):8 * ((Hd // 8) // 2) + 8].any())
        elif slip == "erf":
            # the two forms differ by tens of percent at v in [-5.5, -3], which make_inputs writes into every row
            # that has room (SPECIAL_H: -3.5, -5.5 need 9 columns)
            v = ref["v"]
            there = (v == -3.5) | (v == -5.5)
            rel = ((go.reference(h, ga)["d"] - erf_oracle.reference(h, ga)["d"]).abs() / ref["d"].abs())[there]
            if Hd >= 9:
                assert bool(there.any()) and float(rel.min()) > 0.1, float(rel.min())
                # (at -5.5 both derivatives are below 1e-6: tens of percent of that is inside the fp32 allowance)
                assert bool(bad[v == -3.5].all()), "the erf derivative passes at v = -3.5"
            assert share >= floor_share, (slip, r, Hd, share)
            # ... and so does its activation, where the two differ by more than a rounding of the format: 30 % at -3.5
            bad_a = go.outside_a(a, ref, dtype)[0]
            assert bool(bad_a.any()) and (Hd < 9 or bool(bad_a[v == -3.5].all()))
        else:
            assert share >= floor_share, (slip, r, Hd, share)

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_the_cancelling_activation_falls_outside_below_minus_five(dtype):
    """0.5 v (1 + tanh u) in fp32: 1 + tanh(u) is a multiple of 2^-24 -- tens of percent off at v = -5, nothing left
    below -5.6.  bf16 has the exponent range to see all of it; fp16 sees it where the activation is still above its
    subnormal spacing (2^-24), just below -5."""
    bits = go.every_value(dtype).reshape(-1)
    lo = -9.0 if dtype == torch.bfloat16 else -5.25
    v = bits[(bits.float() <= -5.0) & (bits.float() >= lo)]
    v = torch.cat([v, v[-1:].expand((-v.numel()) % 8)]).reshape(-1, 8)
    ref = go.reference(v)
    good = go.emulate_fp32(v, torch.ones_like(v))[1]
    assert not bool(go.outside_a(good, ref, dtype)[0].any())
    got = go.emulate_fp32(v, torch.ones_like(v), slip="cancelling_act")[1]
    bad, worst = go.outside_a(got, ref, dtype)
    share = float(bad.double().mean())
    print(f"cancelling activation {dtype}: {100 * share:.1f} % of {v.numel()} values in [{lo}, -5] outside, worst {worst:.1f}")
    assert share > (0.9 if dtype == torch.bfloat16 else 0.5)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("slip", go.DB_SLIPS)
def test_wrong_bias_gradients_fall_outside(dtype, slip):
    """As in the erf oracle: db1 is judged against the gh that was stored."""
    shapes = [(1031, 64), (1031, 200)] if slip == "db_unrounded" else [(37, 64), (111, 200), (5, 2056), (301, 8)]
    for r, Hd in shapes:
        h, ga = go.make_inputs(r, Hd, dtype, 3 * r + Hd)
        gh, _, db = go.emulate_fp32(h, ga, slip=slip)
        good = go.emulate_fp32(h, ga)[2]
        assert not bool(go.outside_db(good, gh, dtype)[0].any())
        bad, worst = go.outside_db(db, gh, dtype)
        print(f"{slip} {(r, Hd)} {dtype}: {int(bad.sum())} of {Hd} columns outside, worst {worst:.2f}")
        assert bool(bad.any()), (slip, r, Hd)
