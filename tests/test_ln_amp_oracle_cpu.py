"""tests/ln_amp_oracle.py on the CPU: the bounds accept an honest fp32 evaluation of the mixed-precision add + LayerNorm
and of its backward in every legal type combination, and reject each slip such kernels can make -- weights rounded to
16 bits before use, statistics taken from a 16-bit copy of an fp32 row, the sum of an fp32 stream rounded to 16 bits,
a unit of 8 channels left out of a row, a neighbouring row's statistics, a class row counted in dbias, gx16 taken from
a twice-rounded value."""
import pytest
import torch

import ln_amp_oracle as ao
import ln_bwd_oracle as bo
import ln_oracle as lo

EPS = 1e-5
IDS = ["bf16", "fp16"]
WIDTHS = (8, 64, 200, 768, 1024)


def _outside(y, xs, w, b, half, R=1):
    try:
        lo.check(y, xs, w, b, EPS, dtype=half, R=R, label="slip")
    except AssertionError as e:
        assert "outside the bound" in str(e), e  # (not the condition on the inputs)
        return True
    return False


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_forward_emulation_stays_inside_in_every_type_combination(half):
    for C in WIDTHS:
        w, b = ao.affine(C, 7 + C)
        for x_dtype, a_dtype in ao.combos(half):
            x, a = ao.forward_inputs((2, 9, C), x_dtype, a_dtype, 10 * C)
            xs, y = ao.emulate_forward(x, a, w, b, EPS, half)
            assert xs.dtype == x_dtype and y.dtype == half
            if a is not None and x_dtype == ao.F32:
                assert torch.equal(xs, x + a.float())
            stats = lo.check(y, xs, w, b, EPS, dtype=half, label=f"C={C} x={x_dtype} a={a_dtype}")
            assert stats["exact_share"] >= 0.99


def test_fp32_rows_with_an_fp32_addend_are_not_16_bit_rows():
    """What makes the 16-bit-copy slip visible: no stored value of such a row survives a round trip through bf16 or fp16."""
    x, a = ao.forward_inputs((4, 8, 64), ao.F32, ao.F32, 3)
    xs = ao.stored_sum(x, a)
    for half in ao.HALVES:
        assert not bool((xs.to(half).float() == xs).any())


@pytest.mark.parametrize("slip", ao.FORWARD_SLIPS)
@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_forward_slips_fall_outside(half, slip):
    # the 16-bit copy moves a mean by the mean of C rounding errors: shown at the narrow rows, where that is largest
    widths = (8, 16, 24) if slip == "stats_from_16bit_copy" else WIDTHS
    for C in widths:
        w, b = ao.affine(C, 7 + C)
        x, a = ao.forward_inputs((16, 16, C), ao.F32, ao.F32, 10 * C + 1)
        xs, y = ao.emulate_forward(x, a, w, b, EPS, half)
        xs_slip, y_slip = ao.emulate_forward(x, a, w, b, EPS, half, slip=slip)
        assert not _outside(y, xs, w, b, half)
        if slip == "sum_rounded_16bit":
            assert not torch.equal(xs_slip, x + a.float()) and torch.equal(xs, x + a.float())
            continue
        assert torch.equal(xs_slip, xs)
        assert _outside(y_slip, xs, w, b, half), (slip, C, half)


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_backward_emulation_stays_inside_for_both_streams(half):
    for C in WIDTHS:
        for x_dtype in (half, ao.F32):
            for skip, with_in in ((False, True), (True, False), (True, True)):
                gy, xs, gi, w = ao.backward_inputs((2, 9, C), x_dtype, half, 5 * C + skip, skip_first=skip, with_in=with_in,
                                                   far=C % 16 == 0)
                ref = ao.reference(gy, xs, gi, w, EPS, skip_first=skip)
                gx, gx16, dw, db = ao.emulate_backward(gy, xs, gi, w, EPS, skip_first=skip)
                assert gx.dtype == x_dtype and (gx16 is None) == (x_dtype != ao.F32)
                ao.check_backward(f"C={C} x={x_dtype} skip={skip} in={with_in}", gx, gx16, dw, db, ref, half)


def test_fp32_bounds_are_the_tight_ones():
    """u = 2^-24 on an fp32 gx: a gx rounded to bf16 on the way (the 16-bit kernel's output) is far outside."""
    gy, xs, gi, w = ao.backward_inputs((2, 9, 64), ao.F32, torch.bfloat16, 3)
    ref = ao.reference(gy, xs, gi, w, EPS)
    gx, _, _, _ = ao.emulate_backward(gy, xs, gi, w, EPS)
    assert not bool(ao.outside_gx(gx, ref, ao.F32)[0].any())
    assert bool(ao.outside_gx(gx.bfloat16().float(), ref, ao.F32)[0].all())
    assert not bool(ao.outside_gx(gx.bfloat16(), ref, torch.bfloat16)[0].any())


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_backward_slips_fall_outside(half):
    for C in (64, 768):
        # class rows are one row in 16 (512 rows): a counted class row moves dbias by 1/16 of its terms
        gy, xs, gi, w = ao.backward_inputs((32, 16, C), ao.F32, half, C, skip_first=True)
        ref = ao.reference(gy, xs, gi, w, EPS, skip_first=True)
        good = ao.emulate_backward(gy, xs, gi, w, EPS, skip_first=True)
        ao.check_backward(f"honest C={C}", *good, ref, half)
        gx, gx16, dw, db = ao.emulate_backward(gy, xs, gi, w, EPS, skip_first=True, slip="class_row_counted")
        assert bool(ao.outside_param(db, ref, "db")[0].any()), C
        with pytest.raises(AssertionError):
            ao.check_backward(f"class row C={C}", gx, gx16, dw, db, ref, half)
        gx, gx16, dw, db = ao.emulate_backward(gy, xs, gi, w, EPS, skip_first=True, slip="gx16_twice_rounded")
        assert not torch.equal(gx16, gx.to(half))
        with pytest.raises(AssertionError, match="gx16"):
            ao.check_backward(f"twice C={C}", gx, gx16, dw, db, ref, half)
