"""tests/merge_ln_bwd_amp_oracle.py on the CPU: the bounds accept an honest fp32 evaluation of the fused merge + LayerNorm
backward under autocast in every legal type combination, and reject each slip such a kernel can make -- gm rounded to 16
bits before the scales (on a 16-bit stream: on merge_ln_bwd_oracle's tie row; on an fp32 stream: anywhere), statistics
taken from a 16-bit copy of an fp32 row, out_div read at the token instead of at its merged row, a dropped token that
receives a gradient, a destination counted once per token that landed in it, gx16 taken from a twice-rounded value.
Every input is built so that the reference alone meets the oracle's input condition.  No kernel runs."""
import pytest
import torch

import ln_amp_oracle as ao
import ln_oracle as lo
import merge_ln_bwd_amp_oracle as mo
import merge_ln_bwd_oracle as m16

EPS = 1e-5
IDS = ["bf16", "fp16"]
F32 = torch.float32
CASES = [(1, 9, 1, 8), (3, 16, 8, 64), (2, 33, 6, 200), (3, 10, 4, 768), (1, 13, 6, 1024)]


def _case(n, T, r, C, x_dtype, a_dtype, half, seed, size_dtype=None, drop=False, fan3=False, class_token=False,
          distill=False, with_mul=True, with_in=True):
    src, dst, unm = mo.hand_plan(n, T, r, seed, class_token=class_token, distill=distill, fan3=fan3)
    row_of, owns = mo.rows_of_plan(src, dst, unm, T, r, distill=distill, drop=drop)
    size_dtype = size_dtype or x_dtype
    gy, gi, xs, w, size = mo.make_tensors(n, T, r, C, x_dtype, a_dtype, half, size_dtype, seed, with_mul=with_mul,
                                          with_in=with_in, drop=drop)
    s_out = None if drop else mo.size_out_of(size, row_of, n, T, T - r, size_dtype)
    ref = mo.reference(gy, gi, xs, s_out, size, w, EPS, row_of)
    return dict(gy=gy, gi=gi, xs=xs, w=w, size=size, s_out=s_out, row_of=row_of, owns=owns, ref=ref, n=n, T=T, To=T - r,
                C=C)


def _emulate(c, slip=None):
    return mo.emulate(c["gy"], c["gi"], c["xs"], c["s_out"], c["size"], c["w"], EPS, c["row_of"], c["owns"], slip=slip)


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_emulation_stays_inside_in_every_type_combination(half):
    seed = 0
    for n, T, r, C in CASES:
        for x_dtype, a_dtype in ao.combos(half):
            for size_dtype, drop, with_mul, with_in in ((x_dtype, False, True, True), (F32, False, False, False),
                                                        (F32, True, False, True)):
                seed += 1
                c = _case(n, T, r, C, x_dtype, a_dtype, half, seed, size_dtype=size_dtype, drop=drop, with_mul=with_mul,
                          with_in=with_in, class_token=T % 2 == 1, distill=T == 10)
                gx, gx16, dw, db = _emulate(c)
                assert gx.dtype == x_dtype and (gx16 is None) == (x_dtype != F32)
                mo.check(f"n={n} T={T} r={r} C={C} x={x_dtype} a={a_dtype} size={size_dtype} drop={drop}", gx, gx16, dw, db,
                         c["ref"], half)
                if drop:
                    gone = c["row_of"] < 0
                    assert int(gone.sum()) == n * r and float(gx[gone].abs().max()) == 0.0


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_the_reference_alone_meets_the_input_condition(half):
    """Every combination's stored rows are exact-sum rows (the oracle asserts >= 99 %, these inputs give all of them), and
    the oracle refuses rows that are not: ln_bwd_oracle's rows 30 standard deviations from zero with full mantissas."""
    for x_dtype, a_dtype in ao.combos(half):
        c = _case(3, 16, 4, 64, x_dtype, a_dtype, half, 5)
        assert c["ref"]["exact_share"] == 1.0
        assert bool(lo.exact_sum_rows(c["xs"].reshape(-1, 64)).all())
    c = _case(3, 16, 4, 64, F32, F32, half, 5)
    assert not bool((c["xs"].to(half).float() == c["xs"]).any()), "an fp32 stream's rows are not 16-bit rows"
    far = torch.randn(3, 12, 64, generator=torch.Generator().manual_seed(1)) * 3.0 + 31.0
    with pytest.raises(AssertionError, match="exact-sum"):
        mo.reference(c["gy"], c["gi"], far, c["s_out"], c["size"], c["w"], EPS, c["row_of"])


def test_rejects_gm_rounded_before_the_scales_on_a_16_bit_stream():
    """merge_ln_bwd_oracle's tie row: gx_out chosen so that rounding gm to bf16 first lands the scaled value on a tie of
    the final rounding.  The chain's answer is outside in that row, the reference rounded once inside; a power-of-two
    scale cannot show it."""
    half = torch.bfloat16
    n, T, r, C = 1, 8, 1, 96
    src, dst, unm = torch.tensor([[2]]), torch.tensor([[1]]), torch.tensor([[0, 1, 3]])
    row_of, owns = mo.rows_of_plan(src, dst, unm, T, r)
    gy, gi, xs, w, _ = mo.make_tensors(n, T, r, C, half, half, half, half, 25)
    size = torch.ones(n, T, 1, dtype=half)
    size[0, 4], size[0, 3] = 3.0, 1.0  # even token 4 merges into odd token 3: scales 3/4 and 1/4
    s_out = mo.size_out_of(size, row_of, n, T, T - r, half)
    row = int(row_of[0, 4])
    assert float(s_out[0, row]) == 4.0
    ref_of = lambda g: mo.reference(gy, g, xs, s_out, size, w, EPS, row_of)  # noqa: E731
    gi, tok = m16.tie_row(ref_of, gi, xs, row, half)
    assert tok == 4
    ref = ref_of(gi)
    assert not bool(mo.outside_gx(ref["gx"].to(half), ref)[0].any())
    idx = row_of[..., None].expand(n, T, C)
    twice = (ref["gm"].to(half).double().gather(1, idx) * ref["scale"][..., None]).to(half)
    outside = (twice.double() - ref["gx"]).abs()[0, tok] > mo.bound_gx(ref, half)[0, tok]
    print(f"second rounding: {int(outside.sum())} of {C} channels of the tie row outside the bound")
    assert int(outside.sum()) >= C // 2
    bad, _ = mo.outside_gx(twice, ref)
    assert bool(bad[0, tok]) and not bool(bad[0, 3])
    # the emulation with the slip on the same row: outside too, and inside without it
    args = (gy, gi, xs, s_out, size, w, EPS, row_of, owns)
    assert not bool(mo.outside_gx(mo.emulate(*args)[0], ref)[0].any())
    assert bool(mo.outside_gx(mo.emulate(*args, slip="gm_rounded_16bit")[0], ref)[0][0, tok])


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_rejects_gm_rounded_to_16_bits_on_an_fp32_stream(half):
    for a_dtype in (half, F32, None):
        c = _case(2, 16, 4, 64, F32, a_dtype, half, 31)
        assert not bool(mo.outside_gx(_emulate(c)[0], c["ref"])[0].any())
        bad, _ = mo.outside_gx(_emulate(c, "gm_rounded_16bit")[0], c["ref"])
        assert bool(bad.all()), "u = 2^-24 on an fp32 gx: every token row shows a 16-bit rounding"


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_rejects_statistics_from_a_16_bit_copy(half):
    """fine_addend rows (an fp32 stream with an fp32 addend): no stored value survives a round trip through 16 bits.  The
    copy moves a mean by the mean of C rounding errors: shown at the narrow rows, where that is largest."""
    for C in (8, 16, 24):
        c = _case(3, 16, 4, C, F32, F32, half, 32 + C)
        assert not bool(mo.outside_gx(_emulate(c)[0], c["ref"])[0].any())
        gx, gx16, dw, db = _emulate(c, "stats_from_16bit_copy")
        bad, _ = mo.outside_gx(gx, c["ref"])
        assert float(bad.double().mean()) > 0.9, (C, half)
        with pytest.raises(AssertionError):
            mo.check(f"16-bit copy C={C}", gx, gx16, dw, db, c["ref"], half)


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_rejects_out_div_read_at_the_token(half):
    """Wrong wherever size'[min(t, To - 1)] != size'[o(t)]."""
    for x_dtype in (half, F32):
        c = _case(2, 16, 5, 64, x_dtype, half, half, 33)
        n, T, To = c["n"], c["T"], c["To"]
        so = c["s_out"].double().reshape(n, To)
        at_t = so.gather(1, torch.arange(T).clamp_max(To - 1).expand(n, T))
        differs = at_t != so.gather(1, c["row_of"])
        assert int(differs.sum()) >= n * 3
        bad, _ = mo.outside_gx(_emulate(c, "out_div_at_t")[0], c["ref"])
        assert torch.equal(bad, differs)


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_rejects_a_dropped_token_with_a_gradient(half):
    for x_dtype in (half, F32):
        c = _case(2, 12, 3, 64, x_dtype, half, half, 34, drop=True)
        gone = c["row_of"] < 0
        assert int(gone.sum()) == 2 * 3
        assert not bool(mo.outside_gx(_emulate(c)[0], c["ref"])[0].any())
        bad, _ = mo.outside_gx(_emulate(c, "dropped_token_gets_gm")[0], c["ref"])
        assert torch.equal(bad, gone)
        tiny = _emulate(c)[0]
        tiny[gone] = 2.0 ** -14
        assert torch.equal(mo.outside_gx(tiny, c["ref"])[0], gone)


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_rejects_a_destination_counted_once_per_token(half):
    """A destination with three sources counted 1 + 3 times in dweight / dbias."""
    for x_dtype in (half, F32):
        c = _case(2, 13, 4, 96, x_dtype, half, half, 21, fan3=True)
        assert all(int(torch.bincount(c["row_of"][g]).max()) >= 4 for g in range(c["n"]))
        _, _, dw, db = _emulate(c)
        assert not bool(mo.outside_param(dw, c["ref"], "dw")[0].any())
        assert not bool(mo.outside_param(db, c["ref"], "db")[0].any())
        gx, gx16, dw, db = _emulate(c, "dest_counted_per_token")
        assert float(mo.outside_param(dw, c["ref"], "dw")[0].double().mean()) > 0.9
        assert float(mo.outside_param(db, c["ref"], "db")[0].double().mean()) > 0.9
        with pytest.raises(AssertionError):
            mo.check("counted per token", gx, gx16, dw, db, c["ref"], half)


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_rejects_a_gx16_that_is_not_the_cast_of_gx(half):
    c = _case(2, 16, 5, 64, F32, half, half, 35)
    gx, gx16, dw, db = _emulate(c)
    mo.check("honest", gx, gx16, dw, db, c["ref"], half)
    gx, gx16, dw, db = _emulate(c, "gx16_twice_rounded")
    assert not torch.equal(gx16, gx.to(half))
    with pytest.raises(AssertionError, match="gx16"):
        mo.check("twice", gx, gx16, dw, db, c["ref"], half)


def test_partition_and_form_follow_the_dispatch():
    assert mo.form is m16.form and mo.FORM_WIDTHS is m16.FORM_WIDTHS
    part = mo.parts_of_tokens(3, 13, 96)
    R, spw, parts = mo.form(3, 13, 96)
    assert (R, spw) == (4, 1) and int(part.max()) + 1 == parts
    assert part[0].tolist() == [0] * 13 and part[1, 0] == 1  # 4 slabs of 4 tokens per group, 4 slabs per workgroup
    R, spw, parts = mo.form(70000, 4, 8)
    assert spw > 1 and int(mo.parts_of_tokens(70000, 4, 8).max()) + 1 == parts
