"""CPU side of tome_merge_ln_backward's accounting (tests/merge_ln_bwd_oracle.py): the bound accepts the fp64 reference
rounded once to the token dtype and rejects, one by one, the wrong answers a fused merge + LayerNorm backward can give.
Every input is built so that the slip lands outside the bound with the reference alone inside it.  No kernel runs."""
import pytest
import torch

import merge_ln_bwd_oracle as mo

DTYPES = [torch.bfloat16, torch.float16]
EPS = 1e-5


def _case(n, T, r, C, dtype, seed, size_dtype=None, drop=False, fan3=False, class_token=False, distill=False):
    """(tensors, plan rows, reference, and a builder of the reference for another gx_out)."""
    size_dtype = size_dtype or dtype
    src, dst, unm = mo.hand_plan(n, T, r, seed, class_token=class_token, distill=distill, fan3=fan3)
    row_of, owns = mo.rows_of_plan(src, dst, unm, T, r, distill=distill, drop=drop)
    gy, gi, xs, w, size = mo.make_tensors(n, T, r, C, dtype, size_dtype, seed, drop=drop)
    s_out = None if drop else mo.size_out_of(size, row_of, n, T, T - r, size_dtype)
    ref_of = lambda g: mo.reference(gy, g, xs, s_out, size, w, EPS, row_of)  # noqa: E731
    return dict(gy=gy, gi=gi, xs=xs, w=w, size=size, s_out=s_out, row_of=row_of, owns=owns, ref=ref_of(gi), ref_of=ref_of,
                n=n, T=T, To=T - r, C=C, dst=dst)


def _rounded(ref, dtype):
    return ref["gx"].to(dtype), ref["dw"].to(dtype), ref["db"].to(dtype)


CASES = [(1, 8, 1, 8), (3, 9, 4, 96), (2, 13, 3, 384), (3, 10, 4, 768), (1, 13, 6, 1024)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_bound_accepts_the_rounded_reference(dtype):
    seed = 0
    for n, T, r, C in CASES:
        for size_dtype, drop in ((dtype, False), (torch.float32, False), (dtype, True)):
            seed += 1
            c = _case(n, T, r, C, dtype, seed, size_dtype=size_dtype, drop=drop, class_token=T % 2 == 1)
            gx, dw, db = _rounded(c["ref"], dtype)
            mo.check(f"rounded reference n={n} T={T} r={r} C={C} drop={drop} {dtype}", gx, dw, db, c["ref"], dtype)
            if drop:
                assert bool((c["row_of"] < 0).any()) and float(gx[c["row_of"] < 0].abs().max()) == 0.0


def test_rows_of_plan_is_the_reference_layout():
    """Every merged row has exactly one owner; with a distillation token odd token 0 keeps row 1."""
    for distill in (False, True):
        src, dst, unm = mo.hand_plan(3, 10, 3, 5, class_token=True, distill=distill)
        row_of, owns = mo.rows_of_plan(src, dst, unm, 10, 3, distill=distill)
        for g in range(3):
            owned = sorted(row_of[g][owns[g]].tolist())
            assert owned == list(range(7))
            assert int(row_of[g, 0]) == 0 and int(row_of[g, 1]) == (1 if distill else 2)
            assert int((~owns[g]).sum()) == 3


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rejects_a_destination_counted_once_per_token(dtype):
    """A destination with three sources counted 1 + 3 times in dweight / dbias."""
    c = _case(2, 13, 4, 96, dtype, 21, fan3=True)
    ref, C = c["ref"], c["C"]
    assert all(int(torch.bincount(c["row_of"][g]).max()) >= 4 for g in range(c["n"]))  # a destination and three sources
    # the term of every merged row, taken once per token that landed in it
    g, x = c["gy"].double(), c["xs"].double()
    d = x - x.mean(-1, keepdim=True)
    xhat = d * ((d * d).mean(-1, keepdim=True) + EPS) ** -0.5
    idx = c["row_of"][..., None].expand(c["n"], c["T"], C)
    dw_wrong, db_wrong = (g * xhat).gather(1, idx).sum((0, 1)), g.gather(1, idx).sum((0, 1))
    assert torch.allclose((g * xhat).sum((0, 1)), ref["dw"]) and torch.allclose(g.sum((0, 1)), ref["db"])
    gx, dw, db = _rounded(ref, dtype)
    assert not bool(mo.outside_param(dw, ref, "dw", dtype)[0].any())
    assert not bool(mo.outside_param(db, ref, "db", dtype)[0].any())
    assert float(mo.outside_param(dw_wrong.to(dtype), ref, "dw", dtype)[0].double().mean()) > 0.9
    assert float(mo.outside_param(db_wrong.to(dtype), ref, "db", dtype)[0].double().mean()) > 0.9


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rejects_a_merged_token_with_its_neighbours_row(dtype):
    c = _case(2, 12, 3, 96, dtype, 22)
    ref = c["ref"]
    wrong_rows = torch.where(c["owns"], c["row_of"], (c["row_of"] + 1) % c["To"])
    wrong = mo.reference(c["gy"], c["gi"], c["xs"], c["s_out"], c["size"], c["w"], EPS, wrong_rows)["gx"].to(dtype)
    bad, _ = mo.outside_gx(wrong, ref, dtype)
    assert torch.equal(bad, ~c["owns"]), "exactly the merged-away tokens must be rejected"
    assert not bool(mo.outside_gx(ref["gx"].to(dtype), ref, dtype)[0].any())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rejects_swapped_scales(dtype):
    """gm * out_div / in_mul: wrong wherever size'[o(t)] != size[t], i.e. at least at every token of a merged row."""
    c = _case(2, 12, 3, 96, dtype, 23)
    ref, n, T, To, C = c["ref"], c["n"], c["T"], c["To"], c["C"]
    so = c["s_out"].double().reshape(n, To).gather(1, c["row_of"])
    si = c["size"].double().reshape(n, T)
    wrong = (ref["gm"].gather(1, c["row_of"][..., None].expand(n, T, C)) * (so / si)[..., None]).to(dtype)
    bad, _ = mo.outside_gx(wrong, ref, dtype)
    assert torch.equal(bad, so != si)
    assert bool(bad[~c["owns"]].all()) and int(bad.sum()) >= 2 * 3 * 2


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rejects_a_gradient_without_the_residual_stream(dtype):
    c = _case(2, 12, 3, 96, dtype, 24)
    wrong = mo.reference(c["gy"], None, c["xs"], c["s_out"], c["size"], c["w"], EPS, c["row_of"])["gx"].to(dtype)
    bad, _ = mo.outside_gx(wrong, c["ref"], dtype)
    assert bool(bad.all())


def test_rejects_a_second_rounding_on_a_tie():
    """gm rounded to bf16 before the scales (the two-launch chain) on a row built so that the scaled value sits on a tie of
    the final rounding: the chain's answer is outside the bound in that row, the reference rounded once inside."""
    dtype = torch.bfloat16
    n, T, r, C = 1, 8, 1, 96
    src, dst, unm = torch.tensor([[2]]), torch.tensor([[1]]), torch.tensor([[0, 1, 3]])
    row_of, owns = mo.rows_of_plan(src, dst, unm, T, r)
    gy, gi, xs, w, _ = mo.make_tensors(n, T, r, C, dtype, dtype, 25)
    size = torch.ones(n, T, 1, dtype=dtype)
    size[0, 4], size[0, 3] = 3.0, 1.0  # even token 4 (A index 2) merges into odd token 3 (B index 1): scales 3/4, 1/4
    s_out = mo.size_out_of(size, row_of, n, T, T - r, dtype)
    row = int(row_of[0, 4])
    assert float(s_out[0, row]) == 4.0
    ref_of = lambda g: mo.reference(gy, g, xs, s_out, size, w, EPS, row_of)  # noqa: E731
    gi, tok = mo.tie_row(ref_of, gi, xs, row, dtype)
    assert tok == 4
    ref = ref_of(gi)
    once = ref["gx"].to(dtype)
    idx = row_of[..., None].expand(n, T, C)
    twice = (ref["gm"].to(dtype).double().gather(1, idx) * ref["scale"][..., None]).to(dtype)
    assert not bool(mo.outside_gx(once, ref, dtype)[0].any())
    err = (twice.double() - ref["gx"]).abs()[0, tok]
    outside = err > mo.bound_gx(ref, dtype)[0, tok]
    print(f"second rounding: {int(outside.sum())} of {C} channels of the tie row outside the bound")
    assert int(outside.sum()) >= C // 2
    bad, _ = mo.outside_gx(twice, ref, dtype)
    assert bool(bad[0, tok])
    # a power-of-two scale cannot show it: the token of the same row with scale 1/4 stays inside
    assert not bool(bad[0, 3])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rejects_a_dropped_token_with_a_gradient(dtype):
    c = _case(2, 12, 3, 96, dtype, 26, drop=True)
    ref = c["ref"]
    kept = mo.reference(c["gy"], c["gi"], c["xs"], None, None, c["w"], EPS, c["row_of"].clamp_min(0))["gx"].to(dtype)
    bad, _ = mo.outside_gx(kept, ref, dtype)
    assert torch.equal(bad, c["row_of"] < 0) and int(bad.sum()) == 2 * 3
    tiny = ref["gx"].to(dtype)
    tiny[c["row_of"] < 0] = 2.0 ** -14
    assert torch.equal(mo.outside_gx(tiny, ref, dtype)[0], c["row_of"] < 0)


def test_form_follows_the_dispatch():
    for (nit, R), C in mo.FORM_WIDTHS.items():
        assert mo.expected_form(C) == (nit, R)
    assert {mo.expected_form(C)[1] for C in (8, 96, 384)} == {4}
    R, spw, parts = mo.form(64, 1568, 768)
    assert R == 2 and parts <= mo.MAX_PARTS and spw * parts * 4 * R >= 64 * 1568
    R, spw, parts = mo.form(1, 8, 8)
    assert (R, spw, parts) == (4, 1, 1)
