"""The construction of attn_bwd_accounting.py, proven sharp without a GPU, on every case of the grids that
test_attention_backward_accounting_gpu.py runs:

  * bound        the emulation of the correct kernels (attn_bwd_oracle.emulate / segment_attn_bwd_oracle.emulate) is
                 inside the unchanged bound on every family, encoding, bias form and format, and exactly 0 where the
                 bound is 0;
  * sensitivity  from the fp64 reference alone: leaving a single row out of (or counting it twice in) one row's sum moves
                 the damaged gradient by more than its bound in the "mod" encoding, and so does leaving out any aligned
                 32-, 64- or 128-row block in the "block" encoding -- a condition on the grid, not a measurement;
  * slips        each wrong answer of attn_bwd_accounting.SLIPS is rejected through the gradient it damages: dq for the
                 key-side slips on family K, dk for the query-side slips on family Q (never through dv alone);
  * reach        the grids contain what the kernels' structure asks for (checked at collection)."""
import pytest
import torch

import attn_bwd_accounting as aa
import attn_bwd_oracle as ao
import segment_attn_bwd_oracle as so

DTYPES = [torch.bfloat16, torch.float16]
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}

# (B, H, N, Nk) of every plain GPU case
PLAIN = [aa.PLAIN_BH + s for s in aa.PLAIN_SHAPES] + [bh + s for bh in aa.HEADS for s in aa.HEAD_SHAPES]

# ---- reach: what the grids have to contain -- asserted at collection, on any machine
assert {b * h for b, h in aa.HEADS} >= {9, 17, 24}, "the item map's second and third round of 8 are not reached"
for _edge in (32, 64, 128):
    for _axis in (0, 1):  # N and Nk on both sides of the lane half, the tile and the workgroup block
        _sizes = {s[_axis] for s in aa.PLAIN_SHAPES}
        assert {_edge - 1, _edge, _edge + 1} <= _sizes or (min(_sizes) < _edge < max(_sizes)), (_edge, _axis)
        assert min(_sizes) < _edge < max(_sizes), (_edge, _axis)
assert any(s[1] == 1 for s in aa.PLAIN_SHAPES) and any(s[0] == 1 for s in aa.PLAIN_SHAPES), "Nk = 1 and N = 1"
for _shapes in (aa.TARGET_SHAPES, aa.STRIDE_SHAPES):
    assert set(_shapes) <= set(aa.PLAIN_SHAPES), "a target / stride shape the bound and sensitivity tests do not cover"


def degenerate(N, Nk, kind, enc):
    """The cases in which the family's dq / dk is structurally zero, so that no omission can show in it -- by name:
      "one key":   Nk = 1 -- P = 1, delta_i = a_0, dS = P (a - delta) = 0 whatever the encoding;
      "one block": the "block" encoding with Nk <= 32 -- every key lies in block 0, every a_j = +1, delta_i = 1, dS = 0.
    dv = P^T dO is never degenerate.  Every such shape is covered for dq / dk by "mod" unless Nk = 1."""
    if Nk == 1:
        return "one key"
    if enc == "block" and Nk <= 32:
        return "one block"
    return None


def _id(c):
    return "x".join(str(x) for x in c)


@pytest.mark.parametrize("kind", aa.KINDS)
@pytest.mark.parametrize("case", PLAIN, ids=_id)
def test_emulation_inside_bound_and_omissions_outside(case, kind):
    """Both conditions on one fp64 reference per (encoding, bias form): the inputs are exact in both formats, so the
    reference is shared and only the bound is per format."""
    B, H, N, Nk = case
    covered = {}
    for enc in aa.ENCODINGS:
        for bias in aa.biases_for(N, Nk):
            ref = None
            for dtype in DTYPES:
                sep, qkv = aa.make_family(kind, B, H, N, Nk, dtype, bias, enc, seed=N + Nk)
                if qkv is not None:
                    assert all(torch.equal(getattr(sep, n), getattr(qkv, n)) for n in ("q", "k", "v", "dout"))
                ref = ref or ao.reference(sep)
                bnd = ao.bounds(ref, dtype)
                label = f"{_id(case)} {kind} {enc} {bias} {NAME[dtype]}"
                aa.check("emulation " + label, ao.emulate(sep), ref, bnd)
                own = "dq" if kind == "K" else "dk"
                other = "dk" if kind == "K" else "dq"
                assert float(ref[other].abs().max()) == 0.0 and (dtype != torch.bfloat16 or float(bnd[other].max()) == 0.0)
                for gran in (("row",) if enc == "mod" else (32, 64, 128)):
                    sens = aa.omission_sensitivity(ref, bnd, kind, gran)
                    print(f"sensitivity {label} {gran}: " + "  ".join(f"{n} {x:.2f}" for n, x in sens.items()))
                    for n, x in sens.items():
                        if n.startswith(own) and degenerate(N, Nk, kind, enc):
                            assert x < 1e-9, (label, gran, n, x)   # (named above: dS = 0 up to fp64 rounding -- nothing to leave out)
                            continue
                        assert x > 1.0, f"{label}: leaving out / doubling a unit of {gran} moves {n} by {x:.3f} bounds only"
                        covered.setdefault((dtype, n.split("_")[0]), set()).add(enc)
    for dtype in DTYPES:  # every gradient the shape is meant to check, by at least one encoding
        want = {"dv"} | (set() if Nk == 1 else {"dq" if kind == "K" else "dk"})
        assert {n for (d, n) in covered if d == dtype} == want, (case, kind, covered)


SEG_CASES = [c + ("separate",) for c in aa.SEGMENTS] + [c + ("qkv",) for c in aa.SEGMENTS_QKV]


@pytest.mark.parametrize("kind", aa.KINDS)
@pytest.mark.parametrize("case", SEG_CASES, ids=_id)
def test_segment_emulation_inside_bound(case, kind):
    B, H, N, P, nseg, layout = case
    for enc in aa.ENCODINGS:
        for bias in ("none", "bias"):
            ref = None
            for dtype in DTYPES:
                inp = aa.make_segment_family(kind, B, H, N, P, nseg, dtype, bias, enc, seed=N + P, layout=layout)
                ref = ref or so.reference(inp)
                aa.check(f"segments emulation {_id(case)} {kind} {enc} {bias} {NAME[dtype]}", so.emulate(inp), ref,
                         so.bounds(ref, dtype))


def test_segments_carry_their_own_rotation():
    """Exchanged segments show: keys of family K and every segment's dy are rotated by 5 s."""
    inp = aa.make_segment_family("K", 1, 2, 65, 33, 2, torch.bfloat16, "bias", "mod", seed=1)
    assert not torch.equal(inp.k[:, :, :33], inp.k[:, :, 33:]) and not torch.equal(inp.dy[:, :, 0], inp.dy[:, :, 1])
    ref = so.reference(inp)
    got = so.emulate(inp, slip="dkv_segments_exchanged")
    assert aa.worst(got, ref, so.bounds(ref, torch.bfloat16))["dv"] > 1.0


# (slip, family, gradient it must be rejected through, encodings, (B, H, N, Nk), bias)
SLIP_CASES = [
    ("last_key_tile_dropped", "K", "dq", ("mod", "block"), (2, 3, 129, 129), "none"),   # key 128 alone
    ("last_key_tile_dropped", "K", "dq", ("mod", "block"), (2, 3, 33, 449), "bias"),
    ("key_half_dropped", "K", "dq", ("mod", "block"), (2, 3, 129, 129), "skip"),
    ("key_half_dropped", "K", "dq", ("mod", "block"), (2, 3, 129, 65), "none"),
    ("bias_off_by_one", "K", "dq", ("mod",), (2, 3, 129, 129), "bias"),
    ("head_wrapped", "K", "dq", ("mod", "block"), (3, 3, 129, 65), "none"),
    ("head_wrapped", "K", "dq", ("mod", "block"), (1, 17, 65, 129), "bias"),
    ("query_block_dropped", "Q", "dk", ("mod", "block"), (2, 3, 129, 129), "none"),
    ("query_block_dropped", "Q", "dk", ("mod", "block"), (2, 3, 449, 33), "bias"),
    ("bias_off_by_one", "Q", "dk", ("mod", "block"), (2, 3, 129, 129), "bias"),
    ("head_wrapped", "Q", "dk", ("mod", "block"), (3, 3, 65, 129), "none"),
    ("head_wrapped", "Q", "dk", ("mod", "block"), (2, 12, 129, 65), "bias"),
    ("rows_past_end_added", "Q", "dk", ("mod", "block"), (2, 3, 129, 129), "skip"),
    ("rows_past_end_added", "Q", "dk", ("mod", "block"), (2, 3, 33, 449), "none"),
]
assert {c[0] for c in SLIP_CASES} == set(aa.SLIPS)
assert all(c[0] in (aa.KEY_SIDE if c[1] == "K" else aa.QUERY_SIDE) for c in SLIP_CASES)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", SLIP_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{_id(c[4])}-{c[5]}")
def test_slips_are_rejected_through_the_gradient_they_damage(case, dtype):
    slip, kind, grad, encs, (B, H, N, Nk), bias = case
    for enc in encs:
        sep, _ = aa.make_family(kind, B, H, N, Nk, dtype, bias, enc, seed=3)
        ref = ao.reference(sep)
        bnd = ao.bounds(ref, dtype)
        right = aa.worst(aa.emulate(sep), ref, bnd)
        wrong = aa.worst(aa.emulate(sep, slip=slip), ref, bnd)
        print(f"{slip} {kind} {enc} {NAME[dtype]}: right {right}, wrong {wrong}")
        assert max(right.values()) <= 1.0
        assert wrong[grad] > 1.0, f"{slip} ({enc}): {grad} still inside its bound ({wrong})"


def test_check_demands_exact_zero_where_the_bound_is_zero():
    """bf16, family K: dk's bound is 0 everywhere -- attn_bwd_oracle.worst would divide 0 by 0; here 0 passes, anything
    else (the smallest bf16 number, a NaN) fails; and a wrong element with a positive bound fails as before."""
    dtype = torch.bfloat16
    sep, _ = aa.make_family("K", 1, 2, 65, 65, dtype, "bias", "mod", seed=2)
    ref = ao.reference(sep)
    bnd = ao.bounds(ref, dtype)
    assert float(bnd["dk"].max()) == 0.0
    good = ao.emulate(sep)
    aa.check("good", good, ref, bnd)
    for name, idx, value in (("dk", (0, 1, 64, 63), 2.0 ** -126), ("dk", (0, 0, 0, 0), float("nan")),
                             ("dq", (0, 1, 3, 5), float("inf")), ("dv", (0, 0, 64, 0), None)):
        bad = {n: t.clone() for n, t in good.items()}
        bad[name][idx] = value if value is not None else bad[name][idx] + 2 * float(bnd[name][idx]) + 2.0 ** -6
        assert aa.worst(bad, ref, bnd)[name] > 1.0
        with pytest.raises(AssertionError):
            aa.check("bad", bad, ref, bnd)


def test_reference_depends_on_the_rotation_alone():
    """What the test beyond 2^31 elements relies on: without a bias the reference and bound of (batch b, head h) are
    those of the rotation (7b + 3h) mod 64 -- computed once at B = 64, H = 1 (entry b0 has the rotation 7 b0 mod 64)
    and gathered at b0 = 55 (7b + 3h) mod 64, 7 * 55 being 1 mod 64."""
    dtype, N = torch.bfloat16, 70
    small, _ = aa.make_family("K", 64, 1, N, N, dtype, "none", "mod")
    big, _ = aa.make_family("K", 11, 5, N, N, dtype, "none", "mod")
    rs, rb = ao.reference(small), ao.reference(big)
    bs, bb = ao.bounds(rs, dtype), ao.bounds(rb, dtype)
    b0 = (aa.rotation(11, 5) % 64 * 55) % 64
    for n in ("dq", "dk", "dv"):
        assert torch.equal(rs[n][:, 0][b0], rb[n]) and torch.equal(bs[n][:, 0][b0], bb[n]), n


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_slip_emulation_is_the_oracles_arithmetic(dtype):
    """The lines attn_bwd_accounting.emulate repeats are attn_bwd_oracle.emulate's: a slip with nothing to act on (keys
    32 .. 63 of a 31-key row, the bias read at j - 1 without a bias) returns the same bits, on random heads too."""
    for inp in (ao.make_inputs(2, 2, 40, 31, dtype, 4, bias="bias"), aa.make_family("K", 2, 3, 40, 31, dtype, "bias")[0]):
        want = ao.emulate(inp)
        got = aa.emulate(inp, slip="key_half_dropped")
        assert all(torch.equal(got[n], want[n]) for n in want)
    inp = ao.make_inputs(1, 2, 70, 70, dtype, 5, bias="none", layout="qkv")
    want, got = ao.emulate(inp), aa.emulate(inp, slip="bias_off_by_one")
    assert all(torch.equal(got[n], want[n]) for n in want)
