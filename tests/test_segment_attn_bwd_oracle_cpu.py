"""segment_attn_bwd_oracle.py on the CPU: the bound accepts the emulation of the kernels' arithmetic (q~, P, dS and the
stored O rounded to the format, dq summed over the segments and rounded once) and rejects the wrong answers the
segmented kernels can give."""
import pytest
import torch

import segment_attn_bwd_oracle as so

DTYPES = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_emulation_is_inside_the_bound(dtype):
    for i, (B, H, N, P, nseg, bias, gain) in enumerate([(1, 2, 31, 65, 2, True, 1.0), (2, 1, 24, 3, 8, True, 8.0),
                                                         (1, 1, 70, 129, 1, False, 1.0), (1, 3, 16, 2, 8, False, 1.0)]):
        inp = so.make_inputs(B, H, N, P, nseg, dtype, seed=20 + i, bias=bias, logit_gain=gain,
                             max_size=64 if gain > 1 else 8, layout="qkv" if N == nseg * P else "separate")
        ref = so.reference(inp)
        so.check(f"emulation {B}x{H}x{N}x{nseg}x{P} {dtype}", so.emulate(inp), ref, so.bounds(ref, dtype))


def test_reference_is_the_sum_of_the_segments():
    """The op sequence's gradient and the per-segment references the bound is built from describe the same function."""
    inp = so.make_inputs(1, 2, 9, 5, 3, torch.bfloat16, seed=1)
    ref = so.reference(inp)
    assert torch.allclose(ref["dq"], sum(r["dq"] for r in ref["segs"]), rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref["dk"], torch.cat([r["dk"] for r in ref["segs"]], 2), rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref["dv"], torch.cat([r["dv"] for r in ref["segs"]], 2), rtol=1e-12, atol=1e-12)


# shapes under which each slip shows: eight segments for the ones in the dq sum (a rounding per segment is a random walk
# of eight u-sized steps against one), keys 65 = one whole tile + a partial one for the dropped tile, a common mean in v
# and dy for delta (attn_bwd_oracle.py's "offset" family)
SLIP_CASES = {
    "dq_segment0_only": dict(B=1, H=2, N=24, P=3, nseg=8),
    "bias_of_next_segment": dict(B=1, H=2, N=24, P=12, nseg=2, max_size=64),
    "last_partial_tile_dropped": dict(B=1, H=2, N=33, P=65, nseg=2),
    "dkv_segments_exchanged": dict(B=1, H=2, N=24, P=12, nseg=2),
    "delta_omitted": dict(B=1, H=2, N=24, P=12, nseg=2, offset=2.0),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("slip", [s for s in so.SLIPS if s != "dq_rounded_per_segment"])
def test_wrong_answers_are_outside_the_bound(slip, dtype):
    inp = so.make_inputs(dtype=dtype, seed=4, **SLIP_CASES[slip])
    ref = so.reference(inp)
    w = so.worst(so.emulate(inp, slip), ref, so.bounds(ref, dtype))
    print(slip, dtype, w)
    hit = {"dq_segment0_only": ("dq",), "bias_of_next_segment": ("dq", "dk", "dv"),
           "last_partial_tile_dropped": ("dv",), "dkv_segments_exchanged": ("dk", "dv"), "delta_omitted": ("dq", "dk")}[slip]
    for n in hit:
        assert w[n] > 1.0, f"{slip}: {n} stayed inside the bound ({w[n]:.3f})"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_a_rounding_per_segment_is_rejected_by_the_exact_case(dtype):
    """dq rounded once per segment: no worst-case bound of this construction can reject it (the dS operand's allowance
    alone exceeds it: segment_attn_bwd_oracle.py), so it is held by the case whose roundings are all exact -- summed in
    fp32 and rounded once, dq is the reference bit for bit; rounded per segment it is one unit in the last place off."""
    inp = so.exact_inputs(dtype)
    ref = so.reference(inp)
    want = ref["dq"].to(dtype)
    assert torch.equal(want.double(), ref["dq"]), "the exact dq is a number of the format"
    eps = so.U[dtype] / 2
    assert torch.equal(ref["dq"], torch.full_like(ref["dq"], (1 + 4 * eps) / 4))
    good, bad = so.emulate(inp), so.emulate(inp, "dq_rounded_per_segment")
    assert torch.equal(good["dq"], ref["dq"])
    assert torch.equal(bad["dq"], torch.full_like(ref["dq"], 0.25))
    assert float(ref["dk"].abs().max()) == 0.0 and torch.equal(good["dv"], ref["dv"])
    # ... and stays inside the bound, which is why the bound is not what holds it
    assert so.worst(bad, ref, so.bounds(ref, dtype))["dq"] <= 1.0
