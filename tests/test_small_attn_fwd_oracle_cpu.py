"""tests/small_attn_fwd_oracle.py on the CPU: the derived bound accepts an fp32 evaluation of each kernel's formula (sums
in another order than the kernel's), in both dtypes, with flat and with dominated rows, and rejects each wrong answer
such a streaming kernel can give.  The condition is always zero elements outside."""
import pytest
import torch

import short_attn_bwd_oracle as so
import small_attn_fwd_oracle as fo
import traj_mix_bwd_oracle as to

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
TRAJ_CASES = [(1, 7, 1, 1), (2, 5, 3, 9), (1, 5, 8, 16), (2, 3, 5, 12)]  # B, S, F, H
SHORT_CASES = [(7, 1, 1), (5, 2, 5), (3, 12, 8), (4, 5, 3)]               # B, H, N


def _padded_val(inp: to.Inputs) -> to.Inputs:
    """The same values with val a view of a [B, S, F, C + 8] buffer: its row stride is not k2's."""
    B, S, F, C = inp.val.shape
    buf = torch.full((B, S, F, C + 8), 3.0, dtype=inp.val.dtype)
    buf[..., :C] = inp.val
    return inp._replace(val=buf[..., :C])


def _padded_v(inp: so.Inputs) -> so.Inputs:
    """The same values with v a head view of a [B, N, H*64 + 8] buffer: its token and batch strides are not k's."""
    B, H, N, _ = inp.v.shape
    buf = torch.full((B, N, H * 64 + 8), 3.0, dtype=inp.v.dtype)
    buf[..., :H * 64] = inp.v.permute(0, 2, 1, 3).reshape(B, N, H * 64)
    return inp._replace(v=buf[..., :H * 64].unflatten(-1, (H, 64)).permute(0, 2, 1, 3))


@pytest.mark.parametrize("gain", [1.0, 8.0])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fp32_evaluation_of_the_trajectory_mix_is_inside_the_bound(dtype, gain):
    for i, (B, S, F, H) in enumerate(TRAJ_CASES):
        inp = to.make_inputs(B, S, F, H, dtype, seed=20 + i, logit_gain=gain)
        for x in (inp, _padded_val(inp)):
            worst = fo.check(f"fp32 {B}x{S}x{F}x{H} gain {gain} {dtype}", fo.emulate_fp32(x), fo.reference(x), dtype)
            if F == 1:
                assert worst == dict(out=0.0, tattn=0.0), "one frame: the weight is 1 and out is val, exactly"


@pytest.mark.parametrize("gain", [1.0, 8.0])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fp32_evaluation_of_the_short_attention_is_inside_the_bound(dtype, gain):
    for i, (B, H, N) in enumerate(SHORT_CASES):
        for layout in ("qkv", "separate"):
            inp = so.make_inputs(B, H, N, dtype, 40 + i, layout=layout, logit_gain=gain)
            for x in (inp, _padded_v(inp)):
                worst = fo.check(f"fp32 {B}x{H}x{N} {layout} gain {gain} {dtype}", fo.emulate_fp32(x), fo.reference(x),
                                 dtype)
                if N == 1:
                    assert worst == dict(out=0.0), "one token: out is v, exactly"


def test_gain_8_gives_rows_dominated_by_their_maximum():
    ref = fo.reference(to.make_inputs(2, 5, 8, 12, torch.bfloat16, seed=1, logit_gain=8.0))
    assert float(ref["P"].amax(-1).median()) > 0.5 and float(ref["z"].abs().max()) > 20
    ref = fo.reference(so.make_inputs(3, 12, 8, torch.bfloat16, 1, logit_gain=8.0))
    assert float(ref["P"].amax(-1).median()) > 0.5 and float(ref["z"].abs().max()) > 20


def test_reference_is_the_framework_attention_in_fp64():
    inp = so.make_inputs(2, 3, 8, torch.bfloat16, 5)
    q, k, v = (t.double() for t in (inp.q, inp.k, inp.v))
    want = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=inp.scale).transpose(1, 2).reshape(2, 8, 192)
    assert torch.allclose(fo.reference(inp)["out"], want, rtol=1e-12, atol=1e-14)
    t = to.make_inputs(2, 3, 4, 2, torch.bfloat16, seed=5)
    q2 = t.q2.double().view(2, 3, 2, 64) * t.scale
    k2, val = (x.double().view(2, 3, 4, 2, 64) for x in (t.k2, t.val))
    p = torch.einsum("bshd,bsfhd->bhsf", q2, k2).softmax(-1)
    ref = fo.reference(t)
    assert torch.allclose(ref["tattn"], p, rtol=1e-12, atol=1e-14)
    assert torch.allclose(ref["out"], torch.einsum("bhsf,bsfhd->bshd", p, val).reshape(2, 3, 128), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("slip", fo.TRAJ_SLIPS)
def test_wrong_trajectory_mixes_are_outside_the_bound(slip, dtype):
    # F < 8: a frame past the end exists to be counted twice; H >= 9: a second chunk group; S >= 2: a next token;
    # a padded val row: the two row strides differ
    inp = _padded_val(to.make_inputs(2, 6, 3, 9, dtype, seed=3))
    assert inp.val.stride(2) != inp.k2.stride(2)
    res = fo.outside(fo.emulate_fp32(inp, slip), fo.reference(inp), dtype)
    print(slip, dtype, res)
    hit = {"last_frame_twice": ("out", "tattn"), "no_scale": ("out", "tattn"), "p_rounded_twice": ("out", "tattn"),
           "tattn_frames_of_next_token": ("tattn",)}.get(slip, ("out",))
    for n in hit:
        assert res[n][0] > 0, f"{slip}: {n} stayed inside the bound (worst {res[n][1]:.3f})"
    for n in {"out", "tattn"} - set(hit):
        assert res[n][0] == 0, f"{slip}: {n} should not be affected (worst {res[n][1]:.3f})"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_three_slips_show_only_at_the_shapes_the_gpu_test_adds(dtype):
    """Why the GPU test runs every F, H = 8 and 9 and a padded val: at F = 8, H = 8 and equal row strides the masking,
    group and stride slips change nothing; one frame less, a ninth head or a padded row shows each."""
    inp = to.make_inputs(2, 6, 8, 8, dtype, seed=3)  # eight frames, eight heads, val's row stride = k2's
    right = fo.emulate_fp32(inp)
    for slip in ("second_group_reads_first", "val_with_k_row_stride", "last_frame_twice"):
        wrong = fo.emulate_fp32(inp, slip)
        assert torch.equal(wrong["out"], right["out"]) and torch.equal(wrong["tattn"], right["tattn"]), slip
    inp = to.make_inputs(2, 6, 7, 9, dtype, seed=3)
    ref = fo.reference(inp)
    assert fo.outside(fo.emulate_fp32(_padded_val(inp), "val_with_k_row_stride"), ref, dtype)["out"][0] > 0
    assert fo.outside(fo.emulate_fp32(inp, "second_group_reads_first"), ref, dtype)["out"][0] > 0
    assert fo.outside(fo.emulate_fp32(inp, "last_frame_twice"), ref, dtype)["out"][0] > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("slip", fo.SHORT_SLIPS)
def test_wrong_short_attentions_are_outside_the_bound(slip, dtype):
    # N < 8: keys past the end exist to be counted; H >= 2: heads to swap; a padded v row: its strides are not k's
    inp = _padded_v(so.make_inputs(4, 3, 5, dtype, 11, layout="qkv"))
    assert inp.v.stride(2) != inp.k.stride(2)
    res = fo.outside(fo.emulate_fp32(inp, slip), fo.reference(inp), dtype)
    print(slip, dtype, res)
    assert res["out"][0] > 0, f"{slip}: out stayed inside the bound (worst {res['out'][1]:.3f})"
