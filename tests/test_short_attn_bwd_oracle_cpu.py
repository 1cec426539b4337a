"""tests/short_attn_bwd_oracle.py on the CPU: the derived bound accepts an fp32 evaluation of the kernel's formula, in
both dtypes and at every sequence length, and rejects each wrong answer such a kernel can give."""
import pytest
import torch

import short_attn_bwd_oracle as so

DTYPES = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_fp32_emulation_is_inside_the_bound(dtype):
    for N in range(1, 9):
        for layout, gain in (("qkv", 1.0), ("separate", 8.0)):
            inp = so.make_inputs(5, 3, N, dtype, 100 + N, layout=layout, logit_gain=gain)
            so.check(f"N={N} {layout} gain={gain} {dtype}", so.emulate_fp32(inp), so.reference(inp), dtype)


def test_reference_is_autograd_of_the_framework_attention():
    inp = so.make_inputs(2, 3, 8, torch.bfloat16, 5)
    ref = so.reference(inp)
    q, k, v = (t.detach().double().requires_grad_(True) for t in (inp.q, inp.k, inp.v))
    out = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=inp.scale).transpose(1, 2).reshape(2, 8, 192)
    out.backward(inp.dout.double())
    for n, t in (("dq", q), ("dk", k), ("dv", v)):
        assert torch.allclose(ref[n], t.grad, rtol=1e-12, atol=1e-14), n


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("slip", so.SLIPS)
def test_wrong_answers_are_outside_the_bound(slip, dtype):
    N = 5 if slip == "masked_keys_counted" else 8
    inp = so.make_inputs(4, 3, N, dtype, 11, layout="qkv")
    ref = so.reference(inp)
    res = so.outside(so.emulate_fp32(inp, slip), ref, dtype)
    hit = {n for n in res if res[n][0]}
    print(slip, dtype, res)
    want = {"no_delta": {"dq", "dk"}, "no_scale": {"dq", "dk"}, "masked_keys_counted": {"dq", "dk", "dv"},
            "query_row_dropped": {"dk", "dv"}, "heads_swapped": {"dq", "dk", "dv"}, "p_rounded_twice": {"dv"},
            "dout_with_q_strides": {"dq", "dk", "dv"}}[slip]
    assert want <= hit, (slip, res)
