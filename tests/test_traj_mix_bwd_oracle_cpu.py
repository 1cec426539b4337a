"""traj_mix_bwd_oracle.py on the CPU: the bound accepts an fp32 evaluation of the kernel's formula (sums in another
order than the kernel's) and rejects the wrong answers a streaming kernel of this kind can give."""
import pytest
import torch

import traj_mix_bwd_oracle as to

DTYPES = [torch.bfloat16, torch.float16]
CASES = [(1, 5, 8, 2), (2, 3, 3, 9), (1, 7, 1, 1)]  # B, S, F, H


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("gain", [1.0, 8.0])
def test_fp32_evaluation_is_inside_the_bound(dtype, gain):
    for i, (B, S, F, H) in enumerate(CASES):
        inp = to.make_inputs(B, S, F, H, dtype, seed=10 + i, logit_gain=gain)
        to.check(f"fp32 {B}x{S}x{F}x{H} gain {gain} {dtype}", to.emulate_fp32(inp), to.reference(inp), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("slip", to.SLIPS)
def test_wrong_answers_are_outside_the_bound(slip, dtype):
    B, S, F, H = 2, 6, 3, 9  # F < 8: a frame past the end exists to be counted twice; H >= 2: a neighbouring head
    inp = to.make_inputs(B, S, F, H, dtype, seed=3)
    res = to.outside(to.emulate_fp32(inp, slip), to.reference(inp), dtype)
    hit = {"no_delta": ("dq2", "dk2"), "no_scale_dk2": ("dk2",), "neighbour_head_weights": ("dval",),
           "last_frame_twice": ("dq2", "dk2", "dval"), "dval_rounded_twice": ("dval",)}[slip]
    for n in hit:
        assert res[n][0] > 0, f"{slip}: {n} stayed inside the bound (worst {res[n][1]:.3f})"
    for n in set(to.OUTPUTS) - set(hit):
        assert res[n][0] == 0, f"{slip}: {n} should not be affected (worst {res[n][1]:.3f})"

