"""The bound of attn_bwd_oracle.py, checked without a GPU: a torch emulation of the backward kernels' arithmetic (q~, P
and dS as operands, the stored O and the outputs rounded to the 16-bit format) stays inside it on every input family the
GPU tests use, and each of the wrong answers a backward kernel could plausibly give falls outside it.  No element of any
output is exempt: attn_bwd_oracle.worst takes the maximum over all of dq, dk and dv."""
import pytest
import torch

import attn_bwd_oracle as ao

DTYPES = [torch.bfloat16, torch.float16]

# (B, H, N, Nk, bias, layout, logit_gain, max_size[, offset]): the GPU tests' families at sizes a CPU evaluates quickly
FAMILIES = [
    (2, 2, 8, 8, "bias", "qkv", 1.0, 8),
    (1, 2, 63, 63, "none", "separate", 1.0, 8),
    (1, 2, 65, 65, "skip", "qkv", 1.0, 8),
    (2, 2, 197, 197, "skip", "qkv", 1.0, 8),
    (1, 2, 197, 197, "bias", "separate", 1.0, 8),
    (1, 3, 1, 197, "bias", "separate", 1.0, 8),
    (1, 2, 392, 196, "bias", "separate", 1.0, 8),
    (1, 2, 197, 197, "bias", "qkv", 8.0, 64),
    (1, 1, 392, 392, "none", "qkv", 8.0, 64),
    (1, 2, 197, 197, "bias", "qkv", 1.0, 8, 2.0),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: "-".join(str(x) for x in f))
def test_emulation_inside_bound(fam, dtype):
    B, H, N, Nk, bias, layout, gain, ms = fam[:8]
    inp = ao.make_inputs(B, H, N, Nk, dtype, 11, bias=bias, layout=layout, logit_gain=gain, max_size=ms,
                         offset=fam[8] if len(fam) > 8 else 0.0)
    ref = ao.reference(inp)
    ao.check(f"emulation {fam} {dtype}", ao.emulate(inp), ref, ao.bounds(ref, dtype))


def test_reference_is_the_reference_op_sequence():
    """fp64 autograd of softmax(q scale k^T + log size) v against the closed form dV = P^T dO, dS = P (dP - delta)."""
    inp = ao.make_inputs(1, 2, 37, 37, torch.bfloat16, 3, bias="skip", layout="qkv")
    ref = ao.reference(inp)
    P, g, v, q, k = ref["P"], ref["g"], ref["v"], ref["q"], ref["k"]
    dP = g @ v.transpose(-2, -1)
    dS = P * (dP - (g * ref["out"]).sum(-1, keepdim=True))
    assert torch.allclose(ref["dv"], P.transpose(-2, -1) @ g, rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref["dq"], inp.scale * dS @ k, rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref["dk"], inp.scale * dS.transpose(-2, -1) @ q, rtol=1e-12, atol=1e-12)
    # the skip form: query 0 and key 0 carry no bias
    beta = ao.bias_matrix(inp.log_bias, True, 37, 37)
    assert float(beta[:, :, 0].abs().max()) == 0.0 and float(beta[:, :, :, 0].abs().max()) == 0.0
    assert torch.equal(beta[0, 0, 5, 1:], inp.log_bias[0].double())


# Each slip on a family where it is a different function of the inputs: the bias slips need a bias, the dropped tile a
# row with more than 128 keys, the stale rows a partial last query tile, the exchanged heads two heads.
SLIP_FAMILY = {
    "delta_omitted": (1, 2, 197, 197, "bias", "qkv", 1.0, 8, 2.0),  # (v and dout with a mean: delta is large)
    "bias_ignored": (1, 2, 197, 197, "bias", "qkv", 1.0, 8),
    "bias_shifted": (1, 2, 197, 197, "bias", "qkv", 1.0, 8),
    "tile_dropped": (1, 2, 197, 197, "bias", "qkv", 1.0, 8),
    "stale_rows": (1, 2, 197, 197, "bias", "qkv", 1.0, 8),
    "scale_missing": (1, 2, 197, 197, "bias", "qkv", 1.0, 8),
    "heads_exchanged": (1, 2, 197, 197, "bias", "qkv", 1.0, 8),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("slip", ao.SLIPS)
def test_bound_rejects_wrong_answers(slip, dtype):
    fam = SLIP_FAMILY[slip]
    B, H, N, Nk, bias, layout, gain, ms = fam[:8]
    inp = ao.make_inputs(B, H, N, Nk, dtype, 5, bias=bias, layout=layout, logit_gain=gain, max_size=ms,
                         offset=fam[8] if len(fam) > 8 else 0.0)
    ref = ao.reference(inp)
    bnd = ao.bounds(ref, dtype)
    right = ao.worst(ao.emulate(inp), ref, bnd)
    wrong = ao.worst(ao.emulate(inp, slip=slip), ref, bnd)
    print(f"{slip} {dtype}: right {right}, wrong {wrong}")
    assert max(right.values()) <= 1.0
    assert max(wrong.values()) > 1.0, f"{slip}: every element still inside its bound ({wrong})"


def test_bound_covers_every_element():
    """A single wrong element anywhere -- first or last row, any channel -- is found: nothing is masked or sampled."""
    dtype = torch.bfloat16
    inp = ao.make_inputs(1, 2, 65, 65, dtype, 9, bias="bias", layout="qkv")
    ref = ao.reference(inp)
    bnd = ao.bounds(ref, dtype)
    good = ao.emulate(inp)
    for name in ("dq", "dk", "dv"):
        for idx in ((0, 0, 0, 0), (0, 1, 64, 63), (0, 0, 33, 17)):
            bad = {n: t.clone() for n, t in good.items()}
            bad[name][idx] += 4 * float(bnd[name][idx]) + 1e-3
            assert ao.worst(bad, ref, bnd)[name] > 1.0
        bad = {n: t.clone() for n, t in good.items()}
        bad[name][0, 0, 1, 1] = float("nan")
        assert ao.worst(bad, ref, bnd)[name] == float("inf")
