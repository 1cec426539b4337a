"""tome_prop_attention_segments_backward on the GPU: every element of dq, dk, dv inside the component-wise bound of
segment_attn_bwd_oracle.py (fp64 gradient of the reference's op sequence), and the kernels' properties: one rounding of
the summed dq, every element written once and nothing beside the 64 channels, same bits on every run, nseg = 1 equal to
tome_prop_attention_backward, refusals that launch nothing."""
import ctypes

import pytest
import torch

import segment_attn_bwd_oracle as so

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]


def _abi():
    import tome  # noqa: F401
    from tome import _abi
    return _abi


def _to_dev(inp: so.Inputs) -> so.Inputs:
    if inp.qkv is not None:
        qkv = inp.qkv.to(DEV)
        q, k, v = (qkv[:, 1:, i].permute(0, 2, 1, 3) for i in range(3))
    else:  # (the permuted views keep their strides on the device)
        qkv, q, k, v = None, inp.q.to(DEV), inp.k.to(DEV), inp.v.to(DEV)
    lb = None if inp.log_bias is None else inp.log_bias.to(DEV)
    return so.Inputs(q, k, v, inp.dy.to(DEV), lb, inp.nseg, inp.scale, qkv)


def _native(_abi, d: so.Inputs, **kw):
    y = _abi.prop_attention_segments(d.q, d.k, d.v, d.nseg, d.scale, log_bias=d.log_bias)
    dq, dk, dv = _abi.prop_attention_segments_backward(d.q, d.k, d.v, y, d.dy, d.nseg, d.scale, log_bias=d.log_bias, **kw)
    return dict(dq=dq, dk=dk, dv=dv)


# (B, H, N, P, nseg, bias, layout): every N of {1, 31, 128, 129, 197}, P of {1, 63, 64, 65, 129, 196}, nseg of {1, 2, 8},
# (B, H) of {(1, 1), (1, 3), (2, 12)}; N != nseg * P except in the qkv layout, which needs them equal
CASES = [
    (1, 1, 1, 1, 1, True, "separate"),
    (1, 3, 31, 63, 2, True, "separate"),
    (2, 12, 128, 64, 2, False, "qkv"),
    (1, 3, 129, 65, 2, True, "separate"),
    (1, 1, 197, 129, 1, False, "separate"),
    (1, 3, 31, 196, 2, True, "separate"),
    (1, 1, 128, 1, 8, True, "separate"),
    (1, 3, 504, 63, 8, True, "qkv"),
    (2, 12, 129, 64, 1, True, "separate"),
    (1, 1, 197, 65, 8, False, "separate"),
    (1, 3, 1, 129, 2, False, "separate"),
    (1, 1, 392, 196, 2, True, "qkv"),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(x) for x in c[:5]) + ("b" if c[5] else "") + c[6][0])
def test_gradients_inside_the_bound(case, dtype):
    _a = _abi()
    B, H, N, P, nseg, bias, layout = case
    inp = so.make_inputs(B, H, N, P, nseg, dtype, seed=N + P + nseg, bias=bias, layout=layout)
    d = _to_dev(inp)
    # NaN-filled targets of the projection's layout: every element the kernels own is written, nothing beside it
    K = nseg * P
    pad = torch.full((B, max(N, K), 3, H, 80), float("nan"), dtype=dtype, device=DEV)
    g = pad.permute(2, 0, 3, 1, 4)[..., :64]
    got = _native(_a, d, grads=(g[0][:, :, :N], g[1][:, :, :K], g[2][:, :, :K]))
    torch.cuda.synchronize()
    ref = so.reference(inp)
    so.check(f"segments {case} {dtype}", got, ref, so.bounds(ref, dtype))
    assert bool(pad[..., 64:].isnan().all()), "memory beside the 64 channels was written"
    assert bool(pad[:, N:, 0].isnan().all()) and bool(pad[:, K:, 1:].isnan().all()), "rows past the end were written"
    # three separate fresh targets: the same bits
    again = _native(_a, d)
    for n in got:
        assert torch.equal(again[n], got[n]), f"{n}: one buffer and three differ / bits differ between two runs"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_gradients_where_the_row_maximum_matters(dtype):
    """Logits 8x larger with sizes up to 64; and a common mean in v and dy (delta large against dP - delta)."""
    _a = _abi()
    for kw in (dict(logit_gain=8.0, max_size=64), dict(offset=2.0)):
        inp = so.make_inputs(1, 3, 130, 65, 2, dtype, seed=9, bias=True, layout="qkv", **kw)
        got = _native(_a, _to_dev(inp))
        torch.cuda.synchronize()
        ref = so.reference(inp)
        so.check(f"segments {kw} {dtype}", got, ref, so.bounds(ref, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_dq_is_summed_in_fp32_and_rounded_once(dtype):
    """The case whose roundings are all exact (segment_attn_bwd_oracle.exact_inputs): bit-equal to the reference."""
    _a = _abi()
    inp = so.exact_inputs(dtype)
    got = _native(_a, _to_dev(inp))
    torch.cuda.synchronize()
    ref = so.reference(inp)
    assert torch.equal(got["dq"].double().cpu(), ref["dq"]), (got["dq"].double().cpu() - ref["dq"]).abs().max()
    assert torch.equal(got["dv"].double().cpu(), ref["dv"]) and float(got["dk"].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_one_segment_without_bias_is_the_plain_backward(dtype):
    _a = _abi()
    for N, P in ((197, 197), (31, 129)):
        d = _to_dev(so.make_inputs(2, 3, N, P, 1, dtype, seed=5, bias=False))
        got = _native(_a, d)
        out = _a.prop_attention(d.q, d.k, d.v, None, d.scale)
        dq, dk, dv = _a.prop_attention_backward(d.q, d.k, d.v, out, d.dy[:, :, 0], None, d.scale)
        assert torch.equal(got["dq"], dq) and torch.equal(got["dk"], dk) and torch.equal(got["dv"], dv)


def test_workspace_and_refusals_launch_nothing(monkeypatch):
    _a = _abi()
    L = _a.lib()
    B, H, N, P, nseg = 1, 2, 40, 20, 2
    d = _to_dev(so.make_inputs(B, H, N, P, nseg, torch.bfloat16, seed=2, layout="qkv"))
    base = _native(_a, d)
    need = L.tome_prop_attention_segments_backward_workspace_bytes(B, H, N, P, nseg)
    assert need >= 2 * 4 * nseg * B * H * N and need % 256 == 0
    assert L.tome_prop_attention_segments_backward_workspace_bytes(B, H, N, P, 0) == 0
    guard = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    e = _native(_a, d, workspace=guard[:need])
    torch.cuda.synchronize()
    assert bool((guard[need:] == 0x5A).all()), "wrote past workspace_bytes"
    assert all(torch.equal(base[n], e[n]) for n in base)

    y = _a.prop_attention_segments(d.q, d.k, d.v, nseg, d.scale, log_bias=d.log_bias)
    s3 = lambda t: (ctypes.c_int64 * 3)(*t.stride()[:3])  # noqa: E731
    tgt = [torch.full((B, n, H, 64), float("nan"), dtype=torch.bfloat16, device=DEV).permute(0, 2, 1, 3)
           for n in (N, nseg * P, nseg * P)]
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call(**o):
        a = dict(dtype=1, D=64, nseg=nseg, ws=ws.data_ptr(), ws_bytes=need, dq=tgt[0].data_ptr(), kstep=P * d.k.stride(2),
                 ystr=(ctypes.c_int64 * 3)(y.stride(0), 64, y.stride(1)))
        a.update(o)
        return L.tome_prop_attention_segments_backward(
            d.q.data_ptr(), d.k.data_ptr(), d.v.data_ptr(), y.data_ptr(), d.dy.data_ptr(), a["dtype"], B, H, N, P, a["D"],
            s3(d.q), s3(d.k), s3(d.v), a["ystr"], (ctypes.c_int64 * 3)(d.dy.stride(0), 64, d.dy.stride(1)),
            d.log_bias.data_ptr(), d.log_bias.stride(0), 0.125, a["nseg"],
            (ctypes.c_int64 * 4)(a["kstep"], P * d.v.stride(2), y.stride(2), P),
            (ctypes.c_int64 * 3)(d.dy.stride(2), P * tgt[1].stride(2), P * tgt[2].stride(2)), a["dq"], tgt[1].data_ptr(),
            tgt[2].data_ptr(), s3(tgt[0]), s3(tgt[1]), s3(tgt[2]), a["ws"], a["ws_bytes"], None)

    EINVAL, EWORKSPACE = 1, 2
    assert call(ws=None) == EWORKSPACE and call(ws_bytes=need - 256) == EWORKSPACE
    assert call(dtype=0) == EINVAL          # fp32 heads
    assert call(D=32) == EINVAL             # head dim
    assert call(nseg=0) == EINVAL
    assert call(dq=None) == EINVAL
    assert call(kstep=P * d.k.stride(2) + 4) == EINVAL       # a segment offset that breaks the rows' alignment
    assert call(ystr=(ctypes.c_int64 * 3)(y.stride(0), 64, 60)) == EINVAL
    assert call(ws=ws.data_ptr() + 4) == EINVAL
    assert b"tome_prop_attention_segments_backward" in L.tome_last_error()
    torch.cuda.synchronize()
    assert all(bool(t.isnan().all()) for t in tgt), "a refused call wrote to its targets"
    assert call() == 0
    torch.cuda.synchronize()
    assert all(torch.equal(t, base[n]) for t, n in zip(tgt, ("dq", "dk", "dv")))
    # the wrapper's own refusals
    with pytest.raises(_a.TomeHipError):
        _a.prop_attention_segments_backward(d.q, d.k, d.v, y, d.dy, 3, d.scale)             # 40 keys, 3 segments
    with pytest.raises(_a.TomeHipError):
        _a.prop_attention_segments_backward(d.q.float(), d.k.float(), d.v.float(), y, d.dy, nseg, d.scale)
    with pytest.raises(_a.TomeHipError, match="status 2"):
        _native(_a, d, workspace=guard[:need - 256])
