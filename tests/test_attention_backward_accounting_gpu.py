"""Every key, query and head accounted for in the attention backward (tome_prop_attention_backward and
tome_prop_attention_segments_backward: k_attn_bwd_dq / k_attn_bwd_dkv, csrc/tome_attn_bwd.h) on inputs whose softmax is
known (tests/attn_bwd_accounting.py): q = 0 or k = 0 makes every logit the bias, the q~ term leaves the unchanged bound
of attn_bwd_oracle.py, and a single key missing from dq or a single query missing from dk or dv moves an element by
several bounds (test_attn_bwd_accounting_cpu.py proves that for every shape below, on any machine).  The reference is
the fp64 autograd of attn_bwd_oracle / segment_attn_bwd_oracle, computed on the CPU; where the bound is 0 -- all of dk
in family K, all of dq in family Q -- the kernels' value must be exactly 0.

Shapes around the lane half (32), the key / query tile (64) and the workgroup block (128) with N = Nk, one query
against many keys and many against one, B*H of 9, 17 and 24 (the item map's later rounds of 8 and its padded
workgroups), NaN-prefilled strided targets, strided dout / out / log_bias, the segmented form, and a qkv and a
gradient buffer of more than 2^31 elements each."""
import pytest
import torch

import attn_bwd_accounting as aa
import attn_bwd_oracle as ao
import segment_attn_bwd_oracle as so

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = (torch.bfloat16, torch.float16)
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}
GRADS = ("dq", "dk", "dv")


def _abi():
    import tome  # noqa: F401
    from tome import _abi
    return _abi


def _to_dev(inp: ao.Inputs) -> ao.Inputs:
    if inp.qkv is not None:
        qkv = inp.qkv.to(DEV)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    else:
        qkv, q, k, v = None, inp.q.to(DEV), inp.k.to(DEV), inp.v.to(DEV)
    lb = None if inp.log_bias is None else inp.log_bias.to(DEV)
    return ao.Inputs(q, k, v, inp.dout.to(DEV), lb, inp.skip, inp.scale, qkv)


def _native(_a, d: ao.Inputs, out=None, **kw):
    """Forward launch + backward launch on the device inputs -> dict of [B, H, *, 64] gradients."""
    if out is None:
        out = _a.prop_attention(d.q, d.k, d.v, None, d.scale, bias_skip=d.skip, log_bias=d.log_bias)
    dq, dk, dv = _a.prop_attention_backward(d.q, d.k, d.v, out, d.dout, d.log_bias, d.scale, bias_skip=d.skip, **kw)
    return dict(dq=dq, dk=dk, dv=dv)


def _id(c):
    return "x".join(str(x) for x in c)


def _plain(_a, B, H, N, Nk, kind, encs=aa.ENCODINGS):
    """Every bias form the shape admits, both formats, the separate tensors and (N == Nk) the slices of one qkv buffer;
    one fp64 reference per (encoding, bias form) -- the inputs are exact in both formats."""
    for enc in encs:
        for bias in aa.biases_for(N, Nk):
            ref = None
            for dtype in DTYPES:
                sep, qkv = aa.make_family(kind, B, H, N, Nk, dtype, bias, enc, seed=N + Nk)
                ref = ref or ao.reference(sep)
                bnd = ao.bounds(ref, dtype)
                for inp, layout in ((sep, "separate"), (qkv, "qkv")):
                    if inp is None:
                        continue
                    got = _native(_a, _to_dev(inp))
                    torch.cuda.synchronize()
                    aa.check(f"family {kind} {B}x{H}x{N}x{Nk} {enc} {bias} {layout} {NAME[dtype]}", got, ref, bnd)


@pytest.mark.parametrize("enc", aa.ENCODINGS)
@pytest.mark.parametrize("kind", aa.KINDS)
@pytest.mark.parametrize("shape", aa.PLAIN_SHAPES, ids=_id)
def test_every_key_and_query_counted(shape, kind, enc):
    """Family K: dq counts the keys of every row, dk is exactly 0.  Family Q: dk counts the queries of every key, dq
    is exactly 0.  dv counts the queries in both."""
    _plain(_abi(), *aa.PLAIN_BH, *shape, kind, (enc,))


@pytest.mark.parametrize("kind", aa.KINDS)
@pytest.mark.parametrize("shape", aa.HEAD_SHAPES, ids=_id)
@pytest.mark.parametrize("heads", aa.HEADS, ids=_id)
def test_every_head_counted(heads, shape, kind):
    """B*H = 9, 17, 24: items past the first round of 8 workgroups per block, and the padded workgroups of a B*H that is
    no multiple of 8.  The channel rotation 7b + 3h puts another head's data into the wrong channels."""
    _plain(_abi(), *heads, *shape, kind)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", aa.TARGET_SHAPES, ids=_id)
def test_strided_targets_hold_every_row_and_nothing_else(shape, dtype):
    """The gradients written into NaN-prefilled [B, max(N, Nk) + 2, 3, H, 72] buffers (a spare row before and after,
    8 spare channels): the same bits as fresh targets, inside the bound, everything outside the owned rows and 64
    channels still NaN."""
    _a = _abi()
    B, H = aa.PLAIN_BH
    N, Nk = shape
    for kind in aa.KINDS:
        sep, _ = aa.make_family(kind, B, H, N, Nk, dtype, "bias", "mod", seed=N + Nk)
        d = _to_dev(sep)
        fresh = _native(_a, d)
        buf = torch.full((B, max(N, Nk) + 2, 3, H, 72), float("nan"), dtype=dtype, device=DEV)
        g = buf.permute(2, 0, 3, 1, 4)
        rows = (N, Nk, Nk)
        got = _native(_a, d, grads=tuple(g[i][:, :, 1:1 + rows[i], :64] for i in range(3)))
        torch.cuda.synchronize()
        outside = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
        for i, n in enumerate(GRADS):
            assert got[n].data_ptr() == g[i][:, :, 1:, :64].data_ptr()
            assert torch.equal(got[n], fresh[n]), f"{n}: strided target differs from a fresh one"
            outside[:, 1:1 + rows[i], i, :, :64] = False
        assert bool(torch.isnan(buf[outside]).all()), "written outside the owned rows and channels"
        ref = ao.reference(sep)
        aa.check(f"targets {kind} {_id(shape)} {NAME[dtype]}", got, ref, ao.bounds(ref, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", aa.STRIDE_SHAPES, ids=_id)
def test_strided_dout_out_and_log_bias(shape, dtype):
    """dout and out as [B, N, H*64] views of wider buffers (a spare row before and after, 8 spare channels; rows 16-byte
    aligned, so the entry reads them in place) and log_bias a [B, nb] view of [B, nb + 16]: the same bits as the
    contiguous call, inside the bound."""
    _a = _abi()
    B, H = aa.PLAIN_BH
    N, Nk = shape
    for kind in aa.KINDS:
        for bias in aa.biases_for(N, Nk):
            sep, _ = aa.make_family(kind, B, H, N, Nk, dtype, bias, "mod", seed=N + Nk)
            d = _to_dev(sep)
            out = _a.prop_attention(d.q, d.k, d.v, None, d.scale, bias_skip=d.skip, log_bias=d.log_bias)
            plain = _native(_a, d, out=out)

            def wide(t):
                w = torch.full((B, N + 2, H * 64 + 8), 3.0, dtype=dtype, device=DEV)
                view = w[:, 1:N + 1, :H * 64]
                view.copy_(t)
                assert not view.is_contiguous()
                assert _a._grad_rows("test", view, "rows", (B, N, H * 64), d.q).data_ptr() == view.data_ptr(), "copied"
                return view

            lb = d.log_bias
            if lb is not None:
                nb = lb.shape[1]
                lbw = torch.full((B, nb + 16), 9.0, device=DEV)
                lbw[:, :nb] = lb
                lb = lbw[:, :nb]
                assert lb.stride(0) == nb + 16
            ds = ao.Inputs(d.q, d.k, d.v, wide(d.dout), lb, d.skip, d.scale, None)
            got = _native(_a, ds, out=wide(out))
            torch.cuda.synchronize()
            for n in GRADS:
                assert torch.equal(got[n], plain[n]), f"{n}: strided dout / out / log_bias differ from the contiguous call"
            ref = ao.reference(sep)
            aa.check(f"strides {kind} {_id(shape)} {bias} {NAME[dtype]}", got, ref, ao.bounds(ref, dtype))


def _seg_to_dev(inp: so.Inputs) -> so.Inputs:
    if inp.qkv is not None:
        qkv = inp.qkv.to(DEV)
        q, k, v = (qkv[:, 1:, i].permute(0, 2, 1, 3) for i in range(3))
    else:  # (the permuted views keep their strides on the device)
        qkv, q, k, v = None, inp.q.to(DEV), inp.k.to(DEV), inp.v.to(DEV)
    lb = None if inp.log_bias is None else inp.log_bias.to(DEV)
    return so.Inputs(q, k, v, inp.dy.to(DEV), lb, inp.nseg, inp.scale, qkv)


SEG_CASES = [c + ("separate",) for c in aa.SEGMENTS] + [c + ("qkv",) for c in aa.SEGMENTS_QKV]


@pytest.mark.parametrize("kind", aa.KINDS)
@pytest.mark.parametrize("case", SEG_CASES, ids=_id)
def test_segments_every_key_and_query_counted(case, kind):
    """The segmented form: dq sums the segments' keys (family K), dk and dv count the queries per segment; every
    segment's keys and dy carry a rotation of their own, so exchanged segments show."""
    _a = _abi()
    B, H, N, P, nseg, layout = case
    for enc in aa.ENCODINGS:
        for bias in ("none", "bias"):
            ref = None
            for dtype in DTYPES:
                inp = aa.make_segment_family(kind, B, H, N, P, nseg, dtype, bias, enc, seed=N + P, layout=layout)
                d = _seg_to_dev(inp)
                y = _a.prop_attention_segments(d.q, d.k, d.v, d.nseg, d.scale, log_bias=d.log_bias)
                dq, dk, dv = _a.prop_attention_segments_backward(d.q, d.k, d.v, y, d.dy, d.nseg, d.scale,
                                                                 log_bias=d.log_bias)
                torch.cuda.synchronize()
                ref = ref or so.reference(inp)
                aa.check(f"segments family {kind} {_id(case)} {enc} {bias} {NAME[dtype]}", dict(dq=dq, dk=dk, dv=dv), ref,
                         so.bounds(ref, dtype))


def test_counts_beyond_2_31_elements():
    """A bf16 qkv buffer [3700, 257, 3, 12, 64] and a NaN-prefilled gradient buffer of the same shape (2.2e9 elements
    each: batch offsets past 2^31), family K, "mod", no bias: three query blocks, five key tiles.  The expectation is the
    fp64 reference and bound of the 64 distinct rotations (7b + 3h) mod 64, computed once at B = 64, H = 1 and gathered
    per (batch, head); compared in batch chunks on the device.  A read or write at a wrapped 32-bit offset lands in
    another slice -- other channels -- or leaves NaN behind."""
    _a = _abi()
    B, N, H, dtype = 3700, 257, 12, torch.bfloat16
    small, _ = aa.make_family("K", 64, 1, N, N, dtype, "none", "mod")
    ref = ao.reference(small)
    bnd = ao.bounds(ref, dtype)
    ref_d = {n: ref[n][:, 0].to(DEV) for n in GRADS}   # [64, N, 64]: entry b0 has the rotation 7 b0 mod 64
    bnd_d = {n: bnd[n][:, 0].to(DEV) for n in GRADS}
    d = aa.make_family_qkv("K", B, H, N, dtype, "none", "mod", device=DEV)
    assert d.qkv.numel() > 2 ** 31
    out = _a.prop_attention(d.q, d.k, d.v, None, d.scale)
    gbuf = torch.full((B, N, 3, H, 64), float("nan"), dtype=dtype, device=DEV)
    g = gbuf.permute(2, 0, 3, 1, 4)
    _a.prop_attention_backward(d.q, d.k, d.v, out, d.dout, None, d.scale, grads=(g[0], g[1], g[2]))
    torch.cuda.synchronize()
    worst = dict.fromkeys(GRADS, 0.0)
    step = 100
    for lo in range(0, B, step):
        hi = min(lo + step, B)
        rot = aa.rotation(hi - lo, H, DEV, extra=7 * lo) % 64
        b0 = (rot * 55) % 64                              # 7 * 55 = 1 mod 64
        for i, n in enumerate(GRADS):
            r = aa.ratios(g[i][lo:hi].double(), ref_d[n][b0], bnd_d[n][b0])
            worst[n] = max(worst[n], float(r.max()))
            assert worst[n] <= 1.0, f"batches {lo}..{hi - 1}: {n} is {worst[n]:.3f}x its bound somewhere"
    print("beyond 2^31 family K mod none bf16: worst error / bound  " + "  ".join(f"{n} {worst[n]:.3f}" for n in GRADS))
    del d, out, gbuf, g
    torch.cuda.empty_cache()
