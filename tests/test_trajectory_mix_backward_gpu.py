"""tome_trajectory_mix_backward on the GPU: every element of dq2, dk2, dval inside the component-wise bound of
traj_mix_bwd_oracle.py (fp64 gradient of the reference's op sequence), in every layout the patched block produces, and
the kernel's properties: every element written once and nothing beside a row's channels, same bits on every run,
unwanted gradients not computed, refusals that launch nothing."""
import pytest
import torch

import traj_mix_bwd_oracle as to

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
NAN = float("nan")


def _abi():
    import tome  # noqa: F401
    from tome import _abi
    return _abi


def _layout(inp: to.Inputs, layout: str):
    """Device tensors (q2, k2, val, dout) in one of the layouts of tome/patch/motionformer.py:
    separate  k2 and val tensors of their own, dout contiguous
    halves    k2 and val the two halves of one [B, S, F, 2C] proj_kv output; dout rows 1.. of a [B, 1+S, C] gradient
    tokens    val = the trajectory tokens (a tensor of its own, use_original_code), k2 of its own; dout sliced likewise"""
    q2, k2, val, dout = (t.to(DEV) for t in (inp.q2, inp.k2, inp.val, inp.dout))
    B, S, C = q2.shape
    if layout == "halves":
        kv = torch.cat((k2, val), dim=-1)
        k2, val = kv[..., :C], kv[..., C:]
    if layout != "separate":
        joined = torch.zeros(B, 1 + S, C, dtype=q2.dtype, device=DEV)
        joined[:, 1:] = dout
        dout = joined[:, 1:]
    return q2, k2, val, dout


def _targets(B, S, F, C, dtype, one_buffer: bool):
    """NaN-filled targets with a margin of 16 elements behind every row (and between the halves of one buffer)."""
    dq2 = torch.full((B, S, C), NAN, dtype=dtype, device=DEV)
    if one_buffer:
        buf = torch.full((B, S, F, 2 * (C + 16)), NAN, dtype=dtype, device=DEV)
        return dq2, buf[..., :C], buf[..., C + 16:2 * C + 16], [buf[..., C:C + 16], buf[..., 2 * C + 16:]]
    bk, bv = (torch.full((B, S, F, C + 16), NAN, dtype=dtype, device=DEV) for _ in range(2))
    return dq2, bk[..., :C], bv[..., :C], [bk[..., C:], bv[..., C:]]


# (B, S, F, H, layout, one target buffer): B*S of {1, 5, 1031}, H of {1, 8, 9, 12, 16}, F of {1, 3, 8}
CASES = [
    (1, 1, 1, 1, "separate", False),
    (1, 5, 3, 8, "halves", True),
    (5, 1, 8, 9, "tokens", False),
    (1, 1031, 8, 12, "halves", True),
    (1, 5, 3, 16, "tokens", True),
    (1031, 1, 1, 9, "separate", False),
    (1, 5, 8, 1, "halves", False),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(x) for x in c[:4]) + c[4][0] + ("1" if c[5] else "3"))
def test_gradients_inside_the_bound(case, dtype):
    _a = _abi()
    B, S, F, H, layout, one = case
    inp = to.make_inputs(B, S, F, H, dtype, seed=S + F + H)
    q2, k2, val, dout = _layout(inp, layout)
    C = H * 64
    dq2, dk2, dval, margins = _targets(B, S, F, C, dtype, one)
    got = dict(zip(to.OUTPUTS, _a.trajectory_mix_backward(q2, k2, val, dout, H, inp.scale, grads=(dq2, dk2, dval))))
    torch.cuda.synchronize()
    assert got["dk2"].data_ptr() == dk2.data_ptr() and got["dval"].data_ptr() == dval.data_ptr()
    to.check(f"mix {case} {dtype}", got, to.reference(inp), dtype)
    assert all(bool(m.isnan().all()) for m in margins), "memory beside a row's channels was written"
    # fresh targets, a second run: the same bits
    again = dict(zip(to.OUTPUTS, _a.trajectory_mix_backward(q2, k2, val, dout, H, inp.scale)))
    for n in got:
        assert torch.equal(again[n], got[n]), f"{n}: bits differ between two runs / targets"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rows_whose_maximum_logit_dominates(dtype):
    _a = _abi()
    inp = to.make_inputs(2, 7, 8, 12, dtype, seed=11, logit_gain=8.0)
    q2, k2, val, dout = _layout(inp, "halves")
    got = dict(zip(to.OUTPUTS, _a.trajectory_mix_backward(q2, k2, val, dout, 12, inp.scale)))
    torch.cuda.synchronize()
    ref = to.reference(inp)
    assert float(ref["P"].amax(-1).median()) > 0.5, "the case is meant to have one dominant frame per row"
    to.check(f"mix gain 8 {dtype}", got, ref, dtype)


def test_val_may_be_the_tensor_whose_gradient_is_asked_and_unwanted_gradients_are_not_computed():
    _a = _abi()
    dtype = torch.bfloat16
    inp = to.make_inputs(2, 9, 4, 9, dtype, seed=13)
    q2, k2, val, dout = _layout(inp, "tokens")
    full = _a.trajectory_mix_backward(q2, k2, val, dout, 9, inp.scale)
    ref = to.reference(inp)
    to.check("mix tokens", dict(zip(to.OUTPUTS, full)), ref, dtype)
    for want_k2, want_val in ((True, False), (False, True), (False, False)):
        dq2, dk2, dval = _a.trajectory_mix_backward(q2, k2, val, dout, 9, inp.scale, want_k2=want_k2, want_val=want_val)
        assert (dk2 is None) == (not want_k2) and (dval is None) == (not want_val)
        assert torch.equal(dq2, full[0])
        assert dk2 is None or torch.equal(dk2, full[1])
        assert dval is None or torch.equal(dval, full[2])


def test_refusals_launch_nothing():
    _a = _abi()
    L = _a.lib()
    dtype = torch.bfloat16
    B, S, F, H = 1, 5, 3, 2
    C = H * 64
    inp = to.make_inputs(B, S, F, H, dtype, seed=1)
    q2, k2, val, dout = _layout(inp, "separate")
    dq2, dk2, dval, _ = _targets(B, S, F, C, dtype, False)

    def call(**o):
        a = dict(dtype=1, F=F, H=H, D=64, k_row=k2.stride(2), do_sb=0, dq2=dq2.data_ptr(), dk_row=dk2.stride(2),
                 k2=k2.data_ptr())
        a.update(o)
        return L.tome_trajectory_mix_backward(q2.data_ptr(), a["k2"], val.data_ptr(), dout.data_ptr(), a["dtype"], B, S,
                                              a["F"], a["H"], a["D"], a["k_row"], val.stride(2), a["do_sb"], 0.125,
                                              a["dq2"], dk2.data_ptr(), dval.data_ptr(), a["dk_row"], dval.stride(2), None)

    EINVAL = 1
    for bad in (dict(dtype=0), dict(F=9), dict(H=17), dict(D=32), dict(k_row=C + 4), dict(k_row=C - 8), dict(do_sb=S * C - 8),
                dict(do_sb=S * C + 4), dict(dq2=None), dict(dk_row=C - 8), dict(k2=k2.data_ptr() + 2)):
        assert call(**bad) == EINVAL, bad
        assert b"tome_trajectory_mix_backward" in L.tome_last_error()
    torch.cuda.synchronize()
    assert all(bool(t.isnan().all()) for t in (dq2, dk2, dval)), "a refused call wrote to its targets"
    assert call() == 0
    torch.cuda.synchronize()
    want = _a.trajectory_mix_backward(q2, k2, val, dout, H, 0.125)
    assert all(torch.equal(a, b) for a, b in zip((dq2, dk2, dval), want))
    # the wrapper's own refusals
    with pytest.raises(_a.TomeHipError):
        _a.trajectory_mix_backward(q2.float(), k2.float(), val.float(), dout, H, 0.125)
    with pytest.raises(_a.TomeHipError):
        _a.trajectory_mix_backward(q2, k2, val, dout[:, :4], H, 0.125)
    with pytest.raises(_a.TomeHipError):
        _a.trajectory_mix_backward(q2, k2, val, dout, H, 0.125, grads=(dq2, None, dval))
