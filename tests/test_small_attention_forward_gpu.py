"""The forwards of tome_trajectory_mix (k_trajectory_mix) and tome_short_attention (k_short_attention) on the GPU: every
element of out -- and of the mix's fp32 map -- inside the component-wise bound of small_attn_fwd_oracle.py (fp64 on the
16-bit inputs), at every frame count and sequence length, on both sides of the switch between the mix's two chunk groups
(H = 8 / 9), at the tails of a workgroup's 4 rows, a wave's 8 units and a block's 32, in every layout the models
produce and one whose val rows are not spaced like k2's, with flat rows and with rows dominated by their maximum, and
past 2^31 elements of the input buffer.  Beside the values: the same bits on every run, with and without the map and
into a slice of a larger buffer; nothing written beside the results; one key gives the value row itself."""
import pytest
import torch

import short_attn_bwd_oracle as so
import small_attn_fwd_oracle as fo
import traj_mix_bwd_oracle as to

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
GAINS = [1.0, 8.0]
GUARD = 64  # elements in front of and behind a guarded result
NAN = float("nan")
TRAJ_LAYOUTS = ("halves", "separate", "padded")


def _abi():
    import tome  # noqa: F401
    from tome import _abi
    return _abi


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------------------------------------ trajectory mix

def _traj_layout(inp: to.Inputs, layout: str):
    """Device tensors (q2, k2, val):
    halves    k2 and val the two halves of one [B, S, F, 2C] proj_kv output
    separate  val a contiguous tensor of its own, k2 the first half of a kv buffer
    padded    val a view of a [B, S, F, C + 8] buffer (its row stride is not k2's), k2 contiguous"""
    q2, k2, val = (t.to(DEV) for t in (inp.q2, inp.k2, inp.val))
    B, S, F, C = k2.shape
    if layout == "halves":
        kv = torch.cat((k2, val), dim=-1)
        return q2, kv[..., :C], kv[..., C:]
    if layout == "separate":
        kv = torch.cat((k2, torch.full_like(k2, 5.0)), dim=-1)
        return q2, kv[..., :C], val
    buf = torch.full((B, S, F, C + 8), 5.0, dtype=val.dtype, device=DEV)
    buf[..., :C] = val
    return q2, k2, buf[..., :C]


def _traj_guarded(q2, k2, val, H, scale):
    """The C entry with the map inside a NaN-filled fp32 buffer, GUARD words on each side: (out, map, guards intact)."""
    abi = _abi()
    B, S, C = q2.shape
    F = k2.shape[2]
    n = B * H * S * F
    buf = torch.full((GUARD + n + GUARD,), NAN, dtype=torch.float32, device=DEV)
    sentinel = _bits(buf).clone()
    out = torch.full((B, S, C), NAN, dtype=q2.dtype, device=DEV)
    rc = abi.lib().tome_trajectory_mix(q2.data_ptr(), k2.data_ptr(), val.data_ptr(), abi.dtype_code(q2, "q2"), B, S, F, H,
                                       64, k2.stride(2), val.stride(2), float(scale), out.data_ptr(), out.stride(0),
                                       buf[GUARD:].data_ptr(), abi._stream(q2.device))
    assert rc == 0, abi.lib().tome_last_error()
    torch.cuda.synchronize()
    words = _bits(buf)
    intact = torch.equal(words[:GUARD], sentinel[:GUARD]) and torch.equal(words[GUARD + n:], sentinel[GUARD + n:])
    return out, buf[GUARD:GUARD + n].view(B, H, S, F), intact


def _check_traj(inp: to.Inputs, layout: str, ref: dict, label: str):
    """One input in one layout: the bound on out and the map, and every property that is not a value."""
    abi = _abi()
    dtype, H = inp.q2.dtype, inp.heads
    q2, k2, val = _traj_layout(inp, layout)
    B, S, C = q2.shape
    F = k2.shape[2]
    out, attn = abi.trajectory_mix(q2, k2, val, H, inp.scale)
    assert out.shape == (B, S, C) and out.dtype == dtype and attn.shape == (B, H, S, F) and attn.dtype == torch.float32
    worst = fo.check(f"{label} {layout}", dict(out=out, tattn=attn), ref, dtype)
    # the map between guard words, through the C entry: the same bits, the guards untouched
    out_g, attn_g, intact = _traj_guarded(q2, k2, val, H, inp.scale)
    assert intact, "words beside the attention map were written"
    assert torch.equal(_bits(out_g), _bits(out)) and torch.equal(_bits(attn_g), _bits(attn)), "two calls, other bits"
    # without the map, into rows 1.. of a [B, 1 + S, C] buffer: the same bits, row 0 left alone
    joined = torch.full((B, 1 + S, C), 7.0, dtype=dtype, device=DEV)
    out2, none = abi.trajectory_mix(q2, k2, val, H, inp.scale, want_attn=False, out=joined[:, 1:])
    assert none is None and out2.data_ptr() == joined[:, 1:].data_ptr()
    assert torch.equal(_bits(joined[:, 1:].contiguous()), _bits(out)), "out differs without the map / inside a larger buffer"
    assert bool((joined[:, 0] == 7.0).all()), "the row in front of out was written"
    out3, _ = abi.trajectory_mix(q2, k2, val, H, inp.scale, want_attn=False)
    assert torch.equal(_bits(out3), _bits(out))
    if F == 1:
        assert torch.equal(_bits(out), _bits(val[:, :, 0].contiguous())), "one frame: out is val, bit for bit"
        assert bool((attn == 1.0).all()), "one frame: its weight is exactly 1"
        assert worst == dict(out=0.0, tattn=0.0)
    return worst


def _sweep_traj(B, S, F, H, dtype, seed, layouts=TRAJ_LAYOUTS, gains=GAINS):
    for gain in gains:
        inp = to.make_inputs(B, S, F, H, dtype, seed=seed, logit_gain=gain)
        ref = fo.reference(inp)  # (one reference per input, shared by its layouts)
        for layout in layouts:
            _check_traj(inp, layout, ref, f"{B}x{S}x{F}x{H} gain {gain} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("F", range(1, 9))
def test_trajectory_mix_at_every_frame_count(F, dtype):
    _sweep_traj(2, 37, F, 12, dtype, seed=100 + F)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H", [1, 2, 7, 8, 9, 12, 15, 16])
def test_trajectory_mix_on_both_sides_of_the_second_chunk_group(H, dtype):
    for F in (3, 8):
        _sweep_traj(2, 5, F, H, dtype, seed=200 + 10 * H + F)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,S", [(1, 1), (1, 3), (3, 1), (2, 2), (1, 5), (5, 1)])
def test_trajectory_mix_workgroup_tail(B, S, dtype):
    _sweep_traj(B, S, 5, 9, dtype, seed=300 + 7 * B + S)


# ------------------------------------------------------------------------------------------------ short attention

def _short_guarded(q, k, v, scale):
    """The C entry on a NaN-filled buffer with GUARD elements on each side of out: (out [B, N, H*64], guards intact)."""
    abi = _abi()
    B, H, N, D = q.shape
    n = B * N * H * D
    buf = torch.full((GUARD + n + GUARD,), NAN, dtype=q.dtype, device=DEV)
    sentinel = _bits(buf).clone()
    rc = abi.lib().tome_short_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), abi.dtype_code(q, "q"), B, H, N, D,
                                        abi._head_strides(q), abi._head_strides(k), abi._head_strides(v), float(scale),
                                        buf[GUARD:].data_ptr(), abi._stream(q.device))
    assert rc == 0, abi.lib().tome_last_error()
    torch.cuda.synchronize()
    words = _bits(buf)
    intact = torch.equal(words[:GUARD], sentinel[:GUARD]) and torch.equal(words[GUARD + n:], sentinel[GUARD + n:])
    return buf[GUARD:GUARD + n].view(B, N, H * D), intact


def _check_short(B, H, N, dtype, seed, layout, gain):
    abi = _abi()
    inp = so.make_inputs(B, H, N, dtype, seed, layout=layout, logit_gain=gain, device=DEV)
    assert abi.short_attention_ok(inp.q, inp.k, inp.v)
    out = abi.short_attention(inp.q, inp.k, inp.v, inp.scale)
    assert out.shape == (B, N, H * 64) and out.dtype == dtype and out.is_contiguous()
    worst = fo.check(f"{B}x{H}x{N} {layout} gain {gain} {dtype}", dict(out=out), fo.reference(inp), dtype)
    out_g, intact = _short_guarded(inp.q, inp.k, inp.v, inp.scale)
    assert intact, "elements beside out were written"
    assert torch.equal(_bits(out_g), _bits(out)), "two calls, other bits"
    if N == 1:
        assert torch.equal(_bits(out), _bits(inp.v.permute(0, 2, 1, 3).reshape(B, 1, H * 64))), "one token: out is v"
        assert worst == dict(out=0.0)
    return worst


def _sweep_short(B, H, N, dtype, seed):
    for layout in ("qkv", "separate"):
        for gain in GAINS:
            _check_short(B, H, N, dtype, seed, layout, gain)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", range(1, 9))
def test_short_attention_at_every_sequence_length(N, dtype):
    _sweep_short(37, 12, N, dtype, seed=400 + N)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H", [1, 2, 5, 12, 16])
def test_short_attention_head_counts(H, dtype):
    for N in (3, 8):
        _sweep_short(7, H, N, dtype, seed=500 + 10 * H + N)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,H", [(1, 1), (31, 1), (32, 1), (33, 1), (257, 1), (11, 3)])
def test_short_attention_wave_and_block_tails(B, H, dtype):
    """B * H units, eight to a wave and 32 to a block: one unit, one less and one more than a block, eight blocks and a
    unit, and a block whose last wave starts inside a sequence's heads (33 = 11 x 3)."""
    for N in (5, 8):
        _sweep_short(B, H, N, dtype, seed=600 + B + N)


# ------------------------------------------------------------------------------------------------ past 2^31 elements

def _room_for(nbytes: int):
    free = torch.cuda.mem_get_info(torch.device(DEV))[0]
    if free < nbytes:
        pytest.skip(f"the device has {free >> 20} MiB free, the case needs {nbytes >> 20} MiB")


def test_trajectory_mix_rows_beyond_2_to_the_31_elements():
    """H = 1, F = 8, the halves of one kv buffer of 2^21 + 64 rows of 8 x 128 elements: the last 64 rows start
    2^31 elements or more behind the buffer's first.  Reference and bound on the first and the last 64 rows."""
    abi = _abi()
    dtype, H, F, C = torch.bfloat16, 1, 8, 64
    rows = 2 ** 21 + 64
    _room_for(2 * rows * F * 2 * C + 2 * rows * F * 4 + 16 * rows * C + (1 << 28))
    gen = torch.Generator(device=DEV).manual_seed(31)
    kv = torch.empty((1, rows, F, 2 * C), dtype=dtype, device=DEV).normal_(generator=gen)
    q2 = torch.empty((1, rows, C), dtype=dtype, device=DEV).normal_(generator=gen)
    k2, val = kv[..., :C], kv[..., C:]
    assert (rows - 64) * F * 2 * C >= 2 ** 31
    out, attn = abi.trajectory_mix(q2, k2, val, H, fo.SCALE)
    again, _ = abi.trajectory_mix(q2, k2, val, H, fo.SCALE, want_attn=False)
    assert torch.equal(_bits(out), _bits(again))
    for name, rs in (("first 64 rows", slice(0, 64)), ("last 64 rows", slice(rows - 64, rows))):
        q, k, v = (t[:, rs].cpu().contiguous() for t in (q2, k2, val))
        inp = to.Inputs(q, k, v, torch.zeros_like(q), H, fo.SCALE)
        fo.check(f"2^31 {name}", dict(out=out[:, rs], tattn=attn[:, :, rs]), fo.reference(inp), dtype)


def test_short_attention_sequences_beyond_2_to_the_31_elements():
    """H = 1, N = 8, one qkv buffer of 2^31 / 1536 + 65 sequences of 8 x 3 x 64 elements: the last 64 sequences start
    more than 2^31 elements behind the buffer's first.  Reference and bound on the first and the last 64 sequences."""
    abi = _abi()
    dtype, H, N = torch.bfloat16, 1, 8
    B = 2 ** 31 // (N * 3 * 64) + 1 + 64
    _room_for(2 * B * N * 3 * 64 + 4 * B * N * 64 + (1 << 28))
    gen = torch.Generator(device=DEV).manual_seed(32)
    qkv = torch.empty((B, N, 3, H, 64), dtype=dtype, device=DEV).normal_(generator=gen)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    assert (B - 64) * N * 3 * 64 >= 2 ** 31
    out = abi.short_attention(q, k, v, fo.SCALE)
    assert torch.equal(_bits(out), _bits(abi.short_attention(q, k, v, fo.SCALE)))
    for name, bs in (("first 64 sequences", slice(0, 64)), ("last 64 sequences", slice(B - 64, B))):
        qs, ks, vs = (t[bs].cpu() for t in (q, k, v))
        inp = so.Inputs(qs, ks, vs, torch.zeros((64, N, H * 64), dtype=dtype), fo.SCALE, None)
        fo.check(f"2^31 {name}", dict(out=out[bs]), fo.reference(inp), dtype)
