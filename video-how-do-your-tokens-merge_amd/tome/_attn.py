"""The attention kernels of the patched blocks.  One routed entry per operation: it launches the kernel directly when
no gradient is wanted of any participant, as an autograd Function when one is (models are patched for training,
tools/train_net.py:727-741), and answers None when the caller is to take the framework's ops.  Each `*route` is that
decision alone, without a launch.

    attention(q, k, v, size, scale, dropout_p, bias_skip, qkv=None), short_attention(q, k, v, scale, live_drop, qkv5),
    trajectory_stage1(heads, nseg, log_flat, scale, live_drop, want_attn, join), trajectory_mix(q2p, k2, val, heads, ...)

What each examines and what its Function form needs: the routing table in DESIGN.md section 1.

The Functions: forward = the inference launch (tome_prop_attention) on the detached tensors, backward =
tome_prop_attention_backward (csrc/tome_attn_bwd.h).

    attention_native(q, k, v, size, scale, bias_skip=False)   -> [B, N, H*64]      q, k, v: [B, H, N, 64] head views
    attention_qkv_native(qkv, size, scale, bias_skip=False)   -> [B, N, H*64]      qkv: the [3, B, H, N, 64] view of one
                                                                                   [B, N, 3, H, 64] projection output
    short_attention_native(qkv5, scale)                       -> [B, N, H*64]      qkv5: the [B, N <= 8, 3, H, 64] projection
                                                                                   output itself (TimeSformer's temporal
                                                                                   attention, no size bias)

The backward recomputes the softmax from q, k and the size bias (row maximum and sum included), so the forward saves
nothing but its inputs and the tensor it returns anyway.  `size` gets no gradient.  The qkv form
takes the projection's buffer as its single differentiable input and returns one gradient buffer of that layout, whose
three slices the kernels write directly: autograd's three select_backward passes (zero-fill and add, three times the
token tensor per layer) never run.  Double backward raises.  The short form (sequences of at most 8
tokens) has a backward of its own, tome_short_attention_backward (csrc/tome_short_attn_bwd.h): one launch that
recomputes the softmax and writes the three slices of one gradient buffer.

Motionformer's trajectory attention (tome/patch/motionformer.py) has two more:

    segment_attention_native(q, k, v, nseg, log_bias, scale)   -> [B, N, nseg, H*64]   tome_prop_attention_segments,
    segment_attention_qkv_native(qkv, nseg, log_bias, scale)      backward tome_prop_attention_segments_backward; the qkv
                                                                  form: q = qkv[0][:, :, 1:], k / v = rows 1 .. 1 + nseg*P
                                                                  of qkv[1] / qkv[2], one gradient buffer
    trajectory_mix_native(q2, k2, val, heads, scale)           -> [B, S, C]            tome_trajectory_mix without the map,
                                                                  backward tome_trajectory_mix_backward

The class token's attention over all keys is NOT part of the segment Function: the patch runs it through
attention_native with one query, and autograd adds its dq (row 0) and dk / dv (all rows) to the buffer the qkv form
returns -- two Functions summed by autograd, no read-modify-write of a shared buffer (DESIGN.md section 1 says what
that costs).
"""
from __future__ import annotations

import torch

from . import _abi

# False: `tome/patch/_common.py:attention` takes the framework's scaled_dot_product_attention with the bias tensor the
# reference builds and autograd (the behaviour before the backward kernels existed) -- for A/B in tests and
# tools/attn_backward_bench.py.  Also off when tome.merge.NATIVE_BACKWARD is off.  On by default: faster than the framework path
# at every measured shape.
NATIVE_ATTN_BACKWARD = True


# False: `hosts/timesformer.py::Attention.forward` keeps the framework's scaled_dot_product_attention and autograd for a
# temporal attention that requires grad (the behaviour before tome_short_attention_backward existed) -- for A/B in tests
# and tools/timesformer_backward_bench.py.  Effective only while enabled() below holds too, so that the two older
# switches still restore the framework path as a whole.  What the default rests on is said in DESIGN.md section 1.
NATIVE_SHORT_ATTN_BACKWARD = True


# False: `tome/patch/motionformer.py::_trajectory_forward` keeps the reference's op sequence and autograd for a trajectory
# attention that requires grad (the behaviour before tome_prop_attention_segments_backward and
# tome_trajectory_mix_backward existed) -- for A/B in tests and tools/motionformer_backward_bench.py.  Effective only
# while enabled() below holds too.  What the default rests on is said in DESIGN.md section 1.
NATIVE_TRAJECTORY_BACKWARD = True


def trajectory_enabled() -> bool:
    return bool(NATIVE_TRAJECTORY_BACKWARD and enabled())


def short_enabled() -> bool:
    return bool(NATIVE_SHORT_ATTN_BACKWARD and enabled())


def enabled() -> bool:
    from . import merge
    return bool(NATIVE_ATTN_BACKWARD and merge.NATIVE_BACKWARD)


def route(q, k, v, dropout_p: float = 0.0):
    """How the proportional attention of these heads runs: None (the framework's ops: not the kind of tensors the kernel
    takes), "direct" (the launch itself: no participant wants a gradient) or, when one does, "function" (the same launch
    with the native backward behind it) where the switches allow, else None."""
    if dropout_p != 0.0 or not (_abi._head_view(q) and _abi._head_view(k) and _abi._head_view(v)):
        return None
    if not (torch.is_grad_enabled() and _abi.needs_grad(q, k, v)):
        return "direct"
    return "function" if enabled() else None


def short_route(q, k, v, live_drop: bool = False, qkv5=None):
    """The same for the short attention; qkv5: the [B, N, 3, H, 64] buffer q, k, v are slices of (None: no Function form)."""
    if live_drop or not _abi._short_heads(q, k, v):
        return None
    if not (torch.is_grad_enabled() and _abi.needs_grad(q, k, v)):
        return "direct"
    return "function" if qkv5 is not None and short_enabled() and short_qkv_trainable(qkv5) else None


def trajectory_route(heads, nseg: int, live_drop: bool = False, want_attn: bool = False):
    """The same for the first stage of the trajectory attention; the Functions return no map: None when one is wanted."""
    if live_drop or not all(_abi._head_view(t) for t in heads):
        return None
    if not (torch.is_grad_enabled() and _abi.needs_grad(heads)):
        return "direct"
    return "function" if not want_attn and trajectory_enabled() and segments_qkv_trainable(heads, nseg) else None


def trajectory_mix_route(q2p, k2, val, heads: int, want_attn: bool = False):
    """The same for the second stage (tome_trajectory_mix)."""
    if not _abi._trajectory_rows(q2p, k2, val, heads):
        return None
    if not (torch.is_grad_enabled() and _abi.needs_grad(q2p, k2, val)):
        return "direct"
    return "function" if not want_attn and trajectory_enabled() else None


def _log_bias(size, B):
    """The fp32 [B, keys] bias both launches read (what _abi.prop_attention makes of `size`), or None."""
    if size is None:
        return None
    # (asked of `size` itself: the log the merge kernel emitted travels as an attribute that a detached copy lacks)
    with torch.no_grad():
        return _abi.log_of_size(size).detach().reshape(B, -1).float().contiguous()


def _forward(ctx, saved, q, k, v, size, scale, bias_skip):
    """Both Functions' forward on detached heads; `saved`: the inputs kept for backward, ahead of the output and the bias."""
    log = _log_bias(size, q.shape[0])
    out = _abi.prop_attention(q, k, v, None, scale, bias_skip=bias_skip, log_bias=log, checked=True)
    ctx.scale, ctx.bias_skip, ctx.has_bias = float(scale), bool(bias_skip), log is not None
    ctx.save_for_backward(*saved, out, *(() if log is None else (log,)))
    return out


class _AttentionFunction(torch.autograd.Function):
    """softmax(q k^T scale + log size) v: tome_prop_attention forward, tome_prop_attention_backward backward."""

    @staticmethod
    def forward(ctx, q, k, v, size, scale, bias_skip):
        q, k, v = q.detach(), k.detach(), v.detach()
        return _forward(ctx, (q, k, v), q, k, v, size, scale, bias_skip)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        q, k, v, out = ctx.saved_tensors[:4]
        log = ctx.saved_tensors[4] if ctx.has_bias else None
        dq, dk, dv = _abi.prop_attention_backward(q, k, v, out, g_out, log, ctx.scale, bias_skip=ctx.bias_skip)
        need = ctx.needs_input_grad
        return (dq if need[0] else None), (dk if need[1] else None), (dv if need[2] else None), None, None, None


class _AttentionQKVFunction(torch.autograd.Function):
    """The same for q, k, v = qkv[0], qkv[1], qkv[2] of one projection output: one input, one gradient buffer."""

    @staticmethod
    def forward(ctx, qkv, size, scale, bias_skip):
        qkv = qkv.detach()
        return _forward(ctx, (qkv,), qkv[0], qkv[1], qkv[2], size, scale, bias_skip)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        qkv, out = ctx.saved_tensors[:2]
        log = ctx.saved_tensors[2] if ctx.has_bias else None
        _, B, H, N, D = qkv.shape
        # [B, N, 3, H, 64] like the projection's output, seen as [3, B, H, N, 64]: every element is written below
        g = torch.empty((B, N, 3, H, D), dtype=qkv.dtype, device=qkv.device).permute(2, 0, 3, 1, 4)
        _abi.prop_attention_backward(qkv[0], qkv[1], qkv[2], out, g_out, log, ctx.scale, bias_skip=ctx.bias_skip,
                                     grads=(g[0], g[1], g[2]))
        return g, None, None, None


def _check(what, *heads):
    if not _abi.prop_attention_trainable(*heads):
        raise _abi.TomeHipError(f"{what}: these heads ({tuple(heads[0].shape)} {heads[0].dtype}) are not ones the kernels "
                                "take (_abi.prop_attention_trainable)")


def attention_native(q, k, v, size, scale: float, bias_skip: bool = False):
    """softmax(q k^T * scale + log(size)) v for [B, H, N, 64] head views that require grad; returns [B, N, H*64]."""
    _check("attention_native", q, k, v)
    return _AttentionFunction.apply(q, k, v, size, float(scale), bool(bias_skip))


def qkv_trainable(qkv: torch.Tensor) -> bool:
    """Is `qkv` a [3, B, H, N, 64] view whose three slices the kernels take, q / k / v of equal length?"""
    return qkv.dim() == 5 and qkv.shape[0] == 3 and _abi.prop_attention_trainable(qkv[0], qkv[1], qkv[2])


def attention_qkv_native(qkv, size, scale: float, bias_skip: bool = False):
    """The same for the [3, B, H, N, 64] view of one qkv projection: its gradient comes back as one buffer."""
    if not qkv_trainable(qkv):
        raise _abi.TomeHipError(f"attention_qkv_native: qkv {tuple(qkv.shape)} {qkv.dtype} is not a [3, B, H, N, 64] view "
                                "the kernels take")
    return _AttentionQKVFunction.apply(qkv, size, float(scale), bool(bias_skip))


class _ShortAttentionFunction(torch.autograd.Function):
    """softmax(q k^T scale) v over sequences of at most 8 tokens, q, k, v the slices of one [B, N, 3, H, 64] projection
    output: tome_short_attention forward, tome_short_attention_backward backward.  One input, one gradient buffer."""

    @staticmethod
    def forward(ctx, qkv5, scale):
        qkv5 = qkv5.detach()
        q, k, v = qkv5.permute(2, 0, 3, 1, 4).unbind(0)
        out = _abi.short_attention(q, k, v, scale)
        ctx.scale = float(scale)
        ctx.save_for_backward(qkv5)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        (qkv5,) = ctx.saved_tensors
        q, k, v = qkv5.permute(2, 0, 3, 1, 4).unbind(0)
        g = torch.empty_like(qkv5)  # every element is written by the launch below
        _abi.short_attention_backward(q, k, v, g_out, ctx.scale, grads=tuple(g.permute(2, 0, 3, 1, 4).unbind(0)))
        return g, None


def short_qkv_trainable(qkv5: torch.Tensor) -> bool:
    """Is `qkv5` a [B, N <= 8, 3, H, 64] projection output whose three slices the short kernels take?"""
    if qkv5.dim() != 5 or qkv5.shape[2] != 3 or not qkv5.is_contiguous():
        return False
    q, k, v = qkv5.permute(2, 0, 3, 1, 4).unbind(0)
    return _abi.short_attention_trainable(q, k, v)


def short_attention_native(qkv5, scale: float):
    """softmax(q k^T * scale) v for the [B, N <= 8, 3, H, 64] output of a qkv projection that requires grad; returns
    [B, N, H*64].  The gradient of the buffer comes back as one tensor of its layout."""
    if not short_qkv_trainable(qkv5):
        raise _abi.TomeHipError(f"short_attention_native: qkv {tuple(qkv5.shape)} {qkv5.dtype} is not a contiguous "
                                "[B, N <= 8, 3, H, 64] buffer the kernels take (_abi.short_attention_trainable)")
    return _ShortAttentionFunction.apply(qkv5, float(scale))


def _segments_backward(ctx, q, k, v, y, g_y, log, grads=None):
    return _abi.prop_attention_segments_backward(q, k, v, y, g_y, ctx.nseg, ctx.scale, log_bias=log, grads=grads)


class _SegmentAttentionFunction(torch.autograd.Function):
    """Every query against the keys of one segment at a time, a softmax per segment: tome_prop_attention_segments
    forward, tome_prop_attention_segments_backward backward.  Saves its inputs, y and the bias."""

    @staticmethod
    def forward(ctx, q, k, v, nseg, log_bias, scale):
        q, k, v = q.detach(), k.detach(), v.detach()
        y = _abi.prop_attention_segments(q, k, v, nseg, scale, log_bias=log_bias)
        ctx.nseg, ctx.scale, ctx.has_bias = int(nseg), float(scale), log_bias is not None
        ctx.save_for_backward(q, k, v, y, *(() if log_bias is None else (log_bias,)))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_y):
        q, k, v, y = ctx.saved_tensors[:4]
        dq, dk, dv = _segments_backward(ctx, q, k, v, y, g_y, ctx.saved_tensors[4] if ctx.has_bias else None)
        need = ctx.needs_input_grad
        return (dq if need[0] else None), (dk if need[1] else None), (dv if need[2] else None), None, None, None


def _segment_slices(qkv, nseg):
    """q, k, v of the trajectory attention inside the [3, B, H, N, 64] view of one projection: every token but the class
    token asks, the nseg * P tokens behind the class token are the keys."""
    N = qkv.shape[3]
    P = (N - 1) // nseg
    return qkv[0][:, :, 1:], qkv[1][:, :, 1:1 + nseg * P], qkv[2][:, :, 1:1 + nseg * P]


class _SegmentAttentionQKVFunction(torch.autograd.Function):
    """The same for the slices of one projection output ([3, B, H, N, 64] view, class token in row 0): one input, one
    gradient buffer of its layout whose rows the kernels write; the rows no segment touches (the class token's, and
    tokens past the last whole segment) are zeros."""

    @staticmethod
    def forward(ctx, qkv, nseg, log_bias, scale):
        qkv = qkv.detach()
        q, k, v = _segment_slices(qkv, nseg)
        y = _abi.prop_attention_segments(q, k, v, nseg, scale, log_bias=log_bias)
        ctx.nseg, ctx.scale, ctx.has_bias = int(nseg), float(scale), log_bias is not None
        ctx.save_for_backward(qkv, y, *(() if log_bias is None else (log_bias,)))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_y):
        qkv, y = ctx.saved_tensors[:2]
        _, B, H, N, D = qkv.shape
        g = torch.empty((B, N, 3, H, D), dtype=qkv.dtype, device=qkv.device).permute(2, 0, 3, 1, 4)
        q, k, v = _segment_slices(qkv, ctx.nseg)
        keys = k.shape[2]
        g[:, :, :, :1].zero_()          # the class token asks and is asked elsewhere (attention_native, one query)
        g[1:, :, :, 1 + keys:].zero_()  # (N - 1 not a multiple of nseg: tokens that are queries only)
        _segments_backward(ctx, q, k, v, y, g_y, ctx.saved_tensors[2] if ctx.has_bias else None,
                           grads=_segment_slices(g, ctx.nseg))
        return g, None, None, None


def _segment_bias(log_bias):
    return None if log_bias is None else log_bias.detach().float().contiguous()


def segment_attention_native(q, k, v, nseg: int, log_bias, scale: float):
    """Per-segment attention (see _abi.prop_attention_segments) for head views that require grad; log_bias: the
    [B, nseg*P] bias in natural-log units or None (no gradient).  Returns y [B, N, nseg, H*64]."""
    if not _abi.prop_attention_segments_trainable(q, k, v, nseg):
        raise _abi.TomeHipError(f"segment_attention_native: these heads ({tuple(q.shape)} / {tuple(k.shape)} {q.dtype}, "
                                f"{nseg} segments) are not ones the kernels take "
                                "(_abi.prop_attention_segments_trainable)")
    return _SegmentAttentionFunction.apply(q, k, v, int(nseg), _segment_bias(log_bias), float(scale))


def segments_qkv_trainable(qkv: torch.Tensor, nseg: int) -> bool:
    """Is `qkv` a [3, B, H, N, 64] view whose trajectory slices (_segment_slices) the segment kernels take?"""
    if qkv.dim() != 5 or qkv.shape[0] != 3 or int(nseg) < 1 or qkv.shape[3] - 1 < int(nseg):
        return False
    return _abi.prop_attention_segments_trainable(*_segment_slices(qkv, nseg), nseg)


def segment_attention_qkv_native(qkv, nseg: int, log_bias, scale: float):
    """The same for the [3, B, H, N, 64] view of one qkv projection (class token in row 0): its gradient comes back as
    one buffer.  The class token's own attention is not part of it."""
    if not segments_qkv_trainable(qkv, nseg):
        raise _abi.TomeHipError(f"segment_attention_qkv_native: qkv {tuple(qkv.shape)} {qkv.dtype} is not a "
                                f"[3, B, H, N, 64] view the kernels take with {nseg} segments")
    return _SegmentAttentionQKVFunction.apply(qkv, int(nseg), _segment_bias(log_bias), float(scale))


class _TrajectoryMixFunction(torch.autograd.Function):
    """softmax over the F frames of (q2 * scale . k2[f]), weighted sum of val[f]: tome_trajectory_mix (no map) forward,
    tome_trajectory_mix_backward backward.  The map is not returned, so it gets no gradient."""

    @staticmethod
    def forward(ctx, q2, k2, val, heads, scale):
        q2, k2, val = q2.detach(), k2.detach(), val.detach()
        out, _ = _abi.trajectory_mix(q2, k2, val, heads, scale, want_attn=False)
        ctx.heads, ctx.scale = int(heads), float(scale)
        ctx.save_for_backward(q2, k2, val)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        q2, k2, val = ctx.saved_tensors
        need = ctx.needs_input_grad
        dq2, dk2, dval = _abi.trajectory_mix_backward(q2, k2, val, g_out, ctx.heads, ctx.scale, want_k2=need[1],
                                                      want_val=need[2])
        return (dq2 if need[0] else None), dk2, dval, None, None


def trajectory_mix_native(q2, k2, val, heads: int, scale: float):
    """The temporal stage of the trajectory attention for tensors that require grad (see _abi.trajectory_mix); returns
    out [B, S, C] only.  A caller that wants the attention map under grad keeps the framework's ops."""
    if not _abi.trajectory_mix_trainable(q2, k2, val, heads):
        raise _abi.TomeHipError("trajectory_mix_native: unsupported tensors (_abi.trajectory_mix_trainable)")
    return _TrajectoryMixFunction.apply(q2, k2, val, int(heads), float(scale))


def attention(q, k, v, size, scale: float, dropout_p: float = 0.0, bias_skip: bool = False, qkv=None):
    """softmax(q k^T * scale + log(size)) v for [B, H, N, 64] head views: [B, N, H*64], or None.  qkv: the [3, B, H, N, 64]
    view they are the slices of -- under grad the Function's one input, whose gradient comes back as one buffer."""
    how = route(q, k, v, dropout_p)
    if how == "direct":
        return _abi.prop_attention(q, k, v, size, scale, bias_skip=bias_skip, checked=True)
    if how is None:
        return None
    if qkv is None:
        return attention_native(q, k, v, size, scale, bias_skip=bias_skip)
    return attention_qkv_native(qkv, size, scale, bias_skip=bias_skip)


def short_attention(q, k, v, scale: float, live_drop: bool = False, qkv5=None):
    """softmax(q k^T * scale) v over sequences of at most 8 tokens (TimeSformer's temporal attention), or None."""
    how = short_route(q, k, v, live_drop, qkv5)
    if how == "direct":
        return _abi.short_attention(q, k, v, scale, checked=True)
    return short_attention_native(qkv5, scale) if how == "function" else None


def trajectory_stage1(heads, nseg: int, log_flat, scale: float, live_drop: bool, want_attn: bool, join: bool):
    """The first stage of Motionformer's trajectory attention: (cls_out, y, joined), or None.  cls_out: the class token
    attending to every token, sizes ignored (motionformer.py:54) -- one query per head; y: every other token attending
    to the keys of ONE frame at a time (bias log_flat) -- one launch of the segmented kernel, the [B*h, N, N] logits
    never exist.  joined (direct form with `join`): the [B, N, H*64] buffer whose row 0 cls_out is, for the second stage
    to fill: cat((cls_out, x), dim=1) without the copy.  Under grad autograd adds the two Functions' gradients of qkv."""
    how = trajectory_route(heads, nseg, live_drop, want_attn)
    if how is None:
        return None
    if how == "function":
        return (attention_native(heads[0][:, :, :1], heads[1], heads[2], None, scale),
                segment_attention_qkv_native(heads, nseg, log_flat, scale), None)
    _, B, h, N, hd = heads.shape
    joined = torch.empty((B, N, h * hd), dtype=heads.dtype, device=heads.device) if join else None
    cls_out = _abi.prop_attention(heads[0][:, :, :1], heads[1], heads[2], None, scale,
                                  out=joined[:, :1].unflatten(2, (h, hd)) if join else None)
    q, k, v = _segment_slices(heads, nseg)
    lf = None if log_flat is None else log_flat.float().contiguous()
    return cls_out, _abi.prop_attention_segments(q, k, v, nseg, scale, log_bias=lf), joined


def trajectory_mix(q2p, k2, val, heads: int, scale: float, want_attn: bool = False, out=None):
    """The second stage (see _abi.trajectory_mix): (out [B, S, C], attention map or None, wrote), or None.  wrote: the
    result went into `out` -- the direct form only: under grad the class row and the trajectory rows meet in torch.cat,
    not in a shared buffer."""
    how = trajectory_mix_route(q2p, k2, val, heads, want_attn)
    if how == "direct":
        return (*_abi.trajectory_mix(q2p, k2, val, heads, scale, want_attn=want_attn, out=out), out is not None)
    return (trajectory_mix_native(q2p, k2, val, heads, scale), None, False) if how == "function" else None
