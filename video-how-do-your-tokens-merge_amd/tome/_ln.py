"""The LayerNorms of the patched blocks.  One routed entry per operation: it launches the add + LayerNorm kernel
directly when no gradient is wanted of any participant -- x, the addend, the norm's weight and bias -- as an autograd
Function when one is (models are patched for training, tools/train_net.py:727-741; needs enabled(), for the regrouped
form regrouped_enabled(), and _abi.ln_trainable), and answers None when the caller is to take the framework's ops (not
_abi._ln_of, not an nn.LayerNorm, an addend of another dtype).  `route` is that decision alone, without a launch.

    add_layernorm(x, addend or None, norm, skip_first=False)  -> (x + addend, norm(x + addend), skipped) or None
    add_layernorm_regrouped(x, addend, frames, norm)           -> (cat(cls, x[:, 1:] + addend), norm regrouped) or None

The Functions: forward = the inference kernels (tome_add_layernorm / tome_add_layernorm_skip_first) on the detached
tensors, backward = tome_layernorm_backward (csrc/tome_ln_bwd.h).

    add_layernorm_native(x, addend, norm, skip_first=False) -> (x + addend, norm(x + addend))
    layernorm_native(x, norm, skip_first=False)             -> norm(x)
    add_layernorm_regrouped_native(x, addend, T, norm)      -> (cat(cls, x[:, 1:] + addend), norm of the regrouped tokens)

skip_first (x [B, N, C]): the LayerNorm output leaves out every clip's first row, as `_abi.add_layernorm` does.
The backward recomputes mean and rstd from the stored sum (the row the forward normalised), so the forward saves
nothing but the tensors it returns anyway.  The gradient of the sum that arrives through the residual stream and the
gradient through the LayerNorm are added inside the one launch and rounded once; x and addend receive the same
tensor.  Double backward raises.
merge_ln_native(plan, x, addend, size, norm, drop, log_size) -> (x', norm(x'), size'): the fused residual add + merge (or
drop) + LayerNorm launch (tome_merge_wavg_ln / tome_drop_ln) as a Function, tome_merge_ln_backward behind it -- one
launch each way.  Reached through tome.merge.merge_wavg_ln / drop_ln, which route (the patched blocks take them only with
tome.patch._common.TRAIN_FUSED_LN on).
merge_ln_amp_native: the same under autocast with fp32 LayerNorm parameters (tome_merge_wavg_ln_amp / tome_drop_ln_amp,
tome_merge_ln_backward_amp behind them), reached by the same two calls while NATIVE_MERGE_LN_AUTOCAST_BACKWARD is on.
The regrouped form is the middle of TimeSformer's divided space-time block (tome_add_layernorm_regrouped forward,
tome_layernorm_backward_regrouped backward): x [B, 1 + P*T, C] and addend [B, P*T, C] receive gx and its view gx[:, 1:].
"""
from __future__ import annotations

import torch

from . import _abi

# False: the callers in tome/patch/_common.py take the framework's `x + a`, `norm(x)` and autograd (the behaviour before
# the backward kernel existed) -- for A/B in tests and tools/layernorm_backward_bench.py.  Also off when
# tome.merge.NATIVE_BACKWARD is off.  On by default; what that rests on (measured or not) is said in DESIGN.md section 1.
NATIVE_LN_BACKWARD = True


# False: `tome/patch/timesformer.py::_block_forward` keeps the reference's op sequence (add, transpose, three cats,
# norm1) and autograd for tokens that require grad (the behaviour before tome_layernorm_backward_regrouped existed) -- for
# A/B in tests and tools/timesformer_backward_bench.py.  Effective only while enabled() below holds too.  What the default
# rests on is said in DESIGN.md section 1.
NATIVE_LN_REGROUPED_BACKWARD = True


# False: under autocast the callers take the framework's `x + a`, its fp32 layer_norm and the consumer's cast (the
# behaviour before tome_add_layernorm_amp existed), in both grad modes -- for A/B in tests and tools/autocast_bench.py.
# The Function form also needs enabled() below.  What the default rests on is said in DESIGN.md section 1.
NATIVE_LN_AUTOCAST = True

# True: under autocast, when a participant wants a gradient, tome.merge.merge_wavg_ln / drop_ln (and the flat-layout blocks
# of kinds "merge" and "drop", tome/patch/_common.py::fused_route) run the residual add, the reduction and the LayerNorm as
# _MergeLnAmpFunction below -- tome_merge_wavg_ln_amp / tome_drop_ln_amp forward, tome_merge_ln_backward_amp backward, one
# launch each way -- where _abi.merge_ln_amp_trainable holds, instead of the framework's add, the merge Function and
# _AddLayerNormAmpFunction.  Needs NATIVE_LN_AUTOCAST and enabled() too.  Off by default: what that rests on is said in
# DESIGN.md section 1 (measure with tools/autocast_merge_ln_backward_bench.py).
NATIVE_MERGE_LN_AUTOCAST_BACKWARD = False

AMP_DIRECT, AMP_FUNCTION = "amp_direct", "amp_function"


def regrouped_enabled() -> bool:
    return bool(NATIVE_LN_REGROUPED_BACKWARD and enabled())


def enabled() -> bool:
    from . import merge
    return bool(NATIVE_LN_BACKWARD and merge.NATIVE_BACKWARD)


def route(x: torch.Tensor, norm, addend=None, regrouped: bool = False):
    """How `norm(x [+ addend])` runs: None (the framework's ops: not the kind of tensors the kernel takes), "direct" (the
    launch itself: neither x, the addend nor the norm's weight or bias wants a gradient) or, when one does, "function"
    (the same launch with the native backward behind it) where the switches and ln_trainable allow, else None.  Under
    autocast, for tensors of the kind _abi._ln_amp_of describes, "amp_direct" / "amp_function": the mixed-precision
    launch, by the same rule."""
    if not isinstance(norm, torch.nn.LayerNorm):
        return None
    if not (_abi._ln_of(x, norm) and (addend is None or addend.dtype == x.dtype)):
        return None if regrouped else _route_amp(x, norm, addend)
    if not (torch.is_grad_enabled() and _abi.needs_grad(x, addend, norm.weight, norm.bias)):
        return "direct"
    return "function" if (regrouped_enabled() if regrouped else enabled()) and _abi.ln_trainable(x, norm) else None


def _route_amp(x, norm, addend):
    """route's answer for tensors the 16-bit kernels do not take: the mixed-precision forms under autocast, else None."""
    if not (NATIVE_LN_AUTOCAST and _abi._ln_amp_of(x, norm, addend)):
        return None
    if not (torch.is_grad_enabled() and _abi.needs_grad(x, addend, norm.weight, norm.bias)):
        return AMP_DIRECT
    return AMP_FUNCTION if enabled() and type(norm) is torch.nn.LayerNorm else None  # (the stock module: ln_trainable)


def ln_backward_amp(gy, xs, gx_in, weight, eps, skip_first, want_weight, want_bias, want_gx16):
    """The backward arithmetic of the mixed-precision Functions: (gx, gx16, dweight, dbias).  A seam, like ln_backward."""
    return _abi.layernorm_backward_amp(gy, xs, gx_in, weight, eps, skip_first=skip_first, want_weight=want_weight,
                                       want_bias=want_bias, want_gx16=want_gx16)


def ln_backward(gy, xs, gx_in, weight, eps, skip_first, want_weight, want_bias):
    """The backward arithmetic of both Functions: (gx, dweight, dbias) from the saved tensors.  One module-level seam, so
    that a test can put another evaluation of the same formula in its place."""
    return _abi.layernorm_backward(gy, xs, gx_in, weight, eps, skip_first=skip_first, want_weight=want_weight,
                                   want_bias=want_bias)


def ln_backward_regrouped(gy, xs, gx_in, frames, weight, eps, want_weight, want_bias):
    """The backward arithmetic of the regrouped Function: (gx, dweight, dbias).  A seam of its own, like ln_backward."""
    return _abi.layernorm_backward_regrouped(gy, xs, gx_in, frames, weight, eps, want_weight=want_weight,
                                             want_bias=want_bias)


def _backward(ctx, g_sum, g_y, seam=None):
    """(gx, dweight, dbias) of every Function here.  seam(gy, xs, gx_in, weight, want_weight, want_bias): the backward
    launch, ln_backward unless the Function has another."""
    xs, weight = ctx.saved_tensors
    want_x = ctx.needs_x
    want_w, want_b = ctx.needs_input_grad[ctx.first_param], ctx.needs_input_grad[ctx.first_param + 1]
    if g_y is None:  # nothing read the LayerNorm: the stream's gradient passes through, the parameters get zeros
        gx = g_sum if want_x else None
        return gx, (torch.zeros_like(weight) if want_w else None), (torch.zeros_like(weight) if want_b else None)
    cast = lambda g: g if g is None or g.dtype == xs.dtype else g.to(xs.dtype)  # noqa: E731
    if seam is None:
        gx, dw, db = ln_backward(cast(g_y), xs, cast(g_sum), weight, ctx.eps, ctx.skip_first, want_w, want_b)
    else:
        gx, dw, db = seam(cast(g_y), xs, cast(g_sum), weight, want_w, want_b)
    return (gx if want_x else None), dw, db


class _AddLayerNormFunction(torch.autograd.Function):
    """(x + addend, LayerNorm(x + addend)): tome_add_layernorm[_skip_first] forward, tome_layernorm_backward backward."""

    @staticmethod
    def forward(ctx, x, addend, weight, bias, eps, skip_first):
        x_out, y = _abi.add_layernorm(x.detach(), addend.detach(), weight.detach(), bias.detach(), eps,
                                      skip_first=skip_first)
        ctx.eps, ctx.skip_first, ctx.first_param = float(eps), bool(skip_first), 2
        ctx.needs_x = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        ctx.save_for_backward(x_out, weight)
        ctx.set_materialize_grads(False)  # an output nobody read arrives as None, not as a tensor of zeros
        return x_out, y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sum, g_y):
        gx, dw, db = _backward(ctx, g_sum, g_y)
        return (gx if ctx.needs_input_grad[0] else None), (gx if ctx.needs_input_grad[1] else None), dw, db, None, None


class _LayerNormFunction(torch.autograd.Function):
    """LayerNorm(x) alone: tome_add_layernorm[_skip_first] without addend forward, tome_layernorm_backward backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, skip_first):
        xs, y = _abi.add_layernorm(x.detach(), None, weight.detach(), bias.detach(), eps, skip_first=skip_first)
        ctx.eps, ctx.skip_first, ctx.first_param = float(eps), bool(skip_first), 1
        ctx.needs_x = ctx.needs_input_grad[0]
        ctx.save_for_backward(xs, weight)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_y):
        gx, dw, db = _backward(ctx, None, g_y)
        return gx, dw, db, None, None


class _AddLayerNormRegroupedFunction(torch.autograd.Function):
    """(cat(cls, x[:, 1:] + addend), LayerNorm of the tokens regrouped 'b (p t) m -> (b t) p m' behind a class token per
    frame): tome_add_layernorm_regrouped forward, tome_layernorm_backward_regrouped backward."""

    @staticmethod
    def forward(ctx, x, addend, weight, bias, eps, frames):
        x1, y = _abi.add_layernorm_regrouped(x.detach(), addend.detach(), frames, weight.detach(), bias.detach(), eps)
        ctx.eps, ctx.frames, ctx.first_param = float(eps), int(frames), 2
        ctx.needs_x = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        ctx.save_for_backward(x1, weight)
        ctx.set_materialize_grads(False)  # an output nobody read arrives as None, not as a tensor of zeros
        return x1, y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_x1, g_y):
        gx, dw, db = _backward(ctx, g_x1, g_y, lambda gy, xs, gx_in, weight, want_w, want_b: ln_backward_regrouped(
            gy, xs, gx_in, ctx.frames, weight, ctx.eps, want_w, want_b))
        # x1 = cat(cls, x[:, 1:] + addend): x receives gx, the addend the view behind the class row
        need = ctx.needs_input_grad
        return ((gx if need[0] and gx is not None else None), (gx[:, 1:] if need[1] and gx is not None else None), dw, db,
                None, None)


def merge_ln_backward(plan, gy, gx_out, xs, out_div, in_mul, weight, eps, drop, want_weight, want_bias):
    """The backward arithmetic of _MergeLnFunction: (gx, dweight, dbias).  A seam of its own, like ln_backward."""
    return _abi.merge_ln_backward(plan, gy, gx_out, xs, out_div, in_mul, weight, eps, drop=drop,
                                  want_weight=want_weight, want_bias=want_bias)


class _MergeLnFunction(torch.autograd.Function):
    """(x', LayerNorm(x'), size', log size') with x' = merge_wavg(x + addend) or drop(x + addend): tome_merge_wavg_ln /
    tome_drop_ln forward (no x_out_bias), tome_merge_ln_backward backward -- one launch, the gradient of the merged rows
    never rounded on its way to the tokens.  x and the addend receive the same tensor; the sizes carry no gradient."""

    @staticmethod
    def forward(ctx, x, addend, size, weight, bias, eps, plan, drop, log_size):
        det = lambda t: None if t is None else t.detach()  # noqa: E731
        _abi.plan_row_map(plan)
        if drop:
            x_out, y = _abi.drop_ln(plan, x.detach(), weight.detach(), bias.detach(), eps, addend=det(addend))
            s_out = log = None
        else:
            x_out, y, s_out = _abi.merge_wavg_ln(plan, x.detach(), det(size), weight.detach(), bias.detach(), eps,
                                                 addend=det(addend), log_size=log_size)
            log = getattr(s_out, "_tome_log", None)
            ctx.mark_non_differentiable(*(t for t in (s_out, log) if t is not None))
        ctx.plan, ctx.eps, ctx.drop = plan, float(eps), bool(drop)
        ctx.needs_x = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        ctx.save_for_backward(x_out, weight, size, s_out)
        ctx.set_materialize_grads(False)  # an output nobody read arrives as None, not as a tensor of zeros
        return x_out, y, s_out, log

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_x, g_y, _gs, _gl):
        xs, weight, size, s_out = ctx.saved_tensors
        need = ctx.needs_input_grad
        want_w, want_b = need[3], need[4]
        cast = lambda g: g if g is None or g.dtype == xs.dtype else g.to(xs.dtype)  # noqa: E731
        if g_y is None:  # nothing read the LayerNorm: the merge alone, the parameters get zeros
            gx = None
            if ctx.needs_x and g_x is not None:
                gx = _abi.merge_backward(ctx.plan, cast(g_x), out_div=s_out, in_mul=size, drop=ctx.drop)
            dw = torch.zeros_like(weight) if want_w else None
            db = torch.zeros_like(weight) if want_b else None
        else:
            gx, dw, db = merge_ln_backward(ctx.plan, cast(g_y), cast(g_x), xs, s_out, size, weight, ctx.eps, ctx.drop,
                                           want_w, want_b)
        return ((gx if need[0] else None), (gx if need[1] else None), None, dw, db, None, None, None, None)


def merge_ln_native(plan, x, addend, size, norm, drop: bool = False, log_size: bool = False):
    """`x = x + addend; x, size = merge_wavg(merge, x, size); y = norm(x)` (drop: `x = drop(x)`, no sizes) for
    participants that require grad: (x, y, size or None)."""
    x_out, y, s_out, log = _MergeLnFunction.apply(x, addend, size, norm.weight, norm.bias, norm.eps, plan, bool(drop),
                                                  bool(log_size))
    if log is not None:
        s_out._tome_log = log  # (the size a Function returns is a new tensor object: _abi.log_of_size finds it again)
    return x_out, y, s_out


def _backward_amp(ctx, g_sum, g_y, want_gx16):
    """(gx, gx16, dweight, dbias) of the mixed-precision Functions: _backward with a 16-bit gy beside a stream of its own
    dtype, fp32 parameter gradients and the optional 16-bit copy of gx."""
    xs, weight = ctx.saved_tensors
    want_w, want_b = ctx.needs_input_grad[ctx.first_param], ctx.needs_input_grad[ctx.first_param + 1]
    if g_y is None:  # nothing read the LayerNorm: the stream's gradient passes through, the parameters get zeros
        gx = g_sum if ctx.needs_x else None
        gx16 = gx.to(ctx.y_dtype) if (want_gx16 and gx is not None) else None
        return gx, gx16, (torch.zeros_like(weight) if want_w else None), (torch.zeros_like(weight) if want_b else None)
    if g_y.dtype != ctx.y_dtype:
        g_y = g_y.to(ctx.y_dtype)
    if g_sum is not None and g_sum.dtype != xs.dtype:
        g_sum = g_sum.to(xs.dtype)
    gx, gx16, dw, db = ln_backward_amp(g_y, xs, g_sum, weight, ctx.eps, ctx.skip_first, want_w, want_b, want_gx16)
    return (gx if ctx.needs_x else None), gx16, dw, db


def merge_ln_backward_amp(plan, gy, gx_out, xs, out_div, in_mul, weight, eps, drop, want_weight, want_bias, want_gx16):
    """The backward arithmetic of _MergeLnAmpFunction: (gx, gx16, dweight, dbias).  A seam of its own, like ln_backward."""
    return _abi.merge_ln_backward_amp(plan, gy, gx_out, xs, out_div, in_mul, weight, eps, drop=drop,
                                      want_weight=want_weight, want_bias=want_bias, want_gx16=want_gx16)


class _MergeLnAmpFunction(torch.autograd.Function):
    """_MergeLnFunction under autocast: tome_merge_wavg_ln_amp / tome_drop_ln_amp forward, tome_merge_ln_backward_amp
    backward -- one launch each way, the gradient of the merged rows never written.  x receives gx; the addend gx when
    it has the stream's dtype, gx16 when it is the 16-bit addend of an fp32 stream; the sizes carry no gradient."""

    @staticmethod
    def forward(ctx, x, addend, size, weight, bias, eps, plan, drop, log_size, y_dtype):
        det = lambda t: None if t is None else t.detach()  # noqa: E731
        _abi.plan_row_map(plan)
        if drop:
            x_out, y = _abi.drop_ln_amp(plan, x.detach(), weight.detach(), bias.detach(), eps, y_dtype, addend=det(addend))
            s_out = log = None
        else:
            x_out, y, s_out = _abi.merge_wavg_ln_amp(plan, x.detach(), det(size), weight.detach(), bias.detach(), eps,
                                                     y_dtype, addend=det(addend), log_size=log_size)
            log = getattr(s_out, "_tome_log", None)
            ctx.mark_non_differentiable(*(t for t in (s_out, log) if t is not None))
        ctx.plan, ctx.eps, ctx.drop, ctx.y_dtype = plan, float(eps), bool(drop), y_dtype
        ctx.needs_x = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        ctx.addend16 = addend is not None and addend.dtype != x.dtype
        ctx.save_for_backward(x_out, weight, size, s_out)
        ctx.set_materialize_grads(False)  # an output nobody read arrives as None, not as a tensor of zeros
        return x_out, y, s_out, log

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_x, g_y, _gs, _gl):
        xs, weight, size, s_out = ctx.saved_tensors
        need = ctx.needs_input_grad
        want_w, want_b = need[3], need[4]
        want_gx16 = bool(ctx.addend16 and need[1])
        if g_x is not None and g_x.dtype != xs.dtype:
            g_x = g_x.to(xs.dtype)
        if g_y is None:  # nothing read the LayerNorm: the merge alone, the parameters get zeros
            gx = gx16 = None
            if ctx.needs_x and g_x is not None:
                gx = _abi.merge_backward(ctx.plan, g_x, out_div=s_out, in_mul=size, drop=ctx.drop)
                gx16 = gx.to(ctx.y_dtype) if want_gx16 else None
            dw = torch.zeros_like(weight) if want_w else None
            db = torch.zeros_like(weight) if want_b else None
        else:
            if g_y.dtype != ctx.y_dtype:
                g_y = g_y.to(ctx.y_dtype)
            gx, gx16, dw, db = merge_ln_backward_amp(ctx.plan, g_y, g_x, xs, s_out, size, weight, ctx.eps, ctx.drop,
                                                     want_w, want_b, want_gx16)
        return ((gx if need[0] else None), ((gx16 if ctx.addend16 else gx) if need[1] else None), None, dw, db, None,
                None, None, None, None)


def merge_ln_amp_native(plan, x, addend, size, norm, drop: bool = False, log_size: bool = False):
    """merge_ln_native under autocast (fp32 LayerNorm parameters, a stream of the autocast dtype or fp32), for
    participants that require grad: (x, y, size or None), y in the autocast dtype."""
    x_out, y, s_out, log = _MergeLnAmpFunction.apply(x, addend, size, norm.weight, norm.bias, norm.eps, plan, bool(drop),
                                                     bool(log_size), _abi.autocast_dtype(x.device))
    if log is not None:
        s_out._tome_log = log  # (as in merge_ln_native)
    return x_out, y, s_out


class _AddLayerNormAmpFunction(torch.autograd.Function):
    """(x + addend, LayerNorm(x + addend)) under autocast: tome_add_layernorm_amp forward, tome_layernorm_backward_amp
    backward.  x receives gx; the addend gx when it has the stream's dtype, gx16 when it is the 16-bit addend of an fp32
    stream."""

    @staticmethod
    def forward(ctx, x, addend, weight, bias, eps, skip_first, y_dtype):
        x_out, y = _abi.add_layernorm_amp(x.detach(), addend.detach(), weight.detach(), bias.detach(), eps, y_dtype,
                                          skip_first=skip_first)
        ctx.eps, ctx.skip_first, ctx.first_param, ctx.y_dtype = float(eps), bool(skip_first), 2, y_dtype
        ctx.needs_x = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        ctx.addend16 = addend.dtype != x.dtype
        ctx.save_for_backward(x_out, weight)
        ctx.set_materialize_grads(False)  # an output nobody read arrives as None, not as a tensor of zeros
        return x_out, y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sum, g_y):
        need = ctx.needs_input_grad
        gx, gx16, dw, db = _backward_amp(ctx, g_sum, g_y, want_gx16=ctx.addend16 and need[1])
        return (gx if need[0] else None), ((gx16 if ctx.addend16 else gx) if need[1] else None), dw, db, None, None, None


class _LayerNormAmpFunction(torch.autograd.Function):
    """LayerNorm(x) alone under autocast: tome_add_layernorm_amp without addend, tome_layernorm_backward_amp backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, skip_first, y_dtype):
        xs, y = _abi.add_layernorm_amp(x.detach(), None, weight.detach(), bias.detach(), eps, y_dtype,
                                       skip_first=skip_first)
        ctx.eps, ctx.skip_first, ctx.first_param, ctx.y_dtype = float(eps), bool(skip_first), 1, y_dtype
        ctx.needs_x = ctx.needs_input_grad[0]
        ctx.save_for_backward(xs, weight)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_y):
        gx, _, dw, db = _backward_amp(ctx, None, g_y, want_gx16=False)
        return gx, dw, db, None, None, None


def _add_layernorm_amp(x, addend, norm, skip, how):
    """add_layernorm's two mixed-precision forms: (x + addend, norm(x + addend)) with y of the autocast dtype."""
    y_dtype = _abi.autocast_dtype(x.device)
    if how == AMP_DIRECT:
        return _abi.add_layernorm_amp(x, addend, norm.weight, norm.bias, norm.eps, y_dtype, skip_first=skip)
    if addend is None:
        return x, _LayerNormAmpFunction.apply(x, norm.weight, norm.bias, norm.eps, skip, y_dtype)
    return _AddLayerNormAmpFunction.apply(x, addend, norm.weight, norm.bias, norm.eps, skip, y_dtype)


def _check(x, norm, what):
    if not _abi.ln_trainable(x, norm):
        raise _abi.TomeHipError(f"{what}: this LayerNorm of {tuple(x.shape)} {x.dtype} tokens is not one the kernels take "
                                "(_abi.ln_trainable)")


def add_layernorm_native(x, addend, norm, skip_first: bool = False):
    """`x = x + addend; y = norm(x)` (y without every clip's first row when skip_first) for tokens that require grad."""
    _check(x, norm, "add_layernorm_native")
    return _AddLayerNormFunction.apply(x, addend, norm.weight, norm.bias, norm.eps, bool(skip_first))


def layernorm_native(x, norm, skip_first: bool = False):
    """`norm(x)` (`norm(x)[:, 1:]` when skip_first) for tokens that require grad."""
    _check(x, norm, "layernorm_native")
    return _LayerNormFunction.apply(x, norm.weight, norm.bias, norm.eps, bool(skip_first))


def add_layernorm_regrouped_native(x, addend, T: int, norm):
    """TimeSformer's mid-block step for tokens that require grad: x [B, 1 + P*T, C], addend [B, P*T, C] ->
    (x1, xs_normed) with x1 = cat(cls, x[:, 1:] + addend) and xs_normed = norm of the tokens regrouped
    'b (p t) m -> (b t) p m' with the class token in front of every frame, [B*T, 1 + P, C]."""
    _check(x, norm, "add_layernorm_regrouped_native")
    return _AddLayerNormRegroupedFunction.apply(x, addend, norm.weight, norm.bias, norm.eps, int(T))


def add_layernorm(x, addend, norm, skip_first: bool = False, how=False):
    """`x = x + addend` (addend None: x as it is) and `y = norm(x)`: (x, y, skipped), or None.  skip_first: y without
    every clip's first row where x has one to leave out; `skipped` says whether it was.  how: the route, when the caller
    has asked it already."""
    how = route(x, norm, addend) if how is False else how
    if how is None:
        return None
    skip = bool(skip_first) and x.dim() == 3 and x.shape[1] >= 2
    if how == "direct":
        return (*_abi.add_layernorm(x, addend, norm.weight, norm.bias, norm.eps, skip_first=skip), skip)
    if how == AMP_DIRECT or how == AMP_FUNCTION:
        return (*_add_layernorm_amp(x, addend, norm, skip, how), skip)
    if addend is None:
        return x, layernorm_native(x, norm, skip_first=skip), skip
    return (*add_layernorm_native(x, addend, norm, skip_first=skip), skip)


def add_layernorm_regrouped(x, addend, frames: int, norm):
    """TimeSformer's mid-block step (see _abi.add_layernorm_regrouped): (x1, xs_normed), or None."""
    how = route(x, norm, addend, regrouped=True)
    if how == "direct":
        return _abi.add_layernorm_regrouped(x, addend, frames, norm.weight, norm.bias, norm.eps)
    return add_layernorm_regrouped_native(x, addend, frames, norm) if how == "function" else None
