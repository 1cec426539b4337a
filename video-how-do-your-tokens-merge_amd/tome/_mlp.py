"""The MLP of the patched blocks, `fc2(gelu(fc1(y)))` with the exact-erf GELU (`self.mlp(self.norm2(x))`,
tome/patch/videomae.py:29).  Participants: y and the four parameters.  None of them wants a gradient ("direct"): the
caller's own fc1 / `hidden` / fc2, the activation on tome_gelu_erf in place.  One does ("function"; needs enabled(), a
plain MLP whose dropouts are the identity, _abi.mlp_trainable): `mlp`, one autograd Function around the two library
GEMMs (models are patched for training, tools/train_net.py:727-741).  Otherwise the framework's modules.  `route` is
that decision alone, without a launch.

    mlp_native(mlp, y) -> mlp.fc2(gelu(mlp.fc1(y)))

Forward: fc1 as a library GEMM, tome_gelu_erf out of place, fc2 as a library GEMM -- the inference path's bits.  Saved:
y, the pre-activation h and the two weights; the activation is dropped (autograd keeps both hidden tensors: h for the
GELU, the activation for fc2's weight gradient).  Backward: ga = g W2, then ONE launch of tome_gelu_erf_backward
(csrc/tome_gelu_bwd.h) writes gh over ga, the activation again with the forward's bits (only when fc2's weight needs a
gradient) and fc1's bias gradient (only when it needs one); the remaining products are library GEMMs.
Double backward raises; the routing table is in DESIGN.md section 1.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _abi

# False: the callers in tome/patch/_common.py take the framework's modules and autograd (the behaviour before the
# backward kernel existed) -- for A/B in tests and tools/mlp_backward_bench.py.  Also off when tome.merge.NATIVE_BACKWARD
# is off.  On by default; what that rests on is said in DESIGN.md section 1.
NATIVE_MLP_BACKWARD = True


def enabled() -> bool:
    from . import merge
    return bool(NATIVE_MLP_BACKWARD and merge.NATIVE_BACKWARD)


def _stock_module(m, cls) -> bool:
    """`m` is exactly `cls` (not a subclass with a forward of its own: LoRA, quantised, ... layers), carries no
    parametrization and no forward hook -- only then may its forward be replaced by a hand-made call."""
    return (type(m) is cls and not getattr(m, "parametrizations", None)
            and not m._forward_hooks and not m._forward_pre_hooks)


def _plain_mlp(mlp, training: bool = False) -> bool:
    """An MLP of the usual shape: fc1, exact-erf nn.GELU, fc2 and dropouts -- all of them the stock modules, unhooked
    (feature extractors / flop counters hook mlp, act, fc2: those run the module itself) -- whose dropouts are the
    identity: the module in `.eval()` mode, or, with `training` (the native Function, tome/_mlp.py), in `.train()` mode
    as well when every nn.Dropout child has p == 0.  There a dropout is live by its OWN `.training` flag, the one its
    forward reads, whatever mode the MLP itself is in."""
    act = getattr(mlp, "act", None)
    fc1, fc2 = getattr(mlp, "fc1", None), getattr(mlp, "fc2", None)
    children = dict(mlp.named_children())
    return (act is not None and _stock_module(act, torch.nn.GELU) and getattr(act, "approximate", "none") == "none"
            and fc1 is not None and _stock_module(fc1, torch.nn.Linear)
            and fc2 is not None and _stock_module(fc2, torch.nn.Linear)
            and not mlp._forward_hooks and not mlp._forward_pre_hooks
            and set(children) <= {"fc1", "act", "fc2", "drop", "drop1", "drop2"}
            and (all(_stock_module(m, torch.nn.Dropout) and (m.p == 0 or not m.training)
                     for k, m in children.items() if k.startswith("drop")) if training else not mlp.training))


def route(mlp, y: torch.Tensor):
    """How `mlp(y)` runs: "direct" (neither y nor a parameter wants a gradient and the MLP is plain: the caller's own
    fc1, `hidden`, fc2), "function" (one does, and the native Function takes this MLP) or None (the module as it is)."""
    fc1, fc2, act = getattr(mlp, "fc1", None), getattr(mlp, "fc2", None), getattr(mlp, "act", None)
    if fc1 is None or fc2 is None or act is None:
        return None
    if not (torch.is_grad_enabled() and _abi.needs_grad(y, fc1.weight, fc1.bias, fc2.weight, fc2.bias)):
        return "direct" if _plain_mlp(mlp) else None
    return "function" if enabled() and _plain_mlp(mlp, training=True) and _abi.mlp_trainable(y, fc1, fc2, act) else None


def gelu_backward(h, ga, want_act, want_bias):
    """The backward arithmetic between the two GEMMs: (gh, act or None, db1 or None) from the saved pre-activation; gh
    is written over ga.  One module-level seam, so that a test can put another evaluation of the same formula in its
    place (or watch what is asked for)."""
    return _abi.gelu_erf_backward(h, ga, want_act=want_act, want_bias=want_bias, inplace=True)


class _MlpFunction(torch.autograd.Function):
    """fc2(gelu(fc1(y))): library GEMMs and tome_gelu_erf forward, tome_gelu_erf_backward between the GEMMs backward."""

    @staticmethod
    def forward(ctx, y, W1, b1, W2, b2):
        y2 = y.detach().reshape(-1, y.shape[-1])
        h = F.linear(y2, W1.detach(), None if b1 is None else b1.detach())
        a = _abi.gelu_erf(h, inplace=False)  # out of place: h is what the backward reads
        out = F.linear(a, W2.detach(), None if b2 is None else b2.detach())
        ctx.save_for_backward(y2, h, W1, W2)
        ctx.y_shape = y.shape
        return out.view(*y.shape[:-1], W2.shape[0])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        y2, h, W1, W2 = ctx.saved_tensors
        need_y, need_W1, need_b1, need_W2, need_b2 = ctx.needs_input_grad
        g2 = g.reshape(-1, g.shape[-1])
        g2 = g2 if g2.dtype == h.dtype else g2.to(h.dtype)
        gy = dW1 = db1 = dW2 = db2 = None
        if need_b2:
            db2 = g2.sum(0)
        if need_y or need_W1 or need_b1:
            ga = g2 @ W2  # a tensor of the Function's own: gh is written over it
            gh, a, db1 = gelu_backward(h, ga, need_W2, need_b1)
            if need_W1:
                dW1 = gh.t() @ y2
            if need_y:
                gy = (gh @ W1).view(ctx.y_shape)
        elif need_W2:
            a = _abi.gelu_erf(h, inplace=False)  # fc1 and y frozen: the activation alone, the forward's launch
        if need_W2:
            dW2 = g2.t() @ a
        return gy, dW1, db1, dW2, db2


def mlp_native(mlp, y: torch.Tensor) -> torch.Tensor:
    """`mlp.fc2(mlp.act(mlp.fc1(y)))` for tokens or parameters that require grad."""
    fc1, fc2, act = getattr(mlp, "fc1", None), getattr(mlp, "fc2", None), getattr(mlp, "act", None)
    if fc1 is None or fc2 is None or act is None or not _abi.mlp_trainable(y, fc1, fc2, act):
        raise _abi.TomeHipError(f"mlp_native: this MLP of {tuple(y.shape)} {y.dtype} tokens is not one the kernels take "
                                "(_abi.mlp_trainable)")
    return _MlpFunction.apply(y, fc1.weight, fc1.bias, fc2.weight, fc2.bias)


def hidden(mlp, y: torch.Tensor, kernel: bool = True) -> torch.Tensor:
    """fc1 and the activation of a plain MLP: the tensor its fc2 reads.  The activation runs on tome_gelu_erf (same
    bits as the framework's kernel, non-temporal streaming: 394 -> ~350 us at batch 128) when nothing wants a gradient
    of fc1's output, which requires grad when y or fc1's parameters do."""
    h = mlp.fc1(y)
    if kernel and _abi.gelu_ok(h):
        return _abi.gelu_erf(h, inplace=True)
    return mlp.act(h)


def mlp(module, y: torch.Tensor):
    """`module(y)` as the native Function when a gradient is wanted and the Function takes this MLP; None otherwise."""
    if not torch.is_grad_enabled():  # (no Function form: the no-grad forward is host-bound, spare it the look-ups of route)
        return None
    return mlp_native(module, y) if route(module, y) == "function" else None
