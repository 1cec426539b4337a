"""The MLP of the patched blocks, `fc2(gelu(fc1(y)))` with the exact-erf GELU, for tokens or parameters that require grad
(models are patched for training, tools/train_net.py:727-741; `self.mlp(self.norm2(x))`, tome/patch/videomae.py:29):
one autograd Function around the two library GEMMs.

    mlp_native(mlp, y) -> mlp.fc2(gelu(mlp.fc1(y)))

Forward: fc1 as a library GEMM, tome_gelu_erf out of place, fc2 as a library GEMM -- the inference path's bits.  Saved:
y, the pre-activation h and the two weights; the activation is dropped (autograd keeps both hidden tensors: h for the
GELU, the activation for fc2's weight gradient).  Backward: ga = g W2, then ONE launch of tome_gelu_erf_backward
(csrc/tome_gelu_bwd.h) writes gh over ga, the activation again with the forward's bits (only when fc2's weight needs a
gradient) and fc1's bias gradient (only when it needs one); the remaining products are library GEMMs.
Not covered (they keep the framework's ops: DESIGN.md section 7): the tanh GELU, fp32 tokens, live dropout, hooked or
subclassed layers, double backward (raises).
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


def wants(mlp, y: torch.Tensor) -> bool:
    """Does y or a parameter of this MLP require grad, and does the MLP run on the native Function?"""
    if not (torch.is_grad_enabled() and enabled()):
        return False
    fc1, fc2, act = getattr(mlp, "fc1", None), getattr(mlp, "fc2", None), getattr(mlp, "act", None)
    if fc1 is None or fc2 is None or act is None:
        return False
    params = (fc1.weight, fc1.bias, fc2.weight, fc2.bias)
    return ((y.requires_grad or any(p is not None and p.requires_grad for p in params))
            and _abi.mlp_trainable(y, fc1, fc2, act))


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
