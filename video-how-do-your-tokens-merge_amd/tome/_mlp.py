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

ViViT's MLP is the HF pair instead of one module (`layer.intermediate`: dense -> gelu_fast, the tanh GELU -> dropout;
`layer.output`: dense -> dropout -> + residual; tome/patch/vivit.py:40-43).  `mlp_pair` runs the same Function on it
with the tanh form: tome_gelu_tanh forward, tome_gelu_tanh_backward between the backward's GEMMs.

    mlp_pair(intermediate, output, y) -> output.dense(act(intermediate.dense(y))), or None
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


def gelu_backward(h, ga, want_act, want_bias, form="erf"):
    """The backward arithmetic between the two GEMMs: (gh, act or None, db1 or None) from the saved pre-activation; gh
    is written over ga.  One module-level seam, so that a test can put another evaluation of the same formula in its
    place (or watch what is asked for).  form: "erf" (nn.GELU()) or "tanh" (ViViT's gelu_fast)."""
    backward = _abi.gelu_tanh_backward if form == "tanh" else _abi.gelu_erf_backward
    return backward(h, ga, want_act=want_act, want_bias=want_bias, inplace=True)


class _MlpFunction(torch.autograd.Function):
    """fc2(gelu(fc1(y))): library GEMMs and tome_gelu_erf / tome_gelu_tanh forward, tome_gelu_erf_backward /
    tome_gelu_tanh_backward between the GEMMs backward.  `form` ("erf" / "tanh") is not a tensor."""

    @staticmethod
    def forward(ctx, y, W1, b1, W2, b2, form):
        y2 = y.detach().reshape(-1, y.shape[-1])
        h = F.linear(y2, W1.detach(), None if b1 is None else b1.detach())
        gelu = _abi.gelu_tanh if form == "tanh" else _abi.gelu_erf
        a = gelu(h, inplace=False)  # out of place: h is what the backward reads
        out = F.linear(a, W2.detach(), None if b2 is None else b2.detach())
        ctx.save_for_backward(y2, h, W1, W2)
        ctx.y_shape = y.shape
        ctx.form = form
        return out.view(*y.shape[:-1], W2.shape[0])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        y2, h, W1, W2 = ctx.saved_tensors
        need_y, need_W1, need_b1, need_W2, need_b2 = ctx.needs_input_grad[:5]
        tanh = ctx.form == "tanh"
        g2 = g.reshape(-1, g.shape[-1])
        g2 = g2 if g2.dtype == h.dtype else g2.to(h.dtype)
        gy = dW1 = db1 = dW2 = db2 = None
        if need_b2:
            db2 = g2.sum(0)
        if need_y or need_W1 or need_b1:
            ga = g2 @ W2  # a tensor of the Function's own: gh is written over it
            # (the erf form keeps the seam's four arguments: a stand-in written for them still fits)
            gh, a, db1 = (gelu_backward(h, ga, need_W2, need_b1, "tanh") if tanh
                          else gelu_backward(h, ga, need_W2, need_b1))
            if need_W1:
                dW1 = gh.t() @ y2
            if need_y:
                gy = (gh @ W1).view(ctx.y_shape)
        elif need_W2:
            # fc1 and y frozen: the activation alone, the forward's launch
            a = (_abi.gelu_tanh if tanh else _abi.gelu_erf)(h, inplace=False)
        if need_W2:
            dW2 = g2.t() @ a
        return gy, dW1, db1, dW2, db2, None


def mlp_native(mlp, y: torch.Tensor) -> torch.Tensor:
    """`mlp.fc2(mlp.act(mlp.fc1(y)))` for tokens or parameters that require grad."""
    fc1, fc2, act = getattr(mlp, "fc1", None), getattr(mlp, "fc2", None), getattr(mlp, "act", None)
    if fc1 is None or fc2 is None or act is None or not _abi.mlp_trainable(y, fc1, fc2, act):
        raise _abi.TomeHipError(f"mlp_native: this MLP of {tuple(y.shape)} {y.dtype} tokens is not one the kernels take "
                                "(_abi.mlp_trainable)")
    return _MlpFunction.apply(y, fc1.weight, fc1.bias, fc2.weight, fc2.bias, "erf")


# ---- ViViT's pair: VivitIntermediate (dense, tanh GELU, dropout) and VivitOutput (dense, dropout, + residual) ----------
_TANH_ACTIVATIONS = ("FastGELUActivation", "NewGELUActivation", "PytorchGELUTanh", "GELUTanh")  # transformers.activations
_PAIR_CHILDREN = {"dense", "dropout", "intermediate_act_fn"}


def _tanh_gelu(act) -> bool:
    """A module that computes the tanh GELU: the stock nn.GELU(approximate="tanh"), or one of HF's activation classes
    (matched by module and class name: transformers is not imported), unhooked."""
    if act is None or getattr(act, "_forward_hooks", None) or getattr(act, "_forward_pre_hooks", None):
        return False
    cls = type(act)
    if cls is torch.nn.GELU:
        return getattr(act, "approximate", "none") == "tanh"
    return cls.__module__ == "transformers.activations" and cls.__name__ in _TANH_ACTIVATIONS


def _pair_half(m, name: str) -> bool:
    """One module of the pair as HF lays it out: the class name, no hooks, no forward put on the instance, a stock
    `dense`, no child beyond dense / dropout / intermediate_act_fn, every dropout the identity by its OWN flag."""
    if type(m).__name__ != name or m._forward_hooks or m._forward_pre_hooks or "forward" in m.__dict__:
        return False
    children = dict(m.named_children())
    dense = children.get("dense")
    return (dense is not None and _stock_module(dense, torch.nn.Linear) and set(children) <= _PAIR_CHILDREN
            and all(_stock_module(d, torch.nn.Dropout) and (d.p == 0 or not d.training)
                    for k, d in children.items() if k == "dropout"))


# (rows, C, Hd) at which tools/vivit_backward_bench.py found the native path slower than the switch-off path by more than
# the larger of the two paths' min-max spreads (1337 against 1302 us at 8 x 3137 rows with fc2
# trainable; ties at 2 x 3137 rows, with fc2 frozen, and on the two-layer stack)
_PAIR_EXCLUDED = frozenset({(8 * 3137, 768, 3072)})


def pair_trainable(intermediate, output, y: torch.Tensor) -> bool:
    """Can `output.dense(act(intermediate.dense(y)))` run as the Function with the tanh form?  The modules are ViViT's
    pair (_pair_half), the activation a tanh GELU that belongs to `intermediate` alone, and the tensors those of
    _abi.mlp_tensors_trainable."""
    if not (_pair_half(intermediate, "VivitIntermediate") and _pair_half(output, "VivitOutput")
            and "intermediate_act_fn" not in dict(output.named_children())
            and _tanh_gelu(getattr(intermediate, "intermediate_act_fn", None))):
        return False
    fc1, fc2 = intermediate.dense, output.dense
    return (_abi.mlp_tensors_trainable(y, fc1, fc2)
            and (y.numel() // y.shape[-1], fc1.in_features, fc1.out_features) not in _PAIR_EXCLUDED)


def route_pair(intermediate, output, y: torch.Tensor):
    """How ViViT's MLP runs: "function" (y or one of the four parameters wants a gradient and the Function takes the
    pair) or None (the modules as they are; without grad always: the inference path is the host's own)."""
    fc1, fc2 = getattr(intermediate, "dense", None), getattr(output, "dense", None)
    if not (torch.is_grad_enabled() and isinstance(fc1, torch.nn.Linear) and isinstance(fc2, torch.nn.Linear)
            and _abi.needs_grad(y, fc1.weight, fc1.bias, fc2.weight, fc2.bias)):
        return None
    return "function" if enabled() and pair_trainable(intermediate, output, y) else None


def mlp_pair(intermediate, output, y: torch.Tensor):
    """`output.dense(act(intermediate.dense(y)))` as the native Function (the residual add is the caller's), or None
    when no gradient is wanted or the Function does not take this pair."""
    if not torch.is_grad_enabled():  # (as `mlp`: the no-grad forward looks nothing up)
        return None
    if route_pair(intermediate, output, y) != "function":
        return None
    fc1, fc2 = intermediate.dense, output.dense
    return _MlpFunction.apply(y, fc1.weight, fc1.bias, fc2.weight, fc2.bias, "tanh")


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
