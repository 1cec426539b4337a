"""Shared machinery of the four model patches (reference: tome/patch/{videomae,timesformer,motionformer,
vivit}.py).  The reference imports the concrete slowfast / HF classes and swaps ``__class__``; here the
ToMe subclasses are created on the fly from whatever class the module already has, so the same patch
works on the reference's own model objects and on the host models of this repository
(``video-how-do-your-tokens-merge_amd/hosts``) without importing slowfast.
"""
from __future__ import annotations

import os
import threading
from typing import Callable, Dict, Tuple

import torch

from .. import _abi, _attn, _ln, _mlp, _overlap
from .. import merge as tm
from .._mlp import _plain_mlp, _stock_module  # (the module-kind predicates live beside the MLP's route)
from ..merge import (bipartite_soft_matching, bipartite_soft_matching_drop, bipartite_soft_matching_hybrid, do_nothing,
                     drop_regrouped, merge_source, merge_wavg, merge_wavg_regrouped)
from ..utils import parse_r

_SUBCLASSES: Dict[Tuple[type, str], type] = {}
_FUSE_LN = os.environ.get("TOME_FUSE_LN", "1") != "0"  # measurement switch: 0 = merge and LayerNorm as two steps
_FUSE_ADD = os.environ.get("TOME_FUSE_ADD", "1") != "0"  # measurement switch: 0 = residual add as its own pass
# 0 = only plain 'merge' takes the fused reduction + LayerNorm launch; drop, hybrid and the random modes run add, reduction
# and LayerNorm as three steps
_FUSE_MODES = os.environ.get("TOME_FUSE_MODES", "1") != "0"
_FUSE_NEXT = os.environ.get("TOME_FUSE_NEXT", "1") != "0"  # 0 = second residual and the next block's norm1 separate
_ATTN_KERNEL = os.environ.get("TOME_ATTN_KERNEL", "1") != "0"  # 0 = the framework's fused attention (+ bias tensor)
_GELU_KERNEL = os.environ.get("TOME_GELU_KERNEL", "1") != "0"  # 0 = the framework's GELU pass inside the MLP
_FUSE_FC2 = os.environ.get("TOME_FUSE_FC2", "1") != "0"  # 0 = the MLP's second GEMM writes its own tensor, then an add
# 0 = the last block of a mean-pooling ViT runs fc2 over every token and hands [B, T', C] to the host's `x.mean(1)`
_POOL_TAIL = os.environ.get("TOME_POOL_TAIL", "1") != "0"
_SKIP_FIRST = os.environ.get("TOME_SKIP_FIRST", "1") != "0"  # the temporal hand-over without the class row


def swizzle(module: torch.nn.Module, tag: str, methods: dict) -> None:
    """Give ``module`` a subclass of its current class carrying ``methods`` (the reference assigns
    ``module.__class__ = ToMeBlock``; same effect, no dependency on the concrete base class)."""
    base = module.__class__
    if getattr(base, "_tome_tag", None) == tag:
        return
    key = (base, tag)
    sub = _SUBCLASSES.get(key)
    if sub is None:
        sub = type(tag, (base,), dict(methods, _tome_tag=tag))
        _SUBCLASSES[key] = sub
    module.__class__ = sub


def has_tag(module, tag: str) -> bool:
    return getattr(module.__class__, "_tome_tag", None) == tag


def new_tome_info(trace_source, prop_attn, mode, head_aggregation, threshold, verbose, class_token) -> dict:
    """The shared per-model state dict (videomae.py:181-193)."""
    return {
        "r": 0,
        "size": None,
        "source": None,
        "trace_source": trace_source,
        "prop_attn": prop_attn,
        "verbose": verbose,
        "class_token": class_token,
        "distill_token": False,
        "mode": mode,
        "head_aggregation": head_aggregation,
        "threshold": threshold,
    }


# One forward in flight per process.  Two forwards (patched or not) issued on two HIP streams of one process never
# finish on this platform: two chains of plain library GEMMs (`torch.mm`, nothing of this package) on two streams are
# not finished after 20 s where one stream takes 88 ms (tools/probes/two_stream_gemm.py,
# profiles/r03_two_stream_gemm_probe.txt).  Every GEMM of these models -- under either BLAS preference, as the kernel
# trace in profiles/r04_two_stream_probe_rocblas_kernel.txt shows -- is a persistent Stream-K grid (`..._SK3_...`, one
# workgroup per CU, workgroups spin on each other's partial tiles); two such grids resident at once waiting on
# siblings that cannot be scheduled is the likely cause, but the probe has no non-Stream-K control, so the rule below
# is stated for "two concurrent library GEMM grids".
# The reference's own contract is one forward at a time per model (`_tome_info` is shared state, SURVEY 8b
# "Threading").  So: (1) the ENQUEUEING of a patched forward holds a per-device lock -- a second host thread that
# starts a forward while the first is still issuing kernels (launches release the GIL) waits at the entry, and finds
# the first one's end event when it gets in; (2) a patched forward issued while another one is still in flight on a
# different stream is ORDERED behind it (the stream waits for the other forward's end event; said once in a warning)
# instead of hanging the device: two streams then buy no overlap, and nothing deadlocks.  TOME_ONE_FORWARD=raise
# refuses instead.
_in_flight = {}  # device index -> (stream id, event recorded behind the last patched forward)
_issue_locks: Dict[int, "threading.RLock"] = {}
_issue_locks_guard = threading.Lock()
_warned_two_streams = False


def _current_stream(device):
    """(stream id, stream) of the caller's current HIP stream -- a seam for the CPU-side test of the bookkeeping."""
    cur = torch.cuda.current_stream(device)
    return cur.cuda_stream, cur


def _record_event(stream):
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def _guarded(device) -> bool:
    return device.type == "cuda" and not torch.cuda.is_current_stream_capturing()
    # (a captured forward is ordered by the graph it is replayed from)


def _issue_lock(device):
    with _issue_locks_guard:
        lock = _issue_locks.get(device.index)
        if lock is None:
            lock = _issue_locks[device.index] = threading.RLock()
        return lock


def _guard_one_forward_in_flight(device) -> None:
    """Called at the ENTRY of a patched forward, with the device's issue lock held."""
    global _warned_two_streams
    sid, cur = _current_stream(device)
    last = _in_flight.get(device.index)
    if last is None or last[0] == sid or last[1].query():
        return
    msg = ("a forward issued on another HIP stream of this process is still in flight: the library GEMMs of two "
           "concurrent forwards never finish on this platform")
    if os.environ.get("TOME_ONE_FORWARD", "order") == "raise":
        raise RuntimeError(msg + ".  Run one forward at a time per process (one process per GPU).")
    cur.wait_event(last[1])
    if not _warned_two_streams:
        _warned_two_streams = True
        import warnings
        warnings.warn(msg + "; this forward has been ordered behind it (no overlap between the two streams).",
                      RuntimeWarning, stacklevel=3)


def _note_forward_issued(device) -> None:
    sid, cur = _current_stream(device)
    _in_flight[device.index] = (sid, _record_event(cur))


class one_forward_at_a_time:
    """Context of one patched forward on `device`: takes the device's issue lock (re-entrant: a patched model called
    from inside another patched forward of the same thread), orders the caller's stream behind a forward still in
    flight on another stream, and records the end event on exit -- also when the forward raises, since whatever it
    enqueued before raising is in flight all the same."""

    def __init__(self, device):
        self.device = device
        self.on = device is not None and _guarded(device)

    def __enter__(self):
        if self.on:
            self.lock = _issue_lock(self.device)
            self.lock.acquire()
            try:
                _guard_one_forward_in_flight(self.device)
            except BaseException:
                self.lock.release()
                raise
        return self

    def __exit__(self, *exc):
        if self.on:
            try:
                _note_forward_issued(self.device)
            finally:
                self.lock.release()
        return False


def wrap_model_forward(model_wrapper: torch.nn.Module, blocks_of: Callable, pool_tail: Callable = None) -> None:
    """make_tome_class (videomae.py:160-169): every forward re-reads ``self.r`` into a per-layer list and
    clears size/source.  pool_tail(wrapper) -> the last block when this forward's head reads that block's output through
    an unweighted token mean alone (tome/patch/videomae.py::pooled_tail_block), else None: the block is named in
    `_tome_info["_pool_tail"]` for this forward only, and may then return the pooled row (pooled_tail)."""
    base = model_wrapper.__class__
    if getattr(base, "_tome_tag", None) == "ToMeVisionTransformer":
        return

    def forward(self, *args, **kwdargs):
        param = next(self.parameters(), None)
        with one_forward_at_a_time(None if param is None else param.device):
            # (the shared state is reset under the lock: `_tome_info` belongs to the forward that holds it)
            self._tome_info["r"] = parse_r(len(blocks_of(self)), self.r)
            self._tome_info["size"] = None
            self._tome_info["source"] = None
            self._tome_info.pop("_prenorm", None)
            self._tome_info.pop("_folded", None)
            armed = pool_tail(self) if (pool_tail is not None and _POOL_TAIL) else None
            if armed is not None:
                self._tome_info["_pool_tail"] = armed
            try:
                return super(sub, self).forward(*args, **kwdargs)
            finally:
                self._tome_info.pop("_pool_tail", None)  # (a block called on its own never finds it)
                if param is not None:
                    _overlap.join(param.device)  # (a matching on the side stream no block waited for: a raise mid-block)

    sub = type("ToMeVisionTransformer", (base,), {"forward": forward, "_tome_tag": "ToMeVisionTransformer"})
    model_wrapper.__class__ = sub


keys_ready = _overlap.keys_ready      # the block's matching beside its attention, on a second HIP stream:
match_beside = _overlap.match_beside  # tome/_overlap.py


def attention_qkv(qkv, size, scale: float, dropout_p: float = 0.0, bias_skip: bool = False):
    """`attention(qkv[0], qkv[1], qkv[2], ...)` for the [3, B, H, N, hd] view of one qkv projection."""
    return attention(qkv[0], qkv[1], qkv[2], size, scale, dropout_p, bias_skip, qkv)


def attention(q, k, v, size, scale: float, dropout_p: float = 0.0, bias_skip: bool = False, qkv=None):
    """softmax(q k^T * scale + log(size)) v for [B, H, N, hd] head views; returns [B, N, H*hd].
    16-bit heads of width 64 without dropout go through tome_prop_attention (the size bias is one value per key inside
    the kernel, q/k/v are read in place from the projection's output; under grad as a Function: tome/_attn.py), everything
    else through the framework's attention with the bias tensor the reference builds (videomae.py:62-63, timesformer.py:73-74)."""
    out = _attn.attention(q, k, v, size, scale, dropout_p, bias_skip, qkv) if _ATTN_KERNEL else None
    if out is not None:
        return out
    B, H, N, hd = q.shape
    bias = None
    if size is not None:
        log = _abi.log_of_size(size)[:, None, None, :, 0].to(q.dtype)
        if bias_skip:
            bias = torch.zeros(B, 1, N, N, dtype=q.dtype, device=q.device)
            bias[:, :, 1:, 1:] = log
        else:
            bias = log
    out = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=bias, dropout_p=dropout_p, scale=scale)
    return out.transpose(1, 2).reshape(B, N, H * hd)


def _mlp_steps(mlp, y):
    """`mlp(y)` without the native Function: a plain MLP step by step (tome/_mlp.py::hidden), anything else as it is."""
    return mlp.fc2(_mlp.hidden(mlp, y, _GELU_KERNEL)) if _plain_mlp(mlp) else mlp(y)


def run_mlp(mlp, y):
    """`self.mlp(y)` of the patched block (tome/patch/videomae.py:29); anything but a plain MLP is called as it is."""
    out = _mlp.mlp(mlp, y) if _GELU_KERNEL else None
    return _mlp_steps(mlp, y) if out is None else out


def foldable(linear, eval_mode: bool = True):
    """`linear` when the block's last step `x = x + linear(h)` may run as ONE GEMM that accumulates onto the residual
    stream in place (`x.addmm_(h, Wᵀ)`, finish_linear) -- which needs the bias in the stream beforehand
    (merge_then_norm's `fold`, the merge kernel's x_out_bias); None when it may not."""
    if (_FUSE_FC2 and _FUSE_NEXT and eval_mode and _stock_module(linear, torch.nn.Linear) and linear.bias is not None
            and not (torch.is_grad_enabled() and _abi.needs_grad(linear.weight, linear.bias))):
        return linear
    return None


def mlp_residual(block, mlp, x, y, info, scale=None, drop_path=None):
    """`x + drop_path(scale * mlp(y))` at the end of a patched block (tome/patch/videomae.py:28-29,
    timesformer.py:57, motionformer.py:30), with the next block's first norm handed over (finish_block)."""
    folded = info.get("_folded")
    waiting = folded is not None and folded[0] is x  # fc2's bias sits in the residual stream x: finish_linear's to finish
    out = _mlp.mlp(mlp, y) if _GELU_KERNEL and not waiting else None
    if out is None:
        if _plain_mlp(mlp) and scale is None and (drop_path is None or not block.training):
            return finish_linear(block, x, _mlp.hidden(mlp, y, _GELU_KERNEL), mlp.fc2, info)
        if waiting:
            raise RuntimeError("the residual stream carries a folded bias, but the block's MLP is not the one it was folded for")
        out = _mlp_steps(mlp, y)
    if scale is not None:
        out = scale * out
    return finish_block(block, x, out if drop_path is None else drop_path(out), info)


def _unhooked(*modules) -> bool:
    return not any(m._forward_hooks or m._forward_pre_hooks for m in modules)


def pool_tail_modules_ok(vit, block) -> bool:
    """The module side of the pooled tail's predicate, no tensor and no device involved: `vit` pools its last block's
    output by an unweighted token mean (`norm` the identity, `fc_norm` a LayerNorm), in `.eval()` mode, and `block`, its
    last, is a plain ToMeBlock -- no layer scale, identity drop_path, a plain MLP with a biased fc2, one 16-bit dtype for
    norm2 / fc1 / fc2 -- and nobody observes the block's output: no forward hook or pre-hook on the ViT, its norm, the
    block (the MLP's modules: _plain_mlp), and none registered for all modules."""
    from torch.nn.modules import module as _m
    if _m._global_forward_hooks or _m._global_forward_pre_hooks:
        return False
    norm, fc_norm = getattr(vit, "norm", None), getattr(vit, "fc_norm", None)
    if not (type(norm) is torch.nn.Identity and isinstance(fc_norm, torch.nn.LayerNorm) and not vit.training
            and not block.training and has_tag(block, "ToMeBlock") and getattr(block, "gamma_2", 0) is None
            and type(getattr(block, "drop_path", None)) is torch.nn.Identity
            and _unhooked(vit, norm, block, block.drop_path) and _plain_mlp(block.mlp)):
        return False
    fc1, fc2, norm2 = block.mlp.fc1, block.mlp.fc2, getattr(block, "norm2", None)
    dtype = fc2.weight.dtype
    return (fc2.bias is not None and dtype in _abi._HALF and fc1.weight.dtype == dtype
            and isinstance(norm2, torch.nn.LayerNorm) and norm2.elementwise_affine and norm2.weight.dtype == dtype
            and fc1.in_features % 8 == 0 and fc1.out_features % 8 == 0 and fc2.out_features == fc1.in_features)


def pool_tail_armed(block, x, info) -> bool:
    """At the top of `block`: is it the one this forward named for the pooled tail (popped here), and are these the
    tokens the tail takes -- 16-bit device tokens of the MLP's dtype, no grad mode, no autocast?"""
    if info.get("_pool_tail") is not block:
        return False
    info.pop("_pool_tail")
    return (x.is_cuda and x.dim() == 3 and x.dtype == block.mlp.fc2.weight.dtype and not torch.is_grad_enabled()
            and not torch.is_autocast_enabled("cuda"))


def pooled_tail(mlp, x, y):
    """The end of the last block of a mean-pooling ViT, `mean_t(x + fc2(gelu(fc1(y))))` as [B, 1, C]: the mean commutes
    with everything behind the activation, so fc2 multiplies one row per clip,
        mean_t(x_t) + b2 + W2 mean_t(a_t),      a = gelu(fc1(y)),
    with both means on tome_token_mean (the second of the bits tome_gelu_erf would have stored; the activation is never
    written) and fp32 from the means to the one rounding at the end.  x: the merged stream WITHOUT fc2's bias folded in."""
    h = mlp.fc1(y)
    abar = _abi.token_mean(h if h.is_contiguous() else h.contiguous(), gelu=True)
    xbar = _abi.token_mean(x if x.is_contiguous() else x.contiguous())
    fc2 = mlp.fc2
    pooled = torch.addmm(xbar + fc2.bias.float(), abar, fc2.weight.float().t())
    return pooled.to(x.dtype)[:, None, :]


def pick_reduction(mode: str, merge_fn, drop_fn, hybrid_fn):
    if mode in ("merge", "random_merge"):
        return merge_fn
    if mode in ("drop", "random_drop"):
        return drop_fn
    if mode in ("hybrid",):
        return hybrid_fn
    raise ValueError(f"unknown ToMe mode {mode!r}")


def matching(kind: str, metric, r: int, info):
    """This layer's matching for a reduction of `kind` ("merge", "hybrid" or "drop": fused_kind): the callable that carries
    `.plan` -- merge(x, mode) or drop(x) -- or None when the clamped r is 0, which the matchings report as the
    (do_nothing, do_nothing) pair."""
    if kind == "drop":
        found = bipartite_soft_matching_drop(metric, r, info["class_token"], info["distill_token"], info["mode"])
    elif kind == "hybrid":
        found = bipartite_soft_matching_hybrid(metric, r, info["class_token"], info["distill_token"], info["mode"],
                                               info["threshold"])
    else:
        found = bipartite_soft_matching(metric, r, info["class_token"], info["distill_token"], info["mode"])
    if isinstance(found, tuple):  # (merge, unmerge); the drop matching answers with a pair for a clamped r of 0 alone
        found = found[0]
    return None if found is do_nothing else found


# ---- the reduction step on an already grouped [n, T, C] token tensor ---------------------------------
def reduce_merge(metric, x, info, r):
    return _apply_merge(matching("merge", metric, r, info) or do_nothing, x, info)


def _apply_merge(merge, x, info):
    """The steps behind the matching of reduce_merge / reduce_hybrid: source tracking, merge_wavg, the sizes."""
    if info["trace_source"]:
        info["source"] = merge_source(merge, x, info["source"])
    before = x.size(1)
    x, info["size"] = merge_wavg(merge, x, info["size"], log_size=info["prop_attn"])
    if info["verbose"]:
        print(f"Merged {before} to {x.size(1)} tokens")
    return x


def link_next_norms(blocks, norm_attr: str, tag: str = "ToMeBlock", skip_first: bool = False) -> None:
    """Tell every patched block which LayerNorm reads its output (the next block's first norm), so the block's
    last residual add can hand that norm's result over (finish_block / first_norm).  Stored without registering
    the norm as a submodule of the previous block.  skip_first: that norm's consumer reads `norm(x)[:, 1:]` only
    (TimeSformer's temporal_norm1), so the hand-over leaves the class-token row out."""
    blocks = list(blocks)
    for cur, nxt in zip(blocks, blocks[1:]):
        target = getattr(nxt, norm_attr, None) if has_tag(nxt, tag) and nxt is not cur else None
        object.__setattr__(cur, "_tome_next_norm", target)
        object.__setattr__(cur, "_tome_next_skip_first", bool(skip_first) and _SKIP_FIRST)
    if blocks:
        object.__setattr__(blocks[-1], "_tome_next_norm", None)


def first_norm(block, x, info, norm, skip_first: bool = False):
    """norm(x) at the top of a block -- taken from the previous block's fused add+LayerNorm when it left one
    for exactly this tensor.  skip_first: returns norm(x)[:, 1:] (contiguous when it comes from the hand-over)."""
    pre = info.pop("_prenorm", None)
    if pre is not None and pre[0] is x and pre[2] is norm:
        if bool(pre[3]) == bool(skip_first):
            return pre[1]
        if skip_first:  # a full hand-over for a reader of the patch rows
            return pre[1][:, 1:, :]
    # no hand-over (first block, or a block after one that could not fuse): the same streaming LayerNorm kernel,
    # without an addend (6.4 TB/s against 2 TB/s for the framework's LayerNorm on these shapes)
    out = _ln.add_layernorm(x, None, norm, skip_first) if _FUSE_NEXT else None
    if out is None:
        return norm(x)[:, 1:, :] if skip_first else norm(x)
    _, y, skipped = out
    return y[:, 1:, :] if (skip_first and not skipped) else y


def _hand_over(block, x, addend, info):
    """x [+ addend] and the next block's first LayerNorm of it in one launch (tome/_ln.py), left in info["_prenorm"] for
    that block's first_norm; returns the sum, or None when nothing was launched."""
    nxt = getattr(block, "_tome_next_norm", None)
    out = None if nxt is None else _ln.add_layernorm(x, addend, nxt, getattr(block, "_tome_next_skip_first", False))
    if out is None:
        return None
    x, h, skipped = out
    info["_prenorm"] = (x, h, nxt, skipped)
    return x


def finish_block(block, x, residual, info):
    """x + residual at the end of a block; when the next block's first LayerNorm is known and the tokens are
    16-bit, tome_add_layernorm produces the sum and that norm's output together."""
    out = _hand_over(block, x, residual, info) if _FUSE_NEXT else None
    return x + residual if out is None else out


def finish_linear(block, x, h, linear, info):
    """`x + linear(h)` at the end of a block.  When the merge kernel has put linear's bias into x already (`fold`),
    the GEMM accumulates onto x in place (beta = 1: no tensor for the GEMM's result, no add pass) and the next block's
    first LayerNorm reads the finished sum once (tome_add_layernorm without addend); otherwise finish_block."""
    folded = info.pop("_folded", None)
    if folded is None or folded[0] is not x:
        return finish_block(block, x, linear(h), info)
    if folded[1] is not linear:
        raise RuntimeError("the residual stream carries the bias of another Linear than the one that finishes the block")
    x.view(-1, x.shape[-1]).addmm_(h.view(-1, h.shape[-1]), linear.weight.t())
    _hand_over(block, x, None, info)
    return x


def _trailing_norm(x, norm):
    """norm(x) behind a reduction step that ran on its own (the fused merge + LayerNorm launch is inference-only): the
    streaming LayerNorm kernel as a Function (tome/_ln.py) when a gradient is wanted, the framework's otherwise; under
    autocast the mixed-precision form of that kernel in both grad modes when the route offers it."""
    if _FUSE_LN and torch.is_grad_enabled():  # (without autocast the no-grad layer stops here, as it always has)
        how = _ln.route(x, norm)
        if how == "function" or how == _ln.AMP_FUNCTION or how == _ln.AMP_DIRECT:
            return _ln.add_layernorm(x, None, norm, how=how)[1]
    elif _FUSE_LN and _abi.autocast_dtype(x.device) is not None:
        # under autocast the mixed-precision launch in no-grad too: the framework's fp32 LayerNorm writes fp32 and the
        # Linear behind it casts (tome/_ln.py)
        how = _ln.route(x, norm)
        if how == _ln.AMP_DIRECT:
            return _ln.add_layernorm(x, None, norm, how=how)[1]
    return norm(x)


def fused_kind(mode: str, is_merge: bool, is_drop: bool = False, is_hybrid: bool = False):
    """Which reduction + LayerNorm launch a block in `mode` may take, given which of the model's reduction functions it
    carries: "merge" (tome_merge_wavg_ln), "hybrid" (the same entry with the plan's threshold flags), "drop"
    (tome_drop_ln), or None: the reduction runs on its own.  With _FUSE_MODES off only plain 'merge' has one."""
    if is_merge and (mode == "merge" or (_FUSE_MODES and mode == "random_merge")):
        return "merge"
    if _FUSE_MODES and is_drop and mode in ("drop", "random_drop"):
        return "drop"
    if _FUSE_MODES and is_hybrid and mode == "hybrid":
        return "hybrid"
    return None


def _fold_for(fold, x, mode: str):
    """`fold` when the fused launch may put that Linear's bias into the stream x: a bias of x's dtype and width, in plain
    'merge' mode only.  The fold moves a rounding -- round(round(x' + b) + h W) for round(x' + round(h W + b)) -- and one
    bf16 bit in the stream is enough to reorder near-tied scores in the next layer's matching.  Plain merge has always
    accepted that; drop, hybrid and the random modes keep the stream of the three steps, so that TOME_FUSE_MODES changes no
    matching (tests/test_modes_models_gpu.py)."""
    if fold is None or mode != "merge" or fold.bias.dtype != x.dtype or fold.bias.numel() != x.shape[-1]:
        return None
    return fold


# True: a flat-layout block (VideoMAE, ViViT) in mode 'merge' / 'random_merge' / 'drop' / 'random_drop' whose tokens,
# residual or norm require grad takes the fused add + reduction + LayerNorm launch as an autograd Function
# (tome/_ln.py::_MergeLnFunction, tome_merge_ln_backward behind it) where _abi.merge_ln_trainable holds, instead of the
# three steps `x + residual`, the merge Function and the LayerNorm Function.  Off by default: what that rests on is
# said in DESIGN.md section 1 (measure with tools/merge_ln_backward_bench.py).
TRAIN_FUSED_LN = False

# True: under torch.autocast (fp32 LayerNorm parameters, a 16-bit or fp32 residual stream) a flat-layout block (VideoMAE,
# ViViT) of kind "merge", "hybrid" or "drop" (fused_kind) with nothing wanting a gradient and no trace_source takes the
# residual add, the reduction and the LayerNorm as ONE launch (tome_merge_wavg_ln_amp / tome_drop_ln_amp) instead of the
# framework's add, the reduction kernel and tome_add_layernorm_amp.  The stream and the sizes keep their bits; y is the
# same LayerNorm of the same stored rows by another fp32 summation order.  Yields to tome._ln.NATIVE_LN_AUTOCAST = False,
# TOME_FUSE_LN=0, TOME_FUSE_MODES=0 (all kinds but plain merge) and TOME_FUSE_ADD=0 (the add stays the framework's).  Off
# by default: what that rests on is said in DESIGN.md section 1 (measure with tools/autocast_merge_ln_bench.py).
AUTOCAST_FUSED_LN = False


def fused_route(kind, x, norm, residual, info):
    """How a flat-layout layer runs `x + residual`, its reduction of `kind` (fused_kind) and `norm` as ONE launch, asked
    before the matching exists: "direct" (tome_merge_wavg_ln / tome_drop_ln: 16-bit tokens, nothing wants a gradient),
    "function" (the same launch as tome/_ln.py::_MergeLnFunction: TRAIN_FUSED_LN, a participant wants one),
    _ln.AMP_DIRECT (tome_merge_wavg_ln_amp / tome_drop_ln_amp: AUTOCAST_FUSED_LN under autocast, nothing wants one),
    _ln.AMP_FUNCTION (the same two launches as tome/_ln.py::_MergeLnAmpFunction, tome_merge_ln_backward_amp behind them:
    tome._ln.NATIVE_MERGE_LN_AUTOCAST_BACKWARD under autocast, a participant wants one), or None: the three steps.
    residual: what the launch would read beside x (None: x is the finished sum).
    The switched answers are tome.merge._ln_route's rule about the tensors, asked without a matching; the patch
    layer's own gates go on top: the Functions cover the kinds "merge" and "drop" and sizes as the previous launch left
    them, no switched answer tracks sources, and all want a clamped r > 0 up front (their launches have no r == 0
    form)."""
    r_list = info["r"]
    if not (_FUSE_LN and kind is not None and r_list and r_list[0] > 0):
        return None
    train_amp = _ln.NATIVE_MERGE_LN_AUTOCAST_BACKWARD
    if (TRAIN_FUSED_LN or AUTOCAST_FUSED_LN or train_amp) and not info["trace_source"]:
        size = info["size"]
        if torch.is_grad_enabled() and _abi.needs_grad(x, residual, norm.weight, norm.bias):
            want = TRAIN_FUSED_LN and kind != "hybrid" and "function"
            if size is not None and (size.device != x.device or size.shape != (x.shape[0], x.shape[1], 1)):
                want = False
            elif (train_amp and kind != "hybrid" and _abi.autocast_dtype(x.device) is not None
                  and tm._ln_route(None, x, norm, residual, size) == _ln.AMP_FUNCTION):
                want = _ln.AMP_FUNCTION  # (fp32 LayerNorm parameters under autocast: never the 16-bit Function's tensors)
            addend = residual  # (the Functions read the residual themselves, whatever _FUSE_ADD says)
        else:
            want = AUTOCAST_FUSED_LN and _abi.autocast_dtype(x.device) is not None and _ln.AMP_DIRECT
            addend = residual if _FUSE_ADD else None  # (else the framework adds first, and the sum is asked again)
        if (want and tm._ln_route(None, x, norm, addend, size) == want
                and _abi.effective_r(x.shape[1], r_list[0], info["class_token"], info["distill_token"]) > 0):
            return want
    return "direct" if _abi.ln_fusable(x, norm, residual) else None


# (route, is it a drop) -> the launch behind the matching `m`: (x, y, size) of a merge, (x, y) of a drop.  Every entry is
# looked up on its module at the call: the stage timers and the route tables replace them there.
_LAUNCH = {
    ("direct", False): lambda m, x, info, norm, addend, fold: _abi.merge_wavg_ln(
        m.plan, x, info["size"], norm.weight, norm.bias, norm.eps, addend=addend, log_size=info["prop_attn"],
        out_bias=None if fold is None else fold.bias),
    ("direct", True): lambda m, x, info, norm, addend, fold: _abi.drop_ln(
        m.plan, x, norm.weight, norm.bias, norm.eps, addend=addend, out_bias=None if fold is None else fold.bias),
    ("function", False): lambda m, x, info, norm, addend, fold: tm.merge_wavg_ln(
        m, x, info["size"], norm, addend, log_size=info["prop_attn"]),
    ("function", True): lambda m, x, info, norm, addend, fold: tm.drop_ln(m, x, norm, addend),
    (_ln.AMP_DIRECT, False): lambda m, x, info, norm, addend, fold: _abi.merge_wavg_ln_amp(
        m.plan, x, info["size"], norm.weight, norm.bias, norm.eps, _abi.autocast_dtype(x.device), addend=addend,
        log_size=info["prop_attn"]),
    (_ln.AMP_DIRECT, True): lambda m, x, info, norm, addend, fold: _abi.drop_ln_amp(
        m.plan, x, norm.weight, norm.bias, norm.eps, _abi.autocast_dtype(x.device), addend=addend),
    # (the public calls route once more, now with the plan: _MergeLnAmpFunction while the switch holds)
    (_ln.AMP_FUNCTION, False): lambda m, x, info, norm, addend, fold: tm.merge_wavg_ln(
        m, x, info["size"], norm, addend, log_size=info["prop_attn"]),
    (_ln.AMP_FUNCTION, True): lambda m, x, info, norm, addend, fold: tm.drop_ln(m, x, norm, addend),
}


def _launched(kind, plan, out, info, fold):
    """What follows a fused launch in either layout: the sizes (ones behind a drop), the folded bias, the message."""
    x, y = out[0], out[1]
    info["size"] = torch.ones((plan.n, plan.T - plan.r, 1), device=x.device) if kind == "drop" else out[2]
    if fold is not None:
        info["_folded"] = (x, fold)
    if info["verbose"]:
        print(f"{'Dropped' if kind == 'drop' else 'Merged'} {plan.T} to {plan.T - plan.r} tokens")
    return x, y


def merge_then_norm(metric, x, info, norm, reduction_function, plain_merge_fn, residual=None, fold=None, drop_fn=None,
                    hybrid_fn=None):
    """The block steps `[x = x + residual;] x = reduction_function(metric, x, info); y = norm(x)` with the
    residual add and the LayerNorm fused into the reduction kernel where fused_route names a launch: tome_merge_wavg_ln
    for the model's plain merge function (`plain_merge_fn`; modes 'merge' and 'random_merge') and its hybrid one
    (`hybrid_fn`), tome_drop_ln for its drop function (`drop_fn`; 'drop', 'random_drop'); returns (x, y).
    Anything else runs the steps as the reference does.
    fold: the Linear that finishes the block (`foldable`); when the 16-bit launch runs in plain 'merge' mode (_fold_for), x
    comes back with that bias added (y is the norm of x without it) and info["_folded"] says so for finish_linear.  The
    Functions and the mixed-precision launch ignore it: their stream is the one the three steps store.  Both Functions
    read the residual themselves."""
    kind = fused_kind(info["mode"], reduction_function is plain_merge_fn,
                      drop_fn is not None and reduction_function is drop_fn,
                      hybrid_fn is not None and reduction_function is hybrid_fn)
    how = fused_route(kind, x, norm, residual, info)
    if residual is not None and how != "function" and how != _ln.AMP_FUNCTION:
        # the launch reads the residual as its addend; the 16-bit one only an addend of x's dtype, without source tracking
        # and with a clamped r > 0.  Else the framework adds first, and the sum -- another tensor -- is asked again
        as_addend = how is not None and _FUSE_ADD and (how != "direct" or (
            not info["trace_source"] and residual.dtype == x.dtype
            and _abi.effective_r(x.shape[1], info["r"][0], info["class_token"], info["distill_token"]) > 0))
        if not as_addend:
            x, residual = x + residual, None
            how = how and fused_route(kind, x, norm, None, info)
    if how is None:
        x = reduction_function(metric, x, info)
        return x, _trailing_norm(x, norm)
    r = info["r"].pop(0)
    reduce = matching(kind, metric, r, info)
    if reduce is None:  # clamped r == 0: the unfused steps around a reduction that does nothing
        if residual is not None:
            x = x + residual
        if kind == "drop":
            x = _apply_drop(do_nothing, x, info)
        elif info["mode"] != "merge":  # (plain 'merge' leaves size and source alone here, as it always has)
            x = _apply_merge(do_nothing, x, info)
        return x, norm(x)
    if info["trace_source"]:  # (the 16-bit launch alone gets here with it)
        info["source"] = (_drop_source(reduce, info["source"], x.shape[0], x.shape[1], x.device) if kind == "drop"
                          else merge_source(reduce, x, info["source"]))
    fold = _fold_for(fold, x, info["mode"]) if how == "direct" else None
    out = _LAUNCH[how, kind == "drop"](reduce, x, info, norm, residual, fold)
    return _launched(kind, reduce.plan, out, info, fold)


def _regrouped_by_views(reduce_grouped, metric, x_full, info, r, frames):
    """The reference's own sequence around a grouped reduction (timesformer.py:89-107, motionformer.py:150-168): split
    the class token off, '(p t) -> (b t) p', reduce, back, cat.  Differentiable framework ops end to end: the form the
    regrouped reductions take when the tokens require grad (training, tools/train_net.py:727-741)."""
    B, N, C = x_full.shape
    P = (N - 1) // frames
    body = x_full[:, 1:].reshape(B, P, frames, C).transpose(1, 2).reshape(B * frames, P, C)
    body = reduce_grouped(metric, body, info, r)
    P2 = body.shape[1]
    body = body.reshape(B, frames, P2, C).transpose(1, 2).reshape(B, P2 * frames, C)
    return torch.cat((x_full[:, :1], body), dim=1)


def _native_regrouped(kind: str, x_full, size=None) -> bool:
    """Tokens that require grad: does the regrouped reduction run as a native Function (tome/merge.py: the regrouped
    kernel forward, tome_merge_backward_regrouped backward) instead of `_regrouped_by_views`?  Plain merge and drop
    on 16-byte rows; the matching of these models has no distillation token and, here, no threshold."""
    return (tm.native_backward_covers(kind, even_odd=True, on_device=x_full.is_cuda and x_full.dim() == 3,
                                      dtype=x_full.dtype,
                                      size_requires_grad=size is not None and _abi.needs_grad(size))
            and (x_full.shape[-1] * x_full.element_size()) % 16 == 0)


def reduce_merge_regrouped(metric, x_full, info, r, frames, hybrid=False):
    """reduce_merge / reduce_hybrid for the models whose merge groups are interleaved in the token sequence
    (TimeSformer '(p t)', Motionformer '(s f)'): x_full is [B, 1 + P*F, C] with the class token in front; the
    kernel addresses the groups in place and returns [B, 1 + (P-r)*F, C] (no permuted copies of x)."""
    training = _abi.needs_grad(x_full)
    if training and (hybrid or info["trace_source"] or not _native_regrouped("merge_wavg", x_full, info["size"])):
        return _regrouped_by_views(reduce_hybrid if hybrid else reduce_merge, metric, x_full, info, r, frames)
    merge = matching("hybrid" if hybrid else "merge", metric, r, info)
    if merge is None:
        return x_full
    plan = merge.plan
    if info["trace_source"]:
        shape_only = x_full.new_empty((plan.n, plan.T, 0))
        info["source"] = merge_source(merge, shape_only, info["source"])
    x_out, info["size"] = merge_wavg_regrouped(plan, x_full, info["size"], frames, has_cls=True, log_size=info["prop_attn"])
    if info["verbose"]:
        print(f"Merged {plan.T} to {plan.T - plan.r} tokens")
    return x_out


class GroupedResidual:
    """TimeSformer's second residual as the spatial attention leaves it (tome/patch/timesformer.py:32-52): `rs`
    [(b t), 1 + p, m] with a class row per frame, and the class token averaged over the frames `cls_new` [b, 1, m].
    The reference rearranges it '(b t) p m -> b (p t) m' and concatenates; the fused merge kernel reads it where it
    lies (`addend_grouped`), anything else asks for `.materialize()`."""

    def __init__(self, rs: torch.Tensor, cls_new: torch.Tensor, B: int, T: int, P: int):
        self.rs, self.cls_new, self.B, self.T, self.P = rs, cls_new, B, T, P
        self.dtype = rs.dtype

    def materialize(self) -> torch.Tensor:
        B, T, P, m = self.B, self.T, self.P, self.rs.shape[-1]
        body = self.rs.reshape(B, T, 1 + P, m)[:, :, 1:, :].transpose(1, 2)  # '(b t) p -> b p t', still a view
        if torch.is_grad_enabled() and self.rs.requires_grad:
            return torch.cat((self.cls_new, body.reshape(B, P * T, m)), 1)
        res = torch.empty((B, 1 + P * T, m), dtype=self.rs.dtype, device=self.rs.device)
        res[:, :1, :] = self.cls_new  # assembled by one strided copy
        res[:, 1:, :].view(B, P, T, m).copy_(body)
        return res


def merge_then_norm_regrouped(metric, x_full, info, norm, unfused_reduce, is_plain_merge: bool, frames: int,
                              residual=None, fold=None, is_drop: bool = False, is_hybrid: bool = False):
    """merge_then_norm for the interleaved layouts (TimeSformer '(p t)', Motionformer '(s f)'): x_full is
    [B, 1 + P*F, C]; `unfused_reduce(x)` is the model's own reduction step (it pops r itself).  `residual`: a tensor
    in x's layout, or a GroupedResidual.  is_plain_merge / is_drop / is_hybrid: which of the model's reduction functions
    the block carries (fused_kind)."""
    r_list = info["r"]
    grouped = residual if isinstance(residual, GroupedResidual) else None
    kind = fused_kind(info["mode"], is_plain_merge, is_drop, is_hybrid)
    fusable = (_FUSE_LN and kind is not None and r_list and r_list[0] > 0
               and not info["trace_source"]
               and _abi.ln_fusable(x_full, norm, *((residual,) if grouped is None else (grouped.rs, grouped.cls_new)))
               and _abi.effective_r((x_full.shape[1] - 1) // frames, r_list[0], False, False) > 0)
    if grouped is not None and not (fusable and _FUSE_ADD and grouped.dtype == x_full.dtype):
        residual, grouped = grouped.materialize(), None
    if not fusable:
        if residual is not None:
            x_full = x_full + residual
        x_full = unfused_reduce(x_full)
        return x_full, _trailing_norm(x_full, norm)
    if grouped is None and residual is not None and (not _FUSE_ADD or residual.dtype != x_full.dtype):
        x_full = x_full + residual
        residual = None
    reduce = matching(kind, metric, r_list.pop(0), info)
    assert reduce is not None  # (the clamped r was asked up front)
    plan = reduce.plan
    fold = _fold_for(fold, x_full, info["mode"])
    where = dict(addend=residual) if grouped is None else dict(addend_grouped=grouped.rs, cls_addend=grouped.cls_new)
    ln, out_bias = (norm.weight, norm.bias, norm.eps), None if fold is None else fold.bias
    if kind == "drop":
        out = _abi.drop_regrouped(plan, x_full, frames, has_cls=True, ln=ln, out_bias=out_bias, **where)
    else:
        out = _abi.merge_wavg_regrouped(plan, x_full, info["size"], frames, has_cls=True, ln=ln,
                                        log_size=info["prop_attn"], out_bias=out_bias, **where)
    return _launched(kind, plan, out, info, fold)


def _drop_source(drop, source, n, t, device):
    """`drop(source)` with `source = eye(T)` when None (tome/patch/videomae.py:112-117); the first layer's matrix
    comes straight from the row map (tome_source_init), without the identity."""
    plan = getattr(drop, "plan", None)
    if source is None:
        if plan is not None:
            return _abi.source_init(plan, drop=True)
        source = torch.eye(t, device=device)[None, ...].expand(n, t, t)  # nothing to drop (r clamped to 0)
    return drop(source)


def reduce_drop(metric, x, info, r):
    return _apply_drop(matching("drop", metric, r, info) or do_nothing, x, info)


def _apply_drop(drop, x, info):
    """The steps behind the matching of reduce_drop: source tracking, the drop, sizes of one."""
    if info["trace_source"]:
        info["source"] = _drop_source(drop, info["source"], x.shape[0], x.shape[1], x.device)
    before = x.size(1)
    x = drop(x)
    info["size"] = torch.ones((x.size(0), x.size(1), 1), device=x.device)
    if info["verbose"]:
        print(f"Dropped {before} to {x.size(1)} tokens")
    return x


def reduce_drop_regrouped(metric, x_full, info, r, frames: int):
    """reduce_drop for the interleaved layouts: x_full [B, 1 + P*F, C] with the class token in front; the groups
    are addressed in place by the kernel (tome_drop_regrouped) instead of regrouped by permuted copies
    (timesformer.py:111-131, motionformer.py:172-193)."""
    training = _abi.needs_grad(x_full)
    if training and (info["trace_source"] or not _native_regrouped("drop", x_full)):
        return _regrouped_by_views(reduce_drop, metric, x_full, info, r, frames)
    drop = matching("drop", metric, r, info)
    if drop is None:
        return x_full
    plan = drop.plan
    if info["trace_source"]:
        info["source"] = _drop_source(drop, info["source"], plan.n, plan.T, x_full.device)
    x_out = drop_regrouped(plan, x_full, frames, has_cls=True)
    info["size"] = torch.ones((plan.n, plan.T - plan.r, 1), device=x_full.device)
    if info["verbose"]:
        print(f"Dropped {plan.T} to {plan.T - plan.r} tokens")
    return x_out


def reduce_hybrid(metric, x, info, r):
    return _apply_merge(matching("hybrid", metric, r, info) or do_nothing, x, info)
