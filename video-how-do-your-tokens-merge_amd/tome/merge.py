"""ToMe token merging for MI355X -- same functions and signatures as the reference's
``tome/merge.py``, with the arithmetic done by the hand-written gfx950 kernels behind the C ABI
of ``include/tome_hip.h`` (see ``_abi.py``).

Reference lines each function stands in for (sjpollard/video-how-do-your-tokens-merge):
  bipartite_soft_matching         tome/merge.py:17-102
  bipartite_soft_matching_drop    tome/merge.py:215-271
  bipartite_soft_matching_hybrid  tome/merge.py:274-352
  kth_bipartite_soft_matching     tome/merge.py:105-158
  random_bipartite_soft_matching  tome/merge.py:161-212
  merge_wavg                      tome/merge.py:355-369
  merge_source                    tome/merge.py:372-384
  do_nothing                      tome/merge.py:13-14

The returned ``merge`` / ``unmerge`` / ``drop`` are real closures over ``unm_idx``, ``src_idx``,
``dst_idx`` (int64 device tensors shaped [n,r,1] / [n,T1-r,1]) and ``r`` exactly like the reference's,
so code that introspects them keeps working; they also carry ``.plan`` for the fused paths.  The kth_ / random_
matchings (every source row merged into its best destination, the merged sequence is the destination set alone) are
closures over ``dst_idx`` [n,Na,1], ``r`` and ``k`` / ``a_idx``, ``b_idx``; their ``.plan`` is an ``_abi.PartitionPlan``.

Tensors must live on a HIP device: there is no CPU implementation in this package.

Autograd (only the index computation is ``no_grad`` in the reference, merge.py:49; tools/train_net.py:727-741
patches models for training).  When a tensor handed to ``merge`` / ``unmerge`` / ``drop`` / ``merge_wavg`` requires grad
(and grad mode is on) the call becomes a ``torch.autograd.Function`` of this module: its forward is the same inference
kernel on the detached tensor, its backward one launch of ``tome_merge_backward`` (``k_merge_rows_bwd``: the gather
``gx[t] = gy[row of t] / out_div * in_mul``, no atomics, same bits on every run) -- or ``tome_merge`` in mode sum for
``unmerge``, its adjoint.  Covered (``native_backward_covers``): the even/odd matchings without a threshold, modes
``sum`` / ``mean``, fp32 / bf16 / fp16 tokens on the device, a ``size`` that does not itself require grad, ``unmerge``
without a distillation token.  Everything else (other reduce modes, hybrid and kth_ / random_ partition matchings, a
differentiable ``size``, foreign callables) applies the index tensors with the framework's own differentiable gather /
scatter_reduce ops instead (``_merge_with_autograd`` below: the op sequence of merge.py:75-100), as does every case
when ``NATIVE_BACKWARD`` is switched off.  The Functions are once-differentiable: double backward raises.  The
matching itself always runs on the HIP kernels.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch

from . import _abi, _overlap


def do_nothing(x, mode=None):
    return x


class HeadMeanKeys:
    """The metric ``k.mean(1)`` kept as a promise: holds the per-head keys [n,H,T,64] (a view of the attention's
    qkv buffer) -- or [outer,inner,H,T,64] when the merge groups are interleaved inside a clip's sequence
    (Motionformer's ``'(b h) (s f) d -> (b f) h s d'``; group = outer*inner + inner index).  The matching functions
    of this module read the keys in place (tome_match_keys: head mean, unit vectors, similarity in one pass over
    them); anything else that wants the tensor calls ``.materialize()``.  Shape queries behave like the metric's."""

    def __init__(self, keys: torch.Tensor):
        if keys.dim() not in (4, 5):
            raise ValueError(f"HeadMeanKeys: [n,H,T,D] or [outer,inner,H,T,D] expected, got {tuple(keys.shape)}")
        self.keys = keys
        self.early = None  # (r, class_token, distill_token, plan) of a matching already issued (tome/_overlap.py)

    @property
    def shape(self):
        *lead, _, t, d = self.keys.shape
        n = lead[0] * (lead[1] if len(lead) == 2 else 1)
        return torch.Size((n, t, d))

    @property
    def device(self):
        return self.keys.device

    @property
    def dtype(self):
        return self.keys.dtype

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def materialize(self) -> torch.Tensor:
        m = self.keys.mean(-3)
        return m if m.dim() == 3 else m.reshape(-1, m.shape[-2], m.shape[-1])


def _scores_for_random(metric: torch.Tensor) -> torch.Tensor:
    """merge.py:54-57 / :239-242 -- the random variants replace the similarity by uniform noise drawn on
    the metric's device (torch's generator, exactly as the reference draws it)."""
    length = metric.size(1)
    len_a, len_b = (length + 1) // 2, length // 2
    return torch.rand(size=(metric.size(0), len_a, len_b), device=metric.device)


def _plan(metric, r, class_token, distill_token, random: bool, **want) -> Optional[_abi.MatchPlan]:
    with torch.no_grad():
        if isinstance(metric, HeadMeanKeys):
            found, plan = _overlap.take(metric, r, class_token, distill_token)
            if found and not random and not any(want.values()):
                return plan  # issued beside the block's attention, on the side stream this stream now waits for
            if not random and _abi.keys_fusable(metric.keys):
                return _abi.match_keys(metric.keys, r, class_token, distill_token, checked=True, **want)
            metric = metric.materialize()
        if random:
            _abi.require_device(metric, "bipartite_soft_matching(metric)")
            t = metric.shape[1]
            if _abi.effective_r(t, r, class_token, distill_token) <= 0:
                return None
            return _abi.match_scores(_scores_for_random(metric), t, r, class_token, distill_token, **want)
        return _abi.match(metric, r, class_token, distill_token, **want)


def bipartite_soft_matching(
    metric: torch.Tensor,
    r: int,
    class_token: bool = False,
    distill_token: bool = False,
    mode: str = "merge",
) -> Tuple[Callable, Callable]:
    """Balanced (even/odd) bipartite matching; input [batch, tokens, channels]; at most 50% of the
    unprotected tokens are merged.  Returns (merge, unmerge)."""
    if mode not in ("merge", "random_merge"):
        raise ValueError(f"bipartite_soft_matching: mode {mode!r} (expected 'merge' or 'random_merge')")
    plan = _plan(metric, r, class_token, distill_token, random=(mode == "random_merge"))
    if plan is None:
        return do_nothing, do_nothing
    return _make_merge_pair(plan)


def _wants_autograd(x: torch.Tensor) -> bool:
    return torch.is_grad_enabled() and x.requires_grad


# Tokens that require grad take the native Functions below where `native_backward_covers` says so.  False: every such
# call takes the framework's gather / scatter_reduce chain (the behaviour before the backward kernel existed) -- for
# A/B in tests and tools/merge_backward_bench.py.
NATIVE_BACKWARD = True

_NATIVE_MODES = {"merge": ("sum", "mean"), "merge_wavg": (None,), "drop": (None,), "unmerge": (None,)}


def native_backward_covers(kind: str, *, even_odd: bool, hybrid: bool = False, distill_token: bool = False,
                           on_device: bool = True, dtype=torch.float32, mode: Optional[str] = None,
                           size_requires_grad: bool = False, enabled: Optional[bool] = None) -> bool:
    """Does a call of `kind` ("merge", "merge_wavg", "drop", "unmerge") on tokens that require grad run as a native
    Function (forward kernel + tome_merge_backward)?  Facts only, no tensors: testable without a device."""
    if kind not in _NATIVE_MODES:
        raise ValueError(f"native_backward_covers: unknown kind {kind!r}")
    if not (NATIVE_BACKWARD if enabled is None else enabled):
        return False
    if not even_odd or hybrid or not on_device or dtype not in _abi.DTYPES:
        return False  # kth_ / random_ partition plans, threshold flags, CPU tensors, fp64
    if mode not in _NATIVE_MODES[kind]:
        return False  # "max" (source tracking) and the other reduce modes are never differentiated
    if kind == "merge_wavg" and size_requires_grad:
        return False
    if kind == "unmerge" and distill_token:
        return False  # unmerge reads [unmerged, destinations] whatever merge wrote: not the adjoint of merge there
    return True


def _covers(kind: str, plan, x: torch.Tensor, mode: Optional[str] = None, size: Optional[torch.Tensor] = None) -> bool:
    return native_backward_covers(
        kind, even_odd=isinstance(plan, _abi.MatchPlan), hybrid=getattr(plan, "edge_keep", None) is not None,
        distill_token=bool(getattr(plan, "distill_token", False)),
        on_device=x.is_cuda and x.device == getattr(plan, "device", None) and x.dim() == 3, dtype=x.dtype, mode=mode,
        size_requires_grad=size is not None and _wants_autograd(size))


def _grad_like(ctx, g: torch.Tensor) -> torch.Tensor:
    return g if g.dtype == ctx.dtype else g.to(ctx.dtype)


class _MergeFunction(torch.autograd.Function):
    """merge(x, "sum" | "mean"): tome_merge forward, tome_merge_backward backward."""

    @staticmethod
    def forward(ctx, x, plan, mode):
        ctx.plan, ctx.dtype = plan, x.dtype
        ctx.count = _abi.plan_count(plan) if mode == "mean" else None
        _abi.plan_row_map(plan)
        return _abi.merge(plan, x.detach(), mode)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _abi.merge_backward(ctx.plan, _grad_like(ctx, g), out_div=ctx.count), None, None


class _DropFunction(torch.autograd.Function):
    """drop(x): tome_drop forward; backward = the gather with zero rows for the tokens that were dropped."""

    @staticmethod
    def forward(ctx, x, plan):
        ctx.plan, ctx.dtype = plan, x.dtype
        _abi.plan_row_map(plan)
        return _abi.drop(plan, x.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _abi.merge_backward(ctx.plan, _grad_like(ctx, g), drop=True), None


class _UnmergeFunction(torch.autograd.Function):
    """unmerge(x): tome_unmerge forward; backward = merge(g, "sum"), its adjoint (own term, then the sources in rank
    order: deterministic)."""

    @staticmethod
    def forward(ctx, x, plan):
        ctx.plan, ctx.dtype = plan, x.dtype
        return _abi.unmerge(plan, x.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        g = _grad_like(ctx, g)
        plan = ctx.plan
        if g.dim() != 3 or g.shape[0] != plan.n or g.shape[1] != plan.T or g.device != plan.device:
            raise _abi.TomeHipError(f"unmerge backward: expected a gradient [{plan.n}, {plan.T}, C] on {plan.device}, "
                                    f"got {tuple(g.shape)} on {g.device}")
        return _abi.merge(plan, g.detach(), "sum"), None


class _MergeWavgFunction(torch.autograd.Function):
    """merge_wavg(merge, x, size): tome_merge_wavg forward (sizes and their log are side outputs without a
    gradient), backward gx[t] = g[row of t] / size'[row of t] * size[t]."""

    @staticmethod
    def forward(ctx, x, size, plan, log_size):
        ctx.plan, ctx.dtype = plan, x.dtype
        _abi.plan_row_map(plan)
        x_out, s_out = _abi.merge_wavg(plan, x.detach(), None if size is None else size.detach(), log_size=log_size)
        log = getattr(s_out, "_tome_log", None)
        ctx.save_for_backward(size, s_out)
        ctx.mark_non_differentiable(*(t for t in (s_out, log) if t is not None))
        return x_out, s_out, log

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _gs, _gl):
        size, s_out = ctx.saved_tensors
        return _abi.merge_backward(ctx.plan, _grad_like(ctx, g), out_div=s_out, in_mul=size), None, None, None


class _MergeWavgRegroupedFunction(torch.autograd.Function):
    """_abi.merge_wavg_regrouped (TimeSformer / Motionformer layout) with tome_merge_backward_regrouped behind it."""

    @staticmethod
    def forward(ctx, x_full, size, plan, frames, has_cls, log_size):
        ctx.plan, ctx.dtype, ctx.frames, ctx.has_cls = plan, x_full.dtype, frames, has_cls
        _abi.plan_row_map(plan)
        x_out, s_out = _abi.merge_wavg_regrouped(plan, x_full.detach(), None if size is None else size.detach(), frames,
                                                 has_cls=has_cls, log_size=log_size)
        log = getattr(s_out, "_tome_log", None)
        ctx.save_for_backward(size, s_out)
        ctx.mark_non_differentiable(*(t for t in (s_out, log) if t is not None))
        return x_out, s_out, log

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _gs, _gl):
        size, s_out = ctx.saved_tensors
        gx = _abi.merge_backward_regrouped(ctx.plan, _grad_like(ctx, g), ctx.frames, has_cls=ctx.has_cls, out_div=s_out,
                                           in_mul=size)
        return gx, None, None, None, None, None


class _DropRegroupedFunction(torch.autograd.Function):
    """_abi.drop_regrouped with tome_merge_backward_regrouped (drop) behind it."""

    @staticmethod
    def forward(ctx, x_full, plan, frames, has_cls):
        ctx.plan, ctx.dtype, ctx.frames, ctx.has_cls = plan, x_full.dtype, frames, has_cls
        _abi.plan_row_map(plan)
        return _abi.drop_regrouped(plan, x_full.detach(), frames, has_cls=has_cls)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        gx = _abi.merge_backward_regrouped(ctx.plan, _grad_like(ctx, g), ctx.frames, has_cls=ctx.has_cls, drop=True)
        return gx, None, None, None


def _with_log(s_out: torch.Tensor, log: Optional[torch.Tensor]) -> torch.Tensor:
    # the size a Function returns is a new tensor object: log(size') travels on it again (`_abi.log_of_size`)
    if log is not None:
        s_out._tome_log = log
    return s_out


def merge_wavg_native(plan, x, size, log_size: bool = False):
    x_out, s_out, log = _MergeWavgFunction.apply(x, size, plan, bool(log_size))
    return x_out, _with_log(s_out, log)


def merge_wavg_regrouped_native(plan, x_full, size, frames: int, has_cls: bool = True, log_size: bool = False):
    """`_abi.merge_wavg_regrouped(plan, x_full, size, frames)` for tokens that require grad."""
    x_out, s_out, log = _MergeWavgRegroupedFunction.apply(x_full, size, plan, int(frames), bool(has_cls), bool(log_size))
    return x_out, _with_log(s_out, log)


def drop_regrouped_native(plan, x_full, frames: int, has_cls: bool = True):
    """`_abi.drop_regrouped(plan, x_full, frames)` for tokens that require grad."""
    return _DropRegroupedFunction.apply(x_full, plan, int(frames), bool(has_cls))


def merge_wavg_regrouped(plan, x_full, size, frames: int, has_cls: bool = True, log_size: bool = False):
    """`_abi.merge_wavg_regrouped`, as the Function above when the tokens want a gradient."""
    run = merge_wavg_regrouped_native if _wants_autograd(x_full) else _abi.merge_wavg_regrouped
    return run(plan, x_full, size, frames, has_cls=has_cls, log_size=log_size)


def drop_regrouped(plan, x_full, frames: int, has_cls: bool = True):
    """The same for `_abi.drop_regrouped`."""
    return (drop_regrouped_native if _wants_autograd(x_full) else _abi.drop_regrouped)(plan, x_full, frames, has_cls=has_cls)


_SCATTER_MODE = {"sum": "sum", "mean": "mean", "prod": "prod", "max": "amax", "amax": "amax", "min": "amin", "amin": "amin"}


def _interleave_distill(first: torch.Tensor, second: torch.Tensor) -> torch.Tensor:
    # merge.py:82-83: with a distillation token the class token of `first` and the distill token of `second` lead
    return torch.cat([first[:, :1], second[:, :1], first[:, 1:], second[:, 1:]], dim=1)


def _merge_with_autograd(plan, x: torch.Tensor, mode: str, keep_sources: bool = True) -> torch.Tensor:
    """The merge (keep_sources) or drop callback on differentiable framework ops: even tokens gathered by
    ``unm_idx``, sources scattered onto their odd destinations with ``scatter_reduce(include_self=True)``
    (merge.py:75-85, :257-266), a hybrid matching's threshold flags first (merge.py:326)."""
    if mode not in _SCATTER_MODE:
        raise _abi.TomeHipError(f"merge: unknown reduce mode {mode!r}")
    n, t, c = x.shape
    if n != plan.n or t != plan.T:
        raise _abi.TomeHipError(f"merge(x): expected [{plan.n}, {plan.T}, C], got {tuple(x.shape)}")
    a_rows, b_rows = x[:, 0::2], x[:, 1::2]
    r, t1 = plan.r, a_rows.shape[1]
    kept = a_rows.gather(1, plan.unm_idx.expand(n, t1 - r, c))
    if keep_sources:
        where = plan.dst_idx.expand(n, r, c)
        if plan.edge_keep is not None:
            flags = plan.edge_keep.reshape(n, r, 1).to(x.dtype).expand(n, r, c)
            b_rows = b_rows.scatter_reduce(1, where, flags, reduce="prod")
        b_rows = b_rows.scatter_reduce(1, where, a_rows.gather(1, plan.src_idx.expand(n, r, c)),
                                       reduce=_SCATTER_MODE[mode])
    if plan.distill_token:
        return _interleave_distill(kept, b_rows)
    return torch.cat([kept, b_rows], dim=1)


def _unmerge_with_autograd(plan, x: torch.Tensor) -> torch.Tensor:
    """merge.py:87-100 on differentiable ops: odd slots take the destination rows, even slots their unmerged row or a
    copy of the destination they were merged into."""
    n, _, c = x.shape
    r, t1 = plan.r, (plan.T + 1) // 2
    u = t1 - r
    kept, b_rows = x[:, :u], x[:, u:]
    copies = b_rows.gather(1, plan.dst_idx.expand(n, r, c))
    a_rows = x.new_zeros((n, t1, c)).scatter(1, plan.unm_idx.expand(n, u, c), kept)
    a_rows = a_rows.scatter(1, plan.src_idx.expand(n, r, c), copies)
    return torch.stack([a_rows[:, :b_rows.shape[1]], b_rows], dim=2).flatten(1, 2) if t1 == b_rows.shape[1] \
        else torch.cat([torch.stack([a_rows[:, :-1], b_rows], dim=2).flatten(1, 2), a_rows[:, -1:]], dim=1)


def _make_merge_pair(plan: _abi.MatchPlan) -> Tuple[Callable, Callable]:
    unm_idx, src_idx, dst_idx = plan.unm_idx, plan.src_idx, plan.dst_idx
    r, distill_token = plan.r, plan.distill_token

    def merge(x: torch.Tensor, mode="mean") -> torch.Tensor:
        # the index tensors are closure variables on purpose (same names as the reference's closure, so
        # `merge.__closure__` introspection keeps working); the kernels read them through `plan`
        _closure = (unm_idx, src_idx, dst_idx, r, distill_token)  # noqa: F841
        if _wants_autograd(x):
            if _covers("merge", plan, x, mode=mode):
                return _MergeFunction.apply(x, plan, mode)
            return _merge_with_autograd(plan, x, mode)
        return _abi.merge(plan, x, mode)

    def unmerge(x: torch.Tensor) -> torch.Tensor:
        _closure = (unm_idx, src_idx, dst_idx, r)  # noqa: F841
        if _wants_autograd(x):
            # (also with a distillation token: the reference's unmerge, merge.py:87-100, reads `x` as
            # [unmerged, destinations] whatever the layout `merge` wrote, and so does the kernel)
            if _covers("unmerge", plan, x):
                return _UnmergeFunction.apply(x, plan)
            return _unmerge_with_autograd(plan, x)
        return _abi.unmerge(plan, x)

    merge.plan = plan
    unmerge.plan = plan
    return merge, unmerge


def bipartite_soft_matching_drop(
    metric: torch.Tensor,
    r: int,
    class_token: bool = False,
    distill_token: bool = False,
    mode: str = "drop",
):
    """Same matching, but the selected tokens are discarded instead of merged.  Returns ``drop``
    (a single callable) -- or the (do_nothing, do_nothing) pair when r <= 0, as the reference does."""
    if mode not in ("drop", "random_drop"):
        raise ValueError(f"bipartite_soft_matching_drop: mode {mode!r}")
    plan = _plan(metric, r, class_token, distill_token, random=(mode == "random_drop"))
    if plan is None:
        return do_nothing, do_nothing
    und_idx, src_idx = plan.unm_idx, plan.src_idx
    r, distill_token = plan.r, plan.distill_token

    def drop(x: torch.Tensor) -> torch.Tensor:
        _closure = (und_idx, src_idx, r, distill_token)  # noqa: F841  (closure variables as in the reference)
        if _wants_autograd(x):
            if _covers("drop", plan, x):
                return _DropFunction.apply(x, plan)
            return _merge_with_autograd(plan, x, "sum", keep_sources=False)
        return _abi.drop(plan, x)

    drop.plan = plan
    return drop


def bipartite_soft_matching_hybrid(
    metric: torch.Tensor,
    r: int,
    class_token: bool = False,
    distill_token: bool = False,
    mode: str = "merge",
    threshold: float = 0.0,
) -> Tuple[Callable, Callable]:
    """Merge, but a destination whose incoming edge scores below ``threshold`` loses its own
    contribution first (merge.py:326)."""
    if mode not in ("merge", "hybrid", "random_merge"):
        raise ValueError(f"bipartite_soft_matching_hybrid: mode {mode!r}")
    plan = _plan(metric, r, class_token, distill_token, random=(mode == "random_merge"), want_node_max=True)
    if plan is None:
        return do_nothing, do_nothing
    with torch.no_grad():
        plan.edge_keep = _abi.edge_keep(plan, threshold)
    merge, unmerge = _make_merge_pair(plan)
    return merge, unmerge


def _partition_split(plan, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's `split(x)` on framework ops: the rows of the source set and of the destination set
    (merge.py:119-126 for the kth rule, :179-183 for index lists)."""
    n, t, c = x.shape
    if n != plan.n or t != plan.T:
        raise _abi.TomeHipError(f"merge(x): expected [{plan.n}, {plan.T}, C], got {tuple(x.shape)}")
    if plan.k:
        k = plan.k
        groups = x[:, :(t // k) * k].reshape(n, -1, k, c)
        return groups[:, :, :k - 1].reshape(n, -1, c), groups[:, :, k - 1]
    return x.gather(1, plan.a_idx.expand(n, plan.Na, c)), x.gather(1, plan.b_idx.expand(n, plan.Nb, c))


def _partition_merge_with_autograd(plan, x: torch.Tensor, mode: str) -> torch.Tensor:
    """merge.py:137-142 / :198-203 on differentiable ops: every source row scattered onto its destination."""
    if mode not in _SCATTER_MODE:
        raise _abi.TomeHipError(f"merge: unknown reduce mode {mode!r}")
    src, dst = _partition_split(plan, x)
    n, _, c = src.shape
    return dst.scatter_reduce(1, plan.dst_idx.expand(n, plan.Na, c), src, reduce=_SCATTER_MODE[mode])


def _partition_unmerge_with_autograd(plan, x: torch.Tensor) -> torch.Tensor:
    """merge.py:144-156 / :205-210 on differentiable ops."""
    n, nb, c = x.shape
    if n != plan.n or nb != plan.Nb:
        raise _abi.TomeHipError(f"unmerge(x): expected [{plan.n}, {plan.Nb}, C], got {tuple(x.shape)}")
    src = x.gather(1, plan.dst_idx.expand(n, plan.Na, c))
    if plan.k:
        return torch.cat([src.reshape(n, -1, plan.k - 1, c), x.reshape(n, -1, 1, c)], dim=2).reshape(n, -1, c)
    out = x.new_zeros((n, plan.T, c)).scatter(1, plan.a_idx.expand(n, plan.Na, c), src)
    return out.scatter(1, plan.b_idx.expand(n, plan.Nb, c), x)


def _partition_metric(metric, who: str) -> torch.Tensor:
    if isinstance(metric, HeadMeanKeys):
        metric = metric.materialize()
    _abi.require_device(metric, f"{who}(metric)")
    if metric.dim() != 3:
        raise _abi.TomeHipError(f"metric must be [batch, tokens, channels], got {tuple(metric.shape)}")
    return metric


def kth_bipartite_soft_matching(metric: torch.Tensor, k: int) -> Tuple[Callable, Callable]:
    """The two sets as (every k-th token = destination, the k-1 before it = sources); T // k tokens remain and the
    tokens past (T // k) * k are discarded, as in the reference (merge.py:105-158).  Returns (merge, unmerge)."""
    if k <= 1:
        return do_nothing, do_nothing
    t = metric.shape[1]
    if k > t:
        raise ValueError(f"kth_bipartite_soft_matching: k={k} leaves no destination among {t} tokens")
    with torch.no_grad():
        plan = _abi.match_partition(_partition_metric(metric, "kth_bipartite_soft_matching"), k=int(k))
    dst_idx, r, k = plan.dst_idx, plan.Na, plan.k

    def merge(x: torch.Tensor, mode="mean") -> torch.Tensor:
        _closure = (dst_idx, r, k)  # noqa: F841  (closure variables as in the reference; the kernels read `plan`)
        if _wants_autograd(x):
            return _partition_merge_with_autograd(plan, x, mode)
        return _abi.merge_partition(plan, x, mode)

    def unmerge(x: torch.Tensor) -> torch.Tensor:
        _closure = (dst_idx, r, k)  # noqa: F841
        if _wants_autograd(x):
            return _partition_unmerge_with_autograd(plan, x)
        return _abi.unmerge_partition(plan, x)

    merge.plan = plan
    unmerge.plan = plan
    return merge, unmerge


def random_bipartite_soft_matching(metric: torch.Tensor, r: int) -> Tuple[Callable, Callable]:
    """The two sets as (r tokens chosen at random = sources, the rest = destinations); T - r tokens remain
    (merge.py:161-212).  The permutation is drawn with torch's generator on the metric's device, exactly as the
    reference draws it (merge.py:174), so `torch.manual_seed` makes a call repeatable.  Returns (merge, unmerge)."""
    if r <= 0:
        return do_nothing, do_nothing
    B, N, _ = metric.shape
    if r >= N:
        raise ValueError(f"random_bipartite_soft_matching: r={r} leaves no destination among {N} tokens")
    with torch.no_grad():
        metric = _partition_metric(metric, "random_bipartite_soft_matching")
        rand_idx = torch.rand(B, N, 1, device=metric.device).argsort(dim=1)
        a_idx = rand_idx[:, :r, :].contiguous()
        b_idx = rand_idx[:, r:, :].contiguous()
        plan = _abi.match_partition(metric, a_idx=a_idx, b_idx=b_idx)
    dst_idx = plan.dst_idx

    def merge(x: torch.Tensor, mode="mean") -> torch.Tensor:
        _closure = (a_idx, b_idx, dst_idx, r, B, N)  # noqa: F841  (closure variables as in the reference)
        if _wants_autograd(x):
            return _partition_merge_with_autograd(plan, x, mode)
        return _abi.merge_partition(plan, x, mode)

    def unmerge(x: torch.Tensor) -> torch.Tensor:
        _closure = (a_idx, b_idx, dst_idx, r, B, N)  # noqa: F841
        if _wants_autograd(x):
            return _partition_unmerge_with_autograd(plan, x)
        return _abi.unmerge_partition(plan, x)

    merge.plan = plan
    unmerge.plan = plan
    return merge, unmerge


def merge_wavg(merge: Callable, x: torch.Tensor, size: Optional[torch.Tensor] = None, log_size: bool = False
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Size-weighted average merge; returns the merged tensor and the new token sizes.  With a merge
    made by this package the whole ``x*size -> sum, sum -> x/size`` chain is one kernel launch.
    ``log_size=True`` (not in the reference's signature) makes that launch also emit ``log(size')`` for the
    next block's proportional-attention bias; consumers fetch it with ``_abi.log_of_size(size)``."""
    plan = getattr(merge, "plan", None)
    if plan is not None and not (_wants_autograd(x) or (size is not None and _wants_autograd(size))):
        if isinstance(plan, _abi.PartitionPlan):
            return _abi.merge_wavg_partition(plan, x, size, log_size=log_size)
        return _abi.merge_wavg(plan, x, size, log_size=log_size)
    if plan is not None and _covers("merge_wavg", plan, x, size=size) and _wants_autograd(x):
        return merge_wavg_native(plan, x, size, log_size=log_size)
    # foreign callables, do_nothing, and the tensors that require grad without being covered by the native Functions
    # (the closure's index tensors then run on the framework's differentiable ops): the reference's op sequence on
    # the tensors' own device
    if isinstance(plan, _abi.MatchPlan):
        closure = merge

        def merge(t, mode):
            return _merge_with_autograd(plan, t, mode) if _wants_autograd(t) else closure(t, mode=mode)
    if size is None:
        size = torch.ones_like(x[..., 0, None])
    x = merge(x * size, mode="sum")
    size = merge(size, mode="sum")
    x = x / size
    return x, size


def _ln_route(merge: Optional[Callable], x: torch.Tensor, norm, residual, size=None) -> Optional[str]:
    """How merge_wavg_ln / drop_ln below run: "direct" (the fused launch: no gradient wanted), "function" (the same
    launch as tome/_ln.py::_MergeLnFunction, tome_merge_ln_backward behind it), "amp_direct" (under autocast, tensors of
    the kind _abi._ln_amp_of describes and no gradient wanted: tome_merge_wavg_ln_amp / tome_drop_ln_amp, while
    tome._ln.NATIVE_LN_AUTOCAST is on), "amp_function" (under autocast with a gradient wanted of a participant other than
    the sizes, where _abi.merge_ln_amp_trainable holds: the same launches as tome/_ln.py::_MergeLnAmpFunction,
    tome_merge_ln_backward_amp behind them, while tome._ln.NATIVE_MERGE_LN_AUTOCAST_BACKWARD -- off by default --,
    NATIVE_LN_AUTOCAST and _ln.enabled() hold) or None: the three unfused steps.  Without autocast the answers are those
    of the first three alone.
    merge: the callable that carries the plan; None asks about the tensors alone, before the matching exists (the patched
    blocks: tome/patch/_common.py::fused_route).  The device is asked by each answer's own predicate in _abi."""
    from . import _ln
    if merge is not None:
        plan = getattr(merge, "plan", None)
        if not (isinstance(plan, _abi.MatchPlan) and x.device == plan.device):
            return None
    if not (x.dim() == 3 and isinstance(norm, torch.nn.LayerNorm)
            and (residual is None or (residual.shape == x.shape and residual.device == x.device))):
        return None
    same_dtype = residual is None or residual.dtype == x.dtype
    wanted = _abi.needs_grad(x, residual, size, norm.weight, norm.bias)
    if not wanted:
        if same_dtype and _abi.ln_fusable(x, norm, residual):
            return "direct"
        if (_ln.NATIVE_LN_AUTOCAST and _abi.autocast_dtype(x.device) is not None
                and _abi.ln_amp_fusable(x, norm, residual)):
            return _ln.AMP_DIRECT
        return None
    if size is not None and _wants_autograd(size):
        return None
    if (_ln.NATIVE_MERGE_LN_AUTOCAST_BACKWARD and _ln.NATIVE_LN_AUTOCAST and _ln.enabled()
            and _abi.autocast_dtype(x.device) is not None and _abi.merge_ln_amp_trainable(x, norm, residual, merge)):
        return _ln.AMP_FUNCTION
    if not same_dtype:
        return None
    return "function" if _ln.enabled() and _abi.merge_ln_trainable(x, norm, residual, merge) else None


def merge_wavg_ln(merge: Callable, x: torch.Tensor, size: Optional[torch.Tensor], norm,
                  residual: Optional[torch.Tensor] = None, log_size: bool = False
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``x = x + residual; x, size = merge_wavg(merge, x, size); y = norm(x)``: returns (x, y, size).  One launch
    (tome_merge_wavg_ln) for 16-bit device tokens, a matching of this package and an nn.LayerNorm over C <= 1024
    channels; when x, the residual or the norm requires grad, the same launch as an autograd Function whose backward
    is one launch too (tome_merge_ln_backward) where `_abi.merge_ln_trainable` holds.  Anything else -- a size that
    requires grad, a hybrid or partition matching, fp32 tokens, a LayerNorm subclass under grad, CPU tensors -- runs the
    three steps, so there always is an answer.  Under torch.autocast, with an fp32 LayerNorm, a 16-bit or fp32 x and no
    gradient wanted, the launch is tome_merge_wavg_ln_amp (`_ln_route`: "amp_direct"): y comes back in the autocast dtype,
    x and size are those of the three steps bit for bit; with a gradient wanted and
    tome._ln.NATIVE_MERGE_LN_AUTOCAST_BACKWARD on it is the same launch as a Function with tome_merge_ln_backward_amp
    behind it ("amp_function")."""
    from . import _ln
    how = _ln_route(merge, x, norm, residual, size)
    if how == "direct":
        return _abi.merge_wavg_ln(merge.plan, x, size, norm.weight, norm.bias, norm.eps, addend=residual,
                                  log_size=log_size)
    if how == _ln.AMP_DIRECT:
        return _abi.merge_wavg_ln_amp(merge.plan, x, size, norm.weight, norm.bias, norm.eps,
                                      _abi.autocast_dtype(x.device), addend=residual, log_size=log_size)
    if how == "function":
        return _ln.merge_ln_native(merge.plan, x, residual, size, norm, log_size=log_size)
    if how == _ln.AMP_FUNCTION:
        return _ln.merge_ln_amp_native(merge.plan, x, residual, size, norm, log_size=log_size)
    if residual is not None:
        x = x + residual
    x, size = merge_wavg(merge, x, size, log_size=log_size)
    return x, norm(x), size


def drop_ln(drop: Callable, x: torch.Tensor, norm, residual: Optional[torch.Tensor] = None
            ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``x = x + residual; x = drop(x); y = norm(x)`` for the callable of bipartite_soft_matching_drop: returns (x, y).
    Routed as merge_wavg_ln: tome_drop_ln, with tome_merge_ln_backward behind it under grad, tome_drop_ln_amp under
    autocast without grad ("amp_direct") and, behind tome._ln.NATIVE_MERGE_LN_AUTOCAST_BACKWARD, with
    tome_merge_ln_backward_amp behind it under grad ("amp_function"), else the three steps."""
    from . import _ln
    how = _ln_route(drop, x, norm, residual)
    if how == "direct":
        return _abi.drop_ln(drop.plan, x, norm.weight, norm.bias, norm.eps, addend=residual)
    if how == _ln.AMP_DIRECT:
        return _abi.drop_ln_amp(drop.plan, x, norm.weight, norm.bias, norm.eps, _abi.autocast_dtype(x.device),
                                addend=residual)
    if how == "function":
        return _ln.merge_ln_native(drop.plan, x, residual, None, norm, drop=True)[:2]
    if how == _ln.AMP_FUNCTION:
        return _ln.merge_ln_amp_native(drop.plan, x, residual, None, norm, drop=True)[:2]
    if residual is not None:
        x = x + residual
    x = drop(x)
    return x, norm(x)


def merge_source(merge: Callable, x: torch.Tensor, source: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Source tracking: adjacency between the initial tokens and the merged groups."""
    plan = getattr(merge, "plan", None)
    if source is None:
        if isinstance(plan, _abi.MatchPlan) and plan.edge_keep is None:
            # merging the identity with "max" = the one-hot rows of the matching's row map: written directly
            # (tome_source_init), the [n, T, T] identity is never allocated.  (Not for a hybrid matching: there a
            # destination with an incoming edge below the threshold is zeroed before the amax, merge.py:326-331, so its
            # own column is 0 -- the generic path below keeps that.  A partition matching, kth_ / random_, takes the
            # generic path with the identity as well: `merge(source, mode="max")`, rows of C = T channels.)
            _abi.require_device(x, "merge_source(x)")
            if x.shape[0] != plan.n or x.shape[1] != plan.T or x.device != plan.device:
                raise _abi.TomeHipError(f"merge_source: x {tuple(x.shape)} on {x.device} does not fit the matching "
                                        f"({plan.n} groups of {plan.T} tokens on {plan.device})")
            return _abi.source_init(plan)
        n, t, _ = x.shape
        source = torch.eye(t, device=x.device)[None, ...].expand(n, t, t)
    source = merge(source, mode="max")
    return source
