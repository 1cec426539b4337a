"""ctypes binding of the C ABI in include/tome_hip.h (lib/libtome_hip.so, gfx950 only).

There is no CPU path and no PyTorch fallback: if the shared library is missing or a tensor is not
on a HIP device, the call raises.  PyTorch is used for device memory and streams only.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("TOME_HIP_LIB", os.path.join(_PKG, "lib", "libtome_hip.so"))

i64, i32, vp, sz, f32 = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float
# The C ABI of include/tome_hip.h, name -> (restype, argtypes, later); tests/test_abi_cpu.py holds every row to the header's
# prototype.  later: the entry was added to ABI v11 after its first release -- a v11 library built before it still binds,
# and require_symbol says so when the entry is called.  Every other name must be exported.
SIGNATURES = {
    "tome_abi_version": (i32, [], False),
    "tome_last_error": (ctypes.c_char_p, [], False),
    "tome_effective_r": (i64, [i64, i64, i32, i32], False),
    "tome_match_workspace_bytes": (sz, [i64, i64, i64], False),
    "tome_match": (i32, [vp, i32, i64, i64, i64, i64, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp], False),
    "tome_match_keys": (i32, [vp, i32, i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, i32, i32, vp, vp, vp, vp, vp,
                             vp, sz, vp], False),
    "tome_match_scores": (i32, [vp, i64, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp], False),
    "tome_edge_keep": (i32, [vp, vp, i64, i64, i64, f32, vp, vp], False),
    "tome_merge_wavg": (i32, [vp, i32, vp, i32, i64, i64, i64, i64, vp, vp, vp, i32, vp, vp, vp, vp, vp], False),
    "tome_merge_wavg_ln": (i32, [vp, i32, vp, i32, i64, i64, i64, i64, vp, vp, vp, i32, vp, vp, vp, f32, vp, vp, vp, vp,
                                vp, vp, vp], False),
    "tome_merge_wavg_regrouped": (i32, [vp, i32, vp, i32, i64, i64, i64, i64, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp],
                                       False),
    "tome_merge_wavg_regrouped_ln": (i32, [vp, i32, vp, i32, i64, i64, i64, i64, i64, i32, vp, vp, vp, vp, vp, vp, f32,
                                          vp, i32, vp, vp, vp, vp, vp, vp, vp], False),
    "tome_add_layernorm": (i32, [vp, vp, i32, i64, i64, vp, vp, f32, vp, vp, vp], False),
    "tome_add_layernorm_skip_first": (i32, [vp, vp, i32, i64, i64, i64, vp, vp, f32, vp, vp, vp], False),
    "tome_add_layernorm_regrouped": (i32, [vp, vp, i32, i64, i64, i64, i64, vp, vp, f32, vp, vp, vp], False),
    "tome_prop_attention": (i32, [vp, vp, vp, i32, i64, i64, i64, i64, i64, vp, vp, vp, vp, i64, i32, f32, vp, vp, vp],
                                 False),
    "tome_prop_attention_segments": (i32, [vp, vp, vp, i32, i64, i64, i64, i64, i64, vp, vp, vp, vp, i64, f32, vp, vp,
                                          i64, vp, vp], False),
    "tome_trajectory_mix": (i32, [vp, vp, vp, i32, i64, i64, i64, i64, i64, i64, i64, f32, vp, i64, vp, vp], False),
    "tome_short_attention": (i32, [vp, vp, vp, i32, i64, i64, i64, i64, vp, vp, vp, f32, vp, vp], False),
    "tome_merge": (i32, [vp, i32, i64, i64, i64, i64, vp, vp, vp, i32, i32, vp, vp, vp], False),
    "tome_drop": (i32, [vp, i32, i64, i64, i64, i64, vp, i32, vp, vp], False),
    "tome_drop_regrouped": (i32, [vp, i32, i64, i64, i64, i64, i64, i32, vp, vp, vp], False),
    "tome_unmerge": (i32, [vp, i32, i64, i64, i64, i64, vp, vp, vp, vp, vp], False),
    "tome_merge_backward": (i32, [vp, i32, vp, vp, i32, i64, i64, i64, i64, vp, i32, i32, vp, vp], False),
    "tome_merge_backward_regrouped": (i32, [vp, i32, vp, vp, i32, i64, i64, i64, i64, i64, i32, vp, i32, vp, vp],
                                           False),
    "tome_row_map": (i32, [i64, i64, i64, i32, vp, vp, vp, vp, vp], False),
    "tome_source_init": (i32, [i64, i64, i64, i32, i32, vp, vp, vp], False),
    "tome_gelu_erf": (i32, [vp, i32, i64, vp, vp], False),
    "tome_tubelet_rows": (i32, [vp, i32, i64, i64, i64, i64, i64, vp, i64, i64, i64, vp, vp], False),
    "tome_partition_workspace_bytes": (sz, [i64, i64, i64, i64], False),
    "tome_match_partition": (i32, [vp, i32, i64, i64, i64, i64, i64, i64, vp, vp, i64, i64, vp, vp, vp, vp, sz, vp],
                                  False),
    "tome_merge_partition": (i32, [vp, i32, i64, i64, i64, i64, vp, vp, i64, i64, vp, vp, i32, vp, vp], False),
    "tome_merge_wavg_partition": (i32, [vp, i32, vp, i32, i64, i64, i64, i64, vp, vp, i64, i64, vp, vp, vp, vp, vp, vp],
                                       False),
    "tome_unmerge_partition": (i32, [vp, i32, i64, i64, i64, i64, vp, vp, i64, i64, vp, vp, vp], False),
    "tome_layernorm_backward_workspace_bytes": (sz, [i64, i64], True),
    "tome_layernorm_backward": (i32, [vp, vp, vp, i32, i64, i64, i32, i64, vp, f32, vp, vp, vp, vp, vp], True),
    "tome_prop_attention_backward_workspace_bytes": (sz, [i64, i64, i64, i64], True),
    "tome_prop_attention_backward": (i32, [vp, vp, vp, vp, vp, i32, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp,
                                          i64, i32, f32, vp, vp, vp, vp, vp, vp, vp, sz, vp], True),
    "tome_gelu_erf_backward_workspace_bytes": (sz, [i64, i64], True),
    "tome_gelu_erf_backward": (i32, [vp, vp, i32, i64, i64, vp, vp, vp, vp, sz, vp], True),
    "tome_short_attention_backward": (i32, [vp, vp, vp, vp, i32, i64, i64, i64, i64, vp, vp, vp, f32, vp, vp, vp, vp,
                                           vp, vp, vp], True),
    "tome_layernorm_backward_regrouped_workspace_bytes": (sz, [i64, i64, i64, i64], True),
    "tome_layernorm_backward_regrouped": (i32, [vp, vp, vp, i32, i64, i64, i64, i64, vp, f32, vp, vp, vp, vp, vp],
                                               True),
    "tome_prop_attention_segments_backward_workspace_bytes": (sz, [i64, i64, i64, i64, i64], True),
    "tome_prop_attention_segments_backward": (i32, [vp, vp, vp, vp, vp, i32, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp,
                                                   vp, i64, f32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp], True),
    "tome_trajectory_mix_backward": (i32, [vp, vp, vp, vp, i32, i64, i64, i64, i64, i64, i64, i64, i64, f32, vp, vp, vp,
                                          i64, i64, vp], True),
    "tome_gelu_tanh": (i32, [vp, i32, i64, vp, vp], True),
    "tome_gelu_tanh_backward": (i32, [vp, vp, i32, i64, i64, vp, vp, vp, vp, sz, vp], True),
    "tome_add_layernorm_amp": (i32, [vp, i32, vp, i32, i64, i64, i32, i64, vp, vp, f32, vp, vp, i32, vp], True),
    "tome_layernorm_backward_amp_workspace_bytes": (sz, [i64, i64, i32], True),
    "tome_layernorm_backward_amp": (i32, [vp, i32, vp, vp, i32, i64, i64, i32, i64, vp, f32, vp, vp, vp, vp, vp, vp],
                                         True),
    "tome_token_mean": (i32, [vp, i32, i64, i64, i64, i32, vp, vp], True),
    "tome_drop_ln": (i32, [vp, i32, i64, i64, i64, i64, vp, i32, vp, vp, f32, vp, vp, vp, vp, vp], True),
    "tome_drop_regrouped_ln": (i32, [vp, i32, i64, i64, i64, i64, i64, i32, vp, vp, vp, f32, vp, i32, vp, vp, vp, vp, vp],
                               True),
    "tome_merge_ln_backward_workspace_bytes": (sz, [i64, i64, i64], True),
    "tome_merge_ln_backward": (i32, [vp, vp, vp, i32, vp, vp, i32, i64, i64, i64, i64, vp, i32, i32, vp, f32, vp, vp, vp,
                                    vp, vp], True),
    "tome_merge_wavg_ln_amp": (i32, [vp, i32, vp, i32, vp, i32, i64, i64, i64, i64, vp, vp, vp, i32, vp, vp, vp, f32, vp,
                                    vp, i32, vp, vp, vp], True),
    "tome_drop_ln_amp": (i32, [vp, i32, vp, i32, i64, i64, i64, i64, vp, i32, vp, vp, f32, vp, vp, i32, vp], True),
    "tome_merge_ln_backward_amp_workspace_bytes": (sz, [i64, i64, i64, i32], True),
    "tome_merge_ln_backward_amp": (i32, [vp, i32, vp, vp, i32, vp, vp, i32, i64, i64, i64, i64, vp, i32, i32, vp, f32, vp,
                                        vp, vp, vp, vp, vp], True),
}
SYMBOLS = tuple(SIGNATURES)

ABI_VERSION = 11
DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
MODES = {"sum": 0, "mean": 1, "amax": 2, "max": 2, "prod": 3, "amin": 4, "min": 4}

_lib = None


class TomeHipError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """Load libtome_hip.so once; fail loudly when it is absent (build it with
    `python video-how-do-your-tokens-merge_amd/csrc/build.py`)."""
    global _lib
    if _lib is not None:
        return _lib
    _lib = bind(LIB_PATH)
    return _lib


def bind(path: str) -> ctypes.CDLL:
    """A library file with the C ABI of include/tome_hip.h, loaded and typed.  `lib()` binds the product library once;
    bench.py's stage-timing leg binds the measurement build beside it (lib/libtome_hip_prof.so)."""
    if not os.path.exists(path):
        raise TomeHipError(
            f"HIP extension not found at {path}: the MI355X merge path has no fallback. "
            "Build it with `python video-how-do-your-tokens-merge_amd/csrc/build.py` (needs hipcc).")
    L = ctypes.CDLL(path)
    for name, (restype, argtypes, later) in SIGNATURES.items():
        if later and not _exports(L, name):
            continue
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.tome_abi_version() != ABI_VERSION:
        raise TomeHipError(f"{os.path.basename(path)} ABI {L.tome_abi_version()} != expected {ABI_VERSION}")
    return L


def _exports(L, name: str) -> bool:
    try:
        getattr(L, name)
    except AttributeError:
        return False
    return True


def require_symbol(L, name: str):
    """`L.name`, or a TomeHipError that says the library predates the entry (ABI v11 grew by entries, not by number)."""
    if not _exports(L, name):
        raise TomeHipError(f"{name} is missing from the loaded library: it reports ABI {ABI_VERSION} but was built before "
                           "this entry was added; rebuild it with `python video-how-do-your-tokens-merge_amd/csrc/build.py`")
    return getattr(L, name)


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().tome_last_error().decode("utf-8", "replace")
        raise TomeHipError(f"{what} failed (status {rc}): {msg}")


def require_device(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise TomeHipError(
            f"{what}: tensor is on {t.device}; this build runs only on a HIP device (MI355X) and has no CPU path")


def dtype_code(t: torch.Tensor, what: str) -> int:
    try:
        return DTYPES[t.dtype]
    except KeyError:
        raise TomeHipError(f"{what}: dtype {t.dtype} not supported (float32, bfloat16, float16)") from None


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device) -> int:
    """The caller's current HIP stream on `device` as the raw handle the C ABI takes.  torch's own raw accessor (what
    its compiled-graph runtime calls per kernel) when it exists: `torch.cuda.current_stream(device).cuda_stream` builds
    a Stream object per call, 4-5 us of the ~20 us a wrapper of this module costs at the reference's batch of 8."""
    if _raw_stream is not None:
        idx = device.index
        return _raw_stream(torch.cuda.current_device() if idx is None else idx)
    return torch.cuda.current_stream(device).cuda_stream


class _on_device:
    """`with torch.cuda.device(dev)` without its cost when `dev` already is the current device (the
    common case: one process per GPU)."""

    __slots__ = ("idx", "prev")

    def __init__(self, device):
        self.idx = device.index

    def __enter__(self):
        self.prev = torch.cuda.current_device()
        if self.prev != self.idx:
            torch.cuda.set_device(self.idx)

    def __exit__(self, *exc):
        if self.prev != self.idx:
            torch.cuda.set_device(self.prev)
        return False


def _workspace(device, stream: int, nbytes: int) -> torch.Tensor:
    """Scratch of one matching, taken from PyTorch's caching allocator per call: the allocator hands a block back
    only to later work of the SAME stream (or, under graph capture, keeps it inside that graph's private pool),
    so the kernels still in flight when this tensor is released can never share it with another stream's or
    another graph's matching -- which a process-wide cache keyed by stream handle could not guarantee."""
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _sized_workspace(L, entry_name: str, dims, device, stream: int, what: str) -> torch.Tensor:
    """A workspace of the size `L.<entry_name>(*dims)` asks for; an entry that answers 0 has refused the shape."""
    nbytes = require_symbol(L, entry_name)(*dims)
    if nbytes == 0:
        raise TomeHipError(f"{what}: no workspace size for {tuple(dims)}")
    return _workspace(device, stream, nbytes)


def effective_r(T: int, r: int, class_token: bool, distill_token: bool) -> int:
    """merge.py:36-47 (same clamp as tome_effective_r; tests hold the two together)."""
    return max(0, min(int(r), (int(T) - int(bool(class_token)) - int(bool(distill_token))) // 2))


class MatchPlan:
    """Device-resident result of one matching: the reference's closure variables (int64,
    [n,r,1] / [n,T1-r,1]) plus what the fused kernels want (node_max for the hybrid threshold,
    row_map for source tracking)."""

    __slots__ = ("n", "T", "r", "class_token", "distill_token", "src_idx", "dst_idx", "unm_idx", "node_max",
                 "row_map", "edge_keep", "device", "count")

    def __init__(self, n, T, r, class_token, distill_token, src_idx, dst_idx, unm_idx, node_max, row_map, device):
        self.n, self.T, self.r = n, T, r
        self.class_token, self.distill_token = bool(class_token), bool(distill_token)
        self.src_idx, self.dst_idx, self.unm_idx = src_idx, dst_idx, unm_idx
        self.node_max, self.row_map = node_max, row_map
        self.edge_keep = None
        self.device = device
        self.count = None  # [n, T-r, 1] fp32, 1 + sources of every merged row (plan_count: backward of "mean")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _matching(L, entry, head, n, T, D, r, re, class_token, distill_token, device, want_node_max, want_row_map):
    """The tail of match / match_keys / match_scores behind their own checks: the workspace of a matching of n groups of T
    tokens (D channels), the buffers of its plan (re > 0 merged per group), and the call of `entry` of the library L --
    `head`: its arguments in front of r.  (One frame per matching, as the plan's allocation alone was: match_keys is on
    the host-bound forward.)"""
    T1 = (T + 1) // 2
    with _on_device(device):
        st = _stream(device)
        ws = _workspace(device, st, L.tome_match_workspace_bytes(n, T, D))
        src = torch.empty((n, re, 1), dtype=torch.int64, device=device)
        dst = torch.empty((n, re, 1), dtype=torch.int64, device=device)
        unm = torch.empty((n, T1 - re, 1), dtype=torch.int64, device=device)
        nmax = torch.empty((n, T1), dtype=torch.float32, device=device) if want_node_max else None
        rmap = torch.empty((n, T1), dtype=torch.int32, device=device) if want_row_map else None
        rc = entry(*head, int(r), int(bool(class_token)), int(bool(distill_token)), src.data_ptr(), dst.data_ptr(),
                   unm.data_ptr(), _ptr(nmax), _ptr(rmap), ws.data_ptr(), ws.numel(), st)
    _check(rc, entry.__name__)
    return MatchPlan(n, T, re, class_token, distill_token, src, dst, unm, nmax, rmap, device)


def match(metric: torch.Tensor, r: int, class_token=False, distill_token=False, want_node_max=False,
          want_row_map=False) -> Optional[MatchPlan]:
    """tome_match on `metric` [n,T,D]; returns None when the clamped r is <= 0."""
    require_device(metric, "bipartite_soft_matching(metric)")
    if metric.dim() != 3:
        raise TomeHipError(f"metric must be [batch, tokens, channels], got {tuple(metric.shape)}")
    code = dtype_code(metric, "metric")
    n, T, D = metric.shape
    re = effective_r(T, r, class_token, distill_token)
    if re <= 0 or n == 0:
        return None
    if metric.stride(2) != 1:
        metric = metric.contiguous()
    L = lib()
    return _matching(L, L.tome_match, (metric.data_ptr(), code, n, T, D, metric.stride(0), metric.stride(1)), n, T, D, r, re,
                     class_token, distill_token, metric.device, want_node_max, want_row_map)


def keys_fusable(keys: torch.Tensor) -> bool:
    """Can tome_match_keys read these per-head keys in place?  [n, H, T, 64], or [outer, inner, H, T, 64] when the
    groups are interleaved inside a clip (Motionformer's '(s f)' regrouping), any strides with contiguous channels
    and 16-byte aligned rows."""
    if keys.dim() not in (4, 5) or keys.shape[-1] != 64 or keys.stride(-1) != 1 or keys.dtype not in DTYPES \
            or not keys.is_cuda:
        return False
    es = keys.element_size()
    return keys.data_ptr() % 16 == 0 and all((keys.stride(d) * es) % 16 == 0 for d in range(keys.dim() - 1))


def match_keys(keys: torch.Tensor, r: int, class_token=False, distill_token=False, want_node_max=False,
               want_row_map=False, checked: bool = False) -> Optional[MatchPlan]:
    """tome_match_keys on per-head keys [n,H,T,64] or [outer,inner,H,T,64] (group = outer*inner + inner index;
    the metric = keys.mean(heads) is never materialised)."""
    if not checked and not keys_fusable(keys):
        require_device(keys, "match_keys(keys)")
        raise TomeHipError(f"match_keys: keys {tuple(keys.shape)} strides {keys.stride()} are not readable in place")
    if keys.dim() == 5:
        outer, inner, H, T, D = keys.shape
        n = outer * inner
        s_n, s_in, s_h, s_t = keys.stride()[:4]
    else:
        n, H, T, D = keys.shape
        inner, s_in = 1, 0
        s_n, s_h, s_t = keys.stride()[:3]
    re = effective_r(T, r, class_token, distill_token)
    if re <= 0 or n == 0:
        return None
    L = lib()
    return _matching(L, L.tome_match_keys, (keys.data_ptr(), DTYPES[keys.dtype], n, H, T, D, s_n, inner, s_in, s_h, s_t), n,
                     T, D, r, re, class_token, distill_token, keys.device, want_node_max, want_row_map)


def match_scores(scores: torch.Tensor, T: int, r: int, class_token=False, distill_token=False,
                 want_node_max=False, want_row_map=False) -> Optional[MatchPlan]:
    require_device(scores, "match_scores(scores)")
    n, T1, T2 = scores.shape
    if T1 != (T + 1) // 2 or T2 != T // 2:
        raise TomeHipError(f"scores shape {tuple(scores.shape)} does not fit T={T}")
    re = effective_r(T, r, class_token, distill_token)
    if re <= 0 or n == 0:
        return None
    scores = scores.float().contiguous()
    L = lib()
    return _matching(L, L.tome_match_scores, (scores.data_ptr(), n, T), n, T, 1, r, re, class_token, distill_token,
                     scores.device, want_node_max, want_row_map)


def edge_keep(plan: MatchPlan, threshold: float) -> torch.Tensor:
    if plan.node_max is None:
        raise TomeHipError("edge_keep needs a plan made with want_node_max=True")
    keep = torch.empty((plan.n, plan.r), dtype=torch.uint8, device=plan.device)
    with _on_device(plan.device):
        rc = lib().tome_edge_keep(plan.node_max.data_ptr(), plan.src_idx.data_ptr(), plan.n, plan.T, plan.r,
                                  float(threshold), keep.data_ptr(), _stream(plan.device))
    _check(rc, "tome_edge_keep")
    return keep


def _prep_x(plan, x: torch.Tensor, what: str, tokens: int) -> torch.Tensor:
    require_device(x, what)
    if x.dim() != 3 or x.shape[0] != plan.n or x.shape[1] != tokens:
        raise TomeHipError(f"{what}: expected [{plan.n}, {tokens}, C], got {tuple(x.shape)}")
    if x.device != plan.device:
        raise TomeHipError(f"{what}: tensor on {x.device}, matching was computed on {plan.device}")
    if torch.is_grad_enabled() and x.requires_grad:
        raise TomeHipError(f"{what}: autograd through the HIP merge kernels is not implemented (inference path); "
                           "call under torch.no_grad()")
    return x if x.is_contiguous() else x.contiguous()


def _log_size_like(s_out: torch.Tensor, want: bool) -> Optional[torch.Tensor]:
    """Buffer for log(size') -- the proportional-attention bias of the next block (`size.log()`,
    tome/patch/videomae.py:62-63).  It travels as the attribute `_tome_log` of the size tensor it belongs to, so
    a consumer that finds it (`log_of_size`) can never pair it with another size."""
    if not want:
        return None
    log = torch.empty_like(s_out)
    s_out._tome_log = log
    return log


def log_of_size(size: torch.Tensor) -> torch.Tensor:
    """`size.log()`; free when the merge kernel that produced `size` already emitted it."""
    log = getattr(size, "_tome_log", None)
    return log if log is not None else size.log()


def _prep_size(size: Optional[torch.Tensor], n: int, rows: int, x: torch.Tensor):
    """The token sizes as the weighted merges take them, and the dtype of the sizes they return: `size` [n, rows, 1] on
    x's device, contiguous, in x's dtype or fp32 (anything else is cast to x's) -- or None, which stands for ones of x's
    dtype (torch.ones_like(x[..., 0, None]), merge.py:362-363)."""
    if size is None:
        return None, x.dtype
    if size.device != x.device:  # (x is on a HIP device: every caller has asked require_device of it)
        raise TomeHipError(f"merge_wavg(size): tensor on {size.device}, tokens on {x.device}")
    if size.shape != (n, rows, 1):
        raise TomeHipError(f"size must be [{n}, {rows}, 1], got {tuple(size.shape)}")
    if size.dtype not in (x.dtype, torch.float32):
        size = size.to(x.dtype)
    size = size.contiguous()
    return size, size.dtype


def merge_wavg(plan: MatchPlan, x: torch.Tensor, size: Optional[torch.Tensor], log_size: bool = False):
    x = _prep_x(plan, x, "merge_wavg(x)", plan.T)
    n, T, C = x.shape
    xcode = dtype_code(x, "x")
    size, sdtype = _prep_size(size, n, T, x)
    scode = DTYPES[sdtype]
    x_out = torch.empty((n, T - plan.r, C), dtype=x.dtype, device=x.device)
    s_out = torch.empty((n, T - plan.r, 1), dtype=sdtype, device=x.device)
    log = _log_size_like(s_out, log_size)
    with _on_device(x.device):
        rc = lib().tome_merge_wavg(x.data_ptr(), xcode, _ptr(size), scode, n, T, C, plan.r, plan.src_idx.data_ptr(),
                                   plan.dst_idx.data_ptr(), plan.unm_idx.data_ptr(), int(plan.distill_token),
                                   _ptr(plan.edge_keep), x_out.data_ptr(), s_out.data_ptr(), _ptr(log),
                                   _stream(x.device))
    _check(rc, "tome_merge_wavg")
    return x_out, s_out


_HALF = (torch.bfloat16, torch.float16)


def needs_grad(*tensors) -> bool:
    """Is a gradient wanted of any of these tensors (None: an absent one)?  Asked of every differentiable tensor of an
    operation at once: by every `*_ok` / `ln_fusable` below and by the `route` functions of tome/_ln.py, _attn.py, _mlp.py.
    Those sit on the host-bound no-grad forward and test grad mode in front of the call: that spares the frame and the
    look-up of the arguments (`norm.weight` is a Python-level `__getattr__`)."""
    if torch.is_grad_enabled():
        for t in tensors:
            if t is not None and t.requires_grad:
                return True
    return False


def _ln_of(x: torch.Tensor, norm) -> bool:
    """The LayerNorm kind the kernels take, for a `norm` that is an nn.LayerNorm: affine with a bias, over the C <= 1024
    (C % 8 == 0) channels of 16-bit device tokens x, weight of x's dtype."""
    C = x.shape[-1]
    return (norm.elementwise_affine and norm.bias is not None and tuple(norm.normalized_shape) == (C,)
            and x.dtype in _HALF and norm.weight.dtype == x.dtype and C % 8 == 0 and C <= 1024 and x.is_cuda)


def ln_fusable(x: torch.Tensor, norm, *others) -> bool:
    """Can tome_merge_wavg_ln produce norm(x') for this LayerNorm module (a subclass included), no gradient wanted -- of
    x, of the norm's weight and bias, or of `others`, the residual or addend the launch reads beside x?"""
    return (isinstance(norm, torch.nn.LayerNorm) and _ln_of(x, norm)
            and not (torch.is_grad_enabled() and needs_grad(x, norm.weight, norm.bias, *others)))


def ln_trainable(x: torch.Tensor, norm) -> bool:
    """Can this LayerNorm of x run on the add + LayerNorm kernels (the regrouped one included) with
    tome_layernorm_backward[_regrouped] behind them (tome/_ln.py) when x or its parameters require grad?  The stock
    module only: a subclass may carry a forward of its own, which a training run must keep; and a bias of x's dtype."""
    return type(norm) is torch.nn.LayerNorm and _ln_of(x, norm) and norm.bias.dtype == x.dtype


def merge_ln_trainable(x: torch.Tensor, norm, addend: Optional[torch.Tensor], merge=None) -> bool:
    """Can `norm(merge_wavg(merge, x + addend))` (or the drop form) run as tome_merge_wavg_ln / tome_drop_ln with
    tome_merge_ln_backward behind it (tome/_ln.py::_MergeLnFunction) when a participant requires grad?  Device tokens,
    ln_trainable, an addend that is absent or of x's shape, dtype and device, and the even/odd matching of a MatchPlan
    without threshold flags (hybrid) -- a partition plan (kth_ / random_) has no row map of this kind.  merge: the
    callable that carries the plan; None asks about the tensors alone (before the matching exists)."""
    if not (x.is_cuda and x.dim() == 3 and ln_trainable(x, norm)
            and (addend is None or (addend.shape == x.shape and addend.dtype == x.dtype and addend.device == x.device))):
        return False
    if merge is None:
        return True
    plan = getattr(merge, "plan", None)
    return type(plan) is MatchPlan and plan.edge_keep is None and plan.r > 0 and plan.device == x.device


def autocast_dtype(device) -> Optional[torch.dtype]:
    """The 16-bit dtype autocast casts to on `device`, or None: autocast is off there, its dtype is not bf16 / fp16, or the
    device is not the kernels' kind.  The one place the patch layer asks about autocast (the reference trains and
    benchmarks under it: tools/train_net.py:123, tome/utils.py:54)."""
    if device.type != "cuda" or not torch.is_autocast_enabled("cuda"):
        return None
    dtype = torch.get_autocast_dtype("cuda")
    return dtype if dtype in _HALF else None


def _ln_amp_of(x: torch.Tensor, norm, addend: Optional[torch.Tensor] = None) -> bool:
    """The LayerNorm kind the mixed-precision kernels take under autocast, for a `norm` that is an nn.LayerNorm: fp32
    weight and bias (master weights) over the C <= 1024 (C % 8 == 0) channels of x, where x is the autocast dtype with an
    addend of the same (VideoMAE's stream, `pos_embed.type_as(x)`), or fp32 with an addend of the autocast dtype or fp32
    (`x + self.pos_embed` has promoted the stream).  False whenever autocast is off: nothing changes without it."""
    half = autocast_dtype(x.device)
    if half is None:
        return False
    C = x.shape[-1]
    if not (norm.elementwise_affine and norm.bias is not None and tuple(norm.normalized_shape) == (C,)
            and norm.weight.dtype == torch.float32 and norm.bias.dtype == torch.float32 and C % 8 == 0 and C <= 1024):
        return False
    if addend is not None and (addend.shape != x.shape or addend.device != x.device):
        return False
    if x.dtype == half:
        return addend is None or addend.dtype == half
    return x.dtype == torch.float32 and (addend is None or addend.dtype == half or addend.dtype == torch.float32)


def _out_bias(out_bias, x, C):
    if out_bias is None:
        return None
    if out_bias.numel() != C or out_bias.dtype != x.dtype or out_bias.device != x.device:
        raise TomeHipError(f"out_bias must hold {C} values of x's dtype on x's device")
    return out_bias.contiguous()


def _addend(who: str, addend: Optional[torch.Tensor], x: torch.Tensor, same_dtype: bool = True):
    """The addend a launch reads beside x, made contiguous (None: none): of x's shape and device -- and dtype, unless the
    entry converts (same_dtype=False: the mixed-precision ones)."""
    if addend is None:
        return None
    if addend.shape != x.shape or addend.device != x.device or (same_dtype and addend.dtype != x.dtype):
        raise TomeHipError(f"{who}: addend must match x in shape{', dtype' if same_dtype else ''} and device")
    return addend if addend.is_contiguous() else addend.contiguous()


def merge_wavg_ln(plan: MatchPlan, x: torch.Tensor, size: Optional[torch.Tensor], weight: torch.Tensor,
                  bias: torch.Tensor, eps: float, addend: Optional[torch.Tensor] = None, log_size: bool = False,
                  out_bias: Optional[torch.Tensor] = None):
    """merge_wavg + LayerNorm of the merged tokens in one launch: returns (x_out, y_out, size_out).  With
    `addend` the merged tokens are `x + addend` (the residual in front of the merge, added while loading).
    out_bias [C]: x_out is stored as x' + out_bias (y_out stays LayerNorm(x')) -- for a caller whose next GEMM
    accumulates onto x_out in place."""
    x = _prep_x(plan, x, "merge_wavg_ln(x)", plan.T)
    n, T, C = x.shape
    out_bias = _out_bias(out_bias, x, C)
    addend = _addend("merge_wavg_ln", addend, x)
    xcode = dtype_code(x, "x")
    size, sdtype = _prep_size(size, n, T, x)
    x_out = torch.empty((n, T - plan.r, C), dtype=x.dtype, device=x.device)
    y_out = torch.empty_like(x_out)
    s_out = torch.empty((n, T - plan.r, 1), dtype=sdtype, device=x.device)
    log = _log_size_like(s_out, log_size)
    with _on_device(x.device):
        rc = lib().tome_merge_wavg_ln(x.data_ptr(), xcode, _ptr(size), DTYPES[sdtype], n, T, C, plan.r,
                                      plan.src_idx.data_ptr(), plan.dst_idx.data_ptr(), plan.unm_idx.data_ptr(),
                                      int(plan.distill_token), _ptr(plan.edge_keep), weight.data_ptr(), bias.data_ptr(),
                                      float(eps), _ptr(addend), x_out.data_ptr(), y_out.data_ptr(), s_out.data_ptr(),
                                      _ptr(log), _ptr(out_bias), _stream(x.device))
    _check(rc, "tome_merge_wavg_ln")
    return x_out, y_out, s_out


def add_layernorm(x: torch.Tensor, addend: Optional[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor, eps: float,
                  skip_first: bool = False):
    """(x + addend, LayerNorm(x + addend)) in one launch, for 16-bit [..., C] tensors (C <= 1024, C % 8 == 0).
    skip_first (x [B, N, C]): the LayerNorm output leaves out every clip's first row (the class token) and is
    [B, N-1, C] -- what TimeSformer's temporal_norm1 consumer reads (`xn[:, 1:]`), as a contiguous tensor."""
    require_device(x, "add_layernorm(x)")
    x = x if x.is_contiguous() else x.contiguous()
    C = x.shape[-1]
    addend = _addend("add_layernorm", addend, x)
    if skip_first and (x.dim() != 3 or x.shape[1] < 2):
        raise TomeHipError("add_layernorm(skip_first): x must be [B, N >= 2, C]")
    # without addend: LayerNorm only, x holds the finished sum already (returned as it is)
    x_out = None if addend is None else torch.empty_like(x)
    y_out = (torch.empty((x.shape[0], x.shape[1] - 1, C), dtype=x.dtype, device=x.device) if skip_first
             else torch.empty_like(x))
    with _on_device(x.device):
        if skip_first:
            rc = lib().tome_add_layernorm_skip_first(x.data_ptr(), _ptr(addend), dtype_code(x, "x"), x.shape[0],
                                                     x.shape[1], C, weight.data_ptr(), bias.data_ptr(), float(eps),
                                                     _ptr(x_out), y_out.data_ptr(), _stream(x.device))
        else:
            rc = lib().tome_add_layernorm(x.data_ptr(), _ptr(addend), dtype_code(x, "x"), x.numel() // C, C,
                                          weight.data_ptr(), bias.data_ptr(), float(eps), _ptr(x_out), y_out.data_ptr(),
                                          _stream(x.device))
    # (the name without an addend has always been the plain entry's)
    _check(rc, "tome_add_layernorm_skip_first" if skip_first and addend is not None else "tome_add_layernorm")
    return (x if addend is None else x_out), y_out


def _f32_params(what: str, C: int, device, *params):
    for p in params:
        if p.numel() != C or p.dtype != torch.float32 or p.device != device:
            raise TomeHipError(f"{what}: the LayerNorm's parameters must hold {C} values of torch.float32 on {device}")
    return [p.detach().contiguous() for p in params]


def _amp_rows(what: str, x: torch.Tensor, skip_first: bool):
    """(groups, group_rows) of [..., C] tokens for the mixed-precision entries."""
    C = x.shape[-1]
    if x.dim() < 2 or C % 8 or C > 1024 or x.numel() == 0:
        raise TomeHipError(f"{what}: tokens must be [..., C] with C % 8 == 0 and C <= 1024, got {tuple(x.shape)}")
    if skip_first:
        if x.dim() != 3 or x.shape[1] < 2:
            raise TomeHipError(f"{what}(skip_first): tokens must be [B, N >= 2, C]")
        return x.shape[0], x.shape[1]
    return x.numel() // C, 1


def add_layernorm_amp(x: torch.Tensor, addend: Optional[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor,
                      eps: float, y_dtype: torch.dtype, skip_first: bool = False):
    """tome_add_layernorm_amp: (x + addend, LayerNorm(x + addend)) in one launch for a model under autocast -- fp32
    weight and bias, y of the 16-bit `y_dtype`, x of y_dtype (addend of the same) or fp32 (addend of y_dtype or fp32; the
    sum is `x + addend.float()`).  addend None: LayerNorm only, x comes back as it is.  skip_first as in add_layernorm."""
    require_device(x, "add_layernorm_amp(x)")
    if y_dtype not in _HALF:
        raise TomeHipError(f"add_layernorm_amp: y_dtype must be a 16-bit dtype, got {y_dtype}")
    x = x if x.is_contiguous() else x.contiguous()
    C = x.shape[-1]
    groups, group_rows = _amp_rows("add_layernorm_amp", x, skip_first)
    weight, bias = _f32_params("add_layernorm_amp", C, x.device, weight, bias)
    addend = _addend("add_layernorm_amp", addend, x, same_dtype=False)
    L = lib()
    entry = require_symbol(L, "tome_add_layernorm_amp")
    x_out = None if addend is None else torch.empty_like(x)
    y_out = torch.empty((x.shape[0], x.shape[1] - 1, C) if skip_first else x.shape, dtype=y_dtype, device=x.device)
    with _on_device(x.device):
        rc = entry(x.data_ptr(), dtype_code(x, "x"), _ptr(addend), 0 if addend is None else dtype_code(addend, "addend"),
                   groups, group_rows, int(bool(skip_first)), C, weight.data_ptr(), bias.data_ptr(), float(eps),
                   _ptr(x_out), y_out.data_ptr(), DTYPES[y_dtype], _stream(x.device))
    _check(rc, "tome_add_layernorm_amp")
    return (x if addend is None else x_out), y_out


def ln_amp_fusable(x: torch.Tensor, norm, *others) -> bool:
    """Can tome_merge_wavg_ln_amp / tome_drop_ln_amp produce norm(x') for this LayerNorm module under autocast (the
    tensors of _ln_amp_of; others[0], when given, is the addend the launch reads beside x), no gradient wanted of any
    participant?  False whenever autocast is off."""
    addend = others[0] if others else None
    return (isinstance(norm, torch.nn.LayerNorm) and x.is_cuda and _ln_amp_of(x, norm, addend)
            and not (torch.is_grad_enabled() and needs_grad(x, norm.weight, norm.bias, *others)))


def merge_ln_amp_trainable(x: torch.Tensor, norm, addend: Optional[torch.Tensor], merge=None) -> bool:
    """Can `norm(merge_wavg(merge, x + addend))` (or the drop form) run under autocast as tome_merge_wavg_ln_amp /
    tome_drop_ln_amp with tome_merge_ln_backward_amp behind it (tome/_ln.py::_MergeLnAmpFunction) when a participant
    requires grad?  The tensors of _ln_amp_of on the device, the stock nn.LayerNorm class (a subclass may carry a forward
    of its own, which a training run must keep) and, as for merge_ln_trainable, the even/odd matching of a MatchPlan
    without threshold flags, on x's device, with r > 0.  merge: the callable that carries the plan; None asks about the
    tensors alone (before the matching exists).  False whenever autocast is off."""
    if not (x.is_cuda and x.dim() == 3 and type(norm) is torch.nn.LayerNorm and _ln_amp_of(x, norm, addend)):
        return False
    if merge is None:
        return True
    plan = getattr(merge, "plan", None)
    return type(plan) is MatchPlan and plan.edge_keep is None and plan.r > 0 and plan.device == x.device


def _amp_merge_args(what: str, plan: MatchPlan, x: torch.Tensor, weight, bias, y_dtype, addend):
    """The checks merge_wavg_ln_amp and drop_ln_amp share: (x, weight, bias, addend) as the entries take them."""
    x = _prep_x(plan, x, f"{what}(x)", plan.T)
    if y_dtype not in _HALF:
        raise TomeHipError(f"{what}: y_dtype must be a 16-bit dtype, got {y_dtype}")
    weight, bias = _f32_params(what, x.shape[-1], x.device, weight, bias)
    return x, weight, bias, _addend(what, addend, x, same_dtype=False)


def merge_wavg_ln_amp(plan: MatchPlan, x: torch.Tensor, size: Optional[torch.Tensor], weight: torch.Tensor,
                      bias: torch.Tensor, eps: float, y_dtype: torch.dtype, addend: Optional[torch.Tensor] = None,
                      log_size: bool = False):
    """tome_merge_wavg_ln_amp: merge_wavg_ln for a model under autocast -- fp32 weight and bias, y_out of the 16-bit
    `y_dtype`, x of y_dtype (addend of the same) or fp32 (addend of y_dtype or fp32; the tokens that are merged are
    `x + addend.float()`).  Returns (x_out, y_out, size_out): x_out and size_out are merge_wavg's of the sum, bit for bit,
    y_out = LayerNorm(x_out)."""
    x, weight, bias, addend = _amp_merge_args("merge_wavg_ln_amp", plan, x, weight, bias, y_dtype, addend)
    n, T, C = x.shape
    size, sdtype = _prep_size(size, n, T, x)
    L = lib()
    entry = require_symbol(L, "tome_merge_wavg_ln_amp")
    x_out = torch.empty((n, T - plan.r, C), dtype=x.dtype, device=x.device)
    y_out = torch.empty((n, T - plan.r, C), dtype=y_dtype, device=x.device)
    s_out = torch.empty((n, T - plan.r, 1), dtype=sdtype, device=x.device)
    log = _log_size_like(s_out, log_size)
    with _on_device(x.device):
        rc = entry(x.data_ptr(), dtype_code(x, "x"), _ptr(addend), 0 if addend is None else dtype_code(addend, "addend"),
                   _ptr(size), DTYPES[sdtype], n, T, C, plan.r, plan.src_idx.data_ptr(), plan.dst_idx.data_ptr(),
                   plan.unm_idx.data_ptr(), int(plan.distill_token), _ptr(plan.edge_keep), weight.data_ptr(),
                   bias.data_ptr(), float(eps), x_out.data_ptr(), y_out.data_ptr(), DTYPES[y_dtype], s_out.data_ptr(),
                   _ptr(log), _stream(x.device))
    _check(rc, "tome_merge_wavg_ln_amp")
    return x_out, y_out, s_out


def drop_ln_amp(plan: MatchPlan, x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float,
                y_dtype: torch.dtype, addend: Optional[torch.Tensor] = None):
    """tome_drop_ln_amp: drop_ln for a model under autocast (dtypes as in merge_wavg_ln_amp).  Returns (x_out, y_out): the
    rows drop keeps of `x + addend`, bit for bit, and their LayerNorm in y_dtype."""
    x, weight, bias, addend = _amp_merge_args("drop_ln_amp", plan, x, weight, bias, y_dtype, addend)
    n, T, C = x.shape
    L = lib()
    entry = require_symbol(L, "tome_drop_ln_amp")
    x_out = torch.empty((n, T - plan.r, C), dtype=x.dtype, device=x.device)
    y_out = torch.empty((n, T - plan.r, C), dtype=y_dtype, device=x.device)
    with _on_device(x.device):
        rc = entry(x.data_ptr(), dtype_code(x, "x"), _ptr(addend), 0 if addend is None else dtype_code(addend, "addend"),
                   n, T, C, plan.r, plan.unm_idx.data_ptr(), int(plan.distill_token), weight.data_ptr(), bias.data_ptr(),
                   float(eps), x_out.data_ptr(), y_out.data_ptr(), DTYPES[y_dtype], _stream(x.device))
    _check(rc, "tome_drop_ln_amp")
    return x_out, y_out


def add_layernorm_regrouped(x: torch.Tensor, addend: torch.Tensor, frames: int, weight: torch.Tensor,
                            bias: torch.Tensor, eps: float):
    """TimeSformer's mid-block step in one launch: x [B, 1 + P*F, C] (class token first), addend [B, P*F, C] ->
    (x1, y) with x1 = cat(cls, x[:, 1:] + addend) and y = LayerNorm of the tokens regrouped
    'b (p t) m -> (b t) p m' with the class token in front of every frame: [B*F, 1 + P, C]."""
    require_device(x, "add_layernorm_regrouped(x)")
    B, N, C = x.shape
    F = int(frames)
    P = (N - 1) // F
    if N != 1 + P * F or tuple(addend.shape) != (B, P * F, C) or addend.dtype != x.dtype or addend.device != x.device:
        raise TomeHipError(f"add_layernorm_regrouped: x {tuple(x.shape)} / addend {tuple(addend.shape)} do not hold a "
                           f"class token and {F} frames of tokens")
    x = x if x.is_contiguous() else x.contiguous()
    addend = addend if addend.is_contiguous() else addend.contiguous()
    x_out = torch.empty_like(x)
    y_out = torch.empty((B * F, 1 + P, C), dtype=x.dtype, device=x.device)
    with _on_device(x.device):
        rc = lib().tome_add_layernorm_regrouped(x.data_ptr(), addend.data_ptr(), dtype_code(x, "x"), B, F, P, C,
                                                weight.data_ptr(), bias.data_ptr(), float(eps), x_out.data_ptr(),
                                                y_out.data_ptr(), _stream(x.device))
    _check(rc, "tome_add_layernorm_regrouped")
    return x_out, y_out


def _prep_regrouped(who: str, plan: MatchPlan, x_full: torch.Tensor, frames: int, has_cls: bool):
    """The prologue of merge_wavg_regrouped / drop_regrouped: x_full [B, has_cls + P*F, C] on the plan's device holds the
    plan's B*F groups of P tokens, no gradient wanted.  Returns (x_full made contiguous, B, C, cls, F, P).  (It asks the
    device itself: one frame, as require_device was, on the host-bound forward.)"""
    if not x_full.is_cuda:
        require_device(x_full, f"{who}(x)")
    if x_full.dim() != 3:
        raise TomeHipError(f"{who}: x must be [B, tokens, C], got {tuple(x_full.shape)}")
    B, N, C = x_full.shape
    cls = 1 if has_cls else 0
    F, P = int(frames), plan.T
    if N != cls + P * F or plan.n != B * F:
        raise TomeHipError(f"{who}: x {tuple(x_full.shape)} does not hold {plan.n} groups of {P} tokens ({F} per clip) "
                           f"plus {cls} class token")
    if x_full.device != plan.device:
        raise TomeHipError(f"{who}: tensor and matching on different devices")
    if torch.is_grad_enabled() and x_full.requires_grad:
        raise TomeHipError(f"{who}: autograd through the HIP merge kernels is not implemented")
    return (x_full if x_full.is_contiguous() else x_full.contiguous()), B, C, cls, F, P


def _regrouped_addend(who: str, plan: MatchPlan, x_full: torch.Tensor, cls: int, addend, addend_grouped, cls_addend):
    """The residual a LayerNorm-fused regrouped reduction reads beside x_full: `addend` in x's layout, or `addend_grouped`
    [B*F, has_cls + P, C] where the spatial attention left it (+ the class tokens' own `cls_addend` [B, 1, C]).
    Returns (addend made contiguous or None, the entry's addend_grouped flag, cls_addend for the entry)."""
    B, _, C = x_full.shape
    P = plan.T
    if addend_grouped is not None:
        if addend is not None:
            raise TomeHipError(f"{who}: pass addend or addend_grouped, not both")
        if tuple(addend_grouped.shape) != (plan.n, cls + P, C) or addend_grouped.dtype != x_full.dtype \
                or addend_grouped.device != x_full.device:
            raise TomeHipError(f"{who}: addend_grouped must be {(plan.n, cls + P, C)} of x's dtype")
        if cls_addend is not None:
            if cls_addend.numel() != B * C or cls_addend.dtype != x_full.dtype or cls_addend.device != x_full.device:
                raise TomeHipError(f"{who}: cls_addend must hold {(B, C)} values of x's dtype")
            cls_addend = cls_addend.contiguous()
        return (addend_grouped if addend_grouped.is_contiguous() else addend_grouped.contiguous()), 1, cls_addend
    return _addend(who, addend, x_full), 0, None


def merge_wavg_regrouped(plan: MatchPlan, x_full: torch.Tensor, size: Optional[torch.Tensor], frames: int,
                         has_cls: bool = True, ln=None, addend: Optional[torch.Tensor] = None,
                         log_size: bool = False, addend_grouped: Optional[torch.Tensor] = None,
                         cls_addend: Optional[torch.Tensor] = None, out_bias: Optional[torch.Tensor] = None):
    """merge_wavg on the interleaved layout of TimeSformer / Motionformer: x_full [B, has_cls + P*F, C] whose
    token has_cls + p*F + f belongs to group b*F + f; returns x_out [B, has_cls + (P-r)*F, C] and size
    [B*F, P-r, 1].  Replaces rearrange -> merge_wavg -> rearrange -> cat (timesformer.py:89-107).
    With ln=(weight, bias, eps) it also returns y_out = LayerNorm(x_out) (class-token rows included) between the
    two, and `addend` (same shape as x_full) is added to the tokens while they are loaded."""
    x_full, B, C, cls, F, P = _prep_regrouped("merge_wavg_regrouped", plan, x_full, frames, has_cls)
    xcode = dtype_code(x_full, "x")
    size, sdtype = _prep_size(size, plan.n, P, x_full)
    x_out = torch.empty((B, cls + (P - plan.r) * F, C), dtype=x_full.dtype, device=x_full.device)
    s_out = torch.empty((plan.n, P - plan.r, 1), dtype=sdtype, device=x_full.device)
    log = _log_size_like(s_out, log_size)
    out_bias = _out_bias(out_bias, x_full, C)
    if ln is None:
        if addend is not None or addend_grouped is not None or out_bias is not None:
            raise TomeHipError("merge_wavg_regrouped: addend / out_bias are only fused together with ln")
        with _on_device(x_full.device):
            rc = lib().tome_merge_wavg_regrouped(x_full.data_ptr(), xcode, _ptr(size), DTYPES[sdtype], B, F, P, C,
                                                 plan.r, cls, plan.src_idx.data_ptr(), plan.dst_idx.data_ptr(),
                                                 plan.unm_idx.data_ptr(), _ptr(plan.edge_keep), x_out.data_ptr(),
                                                 s_out.data_ptr(), _ptr(log), _stream(x_full.device))
        _check(rc, "tome_merge_wavg_regrouped")
        return x_out, s_out
    weight, bias, eps = ln
    addend, grouped, cls_addend = _regrouped_addend("merge_wavg_regrouped", plan, x_full, cls, addend, addend_grouped,
                                                    cls_addend)
    y_out = torch.empty_like(x_out)
    with _on_device(x_full.device):
        rc = lib().tome_merge_wavg_regrouped_ln(x_full.data_ptr(), xcode, _ptr(size), DTYPES[sdtype], B, F, P, C,
                                                plan.r, cls, plan.src_idx.data_ptr(), plan.dst_idx.data_ptr(),
                                                plan.unm_idx.data_ptr(), _ptr(plan.edge_keep), weight.data_ptr(),
                                                bias.data_ptr(), float(eps), _ptr(addend), grouped,
                                                _ptr(cls_addend) if grouped else None, x_out.data_ptr(),
                                                y_out.data_ptr(), s_out.data_ptr(), _ptr(log), _ptr(out_bias),
                                                _stream(x_full.device))
    _check(rc, "tome_merge_wavg_regrouped_ln")
    return x_out, y_out, s_out


def merge(plan: MatchPlan, x: torch.Tensor, mode: str) -> torch.Tensor:
    if mode not in MODES:
        raise TomeHipError(f"merge: unknown reduce mode {mode!r}")
    x = _prep_x(plan, x, "merge(x)", plan.T)
    n, T, C = x.shape
    out = torch.empty((n, T - plan.r, C), dtype=x.dtype, device=x.device)
    with _on_device(x.device):
        rc = lib().tome_merge(x.data_ptr(), dtype_code(x, "x"), n, T, C, plan.r, plan.src_idx.data_ptr(),
                              plan.dst_idx.data_ptr(), plan.unm_idx.data_ptr(), int(plan.distill_token), MODES[mode],
                              _ptr(plan.edge_keep), out.data_ptr(), _stream(x.device))
    _check(rc, "tome_merge")
    return out


def drop(plan: MatchPlan, x: torch.Tensor) -> torch.Tensor:
    x = _prep_x(plan, x, "drop(x)", plan.T)
    n, T, C = x.shape
    out = torch.empty((n, T - plan.r, C), dtype=x.dtype, device=x.device)
    with _on_device(x.device):
        rc = lib().tome_drop(x.data_ptr(), dtype_code(x, "x"), n, T, C, plan.r, plan.unm_idx.data_ptr(),
                             int(plan.distill_token), out.data_ptr(), _stream(x.device))
    _check(rc, "tome_drop")
    return out


def drop_ln(plan: MatchPlan, x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float,
            addend: Optional[torch.Tensor] = None, out_bias: Optional[torch.Tensor] = None):
    """drop + LayerNorm of the kept tokens in one launch: returns (x_out, y_out).  `addend` and `out_bias` as in
    merge_wavg_ln: the kept rows are those of `x + addend`, x_out is stored as x' + out_bias, y_out = LayerNorm(x')."""
    x = _prep_x(plan, x, "drop_ln(x)", plan.T)
    n, T, C = x.shape
    out_bias = _out_bias(out_bias, x, C)
    addend = _addend("drop_ln", addend, x)
    x_out = torch.empty((n, T - plan.r, C), dtype=x.dtype, device=x.device)
    y_out = torch.empty_like(x_out)
    L = lib()
    entry = require_symbol(L, "tome_drop_ln")
    with _on_device(x.device):
        rc = entry(x.data_ptr(), dtype_code(x, "x"), n, T, C, plan.r, plan.unm_idx.data_ptr(), int(plan.distill_token),
                   weight.data_ptr(), bias.data_ptr(), float(eps), _ptr(addend), x_out.data_ptr(), y_out.data_ptr(),
                   _ptr(out_bias), _stream(x.device))
    _check(rc, "tome_drop_ln")
    return x_out, y_out


def _head_view(t: torch.Tensor) -> bool:
    """A [B, H, N, 64] view of a 16-bit device tensor with contiguous channels and 16-byte aligned rows."""
    return (t.is_cuda and t.dim() == 4 and t.shape[-1] == 64 and t.dtype in _HALF and t.stride(-1) == 1
            and all(s % 8 == 0 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0)


def prop_attention_ok(q: torch.Tensor) -> bool:
    """Can tome_prop_attention take these heads (_head_view), no gradient wanted?"""
    return _head_view(q) and not (torch.is_grad_enabled() and needs_grad(q))


def _qkv_heads(who: str, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, bias_skip: bool = False):
    """q [B, H, N, 64] and k / v [B, H, Nk, 64] head views agree (one dtype and device, k and v one shape; bias_skip: as
    many keys as queries).  Returns B, H, N, D, Nk and the three {batch, head, token} stride arrays the entries take --
    built here, so prop_attention(checked=True), on the host-bound forward, has two frames fewer than with _head_strides."""
    if k.dtype != q.dtype or v.dtype != q.dtype or k.device != q.device or v.device != q.device:
        raise TomeHipError(f"{who}: q, k, v must share dtype and device")
    B, H, N, D = q.shape
    if k.shape != v.shape or k.shape[:2] != (B, H):
        raise TomeHipError(f"{who}: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not match")
    Nk = k.shape[2]
    if bias_skip and Nk != N:
        raise TomeHipError(f"{who}: bias_skip needs as many keys as queries")
    i64x3 = ctypes.c_int64 * 3
    return B, H, N, D, Nk, i64x3(*q.stride()[:3]), i64x3(*k.stride()[:3]), i64x3(*v.stride()[:3])


def _key_bias(who: str, log_bias: Optional[torch.Tensor], B: int, keys: int, device) -> Optional[torch.Tensor]:
    """The per-key bias as the attention entries read it: an fp32 [B, keys] view with contiguous rows on `device`, or None."""
    if log_bias is not None and (tuple(log_bias.shape) != (B, keys) or log_bias.dtype != torch.float32
                                 or log_bias.stride(1) != 1 or log_bias.device != device):
        raise TomeHipError(f"{who}: log_bias must be an fp32 {(B, keys)} view with contiguous rows")
    return log_bias


def _grad_rows(who: str, t: torch.Tensor, name: str, shape, q: torch.Tensor) -> torch.Tensor:
    """An output of the forward or its gradient as the backward entries read it: `shape` on q's device, detached, in q's
    dtype, channels contiguous and rows 16-byte aligned (anything else is copied once)."""
    if tuple(t.shape) != shape or t.device != q.device:
        raise TomeHipError(f"{who}: {name} must be {shape} on {q.device}, got {tuple(t.shape)}")
    t = t.detach()
    if t.dtype != q.dtype:
        t = t.to(q.dtype)
    if t.stride(-1) != 1 or any(s % 8 for s in t.stride()[:-1]) or t.data_ptr() % 16:
        t = t.contiguous()
    return t


def _grad_heads(who: str, grads, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor):
    """(dq, dk, dv) of the attention backward entries: the three head views given, validated against q, k, v -- or, grads
    None, fresh ones laid out [B, tokens, H, 64]."""
    if grads is None:
        B, H, N, D = q.shape
        dq = torch.empty((B, N, H, D), dtype=q.dtype, device=q.device).permute(0, 2, 1, 3)
        dk = torch.empty((B, k.shape[2], H, D), dtype=q.dtype, device=q.device).permute(0, 2, 1, 3)
        dv = torch.empty((B, k.shape[2], H, D), dtype=q.dtype, device=q.device).permute(0, 2, 1, 3)
        return dq, dk, dv
    for t, like, name in zip(grads, (q, k, v), ("dq", "dk", "dv")):
        if t.shape != like.shape or t.dtype != q.dtype or t.device != q.device or not _head_view(t):
            raise TomeHipError(f"{who}: {name} must be a {tuple(like.shape)} {q.dtype} head view with 16-byte aligned rows")
    dq, dk, dv = grads
    return dq, dk, dv


def prop_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, size: Optional[torch.Tensor], scale: float,
                   bias_skip: bool = False, log_bias: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, checked: bool = False) -> torch.Tensor:
    """softmax(q k^T * scale + log(size) on the keys) v for head views q [B, H, N, 64], k / v [B, H, Nk, 64] (any
    strides with contiguous channels: the slices of a qkv buffer are read in place); returns [B, N, H*64].
    `size` is the token size tensor [B, Nk(-1), 1] (its log comes from the merge kernel when that emitted it),
    or `log_bias` an fp32 [B, Nk(-1)] view that already holds the bias, or both None.  bias_skip: the TimeSformer
    form -- key 0 / query 0 unbiased, the bias describes keys 1..N-1.  `out`: a [B, N, H, 64] view (channels
    contiguous) to write into instead of a fresh tensor."""
    # (checked: the caller has just asked prop_attention_ok about q, k and v -- the patches do, per layer; at the
    # reference's batch of 8 the forward is bound by host time and the three repeated checks are 7 us of it)
    for t, name in (() if checked else ((q, "q"), (k, "k"), (v, "v"))):
        require_device(t, f"prop_attention({name})")
        if not prop_attention_ok(t):
            raise TomeHipError(f"prop_attention: {name} must be a [B, H, N, 64] 16-bit view with 16-byte aligned rows, "
                               f"got {tuple(t.shape)} {t.dtype} strides {t.stride()}")
    B, H, N, D, Nk, qs, ks, vs = _qkv_heads("prop_attention", q, k, v, bias_skip)
    nb = Nk - (1 if bias_skip else 0)
    log = None
    if size is not None:
        if tuple(size.shape) != (B, nb, 1):
            raise TomeHipError(f"prop_attention: size must be {(B, nb, 1)}, got {tuple(size.shape)}")
        log = log_of_size(size).reshape(B, -1).float().contiguous()
    elif log_bias is not None:
        log = _key_bias("prop_attention", log_bias, B, nb, q.device)
    ostr = None
    if out is None:
        result = out = torch.empty((B, N, H * D), dtype=q.dtype, device=q.device)
    else:
        if tuple(out.shape) != (B, N, H, D) or out.dtype != q.dtype or out.device != q.device or out.stride(3) != 1:
            raise TomeHipError(f"prop_attention: out must be a {(B, N, H, D)} view of the q dtype with contiguous channels")
        ostr = (ctypes.c_int64 * 3)(out.stride(0), out.stride(2), out.stride(1))
        result = out
    with _on_device(q.device):
        rc = lib().tome_prop_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), dtype_code(q, "q"), B, H, N, Nk, D,
                                       qs, ks, vs, _ptr(log),
                                       0 if log is None else log.stride(0), 1 if bias_skip else 0, float(scale),
                                       out.data_ptr(), ostr, _stream(q.device))
    _check(rc, "tome_prop_attention")
    return result


def prop_attention_trainable(q: torch.Tensor, k: Optional[torch.Tensor] = None, v: Optional[torch.Tensor] = None) -> bool:
    """_head_view of every tensor given: can tome_prop_attention run on these heads with tome_prop_attention_backward
    behind it (tome/_attn.py) when they require grad?"""
    return all(t is None or _head_view(t) for t in (q, k, v))


def _head_strides(t: torch.Tensor):
    return (ctypes.c_int64 * 3)(*t.stride()[:3])


def prop_attention_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, dout: torch.Tensor,
                            log_bias: Optional[torch.Tensor], scale: float, bias_skip: bool = False,
                            grads=None, workspace: Optional[torch.Tensor] = None):
    """tome_prop_attention_backward: (dq, dk, dv) of out = prop_attention(q, k, v, ...) given dout.  q [B, H, N, 64],
    k / v [B, H, Nk, 64] head views as the forward took them; out and dout [B, N, H*64] (out: what the forward returned;
    rows of dout 16-byte aligned, channels contiguous -- anything else is copied once).  log_bias: the fp32 [B, Nk(-1)]
    bias the forward used, or None.  grads: three head views to write into (the slices of one [B, N, 3, H, 64] buffer,
    say), or None for fresh [B, H, N, 64] tensors.  workspace: a uint8 device tensor to use instead of a fresh one.
    size gets no gradient.  No CPU path."""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        require_device(t, f"prop_attention_backward({name})")
    if not prop_attention_trainable(q, k, v):
        raise TomeHipError("prop_attention_backward: q, k, v must be [B, H, N, 64] 16-bit views with 16-byte aligned rows")
    who = "prop_attention_backward"
    B, H, N, D, Nk, qs, ks, vs = _qkv_heads(who, q, k, v, bias_skip)
    _key_bias(who, log_bias, B, Nk - (1 if bias_skip else 0), q.device)
    # [B, H, N, 64] views of out and dout
    o4, g4 = (_grad_rows(who, t, name, (B, N, H * D), q).unflatten(2, (H, D)).permute(0, 2, 1, 3)
              for t, name in ((out, "out"), (dout, "dout")))
    dq, dk, dv = _grad_heads(who, grads, q, k, v)
    L = lib()
    entry = require_symbol(L, "tome_prop_attention_backward")
    with _on_device(q.device):
        stream = _stream(q.device)
        ws = workspace if workspace is not None else _sized_workspace(
            L, "tome_prop_attention_backward_workspace_bytes", (B, H, N, Nk), q.device, stream, "prop_attention_backward")
        rc = entry(q.data_ptr(), k.data_ptr(), v.data_ptr(), o4.data_ptr(), g4.data_ptr(), dtype_code(q, "q"), B, H, N, Nk,
                   D, qs, ks, vs, _head_strides(o4), _head_strides(g4),
                   _ptr(log_bias), 0 if log_bias is None else log_bias.stride(0), 1 if bias_skip else 0, float(scale),
                   dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), _head_strides(dq), _head_strides(dk), _head_strides(dv),
                   ws.data_ptr(), ws.numel() * ws.element_size(), stream)
    _check(rc, "tome_prop_attention_backward")
    return dq, dk, dv


def prop_attention_segments(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, nseg: int, scale: float,
                            log_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-segment attention in one launch: queries q [B, H, N, 64]; keys / values [B, H, nseg*P, 64] views whose
    rows [s*P, (s+1)*P) form segment s; every query takes softmax(q k_s^T * scale + log_bias_s) v_s for each
    segment separately (Motionformer: the P keys of one frame, motionformer.py:98-121).  log_bias: fp32
    [B, nseg*P] (contiguous rows) or None.  Returns y [B, N, nseg, H*64]."""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        require_device(t, f"prop_attention_segments({name})")
        if not prop_attention_ok(t) or t.dtype != q.dtype or t.device != q.device:
            raise TomeHipError(f"prop_attention_segments: {name} must be a [B, H, N, 64] 16-bit view with 16-byte "
                               f"aligned rows, got {tuple(t.shape)} {t.dtype} strides {t.stride()}")
    B, H, N, D = q.shape
    nseg = int(nseg)
    if k.shape != v.shape or k.shape[:2] != (B, H) or nseg < 1 or k.shape[2] % nseg:
        raise TomeHipError(f"prop_attention_segments: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}, "
                           f"{nseg} segments do not match")
    P = k.shape[2] // nseg
    _key_bias("prop_attention_segments", log_bias, B, nseg * P, q.device)
    y = torch.empty((B, N, nseg, H * D), dtype=q.dtype, device=q.device)
    ostr = (ctypes.c_int64 * 3)(y.stride(0), D, y.stride(1))  # {batch, head, token}
    seg = (ctypes.c_int64 * 4)(P * k.stride(2), P * v.stride(2), y.stride(2), P)
    with _on_device(q.device):
        rc = lib().tome_prop_attention_segments(q.data_ptr(), k.data_ptr(), v.data_ptr(), dtype_code(q, "q"), B, H, N, P,
                                                D, _head_strides(q), _head_strides(k), _head_strides(v), _ptr(log_bias),
                                                0 if log_bias is None else log_bias.stride(0), float(scale),
                                                y.data_ptr(), ostr, nseg, seg, _stream(q.device))
    _check(rc, "tome_prop_attention_segments")
    return y


def prop_attention_segments_trainable(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, nseg: int) -> bool:
    """Can tome_prop_attention_segments run on these heads (_head_view each, one dtype and device, the keys a whole number
    of segments) with tome_prop_attention_segments_backward behind it (tome/_attn.py) when they require grad?"""
    return (all(_head_view(t) and t.dtype == q.dtype and t.device == q.device for t in (q, k, v))
            and k.shape == v.shape and k.shape[:2] == q.shape[:2] and int(nseg) >= 1 and k.shape[2] >= int(nseg)
            and k.shape[2] % int(nseg) == 0)


def prop_attention_segments_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, y: torch.Tensor, dy: torch.Tensor,
                                     nseg: int, scale: float, log_bias: Optional[torch.Tensor] = None, grads=None,
                                     workspace: Optional[torch.Tensor] = None):
    """tome_prop_attention_segments_backward: (dq, dk, dv) of y = prop_attention_segments(q, k, v, nseg, scale, log_bias)
    given dy.  q [B, H, N, 64], k / v [B, H, nseg*P, 64] head views as the forward took them; y and dy [B, N, nseg, H*64]
    (y: what the forward returned; dy is copied once unless its rows are 16-byte aligned with contiguous channels).
    grads: three head views to write into, of q's and k's shapes (rows of the slices of one [B, N, 3, H, 64] buffer,
    say), or None for fresh tensors.  dq is the sum over the segments, taken in fp32 and rounded once.  No CPU path."""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        require_device(t, f"prop_attention_segments_backward({name})")
    nseg = int(nseg)
    if not prop_attention_segments_trainable(q, k, v, nseg):
        raise TomeHipError(f"prop_attention_segments_backward: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} "
                           f"must be [B, H, N, 64] 16-bit views of one dtype with 16-byte aligned rows, the keys {nseg} "
                           "segments of equal length")
    B, H, N, D = q.shape
    P = k.shape[2] // nseg
    who = "prop_attention_segments_backward"
    _key_bias(who, log_bias, B, nseg * P, q.device)
    y, dy = (_grad_rows(who, t, name, (B, N, nseg, H * D), q) for t, name in ((y, "y"), (dy, "dy")))
    dq, dk, dv = _grad_heads(who, grads, q, k, v)
    L = lib()
    entry = require_symbol(L, "tome_prop_attention_segments_backward")
    i64x3 = ctypes.c_int64 * 3
    seg = (ctypes.c_int64 * 4)(P * k.stride(2), P * v.stride(2), y.stride(2), P)
    gseg = i64x3(dy.stride(2), P * dk.stride(2), P * dv.stride(2))
    with _on_device(q.device):
        stream = _stream(q.device)
        ws = workspace if workspace is not None else _sized_workspace(
            L, "tome_prop_attention_segments_backward_workspace_bytes", (B, H, N, P, nseg), q.device, stream,
            "prop_attention_segments_backward")
        rc = entry(q.data_ptr(), k.data_ptr(), v.data_ptr(), y.data_ptr(), dy.data_ptr(), dtype_code(q, "q"), B, H, N, P, D,
                   _head_strides(q), _head_strides(k), _head_strides(v), i64x3(y.stride(0), D, y.stride(1)),
                   i64x3(dy.stride(0), D, dy.stride(1)), _ptr(log_bias), 0 if log_bias is None else log_bias.stride(0),
                   float(scale), nseg, seg, gseg, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), _head_strides(dq),
                   _head_strides(dk), _head_strides(dv), ws.data_ptr(), ws.numel() * ws.element_size(), stream)
    _check(rc, "tome_prop_attention_segments_backward")
    return dq, dk, dv


def _short_heads(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> bool:
    """[B, H, N <= 8, 64] views of 16-bit tensors on one device whose heads lie side by side in a token's row (head
    stride 64), rows 16-byte aligned."""
    def ok(t):
        return (t.is_cuda and t.dim() == 4 and t.shape == q.shape and t.dtype == q.dtype and t.device == q.device
                and t.stride(3) == 1 and t.stride(1) == 64 and t.stride(0) % 8 == 0 and t.stride(2) % 8 == 0
                and t.data_ptr() % 16 == 0)
    return (q.dim() == 4 and q.dtype in _HALF and q.shape[-1] == 64 and 1 <= q.shape[2] <= 8
            and ok(q) and ok(k) and ok(v))


def short_attention_ok(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> bool:
    """Can tome_short_attention take these (_short_heads), no gradient wanted?"""
    return _short_heads(q, k, v) and not (torch.is_grad_enabled() and needs_grad(q, k, v))


def short_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, checked: bool = False
                    ) -> torch.Tensor:
    """softmax(q k^T * scale) v over sequences of at most 8 tokens (TimeSformer's temporal attention): q, k, v
    [B, H, N, 64] views of one qkv projection, read in place; returns [B, N, H*64].  checked: the caller has just
    asked short_attention_ok."""
    for t, name in (() if checked else ((q, "q"), (k, "k"), (v, "v"))):
        require_device(t, f"short_attention({name})")
    if not checked and not short_attention_ok(q, k, v):
        raise TomeHipError(f"short_attention: q, k, v must be [B, H, N <= 8, 64] 16-bit views with head stride 64 and "
                           f"16-byte aligned rows, got {tuple(q.shape)} {q.dtype} strides {q.stride()}")
    B, H, N, D = q.shape
    out = torch.empty((B, N, H * D), dtype=q.dtype, device=q.device)
    with _on_device(q.device):
        rc = lib().tome_short_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), dtype_code(q, "q"), B, H, N, D,
                                        _head_strides(q), _head_strides(k), _head_strides(v), float(scale),
                                        out.data_ptr(), _stream(q.device))
    _check(rc, "tome_short_attention")
    return out


def short_attention_trainable(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> bool:
    """Can tome_short_attention run on these heads (_short_heads) with tome_short_attention_backward behind it
    (tome/_attn.py) when they require grad?  q, k, v that alias one tensor (with_qkv=False) are refused: their three
    gradients would have to be summed."""
    return _short_heads(q, k, v) and len({q.data_ptr(), k.data_ptr(), v.data_ptr()}) == 3


def short_attention_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, dout: torch.Tensor, scale: float,
                             grads=None):
    """tome_short_attention_backward: (dq, dk, dv) of out = short_attention(q, k, v, scale) given dout [B, N, H*64].
    q, k, v: the [B, H, N <= 8, 64] head views the forward took.  grads: three head views to write into (the slices of
    one [B, N, 3, H, 64] buffer, say; every element of them is written), or None for fresh tensors.  No CPU path."""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        require_device(t, f"short_attention_backward({name})")
    if not short_attention_trainable(q, k, v):
        raise TomeHipError(f"short_attention_backward: q, k, v must be three distinct [B, H, N <= 8, 64] 16-bit views with "
                           f"head stride 64 and 16-byte aligned rows, got {tuple(q.shape)} {q.dtype} strides {q.stride()}")
    B, H, N, D = q.shape
    if tuple(dout.shape) != (B, N, H * D) or dout.device != q.device:
        raise TomeHipError(f"short_attention_backward: dout must be {(B, N, H * D)} on {q.device}, got {tuple(dout.shape)}")
    dout = dout.detach()
    if dout.dtype != q.dtype:
        dout = dout.to(q.dtype)
    if not dout.is_contiguous() or dout.data_ptr() % 16:
        dout = dout.contiguous()
    if grads is None:
        dq, dk, dv = (torch.empty((B, N, H, D), dtype=q.dtype, device=q.device).permute(0, 2, 1, 3) for _ in range(3))
    else:
        dq, dk, dv = grads
        for t, name in ((dq, "dq"), (dk, "dk"), (dv, "dv")):
            if (t.shape != q.shape or t.dtype != q.dtype or t.device != q.device or t.stride(3) != 1 or t.stride(1) != 64
                    or t.stride(0) % 8 or t.stride(2) % 8 or t.data_ptr() % 16):
                raise TomeHipError(f"short_attention_backward: {name} must be a {tuple(q.shape)} {q.dtype} head view with "
                                   "head stride 64 and 16-byte aligned rows")
    entry = require_symbol(lib(), "tome_short_attention_backward")
    with _on_device(q.device):
        rc = entry(q.data_ptr(), k.data_ptr(), v.data_ptr(), dout.data_ptr(), dtype_code(q, "q"), B, H, N, D,
                   _head_strides(q), _head_strides(k), _head_strides(v), float(scale), dq.data_ptr(), dk.data_ptr(),
                   dv.data_ptr(), _head_strides(dq), _head_strides(dk), _head_strides(dv), _stream(q.device))
    _check(rc, "tome_short_attention_backward")
    return dq, dk, dv


def _trajectory_rows(q2: torch.Tensor, k2: torch.Tensor, val: torch.Tensor, heads: int) -> bool:
    """q2 [B, S, C], k2 / val [B, S, F, C] views (rows contiguous over C, (b, s, f) rows evenly spaced), 16-bit, head
    dim 64, at most 16 heads and 8 frames."""
    if not (q2.is_cuda and q2.dtype in (torch.bfloat16, torch.float16) and q2.dim() == 3 and k2.dim() == 4):
        return False
    B, S, C = q2.shape
    F = k2.shape[2]
    def rows_ok(t):
        return (t.shape == (B, S, F, C) and t.dtype == q2.dtype and t.stride(3) == 1 and t.stride(2) % 8 == 0
                and t.stride(1) == F * t.stride(2) and t.stride(0) == S * t.stride(1) and t.data_ptr() % 16 == 0)
    return (C == heads * 64 and heads <= 16 and F <= 8 and q2.is_contiguous() and q2.data_ptr() % 16 == 0
            and rows_ok(k2) and rows_ok(val))


def trajectory_mix_ok(q2: torch.Tensor, k2: torch.Tensor, val: torch.Tensor, heads: int) -> bool:
    """Can tome_trajectory_mix take these (_trajectory_rows), no gradient wanted?"""
    return _trajectory_rows(q2, k2, val, heads) and not (torch.is_grad_enabled() and needs_grad(q2, k2, val))


def trajectory_mix_trainable(q2: torch.Tensor, k2: torch.Tensor, val: torch.Tensor, heads: int) -> bool:
    """Can tome_trajectory_mix run on these (_trajectory_rows) with tome_trajectory_mix_backward behind it (tome/_attn.py)
    when they require grad?"""
    return _trajectory_rows(q2, k2, val, heads)


def trajectory_mix(q2: torch.Tensor, k2: torch.Tensor, val: torch.Tensor, heads: int, scale: float,
                   want_attn: bool = True, out: Optional[torch.Tensor] = None):
    """softmax over the F frames of (q2*scale . k2[f]) per (batch, token, head), then the weighted sum of val[f]:
    returns (out [B, S, C], attn [B, heads, S, F] fp32 or None).  `out`: a [B, S, C] view with contiguous rows
    (stride(1) == C) to write into -- e.g. rows 1.. of the [B, 1+S, C] buffer whose row 0 takes the class token."""
    if not trajectory_mix_ok(q2, k2, val, heads):
        raise TomeHipError("trajectory_mix: unsupported tensors (16-bit, head dim 64, <= 16 heads, <= 8 frames, "
                           "evenly spaced 16-byte aligned rows)")
    B, S, C = q2.shape
    F = k2.shape[2]
    if out is None:
        out = torch.empty((B, S, C), dtype=q2.dtype, device=q2.device)
    elif (tuple(out.shape) != (B, S, C) or out.dtype != q2.dtype or out.device != q2.device or out.stride(2) != 1
          or out.stride(1) != C or out.stride(0) % 8 or out.stride(0) < S * C or out.data_ptr() % 16):
        raise TomeHipError(f"trajectory_mix: out must be a {(B, S, C)} view of the q2 dtype with contiguous 16-byte "
                           f"aligned rows, got {tuple(out.shape)} {out.dtype} strides {out.stride()}")
    attn = torch.empty((B, heads, S, F), dtype=torch.float32, device=q2.device) if want_attn else None
    with _on_device(q2.device):
        rc = lib().tome_trajectory_mix(q2.data_ptr(), k2.data_ptr(), val.data_ptr(), dtype_code(q2, "q2"), B, S, F, heads,
                                       64, k2.stride(2), val.stride(2), float(scale), out.data_ptr(), out.stride(0),
                                       _ptr(attn), _stream(q2.device))
    _check(rc, "tome_trajectory_mix")
    return out, attn


def trajectory_mix_backward(q2: torch.Tensor, k2: torch.Tensor, val: torch.Tensor, dout: torch.Tensor, heads: int,
                            scale: float, want_k2: bool = True, want_val: bool = True, grads=None):
    """tome_trajectory_mix_backward: (dq2, dk2, dval) of out = trajectory_mix(q2, k2, val, heads, scale)[0] given dout
    [B, S, C] (rows contiguous, any batch stride: a slice of the [B, 1+S, C] gradient is read in place; anything else is
    copied once).  want_k2 / want_val False: that gradient is not computed and comes back as None.  grads: (dq2, dk2,
    dval) targets -- dq2 [B, S, C] contiguous, dk2 / dval [B, S, F, C] views with evenly spaced rows (the two halves of
    one [B, S, F, 2C] buffer, say), None for an unwanted one -- or None for fresh tensors.  The attention map of the
    forward gets no gradient.  No CPU path."""
    require_device(q2, "trajectory_mix_backward(q2)")
    if not trajectory_mix_trainable(q2, k2, val, heads):
        raise TomeHipError("trajectory_mix_backward: unsupported tensors (16-bit, head dim 64, <= 16 heads, <= 8 frames, "
                           "evenly spaced 16-byte aligned rows)")
    B, S, C = q2.shape
    F = k2.shape[2]
    if tuple(dout.shape) != (B, S, C) or dout.device != q2.device:
        raise TomeHipError(f"trajectory_mix_backward: dout must be {(B, S, C)} on {q2.device}, got {tuple(dout.shape)}")
    dout = dout.detach()
    if dout.dtype != q2.dtype:
        dout = dout.to(q2.dtype)
    if (dout.stride(2) != 1 or dout.stride(1) != C or (B > 1 and (dout.stride(0) % 8 or dout.stride(0) < S * C))
            or dout.data_ptr() % 16):
        dout = dout.contiguous()
    if grads is None:
        dq2 = torch.empty((B, S, C), dtype=q2.dtype, device=q2.device)
        dk2 = torch.empty((B, S, F, C), dtype=q2.dtype, device=q2.device) if want_k2 else None
        dval = torch.empty((B, S, F, C), dtype=q2.dtype, device=q2.device) if want_val else None
    else:
        dq2, dk2, dval = grads
        if (tuple(dq2.shape) != (B, S, C) or dq2.dtype != q2.dtype or dq2.device != q2.device or not dq2.is_contiguous()
                or dq2.data_ptr() % 16):
            raise TomeHipError(f"trajectory_mix_backward: dq2 must be a contiguous {(B, S, C)} {q2.dtype} tensor")
        for t, name, want in ((dk2, "dk2", want_k2), (dval, "dval", want_val)):
            if (t is None) == want or (t is not None and not _trajectory_rows(q2, t, t, heads)):
                raise TomeHipError(f"trajectory_mix_backward: {name} must be a {(B, S, F, C)} {q2.dtype} view with evenly "
                                   "spaced 16-byte aligned rows when wanted, None when not")
    entry = require_symbol(lib(), "tome_trajectory_mix_backward")
    with _on_device(q2.device):
        rc = entry(q2.data_ptr(), k2.data_ptr(), val.data_ptr(), dout.data_ptr(), dtype_code(q2, "q2"), B, S, F, heads, 64,
                   k2.stride(2), val.stride(2), dout.stride(0) if B > 1 else 0, float(scale), dq2.data_ptr(), _ptr(dk2),
                   _ptr(dval), 0 if dk2 is None else dk2.stride(2), 0 if dval is None else dval.stride(2),
                   _stream(q2.device))
    _check(rc, "tome_trajectory_mix_backward")
    return dq2, dk2, dval


def drop_regrouped(plan: MatchPlan, x_full: torch.Tensor, frames: int, has_cls: bool = True, ln=None,
                   addend: Optional[torch.Tensor] = None, addend_grouped: Optional[torch.Tensor] = None,
                   cls_addend: Optional[torch.Tensor] = None, out_bias: Optional[torch.Tensor] = None):
    """drop on the interleaved layout (see merge_wavg_regrouped): x_full [B, has_cls + P*F, C] ->
    [B, has_cls + (P-r)*F, C], replacing rearrange -> drop -> rearrange -> cat (timesformer.py:111-131).
    With ln=(weight, bias, eps) it returns (x_out, y_out), y_out = LayerNorm(x_out) (class-token rows included);
    addend / addend_grouped + cls_addend / out_bias as in merge_wavg_regrouped."""
    x_full, B, C, cls, F, P = _prep_regrouped("drop_regrouped", plan, x_full, frames, has_cls)
    out = torch.empty((B, cls + (P - plan.r) * F, C), dtype=x_full.dtype, device=x_full.device)
    out_bias = _out_bias(out_bias, x_full, C)
    if ln is not None:
        weight, bias, eps = ln
        addend, grouped, cls_addend = _regrouped_addend("drop_regrouped", plan, x_full, cls, addend, addend_grouped,
                                                        cls_addend)
        y_out = torch.empty_like(out)
        L = lib()
        entry = require_symbol(L, "tome_drop_regrouped_ln")
        with _on_device(x_full.device):
            rc = entry(x_full.data_ptr(), dtype_code(x_full, "x"), B, F, P, C, plan.r, cls, plan.unm_idx.data_ptr(),
                       weight.data_ptr(), bias.data_ptr(), float(eps), _ptr(addend), grouped, _ptr(cls_addend),
                       out.data_ptr(), y_out.data_ptr(), _ptr(out_bias), _stream(x_full.device))
        _check(rc, "tome_drop_regrouped_ln")
        return out, y_out
    if addend is not None or addend_grouped is not None or out_bias is not None:
        raise TomeHipError("drop_regrouped: addend / out_bias are only fused together with ln")
    with _on_device(x_full.device):
        rc = lib().tome_drop_regrouped(x_full.data_ptr(), dtype_code(x_full, "x"), B, F, P, C, plan.r, cls,
                                       plan.unm_idx.data_ptr(), out.data_ptr(), _stream(x_full.device))
    _check(rc, "tome_drop_regrouped")
    return out


def unmerge(plan: MatchPlan, x: torch.Tensor) -> torch.Tensor:
    x = _prep_x(plan, x, "unmerge(x)", plan.T - plan.r)
    n, _, C = x.shape
    out = torch.empty((n, plan.T, C), dtype=x.dtype, device=x.device)
    with _on_device(x.device):
        rc = lib().tome_unmerge(x.data_ptr(), dtype_code(x, "x"), n, plan.T, C, plan.r, plan.src_idx.data_ptr(),
                                plan.dst_idx.data_ptr(), plan.unm_idx.data_ptr(), out.data_ptr(), _stream(x.device))
    _check(rc, "tome_unmerge")
    return out


def gelu_ok(x: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and x.is_contiguous() and x.numel() % 8 == 0
            and x.numel() > 0 and x.data_ptr() % 16 == 0 and not (torch.is_grad_enabled() and needs_grad(x)))


def _gelu(name: str, x: torch.Tensor, inplace: bool) -> torch.Tensor:
    """The streaming activation launch `tome_<name>` (gelu_erf / gelu_tanh) of a contiguous 16-bit tensor."""
    if not gelu_ok(x):
        raise TomeHipError(f"{name}: contiguous 16-bit device tensor with a multiple of 8 elements required")
    entry = require_symbol(lib(), "tome_" + name)
    y = x if inplace else torch.empty_like(x)
    with _on_device(x.device):
        rc = entry(x.data_ptr(), dtype_code(x, "x"), x.numel(), y.data_ptr(), _stream(x.device))
    _check(rc, "tome_" + name)
    return y


def gelu_erf(x: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """nn.GELU() (exact erf form) of a contiguous 16-bit tensor, bit-identical to torch's, as one streaming pass."""
    return _gelu("gelu_erf", x, inplace)


def gelu_tanh(x: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """The tanh GELU (HF's gelu_fast, F.gelu(approximate="tanh")) of a contiguous 16-bit tensor in the sigmoid form of
    include/tome_hip.h: x * sigma(2 beta (x + kappa x^3)), no cancellation on the negative side; one streaming pass."""
    return _gelu("gelu_tanh", x, inplace)


def token_mean_ok(x: torch.Tensor) -> bool:
    """Can tome_token_mean read these tokens?  A contiguous 16-bit [groups, tokens, width] device tensor with
    width % 8 == 0, 16-byte aligned, no gradient wanted."""
    return (x.is_cuda and x.dim() == 3 and x.dtype in _HALF and x.is_contiguous() and x.numel() > 0
            and x.shape[-1] % 8 == 0 and x.data_ptr() % 16 == 0 and not (torch.is_grad_enabled() and needs_grad(x)))


def token_mean(x: torch.Tensor, gelu: bool = False) -> torch.Tensor:
    """tome_token_mean: the fp32 mean over the tokens of x [groups, tokens, width] -> [groups, width]; gelu: of the
    16-bit values gelu_erf(x) would hold (the activation is not written).  Fixed summation order, no atomics."""
    if not token_mean_ok(x):
        raise TomeHipError("token_mean: contiguous 16-bit [groups, tokens, width] device tensor with width % 8 == 0 "
                           f"required, got {tuple(x.shape)} {x.dtype} on {x.device}")
    groups, tokens, width = x.shape
    entry = require_symbol(lib(), "tome_token_mean")
    out = torch.empty((groups, width), dtype=torch.float32, device=x.device)
    with _on_device(x.device):
        rc = entry(x.data_ptr(), DTYPES[x.dtype], groups, tokens, width, int(bool(gelu)), out.data_ptr(), _stream(x.device))
    _check(rc, "tome_token_mean")
    return out


GELU_BWD_MAX_WIDTH = 8192  # csrc/tome_kernels.hip: GELU_BWD_MAX_WIDTH


def mlp_trainable(y: torch.Tensor, fc1, fc2, act) -> bool:
    """Can `fc2(act(fc1(y)))` run as the Function of tome/_mlp.py (library GEMMs, tome_gelu_erf forward,
    tome_gelu_erf_backward backward) when y or the parameters require grad?  16-bit device tokens, the stock nn.Linear /
    exact-erf nn.GELU modules, parameters of the tokens' dtype, hidden width within the kernel's limits, 16-byte rows."""
    from ._mlp import _stock_module
    if not (_stock_module(fc1, torch.nn.Linear) and _stock_module(fc2, torch.nn.Linear)
            and _stock_module(act, torch.nn.GELU) and getattr(act, "approximate", "none") == "none"):
        return False
    return mlp_tensors_trainable(y, fc1, fc2)


def mlp_tensors_trainable(y: torch.Tensor, fc1, fc2) -> bool:
    """The dtype, device and width conditions of the MLP Function for two nn.Linear layers, whatever the activation's
    form (mlp_trainable: exact-erf; tome/_mlp.py pair_trainable: ViViT's tanh pair)."""
    C, Hd = fc1.in_features, fc1.out_features
    params = [fc1.weight, fc2.weight] + [b for b in (fc1.bias, fc2.bias) if b is not None]
    return (y.is_cuda and y.dtype in (torch.bfloat16, torch.float16) and y.dim() >= 2 and y.shape[-1] == C
            and y.numel() > 0 and fc2.in_features == Hd and Hd % 8 == 0 and Hd <= GELU_BWD_MAX_WIDTH
            and (C * y.element_size()) % 16 == 0 and (fc2.out_features * y.element_size()) % 16 == 0
            and all(p.dtype == y.dtype and p.device == y.device for p in params))


def _gelu_backward(name: str, h: torch.Tensor, ga: torch.Tensor, want_act: bool, want_bias: bool, inplace: bool):
    """`tome_<name>` (gelu_erf_backward / gelu_tanh_backward): the checks, buffers and workspace the two entries share
    (the workspace is sized by tome_gelu_erf_backward_workspace_bytes for both)."""
    require_device(h, f"{name}(h)")
    if h.dtype not in (torch.bfloat16, torch.float16):
        raise TomeHipError(f"{name}: 16-bit tensors only, got {h.dtype}")
    Hd = h.shape[-1] if h.dim() >= 2 else 0
    if Hd == 0 or Hd % 8 or Hd > GELU_BWD_MAX_WIDTH or h.numel() == 0:
        raise TomeHipError(f"{name}: h must be [..., Hd] with Hd % 8 == 0 and Hd <= {GELU_BWD_MAX_WIDTH}, "
                           f"got {tuple(h.shape)}")
    if ga.shape != h.shape or ga.dtype != h.dtype or ga.device != h.device:
        raise TomeHipError(f"{name}: ga must have h's shape, dtype and device")
    if not h.is_contiguous() or not ga.is_contiguous():
        raise TomeHipError(f"{name}: contiguous tensors required")
    h, ga = h.detach(), ga.detach()
    rows = h.numel() // Hd
    L = lib()
    entry = require_symbol(L, "tome_" + name)
    gh = ga if inplace else torch.empty_like(ga)
    act = torch.empty_like(h) if want_act else None
    dbias = torch.empty(Hd, dtype=h.dtype, device=h.device) if want_bias else None
    with _on_device(h.device):
        stream = _stream(h.device)
        ws = _sized_workspace(L, "tome_gelu_erf_backward_workspace_bytes", (rows, Hd), h.device, stream,
                              name) if want_bias else None
        rc = entry(h.data_ptr(), ga.data_ptr(), dtype_code(h, "h"), rows, Hd, gh.data_ptr(), _ptr(act), _ptr(dbias),
                   _ptr(ws), 0 if ws is None else ws.numel(), stream)
    _check(rc, "tome_" + name)
    return gh, act, dbias


def gelu_erf_backward(h: torch.Tensor, ga: torch.Tensor, *, want_act: bool, want_bias: bool, inplace: bool = True):
    """tome_gelu_erf_backward for contiguous 16-bit h, ga [..., Hd]: (gh, act, dbias).  gh = ga * gelu'(h), written over
    ga when `inplace`; act = gelu(h) with the forward's bits when want_act, else None; dbias [Hd] = the column sums of
    the rounded gh when want_bias, else None (then no workspace is taken).  No CPU path."""
    return _gelu_backward("gelu_erf_backward", h, ga, want_act, want_bias, inplace)


def gelu_tanh_backward(h: torch.Tensor, ga: torch.Tensor, *, want_act: bool, want_bias: bool, inplace: bool = True):
    """tome_gelu_tanh_backward: gelu_erf_backward for the tanh form (ViViT's MLP); act has tome_gelu_tanh's bits."""
    return _gelu_backward("gelu_tanh_backward", h, ga, want_act, want_bias, inplace)


def tubelet_rows_ok(x: torch.Tensor, kt: int, kh: int, kw: int) -> bool:
    """x [B, C, T, H, W] (any view with unit stride along W) can be regrouped by tome_tubelet_rows."""
    if not (x.is_cuda and x.dim() == 5 and x.dtype in DTYPES and x.numel() > 0 and x.stride(4) == 1
            and not (torch.is_grad_enabled() and needs_grad(x))):
        return False
    es = x.element_size()
    _, _, T, H, W = x.shape
    return (T % kt == 0 and H % kh == 0 and W % kw == 0 and (kw * es) % 16 == 0 and x.data_ptr() % 16 == 0
            and all(s >= 0 and (s * es) % 16 == 0 for s in x.stride()[:4]))


def tubelet_rows(x: torch.Tensor, kt: int, kh: int, kw: int) -> torch.Tensor:
    """rows [B, T'*H'*W', C*kt*kh*kw] of a clip x [B, C, T, H, W]: the matrix a stride == kernel convolution's weight
    multiplies (tome_tubelet_rows: a pure 16-byte move, token order = conv(x).flatten(2).transpose(1, 2))."""
    if not tubelet_rows_ok(x, kt, kh, kw):
        require_device(x, "tubelet_rows(x)")
        raise TomeHipError(f"tubelet_rows: x {tuple(x.shape)} strides {x.stride()} with tubelets {(kt, kh, kw)} "
                           "cannot be regrouped in 16-byte chunks")
    B, C, T, H, W = x.shape
    rows = torch.empty((B, (T // kt) * (H // kh) * (W // kw), C * kt * kh * kw), dtype=x.dtype, device=x.device)
    strides = (ctypes.c_int64 * 4)(*x.stride()[:4])
    with _on_device(x.device):
        rc = lib().tome_tubelet_rows(x.data_ptr(), x.element_size(), B, C, T, H, W, strides, kt, kh, kw,
                                     rows.data_ptr(), _stream(x.device))
    _check(rc, "tome_tubelet_rows")
    return rows


def plan_row_map(plan: MatchPlan) -> torch.Tensor:
    """The matching's row map [n, T1] int32 (merged row of every even token); made once per plan by tome_row_map when
    the matching was not asked for it."""
    if plan.row_map is None:
        T1 = (plan.T + 1) // 2
        row_map = torch.empty((plan.n, T1), dtype=torch.int32, device=plan.device)
        with _on_device(plan.device):
            _check(lib().tome_row_map(plan.n, plan.T, plan.r, int(plan.distill_token), plan.src_idx.data_ptr(),
                                      plan.dst_idx.data_ptr(), plan.unm_idx.data_ptr(), row_map.data_ptr(),
                                      _stream(plan.device)), "tome_row_map")
        plan.row_map = row_map
    return plan.row_map


def plan_count(plan: MatchPlan) -> torch.Tensor:
    """[n, T-r, 1] fp32: how many tokens every merged row holds (the divisor of merge(x, "mean")); made once per plan
    by tome_merge of a column of ones in mode sum."""
    if plan.count is None:
        with torch.no_grad():
            plan.count = merge(plan, torch.ones((plan.n, plan.T, 1), dtype=torch.float32, device=plan.device), "sum")
    return plan.count


def _prep_grad(g: torch.Tensor, shape, dtype, device, what: str) -> torch.Tensor:
    require_device(g, what)
    if tuple(g.shape) != tuple(shape) or g.dtype != dtype or g.device != device:
        raise TomeHipError(f"{what}: expected a gradient {tuple(shape)} of {dtype} on {device}, got {tuple(g.shape)} of "
                           f"{g.dtype} on {g.device}")
    g = g.detach()
    return g if g.is_contiguous() else g.contiguous()


def _prep_scales(out_div, in_mul, n, T, To, x_dtype, device, what: str):
    """out_div [n, To, 1] / in_mul [n, T, 1] (either may be None) in one dtype the kernel takes: x's or fp32."""
    given = [s for s in (out_div, in_mul) if s is not None]
    if not given:
        return None, None, x_dtype
    for s, rows in ((out_div, To), (in_mul, T)):
        if s is not None and (s.numel() != n * rows or s.device != device):
            raise TomeHipError(f"{what}: a scale with {n * rows} values on {device} expected, got {tuple(s.shape)} on "
                               f"{s.device}")
    sdtype = given[0].dtype if all(s.dtype == given[0].dtype for s in given) else torch.float32
    if sdtype not in (x_dtype, torch.float32):
        sdtype = torch.float32
    conv = lambda s: None if s is None else s.detach().to(sdtype).contiguous()  # noqa: E731
    return conv(out_div), conv(in_mul), sdtype


def merge_backward(plan: MatchPlan, grad_out: torch.Tensor, out_div: Optional[torch.Tensor] = None,
                   in_mul: Optional[torch.Tensor] = None, drop: bool = False) -> torch.Tensor:
    """tome_merge_backward: grad_in[t] = grad_out[row of t] / out_div[row of t] * in_mul[t] for a gradient
    [n, T-r, C] of merge / merge_wavg / drop; returns [n, T, C]."""
    if grad_out.dim() != 3:
        raise TomeHipError(f"merge_backward: gradient must be [n, tokens, C], got {tuple(grad_out.shape)}")
    n, T, To, C = plan.n, plan.T, plan.T - plan.r, grad_out.shape[-1]
    g = _prep_grad(grad_out, (n, To, C), grad_out.dtype, plan.device, "merge_backward(grad)")
    xcode = dtype_code(g, "grad")
    out_div, in_mul, sdtype = _prep_scales(out_div, in_mul, n, T, To, g.dtype, plan.device, "merge_backward")
    row_map = plan_row_map(plan)
    gx = torch.empty((n, T, C), dtype=g.dtype, device=g.device)
    with _on_device(g.device):
        rc = lib().tome_merge_backward(g.data_ptr(), xcode, _ptr(out_div), _ptr(in_mul), DTYPES[sdtype], n, T, C, plan.r,
                                       row_map.data_ptr(), int(plan.distill_token), int(bool(drop)), gx.data_ptr(),
                                       _stream(g.device))
    _check(rc, "tome_merge_backward")
    return gx


def merge_backward_regrouped(plan: MatchPlan, grad_out: torch.Tensor, frames: int, has_cls: bool = True,
                             out_div: Optional[torch.Tensor] = None, in_mul: Optional[torch.Tensor] = None,
                             drop: bool = False) -> torch.Tensor:
    """tome_merge_backward_regrouped: the gradient [B, has_cls + (P-r)*F, C] of merge_wavg_regrouped / drop_regrouped
    taken back to [B, has_cls + P*F, C]; class rows pass through."""
    if grad_out.dim() != 3:
        raise TomeHipError(f"merge_backward_regrouped: gradient must be [B, tokens, C], got {tuple(grad_out.shape)}")
    cls = 1 if has_cls else 0
    F, P = int(frames), plan.T
    if F <= 0 or plan.n % F:
        raise TomeHipError(f"merge_backward_regrouped: {plan.n} groups do not split into clips of {F} frames")
    B, C = plan.n // F, grad_out.shape[-1]
    g = _prep_grad(grad_out, (B, cls + (P - plan.r) * F, C), grad_out.dtype, plan.device,
                   "merge_backward_regrouped(grad)")
    xcode = dtype_code(g, "grad")
    out_div, in_mul, sdtype = _prep_scales(out_div, in_mul, plan.n, P, P - plan.r, g.dtype, plan.device,
                                           "merge_backward_regrouped")
    row_map = plan_row_map(plan)
    gx = torch.empty((B, cls + P * F, C), dtype=g.dtype, device=g.device)
    with _on_device(g.device):
        rc = lib().tome_merge_backward_regrouped(g.data_ptr(), xcode, _ptr(out_div), _ptr(in_mul), DTYPES[sdtype], B, F, P,
                                                 C, plan.r, cls, row_map.data_ptr(), int(bool(drop)), gx.data_ptr(),
                                                 _stream(g.device))
    _check(rc, "tome_merge_backward_regrouped")
    return gx


def _layernorm_backward_call(what: str, gy, gy_shape, xs, gx_in, weight, eps, want_weight, want_bias, dims, ws_dims):
    """What tome_layernorm_backward and its regrouped form share behind their shape checks: the gradients prepared,
    gx / dweight / dbias allocated, the workspace taken when a parameter gradient is wanted, and the call of entry
    tome_<what>(gy, xs, gx_in, dtype, *dims, C, weight, eps, gx, dweight, dbias, workspace, stream) with a workspace of
    tome_<what>_workspace_bytes(*ws_dims).  Returns (gx, dweight, dbias)."""
    C = xs.shape[-1]
    if weight.numel() != C or weight.dtype != xs.dtype or weight.device != xs.device:
        raise TomeHipError(f"{what}: weight must hold {C} values of {xs.dtype} on {xs.device}")
    gy = _prep_grad(gy, gy_shape, xs.dtype, xs.device, f"{what}(gy)")
    if gx_in is not None:
        gx_in = _prep_grad(gx_in, tuple(xs.shape), xs.dtype, xs.device, f"{what}(gx_in)")
    xs = xs.detach()
    xs = xs if xs.is_contiguous() else xs.contiguous()
    weight = weight.detach().contiguous()
    L = lib()
    entry = require_symbol(L, f"tome_{what}")
    gx = torch.empty_like(xs)
    dweight = torch.empty(C, dtype=xs.dtype, device=xs.device) if want_weight else None
    dbias = torch.empty(C, dtype=xs.dtype, device=xs.device) if want_bias else None
    with _on_device(xs.device):
        stream = _stream(xs.device)
        ws = _sized_workspace(L, f"tome_{what}_workspace_bytes", ws_dims, xs.device, stream,
                              what) if want_weight or want_bias else None
        rc = entry(gy.data_ptr(), xs.data_ptr(), _ptr(gx_in), dtype_code(xs, "xs"), *dims, C, weight.data_ptr(), float(eps),
                   gx.data_ptr(), _ptr(dweight), _ptr(dbias), _ptr(ws), stream)
    _check(rc, f"tome_{what}")
    return gx, dweight, dbias


def layernorm_backward(gy: torch.Tensor, xs: torch.Tensor, gx_in: Optional[torch.Tensor], weight: torch.Tensor,
                       eps: float, skip_first: bool = False, want_weight: bool = True, want_bias: bool = True):
    """tome_layernorm_backward: the gradient of y = LayerNorm(xs) (and of the residual stream through xs) for the
    stored 16-bit rows xs [..., C] the forward kernels normalised.  gy: gradient of y, xs's shape -- or, skip_first
    (xs [B, N, C]), [B, N-1, C]: every clip's first row has no row in y.  gx_in: optional gradient that reaches xs
    directly, xs's shape.  Returns (gx, dweight, dbias); a gradient that is not wanted is None.  No CPU path."""
    require_device(xs, "layernorm_backward(xs)")
    if xs.dtype not in _HALF:
        raise TomeHipError(f"layernorm_backward: 16-bit tokens only, got {xs.dtype}")
    C = xs.shape[-1]
    if xs.dim() < 2 or C % 8 or C > 1024 or xs.numel() == 0:
        raise TomeHipError(f"layernorm_backward: xs must be [..., C] with C % 8 == 0 and C <= 1024, got {tuple(xs.shape)}")
    if skip_first:
        if xs.dim() != 3 or xs.shape[1] < 2:
            raise TomeHipError("layernorm_backward(skip_first): xs must be [B, N >= 2, C]")
        groups, group_rows = xs.shape[0], xs.shape[1]
        gy_shape = (groups, group_rows - 1, C)
    else:
        groups, group_rows = xs.numel() // C, 1
        gy_shape = tuple(xs.shape)
    return _layernorm_backward_call("layernorm_backward", gy, gy_shape, xs, gx_in, weight, eps, want_weight, want_bias,
                                    (groups, group_rows, int(bool(skip_first))), (groups * group_rows, C))


def merge_ln_backward(plan: MatchPlan, gy: torch.Tensor, gx_out: Optional[torch.Tensor], xs: torch.Tensor,
                      out_div: Optional[torch.Tensor], in_mul: Optional[torch.Tensor], weight: torch.Tensor, eps: float,
                      drop: bool = False, want_weight: bool = True, want_bias: bool = True):
    """tome_merge_ln_backward: the backward of merge_wavg_ln / drop_ln as one launch.  xs [n, T-r, C]: the forward's
    stored x_out; gy its y_out's gradient; gx_out (or None) the gradient that reaches x_out through the residual stream;
    out_div = size_out, in_mul = size or None (both None with drop).  Returns (gx [n, T, C], dweight, dbias); a
    gradient that is not wanted is None.  No CPU path."""
    what = "merge_ln_backward"
    require_device(xs, f"{what}(xs)")
    if xs.dtype not in _HALF:
        raise TomeHipError(f"{what}: 16-bit tokens only, got {xs.dtype}")
    n, T, To = plan.n, plan.T, plan.T - plan.r
    if xs.dim() != 3 or tuple(xs.shape[:2]) != (n, To):
        raise TomeHipError(f"{what}: xs must be [{n}, {To}, C], got {tuple(xs.shape)}")
    C = xs.shape[-1]
    if weight.numel() != C or weight.dtype != xs.dtype or weight.device != xs.device:
        raise TomeHipError(f"{what}: weight must hold {C} values of {xs.dtype} on {xs.device}")
    if drop and (out_div is not None or in_mul is not None):
        raise TomeHipError(f"{what}: drop takes no scales")
    gy = _prep_grad(gy, (n, To, C), xs.dtype, xs.device, f"{what}(gy)")
    if gx_out is not None:
        gx_out = _prep_grad(gx_out, (n, To, C), xs.dtype, xs.device, f"{what}(gx_out)")
    out_div, in_mul, sdtype = _prep_scales(out_div, in_mul, n, T, To, xs.dtype, xs.device, what)
    xs = xs.detach()
    xs = xs if xs.is_contiguous() else xs.contiguous()
    weight = weight.detach().contiguous()
    row_map = plan_row_map(plan)
    L = lib()
    entry = require_symbol(L, "tome_merge_ln_backward")
    gx = torch.empty((n, T, C), dtype=xs.dtype, device=xs.device)
    dweight = torch.empty(C, dtype=xs.dtype, device=xs.device) if want_weight else None
    dbias = torch.empty(C, dtype=xs.dtype, device=xs.device) if want_bias else None
    with _on_device(xs.device):
        stream = _stream(xs.device)
        ws = _sized_workspace(L, "tome_merge_ln_backward_workspace_bytes", (n, T, C), xs.device, stream,
                              what) if want_weight or want_bias else None
        rc = entry(gy.data_ptr(), _ptr(gx_out), xs.data_ptr(), dtype_code(xs, "xs"), _ptr(out_div), _ptr(in_mul),
                   DTYPES[sdtype], n, T, C, plan.r, row_map.data_ptr(), int(plan.distill_token), int(bool(drop)),
                   weight.data_ptr(), float(eps), gx.data_ptr(), _ptr(dweight), _ptr(dbias), _ptr(ws), stream)
    _check(rc, "tome_merge_ln_backward")
    return gx, dweight, dbias


def layernorm_backward_amp(gy: torch.Tensor, xs: torch.Tensor, gx_in: Optional[torch.Tensor], weight: torch.Tensor,
                           eps: float, skip_first: bool = False, want_weight: bool = True, want_bias: bool = True,
                           want_gx16: bool = False):
    """tome_layernorm_backward_amp: layernorm_backward for the rows add_layernorm_amp stored.  gy: 16-bit gradient of y
    (xs's shape; skip_first: [B, N-1, C]); xs, gx_in (optional) and the returned gx of gy's dtype or fp32; weight fp32;
    dweight / dbias fp32.  want_gx16 (fp32 xs only): also gx rounded to gy's dtype, bit-equal to `gx.to(gy.dtype)`.
    Returns (gx, gx16, dweight, dbias); what is not wanted is None.  No CPU path."""
    what = "layernorm_backward_amp"
    require_device(xs, f"{what}(xs)")
    if gy.dtype not in _HALF or xs.dtype not in (gy.dtype, torch.float32):
        raise TomeHipError(f"{what}: a 16-bit gy and xs of its dtype or fp32 required, got {gy.dtype} / {xs.dtype}")
    if want_gx16 and xs.dtype != torch.float32:
        raise TomeHipError(f"{what}: gx16 belongs to an fp32 stream")
    C = xs.shape[-1]
    groups, group_rows = _amp_rows(what, xs, skip_first)
    gy_shape = (groups, group_rows - 1, C) if skip_first else tuple(xs.shape)
    (weight,) = _f32_params(what, C, xs.device, weight)
    gy = _prep_grad(gy, gy_shape, gy.dtype, xs.device, f"{what}(gy)")
    if gx_in is not None:
        gx_in = _prep_grad(gx_in, tuple(xs.shape), xs.dtype, xs.device, f"{what}(gx_in)")
    xs = xs.detach()
    xs = xs if xs.is_contiguous() else xs.contiguous()
    L = lib()
    entry = require_symbol(L, "tome_layernorm_backward_amp")
    gx = torch.empty_like(xs)
    gx16 = torch.empty_like(xs, dtype=gy.dtype) if want_gx16 else None
    dweight = torch.empty(C, dtype=torch.float32, device=xs.device) if want_weight else None
    dbias = torch.empty(C, dtype=torch.float32, device=xs.device) if want_bias else None
    with _on_device(xs.device):
        stream = _stream(xs.device)
        ws = _sized_workspace(L, "tome_layernorm_backward_amp_workspace_bytes", (groups * group_rows, C, DTYPES[xs.dtype]),
                              xs.device, stream, what) if want_weight or want_bias else None
        rc = entry(gy.data_ptr(), DTYPES[gy.dtype], xs.data_ptr(), _ptr(gx_in), DTYPES[xs.dtype], groups, group_rows,
                   int(bool(skip_first)), C, weight.data_ptr(), float(eps), gx.data_ptr(), _ptr(gx16), _ptr(dweight),
                   _ptr(dbias), _ptr(ws), stream)
    _check(rc, "tome_layernorm_backward_amp")
    return gx, gx16, dweight, dbias


def merge_ln_backward_amp(plan: MatchPlan, gy: torch.Tensor, gx_out: Optional[torch.Tensor], xs: torch.Tensor,
                          out_div: Optional[torch.Tensor], in_mul: Optional[torch.Tensor], weight: torch.Tensor,
                          eps: float, drop: bool = False, want_weight: bool = True, want_bias: bool = True,
                          want_gx16: bool = False):
    """tome_merge_ln_backward_amp: the backward of merge_wavg_ln_amp / drop_ln_amp as one launch.  xs [n, T-r, C]: the
    forward's stored x_out, of gy's dtype or fp32; gy the 16-bit gradient of its y_out; gx_out (or None) the gradient that
    reaches x_out through the residual stream, of xs's dtype; out_div = size_out, in_mul = size or None (both None with
    drop); weight fp32.  want_gx16 (fp32 xs only): also gx rounded to gy's dtype, bit-equal to `gx.to(gy.dtype)`.
    Returns (gx [n, T, C] of xs's dtype, gx16, dweight, dbias) with fp32 parameter gradients; what is not wanted is
    None.  No CPU path."""
    what = "merge_ln_backward_amp"
    require_device(xs, f"{what}(xs)")
    if gy.dtype not in _HALF or xs.dtype not in (gy.dtype, torch.float32):
        raise TomeHipError(f"{what}: a 16-bit gy and xs of its dtype or fp32 required, got {gy.dtype} / {xs.dtype}")
    if want_gx16 and xs.dtype != torch.float32:
        raise TomeHipError(f"{what}: gx16 belongs to an fp32 stream")
    n, T, To = plan.n, plan.T, plan.T - plan.r
    if xs.dim() != 3 or tuple(xs.shape[:2]) != (n, To):
        raise TomeHipError(f"{what}: xs must be [{n}, {To}, C], got {tuple(xs.shape)}")
    C = xs.shape[-1]
    (weight,) = _f32_params(what, C, xs.device, weight)
    if drop and (out_div is not None or in_mul is not None):
        raise TomeHipError(f"{what}: drop takes no scales")
    gy = _prep_grad(gy, (n, To, C), gy.dtype, xs.device, f"{what}(gy)")
    if gx_out is not None:
        gx_out = _prep_grad(gx_out, (n, To, C), xs.dtype, xs.device, f"{what}(gx_out)")
    out_div, in_mul, sdtype = _prep_scales(out_div, in_mul, n, T, To, xs.dtype, xs.device, what)
    xs = xs.detach()
    xs = xs if xs.is_contiguous() else xs.contiguous()
    row_map = plan_row_map(plan)
    L = lib()
    entry = require_symbol(L, "tome_merge_ln_backward_amp")
    gx = torch.empty((n, T, C), dtype=xs.dtype, device=xs.device)
    gx16 = torch.empty((n, T, C), dtype=gy.dtype, device=xs.device) if want_gx16 else None
    dweight = torch.empty(C, dtype=torch.float32, device=xs.device) if want_weight else None
    dbias = torch.empty(C, dtype=torch.float32, device=xs.device) if want_bias else None
    with _on_device(xs.device):
        stream = _stream(xs.device)
        ws = _sized_workspace(L, "tome_merge_ln_backward_amp_workspace_bytes", (n, T, C, DTYPES[xs.dtype]), xs.device,
                              stream, what) if want_weight or want_bias else None
        rc = entry(gy.data_ptr(), DTYPES[gy.dtype], _ptr(gx_out), xs.data_ptr(), DTYPES[xs.dtype], _ptr(out_div),
                   _ptr(in_mul), DTYPES[sdtype], n, T, C, plan.r, row_map.data_ptr(), int(plan.distill_token),
                   int(bool(drop)), weight.data_ptr(), float(eps), gx.data_ptr(), _ptr(gx16), _ptr(dweight), _ptr(dbias),
                   _ptr(ws), stream)
    _check(rc, "tome_merge_ln_backward_amp")
    return gx, gx16, dweight, dbias


def layernorm_backward_regrouped(gy: torch.Tensor, xs: torch.Tensor, gx_in: Optional[torch.Tensor], frames: int,
                                 weight: torch.Tensor, eps: float, want_weight: bool = True, want_bias: bool = True):
    """tome_layernorm_backward_regrouped: the backward of add_layernorm_regrouped.  xs [B, 1 + P*F, C]: the x1 that
    call returned (the stored rows it normalised); gy [B*F, 1 + P, C]: the gradient of its regrouped, normalised output;
    gx_in: optional gradient that reaches xs directly, xs's shape.  Returns (gx, dweight, dbias), gx of xs's shape (the
    addend's gradient is gx[:, 1:]); a gradient that is not wanted is None.  No CPU path."""
    require_device(xs, "layernorm_backward_regrouped(xs)")
    if xs.dtype not in _HALF:
        raise TomeHipError(f"layernorm_backward_regrouped: 16-bit tokens only, got {xs.dtype}")
    F = int(frames)
    if xs.dim() != 3 or F < 1 or xs.shape[1] < 1 + F or (xs.shape[1] - 1) % F or xs.shape[0] < 1:
        raise TomeHipError(f"layernorm_backward_regrouped: xs {tuple(xs.shape)} does not hold a class token and {F} "
                           "frames of tokens")
    B, N, C = xs.shape
    P = (N - 1) // F
    if C % 8 or C > 1024:
        raise TomeHipError(f"layernorm_backward_regrouped: C % 8 == 0 and C <= 1024 required, got {C}")
    return _layernorm_backward_call("layernorm_backward_regrouped", gy, (B * F, 1 + P, C), xs, gx_in, weight, eps,
                                    want_weight, want_bias, (B, F, P), (B, F, P, C))


def source_init(plan: MatchPlan, drop: bool = False) -> torch.Tensor:
    """The first layer's source matrix [n, T-r, T] fp32 (merge_source with source=None, merge.py:372-384; `drop`:
    what the drop closure makes of the identity) written straight from the matching's row map -- no [n,T,T]
    identity, no reduction over its zeros."""
    plan_row_map(plan)
    with _on_device(plan.device):
        st = _stream(plan.device)
        out = torch.empty((plan.n, plan.T - plan.r, plan.T), dtype=torch.float32, device=plan.device)
        _check(lib().tome_source_init(plan.n, plan.T, plan.r, int(plan.distill_token), int(bool(drop)),
                                      plan.row_map.data_ptr(), out.data_ptr(), st), "tome_source_init")
    return out


class PartitionPlan:
    """Device-resident result of one partition matching (kth_ / random_bipartite_soft_matching): per group an ordered
    source set A (Na positions) and destination set B (Nb positions), given by the kth rule (`k` > 1) or by the index
    lists `a_idx` [n,Na,1] / `b_idx` [n,Nb,1] (`k` = 0); `dst_idx` (int64 [n,Na,1], the reference's closure variable)
    and the inverted list the merge kernel walks (`offsets` [n,Nb+1], `sources` [n,Na], int32)."""

    __slots__ = ("n", "T", "Na", "Nb", "k", "a_idx", "b_idx", "dst_idx", "offsets", "sources", "device")

    def __init__(self, n, T, Na, Nb, k, a_idx, b_idx, dst_idx, offsets, sources, device):
        self.n, self.T, self.Na, self.Nb, self.k = n, T, Na, Nb, k
        self.a_idx, self.b_idx = a_idx, b_idx
        self.dst_idx, self.offsets, self.sources = dst_idx, offsets, sources
        self.device = device

    @property
    def tokens_out(self) -> int:
        """Rows `unmerge` writes: the kth rule loses the tail past (T // k) * k (merge.py:120), lists cover T."""
        return (self.T // self.k) * self.k if self.k else self.T


def _partition_index(idx: torch.Tensor, n: int, T: int, device, what: str) -> torch.Tensor:
    require_device(idx, what)
    if idx.dim() == 2:
        idx = idx[..., None]
    if idx.dim() != 3 or idx.shape[0] != n or idx.shape[2] != 1 or idx.dtype != torch.int64:
        raise TomeHipError(f"{what}: expected int64 [{n}, rows, 1], got {idx.dtype} {tuple(idx.shape)}")
    if idx.device != device:
        raise TomeHipError(f"{what}: tensor on {idx.device}, metric on {device}")
    return idx if idx.is_contiguous() else idx.contiguous()


def match_partition(metric: torch.Tensor, k: int = 0, a_idx: Optional[torch.Tensor] = None,
                    b_idx: Optional[torch.Tensor] = None) -> PartitionPlan:
    """tome_match_partition on `metric` [n,T,D]: the kth rule (k > 1) or the position lists a_idx / b_idx (k = 0;
    int64 [n,Na,1] / [n,Nb,1], disjoint positions in [0,T) -- the caller's promise, as in the reference)."""
    require_device(metric, "partition matching(metric)")
    if metric.dim() != 3:
        raise TomeHipError(f"metric must be [batch, tokens, channels], got {tuple(metric.shape)}")
    code = dtype_code(metric, "metric")
    n, T, D = metric.shape
    dev = metric.device
    k = int(k)
    if k:
        if k <= 1:
            raise TomeHipError(f"partition matching: k={k} (k > 1 expected)")
        Na, Nb = (T // k) * (k - 1), T // k
        a_idx = b_idx = None
    else:
        if a_idx is None or b_idx is None:
            raise TomeHipError("partition matching: k or both of a_idx / b_idx are needed")
        a_idx = _partition_index(a_idx, n, T, dev, "partition matching(a_idx)")
        b_idx = _partition_index(b_idx, n, T, dev, "partition matching(b_idx)")
        Na, Nb = a_idx.shape[1], b_idx.shape[1]
    if n == 0 or Na <= 0 or Nb <= 0:
        raise TomeHipError(f"partition matching: empty set (n={n}, Na={Na}, Nb={Nb})")
    if metric.stride(2) != 1:
        metric = metric.contiguous()
    L = lib()
    with _on_device(dev):
        st = _stream(dev)
        ws = _workspace(dev, st, L.tome_partition_workspace_bytes(n, Na, Nb, D))
        dst = torch.empty((n, Na, 1), dtype=torch.int64, device=dev)
        offsets = torch.empty((n, Nb + 1), dtype=torch.int32, device=dev)
        sources = torch.empty((n, Na), dtype=torch.int32, device=dev)
        rc = L.tome_match_partition(metric.data_ptr(), code, n, T, D, metric.stride(0), metric.stride(1), k,
                                    _ptr(a_idx), _ptr(b_idx), Na, Nb, dst.data_ptr(), offsets.data_ptr(),
                                    sources.data_ptr(), ws.data_ptr(), ws.numel(), st)
    _check(rc, "tome_match_partition")
    return PartitionPlan(n, T, Na, Nb, k, a_idx, b_idx, dst, offsets, sources, dev)


def merge_partition(plan: PartitionPlan, x: torch.Tensor, mode: str) -> torch.Tensor:
    if mode not in MODES:
        raise TomeHipError(f"merge: unknown reduce mode {mode!r}")
    x = _prep_x(plan, x, "merge(x)", plan.T)
    n, T, C = x.shape
    out = torch.empty((n, plan.Nb, C), dtype=x.dtype, device=x.device)
    with _on_device(x.device):
        rc = lib().tome_merge_partition(x.data_ptr(), dtype_code(x, "x"), n, T, C, plan.k, _ptr(plan.a_idx),
                                        _ptr(plan.b_idx), plan.Na, plan.Nb, plan.offsets.data_ptr(),
                                        plan.sources.data_ptr(), MODES[mode], out.data_ptr(), _stream(x.device))
    _check(rc, "tome_merge_partition")
    return out


def merge_wavg_partition(plan: PartitionPlan, x: torch.Tensor, size: Optional[torch.Tensor], log_size: bool = False):
    x = _prep_x(plan, x, "merge_wavg(x)", plan.T)
    n, T, C = x.shape
    xcode = dtype_code(x, "x")
    size, sdtype = _prep_size(size, n, T, x)
    x_out = torch.empty((n, plan.Nb, C), dtype=x.dtype, device=x.device)
    s_out = torch.empty((n, plan.Nb, 1), dtype=sdtype, device=x.device)
    log = _log_size_like(s_out, log_size)
    with _on_device(x.device):
        rc = lib().tome_merge_wavg_partition(x.data_ptr(), xcode, _ptr(size), DTYPES[sdtype], n, T, C, plan.k,
                                             _ptr(plan.a_idx), _ptr(plan.b_idx), plan.Na, plan.Nb,
                                             plan.offsets.data_ptr(), plan.sources.data_ptr(), x_out.data_ptr(),
                                             s_out.data_ptr(), _ptr(log), _stream(x.device))
    _check(rc, "tome_merge_wavg_partition")
    return x_out, s_out


def unmerge_partition(plan: PartitionPlan, x: torch.Tensor) -> torch.Tensor:
    x = _prep_x(plan, x, "unmerge(x)", plan.Nb)
    n, _, C = x.shape
    out = torch.empty((n, plan.tokens_out, C), dtype=x.dtype, device=x.device)
    with _on_device(x.device):
        rc = lib().tome_unmerge_partition(x.data_ptr(), dtype_code(x, "x"), n, plan.T, C, plan.k, _ptr(plan.a_idx),
                                          _ptr(plan.b_idx), plan.Na, plan.Nb, plan.dst_idx.data_ptr(),
                                          out.data_ptr(), _stream(x.device))
    _check(rc, "tome_unmerge_partition")
    return out
