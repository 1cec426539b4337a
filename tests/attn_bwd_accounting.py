"""Inputs whose softmax is known, so that the bound of attn_bwd_oracle.py becomes tight enough to count every key, query
and head in dq and dk (k_attn_bwd_dq / k_attn_bwd_dkv, csrc/tome_attn_bwd.h, and their segmented form).  No test
functions; CPU-importable (torch only).  The reference stays attn_bwd_oracle.reference (fp64 autograd), the bound stays
attn_bwd_oracle.bounds, both unchanged.

On random heads that bound is dominated by the rounding of q~ (rho = expm1(E + Ebar)): a correct kernel sits at ~0.01 of
the dq / dk bounds and a missing key tile stays inside them.  If every logit is exactly the bias -- q = 0 or k = 0 -- then
E = 0 and rho collapses to the fp32 term eta; what is left are the 16-bit roundings of the P / dS operands, of the stored O
and of the outputs.  scale = 0.125 throughout; channels are rotated per batch and head by 7b + 3h (attn_oracle.channel_of)
and by 5 more per segment, so a read from another head's or segment's slice lands in the wrong channels.

  common    v[b, h, j] = a_j e_0 with a_j = +1 / -1 by the parity of the key's un-rotated channel index (j for the "mod"
            encoding, j // 32 for "block"); dout[b, i, h] = e_0 + e_{1 + c(i)}, c(i) = chan(i) mod 63.  Hence dP_ij = a_j,
            delta_i = sum_j P_ij a_j, dS_ij = P_ij (a_j - delta_i), and dv_j = sum_i P_ij dout_i counts every query.
  family K  q = 0, k[b, h, j] = e_chan(j): dq_i[c] = scale sum_{j in c} dS_ij counts every key; dk is exactly 0.
  family Q  k = 0, q[b, h, i] = e_chan(i): dk_j[c] = scale sum_{i in c} dS_ij counts every query; dq is exactly 0.
  bias      "none", "bias" (integer sizes 1..3 as log_bias) or "skip" (TimeSformer's form, N == Nk >= 2).
  encoding  "mod": chan = (row + rot) mod 64, neighbouring rows in different channels -- a single missing or doubled row;
            "block": chan = (row // 32 + rot) mod 64 -- a missing lane half (key / key + 32 in dq), 32-query block (the qb
            loop of dkv), 64-row tile or 128-row workgroup block.

`check` is attn_bwd_oracle.check with one rule added: where the bound is 0 (bf16 has no absolute term, so every
structurally zero element: all of dk in family K, all of dq in family Q) the value must be exactly 0.
`omission_sensitivity` says, from the fp64 reference alone, by how many bounds the damaged gradient moves when a unit of
rows is left out of (or counted twice in) one row's sum -- the figure that has to exceed 1 for the construction to see it.
`emulate` adds the slips of this construction to those of attn_bwd_oracle.emulate.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

import attn_bwd_oracle as ao
import segment_attn_bwd_oracle as so

SCALE = 0.125
KINDS = ("K", "Q")
ENCODINGS = ("mod", "block")
BIASES = ("none", "bias", "skip")


# ---- the shapes the GPU file runs and the CPU file proves sharp (test_attention_backward_accounting_gpu.py,
# test_attn_bwd_accounting_cpu.py) -------------------------------------------------------------------------------------
PLAIN_BH = (2, 3)
SQUARE = [(n, n) for n in (1, 31, 32, 33, 64, 65, 127, 128, 129, 193, 257, 449)]
WIDE = [(1, 2), (1, 65), (1, 217), (33, 449), (33, 700)]
TALL = [(2, 1), (130, 1), (129, 32), (449, 33), (700, 65)]
PLAIN_SHAPES = SQUARE + WIDE + TALL
HEADS = [(3, 3), (1, 17), (2, 12)]                     # B*H = 9, 17, 24: the item map's second and third round of 8
HEAD_SHAPES = [(129, 65), (65, 129)]
TARGET_SHAPES = [(33, 33), (129, 129), (33, 449), (449, 33)]
STRIDE_SHAPES = [(65, 65), (129, 129), (33, 449)]
SEGMENTS = [(2, 3, 65, 33, 2), (1, 3, 130, 65, 2), (2, 12, 129, 64, 3), (1, 1, 128, 1, 8), (1, 3, 257, 129, 3)]  # B H N P nseg
SEGMENTS_QKV = [(1, 3, 195, 65, 3)]


def biases_for(N: int, Nk: int):
    """The bias forms a shape admits: the skip form needs N == Nk >= 2."""
    return ("none", "bias") + (("skip",) if N == Nk and Nk >= 2 else ())


def _base(n: int, enc: str, device) -> torch.Tensor:
    j = torch.arange(n, device=device)
    if enc == "mod":
        return j
    if enc == "block":
        return j // 32
    raise ValueError(enc)


def rotation(B: int, H: int, device="cpu", extra: int = 0) -> torch.Tensor:
    """7b + 3h (+ extra): int64 [B, H]"""
    return 7 * torch.arange(B, device=device).view(B, 1) + 3 * torch.arange(H, device=device).view(1, H) + extra


def channel_of(B: int, H: int, n: int, enc: str, device="cpu", extra: int = 0) -> torch.Tensor:
    """Channel of row j of (batch b, head h): (base(j) + 7b + 3h + extra) mod 64, int64 [B, H, n]."""
    return (_base(n, enc, device).view(1, 1, n) + rotation(B, H, device, extra).view(B, H, 1)) % 64


def sign_of(n: int, enc: str, device="cpu") -> torch.Tensor:
    """a_j = +1 / -1 by the parity of the un-rotated channel index: float32 [n]"""
    return (1 - 2 * (_base(n, enc, device) % 2)).float()


def _fill_common(v, g, enc, extra=0):
    """v = a_j e_0 and dout = e_0 + e_{1 + c(i)} into zeroed head views v [B, H, Nk, 64] and g [B, H, N, 64], in place."""
    B, H, N, _ = g.shape
    v[..., 0] = sign_of(v.shape[2], enc, v.device).to(v.dtype)
    g[..., 0] = 1.0
    g.scatter_(-1, (1 + channel_of(B, H, N, enc, g.device, extra) % 63).unsqueeze(-1), 1.0)


def _fill_onehot(t, enc, extra=0):
    """t[b, h, j] = e_chan(j) into a zeroed head view [B, H, n, 64] (any strides), in place."""
    B, H, n, _ = t.shape
    t.scatter_(-1, channel_of(B, H, n, enc, t.device, extra).unsqueeze(-1), 1.0)


def _fill(kind, q, k, v, g, enc):
    if kind not in KINDS:
        raise ValueError(kind)
    _fill_onehot(k if kind == "K" else q, enc)
    _fill_common(v, g, enc)


def _sizes(B, n, seed):
    return torch.randint(1, 4, (B, n), generator=torch.Generator().manual_seed(seed)).float().log()


def make_family(kind: str, B: int, H: int, N: int, Nk: int, dtype, bias: str = "none", enc: str = "mod", seed: int = 0,
                device="cpu") -> Tuple[ao.Inputs, Optional[ao.Inputs]]:
    """(separate, qkv): the family as attn_bwd_oracle.Inputs in the "separate" layout and, for N == Nk, the same values
    as the three slices of one [B, N, 3, H, 64] buffer (else None)."""
    assert bias in BIASES and (bias != "skip" or (N == Nk and Nk >= 2)), (bias, N, Nk)
    skip = bias == "skip"
    lb = None if bias == "none" else _sizes(B, Nk - int(skip), seed).to(device)
    dout = torch.zeros(B, N, H * 64, dtype=dtype, device=device)
    g = dout.view(B, N, H, 64).permute(0, 2, 1, 3)
    q = torch.zeros(B, H, N, 64, dtype=dtype, device=device)
    k = torch.zeros(B, H, Nk, 64, dtype=dtype, device=device)
    v = torch.zeros(B, H, Nk, 64, dtype=dtype, device=device)
    _fill(kind, q, k, v, g, enc)
    sep = ao.Inputs(q, k, v, dout, lb, skip, SCALE, None)
    if N != Nk:
        return sep, None
    return sep, make_family_qkv(kind, B, H, N, dtype, bias, enc, seed, device)


def make_family_qkv(kind, B, H, N, dtype, bias="none", enc="mod", seed=0, device="cpu") -> ao.Inputs:
    """The "qkv" layout alone, filled in place (no second copy of the heads: the buffer may exceed 2^31 elements)."""
    skip = bias == "skip"
    lb = None if bias == "none" else _sizes(B, N - int(skip), seed).to(device)
    qkv = torch.zeros(B, N, 3, H, 64, dtype=dtype, device=device)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    dout = torch.zeros(B, N, H * 64, dtype=dtype, device=device)
    _fill(kind, q, k, v, dout.view(B, N, H, 64).permute(0, 2, 1, 3), enc)
    return ao.Inputs(q, k, v, dout, lb, skip, SCALE, qkv)


def make_segment_family(kind: str, B: int, H: int, N: int, P: int, nseg: int, dtype, bias: str = "none", enc: str = "mod",
                        seed: int = 0, layout: str = "separate", device="cpu") -> so.Inputs:
    """The segmented twin: every segment carries the family over its own P keys, its rotation increased by 5 s (keys of
    family K and every segment's dy; the queries of family Q are common to the segments and keep the plain rotation).
    layout "qkv": rows 1.. of one [B, 1 + N, 3, H, 64] buffer (N == nseg * P) behind a class-token row of 0.5."""
    assert bias in ("none", "bias"), bias
    K = nseg * P
    lb = None if bias == "none" else _sizes(B, K, seed).to(device)
    if layout == "qkv":
        assert N == K
        qkv = torch.zeros(B, 1 + N, 3, H, 64, dtype=dtype, device=device)
        qkv[:, 0] = 0.5
        q, k, v = (qkv[:, 1:, i].permute(0, 2, 1, 3) for i in range(3))
    else:
        qkv = None
        q = torch.zeros(B, N, H, 64, dtype=dtype, device=device).permute(0, 2, 1, 3)
        k = torch.zeros(B, K, H, 64, dtype=dtype, device=device).permute(0, 2, 1, 3)
        v = torch.zeros(B, K, H, 64, dtype=dtype, device=device).permute(0, 2, 1, 3)
    dy = torch.zeros(B, N, nseg, H * 64, dtype=dtype, device=device)
    for s in range(nseg):
        sl = slice(s * P, (s + 1) * P)
        _fill_common(v[:, :, sl], dy[:, :, s].view(B, N, H, 64).permute(0, 2, 1, 3), enc, extra=5 * s)
        if kind == "K":
            _fill_onehot(k[:, :, sl], enc, extra=5 * s)
    if kind == "Q":
        _fill_onehot(q, enc)
    return so.Inputs(q, k, v, dy, lb, nseg, SCALE, qkv)


# ---- the check ---------------------------------------------------------------------------------------------------------

def ratios(x: torch.Tensor, ref: torch.Tensor, bnd: torch.Tensor) -> torch.Tensor:
    """|x - ref| / bound per element; where the bound is 0 the value must be exactly 0 (ratio 0, else inf); a
    non-finite value counts as inf."""
    err = (x - ref).abs()
    zero = bnd == 0
    r = torch.where(zero, torch.where(x == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))),
                    err / torch.where(zero, torch.ones_like(bnd), bnd))
    return torch.where(torch.isfinite(x), r, torch.full_like(r, float("inf")))


def worst(got: dict, ref: dict, bnd: dict) -> dict:
    res = {}
    for n in ("dq", "dk", "dv"):
        x = got[n].detach().cpu().double()
        assert x.shape == ref[n].shape, (n, x.shape, ref[n].shape)
        res[n] = float(ratios(x, ref[n], bnd[n]).max())
    return res


def check(label: str, got: dict, ref: dict, bnd: dict) -> dict:
    """attn_bwd_oracle.check with the zero-bound rule: every element inside its bound, and exactly 0 where the bound is 0.
    Prints the worst and the RMS of error / bound (the RMS over the elements whose bound is not 0)."""
    w, rms = {}, {}
    for n in ("dq", "dk", "dv"):
        x = got[n].detach().cpu().double()
        assert x.shape == ref[n].shape, (n, x.shape, ref[n].shape)
        r = ratios(x, ref[n], bnd[n])
        w[n] = float(r.max())
        live = r[bnd[n] != 0]
        rms[n] = float(live.square().mean().sqrt()) if live.numel() else 0.0
    print(f"{label}: worst error / bound  dq {w['dq']:.3f}  dk {w['dk']:.3f}  dv {w['dv']:.3f}"
          f"   (rms  dq {rms['dq']:.4f}  dk {rms['dk']:.4f}  dv {rms['dv']:.4f})")
    for n, r in w.items():
        assert r <= 1.0, f"{label}: {n} is {r:.3f}x its bound somewhere (inf: not 0 where the bound is 0, or not finite)"
    return w


# ---- what an omission would do to the reference ------------------------------------------------------------------------

GRANULARITIES = ("row", 32, 64, 128)


def _units(n: int, granularity):
    if granularity == "row":
        return None
    return [(lo, min(lo + granularity, n)) for lo in range(0, n, granularity)]


def _min_of_max(W: torch.Tensor, X: torch.Tensor, bnd: torch.Tensor, factor: float, granularity) -> float:
    """W [.., R, M]: the weight of term m in row r's sum; X [.., M, 64]: the term's vector; bnd [.., R, 64].  The sum of
    row r is factor * sum_m W_rm X_m.  For every (row r, unit of terms U): change = factor * sum_{m in U} W_rm X_m, the
    largest |change| / bound over the 64 elements (0 / 0 ignored, x / 0 = inf); returns the smallest over (r, U)."""
    def rat(change, b):
        r = change.abs() / torch.where(b == 0, torch.ones_like(b), b)
        r = torch.where((b == 0) & (change != 0), torch.full_like(r, float("inf")), r)
        return r

    units = _units(W.shape[-1], granularity)
    if units is None:
        best = torch.zeros_like(W)
        for c in range(X.shape[-1]):  # (a [.., R, M, 64] tensor would be 64 x the softmax; one channel at a time)
            change = factor * W * X[..., c].unsqueeze(-2)
            best = torch.maximum(best, rat(change, bnd[..., c].unsqueeze(-1)))
        return float(best.min())
    res = float("inf")
    for lo, hi in units:
        change = factor * (W[..., lo:hi] @ X[..., lo:hi, :])
        res = min(res, float(rat(change, bnd).amax(-1).min()))
    return res


def omission_sensitivity(ref: dict, bnd: dict, kind: str, granularity="row") -> dict:
    """By how many bounds the reference itself moves when a unit of rows goes missing from one row's sum: the smallest,
    over every (row, omitted unit), of the largest |change| / bound over the elements of the gradient the omission
    touches.  Units: a single key or query ("row"), or an aligned block of 32, 64 or 128 rows.  Covers the gradient the
    family counts in -- dq over keys (family K), dk over queries (family Q) -- and dv over queries (both); "row" also
    returns the doubling variant (the unit added once more instead of left out).  Elements where both the change and
    the bound are 0 are ignored.  fp64, from `ref` alone."""
    P, g, v, scale = ref["P"], ref["g"], ref["v"], ref["scale"]
    dS = P * (g @ v.transpose(-2, -1) - (g * ref["out"]).sum(-1, keepdim=True))
    res = {}
    if kind == "K":    # dq_i = scale sum_j dS_ij k_j: keys left out of row i
        res["dq"] = _min_of_max(dS, ref["k"], bnd["dq"], scale, granularity)
    elif kind == "Q":  # dk_j = scale sum_i dS_ij q_i: queries left out of key j
        res["dk"] = _min_of_max(dS.transpose(-2, -1), ref["q"], bnd["dk"], scale, granularity)
    else:
        raise ValueError(kind)
    res["dv"] = _min_of_max(P.transpose(-2, -1), g, bnd["dv"], 1.0, granularity)  # dv_j = sum_i P_ij dout_i
    if granularity == "row":  # counted twice: the same terms with the other sign
        for n in list(res):
            res[n + "_doubled"] = res[n]
        if kind == "K":
            res["dq_doubled"] = _min_of_max(-dS, ref["k"], bnd["dq"], scale, granularity)
        else:
            res["dk_doubled"] = _min_of_max(-dS.transpose(-2, -1), ref["q"], bnd["dk"], scale, granularity)
        res["dv_doubled"] = _min_of_max(-P.transpose(-2, -1), g, bnd["dv"], 1.0, granularity)
    return res


# ---- the slips of this construction ------------------------------------------------------------------------------------

SLIPS = ("last_key_tile_dropped", "key_half_dropped", "query_block_dropped", "bias_off_by_one", "head_wrapped",
         "rows_past_end_added")
KEY_SIDE = ("last_key_tile_dropped", "key_half_dropped", "bias_off_by_one", "head_wrapped")         # damage dq (family K)
QUERY_SIDE = ("query_block_dropped", "bias_off_by_one", "head_wrapped", "rows_past_end_added")      # damage dk (family Q)


def emulate(inp: ao.Inputs, slip: Optional[str] = None) -> dict:
    """attn_bwd_oracle.emulate (its arithmetic, line for line) with the slips of SLIPS; any other slip, and none, is
    attn_bwd_oracle.emulate itself.
      last_key_tile_dropped   the last 64-key tile is missing from sweep 2 of dq (every row)
      key_half_dropped        keys 32 .. 63 of tile 0 (the upper lane half's accumulator block) missing from dq
      query_block_dropped     queries 32 .. 63 of tile 0 (block qb = 1) missing from dk and dv
      bias_off_by_one         the plain bias read at j - 1 (key 0 reads its own)
      head_wrapped            item bh >= 8 computed from the data of bh - 8 (the second round of the item map)
      rows_past_end_added     attn_bwd_oracle's "stale_rows": rows past the end repeat row N - 1 and are added"""
    if slip == "rows_past_end_added":
        return ao.emulate(inp, slip="stale_rows")
    if slip not in SLIPS:
        return ao.emulate(inp, slip=slip)
    dt = inp.q.dtype
    q, k, v = inp.q.cpu(), inp.k.cpu(), inp.v.cpu()
    B, H, N, D = q.shape
    Nk = k.shape[2]
    if slip == "head_wrapped":
        got = ao.emulate(inp)
        for n in got:
            flat = got[n].reshape(B * H, *got[n].shape[2:])
            flat = torch.cat([flat[:8], flat[:-8]], 0) if B * H > 8 else flat
            got[n] = flat.reshape(got[n].shape)
        return got
    g = inp.dout.cpu().double().view(B, N, H, D).permute(0, 2, 1, 3)
    sl = torch.tensor(inp.scale, dtype=torch.float32) * torch.tensor(ao.LOG2E, dtype=torch.float32)
    qt = (q.float() * sl).to(dt).double()
    beta = ao.bias_matrix(inp.log_bias, inp.skip, N, Nk) * ao.LOG2E

    def softmax2(s):
        m = s.amax(-1, keepdim=True)
        return torch.exp2(s - (m + torch.log2(torch.exp2(s - m).sum(-1, keepdim=True))))

    s = qt @ k.double().transpose(-2, -1)
    o16 = ao._r16(ao._r16(softmax2(s + beta), dt) @ v.double(), dt)   # the forward's stored output: its bias is right
    if slip == "bias_off_by_one" and inp.log_bias is not None and not inp.skip:
        beta = torch.cat([beta[..., :1], beta[..., :-1]], -1)
    P = softmax2(s + beta)
    delta = (g * o16).sum(-1, keepdim=True)
    dS = P * (g @ v.double().transpose(-2, -1) - delta)
    P16, dS16 = ao._r16(P, dt), ao._r16(dS, dt)
    keys, queries = torch.ones(Nk, dtype=torch.float64), torch.ones(N, 1, dtype=torch.float64)
    if slip == "last_key_tile_dropped":
        keys[64 * ((Nk - 1) // 64):] = 0
    elif slip == "key_half_dropped":
        keys[32:64] = 0
    elif slip == "query_block_dropped":
        queries[32:64] = 0
    dv = (P16 * queries).transpose(-2, -1) @ g
    dk = inp.scale * ((dS16 * queries).transpose(-2, -1) @ q.double())
    dq = inp.scale * ((dS16 * keys) @ k.double())
    return dict(dq=ao._r16(dq, dt), dk=ao._r16(dk, dt), dv=ao._r16(dv, dt))
