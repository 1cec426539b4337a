"""Exact expectations for the attention kernels (tome_prop_attention / tome_prop_attention_segments).

The checks in the parity tests compare with an fp32 softmax at an absolute tolerance; at 1568 keys a flat row gives
every key a weight of ~6e-4, so a key counted twice, dropped, or biased with its neighbour's size passes them.  The
helpers here build inputs whose correct output is known exactly or within a bound derived from the kernels' own
rounding, small enough that a single key going wrong exceeds it:

  * counting: q = 0 makes every logit 0 (or the same constant bias), exp2(0) = 1, and a one-hot v (`onehot_values`)
    turns the output into  count of keys of channel c / Nk  -- `check_counts` recovers the counts exactly;
  * weighted: fp64 weights from the inputs the kernel multiplies (`weighted_reference`), a one-hot v, so every output
    channel is the weight mass of its keys, and `weighted_bound` is the kernels' rounding error of that mass.

CPU-importable (torch only, no GPU at import); the functions work on tensors of any device.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

LOG2E = 1.4426950408889634
RES_ROWS = 224   # tome_attn_resident.h: keys resident per workgroup
ATT_BN = 64      # tome_attn.h: keys per tile

# launch forms and the measurement switches that force them (read per call by the dispatcher)
FORMS = {
    "resident": {},
    "wave4": {"TOME_ATTN_RESIDENT": "0", "TOME_ATTN_WAVES": "4"},
    "wave8": {"TOME_ATTN_RESIDENT": "0", "TOME_ATTN_WAVES": "8", "TOME_ATTN_STREAM": "0"},
    "stream": {"TOME_ATTN_RESIDENT": "0", "TOME_ATTN_WAVES": "8", "TOME_ATTN_STREAM": "1"},
    "pair": {"TOME_ATTN_RESIDENT": "0", "TOME_ATTN_WAVES": "8", "TOME_ATTN_STREAM": "2"},
}
FORM_KERNEL = {"resident": "k_resident_attention", "wave4": "k_prop_attention<.., 4, ..>",
               "wave8": "k_prop_attention<.., 8, ..>", "stream": "k_prop_attention_stream<.., PAIR = false>",
               "pair": "k_prop_attention_stream<.., PAIR = true>"}
ATT_LIMIT_LOG2 = {torch.bfloat16: 60.0, torch.float16: 15.0}  # log2 of AttLimit (tome_attn_tile.h): the overflow guard


def unit_roundoff(dtype) -> float:
    """u of the 16-bit format: half an ulp of 1 (bf16: 8 significant bits, fp16: 11)."""
    if dtype == torch.bfloat16:
        return 2.0 ** -8
    if dtype == torch.float16:
        return 2.0 ** -11
    raise ValueError(f"16-bit format expected, got {dtype}")


def expected_form(N: int, Nk: int, items: int, env: Optional[dict] = None, off32: bool = True,
                  sn_ok: bool = True, cus: int = 256) -> str:
    """Which launch form attn_form and prop_attention_impl (csrc/tome_kernels.hip) give N queries against Nk keys per
    item, items = B * H * nseg, under the switches in `env`.  off32: the resident kernel's 32-bit token offsets fit (N
    and Nk times the token strides < 2^31); sn_ok: every token stride < 2^22 (the stream kernel's 32-bit tile offsets).
    cus: the device's compute units -- the persistent kernel runs as two 128-register workgroups per CU ("pair") when
    TOME_ATTN_STREAM=2 says so or, with that switch unset, when the launch has more items (query blocks of 256 rows,
    the slices rounded up to a multiple of 8) than CUs (rounded down to one); TOME_ATTN_STREAM=1 keeps one per CU."""
    env = env or {}
    res = env.get("TOME_ATTN_RESIDENT", "")
    if Nk <= RES_ROWS and off32 and not res.startswith("0"):
        return "resident"
    w = env.get("TOME_ATTN_WAVES", "")
    waves_env = int(w) if w in ("4", "8") else 0
    waves = waves_env or (8 if N > 128 and items * ((N + 255) // 256) >= 1024 else 4)
    se = env.get("TOME_ATTN_STREAM", "")
    if Nk > ATT_BN and sn_ok and not se.startswith("0") and (waves == 8 or (not waves_env and N > 128)):
        if se.startswith("2"):
            return "pair"
        if se.startswith("1"):
            return "stream"
        return "pair" if ((items + 7) // 8 * 8) * ((N + 255) // 256) > cus // 8 * 8 else "stream"
    return "wave8" if waves == 8 else "wave4"


# ---- one-hot values and counting --------------------------------------------------------------------------------

def channel_of(B: int, H: int, Nk: int, enc: str, device="cpu") -> torch.Tensor:
    """Channel of key j of (batch b, head h): (j + 7b + 3h) mod 64 ("mod": neighbouring keys in different channels)
    or (j // 64 + 7b + 3h) mod 64 ("tile": one channel per 64-key tile).  The rotation by b and h makes a read from
    another batch's or head's slice land in the wrong channels.  -> int64 [B, H, Nk]"""
    j = torch.arange(Nk, device=device)
    if enc == "mod":
        base = j
    elif enc == "tile":
        base = j // 64
    else:
        raise ValueError(enc)
    rot = 7 * torch.arange(B, device=device).view(B, 1, 1) + 3 * torch.arange(H, device=device).view(1, H, 1)
    return (base.view(1, 1, Nk) + rot) % 64


def onehot_values(B: int, H: int, Nk: int, enc: str, dtype, device="cpu",
                  gain: Optional[torch.Tensor] = None) -> torch.Tensor:
    """v[b, h, j] = e_c, c = channel_of(...)[b, h, j] -- or gain[j] * e_c (gain [Nk]: powers of two that `dtype`
    holds exactly, see weighted_reference).  -> [B, H, Nk, 64] of `dtype`"""
    chan = channel_of(B, H, Nk, enc, device)
    v = torch.zeros(B, H, Nk, 64, dtype=dtype, device=device)
    if gain is None:
        v.scatter_(-1, chan.unsqueeze(-1), 1.0)
    else:
        g16 = gain.to(device=device, dtype=dtype)
        assert gain.shape == (Nk,) and torch.equal(g16.double().cpu(), gain.double().cpu()), "gain not exact in dtype"
        v.scatter_(-1, chan.unsqueeze(-1), g16.view(1, 1, Nk, 1).expand(B, H, Nk, 1))
    return v


def expected_counts(B: int, H: int, Nk: int, enc: str, nseg: int = 1, device="cpu") -> torch.Tensor:
    """Keys of each channel in the key range a query sees: all Nk keys (nseg = 1) or, for the segmented form, the P =
    Nk / nseg keys of each segment.  The count does not depend on the query.  -> float64 [B, 1, H, 64] (nseg = 1) or
    [B, 1, nseg, H, 64]: broadcastable against the outputs viewed as [B, N, H, 64] / [B, N, nseg, H, 64]."""
    assert Nk % nseg == 0
    P = Nk // nseg
    chan = channel_of(B, H, Nk, enc, device).view(B, H, nseg, P)
    cnt = torch.zeros(B, H, nseg, 64, dtype=torch.float64, device=device)
    cnt.scatter_add_(-1, chan, torch.ones_like(chan, dtype=torch.float64))
    cnt = cnt.permute(0, 2, 1, 3).unsqueeze(1)  # [B, 1, nseg, H, 64]
    return cnt[:, :, 0] if nseg == 1 else cnt


def _ulp16(x: torch.Tensor, dtype) -> torch.Tensor:
    """One ulp of the 16-bit format at |x| (0 at x = 0; fp16 below 2^-14: the subnormal spacing 2^-24)."""
    mant = 7 if dtype == torch.bfloat16 else 10
    ax = x.abs()
    e = torch.floor(torch.log2(torch.where(ax > 0, ax, torch.ones_like(ax))))
    if dtype == torch.float16:
        e = torch.clamp(e, min=-14.0)
    return torch.where(ax > 0, torch.exp2(e - mant), torch.zeros_like(ax))


def check_counts(out: torch.Tensor, counts: torch.Tensor, nk: int, what: str = "") -> None:
    """out (16-bit, viewed so that it broadcasts with `counts`) must be count / nk per channel: round(out * nk) equal
    to the count EXACTLY, and |out - count / nk| at most one ulp of the 16-bit format.

    Why exact: with q = 0 every weight is exp2(0) = 1, the row sum is nk exactly in fp32 (nk < 2^24) and O_c = count,
    so the kernel returns round16(count * (1 / nk)) -- the reciprocal from 1.0f / l (0.5 ulp of fp32) or v_rcp_f32
    (1 ulp), then one rounding to 16 bits (relative error <= u; u = 2^-8 for bf16, 2^-11 for fp16).  Hence
    |out * nk - count| <= count * (u + 2^-22) < 1/2 as long as count < 2^7 (bf16) / 2^10 (fp16): recovery is exact in
    that range, which is asserted here so that a test cannot pass outside it.  The one-ulp condition is what both
    reciprocals allow; a fixed bit pattern is not demanded."""
    dt = out.dtype
    lim = 2 ** 7 if dt == torch.bfloat16 else 2 ** 10
    assert float(counts.max()) < lim, f"counts up to {float(counts.max())}: recovery is exact only below {lim}"
    o = out.double()
    finite = torch.isfinite(o)
    assert bool(finite.all()), f"{what}: {int((~finite).sum())} non-finite outputs"
    rec = torch.round(o * nk)
    bad = rec != counts
    if bool(bad.any()):
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} channels with a wrong key count, first at {idx}: "
                             f"recovered {float(rec[tuple(idx)])}, expected {float(counts.expand_as(rec)[tuple(idx)])}")
    want = counts / nk
    err = (o - want).abs() - _ulp16(want, dt)
    assert float(err.max()) <= 0.0, f"{what}: counts right but an output is more than one ulp from count / nk"


# ---- weighted accounting ----------------------------------------------------------------------------------------

class Reference(NamedTuple):
    out: torch.Tensor      # float64 [B, N, H, 64] (nseg = 1) or [B, N, nseg, H, 64]: weight mass of each channel
    eta: torch.Tensor      # float64, broadcastable against out: relative error besides the 2u of the roundings
    weights: torch.Tensor  # float64 [B, H, N, nseg, P]: unnormalised weights (row maximum 1)
    chan: torch.Tensor     # int64 [B, H, nseg, P]: channel of every key
    nk: int                # keys per softmax (P)


def kernel_q(q: torch.Tensor, scale: float) -> torch.Tensor:
    """What the kernels multiply the keys with: q * (scale * log2 e), both factors in fp32, rounded once to q's
    16-bit format (att_scaled in tome_attn_tile.h, called by every attention kernel).  This rounding is
    part of the kernels' definition of the logits -- the prescaled q of any fused attention -- not an error to bound:
    its effect on a logit, ~u * |q.k| * scale, would exceed 2u of a weight on rows with large logits."""
    sl = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    return (q.float() * sl.to(q.device)).to(q.dtype)


def log2_bias(log_bias: Optional[torch.Tensor], skip: bool, N: int, Nk: int, device="cpu") -> torch.Tensor:
    """The bias of every (query, key) pair in log2 units, float64 [B or 1, 1, N, Nk]: log_bias[b, j] * log2 e on key j
    for every query, or TimeSformer's skip form (timesformer.py:73-74): query 0 and key 0 unbiased, log_bias[b, j - 1]
    on key j."""
    if log_bias is None:
        return torch.zeros(1, 1, N, Nk, dtype=torch.float64, device=device)
    lb = log_bias.double() * LOG2E
    beta = torch.zeros(lb.shape[0], 1, N, Nk, dtype=torch.float64, device=device)
    if skip:
        assert N == Nk and lb.shape[1] == Nk - 1
        beta[:, :, 1:, 1:] = lb[:, None, None, :]
    else:
        assert lb.shape[1] == Nk
        beta[:, :, :, :] = lb[:, None, None, :]
    return beta


def weighted_reference(q: torch.Tensor, k: torch.Tensor, log_bias: Optional[torch.Tensor], skip: bool, scale: float,
                       v_enc: str, nseg: int = 1, beta: Optional[torch.Tensor] = None,
                       gain: Optional[torch.Tensor] = None) -> Reference:
    """fp64 attention of q [B, H, N, 64] against k [B, H, nseg * P, 64] with one-hot values of encoding `v_enc`: the
    output channel c of a row is the weight mass of the keys of channel c over the row's total.  Logits in log2
    units from the exact 16-bit Q~ (kernel_q) and k, plus log_bias * log2 e from the exact fp32 log_bias
    ([B, nseg * P], or [B, Nk - 1] in the skip form) -- per key, or TimeSformer's skip form: key 0 and query 0 carry no
    bias, log_bias[j - 1] belongs to key j (_attn_reference in test_hip_parity.py).  Segments: a softmax per segment.

    eta: what the kernels' arithmetic adds beyond the two 16-bit roundings of weighted_bound, per row:
      * 2^-16: fp32 sums of the scores (64 products), of the row sum and the PV products, v_exp_f32 and the reciprocal
        (each a few 2^-24 relative; a realistic budget, not a worst case over all summation orders);
      * the resident and stream kernels feed log2 e * log(size) and the resident kernel also -m_ref through the matrix
        pipe as two 16-bit terms hi + lo: the residual is below u^2 |x| (u = 2^-8: 2^-16; fp16 2^-22, plus 2^-25
        absolute where lo is subnormal).  A weight then carries a factor 2^e, |e| <= u^2 (|m| + |bias|) + ..., and a
        channel's share moves by at most 2 ln2 |e| (numerator and row sum).  |m| <= max |logit| of the row.
    beta: a log2-unit bias [B or 1, 1, N, Nk] to use instead of log_bias (the tests' deliberately wrong biases).
    gain: float64 [Nk], powers of two -- key j's value is gain[j] * e_c (onehot_values(gain=...)), so the channel mass
      is sum w_j gain[j] over the unchanged row total: a key whose weight is 2^-65 of the row's largest still shows
      in its channel (staircase_inputs).  `weights` stay the plain w_j."""
    B, H, N, D = q.shape
    Nk = k.shape[2]
    assert Nk % nseg == 0 and not (skip and nseg != 1)
    P = Nk // nseg
    dt = q.dtype
    u = unit_roundoff(dt)
    qt = kernel_q(q, scale).double()
    s = qt @ k.double().transpose(-1, -2)                     # [B, H, N, Nk] log2 units (exact products, fp64 sums)
    if beta is None:
        beta = log2_bias(log_bias, skip, N, Nk, q.device)
    beta = beta.expand(B, 1, N, Nk)
    s = (s + beta).reshape(B, H, N, nseg, P)
    w = torch.exp2(s - s.amax(-1, keepdim=True))
    chan = channel_of(B, H, Nk, v_enc, q.device).view(B, H, nseg, P)
    idx = chan.unsqueeze(2).expand(B, H, N, nseg, P)
    wv = w if gain is None else w * gain.to(q.device).double().view(nseg, P)
    mass = torch.zeros(B, H, N, nseg, 64, dtype=torch.float64, device=q.device).scatter_add_(-1, idx, wv)
    ref = mass / w.sum(-1, keepdim=True)                      # [B, H, N, nseg, 64]
    rho, tau = (u * u, 0.0) if dt == torch.bfloat16 else (u * u, 2.0 ** -25)
    smax = s.abs().amax(-1, keepdim=True)
    bmax = beta.abs().reshape(B, 1, N, nseg, P).amax(-1, keepdim=True)
    eta = 2.0 ** -16 + 2.0 * math.log(2.0) * (rho * (smax + bmax) + 2 * tau)   # [B, H, N, nseg, 1]
    ref = ref.permute(0, 2, 3, 1, 4)                          # [B, N, nseg, H, 64]
    eta = eta.permute(0, 2, 3, 1, 4)
    if nseg == 1:
        ref, eta = ref[:, :, 0], eta[:, :, 0]
    return Reference(ref, eta, w, chan, P)


def weighted_bound(ref_c: torch.Tensor, dtype, nk: int, eta=2.0 ** -16) -> torch.Tensor:
    """Largest |out_c - ref_c| the kernels' arithmetic allows for a channel of mass ref_c (one-hot v):
        2u * ref_c + eta * ref_c + floor.
    Derivation (att_fast_weights, att_sum_*, att_store_row in tome_attn_tile.h and their callers): the row sum
    l adds the fp32 weights P (unrounded); the PV product multiplies the same weights rounded to the 16-bit format,
    P16 = P (1 + d), |d| <= u, by v in {0, 1}, so O_c = (1 + d') * mass_c with |d'| <= u; out = round16(O_c * (1/l))
    adds one more relative u.  Round-to-nearest keeps each of the two below u / (1 + u), so together they stay
    2u^2 / (1 + u) (bf16: ~2^-15) under 2u, on top of eta (weighted_reference): the fp32 arithmetic and the hi + lo
    splits, 2^-16 at least.  The bound is tight: a channel holding a single key (Nk <= 64 with the "mod" encoding)
    reaches ~0.94 of it on random q in every launch form, as much as the two roundings alone give when emulated.
    floor: fp16 has no range below 2^-24 -- weights under it are flushed and subnormal ones lose their relative
    precision, at most 2^-24 each; the reference point of every kernel is a key's own logit, so l >= 1 and the flushed
    mass of a channel is at most nk * 2^-24 of the output.  bf16 has fp32's range: a floor of 1e-6 for what
    underflows nowhere in practice.  A channel with no keys is exactly 0 (0 * P16 sums to 0).
    Values gain * e_c (weighted_reference's `gain`) need no further term: a power of two times P16 is exact in the
    fp32 product (the staircase keeps it inside fp32's range), the channel is still a sum of positive terms, whose
    fp32 accumulation error stays relative to the sum, and the rescaling by alpha = exp2(m_old - m_new) when the
    reference point moves multiplies O and l alike (one v_exp_f32 and one product each per move: inside eta)."""
    u = unit_roundoff(dtype)
    floor = nk * 2.0 ** -24 if dtype == torch.float16 else 1e-6
    return (2 * u + eta) * ref_c + floor


def check_weighted(out: torch.Tensor, ref: Reference, what: str = "") -> float:
    """Every channel of out (16-bit, shaped like ref.out) within weighted_bound of the fp64 reference; returns the
    largest |out - ref| / bound (<= 1)."""
    o = out.double()
    assert bool(torch.isfinite(o).all()), f"{what}: non-finite outputs"
    bound = weighted_bound(ref.out, out.dtype, ref.nk, ref.eta)
    ratio = (o - ref.out).abs() / bound
    worst = float(ratio.max())
    if worst > 1.0:
        idx = (ratio == ratio.max()).nonzero()[0].tolist()
        raise AssertionError(f"{what}: channel {idx} off by {worst:.3f}x its bound "
                             f"(out {float(o[tuple(idx)])}, reference {float(ref.out[tuple(idx)])})")
    return worst


def sensitivity(ref: Reference, dtype) -> float:
    """The smallest change that dropping or doubling any single key would make to its own channel, over that
    channel's bound; > 1 means no such mistake can hide inside the bound.  For a key of weight w in a channel of
    mass W_c out of W: dropping moves the channel by w (W - W_c) / (W (W - w)), doubling by w (W - W_c) / (W (W + w))
    (the smaller of the two).  Channels that hold every key of a row (W_c = W) are left out: no key count changes
    them, and the other channels of such a row are empty."""
    w, chan = ref.weights, ref.chan
    B, H, N, S, P = w.shape
    idx = chan.unsqueeze(2).expand(B, H, N, S, P)
    wmin = torch.full((B, H, N, S, 64), float("inf"), dtype=torch.float64, device=w.device)
    wmin = wmin.scatter_reduce(-1, idx, w, reduce="amin")
    mass = torch.zeros_like(wmin).scatter_add_(-1, idx, w)
    W = w.sum(-1, keepdim=True)
    delta = wmin * (W - mass) / (W * (W + wmin))
    share = mass / W
    eta = ref.eta.unsqueeze(2) if S == 1 else ref.eta
    eta = eta.permute(0, 3, 1, 2, 4)  # -> [B, H, N, S, 1]
    bound = weighted_bound(share, dtype, P, eta)
    live = (mass > 0) & (mass < W)
    assert bool(live.any()), "no channel where a single key shows"
    return float((delta / bound)[live].min())


# ---- a reference point that has to move ---------------------------------------------------------------------------

def staircase_inputs(B: int, H: int, N: int, Nk: int, dtype, step: int, generator: torch.Generator):
    """Inputs whose logits climb by `step` log2 units (at scale 1/8) from one 64-key tile to the next, so that the
    first pass's reference point (tile 0's maximum) falls behind by more than the 16-bit weights hold and has to move
    -- and values that keep every tile visible in the result all the same:
      q = 8 d + 0.05 noise along a unit direction d per (b, h); k_j = (step * (j // 64) / log2 e) d + 0.05 noise;
      bf16: gain[j] = 2^(step * (ntiles - 1 - j // 64)), for onehot_values / weighted_reference -- tile t's weights are
        ~2^(-step (ntiles - 1 - t)) of the last tile's, its values that much larger: every key contributes about
        equally to its channel, and a factor lost between the tiles before and after a move of the reference point
        shows in every channel;
      fp16: gain = None -- its range (65504) cannot hold the gains; with a channel per tile ("tile") its 2u = 2^-10
        and floor still show the tiles within two steps of the last one.
    Drawn on the generator's device.  -> q [B, H, N, 64], k [B, H, Nk, 64] of `dtype`, gain float64 [Nk] or None"""
    assert float(step).is_integer() and step > 0
    dev = generator.device
    d = torch.randn(B, H, 1, 64, generator=generator, device=dev)
    d = d / d.norm(dim=-1, keepdim=True)
    tile = torch.arange(Nk, device=dev) // ATT_BN
    ntiles = (Nk + ATT_BN - 1) // ATT_BN
    q = (8.0 * d + 0.05 * torch.randn(B, H, N, 64, generator=generator, device=dev)).to(dtype)
    amp = (float(step) / LOG2E) * tile.float().view(1, 1, Nk, 1)
    k = (amp * d + 0.05 * torch.randn(B, H, Nk, 64, generator=generator, device=dev)).to(dtype)
    gain = torch.exp2(float(step) * (ntiles - 1 - tile).double()) if dtype == torch.bfloat16 else None
    return q, k, gain


def rise(ref: Reference) -> float:
    """The smallest, over the rows, of (largest logit of the last tile) - (largest logit of tile 0), in log2 units,
    read from the reference's weights (log2 w = logit - row maximum).  Above log2(AttLimit) the lane that holds the
    row's largest key of the last tile sums >= 2^rise there against tile 0's reference point: a guard that has not
    tripped before the last tile must trip in it."""
    w = ref.weights
    assert w.shape[3] == 1, "one softmax per row"
    lw = torch.log2(w[:, :, :, 0])
    last0 = (ref.nk - 1) // ATT_BN * ATT_BN
    return float((lw[..., last0:].amax(-1) - lw[..., :ATT_BN].amax(-1)).min())


def tile_visibility(ref: Reference, gain: Optional[torch.Tensor], dtype, tiles=None) -> float:
    """The smallest, over the rows, the 64-key tiles (all, or `tiles`) and the channels a tile touches, of that
    tile's contribution to the channel (sum of w_j gain[j] over its keys of the channel, over the row total) divided
    by the channel's bound; > 1: no tile can go missing, or be scaled away, inside the bound."""
    w, chan = ref.weights, ref.chan
    B, H, N, S, P = w.shape
    assert S == 1
    wv = w[:, :, :, 0] if gain is None else w[:, :, :, 0] * gain.to(w.device).double()
    W = w[:, :, :, 0].sum(-1, keepdim=True)
    bound = weighted_bound(ref.out, dtype, P, ref.eta).permute(0, 2, 1, 3)   # [B, H, N, 64]
    ntiles = (P + ATT_BN - 1) // ATT_BN
    worst = float("inf")
    for t in (range(ntiles) if tiles is None else tiles):
        lo, hi = t * ATT_BN, min((t + 1) * ATT_BN, P)
        idx = chan[:, :, 0, lo:hi].unsqueeze(2).expand(B, H, N, hi - lo)
        part = torch.zeros(B, H, N, 64, dtype=torch.float64, device=w.device).scatter_add_(-1, idx, wv[..., lo:hi] / W)
        touched = torch.zeros(B, H, N, 64, dtype=torch.bool, device=w.device).scatter_(-1, idx, True)
        worst = min(worst, float((part / bound)[touched].min()))
    return worst
