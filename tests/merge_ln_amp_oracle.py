"""Accounting for the add + merge + LayerNorm launch under autocast (tome_merge_wavg_ln_amp, tome_drop_ln_amp): cases,
inputs, an fp32 emulation on the CPU with the slips such a kernel can make.  No test functions; importable without a GPU.
tests/test_merge_ln_amp_oracle_cpu.py shows on the CPU that the checks accept the emulation and reject every slip at the
shapes tests/test_merge_ln_amp_gpu.py uses; that file applies the same checks to the kernels.

Checks.  x_out, size_out (and log(size_out)) are compared BIT FOR BIT with the unfused route on the same plan
(`ln_amp_oracle.stored_sum`, then tome_merge_wavg / tome_drop -- here: `emulate` without a slip, which restates the
contract's order: fp32 products, the destination's own term first, then its sources in src_idx order, one division, one
rounding to x's dtype).  y_out goes through ln_oracle.check on the STORED x_out rows with the fp32 parameters.

Inputs.  ln_oracle.check asserts that at least 99 % of the rows it is given are exact-sum rows.  The merged rows are kept
so by construction:
  * every token of one merge group (a destination and its sources) has the signature class of its OUTPUT row
    (`token_rows`), so the group averages rows of one class;
  * the matching is made by a metric that is designed, not drawn: `paired_metric` gives every source a destination of its
    own (one source per destination), `dominant_metric` sends every source to ONE destination (several sources share it);
  * the sizes are powers of two whose total per destination is a power of two again (`pow2_sizes`): the division is exact
    on the rows' grid.  size=None (ones) is used with the paired metric only: 1 + 1 = 2.
"plain" inputs (ln_oracle.plain_rows, sizes 1..5) have no grid: they are what makes the ORDER of a destination's sources
visible in x_out's bits; their y is checked without the condition on the inputs, as the 16-bit tests do.
"""
import torch

import ln_amp_oracle as ao
import ln_oracle as lo

F32 = torch.float32
EPS = 1e-6
# (T, class token, distillation token): n = 3 groups each
TOKENS = ((9, True, False), (10, False, False), (197, True, False), (12, True, True))
# widths: the issue's six, and one per launch form of the kernel (slots per lane, rows per wave, a row boundary inside
# an iteration) -- see form()
WIDTHS = (8, 64, 192, 520, 768, 1024, 512)
N = 3
# several sources per destination (dominant_metric, r = 3): signature rows at widths whose merged fp32 rows (a grid 1024
# times finer than the class's step) still sum exactly, plain rows at the widths of two slots per lane
DOMINANT = ((10, False, False), (12, True, True))
DOMINANT_R = 3
DOMINANT_SIG_WIDTHS = (8, 64, 192)
DOMINANT_PLAIN_WIDTHS = (768, 1024)
# ... and signature rows with sizes 1..5 on a 16-bit stream: the division is rounded to 16 bits on rows far from zero (what
# shows statistics taken from the accumulator); an fp32 stream would leave the grid there
DOMINANT_ODD_WIDTHS = (64, 192, 768)
HYBRID = (("paired", (10, False, False), 5), ("paired", (197, True, False), 98), ("dominant", (10, False, False), 3))
HYBRID_WIDTHS = (64, 768)
DROP_WIDTHS = (8, 200, 768, 1024)


def merge_cases(C, r1, rc):
    """(r, size mode) of test_merge_every_width_and_token_count at width C: r = 1 without sizes, r at the clamp with fp32
    sizes, and with 16-bit sizes at two widths."""
    return [(r1, None), (rc, "f32")] + ([(rc, "half")] if C in (64, 768) else [])
SLIPS = ("stats_unmerged_row", "stats_from_accumulator", "sum_rounded_16bit", "sources_reversed", "neighbour_rstd",
         "weights_16bit", "dropped_row_normalised")


def form(C):
    """(NIT, R) of k_merge_rows_ln_amp (csrc/tome_kernels.hip: merge_ln_amp_impl): three slots per lane, R rows per
    wave -- tome_add_layernorm_amp's form, ln_oracle.expected_form("add_layernorm", C)."""
    nit, R, _ = lo.expected_form("add_layernorm", C)
    return nit, R


def launch_form(C):
    """What distinguishes the launches: (rows per wave, slots per lane in use, a row boundary inside an iteration)."""
    _, R = form(C)
    cpr = C // 8
    return R, -(-R * cpr // lo.WAVE), lo.boundary_inside_iteration(C, R)


def clamp_r(T, cls, distill):
    return (T - int(cls) - int(distill)) // 2


def reductions(T, cls, distill):
    """r = 1 and r at the clamp."""
    return (1, clamp_r(T, cls, distill))


# ---------------------------------------------------------------------------------------------------------------------
# designed matchings
# ---------------------------------------------------------------------------------------------------------------------
def paired_metric(n, T, seed):
    """Every unprotected even token is most similar to an odd token of its own (a basis vector they share: odd token
    2i+1 for even token 2i when T is even, 2i-1 when T is odd and token 0 is the class token), with a similarity drawn
    per group: every source has a destination of its own, all scores distinct."""
    D = T // 2 + 2
    gen = torch.Generator().manual_seed(seed)
    m = torch.zeros(n, T, D)
    T1, T2 = (T + 1) // 2, T // 2
    for g in range(n):
        tilt = (torch.randperm(T1, generator=gen).float() + 1.0) / (2.0 * T1)  # distinct angles to the partner
        for i in range(T1):
            j = i if T % 2 == 0 else max(i - 1, 0)
            m[g, 2 * i, j] = 1.0
            m[g, 2 * i, D - 1] = tilt[i]
        for j in range(T2):
            m[g, 2 * j + 1, j] = 1.0
    return m


def dominant_metric(n, T, seed, D=32):
    """Every even token is most similar to ONE odd token (the dominant key, drawn per group; not odd token 0, which a
    distillation token protects), with distinct similarities: all r sources share that destination."""
    gen = torch.Generator().manual_seed(seed)
    m = 0.01 * torch.randn(n, T, D, generator=gen)
    T1, T2 = (T + 1) // 2, T // 2
    for g in range(n):
        star = 1 + int(torch.randint(0, T2 - 1, (1,), generator=gen))
        m[g, 1::2, 0] -= 1.0
        m[g, 2 * star + 1] = 0.0
        m[g, 2 * star + 1, 0] = 1.0
        m[g, 0::2, 0] = 1.0
        m[g, 0::2, 1] = (torch.randperm(T1, generator=gen).float() + 1.0) / (2.0 * T1)
    return m


def token_rows(src_idx, dst_idx, unm_idx, T, distill):
    """Output row of every token ([n, T]; -1: an even token that is merged away -- its destination's row is in
    `merged_into`), and merged_into [n, T]: the row a token's values end up in (a drop: -1 for the dropped ones)."""
    src, dst, unm = (t.cpu().long().reshape(t.shape[0], -1) for t in (src_idx, dst_idx, unm_idx))
    n, U = unm.shape
    T2 = T // 2
    i, j = torch.arange(U), torch.arange(T2)
    if distill:
        a_row, b_row = torch.where(i == 0, 0, i + 1), torch.where(j == 0, 1, U + j)
    else:
        a_row, b_row = i, U + j
    own = torch.full((n, T), -1, dtype=torch.long)
    g = torch.arange(n)[:, None]
    own[:, 1::2] = b_row[None, :]
    own[g, 2 * unm] = a_row[None, :].expand(n, U)
    into = own.clone()
    into[g, 2 * src] = b_row[dst]
    return own, into


def pow2_sizes(src_idx, dst_idx, T, seed, dtype=F32):
    """[n, T, 1] sizes, powers of two, whose total over every destination and its sources is a power of two: a
    destination with k sources has size 2^(k-1), its sources 1, 1, 2, 4, ... in rank order (with its own term zeroed by
    a hybrid flag the sources alone still total 2^(k-1)); tokens outside every merge 1, 2, 4 or 8."""
    src, dst = (t.cpu().long().reshape(t.shape[0], -1) for t in (src_idx, dst_idx))
    n, r = src.shape
    gen = torch.Generator().manual_seed(seed)
    size = torch.exp2(torch.randint(0, 4, (n, T), generator=gen).float())
    for g in range(n):
        count = {}
        for k in range(r):
            j = int(dst[g, k])
            c = count.get(j, 0)
            size[g, 2 * int(src[g, k])] = 1.0 if c == 0 else 2.0 ** (c - 1)
            count[j] = c + 1
        for j, c in count.items():
            size[g, 2 * j + 1] = 2.0 ** (c - 1)
    return size[..., None].to(dtype)


def inputs(kind, shape, x_dtype, a_dtype, seed, klass):
    """(x, addend or None) on the CPU: "sig" = ln_amp_oracle.forward_inputs with the classes of the output rows,
    "plain" = ln_oracle.plain_rows in the dtypes."""
    if kind == "sig":
        return ao.forward_inputs(shape, x_dtype, a_dtype, seed, klass)
    x = lo.plain_rows(shape, x_dtype, seed)
    a = None if a_dtype is None else (0.5 * lo.plain_rows(shape, torch.float64, seed + 1)).to(a_dtype)
    return x, a


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulation (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def emulate(x, a, size, src_idx, dst_idx, unm_idx, distill, w, b, eps, half, keep=None, drop=False, slip=None):
    """(x_out, y_out, size_out or None): the launch as an honest fp32 evaluation -- ln_amp_oracle.stored_sum, the merge
    in the contract's order, ln_amp_oracle.emulate_forward's LayerNorm of the stored rows.  keep [n, r] (hybrid flags):
    a destination with an edge below the threshold loses its own term.  slip: one of SLIPS."""
    assert slip is None or slip in SLIPS
    xs = ao.stored_sum(x, a)
    if slip == "sum_rounded_16bit" and xs.dtype == F32:
        xs = xs.to(half).float()
    n, T, C = xs.shape
    src, dst, unm = (t.cpu().long().reshape(n, -1) for t in (src_idx, dst_idx, unm_idx))
    r = src.shape[1]
    own, into = token_rows(src_idx, dst_idx, unm_idx, T, distill)
    To = T - r
    g = torch.arange(n)[:, None]
    tok = torch.zeros((n, To), dtype=torch.long)  # the token that owns every output row
    kept = own >= 0
    tok[g.expand(n, T)[kept], own[kept]] = torch.arange(T)[None, :].expand(n, T)[kept]
    xf = xs.float()
    rows = xf[g, tok]                                                        # [n, To, C]
    if drop:
        x_out, s_out, acc_rows = rows.to(xs.dtype), None, rows
    else:
        sf = torch.ones((n, T), dtype=F32) if size is None else size.float().reshape(n, T)
        s_own = sf[g, tok]
        acc, ssum = rows * s_own[..., None], s_own.clone()
        if keep is not None:
            kill = torch.zeros((n, To), dtype=torch.bool)
            bad = keep.cpu().reshape(n, r) == 0
            kill[g.expand(n, r)[bad], into[g, 2 * src][bad]] = True
            acc = torch.where(kill[..., None], acc * 0.0, acc)
            ssum = torch.where(kill, ssum * 0.0, ssum)
        order = range(r - 1, -1, -1) if slip == "sources_reversed" else range(r)
        gi = torch.arange(n)
        for k in order:  # rank order: one source per group and step, so every destination adds its sources in sequence
            t = 2 * src[:, k]
            o = into[gi, t]
            acc[gi, o] = acc[gi, o] + xf[gi, t] * sf[gi, t][:, None]
            ssum[gi, o] = ssum[gi, o] + sf[gi, t]
        acc_rows = acc / ssum[..., None]
        x_out = acc_rows.to(xs.dtype)
        s_dtype = xs.dtype if size is None else size.dtype
        s_out = ssum[..., None].to(s_dtype)
    v = x_out.float().reshape(n * To, C)
    if slip is None:
        return x_out, ao.emulate_forward(v, None, w, b, eps, half)[1].reshape(n, To, C), s_out
    stats = v
    if slip == "stats_unmerged_row":
        stats = rows.reshape(n * To, C)
    elif slip == "stats_from_accumulator":
        stats = acc_rows.reshape(n * To, C)
    elif slip == "dropped_row_normalised":  # a dropped even token in place of the first kept row
        assert drop
        wrong = x_out.float().clone()
        wrong[:, 0] = xf[torch.arange(n), 2 * src[:, 0]]
        v = stats = wrong.reshape(n * To, C)
    wl, bl = (w.to(half), b.to(half)) if slip == "weights_16bit" else (w, b)
    y = _apply_stats(v, stats, wl, bl, eps, half, roll_rstd=slip == "neighbour_rstd")
    return x_out, y.reshape(n, To, C), s_out


def _apply_stats(v, stats, w, b, eps, half, roll_rstd=False):
    """ln_amp_oracle.emulate_forward's arithmetic with the mean and rstd of `stats` applied to the rows `v`."""
    inv_c = torch.tensor(1.0 / v.shape[-1], dtype=F32)
    m = stats.sum(-1, keepdim=True) * inv_c
    ds = stats - m
    rstd = torch.rsqrt((ds * ds).sum(-1, keepdim=True) * inv_c + torch.tensor(eps, dtype=F32))
    if roll_rstd:
        rstd = torch.roll(rstd, 1, 0)
    return ((v - m) * (w.float() * rstd) + b.float()).to(half)


def received(src_idx, dst_idx, unm_idx, T, distill):
    """[n, T - r] mask of the output rows that receive sources (the rows the edge waves build)."""
    own, into = token_rows(src_idx, dst_idx, unm_idx, T, distill)
    n = own.shape[0]
    r = src_idx.shape[1]
    recv = torch.zeros((n, T - r), dtype=torch.bool)
    moved = (own < 0)
    recv[torch.arange(n)[:, None].expand(n, T)[moved], into[moved]] = True
    return recv
