"""The checks of tests/test_merge_ln_amp_gpu.py on the CPU: they accept the fp32 emulation of the launch
(tests/merge_ln_amp_oracle.py) and reject every slip it names, at the GPU test's own shapes; and the emulation alone meets
ln_oracle.check's input condition (>= 99 % exact-sum rows) at every shape used.  The matchings are those of the designed
metrics, computed by oracle/torch_port.py on the CPU."""
import pytest
import torch

import ln_amp_oracle as ao
import ln_oracle as lo
import merge_ln_amp_oracle as mo
from oracle import torch_port

F32 = torch.float32
EPS = mo.EPS
HALVES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


def _plan(how, T, cls, distill, r):
    metric = mo.paired_metric(mo.N, T, 100 * T + r) if how == "paired" else mo.dominant_metric(mo.N, T, 31 * T)
    plan = torch_port.match(metric, r, cls, distill)
    assert plan is not None and plan.r == r
    return plan, metric


def _keep(plan, metric):
    """The hybrid flags at the median score of the selected edges (merge.py:326): edge_keep [n, r]."""
    m = metric.double()
    m = m / m.norm(dim=-1, keepdim=True)
    best = (m[:, 0::2] @ m[:, 1::2].transpose(1, 2)).max(-1).values
    picked = best.gather(1, plan.src_idx.reshape(mo.N, -1))
    thr = picked.reshape(-1).sort().values[(picked.numel() - 1) // 2]
    keep = picked >= thr
    assert 0 < int(keep.sum()) < keep.numel()
    return keep


def _sizes(mode, plan, T, half, x_dtype, seed):
    if mode is None:
        return None
    if mode == "plain":
        return torch.randint(1, 6, (mo.N, T, 1), generator=torch.Generator().manual_seed(seed)).float()
    size = mo.pow2_sizes(plan.src_idx, plan.dst_idx, T, seed, F32 if mode == "f32" else half)
    return size if size.dtype in (x_dtype, F32) else size.to(x_dtype)  # (what _abi._prep_size hands the kernel)


def _emulated(plan, T, distill, C, half, x_dtype, a_dtype, size_mode, kind, seed, keep=None, drop=False, slip=None):
    own, into = mo.token_rows(plan.src_idx, plan.dst_idx, plan.unm_idx, T, distill)
    klass = (own.clamp(min=0) + (own < 0) * 4) if drop else into
    x, a = mo.inputs(kind, (mo.N, T, C), x_dtype, a_dtype, seed, klass)
    w, b = ao.affine(C, 7 + C)
    size = None if drop else _sizes(size_mode, plan, T, half, x_dtype, seed + 5)
    out = mo.emulate(x, a, size, plan.src_idx, plan.dst_idx, plan.unm_idx, distill, w, b, EPS, half, keep=keep, drop=drop,
                     slip=slip)
    return out, (w, b)


def _accepts(out, honest, wb, C, half, sig, tag):
    """The GPU test's check: x_out and size_out bit for bit with the unfused route (here: the honest emulation), y inside
    ln_oracle's bound on the stored rows.  Returns None when it passes, else what it saw."""
    (x0, y0, s0), (hx, _, hs) = out, honest
    if not torch.equal(x0, hx):
        return "x_out bits"
    if (s0 is None) != (hs is None) or (s0 is not None and not torch.equal(s0, hs)):
        return "size_out bits"
    To = x0.shape[1]
    try:
        lo.check(y0, x0, wb[0], wb[1], EPS, dtype=half, R=mo.form(C)[1], out_index=torch.arange(To).repeat(mo.N),
                 signature=sig, label=tag)
    except AssertionError as e:
        return str(e)
    return None


def _merge_shapes():
    """(how, T, cls, distill, r, C, size mode, kind, seed, hybrid) of every merge launch the GPU test makes."""
    for T, cls, distill in mo.TOKENS:
        r1, rc = mo.reductions(T, cls, distill)
        for C in mo.WIDTHS:
            for r, mode in mo.merge_cases(C, r1, rc):
                yield "paired", T, cls, distill, r, C, mode, "sig", 40 * C + T + r, False
    for T, cls, distill in mo.DOMINANT:
        for C in mo.DOMINANT_SIG_WIDTHS:
            for mode in ("f32", "half"):
                yield "dominant", T, cls, distill, mo.DOMINANT_R, C, mode, "sig", 13 * C + T, False
        for C in mo.DOMINANT_PLAIN_WIDTHS:
            for mode in ("plain", None):
                yield "dominant", T, cls, distill, mo.DOMINANT_R, C, mode, "plain", 13 * C + T, False
        for C in mo.DOMINANT_ODD_WIDTHS:
            yield "dominant", T, cls, distill, mo.DOMINANT_R, C, "plain", "sig", 13 * C + T, False
    for how, (T, cls, distill), r in mo.HYBRID:
        for C in mo.HYBRID_WIDTHS:
            yield how, T, cls, distill, r, C, "f32", "sig", 17 * C + T, True


@pytest.mark.parametrize("half", HALVES, ids=IDS)
def test_the_emulation_passes_at_every_shape(half, capsys):
    """Every launch of the GPU test, every dtype pair: the honest emulation is accepted -- which includes the 99 %
    condition on the merged rows, asserted by ln_oracle.check itself."""
    plans = {}
    count = 0
    for how, T, cls, distill, r, C, mode, kind, seed, hybrid in _merge_shapes():
        if (how, T, r) not in plans:
            plans[how, T, r] = _plan(how, T, cls, distill, r)
        plan, metric = plans[how, T, r]
        keep = _keep(plan, metric) if hybrid else None
        for x_dtype, a_dtype in ao.combos(half):
            if (kind, mode) == ("sig", "plain") and x_dtype == F32:  # (DOMINANT_ODD_WIDTHS: 16-bit streams)
                continue
            tag = f"{how} T={T} r={r} C={C} x={x_dtype} a={a_dtype} size={mode} {kind} hybrid={hybrid}"
            out, wb = _emulated(plan, T, distill, C, half, x_dtype, a_dtype, mode, kind, seed, keep=keep)
            assert _accepts(out, out, wb, C, half, kind == "sig", tag) is None, tag
            count += 1
    for T, cls, distill in mo.TOKENS:
        for r in mo.reductions(T, cls, distill):
            plan, _ = _plan("paired", T, cls, distill, r)
            for C in mo.DROP_WIDTHS:
                for x_dtype, a_dtype in ao.combos(half):
                    tag = f"drop T={T} r={r} C={C} x={x_dtype} a={a_dtype}"
                    out, wb = _emulated(plan, T, distill, C, half, x_dtype, a_dtype, None, "sig", 50 * C + T + r, drop=True)
                    assert _accepts(out, out, wb, C, half, True, tag) is None, tag
                    count += 1
    capsys.readouterr()
    print(f"{count} launches emulated and accepted for {half}")


# slip -> the launches that can show it: (how, T index in TOKENS / DOMINANT, r, C, size mode, kind, combos, drop)
def _slip_cases(slip, half):
    f32_only = [(F32, F32), (F32, None)]
    half_only = [(half, half), (half, None)]
    every = ao.combos(half)
    if slip == "sum_rounded_16bit":      # an fp32 stream whose sum no 16-bit format holds
        return [("paired", (10, False, False), 5, C, "f32", "sig", f32_only, False) for C in (64, 768)]
    if slip == "stats_from_accumulator":
        # a 16-bit stream whose division is rounded (sizes 1..5: the total is no power of two) on rows far from zero: the
        # mean of the rounding errors moves every element of the row.  (An fp32 stream stores the accumulator itself.)
        return [("dominant", d, 3, C, "plain", "sig", half_only, False) for d in mo.DOMINANT for C in mo.DOMINANT_ODD_WIDTHS]
    if slip == "sources_reversed":
        # plain rows, sizes 1..5 on an fp32 stream: the order of the additions is in x_out's bits (the rounding of a
        # 16-bit stream swallows the last fp32 bit on all but a few elements)
        x32 = [c for c in every if c[0] == F32]
        return [("dominant", d, 3, C, "plain", "plain", x32, False) for d in mo.DOMINANT for C in mo.DOMINANT_PLAIN_WIDTHS]
    if slip == "dropped_row_normalised":
        return [("paired", t, 1, C, None, "sig", every, True) for t in (mo.TOKENS[1], mo.TOKENS[3]) for C in (8, 768)]
    if slip == "stats_unmerged_row":
        return [("paired", t, mo.clamp_r(*t), C, "f32", "sig", every, False) for t in mo.TOKENS for C in (64, 1024)]
    return [("paired", t, mo.clamp_r(*t), C, "f32", "sig", every, False) for t in mo.TOKENS[:2] for C in (64, 520, 1024)]


@pytest.mark.parametrize("slip", mo.SLIPS)
@pytest.mark.parametrize("half", HALVES, ids=IDS)
def test_every_slip_is_rejected(half, slip):
    for how, (T, cls, distill), r, C, mode, kind, combos, drop in _slip_cases(slip, half):
        plan, _ = _plan(how, T, cls, distill, r)
        for x_dtype, a_dtype in combos:
            tag = f"{slip} {how} T={T} r={r} C={C} x={x_dtype} a={a_dtype}"
            seed = 13 * C + T
            honest, wb = _emulated(plan, T, distill, C, half, x_dtype, a_dtype, mode, kind, seed, drop=drop)
            assert _accepts(honest, honest, wb, C, half, kind == "sig", tag) is None, tag + ": the honest emulation"
            slipped, _ = _emulated(plan, T, distill, C, half, x_dtype, a_dtype, mode, kind, seed, drop=drop, slip=slip)
            seen = _accepts(slipped, honest, wb, C, half, kind == "sig", tag)
            assert seen is not None, tag + ": the slip went unseen"


def test_designed_matchings():
    """paired: one source per destination at r = 1 and at the clamp; dominant: every source of a group shares one."""
    for T, cls, distill in mo.TOKENS:
        for r in mo.reductions(T, cls, distill):
            plan, _ = _plan("paired", T, cls, distill, r)
            dst = plan.dst_idx.reshape(mo.N, -1)
            assert all(len(set(row.tolist())) == r for row in dst), (T, r)
    for T, cls, distill in mo.DOMINANT:
        plan, _ = _plan("dominant", T, cls, distill, mo.DOMINANT_R)
        dst = plan.dst_idx.reshape(mo.N, -1)
        assert bool((dst == dst[:, :1]).all()) and (not distill or int(dst.min()) > 0), T


def test_emulation_restates_the_contract():
    """Without addend, distillation token and flags the emulation's merge is oracle/torch_port.merge_wavg on fp32 rows
    whenever the sums are exact (signature rows, power-of-two sizes): the same values, whatever the order."""
    T, cls, distill = mo.TOKENS[2]
    for how, r in (("paired", mo.clamp_r(T, cls, distill)), ("dominant", 3)):
        plan, _ = _plan(how, T, cls, distill, r)
        _, into = mo.token_rows(plan.src_idx, plan.dst_idx, plan.unm_idx, T, distill)
        x = lo.signature_rows((mo.N, T, 64), F32, 5, 1, into)
        size = mo.pow2_sizes(plan.src_idx, plan.dst_idx, T, 6)
        w, b = ao.affine(64, 1)
        x_out, _, s_out = mo.emulate(x, None, size, plan.src_idx, plan.dst_idx, plan.unm_idx, distill, w, b, EPS,
                                     torch.bfloat16)
        want_x, want_s = torch_port.merge_wavg(plan, x, size)
        assert torch.equal(x_out, want_x) and torch.equal(s_out, want_s), how
