"""tome_merge_wavg_ln_amp / tome_drop_ln_amp: the residual add + reduction + LayerNorm launch under autocast.
x_out, size_out and log(size_out) bit for bit against the unfused route on the same plan (the framework's stored sum, then
tome_merge_wavg / tome_drop); y_out against the fp64 LayerNorm of the STORED x_out rows with the fp32 parameters inside
tests/ln_oracle.py's bound, whose input condition (>= 99 % exact-sum rows) the check asserts itself -- the inputs are made
for it by tests/merge_ln_amp_oracle.py (designed matchings, one signature class per merge group, power-of-two sizes), and
tests/test_merge_ln_amp_oracle_cpu.py shows on the CPU that these checks see the slips such a kernel can make.  Small
shapes throughout: n = 3 groups; T = 9 / 197 with a class token, 10 without, 12 with class and distillation token; r = 1
and r at the clamp; one r where several sources share a destination; every legal dtype pair of both halves; widths that
reach every launch form."""
import pytest
import torch

import ln_amp_oracle as ao
import ln_oracle as lo
import merge_ln_amp_oracle as mo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = mo.EPS
F32 = torch.float32
HALVES = [torch.bfloat16, torch.float16]
HALF_IDS = ["bf16", "fp16"]
COMBO_IDS = ["x16_a16", "x16", "x32_a16", "x32_a32", "x32"]

# checked at collection, on any machine: the widths reach one to four rows per wave, one to three slots per lane, and
# rows that start inside a lane iteration as well as on its boundary
_forms = {mo.launch_form(C) for C in mo.WIDTHS}
assert {R for R, _, _ in _forms} == {1, 2, 3, 4} and {s for _, s, _ in _forms} == {1, 2, 3}, sorted(_forms, key=str)
assert {b for _, _, b in _forms} == {None, False, True}, sorted(_forms, key=str)
assert all(mo.form(C) == lo.expected_form("add_layernorm", C)[:2] for C in mo.WIDTHS)


def _abi():
    from tome import _abi
    return _abi


def _tome():
    from tome import merge as tm
    return tm


def _match(metric, r, cls, distill, how="merge", threshold=None):
    tm = _tome()
    m = metric.to(DEV)
    if how == "drop":
        return tm.bipartite_soft_matching_drop(m, r, cls, distill).plan
    if how == "hybrid":
        return tm.bipartite_soft_matching_hybrid(m, r, cls, distill, "hybrid", threshold)[0].plan
    return tm.bipartite_soft_matching(m, r, cls, distill)[0].plan


def _median_threshold(metric, plan):
    """The median score of the selected edges, fp64 on the CPU: about half of them fall below it."""
    m = metric.double()
    m = m / m.norm(dim=-1, keepdim=True)
    best = (m[:, 0::2] @ m[:, 1::2].transpose(1, 2)).max(-1).values
    picked = best.gather(1, plan.src_idx.cpu().long().reshape(plan.n, -1)).reshape(-1).sort().values
    return float(picked[(picked.numel() - 1) // 2])


def _sizes(mode, plan, T, half, x_dtype, seed):
    """None, or [n, T, 1] on the device: powers of two (fp32 / 16-bit), or 1..5 for the plain inputs."""
    if mode is None:
        return None
    if mode == "plain":
        gen = torch.Generator().manual_seed(seed)
        return torch.randint(1, 6, (plan.n, T, 1), generator=gen).float().to(DEV)
    return mo.pow2_sizes(plan.src_idx, plan.dst_idx, T, seed, F32 if mode == "f32" else half).to(DEV)


def _merge_case(plan, T, C, half, x_dtype, a_dtype, size_mode, kind, seed, tag, twice=False):
    """One launch of the merge entry against the unfused route and the LayerNorm bound; returns worst err / bound."""
    abi = _abi()
    n, To = plan.n, T - plan.r
    _, into = mo.token_rows(plan.src_idx, plan.dst_idx, plan.unm_idx, T, plan.distill_token)
    x, a = mo.inputs(kind, (n, T, C), x_dtype, a_dtype, seed, into)
    x, a = x.to(DEV), None if a is None else a.to(DEV)
    w, b = (t.to(DEV) for t in ao.affine(C, 7 + C))
    size = _sizes(size_mode, plan, T, half, x_dtype, seed + 5)
    s = ao.stored_sum(x, a)  # the framework's own add, on the device
    want_x, want_s = abi.merge_wavg(plan, s, size, log_size=True)
    x0, y0, s0 = abi.merge_wavg_ln_amp(plan, x, size, w, b, EPS, half, addend=a, log_size=True)
    assert x0.dtype == x_dtype and y0.dtype == half and s0.dtype == want_s.dtype, tag
    assert tuple(x0.shape) == (n, To, C) and tuple(y0.shape) == (n, To, C), tag
    assert torch.equal(x0, want_x), tag + ": x_out differs from merge_wavg of the stored sum"
    assert torch.equal(s0, want_s), tag + ": size_out"
    assert torch.equal(s0._tome_log, want_s._tome_log), tag + ": log(size_out)"
    recv = mo.received(plan.src_idx, plan.dst_idx, plan.unm_idx, T, plan.distill_token)
    assert bool(recv.any()), tag + ": no row receives a source"
    R = mo.form(C)[1]
    worst = lo.check(y0, x0, w, b, EPS, dtype=half, R=R, out_index=torch.arange(To).repeat(n), signature=kind == "sig",
                     label=tag)["worst"]
    if twice:
        x1, y1, s1 = abi.merge_wavg_ln_amp(plan, x, size, w, b, EPS, half, addend=a, log_size=True)
        assert torch.equal(x1, x0) and torch.equal(y1, y0) and torch.equal(s1, s0), tag + ": second run"
        assert torch.equal(s1._tome_log, s0._tome_log), tag + ": second run"
    return worst


@pytest.fixture(scope="module")
def plans():
    """The matchings of the module, made once: paired (r = 1 and the clamp) for every token count, dominant (r = 3)."""
    out = {}
    for T, cls, distill in mo.TOKENS:
        for r in mo.reductions(T, cls, distill):
            metric = mo.paired_metric(mo.N, T, 100 * T + r)
            plan = _match(metric, r, cls, distill)
            assert plan.r == r, (T, r, plan.r)
            _, into = mo.token_rows(plan.src_idx, plan.dst_idx, plan.unm_idx, T, distill)
            dstrows = into[torch.arange(mo.N)[:, None], 2 * plan.src_idx.cpu().long().reshape(mo.N, -1)]
            assert all(len(set(row.tolist())) == r for row in dstrows), "paired metric: a destination is shared"
            out["paired", T, r] = (plan, metric)
    for T, cls, distill in mo.DOMINANT:
        metric = mo.dominant_metric(mo.N, T, 31 * T)
        plan = _match(metric, mo.DOMINANT_R, cls, distill)
        dst = plan.dst_idx.cpu().reshape(mo.N, -1)
        assert plan.r == 3 and bool((dst == dst[:, :1]).all()), "dominant metric: the sources do not share a destination"
        out["dominant", T, 3] = (plan, metric)
    return out


@pytest.mark.parametrize("combo", range(5), ids=COMBO_IDS)
@pytest.mark.parametrize("half", HALVES, ids=HALF_IDS)
def test_merge_every_width_and_token_count(half, combo, plans, capsys):
    """Every width x token count: r = 1 without sizes, r at the clamp with fp32 sizes (16-bit sizes at two widths), one
    source per destination; the same bits on two runs."""
    x_dtype, a_dtype = ao.combos(half)[combo]
    worst = 0.0
    for T, cls, distill in mo.TOKENS:
        r1, rc = mo.reductions(T, cls, distill)
        for C in mo.WIDTHS:
            for r, size_mode in mo.merge_cases(C, r1, rc):
                plan = plans["paired", T, r][0]
                tag = f"merge_wavg_ln_amp T={T} r={r} distill={distill} C={C} x={x_dtype} a={a_dtype} size={size_mode}"
                worst = max(worst, _merge_case(plan, T, C, half, x_dtype, a_dtype, size_mode, "sig", 40 * C + T + r, tag,
                                               twice=C == 768 and r == rc))
    capsys.readouterr()
    print(f"tome_merge_wavg_ln_amp {half} {COMBO_IDS[combo]}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("combo", range(5), ids=COMBO_IDS)
@pytest.mark.parametrize("half", HALVES, ids=HALF_IDS)
def test_merge_sources_share_a_destination(half, combo, plans):
    """r = 3 with a dominant key: all sources of a group merge into one destination, with and without a distillation
    token.  Signature rows with power-of-two sizes for the LayerNorm condition; plain rows with sizes 1..5, whose x_out
    bits depend on the order of the sources."""
    x_dtype, a_dtype = ao.combos(half)[combo]
    for T, _, _ in mo.DOMINANT:
        plan = plans["dominant", T, 3][0]
        todo = [(C, "sig", m) for C in mo.DOMINANT_SIG_WIDTHS for m in ("f32", "half")]
        todo += [(C, "plain", m) for C in mo.DOMINANT_PLAIN_WIDTHS for m in ("plain", None)]
        if x_dtype != F32:  # a division that is rounded to 16 bits on rows far from zero
            todo += [(C, "sig", "plain") for C in mo.DOMINANT_ODD_WIDTHS]
        for C, kind, size_mode in todo:
            tag = f"merge_wavg_ln_amp dominant T={T} C={C} x={x_dtype} a={a_dtype} {kind} size={size_mode}"
            _merge_case(plan, T, C, half, x_dtype, a_dtype, size_mode, kind, 13 * C + T, tag)


@pytest.mark.parametrize("combo", range(5), ids=COMBO_IDS)
@pytest.mark.parametrize("half", HALVES, ids=HALF_IDS)
def test_hybrid_flags(half, combo, plans):
    """The plan's threshold flags: a destination with an edge below the threshold loses its own term (and is zeroed
    when all its edges are below it), as in tome_merge_wavg on the stored sum.  The threshold is the median score of the
    selected edges, so at least one destination is zeroed and at least one is not."""
    x_dtype, a_dtype = ao.combos(half)[combo]
    for how, (T, cls, distill), r in mo.HYBRID:
        key = (how, T, r)
        plain, metric = plans[key]
        plan = _match(metric, r, cls, distill, "hybrid", _median_threshold(metric, plain))
        keep = plan.edge_keep
        assert keep is not None and 0 < int(keep.sum()) < keep.numel(), (int(keep.sum()), keep.numel())
        assert torch.equal(plan.src_idx, plain.src_idx)
        for C in mo.HYBRID_WIDTHS:
            tag = f"merge_wavg_ln_amp hybrid {key} C={C} x={x_dtype} a={a_dtype}"
            _merge_case(plan, T, C, half, x_dtype, a_dtype, "f32", "sig", 17 * C + T, tag)


@pytest.mark.parametrize("combo", range(5), ids=COMBO_IDS)
@pytest.mark.parametrize("half", HALVES, ids=HALF_IDS)
def test_drop(half, combo):
    """tome_drop_ln_amp: x_out bit-equal to tome_drop of the stored sum, y_out the LayerNorm of the kept rows; with and
    without a distillation token, r = 1 and the clamp, the same bits on two runs."""
    abi = _abi()
    x_dtype, a_dtype = ao.combos(half)[combo]
    for T, cls, distill in mo.TOKENS:
        for r in mo.reductions(T, cls, distill):
            plan = _match(mo.paired_metric(mo.N, T, 100 * T + r), r, cls, distill, "drop")
            n, To = plan.n, T - plan.r
            own, _ = mo.token_rows(plan.src_idx, plan.dst_idx, plan.unm_idx, T, distill)
            for C in mo.DROP_WIDTHS:
                tag = f"drop_ln_amp T={T} r={r} distill={distill} C={C} x={x_dtype} a={a_dtype}"
                x, a = mo.inputs("sig", (n, T, C), x_dtype, a_dtype, 50 * C + T + r, own.clamp(min=0) + (own < 0) * 4)
                x, a = x.to(DEV), None if a is None else a.to(DEV)
                w, b = (t.to(DEV) for t in ao.affine(C, 7 + C))
                want = abi.drop(plan, ao.stored_sum(x, a))
                x0, y0 = abi.drop_ln_amp(plan, x, w, b, EPS, half, addend=a)
                assert x0.dtype == x_dtype and y0.dtype == half and tuple(y0.shape) == (n, To, C), tag
                assert torch.equal(x0, want), tag + ": x_out differs from drop of the stored sum"
                lo.check(y0, x0, w, b, EPS, dtype=half, R=mo.form(C)[1], out_index=torch.arange(To).repeat(n), label=tag)
                x1, y1 = abi.drop_ln_amp(plan, x, w, b, EPS, half, addend=a)
                assert torch.equal(x1, x0) and torch.equal(y1, y0), tag + ": second run"


def test_grid_split_beyond_65535_groups():
    """n = 70000 groups of T = 4 tokens, C = 8, r = 1: the group index spans grid.y and grid.z."""
    abi = _abi()
    n, T, C, half = 70000, 4, 8, torch.bfloat16
    metric = torch.randn(n, T, 8, generator=torch.Generator().manual_seed(3))
    plan = _match(metric, 1, False, False)
    x = lo.plain_rows((n, T, C), half, 11).to(DEV)
    a = lo.plain_rows((n, T, C), half, 12).to(DEV)
    w, b = (t.to(DEV) for t in ao.affine(C, 5))
    want_x, want_s = abi.merge_wavg(plan, x + a, None)
    x0, y0, s0 = abi.merge_wavg_ln_amp(plan, x, None, w, b, EPS, half, addend=a)
    assert torch.equal(x0, want_x) and torch.equal(s0, want_s)
    lo.check(y0, x0, w, b, EPS, dtype=half, R=4, out_index=torch.arange(T - 1).repeat(n), signature=False, label="n=70000")


# ---------------------------------------------------------------------------------------------------------------------
# refusals: an error code with its message, and nothing launched
# ---------------------------------------------------------------------------------------------------------------------
def _raw(abi, plan, x, a, w, b, xo, y, so, C=None, y_code=None, drop=False):
    code = abi.DTYPES
    n, T = plan.n, plan.T
    C = x.shape[-1] if C is None else C
    yc = code[y.dtype] if y_code is None else y_code
    L = abi.lib()
    if drop:
        return L.tome_drop_ln_amp(x.data_ptr(), code[x.dtype], abi._ptr(a), 0 if a is None else code[a.dtype], n, T, C,
                                  plan.r, plan.unm_idx.data_ptr(), 0, w.data_ptr(), b.data_ptr(), EPS, xo.data_ptr(),
                                  y.data_ptr(), yc, abi._stream(x.device))
    return L.tome_merge_wavg_ln_amp(x.data_ptr(), code[x.dtype], abi._ptr(a), 0 if a is None else code[a.dtype], None,
                                    code[so.dtype], n, T, C, plan.r, plan.src_idx.data_ptr(), plan.dst_idx.data_ptr(),
                                    plan.unm_idx.data_ptr(), 0, None, w.data_ptr(), b.data_ptr(), EPS, xo.data_ptr(),
                                    y.data_ptr(), yc, so.data_ptr(), None, abi._stream(x.device))


@pytest.mark.parametrize("drop", [False, True], ids=["merge", "drop"])
def test_refusals(drop):
    abi = _abi()
    L = abi.lib()
    name = b"tome_drop_ln_amp" if drop else b"tome_merge_wavg_ln_amp"
    n, T, r = 2, 8, 2
    plan = _match(torch.randn(n, T, 16, generator=torch.Generator().manual_seed(1)), r, False, False,
                  "drop" if drop else "merge")

    def mk(dtype, C, rows=T, fill=0.0):
        return torch.full((n, rows, C), fill, dtype=dtype, device=DEV)

    def refused(x, a, w, b, yd, C, what, text, y_code=None):
        xo, y, so = mk(x.dtype, C, T - r, 7.0), mk(yd, C, T - r, 7.0), mk(F32, 1, T - r, 7.0)
        rc = _raw(abi, plan, x, a, w, b, xo, y, so, C=C, y_code=y_code, drop=drop)
        err = L.tome_last_error()
        assert rc != 0 and name in err and text in err, (what, rc, err)
        torch.cuda.synchronize()
        assert bool((xo == 7).all()) and bool((y == 7).all()) and bool((so == 7).all()), f"{what}: something was launched"

    C = 64
    w = torch.ones(C, dtype=F32, device=DEV)
    for xd, ad, yd in ao.illegal_combos():
        refused(mk(xd, C), None if ad is None else mk(ad, C), w, w, yd, C, (xd, ad, yd), b"unsupported dtypes")
    w12, w1032 = torch.ones(12, dtype=F32, device=DEV), torch.ones(1032, dtype=F32, device=DEV)
    refused(mk(F32, 12), None, w12, w12, torch.bfloat16, 12, "C = 12", b"C=12 must be a multiple of 8")
    refused(mk(F32, 1032), None, w1032, w1032, torch.bfloat16, 1032, "C = 1032", b"C=1032 must be a multiple of 8, at most")
    flat = torch.zeros(n * T * C + 8, dtype=torch.bfloat16, device=DEV)
    view = flat[4:4 + n * T * C].view(n, T, C)  # 8 bytes off a 16-byte boundary
    assert view.data_ptr() % 16 == 8
    refused(view, None, w, w, torch.bfloat16, C, "misaligned x", b"x / x_out not 16-byte aligned")
    refused(mk(torch.bfloat16, C), view, w, w, torch.bfloat16, C, "misaligned addend", b"addend not 16-byte aligned")
    wv = torch.ones(C + 4, dtype=F32, device=DEV)[2:2 + C]
    assert wv.data_ptr() % 16 == 8
    refused(mk(F32, C), None, wv, w, torch.bfloat16, C, "misaligned weight", b"weight_f32 / bias_f32 not 16-byte aligned")
    # 16-bit parameters have no dtype code in the C entry: the binding refuses them, before the library is called
    x = mk(torch.bfloat16, C)
    for bad_w, bad_b in ((w.bfloat16(), w), (w, w.half())):
        with pytest.raises(abi.TomeHipError, match="torch.float32"):
            (abi.drop_ln_amp(plan, x, bad_w, bad_b, EPS, torch.bfloat16) if drop
             else abi.merge_wavg_ln_amp(plan, x, None, bad_w, bad_b, EPS, torch.bfloat16))
    with pytest.raises(abi.TomeHipError, match="16-bit"):
        (abi.drop_ln_amp(plan, x, w, w, EPS, F32) if drop else abi.merge_wavg_ln_amp(plan, x, None, w, w, EPS, F32))


# ---------------------------------------------------------------------------------------------------------------------
# the public calls: tome.merge.merge_wavg_ln / drop_ln under torch.autocast
# ---------------------------------------------------------------------------------------------------------------------
def _count(monkeypatch, abi, name):
    calls = []
    real = getattr(abi, name)

    def counted(*args, **kw):
        calls.append(name)
        return real(*args, **kw)

    monkeypatch.setattr(abi, name, counted)
    return calls


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, F32], ids=["stream16", "stream32"])
def test_public_calls_take_the_entry_under_autocast(x_dtype, monkeypatch):
    abi, tm = _abi(), _tome()
    from tome import _ln
    n, T, C, r, half = 2, 20, 64, 4, torch.bfloat16
    gen = torch.Generator().manual_seed(9)
    metric = torch.randn(n, T, 16, generator=gen).to(DEV)
    x = torch.randn(n, T, C, generator=gen).to(x_dtype).to(DEV)
    res = torch.randn(n, T, C, generator=gen).to(half).to(DEV)
    size = torch.randint(1, 4, (n, T, 1), generator=gen).float().to(DEV)
    norm = torch.nn.LayerNorm(C, eps=EPS).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(1.0 + 0.1 * torch.randn(C, generator=gen))
        norm.bias.copy_(0.1 * torch.randn(C, generator=gen))
    merge, _ = tm.bipartite_soft_matching(metric, r)
    drop = tm.bipartite_soft_matching_drop(metric, r)
    merges, drops = _count(monkeypatch, abi, "merge_wavg_ln_amp"), _count(monkeypatch, abi, "drop_ln_amp")
    with torch.no_grad(), torch.autocast("cuda", dtype=half):
        mx, my, ms = tm.merge_wavg_ln(merge, x, size, norm, res, log_size=True)
        dx, dy = tm.drop_ln(drop, x, norm, res)
        assert (len(merges), len(drops)) == (1, 1)
        # the three steps of the parent's route
        s = x + res
        wx, ws = tm.merge_wavg(merge, s, size, log_size=True)
        wy = abi.add_layernorm_amp(wx, None, norm.weight, norm.bias, norm.eps, half)[1]
        wdx = drop(s)
        wdy = abi.add_layernorm_amp(wdx, None, norm.weight, norm.bias, norm.eps, half)[1]
    assert mx.dtype == x_dtype and my.dtype == half and torch.equal(mx, wx) and torch.equal(ms, ws)
    assert torch.equal(ms._tome_log, ws._tome_log) and torch.equal(dx, wdx)
    w, b = norm.weight.detach(), norm.bias.detach()
    lo.check(my, mx, w, b, EPS, dtype=half, signature=False, label="public merge")
    lo.check(wy, wx, w, b, EPS, dtype=half, signature=False, label="three steps merge")
    lo.check(dy, dx, w, b, EPS, dtype=half, signature=False, label="public drop")
    lo.check(wdy, wdx, w, b, EPS, dtype=half, signature=False, label="three steps drop")
    # not launched: grad wanted, autocast off, NATIVE_LN_AUTOCAST off
    with torch.autocast("cuda", dtype=half):
        tm.merge_wavg_ln(merge, x, size, norm, res)
        tm.drop_ln(drop, x, norm, res)
    with torch.no_grad():
        tm.merge_wavg_ln(merge, x.float(), size, norm, res.float())
        tm.drop_ln(drop, x.float(), norm, res.float())
    monkeypatch.setattr(_ln, "NATIVE_LN_AUTOCAST", False)
    with torch.no_grad(), torch.autocast("cuda", dtype=half):
        tm.merge_wavg_ln(merge, x, size, norm, res)
        tm.drop_ln(drop, x, norm, res)
    assert (len(merges), len(drops)) == (1, 1)
