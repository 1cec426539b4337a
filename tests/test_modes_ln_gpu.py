"""The reduction + LayerNorm launch in the modes beside plain merge: tome_drop_ln, tome_drop_regrouped_ln, and the hybrid
(threshold) flags through tome_merge_wavg_ln / tome_merge_wavg_regrouped_ln.  x_out (and the sizes) bit for bit against the
unfused entries on the pre-added tokens, y_out against the fp64 LayerNorm of the rows as stored within tests/ln_oracle.py's
bound (the inputs, `check` and the bound of tests/test_layernorm_accounting_gpu.py), on every row; class rows, streamed
rows and rows built by the edge waves each on their own.  Small shapes: r = 1 and r = clamp, class and distillation token,
more than one wave per group, r > 64; the 13 widths reach both chunk counts per lane and one to four rows per wave."""
import pytest
import torch

import ln_oracle as lo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-6
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
KINDS = ["sig+", "sig-", "plain"]
SUBSET = [8, 24, 40, 128, 200, 392, 400, 512, 520, 768, 776, 1000, 1024]
# (n, T, r, class token, distillation token)
FLAT = [(3, 16, 1, False, False), (3, 16, 8, False, False), (3, 17, 8, True, False), (2, 40, 3, True, False),
        (1, 197, 98, True, False)]
DROP_FLAT = FLAT + [(2, 18, 4, True, True)]
HYBRID_FLAT = FLAT + [(2, 150, 70, False, False)]  # r > 64 without a class token as well: the general edge waves
REGROUPED = [(2, 4, 36, 6), (1, 8, 49, 24), (2, 2, 40, 3), (1, 3, 9, 1)]  # (B, F, P, r)
HYBRID_REGROUPED = REGROUPED + [(1, 2, 150, 70)]


def form(C, addend):
    """(NIT, R) of the drop launch (launch_merge_rows): three chunks per lane with an addend on rows of at most 192
    chunks, else six; R rows per wave.  The merge entries pick theirs the same way (lo.expected_form)."""
    cpr = C // 8
    nit = 3 if (addend and cpr <= 3 * lo.WAVE) else 6
    return nit, min(4, nit * lo.WAVE // cpr)


# checked at collection, on any machine: the widths reach both forms and every row count
_forms = {form(C, a) for C in SUBSET for a in (False, True)}
assert {nit for nit, _ in _forms} == {3, 6} and {R for _, R in _forms} == {1, 2, 3, 4}, sorted(_forms)
assert all(form(C, a) == lo.expected_form("merge_wavg_ln", C, a)[:2] for C in SUBSET for a in (False, True))
assert any(r > 64 for _, _, r, _, _ in HYBRID_FLAT) and any(r > 64 for _, _, _, r in HYBRID_REGROUPED)


def _abi():
    from tome import _abi
    return _abi


def _tome():
    from tome import merge as tm
    return tm


def _rows(kind, shape, dtype, seed, klass=None):
    if kind == "plain":
        return lo.plain_rows(shape, dtype, seed).to(DEV)
    return lo.signature_rows(shape, dtype, seed, 1 if kind == "sig+" else -1, klass).to(DEV)


def _addend(kind, shape, dtype, seed, klass=None):
    if kind == "plain":
        return (0.5 * lo.plain_rows(shape, dtype, seed).double()).to(dtype).to(DEV)
    return lo.signature_rows(shape, dtype, seed, 1, klass, 0.5, offset=False).to(DEV)


def _affine(C, dtype):
    w, b = lo.affine(C, dtype, 7 + C)
    return w.to(DEV), b.to(DEV)


def _metric(n, T, seed):
    return torch.randn(n, T, 32, generator=torch.Generator().manual_seed(seed))


def _drop_rows(plan, T):
    """Output row of every token a drop keeps ([n, T]; the dropped tokens: row 0, they are never stored)."""
    unm = plan.unm_idx.cpu().long().reshape(plan.n, -1)
    n, U = unm.shape
    row = torch.zeros((n, T), dtype=torch.long)
    i, j = torch.arange(U), torch.arange(T // 2)
    if plan.distill_token:
        a_row, b_row = torch.where(i == 0, 0, i + 1), torch.where(j == 0, 1, U + j)
    else:
        a_row, b_row = i, U + j
    row[:, 1::2] = b_row[None, :]
    row[torch.arange(n)[:, None], 2 * unm] = a_row[None, :].expand(n, U)
    return row


def _hybrid_threshold(metric, plan, class_token):
    """The median of the selected edges' scores (the best cosine similarity of every selected even token to an odd one),
    in fp64 on the CPU from the metric: about half of the edges fall below it."""
    m = metric.double()
    m = m / m.norm(dim=-1, keepdim=True)
    scores = m[:, 0::2] @ m[:, 1::2].transpose(1, 2)
    best = scores.max(-1).values
    picked = best.gather(1, plan.src_idx.cpu().long().reshape(plan.n, -1)).reshape(-1).sort().values
    return float(picked[(picked.numel() - 1) // 2])


def _hybrid(metric, r, class_token):
    tm = _tome()
    plain, _ = tm.bipartite_soft_matching(metric.to(DEV), r, class_token)
    thr = _hybrid_threshold(metric, plain.plan, class_token)
    merge, _ = tm.bipartite_soft_matching_hybrid(metric.to(DEV), r, class_token, False, "hybrid", thr)
    keep = merge.plan.edge_keep
    assert keep is not None and 0 < int(keep.sum()) < keep.numel(), (int(keep.sum()), keep.numel(), thr)
    assert torch.equal(merge.plan.src_idx, plain.plan.src_idx)
    return merge


def _check_sets(y, stored, w, b, R, recv, sig, tag, To):
    """streamed rows (no source) and rows built by the edge waves, each set on its own and non-empty"""
    out_index = torch.arange(To).repeat(stored.shape[0] // To)
    worst = 0.0
    for name, rows in (("streamed", ~recv), ("edge", recv)):
        assert bool(rows.any()), f"{tag}: no {name} rows"
        worst = max(worst, lo.check(y, stored, w, b, EPS, R=R, out_index=out_index, rows=rows, signature=sig,
                                    label=f"{tag} {name}")["worst"])
    return worst


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_drop_ln(dtype, kind, capsys):
    """tome_drop_ln: no addend / addend, with and without x_out_bias; x_out bit-equal to tome_drop of the pre-added tokens,
    y_out the LayerNorm of the stored row on every row, the same bits on a second run."""
    abi, tm = _abi(), _tome()
    sig = kind != "plain"
    worst = 0.0
    gen = torch.Generator().manual_seed(17)
    for n, T, r, cls, distill in DROP_FLAT:
        drop = tm.bipartite_soft_matching_drop(_metric(n, T, 100 * T + r).to(DEV), r, cls, distill)
        plan, To = drop.plan, T - drop.plan.r
        row = _drop_rows(plan, T)
        for C in SUBSET:
            w, b = _affine(C, dtype)
            x = _rows(kind, (n, T, C), dtype, 50 * C + T + r, row)
            a = _addend(kind, (n, T, C), dtype, 50 * C + T + r + 1, row)
            ob = (0.3 * torch.randn(C, generator=gen)).to(dtype).to(DEV)
            for addend in (None, a):
                _, R = form(C, addend is not None)
                tag = f"drop_ln {kind} T={T} r={plan.r} cls={cls} distill={distill} C={C} addend={addend is not None}"
                want = abi.drop(plan, x if addend is None else x + addend)
                x0, y0 = abi.drop_ln(plan, x, w, b, EPS, addend=addend)
                assert tuple(x0.shape) == (n, To, C) and torch.equal(x0, want), tag
                if sig:
                    lo.assert_rows_in_a_wave_differ(x0.view(n * To, C), To, tag)
                idx = torch.arange(To).repeat(n)
                worst = max(worst, lo.check(y0, x0, w, b, EPS, R=R, out_index=idx, signature=sig, label=tag)["worst"])
                x1, y1 = abi.drop_ln(plan, x, w, b, EPS, addend=addend)
                assert torch.equal(x1, x0) and torch.equal(y1, y0), tag + " second run"
                bx, by = abi.drop_ln(plan, x, w, b, EPS, addend=addend, out_bias=ob)
                assert torch.equal(bx, x0 + ob), tag + " out_bias"
                if not torch.equal(by, y0):  # y is the norm of the row WITHOUT the bias
                    worst = max(worst, lo.check(by, x0, w, b, EPS, R=R, out_index=idx, signature=sig,
                                                label=tag + " out_bias")["worst"])
    capsys.readouterr()
    print(f"tome_drop_ln {kind} {dtype}: worst err / bound {worst:.3f}")


def _groups(t, B, F, To, C):
    """[B, 1 + To * F, C] -> rows in (group, output row) order"""
    return t[:, 1:].view(B, To, F, C).permute(0, 2, 1, 3).reshape(B * F * To, C)


def _regrouped_inputs(kind, dtype, B, F, P, C, row, seed):
    n, N = B * F, 1 + P * F
    # class of token 1 + p * F + f of clip b: the output row of token p of group b * F + f; class rows: class 5
    klass = torch.cat((torch.full((B, 1), 5), row.view(B, F, P).permute(0, 2, 1).reshape(B, P * F)), 1)
    x = _rows(kind, (B, N, C), dtype, seed, klass)
    res = _addend(kind, (B, N, C), dtype, seed + 1, klass)
    junk = _rows(kind, (n, 1, C), dtype, seed + 2)  # the grouped residual's own class rows: never read
    grouped = torch.cat((junk, res[:, 1:].view(B, P, F, C).permute(0, 2, 1, 3).reshape(n, P, C)), 1).contiguous()
    return x, res, grouped


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_drop_regrouped_ln(dtype, kind, capsys):
    """tome_drop_regrouped_ln on the interleaved layout: no addend, `addend`, `addend_grouped` + `cls_addend` (junk in the
    grouped tensor's class rows), x_out_bias; the class rows on their own."""
    abi, tm = _abi(), _tome()
    sig = kind != "plain"
    worst = worst_cls = 0.0
    gen = torch.Generator().manual_seed(19)
    for B, F, P, r in REGROUPED:
        n = B * F
        drop = tm.bipartite_soft_matching_drop(_metric(n, P, 100 * P + r).to(DEV), r)
        plan, To = drop.plan, P - drop.plan.r
        row = _drop_rows(plan, P)
        idx = torch.arange(To).repeat(n)
        for C in SUBSET:
            w, b = _affine(C, dtype)
            x, res, grouped = _regrouped_inputs(kind, dtype, B, F, P, C, row, 60 * C + P + r)
            ob = (0.3 * torch.randn(C, generator=gen)).to(dtype).to(DEV)
            for addend in (None, res):
                _, R = form(C, addend is not None)
                tag = f"drop_regrouped_ln {kind} B={B} F={F} P={P} r={plan.r} C={C} addend={addend is not None}"
                want = abi.drop_regrouped(plan, x if addend is None else x + addend, F, has_cls=True)
                kw = {} if addend is None else dict(addend=addend)
                x0, y0 = abi.drop_regrouped(plan, x, F, has_cls=True, ln=(w, b, EPS), **kw)
                assert torch.equal(x0, want), tag
                if sig:
                    lo.assert_rows_in_a_wave_differ(_groups(x0, B, F, To, C), To, tag)

                def check_all(y, what):
                    nonlocal worst, worst_cls
                    worst = max(worst, lo.check(_groups(y, B, F, To, C), _groups(x0, B, F, To, C), w, b, EPS, R=R,
                                                out_index=idx, signature=sig, label=f"{tag} {what}")["worst"])
                    worst_cls = max(worst_cls, lo.check(y[:, 0], x0[:, 0], w, b, EPS, R=1, signature=sig,
                                                        label=f"{tag} {what} class rows")["worst"])

                check_all(y0, "")
                variants = [dict(kw, out_bias=ob)]
                if addend is not None:
                    g = dict(addend_grouped=grouped, cls_addend=res[:, :1].contiguous())
                    variants += [g, dict(g, out_bias=ob)]
                for v in variants:
                    vx, vy = abi.drop_regrouped(plan, x, F, has_cls=True, ln=(w, b, EPS), **v)
                    assert torch.equal(vx, x0 + ob if "out_bias" in v else x0), (tag, sorted(v))
                    if not torch.equal(vy, y0):
                        check_all(vy, "+".join(sorted(v)))
    capsys.readouterr()
    print(f"tome_drop_regrouped_ln {kind} {dtype}: worst err / bound {worst:.3f}, class rows {worst_cls:.3f}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hybrid_merge_wavg_ln(dtype, kind, capsys):
    """tome_merge_wavg_ln with the hybrid flags: a destination with an edge below the threshold loses its own
    round16(x + addend) term and its own size.  x_out and the sizes bit-equal to merge_wavg(hybrid merge, x + addend,
    size); y_out on the streamed rows and on the edge rows."""
    abi, tm = _abi(), _tome()
    sig = kind != "plain"
    worst = 0.0
    gen = torch.Generator().manual_seed(23)
    for n, T, r, cls, _ in HYBRID_FLAT:
        merge = _hybrid(_metric(n, T, 100 * T + r), r, cls)
        plan, To = merge.plan, T - merge.plan.r
        row, recv = lo.merged_row_of_token(plan.src_idx, plan.dst_idx, plan.unm_idx, T)
        size = torch.randint(1, 5, (n, T, 1), generator=gen).to(dtype).to(DEV)
        for C in SUBSET:
            w, b = _affine(C, dtype)
            x = _rows(kind, (n, T, C), dtype, 70 * C + T + r, row)
            a = _addend(kind, (n, T, C), dtype, 70 * C + T + r + 1, row)
            ob = (0.3 * torch.randn(C, generator=gen)).to(dtype).to(DEV)
            for addend, sz, bias in ((None, None, False), (a, size, False), (a, None, True), (None, size, True)):
                _, R, eager = lo.expected_form("merge_wavg_ln", C, addend is not None, T, plan.r)
                tag = (f"hybrid merge_wavg_ln {kind} T={T} r={plan.r} cls={cls} C={C} addend={addend is not None} "
                       f"sizes={sz is not None} bias={bias} eager={eager}")
                want_x, want_s = tm.merge_wavg(merge, x if addend is None else x + addend, sz)
                x0, y0, s0 = abi.merge_wavg_ln(plan, x, sz, w, b, EPS, addend=addend)
                assert torch.equal(x0, want_x) and torch.equal(s0, want_s), tag
                y = y0
                if bias:
                    bx, y, bs = abi.merge_wavg_ln(plan, x, sz, w, b, EPS, addend=addend, out_bias=ob)
                    assert torch.equal(bx, x0 + ob) and torch.equal(bs, s0), tag
                worst = max(worst, _check_sets(y, x0.view(n * To, C), w, b, R, recv.reshape(-1), sig, tag, To))
    capsys.readouterr()
    print(f"hybrid tome_merge_wavg_ln {kind} {dtype}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hybrid_merge_wavg_regrouped_ln(dtype, kind, capsys):
    """tome_merge_wavg_regrouped_ln with the hybrid flags: `addend`, `addend_grouped` + `cls_addend`, x_out_bias; bit-equal
    to the regrouped entry without LayerNorm on the pre-added tokens."""
    abi = _abi()
    sig = kind != "plain"
    worst = worst_cls = 0.0
    gen = torch.Generator().manual_seed(29)
    for B, F, P, r in HYBRID_REGROUPED:
        n = B * F
        merge = _hybrid(_metric(n, P, 100 * P + r), r, False)
        plan, To = merge.plan, P - merge.plan.r
        row, recv = lo.merged_row_of_token(plan.src_idx, plan.dst_idx, plan.unm_idx, P)
        size = torch.randint(1, 5, (n, P, 1), generator=gen).to(dtype).to(DEV)
        for C in SUBSET:
            w, b = _affine(C, dtype)
            x, res, grouped = _regrouped_inputs(kind, dtype, B, F, P, C, row, 80 * C + P + r)
            ob = (0.3 * torch.randn(C, generator=gen)).to(dtype).to(DEV)
            for addend, sz in ((None, size), (res, None), (res, size)):
                _, R, eager = lo.expected_form("merge_wavg_regrouped_ln", C, addend is not None, P, plan.r)
                tag = (f"hybrid merge_wavg_regrouped_ln {kind} B={B} F={F} P={P} r={plan.r} C={C} "
                       f"addend={addend is not None} sizes={sz is not None} eager={eager}")
                want_x, want_s = abi.merge_wavg_regrouped(plan, x if addend is None else x + addend, sz, F, has_cls=True)
                kw = {} if addend is None else dict(addend=addend)
                x0, y0, s0 = abi.merge_wavg_regrouped(plan, x, sz, F, has_cls=True, ln=(w, b, EPS), **kw)
                assert torch.equal(x0, want_x) and torch.equal(s0, want_s), tag

                def check_all(y, what):
                    nonlocal worst, worst_cls
                    worst = max(worst, _check_sets(_groups(y, B, F, To, C), _groups(x0, B, F, To, C), w, b, R,
                                                   recv.reshape(-1), sig, f"{tag} {what}", To))
                    worst_cls = max(worst_cls, lo.check(y[:, 0], x0[:, 0], w, b, EPS, R=1, signature=sig,
                                                        label=f"{tag} {what} class rows")["worst"])

                check_all(y0, "")
                variants = [dict(kw, out_bias=ob)]
                if addend is not None:
                    g = dict(addend_grouped=grouped, cls_addend=res[:, :1].contiguous())
                    variants += [g, dict(g, out_bias=ob)]
                for v in variants:
                    vx, vy, vs = abi.merge_wavg_regrouped(plan, x, sz, F, has_cls=True, ln=(w, b, EPS), **v)
                    assert torch.equal(vx, x0 + ob if "out_bias" in v else x0) and torch.equal(vs, s0), (tag, sorted(v))
                    if not torch.equal(vy, y0):
                        check_all(vy, "+".join(sorted(v)))
    capsys.readouterr()
    print(f"hybrid tome_merge_wavg_regrouped_ln {kind} {dtype}: worst err / bound {worst:.3f}, class rows {worst_cls:.3f}")
