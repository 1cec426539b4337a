"""Every channel and row accounted for in the fused LayerNorm kernels: y_out of tome_add_layernorm (with and without
addend, skip_first), tome_add_layernorm_regrouped, tome_merge_wavg_ln and tome_merge_wavg_regrouped_ln against the fp64
LayerNorm of the rows as stored, within one rounding of the format plus a derived fp32 allowance (tests/ln_oracle.py;
tests/test_ln_oracle_cpu.py shows that this rejects a chunk left out of a row's statistics, a chunk normalised with
the row next to it in the wave, a weight chunk of the wrong column, a second rounding, a misplaced eps).

Inputs: rows whose means differ by many standard deviations from the rows they share a wave with (signature rows, both
signs) and scaled N(0,1) rows; both 16-bit formats; every width C = 8 .. 1024 for the add entries and the plain merge
entry, a subset that reaches every launch form for the regrouped ones.  x_out and the sizes are compared bit for bit
with the unfused entry points on the same inputs.  Every shape is a legal input."""
import pytest
import torch

import ln_oracle as lo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-6
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
KINDS = ["sig+", "sig-", "plain"]

ROW_COUNTS = [1, 2, 3, 4, 5, 7, 257, 1001]                      # the last wave partly filled for every R
SKIP_SHAPES = {2: (1, 2), 3: (1, 3), 4: (2, 2), 5: (1, 5), 7: (1, 7), 257: (1, 257), 1001: (7, 143)}  # rows -> (B, N)
REGROUP_ADD = [(2, 8, 196), (3, 4, 36), (1, 2, 1), (2, 3, 50), (5, 1, 7), (1, 3, 2)]  # (B, F, P); 151 and 7 rows: no R divides
SUBSET = [8, 24, 40, 128, 200, 392, 400, 512, 520, 768, 776, 1000, 1024]
# (n, T, r, class token): r = 1 and r = clamp, EAGER (r <= 64 and 8 r >= T) and not, r > 64 (the general edge waves)
MERGE_CASES = [(3, 16, 1, False), (3, 16, 8, False), (3, 17, 8, True), (3, 8, 1, False), (2, 40, 3, True),
               (1, 197, 98, True)]
REGROUP_MERGE = [(2, 4, 36, 6), (1, 8, 49, 24), (2, 2, 40, 3), (1, 3, 9, 1)]  # (B, F, P, r)


def _reached(entry, widths, cases):
    forms, inside = set(), set()
    for C in widths:
        for addend in ((False,) if entry.startswith("add") else (False, True)):
            for T, r in cases:
                nit, R, eager = lo.expected_form(entry, C, addend, T, r)
                forms.add((nit, R, eager))
                inside.add(lo.boundary_inside_iteration(C, R))
    return forms, inside


# the grids must reach every launch form: checked here, at collection, on any machine
for _entry, _widths, _cases in (("add_layernorm", lo.WIDTHS, [(0, 0)]), ("add_layernorm_skip_first", lo.WIDTHS, [(0, 0)]),
                                ("add_layernorm_regrouped", SUBSET, [(0, 0)]),
                                ("merge_wavg_ln", lo.WIDTHS, [(T, r) for _, T, r, _ in MERGE_CASES]),
                                ("merge_wavg_regrouped_ln", SUBSET, [(P, r) for _, _, P, r in REGROUP_MERGE])):
    _forms, _inside = _reached(_entry, _widths, _cases)
    _eager = (False,) if _entry.startswith("add") else (False, True)
    assert _forms == {(nit, R, e) for nit, R in lo.forms_that_exist(_entry) for e in _eager}, (_entry, sorted(_forms))
    assert {True, False} <= _inside, (_entry, "row boundaries inside and between lane iterations")


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
    """a residual of the rows' own kind: grid noise of the row's class (the sum stays a signature row) or half-size
    plain rows"""
    if kind == "plain":
        return (0.5 * lo.plain_rows(shape, dtype, seed).double()).to(dtype).to(DEV)
    return lo.signature_rows(shape, dtype, seed, 1, klass, 0.5, offset=False).to(DEV)


def _affine(C, dtype):
    w, b = lo.affine(C, dtype, 7 + C)
    return w.to(DEV), b.to(DEV)


def _summary(capsys, name, worst):
    capsys.readouterr()
    print(f"{name}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_add_layernorm_every_width(dtype, kind, capsys):
    """tome_add_layernorm with an addend, without one, and skip_first (compacted: the rows must be the right ones, which
    their signatures decide), rows = 1 .. 1001, C = 8 .. 1024."""
    abi = _abi()
    sig = kind != "plain"
    worst = 0.0
    for C in lo.WIDTHS:
        _, R, _ = lo.expected_form("add_layernorm", C)
        w, b = _affine(C, dtype)
        x_all = _rows(kind, (ROW_COUNTS[-1], C), dtype, 10 * C + 1)
        a_all = _addend(kind, (ROW_COUNTS[-1], C), dtype, 10 * C + 2)
        for rows in ROW_COUNTS:
            x, a = x_all[:rows].contiguous(), a_all[:rows].contiguous()
            tag = f"add_layernorm {kind} rows={rows} C={C}"
            xo, yo = abi.add_layernorm(x, a, w, b, EPS)
            assert torch.equal(xo, x + a), tag
            if sig:
                lo.assert_rows_in_a_wave_differ(xo, rows, tag)
            worst = max(worst, lo.check(yo, xo, w, b, EPS, R=R, signature=sig, label=tag)["worst"])
            keep = xo.clone()
            xn, yn = abi.add_layernorm(xo, None, w, b, EPS)
            assert xn is xo and torch.equal(xo, keep), tag
            if not torch.equal(yn, yo):
                worst = max(worst, lo.check(yn, xo, w, b, EPS, R=R, signature=sig, label=tag + " no addend")["worst"])
            if rows in SKIP_SHAPES:
                B, N = SKIP_SHAPES[rows]
                for add in (a, None):
                    xin = x if add is not None else xo
                    xs, ys = abi.add_layernorm(xin.view(B, N, C), None if add is None else add.view(B, N, C), w, b, EPS,
                                               skip_first=True)
                    assert torch.equal(xs.reshape(rows, C), xo) and tuple(ys.shape) == (B, N - 1, C) and ys.is_contiguous()
                    kept = torch.arange(rows).view(B, N)[:, 1:].reshape(-1)
                    if rows > 7 and torch.equal(ys, yo.view(B, N, C)[:, 1:]):
                        continue
                    worst = max(worst, lo.check(ys, xo[kept.to(DEV)], w, b, EPS, R=R, out_index=kept, signature=sig,
                                                label=tag + f" skip_first addend={add is not None}")["worst"])
    _summary(capsys, f"tome_add_layernorm(+skip_first) {kind} {dtype}", worst)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_add_layernorm_regrouped(dtype, kind, capsys):
    """tome_add_layernorm_regrouped: every row of the regrouped y is the LayerNorm of the row the rearrangement puts
    there, the class row of a clip in front of each of its frames."""
    abi = _abi()
    sig = kind != "plain"
    worst = 0.0
    for C in SUBSET:
        _, R, _ = lo.expected_form("add_layernorm_regrouped", C)
        w, b = _affine(C, dtype)
        for B, F, P in REGROUP_ADD:
            N = 1 + P * F
            tag = f"add_layernorm_regrouped {kind} B={B} F={F} P={P} C={C}"
            x = _rows(kind, (B, N, C), dtype, 20 * C + N)
            a = _addend(kind, (B, P * F, C), dtype, 20 * C + N + 1, torch.arange(B * N).view(B, N)[:, 1:])
            x1, y = abi.add_layernorm_regrouped(x, a, F, w, b, EPS)
            assert torch.equal(x1, torch.cat((x[:, :1], x[:, 1:] + a), 1)), tag
            # row of x1 behind every row of y: '(b t) (1 + p)' <- class row of clip b | token 1 + p * F + t of clip b
            idx = torch.arange(B * N).view(B, N)
            tok = idx[:, 1:].view(B, P, F).permute(0, 2, 1).reshape(B * F, P)
            src = torch.cat((idx[:, :1].expand(B, F).reshape(B * F, 1), tok), 1).reshape(-1)
            assert tuple(y.shape) == (B * F, 1 + P, C), tag
            stored = x1.view(B * N, C)[src.to(DEV)]
            if sig:
                lo.assert_rows_in_a_wave_differ(x1.view(B * N, C), B * N, tag)
            worst = max(worst, lo.check(y, stored, w, b, EPS, R=R, out_index=src, signature=sig, label=tag)["worst"])
            is_cls = torch.zeros(B * F, 1 + P, dtype=torch.bool)
            is_cls[:, 0] = True
            lo.check(y, stored, w, b, EPS, R=R, out_index=src, signature=sig, rows=is_cls, label=tag + " class rows")
            yc = y[:, 0].view(B, F, C)
            assert torch.equal(yc, yc[:, :1].expand(B, F, C)), tag
    _summary(capsys, f"tome_add_layernorm_regrouped {kind} {dtype}", worst)


def _plan_rows(plan, T):
    row, recv = lo.merged_row_of_token(plan.src_idx, plan.dst_idx, plan.unm_idx, T)
    return row, recv


def _check_merged(y, stored, w, b, R, recv, sig, tag, To):
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
def test_merge_wavg_ln_every_width(dtype, kind, capsys):
    """tome_merge_wavg_ln: without addend (six chunks per lane) and with (three), sizes None and 1 .. 4, x_out_bias,
    class token, EAGER and not, r = 1, r = clamp, r > 64; x_out and the sizes bit-equal to tome_merge_wavg of the
    pre-added tokens.  Tokens carry the signature class of the OUTPUT row they end up in, so the rows of one wave
    differ whatever the matching is -- asserted on the returned x_out.  With x_out_bias the normalised row is the
    x_out of the same call without the bias."""
    abi, tm = _abi(), _tome()
    sig = kind != "plain"
    worst = 0.0
    gen = torch.Generator().manual_seed(11)
    for n, T, r, cls in MERGE_CASES:
        metric = torch.randn(n, T, 32, generator=torch.Generator().manual_seed(100 * T + r)).to(DEV)
        merge, _ = tm.bipartite_soft_matching(metric, r, cls)
        plan, To = merge.plan, T - merge.plan.r
        row, recv = _plan_rows(plan, T)
        size = torch.randint(1, 5, (n, T, 1), generator=gen).to(dtype).to(DEV)
        for C in lo.WIDTHS:
            w, b = _affine(C, dtype)
            x = _rows(kind, (n, T, C), dtype, 30 * C + T + r, row)
            a = _addend(kind, (n, T, C), dtype, 30 * C + T + r + 1, row)
            ob = (0.3 * torch.randn(C, generator=gen)).to(dtype).to(DEV)
            for addend, sz, bias in ((None, None, False), (a, size, False), (a, None, True), (None, size, True)):
                _, R, eager = lo.expected_form("merge_wavg_ln", C, addend is not None, T, plan.r)
                tag = (f"merge_wavg_ln {kind} T={T} r={plan.r} cls={cls} C={C} addend={addend is not None} "
                       f"sizes={sz is not None} bias={bias} eager={eager}")
                want_x, want_s = tm.merge_wavg(merge, x if addend is None else x + addend, sz)
                x0, y0, s0 = abi.merge_wavg_ln(plan, x, sz, w, b, EPS, addend=addend)
                assert torch.equal(x0, want_x) and torch.equal(s0, want_s), tag
                y = y0
                if bias:
                    bx, y, bs = abi.merge_wavg_ln(plan, x, sz, w, b, EPS, addend=addend, out_bias=ob)
                    assert torch.equal(bx, x0 + ob) and torch.equal(bs, s0), tag
                if sig:
                    lo.assert_rows_in_a_wave_differ(x0.view(n * To, C), To, tag)
                worst = max(worst, _check_merged(y, x0.view(n * To, C), w, b, R, recv.reshape(-1), sig, tag, To))
    _summary(capsys, f"tome_merge_wavg_ln {kind} {dtype}", worst)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_merge_wavg_regrouped_ln(dtype, kind, capsys):
    """tome_merge_wavg_regrouped_ln on the interleaved layout: no addend, `addend`, `addend_grouped` + `cls_addend`,
    x_out_bias; the class rows on their own."""
    abi, tm = _abi(), _tome()
    sig = kind != "plain"
    worst = worst_cls = 0.0
    gen = torch.Generator().manual_seed(13)
    for B, F, P, r in REGROUP_MERGE:
        n, N = B * F, 1 + P * F
        metric = torch.randn(n, P, 16, generator=torch.Generator().manual_seed(100 * P + r)).to(DEV)
        merge, _ = tm.bipartite_soft_matching(metric, r)
        plan, To = merge.plan, P - merge.plan.r
        row, recv = _plan_rows(plan, P)
        # class of token 1 + p * F + f of clip b: the output row of token p of group b * F + f; class rows: class 5
        klass = torch.cat((torch.full((B, 1), 5), row.view(B, F, P).permute(0, 2, 1).reshape(B, P * F)), 1)
        size = torch.randint(1, 5, (n, P, 1), generator=gen).to(dtype).to(DEV)
        for C in SUBSET:
            w, b = _affine(C, dtype)
            x = _rows(kind, (B, N, C), dtype, 40 * C + P + r, klass)
            res = _addend(kind, (B, N, C), dtype, 40 * C + P + r + 1, klass)
            junk = _rows(kind, (n, 1, C), dtype, 40 * C + 3)
            grouped = torch.cat((junk, res[:, 1:].view(B, P, F, C).permute(0, 2, 1, 3).reshape(n, P, C)), 1).contiguous()
            ob = (0.3 * torch.randn(C, generator=gen)).to(dtype).to(DEV)
            for addend, sz in ((None, size), (res, None), (res, size)):
                _, R, eager = lo.expected_form("merge_wavg_regrouped_ln", C, addend is not None, P, plan.r)
                tag = (f"merge_wavg_regrouped_ln {kind} B={B} F={F} P={P} r={plan.r} C={C} addend={addend is not None} "
                       f"sizes={sz is not None} eager={eager}")
                want_x, want_s = abi.merge_wavg_regrouped(plan, x if addend is None else x + addend, sz, F, has_cls=True)
                kw = {} if addend is None else dict(addend=addend)
                x0, y0, s0 = abi.merge_wavg_regrouped(plan, x, sz, F, has_cls=True, ln=(w, b, EPS), **kw)
                assert torch.equal(x0, want_x) and torch.equal(s0, want_s), tag

                def groups(t):  # [B, 1 + To * F, C] -> rows in (group, output row) order
                    return t[:, 1:].view(B, To, F, C).permute(0, 2, 1, 3).reshape(n * To, C)

                def check_all(y, what):
                    nonlocal worst, worst_cls
                    worst = max(worst, _check_merged(groups(y), groups(x0), w, b, R, recv.reshape(-1), sig,
                                                     f"{tag} {what}", To))
                    worst_cls = max(worst_cls, lo.check(y[:, 0], x0[:, 0], w, b, EPS, R=1, signature=sig,
                                                        label=f"{tag} {what} class rows")["worst"])

                if sig:
                    lo.assert_rows_in_a_wave_differ(groups(x0), To, tag)
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
    print(f"tome_merge_wavg_regrouped_ln {kind} {dtype}: worst err / bound {worst:.3f}, class rows {worst_cls:.3f}")
