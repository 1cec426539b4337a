"""The mixed-precision add + LayerNorm kernels on the GPU (tome_add_layernorm_amp / k_add_ln_rows,
tome_layernorm_backward_amp / k_ln_rows_bwd_amp): every width and every legal type combination against the bounds of
tests/ln_amp_oracle.py, the stored sum bit for bit, launches whose workgroups walk several slabs, bit-level properties
and every refusal."""
import pytest
import torch

import ln_amp_oracle as ao
import ln_bwd_oracle as bo
import ln_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
IDS = ["bf16", "fp16"]
F32 = torch.float32
G, N = 2, 9  # 2 groups of 9 rows: no multiple of R = 2, 4 nor of a workgroup's 4 R rows, two workgroups at R <= 2


def _abi():
    from tome import _abi
    return _abi


def _dev(t):
    return None if t is None else t.to(DEV)


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _kept(groups, rows):
    keep = torch.ones(groups, rows, dtype=torch.bool)
    keep[:, 0] = False
    return torch.nonzero(keep.reshape(-1)).reshape(-1)


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_forward_at_every_width_in_every_type_combination(half):
    """C = 8 .. 1024 (every (slots per lane, rows per wave) form), 2 x 9 rows, the five legal (stream, addend) dtype
    pairs, plain and skip_first: x' bit-equal to torch's own sum, every element of y inside ln_oracle's bound."""
    abi = _abi()
    forms, worst = set(), 0.0
    kept = _kept(G, N)
    for C in lo.WIDTHS:
        nit, R, _ = lo.expected_form("add_layernorm", C)
        forms.add((nit, R))
        w, b = ao.affine(C, 7 + C)
        wd, bd = _dev(w), _dev(b)
        for x_dtype, a_dtype in ao.combos(half):
            x, a = ao.forward_inputs((G, N, C), x_dtype, a_dtype, 10 * C)
            want = ao.stored_sum(x, a)
            tag = f"C={C} x={x_dtype} a={a_dtype} y={half}"
            for skip in (False, True):
                xo, y = abi.add_layernorm_amp(_dev(x), _dev(a), wd, bd, EPS, half, skip_first=skip)
                assert xo.dtype == x_dtype and y.dtype == half and y.shape == (G, N - skip, C), tag
                assert torch.equal(_bits(xo.cpu()), _bits(want)), f"{tag}: the stored sum is not torch's x + addend"
                if skip:
                    worst = max(worst, lo.check(y, want.reshape(-1, C)[kept], w, b, EPS, dtype=half, R=R, out_index=kept,
                                                label=tag + " skip_first")["worst"])
                else:
                    worst = max(worst, lo.check(y, want, w, b, EPS, dtype=half, R=R, label=tag)["worst"])
    assert forms == {(3, 1), (3, 2), (3, 3), (3, 4)} == lo.forms_that_exist("add_layernorm")
    print(f"tome_add_layernorm_amp {half}: worst err / bound {worst:.3f}")


def _backward(abi, gy, xs, gi, w, skip, params, gx16):
    return abi.layernorm_backward_amp(_dev(gy), _dev(xs), _dev(gi), _dev(w), EPS, skip_first=skip, want_weight=params,
                                      want_bias=params, want_gx16=gx16)


def _class_rows_pass_through(gx, gx16, gi, half, label):
    want = torch.zeros_like(gx[:, 0]) if gi is None else gi[:, 0].to(gx.device)
    assert torch.equal(_bits(gx[:, 0].contiguous()), _bits(want.contiguous())), f"{label}: class rows of gx are not gx_in's bits"
    if gx16 is not None:
        assert torch.equal(_bits(gx16[:, 0].contiguous()), _bits(want.to(half).contiguous())), label


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_backward_at_every_width_for_both_streams(half):
    """C = 8 .. 1024, 2 x 9 rows, 16-bit and fp32 stream, with and without gx_in, plain and skip_first, with the
    parameter gradients and frozen, gx16 whenever the stream is fp32: gx (u of its own dtype), fp32 dweight / dbias
    inside the bounds, gx16 = gx.to(dtype) bit for bit, class rows moved as bits."""
    abi = _abi()
    forms = set()
    for C in lo.WIDTHS:
        forms.add((3, bo.form(G * N, C)[0]))
        for x_dtype in (half, F32):
            for skip, with_in in ((False, True), (True, False), (True, True), (False, False)):
                gy, xs, gi, w = ao.backward_inputs((G, N, C), x_dtype, half, 7 * C + 2 * skip + with_in, skip_first=skip,
                                                   with_in=with_in, far=(C // 8) % 4 != 0,
                                                   grad_scale=1e-3 if (C // 8) % 3 == 0 else 1.0)
                ref = ao.reference(gy, xs, gi, w, EPS, skip_first=skip)
                for params in (False, True):
                    gx, gx16, dw, db = _backward(abi, gy, xs, gi, w, skip, params, x_dtype == F32)
                    label = f"C={C} x={x_dtype} skip={skip} gx_in={with_in} params={params} {half}"
                    assert gx.dtype == x_dtype and (dw is None) == (not params) and (db is None) == (not params)
                    ao.check_backward(label, gx, gx16, dw, db, ref, half)
                    if skip:
                        _class_rows_pass_through(gx, gx16, gi, half, label)
    assert forms == {(3, 1), (3, 2), (3, 3), (3, 4)}


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_launches_whose_workgroups_walk_several_slabs(half):
    """7 x 1201 = 8407 rows: more than 512 workgroups' worth at C = 64, 768 and 1024, so every wave of the backward walks
    2 .. 5 slabs and the last workgroups run out of rows part-way; the forward's grid is as many workgroups long."""
    abi = _abi()
    shape = (7, 1201)
    kept = _kept(*shape)
    for C in (64, 768, 1024):
        R, spw, parts = bo.form(shape[0] * shape[1], C)
        assert spw >= 2 and parts <= bo.MAX_PARTS
        w, b = ao.affine(C, 7 + C)
        for x_dtype, a_dtype in ((half, half), (F32, half)):
            x, a = ao.forward_inputs((*shape, C), x_dtype, a_dtype, 3 * C)
            want = ao.stored_sum(x, a)
            xo, y = abi.add_layernorm_amp(_dev(x), _dev(a), _dev(w), _dev(b), EPS, half, skip_first=True)
            assert torch.equal(_bits(xo.cpu()), _bits(want))
            lo.check(y, want.reshape(-1, C)[kept], w, b, EPS, dtype=half, R=R, out_index=kept, label=f"long forward C={C}")
            gy, xs, gi, wt = ao.backward_inputs((*shape, C), x_dtype, half, 31 * C, skip_first=True)
            ref = ao.reference(gy, xs, gi, wt, EPS, skip_first=True)
            for params in (False, True):
                gx, gx16, dw, db = _backward(abi, gy, xs, gi, wt, True, params, x_dtype == F32)
                ao.check_backward(f"long C={C} x={x_dtype} params={params} {half}", gx, gx16, dw, db, ref, half)
                _class_rows_pass_through(gx, gx16, gi, half, f"long C={C}")


def test_same_bits_on_every_run_and_a_frozen_norm_needs_no_workspace(monkeypatch):
    abi = _abi()
    half = torch.bfloat16
    for C, shape, x_dtype in ((96, (5, 77), F32), (768, (9, 601), F32), (1024, (2, 333), half)):
        gy, xs, gi, w = ao.backward_inputs((*shape, C), x_dtype, half, C, skip_first=True)
        first = _backward(abi, gy, xs, gi, w, True, True, x_dtype == F32)
        again = _backward(abi, gy, xs, gi, w, True, True, x_dtype == F32)
        for ta, tb in zip(first, again):
            assert (ta is None and tb is None) or torch.equal(_bits(ta), _bits(tb))
        asked = []
        orig = abi._workspace
        monkeypatch.setattr(abi, "_workspace", lambda *args: asked.append(args) or orig(*args))
        gx, gx16, dw, db = _backward(abi, gy, xs, gi, w, True, False, False)
        monkeypatch.setattr(abi, "_workspace", orig)
        assert not asked and dw is None and db is None and gx16 is None
        assert torch.equal(_bits(gx), _bits(first[0])), "gx must not depend on the parameter work or on gx16"
        x, a = ao.forward_inputs((*shape, C), x_dtype, half, C)
        wb = [_dev(t) for t in ao.affine(C, C)]
        one = abi.add_layernorm_amp(_dev(x), _dev(a), *wb, EPS, half)
        two = abi.add_layernorm_amp(_dev(x), _dev(a), *wb, EPS, half)
        assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(one, two))


def _raw_forward(abi, x, a, w, b, xo, y, skip=0, groups=G, group_rows=N, C=None, y_code=None):
    C = x.shape[-1] if C is None else C
    code = abi.DTYPES
    return abi.lib().tome_add_layernorm_amp(
        x.data_ptr(), code[x.dtype], abi._ptr(a), 0 if a is None else code[a.dtype], groups, group_rows, skip, C,
        w.data_ptr(), b.data_ptr(), EPS, abi._ptr(xo), y.data_ptr(), code[y.dtype] if y_code is None else y_code,
        abi._stream(x.device))


def _raw_backward(abi, gy, xs, gi, w, gx, gx16, dw, db, ws, skip=0, groups=G, group_rows=N, C=None):
    C = xs.shape[-1] if C is None else C
    code = abi.DTYPES
    return abi.lib().tome_layernorm_backward_amp(
        gy.data_ptr(), code[gy.dtype], xs.data_ptr(), abi._ptr(gi), code[xs.dtype], groups, group_rows, skip, C,
        w.data_ptr(), EPS, gx.data_ptr(), abi._ptr(gx16), abi._ptr(dw), abi._ptr(db), abi._ptr(ws), abi._stream(xs.device))


@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_every_output_element_is_written_and_nothing_else(half):
    """Outputs filled with NaN beforehand hold no NaN afterwards; without an addend x_out is left alone; the class rows of
    a skip_first y do not exist (y is compact)."""
    abi = _abi()
    nan = lambda shape, dtype: torch.full(shape, float("nan"), dtype=dtype, device=DEV)  # noqa: E731
    for C in (8, 200, 768, 1024):
        w, b = [_dev(t) for t in ao.affine(C, C)]
        for x_dtype, a_dtype in ao.combos(half):
            x, a = [_dev(t) for t in ao.forward_inputs((G, N, C), x_dtype, a_dtype, C)]
            for skip in (0, 1):
                xo, y = nan((G, N, C), x_dtype), nan((G, N - skip, C), half)
                assert _raw_forward(abi, x, a, w, b, xo, y, skip) == 0
                assert bool(torch.isfinite(y).all()) and bool(torch.isnan(xo).all() if a is None else torch.isfinite(xo).all())
        for x_dtype in (half, F32):
            for skip in (0, 1):
                gy, xs, gi, wt = [_dev(t) for t in ao.backward_inputs((G, N, C), x_dtype, half, C, skip_first=bool(skip))]
                gx, dw, db = nan((G, N, C), x_dtype), nan((C,), F32), nan((C,), F32)
                gx16 = nan((G, N, C), half) if x_dtype == F32 else None
                nbytes = abi.lib().tome_layernorm_backward_amp_workspace_bytes(G * N, C, abi.DTYPES[x_dtype])
                assert nbytes > 0
                ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)  # (fp32 NaN patterns)
                assert _raw_backward(abi, gy, xs, gi, wt, gx, gx16, dw, db, ws, skip) == 0
                for t in (gx, gx16, dw, db):
                    assert t is None or bool(torch.isfinite(t).all()), (C, x_dtype, skip)
                # one parameter gradient alone, the other buffer untouched
                dw2, db2 = nan((C,), F32), nan((C,), F32)
                assert _raw_backward(abi, gy, xs, gi, wt, gx, None, dw2, None, ws, skip) == 0
                assert torch.equal(dw2, dw) and bool(torch.isnan(db2).all())


def test_refusals():
    abi = _abi()
    L = abi.lib()
    code = abi.DTYPES
    C = 64
    mk = lambda dtype, *shape: torch.ones(*shape, dtype=dtype, device=DEV)  # noqa: E731
    w, b = mk(F32, C), mk(F32, C)
    for xd, ad, yd in ao.illegal_combos():
        rc = _raw_forward(abi, mk(xd, G, N, C), None if ad is None else mk(ad, G, N, C), w, b, mk(xd, G, N, C), mk(yd, G, N, C))
        assert rc != 0, (xd, ad, yd)
        assert b"tome_add_layernorm_amp" in L.tome_last_error()
    x, y = mk(F32, G, N, 1032), mk(torch.bfloat16, G, N, 1032)
    w2 = mk(F32, 1032)
    assert _raw_forward(abi, x, None, w2, w2, None, y) != 0                      # C > 1024
    assert _raw_forward(abi, x, None, w2, w2, None, y, C=12) != 0                # C % 8
    x, y = mk(F32, G, N, C), mk(torch.bfloat16, G, N, C)
    assert _raw_forward(abi, x, None, w, b, None, y, y_code=7) != 0              # no such dtype
    assert _raw_forward(abi, x, x, w, b, None, y) != 0                           # an addend needs x_out
    assert _raw_forward(abi, x, None, w, b, None, y, skip=1, groups=G * N, group_rows=1) != 0
    assert _raw_forward(abi, x, None, w, b, None, y, groups=0) != 0
    assert _raw_forward(abi, x, None, w, b, None, y) == 0
    with pytest.raises(abi.TomeHipError):
        abi.add_layernorm_amp(x, None, w.bfloat16(), b, EPS, torch.bfloat16)     # master weights are fp32
    with pytest.raises(abi.TomeHipError):
        abi.add_layernorm_amp(x, None, w, b, EPS, F32)
    with pytest.raises(abi.TomeHipError):
        abi.add_layernorm_amp(x.cpu(), None, w, b, EPS, torch.bfloat16)

    half = torch.bfloat16
    gy, xs, gx, gx16 = mk(half, G, N, C), mk(F32, G, N, C), mk(F32, G, N, C), mk(half, G, N, C)
    dw = mk(F32, C)
    ws = torch.empty(L.tome_layernorm_backward_amp_workspace_bytes(G * N, C, code[F32]), dtype=torch.uint8, device=DEV)
    assert _raw_backward(abi, gy, xs, None, w, gx, gx16, dw, dw, ws) == 0
    assert _raw_backward(abi, gy, xs, None, w, gx, None, dw, None, None) != 0    # parameter work without a workspace
    assert b"workspace" in L.tome_last_error()
    assert _raw_backward(abi, gy, xs, None, w, gx, None, None, None, None) == 0  # a frozen norm needs none
    assert _raw_backward(abi, xs, xs, None, w, gx, None, None, None, None) != 0  # fp32 gy
    assert _raw_backward(abi, gy, mk(torch.float16, G, N, C), None, w, mk(torch.float16, G, N, C), None, None, None, None) != 0
    xs16 = mk(half, G, N, C)
    assert _raw_backward(abi, gy, xs16, None, w, mk(half, G, N, C), gx16, None, None, None) != 0  # gx16: fp32 streams only
    assert _raw_backward(abi, gy, xs, None, w, gx, None, None, None, None, C=12) != 0
    assert _raw_backward(abi, gy, xs, None, w, gx, None, None, None, None, C=1032) != 0
    assert _raw_backward(abi, gy, xs, None, w, gx, None, None, None, None, skip=1, groups=G * N, group_rows=1) != 0
    assert _raw_backward(abi, gy, xs, None, w, gx, None, None, None, None, groups=0) != 0
    for rows, width, dt in ((0, C, 0), (G * N, 12, 0), (G * N, 1032, 1), (G * N, C, 5), (2 ** 31, C, 0)):
        assert L.tome_layernorm_backward_amp_workspace_bytes(rows, width, dt) == 0
    with pytest.raises(abi.TomeHipError):
        abi.layernorm_backward_amp(gy, xs16, None, w, EPS, want_gx16=True)
    with pytest.raises(abi.TomeHipError):
        abi.layernorm_backward_amp(xs, xs, None, w, EPS)
    with pytest.raises(abi.TomeHipError):
        abi.layernorm_backward_amp(gy, xs, None, w.bfloat16(), EPS)
    with pytest.raises(abi.TomeHipError):
        abi.layernorm_backward_amp(gy[:, 1:], xs, None, w, EPS)
