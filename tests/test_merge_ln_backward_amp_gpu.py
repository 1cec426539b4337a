"""tome_merge_ln_backward_amp (k_merge_ln_rows_bwd_amp), the backward of the fused residual add + merge + LayerNorm
launches under autocast, on the GPU: the entry against the fp64 reference and derived bounds of
tests/merge_ln_bwd_amp_oracle.py at every width form, token layout, r and legal type combination; its bits (two runs,
the LayerNorm backward's own rows, zeros for dropped tokens, gx16); what it must not touch; its refusals; and the Function
and the two public calls of tome/merge.py behind tome._ln.NATIVE_MERGE_LN_AUTOCAST_BACKWARD."""
import pytest
import torch

import ln_amp_oracle as ao
import merge_ln_bwd_amp_oracle as mo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = ["bf16", "fp16"]
F32 = torch.float32
EPS = 1e-5
POISON = 0x7FC1  # a NaN pattern of both 16-bit formats (and, doubled, of fp32): a buffer that keeps it was not written
# 8 and 64 (four rows per wave, one lane iteration) plus one width per (slots per lane, rows per wave) form
WIDTHS = sorted({8, 64} | set(mo.FORM_WIDTHS.values()))
# (T, class token, distillation token): odd and even, with and without the protected tokens, several slabs per group
TOKENS = [(9, False, False), (9, True, False), (16, False, False), (16, True, True), (33, True, False), (33, False, False)]


def _mods():
    from tome import _abi, _ln
    from tome import merge as M
    return _abi, _ln, M


def _matching(M, n, T, cls, distill, r, seed):
    metric = torch.randn(n, T, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    merge, _ = M.bipartite_soft_matching(metric, r, class_token=cls, distill_token=distill)
    return merge


def _rows(plan, drop):
    return mo.rows_of_plan(plan.src_idx, plan.dst_idx, plan.unm_idx, plan.T, plan.r, distill=plan.distill_token, drop=drop)


def _dev(t):
    return None if t is None else t.to(DEV)


def _case(plan, C, x_dtype, a_dtype, half, size_dtype, seed, with_mul, with_in, drop):
    """CPU tensors of one call and its fp64 reference."""
    n, T, r = plan.n, plan.T, plan.r
    row_of, owns = _rows(plan, drop)
    gy, gi, xs, w, size = mo.make_tensors(n, T, r, C, x_dtype, a_dtype, half, size_dtype, seed, with_mul=with_mul,
                                          with_in=with_in, drop=drop)
    s_out = None if drop else mo.size_out_of(size, row_of, n, T, T - r, size_dtype)
    ref = mo.reference(gy, gi, xs, s_out, size, w, EPS, row_of)
    return dict(gy=gy, gi=gi, xs=xs, w=w, size=size, s_out=s_out, ref=ref, row_of=row_of, owns=owns)


def _run(_abi, plan, c, drop, want_weight=True, want_bias=True, want_gx16=False):
    return _abi.merge_ln_backward_amp(plan, _dev(c["gy"]), _dev(c["gi"]), _dev(c["xs"]), _dev(c["s_out"]), _dev(c["size"]),
                                      _dev(c["w"]), EPS, drop=drop, want_weight=want_weight, want_bias=want_bias,
                                      want_gx16=want_gx16)


def _r_values(T, cls, distill):
    return sorted({1, (T - int(cls) - int(distill)) // 2})


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_gradients_against_the_oracle(half, C):
    """Every width form; T = 9 / 16 / 33 with and without class and distillation tokens; n = 1 and 3; r = 1 and the clamp
    maximum (T = 16 without protected tokens: no unmerged even token is left, U = 0); every legal (stream, addend) dtype
    pair; sizes absent, fp32 and of the stream's dtype; gx_out given and NULL; merge and drop; with parameter gradients
    and frozen; gx16 on every fp32 stream: gx, dweight, dbias inside the oracle's bounds, gx16 the cast of gx."""
    _abi, _, M = _mods()
    k = 0
    seen, sizes, u0 = set(), set(), False
    combos = ao.combos(half)
    for T, cls, distill in TOKENS:
        for r in _r_values(T, cls, distill):
            n = (1, 3)[k % 2]
            x_dtype, a_dtype = combos[k % len(combos)]
            size_dtype, with_mul, with_in = (x_dtype, F32)[(k // 2) % 2], k % 3 != 2, k % 4 != 3
            k += 1
            plan = _matching(M, n, T, cls, distill, r, 100 * T + r).plan
            assert plan.r == r and plan.T == T
            u0 = u0 or (T + 1) // 2 - r == 0
            for drop in (False, True):
                seen.add((x_dtype, a_dtype))
                # (without in_mul a merge still divides by size', made in size_dtype)
                sizes.add("absent" if drop else "fp32" if size_dtype == F32 else "stream")
                c = _case(plan, C, x_dtype, a_dtype, half, size_dtype, 1000 * C + 10 * T + r, with_mul, with_in, drop)
                for params in (True, False):
                    gx, gx16, dw, db = _run(_abi, plan, c, drop, params, params, want_gx16=x_dtype == F32)
                    assert gx.dtype == x_dtype and (gx16 is None) == (x_dtype != F32)
                    assert (dw is None) == (not params) and (db is None) == (not params)
                    mo.check(f"C={C} T={T} n={n} r={r} cls={cls} distill={distill} drop={drop} x={x_dtype} a={a_dtype} "
                             f"size={size_dtype} in_mul={with_mul} gx_out={with_in} params={params} {half}", gx, gx16, dw, db,
                             c["ref"], half)
                    if drop:
                        gone = c["row_of"] < 0
                        assert int(gone.sum()) == n * r and float(gx.cpu()[gone].abs().max()) == 0.0
                        if gx16 is not None:
                            assert float(gx16.cpu()[gone].abs().max()) == 0.0
    assert seen == set(combos) and sizes == {"absent", "fp32", "stream"} and u0


def test_the_width_list_covers_every_form_of_the_dispatch():
    assert {mo.expected_form(C) for C in WIDTHS} == set(mo.FORM_WIDTHS) == {(3, 1), (3, 2), (3, 3), (3, 4)}


@pytest.mark.parametrize("drop", [False, True], ids=["merge", "drop"])
@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_a_destination_with_three_sources(half, drop):
    """A metric in which three even tokens equal one odd token: that destination receives three sources; its row enters
    dweight / dbias once and every one of its four tokens gets its own scale."""
    _abi, _, M = _mods()
    n, T, r, C = 3, 13, 4, 96
    metric = torch.randn(n, T, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    for t in (0, 2, 4):
        metric[:, t] = metric[:, 5]
    plan = M.bipartite_soft_matching(metric, r)[0].plan
    for x_dtype in (half, F32):
        c = _case(plan, C, x_dtype, half, half, x_dtype, 77, True, True, drop)
        if not drop:
            assert all(int(torch.bincount(c["row_of"][g]).max()) >= 4 for g in range(n)), "the metric did not fan in"
        else:
            assert bool((c["row_of"][:, (0, 2, 4)] < 0).all())
        gx, gx16, dw, db = _run(_abi, plan, c, drop, want_gx16=x_dtype == F32)
        mo.check(f"fan-in drop={drop} x={x_dtype} {half}", gx, gx16, dw, db, c["ref"], half)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def test_bits_are_the_same_on_every_run():
    _abi, _, M = _mods()
    half = torch.bfloat16
    for (n, T, r, C), drop, x_dtype in (((3, 13, 3, 96), False, half), ((5, 197, 16, 768), False, F32),
                                        ((2, 64, 6, 1024), True, F32), ((3, 33, 16, 384), False, half)):
        plan = _matching(M, n, T, T % 2 == 1, False, r, T).plan
        c = _case(plan, C, x_dtype, half, half, x_dtype, C + T, True, True, drop)
        a, b = (_run(_abi, plan, c, drop, want_gx16=x_dtype == F32) for _ in range(2))
        for ta, tb in zip(a, b):
            assert (ta is None and tb is None) or torch.equal(_bits(ta), _bits(tb))
        mo.check(f"determinism case {n, T, r, C} drop={drop}", *a, c["ref"], half)


def same_reduction_at_every_slab_row(C):
    """Does a row's statistics reduction have the same shape wherever the row sits among the R rows of a wave?  The slots
    of row rr are q = rr cpr .. rr cpr + cpr - 1, slot q in lane q % 64 of iteration q / 64; a lane adds its slots in
    iteration order and the wave total is a fixed tree over the lanes (tome_ln_rows.h).  R = 1: one place.  cpr a power of
    two: a row fills an aligned block of lanes of one iteration, the tree over that block is the same everywhere and
    what it meets outside is zeros.  cpr = 96 (C = 768, R = 2): row 1 is row 0 turned by 32 lanes, which swaps the two
    halves of the last addition.  Any other width (384: rows start at lanes 0, 48, 32, 16) groups the same values
    differently, and fp32 sums then differ in their last bits."""
    cpr = C // 8
    return min(4, 192 // cpr) == 1 or 64 % cpr == 0 or cpr == 96


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("half", ao.HALVES, ids=IDS)
def test_drop_gives_the_layernorm_backwards_own_rows(half, C):
    """With drop nothing is scaled: every kept token's gx row is row o(t) of tome_layernorm_backward_amp(gy, xs, gx_out)
    bit for bit -- both kernels call the same two rounds and write the same expression -- and every dropped row is zero.
    The LayerNorm launch is given every group's rows in token order (row o(t) at place t, so that a row sits in the same
    place of its wave's slab in both launches: that is all an fp32 reduction's bits depend on beyond the shared code);
    at the widths where the place does not matter (same_reduction_at_every_slab_row) also as it stands, [n, To, C]."""
    _abi, _, M = _mods()
    for (T, cls, distill), n in zip(TOKENS, (3, 1, 3, 1, 3, 1)):
        for r in _r_values(T, cls, distill):
            plan = _matching(M, n, T, cls, distill, r, 7 * T + r).plan
            for x_dtype in (half, F32):
                c = _case(plan, C, x_dtype, half, half, F32, 3 * C + T + r, False, (T + r) % 2 == 0, True)
                gx, gx16, _, _ = _run(_abi, plan, c, True, want_gx16=x_dtype == F32)
                kept = (c["row_of"] >= 0).to(DEV)
                o = c["row_of"].clamp_min(0).to(DEV)
                idx = o[..., None].expand(n, T, C)
                gather = lambda t: None if t is None else _dev(t).gather(1, idx)  # noqa: E731
                for g in range(n):
                    args = [None if t is None else t[g].contiguous() for t in map(gather, (c["gy"], c["xs"], c["gi"]))]
                    want, want16, _, _ = _abi.layernorm_backward_amp(args[0], args[1], args[2], _dev(c["w"]), EPS,
                                                                     want_weight=False, want_bias=False,
                                                                     want_gx16=x_dtype == F32)
                    assert torch.equal(_bits(gx[g][kept[g]]), _bits(want[kept[g]])), (T, r, g, x_dtype)
                    if gx16 is not None:
                        assert torch.equal(_bits(gx16[g][kept[g]]), _bits(want16[kept[g]]))
                if same_reduction_at_every_slab_row(C):
                    want, _, _, _ = _abi.layernorm_backward_amp(_dev(c["gy"]), _dev(c["xs"]), _dev(c["gi"]), _dev(c["w"]), EPS,
                                                                want_weight=False, want_bias=False)
                    assert torch.equal(_bits(gx[kept]), _bits(want.gather(1, idx)[kept])), (T, r, x_dtype)
                assert int((~kept).sum()) == n * r and not bool(_bits(gx[~kept]).any())
                if gx16 is not None:
                    assert torch.equal(_bits(gx16), _bits(gx.to(half))) and not bool(_bits(gx16[~kept]).any())


def _raw(_abi, plan, t, C, *, gy_code=None, x_code=None, r=None, row_map=True, drop=0, gx=None, gx16=None, dw=None,
         db=None, ws=None, size_code=None, **swap):
    """The entry itself, pointer by pointer.  t: device tensors gy, gi, xs, s_out, size, w (swap replaces some)."""
    L = _abi.lib()
    ptr = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    gy_code = _abi.DTYPES[t["gy"].dtype] if gy_code is None else gy_code
    x_code = _abi.DTYPES[t["xs"].dtype] if x_code is None else x_code
    size_code = (_abi.DTYPES[t["s_out"].dtype] if t["s_out"] is not None else x_code) if size_code is None else size_code
    t = dict(t, **swap)
    rm = _abi.plan_row_map(plan)
    rc = L.tome_merge_ln_backward_amp(ptr(t["gy"]), gy_code, ptr(t["gi"]), ptr(t["xs"]), x_code, ptr(t["s_out"]),
                                      ptr(t["size"]), size_code, plan.n, plan.T, C, plan.r if r is None else r,
                                      ptr(rm) if row_map else None, int(plan.distill_token), drop, ptr(t["w"]), EPS,
                                      ptr(gx), ptr(gx16), ptr(dw), ptr(db), ptr(ws), _abi._stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, L.tome_last_error().decode()


def _poisoned(*shape):
    return torch.full(shape, POISON, dtype=torch.int16, device=DEV)


def _device_case(plan, C, x_dtype, half, seed, drop=False):
    c = _case(plan, C, x_dtype, half, half, x_dtype, seed, True, True, drop)
    return c, {k: _dev(c[k]) for k in ("gy", "gi", "xs", "s_out", "size", "w")}


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, F32], ids=["bf16-stream", "fp32-stream"])
def test_frozen_and_partly_frozen_norms_touch_nothing_else(x_dtype):
    """Both parameter pointers NULL: the workspace keeps its bits and none is needed.  One of them NULL: the other
    gradient has the bits of the full call and nothing is written beside it."""
    _abi, _, M = _mods()
    half, C = torch.bfloat16, 96
    plan = _matching(M, 3, 13, False, False, 3, 5).plan
    c, t = _device_case(plan, C, x_dtype, half, 41)
    words = 2 if x_dtype == F32 else 1
    full = _run(_abi, plan, c, False)
    nbytes = _abi.lib().tome_merge_ln_backward_amp_workspace_bytes(plan.n, plan.T, C, _abi.DTYPES[x_dtype])
    assert nbytes >= 2 * C * 4
    ws = _poisoned(nbytes // 2)
    gx = _poisoned(plan.n, plan.T, C * words)
    rc, msg = _raw(_abi, plan, t, C, gx=gx, ws=ws)
    assert rc == 0, msg
    assert bool((ws == POISON).all()), "a frozen LayerNorm must not touch the workspace"
    assert torch.equal(gx, full[0].view(torch.int16)), "gx must not depend on the parameter work"
    rc, msg = _raw(_abi, plan, t, C, gx=gx)  # ... and needs none
    assert rc == 0, msg
    for which in (2, 3):
        guard = _poisoned(3, 2 * C)
        gx = _poisoned(plan.n, plan.T, C * words)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        rc, msg = _raw(_abi, plan, t, C, gx=gx, ws=ws, **{("dw", "db")[which - 2]: guard[1]})
        assert rc == 0, msg
        assert bool((guard[0] == POISON).all()) and bool((guard[2] == POISON).all())
        assert torch.equal(guard[1], full[which].view(torch.int16)) and torch.equal(gx, full[0].view(torch.int16))
    only_b = _run(_abi, plan, c, False, want_weight=False, want_bias=True)
    only_w = _run(_abi, plan, c, False, want_weight=True, want_bias=False)
    assert only_b[2] is None and only_w[3] is None
    assert torch.equal(only_b[3], full[3]) and torch.equal(only_w[2], full[2])


def test_more_groups_than_a_grid_dimension_holds():
    """n = 70000 groups of T = 4 tokens (r = 1, C = 8): the frozen form's group index spans blockIdx.y and .z, the
    parameter form walks 70000 slabs with 512 workgroups; every group's gx is checked, and dweight / dbias."""
    _abi, _, _ = _mods()
    n, T, r, C, half = 70000, 4, 1, 8, torch.bfloat16
    gen = torch.Generator().manual_seed(3)
    src = torch.randint(0, 2, (n, 1, 1), generator=gen)
    dst = torch.randint(0, 2, (n, 1, 1), generator=gen)
    dev = torch.device(DEV)
    plan = _abi.MatchPlan(n, T, r, False, False, src.to(dev), dst.to(dev), (1 - src).to(dev), None, None, dev)
    assert mo.form(n, T, C)[1] > 1
    c = _case(plan, C, F32, half, half, F32, 8, True, True, False)
    for params in (False, True):
        gx, gx16, dw, db = _run(_abi, plan, c, False, params, params, want_gx16=True)
        mo.check(f"n={n} params={params}", gx, gx16, dw, db, c["ref"], half)


def test_refusals_write_nothing():
    """Every refusal: status 1 (TOME_EINVAL), a text of its own that names the entry, and no buffer touched."""
    _abi, _, M = _mods()
    plan = _matching(M, 2, 8, False, False, 2, 1).plan
    bf, hf = torch.bfloat16, torch.float16
    L = _abi.lib()

    def refused(C=96, x_dtype=bf, **kw):
        c = _case(plan, 96, x_dtype, bf, bf, x_dtype, 3, True, True, False)
        t = {k: _dev(c[k]) for k in ("gy", "gi", "xs", "s_out", "size", "w")}
        if C != 96:
            t["w"] = torch.ones(C, device=DEV)
        swap = {k: (v(t) if callable(v) else v) for k, v in kw.pop("swap", {}).items()}
        bufs = dict(gx=_poisoned(2, 8, 4 * 1032), dw=_poisoned(4 * 1032), db=_poisoned(4 * 1032), ws=_poisoned(1 << 16))
        if kw.pop("with_gx16", False):
            bufs["gx16"] = _poisoned(2, 8, 1032)
        for k in kw.pop("without", ()):
            bufs[k] = None
        rc, msg = _raw(_abi, plan, t, C, **bufs, **kw, **swap)
        assert rc == 1 and "tome_merge_ln_backward_amp" in msg, (C, kw, rc, msg)
        for buf in bufs.values():
            assert buf is None or bool((buf == POISON).all()), (C, kw, "a refused call wrote")
        return msg

    off = lambda v: torch.cat((v.reshape(-1), v.reshape(-1)[:8]))[4:4 + v.numel()].view(v.shape)  # noqa: E731 (8 bytes off)
    texts = [refused(1032), refused(100), refused(r=0), refused(r=5), refused(row_map=False),
             refused(gy_code=_abi.DTYPES[F32]), refused(x_code=_abi.DTYPES[hf]), refused(with_gx16=True),
             refused(size_code=_abi.DTYPES[hf]), refused(drop=1), refused(without=("ws",)),
             refused(swap=dict(xs=lambda t: off(t["xs"]))), refused(swap=dict(xs=None)), refused(swap=dict(w=None))]
    assert "1024" in texts[0] and "C % 8" in texts[1] and "r=0" in texts[2] and "r=5" in texts[3]
    assert "row_map" in texts[4] and "unsupported dtypes" in texts[5] and "unsupported dtypes" in texts[6]
    assert "gx16 belongs to an fp32 stream" in texts[7] and "sizes must be of x's dtype or fp32" in texts[8]
    assert "drop takes no scales" in texts[9] and "workspace" in texts[10] and "16-byte aligned" in texts[11]
    assert "null buffer" in texts[12] and "null buffer" in texts[13]
    assert len(set(texts[:12])) == 12, "each refusal has a text of its own"
    code = _abi.DTYPES
    assert L.tome_merge_ln_backward_amp_workspace_bytes(2, 8, 1032, code[bf]) == 0
    assert L.tome_merge_ln_backward_amp_workspace_bytes(2, 8, 100, code[F32]) == 0
    assert L.tome_merge_ln_backward_amp_workspace_bytes(2, 8, 96, 7) == 0
    assert L.tome_merge_ln_backward_amp_workspace_bytes(2, 8, 96, code[F32]) > 0


def _norm(C):
    torch.manual_seed(C)
    n = torch.nn.LayerNorm(C, eps=EPS)
    with torch.no_grad():
        n.weight.add_(0.1 * torch.randn(C))
        n.bias.add_(0.1 * torch.randn(C))
    return n.to(DEV)


@pytest.mark.parametrize("x_dtype,a_dtype", [(torch.bfloat16, torch.bfloat16), (F32, torch.bfloat16), (F32, F32)],
                         ids=["bf16+bf16", "fp32+bf16", "fp32+fp32"])
def test_function_of_the_public_calls(x_dtype, a_dtype, monkeypatch):
    """merge_wavg_ln and drop_ln under bf16 autocast with the switch on: the forward is the inference launch bit for bit,
    x and a residual of the stream's dtype receive one tensor, a 16-bit residual of an fp32 stream the cast of it, the
    gradients are inside the oracle's bounds; with the switch off the grad_fn is not the Function's."""
    _abi, _ln, M = _mods()
    half = torch.bfloat16
    n, T, C, r = 2, 16, 96, 5
    merge = _matching(M, n, T, False, False, r, 4)
    norm = _norm(C)
    gen = torch.Generator().manual_seed(1)
    x0 = torch.randn(n, T, C, generator=gen).to(x_dtype).to(DEV)
    res0 = (0.5 * torch.randn(n, T, C, generator=gen)).to(a_dtype).to(DEV)
    size = torch.randint(1, 4, (n, T, 1), generator=gen).float().to(DEV)
    g_x = torch.randn(n, T - r, C, generator=gen).to(x_dtype).to(DEV)
    g_y = torch.randn(n, T - r, C, generator=gen).to(half).to(DEV)
    with torch.autocast("cuda", dtype=half):
        x, res = x0.clone().requires_grad_(True), res0.clone().requires_grad_(True)
        xo, y, so = M.merge_wavg_ln(merge, x, size, norm, residual=res)
        assert "_MergeLnAmpFunction" not in type(xo.grad_fn).__name__, "off by default"
        monkeypatch.setattr(_ln, "NATIVE_MERGE_LN_AUTOCAST_BACKWARD", True)
        x, res = x0.clone().requires_grad_(True), res0.clone().requires_grad_(True)
        x_out, y, size_out = M.merge_wavg_ln(merge, x, size, norm, residual=res, log_size=True)
        assert type(x_out.grad_fn).__name__ == "_MergeLnAmpFunctionBackward" and y.grad_fn is x_out.grad_fn
        assert y.dtype == half and x_out.dtype == x_dtype and size_out.grad_fn is None
        assert torch.equal(_abi.log_of_size(size_out), size_out.log())
        fx, fy, fs = _abi.merge_wavg_ln_amp(merge.plan, x0, size, norm.weight.detach(), norm.bias.detach(), norm.eps, half,
                                            addend=res0)
        assert torch.equal(x_out, fx) and torch.equal(y, fy) and torch.equal(size_out, fs), "forward = the inference launch"
        assert torch.equal(xo, fx) and torch.equal(so, fs), "the three steps store the same stream"
        torch.autograd.backward([x_out, y], [g_x, g_y])
        assert x.grad.dtype == x_dtype and res.grad.dtype == a_dtype and norm.weight.grad.dtype == F32
        assert torch.equal(res.grad, x.grad.to(a_dtype)), "the residual receives gx, cast once where it is 16-bit"
        # (the entry is held to the oracle above; the Function is held to the entry, bit for bit)
        want = _abi.merge_ln_backward_amp(merge.plan, g_y, g_x, x_out.detach(), size_out, size, norm.weight, EPS,
                                          want_gx16=a_dtype != x_dtype)
        assert torch.equal(x.grad, want[0]) and torch.equal(norm.weight.grad, want[2]) and torch.equal(norm.bias.grad, want[3])
        if a_dtype != x_dtype:
            assert torch.equal(res.grad, want[1])
        # nothing read y: the merge alone, zeros for the parameters
        x, res = x0.clone().requires_grad_(True), res0.clone().requires_grad_(True)
        norm.zero_grad(set_to_none=True)
        x_out, y, _ = M.merge_wavg_ln(merge, x, size, norm, residual=res)
        x_out.backward(g_x)
        assert torch.equal(x.grad, _abi.merge_backward(merge.plan, g_x, out_div=size_out, in_mul=size))
        assert float(norm.weight.grad.abs().max()) == 0.0 and float(norm.bias.grad.abs().max()) == 0.0
        # drop_ln
        drop = M.bipartite_soft_matching_drop(torch.randn(n, T, 32, device=DEV,
                                                          generator=torch.Generator(device=DEV).manual_seed(7)), r)
        x, res = x0.clone().requires_grad_(True), res0.clone().requires_grad_(True)
        norm.zero_grad(set_to_none=True)
        xd, yd = M.drop_ln(drop, x, norm, residual=res)
        assert type(xd.grad_fn).__name__ == "_MergeLnAmpFunctionBackward" and yd.grad_fn is xd.grad_fn
        fx, fy = _abi.drop_ln_amp(drop.plan, x0, norm.weight.detach(), norm.bias.detach(), norm.eps, half, addend=res0)
        assert torch.equal(xd, fx) and torch.equal(yd, fy)
        torch.autograd.backward([xd, yd], [g_x, g_y])
        want = _abi.merge_ln_backward_amp(drop.plan, g_y, g_x, xd.detach(), None, None, norm.weight, EPS, drop=True)
        assert torch.equal(x.grad, want[0]) and torch.equal(res.grad, want[0].to(a_dtype))
        assert torch.equal(norm.weight.grad, want[2]) and torch.equal(norm.bias.grad, want[3])
        gone = (_rows(drop.plan, True)[0] < 0).to(DEV)
        assert int(gone.sum()) == n * r and float(x.grad[gone].abs().max()) == 0.0
        # a frozen norm and x without grad: the residual alone
        frozen = _norm(C).requires_grad_(False)
        x, res = x0.clone(), res0.clone().requires_grad_(True)
        xf, yf, _ = M.merge_wavg_ln(merge, x, size, frozen, residual=res)
        assert type(xf.grad_fn).__name__ == "_MergeLnAmpFunctionBackward"
        torch.autograd.backward([xf, yf], [g_x, g_y])
        assert res.grad is not None and res.grad.dtype == a_dtype and bool(torch.isfinite(res.grad.float()).all())
        # without a gradient wanted: no graph
        with torch.no_grad():
            nx, ny, ns = M.merge_wavg_ln(merge, x0, size, norm, residual=res0)
        assert nx.grad_fn is None and torch.equal(nx, x_out.detach())
