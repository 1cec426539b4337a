"""tome_merge_ln_backward (k_merge_ln_rows_bwd), the backward of the fused residual add + merge + LayerNorm launches,
on the GPU: the entry against the fp64 reference and derived bound of tests/merge_ln_bwd_oracle.py at every width form,
token layout and r; what it must not touch; its refusals; the Function and the two public calls of tome/merge.py; and
patched models that train through it with the switch tome.patch._common.TRAIN_FUSED_LN on."""
import copy

import pytest
import torch

import ln_bwd_oracle as bo
import merge_ln_bwd_oracle as mo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
EPS = 1e-5
POISON = 0x7FC1  # a NaN pattern of both 16-bit formats: a buffer that keeps it was not written
WIDTHS = sorted({8, 96, 1024} | set(mo.FORM_WIDTHS.values()))
# (T, class token, distillation token): even, odd with a class token, both protected tokens, a partial last slab
TOKENS = [(8, False, False), (9, True, False), (10, True, True), (13, False, False)]


def _mods():
    from tome import _abi, _ln
    from tome import merge as M
    from tome.patch import _common
    return _abi, _ln, M, _common


def _matching(M, n, T, cls, distill, r, seed, metric=None):
    if metric is None:
        metric = torch.randn(n, T, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    merge, _ = M.bipartite_soft_matching(metric, r, class_token=cls, distill_token=distill)
    return merge


def _rows(plan, drop):
    return mo.rows_of_plan(plan.src_idx, plan.dst_idx, plan.unm_idx, plan.T, plan.r, distill=plan.distill_token, drop=drop)


def _dev(t):
    return None if t is None else t.to(DEV)


def _case(plan, C, dtype, size_dtype, seed, with_mul, with_in, drop):
    """CPU tensors of one call and its fp64 reference."""
    n, T, r = plan.n, plan.T, plan.r
    row_of, owns = _rows(plan, drop)
    gy, gi, xs, w, size = mo.make_tensors(n, T, r, C, dtype, size_dtype, seed, with_mul=with_mul, with_in=with_in, drop=drop)
    s_out = None if drop else mo.size_out_of(size, row_of, n, T, T - r, size_dtype)
    ref = mo.reference(gy, gi, xs, s_out, size, w, EPS, row_of)
    return dict(gy=gy, gi=gi, xs=xs, w=w, size=size, s_out=s_out, ref=ref, row_of=row_of, owns=owns)


def _run(_abi, plan, c, drop, params=True, want_weight=None, want_bias=None):
    return _abi.merge_ln_backward(plan, _dev(c["gy"]), _dev(c["gi"]), _dev(c["xs"]), _dev(c["s_out"]), _dev(c["size"]),
                                  _dev(c["w"]), EPS, drop=drop, want_weight=params if want_weight is None else want_weight,
                                  want_bias=params if want_bias is None else want_bias)


def _r_values(T, cls, distill):
    top = (T - int(cls) - int(distill)) // 2
    return sorted({1, max(1, top // 2), top})


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_gradients_against_the_oracle(dtype, C):
    """Every width form, T = 8 / 9 (class token) / 10 (class + distillation token) / 13 (partial last slab), n = 1 and 3,
    r = 1, a middle value and the clamp maximum; sizes in the token dtype and in fp32, in_mul given and NULL, gx_out given
    and NULL, merge and drop, with and without parameter gradients: gx, dweight, dbias inside the oracle's bound."""
    _abi, _, M, _ = _mods()
    k = 0
    combos = set()
    for T, cls, distill in TOKENS:
        for r in _r_values(T, cls, distill):
            n = (1, 3)[k % 2]
            size_dtype, with_mul, with_in = (dtype, torch.float32)[(k // 2) % 2], k % 3 != 2, k % 5 != 4
            k += 1
            combos.add((size_dtype, with_mul))
            plan = _matching(M, n, T, cls, distill, r, 100 * T + r).plan
            assert plan.r == r and plan.T == T
            for drop in (False, True):
                c = _case(plan, C, dtype, size_dtype, 1000 * C + 10 * T + r, with_mul, with_in, drop)
                for params in (True, False):
                    gx, dw, db = _run(_abi, plan, c, drop, params)
                    assert (dw is None) == (not params) and (db is None) == (not params)
                    mo.check(f"C={C} T={T} n={n} r={r} cls={cls} distill={distill} drop={drop} size={size_dtype} "
                             f"in_mul={with_mul} gx_out={with_in} params={params} {dtype}", gx, dw, db, c["ref"], dtype)
                    if drop:
                        gone = c["row_of"] < 0
                        assert int(gone.sum()) == n * r and float(gx.cpu()[gone].abs().max()) == 0.0
    assert combos == {(dtype, True), (dtype, False), (torch.float32, True), (torch.float32, False)}


def test_the_width_list_covers_every_form_of_the_dispatch():
    assert {mo.expected_form(C) for C in WIDTHS} == set(mo.FORM_WIDTHS) == {(3, 1), (3, 2), (3, 3), (3, 4)}
    assert all(mo.expected_form(C) == form for form, C in mo.FORM_WIDTHS.items())


@pytest.mark.parametrize("drop", [False, True], ids=["merge", "drop"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_a_destination_with_three_sources(dtype, drop):
    """A metric in which three even tokens equal one odd token: that destination receives three sources; its row enters
    dweight / dbias once and every one of its four tokens gets its own scale."""
    _abi, _, M, _ = _mods()
    n, T, r, C = 3, 13, 4, 96
    metric = torch.randn(n, T, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    for t in (0, 2, 4):
        metric[:, t] = metric[:, 5]
    plan = _matching(M, n, T, False, False, r, 0, metric=metric).plan
    c = _case(plan, C, dtype, dtype, 77, True, True, drop)
    if not drop:
        assert all(int(torch.bincount(c["row_of"][g]).max()) >= 4 for g in range(n)), "the metric did not fan in"
    else:
        assert bool((c["row_of"][:, (0, 2, 4)] < 0).all())
    gx, dw, db = _run(_abi, plan, c, drop)
    mo.check(f"fan-in drop={drop} {dtype}", gx, dw, db, c["ref"], dtype)


def _raw(_abi, plan, t, C, *, x_code=None, r=None, row_map=True, drop=0, gx=None, dw=None, db=None, ws=None,
         size_code=None):
    """The entry itself, pointer by pointer.  t: device tensors gy, gi, xs, s_out, size, w."""
    L = _abi.lib()
    ptr = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    x_code = _abi.DTYPES[t["xs"].dtype] if x_code is None else x_code
    size_code = (_abi.DTYPES[t["s_out"].dtype] if t["s_out"] is not None else x_code) if size_code is None else size_code
    rm = _abi.plan_row_map(plan)
    rc = L.tome_merge_ln_backward(ptr(t["gy"]), ptr(t["gi"]), ptr(t["xs"]), x_code, ptr(t["s_out"]), ptr(t["size"]),
                                  size_code, plan.n, plan.T, C, plan.r if r is None else r, ptr(rm) if row_map else None,
                                  int(plan.distill_token), drop, ptr(t["w"]), EPS, ptr(gx), ptr(dw), ptr(db), ptr(ws),
                                  _abi._stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, L.tome_last_error().decode()


def _poisoned(*shape):
    return torch.full(shape, POISON, dtype=torch.int16, device=DEV)


def _device_case(plan, C, dtype, seed, drop=False):
    c = _case(plan, C, dtype, dtype, seed, True, True, drop)
    return c, {k: _dev(c[k]) for k in ("gy", "gi", "xs", "s_out", "size", "w")}


def test_frozen_and_partly_frozen_norms_touch_nothing_else():
    """Both parameter pointers NULL: the workspace keeps its bits.  One of them NULL: the other gradient has the bits of
    the full call and nothing is written beside it."""
    _abi, _, M, _ = _mods()
    dtype, C = torch.bfloat16, 96
    plan = _matching(M, 3, 13, False, False, 3, 5).plan
    c, t = _device_case(plan, C, dtype, 41)
    full = _run(_abi, plan, c, False)
    nbytes = _abi.lib().tome_merge_ln_backward_workspace_bytes(plan.n, plan.T, C)
    assert nbytes >= 2 * C * 4
    ws = _poisoned(nbytes // 2)
    gx = _poisoned(plan.n, plan.T, C)
    rc, msg = _raw(_abi, plan, t, C, gx=gx, ws=ws)
    assert rc == 0, msg
    assert bool((ws == POISON).all()), "a frozen LayerNorm must not touch the workspace"
    assert torch.equal(gx, full[0].view(torch.int16)), "gx must not depend on the parameter work"
    rc, msg = _raw(_abi, plan, t, C, gx=gx)  # ... and needs none
    assert rc == 0, msg
    for which in (1, 2):
        guard = _poisoned(3, C)
        gx = _poisoned(plan.n, plan.T, C)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        rc, msg = _raw(_abi, plan, t, C, gx=gx, ws=ws, **{("dw", "db")[which - 1]: guard[1]})
        assert rc == 0, msg
        assert bool((guard[0] == POISON).all()) and bool((guard[2] == POISON).all())
        assert torch.equal(guard[1], full[which].view(torch.int16)) and torch.equal(gx, full[0].view(torch.int16))
    only_b = _run(_abi, plan, c, False, want_weight=False, want_bias=True)
    only_w = _run(_abi, plan, c, False, want_weight=True, want_bias=False)
    assert only_b[1] is None and only_w[2] is None
    assert torch.equal(only_b[2], full[2]) and torch.equal(only_w[1], full[1])
    rc, msg = _raw(_abi, plan, t, C, gx=gx, dw=guard[1])  # parameter gradients without a workspace
    assert rc != 0 and "workspace" in msg


def test_bits_are_the_same_on_every_run():
    _abi, _, M, _ = _mods()
    for (n, T, r, C), drop in (((3, 13, 3, 96), False), ((5, 197, 16, 768), False), ((2, 64, 6, 1024), True)):
        plan = _matching(M, n, T, T % 2 == 1, False, r, T).plan
        c = _case(plan, C, torch.bfloat16, torch.bfloat16, C + T, True, True, drop)
        a, b = _run(_abi, plan, c, drop), _run(_abi, plan, c, drop)
        for ta, tb in zip(a, b):
            assert torch.equal(ta.view(torch.int16), tb.view(torch.int16))
        mo.check(f"determinism case {n, T, r, C} drop={drop}", *a, c["ref"], torch.bfloat16)


def test_more_groups_than_a_grid_dimension_holds():
    """n = 70000 groups of T = 4 tokens (r = 1, C = 8): the frozen form's group index spans blockIdx.y and .z, the
    parameter form walks 70000 slabs with 512 workgroups; every group's gx is checked, and dweight / dbias."""
    _abi, _, _, _ = _mods()
    n, T, r, C, dtype = 70000, 4, 1, 8, torch.bfloat16
    gen = torch.Generator().manual_seed(3)
    src = torch.randint(0, 2, (n, 1, 1), generator=gen)
    dst = torch.randint(0, 2, (n, 1, 1), generator=gen)
    dev = torch.device(DEV)
    plan = _abi.MatchPlan(n, T, r, False, False, src.to(dev), dst.to(dev), (1 - src).to(dev), None, None, dev)
    assert mo.form(n, T, C)[1] > 1
    c = _case(plan, C, dtype, dtype, 8, True, True, False)
    for params in (False, True):
        gx, dw, db = _run(_abi, plan, c, False, params)
        mo.check(f"n={n} params={params}", gx, dw, db, c["ref"], dtype)


def test_refusals_write_nothing():
    _abi, _, M, _ = _mods()
    plan = _matching(M, 2, 8, False, False, 2, 1).plan

    def refused(C, dtype=torch.bfloat16, **kw):
        c = _case(plan, C, torch.bfloat16, torch.bfloat16, 3, True, True, False)
        t = {k: _dev(c[k] if c[k] is None or dtype == torch.bfloat16 else c[k].to(dtype))
             for k in ("gy", "gi", "xs", "s_out", "size", "w")}
        gx = _poisoned(2, 8, 2 * C)  # (room for fp32 tokens too)
        dw, db = _poisoned(2 * C), _poisoned(2 * C)
        ws = _poisoned(1 << 16)
        rc, msg = _raw(_abi, plan, t, C, gx=gx, dw=dw, db=db, ws=ws, **kw)
        assert rc != 0 and msg, (C, kw, rc, msg)
        for buf in (gx, dw, db, ws):
            assert bool((buf == POISON).all()), (C, kw, "a refused call wrote")
        return msg

    assert "1024" in refused(1032)
    assert "C % 8" in refused(100)
    assert "16-bit" in refused(96, dtype=torch.float32)
    assert "r=0" in refused(96, r=0)
    assert "row_map" in refused(96, row_map=False)
    assert _abi.lib().tome_merge_ln_backward_workspace_bytes(2, 8, 1032) == 0
    assert _abi.lib().tome_merge_ln_backward_workspace_bytes(2, 8, 100) == 0


def _norm(C, dtype, cls=torch.nn.LayerNorm):
    torch.manual_seed(C)
    n = cls(C, eps=EPS)
    with torch.no_grad():
        n.weight.add_(0.1 * torch.randn(C))
        n.bias.add_(0.1 * torch.randn(C))
    return n.to(DEV).to(dtype)


def _tokens(n, T, C, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, T, C, generator=gen).to(dtype).to(DEV)
    return x, (0.5 * torch.randn(n, T, C, generator=gen)).to(dtype).to(DEV)


def test_function_of_the_public_call():
    _abi, _ln, M, _ = _mods()
    n, T, C, r, dtype = 2, 8, 96, 2, torch.bfloat16
    merge = _matching(M, n, T, False, False, r, 4)
    norm = _norm(C, dtype)
    x0, res0 = _tokens(n, T, C, dtype, 1)
    size = torch.randint(1, 4, (n, T, 1), generator=torch.Generator().manual_seed(2)).to(dtype).to(DEV)
    gen = torch.Generator().manual_seed(5)
    g_x, g_y = (torch.randn(n, T - r, C, generator=gen).to(dtype).to(DEV) for _ in range(2))
    x, res = x0.clone().requires_grad_(True), res0.clone().requires_grad_(True)
    x_out, y, size_out = M.merge_wavg_ln(merge, x, size, norm, residual=res, log_size=True)
    assert type(x_out.grad_fn).__name__ == "_MergeLnFunctionBackward" and y.grad_fn is x_out.grad_fn
    assert size_out.grad_fn is None and not size_out.requires_grad
    log = _abi.log_of_size(size_out)
    assert log.grad_fn is None and torch.equal(log, size_out.log())
    fx, fy, fs = _abi.merge_wavg_ln(merge.plan, x0, size, norm.weight.detach(), norm.bias.detach(), norm.eps, addend=res0)
    assert torch.equal(x_out, fx) and torch.equal(y, fy) and torch.equal(size_out, fs), "forward = the inference launch"
    torch.autograd.backward([x_out, y], [g_x, g_y], retain_graph=True)
    assert torch.equal(x.grad, res.grad), "x and the residual receive one tensor"
    first = (x.grad.clone(), norm.weight.grad.clone(), norm.bias.grad.clone())
    x.grad = res.grad = norm.weight.grad = norm.bias.grad = None
    torch.autograd.backward([x_out, y], [g_x, g_y])
    for a, b in zip(first, (x.grad, norm.weight.grad, norm.bias.grad)):
        assert torch.equal(a, b), "a second backward over the retained graph gives the same bits"
    row_of, _ = _rows(merge.plan, False)
    ref = mo.reference(g_y, g_x, x_out.detach(), size_out, size, norm.weight, EPS, row_of)
    mo.check("Function", x.grad, norm.weight.grad, norm.bias.grad, ref, dtype)
    # the residual alone requires grad, the norm is frozen
    frozen = copy.deepcopy(norm).requires_grad_(False)
    bo.residual_gradient_survives(lambda xi, ri: M.merge_wavg_ln(merge, xi, size, frozen, residual=ri)[:2], x0, res0, DEV)
    # drop_ln
    drop = M.bipartite_soft_matching_drop(torch.randn(n, T, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7)),
                                          r)
    x, res = x0.clone().requires_grad_(True), res0.clone().requires_grad_(True)
    norm.zero_grad(set_to_none=True)
    xd, yd = M.drop_ln(drop, x, norm, residual=res)
    assert type(xd.grad_fn).__name__ == "_MergeLnFunctionBackward" and yd.grad_fn is xd.grad_fn
    torch.autograd.backward([xd, yd], [g_x, g_y])
    assert torch.equal(x.grad, res.grad)
    ref = mo.reference(g_y, g_x, xd.detach(), None, None, norm.weight, EPS, _rows(drop.plan, True)[0])
    mo.check("Function, drop", x.grad, norm.weight.grad, norm.bias.grad, ref, dtype)
    bo.residual_gradient_survives(lambda xi, ri: M.drop_ln(drop, xi, frozen, residual=ri), x0, res0, DEV)
    # without a gradient wanted: the existing launches, no graph
    with torch.no_grad():
        nx, ny, ns = M.merge_wavg_ln(merge, x0, size, norm, residual=res0)
    assert torch.equal(nx, fx) and torch.equal(ny, fy) and torch.equal(ns, fs) and nx.grad_fn is None


def test_what_the_function_does_not_cover_takes_the_three_steps():
    """A hybrid matching, a kth_ matching, fp32 tokens and a LayerNorm subclass: not the Function's grad_fn, finite
    gradients, and the bits of the three steps written out."""
    _, _, M, _ = _mods()

    class Sub(torch.nn.LayerNorm):
        pass

    n, T, C, r = 2, 8, 96, 2
    metric = torch.randn(n, T, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    plain, _ = M.bipartite_soft_matching(metric, r)
    cases = [("hybrid", M.bipartite_soft_matching_hybrid(metric, r, threshold=0.5)[0], torch.bfloat16, torch.nn.LayerNorm),
             ("kth", M.kth_bipartite_soft_matching(metric, 2)[0], torch.bfloat16, torch.nn.LayerNorm),
             ("fp32", plain, torch.float32, torch.nn.LayerNorm),
             ("subclass", plain, torch.bfloat16, Sub)]
    for name, merge, dtype, cls in cases:
        norm = _norm(C, dtype, cls)
        x0, res0 = _tokens(n, T, C, dtype, 8)
        grads = []
        for public in (True, False):
            x, res = x0.clone().requires_grad_(True), res0.clone().requires_grad_(True)
            norm.zero_grad(set_to_none=True)
            if public:
                xo, y, _ = M.merge_wavg_ln(merge, x, None, norm, residual=res)
                assert "_MergeLnFunction" not in type(xo.grad_fn).__name__ + type(y.grad_fn).__name__, name
            else:
                xo, _ = M.merge_wavg(merge, x + res, None)
                y = norm(xo)
            (xo.float().square().sum() + y.float().square().sum()).backward()
            grads.append((x.grad, res.grad, norm.weight.grad.clone(), norm.bias.grad.clone()))
        for a, b in zip(*grads):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), name


def _graph_nodes(root, name):
    seen, stack, count = set(), [root], 0
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        count += type(fn).__name__ == name
        stack.extend(f for f, _ in fn.next_functions)
    return count


def _train_hosts():
    import tome
    from hosts import videomae, vivit
    return dict(
        videomae=(lambda: videomae.VideoMAE(num_frames=8, img_size=64, patch_size=16, embed_dim=64, depth=3,
                                            num_heads=1, num_classes=9), (2, 3, 8, 64, 64), tome.patch.videomae),
        vivit=(lambda: vivit.ViViT(num_classes=9, image_size=64, num_frames=8, hidden_size=64, num_hidden_layers=3,
                                   num_attention_heads=1, intermediate_size=256), (2, 3, 8, 64, 64), tome.patch.vivit))


@pytest.mark.parametrize("name", ["videomae", "vivit"])
def test_patched_model_trains_through_the_function(name, monkeypatch):
    """Reduced-width hosts, bf16, .train(), r = 6 in every block, three runs on the same weights and clip: (on) the switch
    on, (off) the switch off -- today's three steps --, (ref) the switch off with the merge chain of every block (merge_wavg
    and the LayerNorm behind it) evaluated in fp64 on the framework's ops: the forward stores the same 16-bit rows (the
    merged rows are rounded with a straight-through gradient, the LayerNorm reads the rounded rows), the backward adds the
    stream's gradient and the LayerNorm's in fp64 and rounds once, at the tokens.  (With the merge alone in fp64 the
    reference rounds the LayerNorm's gradient of the merged rows to bf16 exactly where (off) does; measured on the
    MI355X, (off) then equals the reference bit for bit in every parameter, err_off = 0, and the rule would ask the one
    launch to reproduce the rounding it exists to leave out.)
    Switch on: three _MergeLnFunctionBackward nodes, no call of merge_wavg_native, a finite gradient for every block
    parameter, and per parameter (max-norm scaled by the parameter's largest reference gradient)
    err_on <= 2 err_off + 2^-20: two 16-bit evaluations of one formula, the bound comes from the third."""
    _abi, _ln, M, common = _mods()
    make, clip_shape, patch = _train_hosts()[name]
    torch.manual_seed(0)
    model = make().to(DEV).to(torch.bfloat16).train()
    patch(model)
    clip = torch.rand(*clip_shape, generator=torch.Generator().manual_seed(3)).to(DEV).to(torch.bfloat16)
    native_calls = []
    orig_native = M.merge_wavg_native
    monkeypatch.setattr(M, "merge_wavg_native", lambda *a, **kw: native_calls.append(1) or orig_native(*a, **kw))
    wavg = common.merge_wavg

    trailing = common._trailing_norm

    def wavg64(merge, x, size=None, log_size=False):
        plan = getattr(merge, "plan", None)
        if plan is None:
            return wavg(merge, x, size, log_size=log_size)
        s64 = torch.ones_like(x[..., 0, None], dtype=torch.float64) if size is None else size.double()
        s_sum = M._merge_with_autograd(plan, s64, "sum")
        x64 = M._merge_with_autograd(plan, x.double() * s64, "sum") / s_sum
        stored = x64 + (x64.to(x.dtype).double() - x64).detach()  # the 16-bit rows the forward stores, gradient in fp64
        out = stored.to(x.dtype)
        out._fp64_rows = stored
        return out, s_sum.to(x.dtype)

    def norm64(x, norm):
        rows = getattr(x, "_fp64_rows", None)
        if rows is None:
            return trailing(x, norm)
        return torch.nn.functional.layer_norm(rows, (rows.shape[-1],), norm.weight.double(), norm.bias.double(),
                                              norm.eps).to(x.dtype)

    def run(switch, fp64):
        monkeypatch.setattr(common, "TRAIN_FUSED_LN", switch)
        monkeypatch.setattr(common, "merge_wavg", wavg64 if fp64 else wavg)
        monkeypatch.setattr(common, "_trailing_norm", norm64 if fp64 else trailing)
        model.zero_grad(set_to_none=True)
        model.r = 6
        del native_calls[:]
        torch.manual_seed(1)
        out = model([clip])
        nodes = _graph_nodes(out.grad_fn, "_MergeLnFunctionBackward")
        out.float().square().sum().backward()
        grads = {k: q.grad.detach().double().cpu() for k, q in model.named_parameters() if q.grad is not None}
        return grads, nodes, len(native_calls)

    g_on, nodes_on, native_on = run(True, False)
    g_off, nodes_off, native_off = run(False, False)
    g_ref, nodes_ref, _ = run(False, True)
    assert nodes_on == 3 and native_on == 0, (nodes_on, native_on)
    assert nodes_off == 0 and native_off == 3 and nodes_ref == 0, (nodes_off, native_off, nodes_ref)
    block = lambda k: ("blocks" in k or ".layer." in k)  # noqa: E731
    missing = [k for k, q in model.named_parameters() if block(k) and (k not in g_on or not torch.isfinite(g_on[k]).all())]
    assert not missing, missing
    assert g_on.keys() == g_off.keys() == g_ref.keys()
    worst_on = worst_off = 0.0
    bad = []
    for k in g_ref:
        scale = g_ref[k].abs().max().item()
        if scale == 0.0:
            assert g_on[k].abs().max().item() == 0.0, k
            continue
        e_on = (g_on[k] - g_ref[k]).abs().max().item() / scale
        e_off = (g_off[k] - g_ref[k]).abs().max().item() / scale
        worst_on, worst_off = max(worst_on, e_on), max(worst_off, e_off)
        if not e_on <= 2 * e_off + 2.0 ** -20:
            bad.append((k, e_on, e_off))
    print(f"{name}: worst scaled gradient error, switch on vs the fp64 chain {worst_on:.3e}, switch off vs the fp64 chain "
          f"{worst_off:.3e}")
    assert not bad, bad
