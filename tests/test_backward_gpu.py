"""Native backward of merge / merge_wavg / unmerge / drop (tome_merge_backward, k_merge_rows_bwd) on the GPU: the
Functions are taken, their gradients equal the reference's op sequence differentiated by autograd in fp64
(oracle/torch_port.py, pinned to the reference by tests/test_torch_port.py) within bounds derived from the number
formats, they are deterministic, the regrouped layout equals the plain one bit for bit, everything that is not covered
keeps the framework path, and a patched model trains through them."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# relative bound of one fp32 division and one fp32 product followed by one rounding to the token dtype, against the exact
# value: fp32 2 roundings of 2^-24 (stated as 2^-22), 16-bit formats their unit roundoff times (1 + 2^-20) for the fp32
# intermediate.  fp16 alone also gets an absolute term: its subnormals (below 2^-14; N(0,1) gradients divided by a size
# reach them a few times per million elements) are spaced 2^-24 apart, so a correctly rounded result is off by up to
# 2^-25 there whatever its size; fp32 and bf16 have no such values in these tests and keep atol = 0.
RTOL = {torch.float32: 2.0 ** -22, torch.bfloat16: 2.0 ** -8 * (1 + 2.0 ** -20), torch.float16: 2.0 ** -11 * (1 + 2.0 ** -20)}
ATOL = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}


def _mods():
    from oracle import torch_port
    from tome import _abi
    from tome import merge as M
    return M, _abi, torch_port


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _matching(M, n, T, cls, distill, r, seed, drop=False):
    metric = torch.randn(n, T, 32, device=DEV, generator=_gen(seed))
    if drop:
        return M.bipartite_soft_matching_drop(metric, r, class_token=cls, distill_token=distill)
    return M.bipartite_soft_matching(metric, r, class_token=cls, distill_token=distill)


def _cpu_plan(torch_port, p):
    return torch_port.TorchPlan(p.r, p.src_idx.cpu(), p.dst_idx.cpu(), p.unm_idx.cpu(), p.T)


def _layout(plan, y):
    """merge.py:82-85: with a distillation token the class token and the distillation token lead the merged sequence
    (torch_port.merge writes [unmerged, destinations])."""
    if not plan.distill_token:
        return y
    u = (plan.T + 1) // 2 - plan.r
    kept, dst = y[:, :u], y[:, u:]
    return torch.cat([kept[:, :1], dst[:, :1], kept[:, 1:], dst[:, 1:]], dim=1)


def _ref_drop(tp, x):
    """merge.py:253-262: the unmerged even tokens, then every odd token."""
    even, odd = x[:, ::2], x[:, 1::2]
    n, t1, c = even.shape
    return torch.cat([even.gather(1, tp.unm_idx.expand(n, t1 - tp.r, c)), odd], dim=1)


def _ref_grad(fn, x64, g64):
    x64 = x64.clone().requires_grad_(True)
    fn(x64).backward(g64)
    return x64.grad


def _assert_within(got, ref64, dtype, what):
    got64 = got.double().cpu()
    err = (got64 - ref64).abs()
    bound = RTOL[dtype] * ref64.abs() + ATOL[dtype]
    worst = (err - bound).max().item()
    rel = (err / ref64.abs().clamp_min(1e-300)).max().item()
    print(f"{what}: max relative error {rel:.3e} (bound {RTOL[dtype]:.3e})")
    assert worst <= 0.0, (what, worst, rel)


# T even and odd, with and without class token, with distillation token
SHAPES = [(16, False, False), (17, False, False), (197, True, False), (198, True, True), (64, False, False)]
CHANNELS = [8, 96, 768, 100]


def test_grad_fn_is_native_and_library_exports_the_backward():
    """Fails without the feature: tokens that require grad take this package's Functions, and the library is ABI 11
    with tome_merge_backward."""
    M, _abi, _ = _mods()
    L = _abi.lib()
    assert L.tome_abi_version() == 11
    assert hasattr(L, "tome_merge_backward") and hasattr(L, "tome_merge_backward_regrouped")
    merge, unmerge = _matching(M, 2, 64, False, False, 8, 1)
    drop = _matching(M, 2, 64, False, False, 8, 1, drop=True)
    x = torch.randn(2, 64, 96, device=DEV, requires_grad=True)
    size = torch.randint(1, 5, (2, 64, 1), device=DEV).float()
    names = {
        "merge": type(merge(x).grad_fn).__name__,
        "merge_sum": type(merge(x, mode="sum").grad_fn).__name__,
        "merge_wavg": type(M.merge_wavg(merge, x, size)[0].grad_fn).__name__,
        "unmerge": type(unmerge(torch.randn(2, 56, 96, device=DEV, requires_grad=True)).grad_fn).__name__,
        "drop": type(drop(x).grad_fn).__name__,
    }
    assert names == {"merge": "_MergeFunctionBackward", "merge_sum": "_MergeFunctionBackward",
                     "merge_wavg": "_MergeWavgFunctionBackward", "unmerge": "_UnmergeFunctionBackward",
                     "drop": "_DropFunctionBackward"}, names
    xs, ss = M.merge_wavg(merge, x, size, log_size=True)
    assert not ss.requires_grad and ss.grad_fn is None
    log = _abi.log_of_size(ss)
    assert log is getattr(ss, "_tome_log") and not log.requires_grad
    with torch.no_grad():
        wx, ws = M.merge_wavg(merge, x, size, log_size=True)
    assert torch.equal(xs, wx) and torch.equal(ss, ws) and torch.equal(log, _abi.log_of_size(ws))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_op_gradients_against_the_reference_op_sequence(dtype):
    """Reference: oracle/torch_port.py on CPU in fp64 with the plan's own index tensors, upstream gradient N(0,1),
    sizes random integers 1..4 and None.  mean / merge_wavg within the derived bound (RTOL / ATOL above); sum and drop
    bit-equal to the gathered upstream gradient."""
    M, _abi, torch_port = _mods()
    seed = 100
    for (T, cls, distill), C, n in itertools.product(SHAPES, CHANNELS, (1, 4)):
        clamp = (T - int(cls) - int(distill)) // 2
        for r in (1, clamp):
            seed += 1
            merge, _ = _matching(M, n, T, cls, distill, r, seed)
            drop = _matching(M, n, T, cls, distill, r, seed, drop=True)
            plan = merge.plan
            tp = _cpu_plan(torch_port, plan)
            gen = _gen(seed)
            x = torch.randn(n, T, C, device=DEV, generator=gen).to(dtype)
            g = torch.randn(n, T - plan.r, C, device=DEV, generator=gen).to(dtype)
            size = torch.randint(1, 5, (n, T, 1), device=DEV, generator=gen).to(dtype)
            x64, g64, s64 = x.double().cpu(), g.double().cpu(), size.double().cpu()
            tag = f"T={T} cls={cls} distill={distill} r={plan.r} C={C} n={n} {dtype}"

            def native(fn):
                xg = x.clone().requires_grad_(True)
                out = fn(xg)
                assert "Function" in type(out.grad_fn).__name__, (tag, out.grad_fn)
                out.backward(g)
                return xg.grad

            for mode in ("sum", "mean"):
                ref = _ref_grad(lambda t: _layout(plan, torch_port.merge(tp, t, mode)), x64, g64)
                got = native(lambda t: merge(t, mode=mode))
                if mode == "sum":
                    assert torch.equal(got.double().cpu(), ref), (tag, mode)
                else:
                    _assert_within(got, ref, dtype, f"mean {tag}")
            for sz, sz64 in ((None, None), (size, s64)):
                ref = _ref_grad(lambda t: _layout(plan, torch_port.merge_wavg(tp, t, sz64)[0]), x64, g64)
                got = native(lambda t: M.merge_wavg(merge, t, sz)[0])
                _assert_within(got, ref, dtype, f"merge_wavg size={'given' if sz is not None else None} {tag}")
            ref = _ref_grad(lambda t: _layout(plan, _ref_drop(tp, t)), x64, g64)
            got = native(drop)
            assert torch.equal(got.double().cpu(), ref), (tag, "drop")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_unmerge_backward_is_the_sum_merge(dtype):
    """unmerge backward: bit-equal to _abi.merge(plan, g, "sum"); fp32 within the summation bound
    (k-1) * 2^-24 * sum|terms| of the fp64 reference (torch_port.merge in mode sum, the adjoint), k = terms of the row."""
    M, _abi, torch_port = _mods()
    seed = 300
    for (T, cls, distill), C, n in itertools.product([s for s in SHAPES if not s[2]], CHANNELS, (1, 4)):
        for r in (1, (T - int(cls)) // 2):
            seed += 1
            merge, unmerge = _matching(M, n, T, cls, distill, r, seed)
            plan = merge.plan
            gen = _gen(seed)
            y = torch.randn(n, T - plan.r, C, device=DEV, generator=gen).to(dtype).requires_grad_(True)
            g = torch.randn(n, T, C, device=DEV, generator=gen).to(dtype)
            out = unmerge(y)
            assert type(out.grad_fn).__name__ == "_UnmergeFunctionBackward"
            out.backward(g)
            with torch.no_grad():
                assert torch.equal(y.grad, _abi.merge(plan, g, "sum"))
            if dtype is torch.float32:
                tp = _cpu_plan(torch_port, plan)
                g64 = g.double().cpu()
                ref = torch_port.merge(tp, g64, "sum")
                terms = torch_port.merge(tp, g64.abs(), "sum")
                k = torch_port.merge(tp, torch.ones(n, T, 1, dtype=torch.float64), "sum")
                bound = (k - 1) * 2.0 ** -24 * terms
                assert ((y.grad.double().cpu() - ref).abs() <= bound).all(), (T, cls, r, C, n)


def test_adjointness_in_fp32():
    """<merge_sum(x), g> == <x, backward(g)> and <unmerge(y), h> == <y, backward(h)>, in fp64 from the kernel outputs.
    The gathers are exact; the sums carry (k-1) * 2^-24 * sum|terms| per element, weighted by the other factor, plus
    2^-40 of the absolute inner product for the fp64 accumulation itself."""
    M, _abi, _ = _mods()
    seed = 500
    for (T, cls, distill), C, n in itertools.product(SHAPES, (96, 100), (1, 4)):
        for r in (1, (T - int(cls) - int(distill)) // 2):
            seed += 1
            merge, unmerge = _matching(M, n, T, cls, distill, r, seed)
            plan = merge.plan
            gen = _gen(seed)
            x = torch.randn(n, T, C, device=DEV, generator=gen)
            g = torch.randn(n, T - plan.r, C, device=DEV, generator=gen)
            with torch.no_grad():
                y = _abi.merge(plan, x, "sum")
                gx = _abi.merge_backward(plan, g)
                k = _abi.merge(plan, torch.ones(n, T, 1, device=DEV), "sum").double()
                terms = _abi.merge(plan, x.abs(), "sum").double()
            lhs, rhs = (y.double() * g.double()).sum(), (x.double() * gx.double()).sum()
            bound = ((k - 1) * 2.0 ** -24 * terms * g.double().abs()).sum() * (1 + 2.0 ** -20) \
                + 2.0 ** -40 * (x.double() * gx.double()).abs().sum()
            assert (lhs - rhs).abs() <= bound, ("merge", T, cls, distill, r, C, n, lhs.item(), rhs.item())
            if distill:
                continue
            h = torch.randn(n, T, C, device=DEV, generator=gen)
            yy = g.clone().requires_grad_(True)
            up = unmerge(yy)
            up.backward(h)
            with torch.no_grad():
                terms = _abi.merge(plan, h.abs(), "sum").double()
            lhs, rhs = (up.detach().double() * h.double()).sum(), (yy.detach().double() * yy.grad.double()).sum()
            bound = ((k - 1) * 2.0 ** -24 * terms * yy.detach().double().abs()).sum() * (1 + 2.0 ** -20) \
                + 2.0 ** -40 * (up.detach().double() * h.double()).abs().sum()
            assert (lhs - rhs).abs() <= bound, ("unmerge", T, cls, r, C, n, lhs.item(), rhs.item())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("B,F,P,C,r", [(2, 4, 50, 64, 5), (1, 8, 196, 768, 16), (3, 2, 37, 96, 18)])
def test_regrouped_gradient_equals_plain_layout_on_rearranged_tensors(B, F, P, C, r, dtype):
    """The regrouped Functions' gradient == the plain-layout Functions on '(p t) -> (b t) p' tensors, bit for bit;
    the class row's gradient passes through."""
    M, _abi, _ = _mods()
    gen = _gen(700 + P)
    metric = torch.randn(B * F, P, 16, device=DEV, generator=gen)
    merge, _ = M.bipartite_soft_matching(metric, r)
    drop = M.bipartite_soft_matching_drop(metric, r)
    plan = merge.plan
    P2 = P - plan.r
    x_full = torch.randn(B, 1 + P * F, C, device=DEV, generator=gen).to(dtype)
    g_full = torch.randn(B, 1 + P2 * F, C, device=DEV, generator=gen).to(dtype)
    size = torch.randint(1, 5, (B * F, P, 1), device=DEV, generator=gen).to(dtype)

    def grouped(t, p):
        return t[:, 1:, :].reshape(B, p, F, C).transpose(1, 2).reshape(B * F, p, C).contiguous()

    def ungrouped(t, p):
        return t.reshape(B, F, p, C).transpose(1, 2).reshape(B, p * F, C)

    for kind, sz in (("wavg", None), ("wavg", size), ("drop", None)):
        xr = x_full.clone().requires_grad_(True)
        if kind == "wavg":
            out, s_out = M.merge_wavg_regrouped_native(plan, xr, sz, F, has_cls=True)
            assert type(out.grad_fn).__name__ == "_MergeWavgRegroupedFunctionBackward" and not s_out.requires_grad
        else:
            out = M.drop_regrouped_native(drop.plan, xr, F, has_cls=True)
            assert type(out.grad_fn).__name__ == "_DropRegroupedFunctionBackward"
        out.backward(g_full)
        xp = grouped(x_full, P).requires_grad_(True)
        if kind == "wavg":
            want_out, want_s = M.merge_wavg(merge, xp, sz)
            assert torch.equal(s_out, want_s)
        else:
            want_out = drop(xp)
        assert torch.equal(out[:, 1:].detach(), ungrouped(want_out.detach(), P2))
        want_out.backward(grouped(g_full, P2))
        assert torch.equal(xr.grad[:, 1:], ungrouped(xp.grad, P)), (kind, sz is not None)
        assert torch.equal(xr.grad[:, :1], g_full[:, :1]), kind


def test_backward_is_deterministic():
    """Two backward calls on the same inputs return identical bits (asserted for the native path only)."""
    M, _abi, _ = _mods()
    merge, unmerge = _matching(M, 4, 197, True, False, 16, 900)
    gen = _gen(901)
    x = torch.randn(4, 197, 768, device=DEV, generator=gen).bfloat16().requires_grad_(True)
    size = torch.randint(1, 5, (4, 197, 1), device=DEV, generator=gen).bfloat16()
    out = M.merge_wavg(merge, x, size)[0]
    g = torch.randn(out.shape, device=DEV, generator=gen).bfloat16()
    a, = torch.autograd.grad(out, x, g, retain_graph=True)
    b, = torch.autograd.grad(out, x, g, retain_graph=True)
    assert torch.equal(a, b)
    y = out.detach().requires_grad_(True)
    up = unmerge(y)
    h = torch.randn(up.shape, device=DEV, generator=gen).bfloat16()
    a, = torch.autograd.grad(up, y, h, retain_graph=True)
    b, = torch.autograd.grad(up, y, h, retain_graph=True)
    assert torch.equal(a, b)


def _is_native(t):
    return type(t.grad_fn).__name__.endswith("FunctionBackward")


def test_not_covered_cases_keep_the_framework_path(monkeypatch):
    """Reduce modes other than sum / mean, a size that requires grad, hybrid matchings, unmerge with a distillation
    token, the kth_ / random_ matchings, fp64 tensors and the switched-off flag: a gradient through the framework's
    ops, a framework grad_fn.  A CPU tensor meets the device index tensors in the framework's gather exactly as
    before.  Double backward raises; a gradient of another shape or device is refused on the host."""
    M, _abi, _ = _mods()
    n, T, C = 2, 64, 96
    gen = _gen(1000)
    metric = torch.randn(n, T, 32, device=DEV, generator=gen)
    merge, unmerge = M.bipartite_soft_matching(metric, 8)
    x = torch.randn(n, T, C, device=DEV, generator=gen)
    size = torch.randint(1, 5, (n, T, 1), device=DEV, generator=gen).float()

    def check(make, *leaves):
        out = make()
        assert out.requires_grad and not _is_native(out), out.grad_fn
        out.square().sum().backward()
        for leaf in leaves:
            assert leaf.grad is not None and torch.isfinite(leaf.grad).all()

    for mode in ("max", "amax", "min", "prod"):
        xg = x.clone().requires_grad_(True)
        check(lambda: merge(xg, mode=mode), xg)
    xg, sg = x.clone().requires_grad_(True), size.clone().requires_grad_(True)
    check(lambda: M.merge_wavg(merge, xg, sg)[0], xg, sg)
    sg = size.clone().requires_grad_(True)
    check(lambda: M.merge_wavg(merge, x, sg)[0], sg)
    hmerge, hunmerge = M.bipartite_soft_matching_hybrid(metric, 8, threshold=0.5)
    xg = x.clone().requires_grad_(True)
    check(lambda: M.merge_wavg(hmerge, xg, size)[0], xg)
    xg = x.clone().requires_grad_(True)
    check(lambda: hmerge(xg, mode="sum"), xg)
    yg = torch.randn(n, T - 8, C, device=DEV, generator=gen).requires_grad_(True)
    check(lambda: hunmerge(yg), yg)
    dmerge, dunmerge = M.bipartite_soft_matching(metric, 8, class_token=True, distill_token=True)
    yg = torch.randn(n, T - 8, C, device=DEV, generator=gen).requires_grad_(True)
    check(lambda: dunmerge(yg), yg)
    for pmerge, punmerge in (M.kth_bipartite_soft_matching(metric, 4), M.random_bipartite_soft_matching(metric, 8)):
        xg = x.clone().requires_grad_(True)
        check(lambda: M.merge_wavg(pmerge, xg, size)[0], xg)
        xg = x.clone().requires_grad_(True)
        out = pmerge(xg, mode="sum")
        assert not _is_native(out)
        yg = out.detach().requires_grad_(True)
        check(lambda: punmerge(yg), yg)
    xg = x.double().requires_grad_(True)
    check(lambda: merge(xg, mode="sum"), xg)
    yg = torch.randn(n, T - 8, C, device=DEV, generator=gen).double().requires_grad_(True)
    check(lambda: unmerge(yg), yg)
    with pytest.raises(RuntimeError, match="same device"):
        merge(x.cpu().requires_grad_(True), mode="sum")
    monkeypatch.setattr(M, "NATIVE_BACKWARD", False)
    xg = x.clone().requires_grad_(True)
    check(lambda: M.merge_wavg(merge, xg, size)[0], xg)
    xg = x.clone().requires_grad_(True)
    check(lambda: merge(xg), xg)
    yg = torch.randn(n, T - 8, C, device=DEV, generator=gen).requires_grad_(True)
    check(lambda: unmerge(yg), yg)
    monkeypatch.setattr(M, "NATIVE_BACKWARD", True)

    # double backward
    xg = x.clone().requires_grad_(True)
    out = M.merge_wavg(merge, xg, size)[0]
    assert _is_native(out)
    first, = torch.autograd.grad(out.square().sum(), xg, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        first.sum().backward()

    # host-side refusals: nothing reaches a kernel
    plan = merge.plan
    with pytest.raises(_abi.TomeHipError, match="expected a gradient"):
        _abi.merge_backward(plan, torch.randn(n, T - 7, C, device=DEV))
    with pytest.raises(_abi.TomeHipError, match="expected a gradient"):
        _abi.merge_backward(plan, torch.randn(n + 1, T - 8, C, device=DEV))
    with pytest.raises(_abi.TomeHipError, match="no CPU path"):
        _abi.merge_backward(plan, torch.randn(n, T - 8, C))
    with pytest.raises(_abi.TomeHipError, match="expected a gradient"):
        _abi.merge_backward_regrouped(plan, torch.randn(2, 1 + (T - 8) * 2, C, device=DEV), 2, has_cls=True)
    with pytest.raises(_abi.TomeHipError, match="scale"):
        _abi.merge_backward(plan, torch.randn(n, T - 8, C, device=DEV), out_div=torch.ones(n, T, 1, device=DEV))
    L = _abi.lib()
    buf = torch.zeros(64, device=DEV)
    rc = L.tome_merge_backward(buf.data_ptr(), 0, None, None, 0, 1, 8, 4, 9, buf.data_ptr(), 0, 0, buf.data_ptr(), None)
    assert rc == 1 and b"tome_merge_backward" in L.tome_last_error()
    rc = L.tome_merge_backward(buf.data_ptr(), 0, None, None, 0, 1, 8, 4, 2, None, 0, 0, buf.data_ptr(), None)
    assert rc == 1 and b"row_map" in L.tome_last_error()
    # direct kernel calls keep refusing tensors that require grad (the Functions hand them detached tensors)
    with pytest.raises(_abi.TomeHipError):
        _abi.merge_wavg(plan, x.clone().requires_grad_(True), size)


def _train_hosts():
    import tome
    from hosts import timesformer, videomae
    return (
        ("videomae", lambda: videomae.VideoMAE(num_frames=8, img_size=64, patch_size=16, embed_dim=64, depth=3,
                                               num_heads=1, num_classes=9), (2, 3, 8, 64, 64), tome.patch.videomae),
        ("timesformer", lambda: timesformer.TimeSformer(num_frames=4, img_size=64, patch_size=8, embed_dim=64, depth=3,
                                                        num_heads=1, num_classes=9), (2, 3, 4, 64, 64),
         tome.patch.timesformer))


def _count_calls(monkeypatch, _abi, counts):
    for name in ("merge_backward", "merge_backward_regrouped"):
        orig = getattr(_abi, name)

        def counted(*a, _orig=orig, _name=name, **kw):
            counts[_name] = counts.get(_name, 0) + 1
            return _orig(*a, **kw)
        monkeypatch.setattr(_abi, name, counted)


@pytest.mark.parametrize("which", [0, 1], ids=["videomae", "timesformer"])
def test_patched_model_trains_on_the_native_path(which, monkeypatch):
    """Reduced-width hosts, fp32, .train(), merging in block 0 only (model.r = [6, 0, 0]) so that the matching sees
    bit-identical inputs on every path (asserted).  Forward + backward three ways on the same weights and clip:
    (a) native, (b) framework path, (c) framework path with the merge evaluated in fp64 and cast back.  Per parameter,
    max-norm scaled by the parameter's largest gradient: err(a vs c) <= 2 * err(b vs c) + 2^-20 -- (a) and (b) are two
    single-precision evaluations of one formula that differ in summation order only; the bound comes from (c)."""
    M, _abi, _ = _mods()
    from tome.patch import _common
    name, make, clip_shape, patch = _train_hosts()[which]
    torch.manual_seed(0)
    model = make().to(DEV).train()
    patch(model)
    clip = torch.rand(*clip_shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    counts, plans = {}, []
    _count_calls(monkeypatch, _abi, counts)
    make_pair = M._make_merge_pair

    def recording_pair(plan):
        plans.append(plan)
        return make_pair(plan)
    monkeypatch.setattr(M, "_make_merge_pair", recording_pair)
    wavg = M.merge_wavg

    def wavg64(merge, x, size=None, log_size=False):
        plan = getattr(merge, "plan", None)
        if plan is None:  # r = 0: do_nothing
            return wavg(merge, x, size, log_size=log_size)
        # merge.py:355-369 on the framework's ops (the kernels take no fp64), every step in fp64
        s64 = torch.ones_like(x[..., 0, None], dtype=torch.float64) if size is None else size.double()
        x_sum = M._merge_with_autograd(plan, x.double() * s64, "sum")
        s_sum = M._merge_with_autograd(plan, s64, "sum")
        return (x_sum / s_sum).to(x.dtype), s_sum.to(x.dtype)

    def run(native, fp64):
        monkeypatch.setattr(M, "NATIVE_BACKWARD", native)
        monkeypatch.setattr(_common, "merge_wavg", wavg64 if fp64 else wavg)
        plans.clear()
        model.zero_grad(set_to_none=True)
        model.r = [6, 0, 0]
        torch.manual_seed(1)
        out = model([clip])
        out.square().sum().backward()
        idx = [(p.src_idx.clone(), p.dst_idx.clone(), p.unm_idx.clone()) for p in plans]
        return {k: q.grad.detach().double().clone() for k, q in model.named_parameters() if q.grad is not None}, idx

    ga, ia = run(True, False)
    native_launches = dict(counts)
    gb, ib = run(False, False)
    gc, ic = run(False, True)
    assert counts == native_launches, "the framework path must not launch the backward kernel"
    assert sum(native_launches.values()) >= 1, native_launches
    assert len(ia) >= 1 and len(ia) == len(ib) == len(ic)
    for pa, pb, pc in zip(ia, ib, ic):
        for ta, tb, tc in zip(pa, pb, pc):
            assert torch.equal(ta, tb) and torch.equal(ta, tc), "the three paths must merge the same tokens"
    assert ga.keys() == gb.keys() == gc.keys()
    missing = [k for k, q in model.named_parameters() if k not in ga or not torch.isfinite(ga[k]).all()]
    assert not [k for k in missing if "blocks" in k and ("qkv" in k or "mlp" in k or "norm" in k)], (name, missing)
    worst_a = worst_b = 0.0
    bad = []
    for k in ga:
        scale = gc[k].abs().max().item()
        if scale == 0.0:
            assert ga[k].abs().max().item() == 0.0, k
            continue
        ea = (ga[k] - gc[k]).abs().max().item() / scale
        eb = (gb[k] - gc[k]).abs().max().item() / scale
        worst_a, worst_b = max(worst_a, ea), max(worst_b, eb)
        if not ea <= 2 * eb + 2.0 ** -20:
            bad.append((k, ea, eb))
    print(f"{name}: worst scaled gradient error native vs fp64-merge {worst_a:.3e}, framework vs fp64-merge {worst_b:.3e}, "
          f"backward launches {native_launches}")
    assert not bad, bad


@pytest.mark.parametrize("which", [0, 1], ids=["videomae", "timesformer"])
def test_patched_model_trains_in_bf16_on_the_full_schedule(which, monkeypatch):
    """bf16, model.r = 6 in every block: finite gradients everywhere, native grad_fns at every merge."""
    M, _abi, _ = _mods()
    name, make, clip_shape, patch = _train_hosts()[which]
    torch.manual_seed(0)
    model = make().to(DEV).to(torch.bfloat16).train()
    patch(model)
    clip = torch.rand(*clip_shape, generator=torch.Generator().manual_seed(3)).to(DEV).to(torch.bfloat16)
    counts, fns = {}, []
    _count_calls(monkeypatch, _abi, counts)
    for fn_name in ("merge_wavg_native", "merge_wavg_regrouped_native"):
        orig = getattr(M, fn_name)

        def seen(*a, _orig=orig, **kw):
            x_out, s_out = _orig(*a, **kw)
            fns.append(type(x_out.grad_fn).__name__)
            return x_out, s_out
        monkeypatch.setattr(M, fn_name, seen)
    model.r = 6
    out = model([clip])
    assert out.requires_grad
    out.float().square().sum().backward()
    want = "_MergeWavgFunctionBackward" if name == "videomae" else "_MergeWavgRegroupedFunctionBackward"
    assert len(fns) == 3 and set(fns) == {want}, fns
    assert sum(counts.values()) == 3, counts
    grads = {k: q.grad for k, q in model.named_parameters()}
    assert not [k for k, q in grads.items() if q is not None and not torch.isfinite(q).all()]
    assert not [k for k, q in grads.items() if q is None and "blocks" in k and ("qkv" in k or "mlp" in k or "norm" in k)]


# ---------------------------------------------------------------------------------------------------------------------
# width sweep of k_merge_rows_bwd: the same rows-per-wave packing as the fused LayerNorm kernels (R rows of cpr 16-byte
# chunks over the lanes of a wave, csrc/tome_kernels.hip launch_merge_bwd), at every width the fast path takes
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_SHAPES = [(16, False), (17, False), (197, True)]


def _sweep_widths(dtype):
    """every multiple of the 16-byte vector up to the fast path's limit (6 chunks per lane * 64 lanes), one beyond it
    and one that is no multiple (both run k_merge_rows_bwd_any)"""
    vec = 16 // torch.empty((), dtype=dtype).element_size()
    limit = 6 * 64 * vec
    return list(range(vec, limit + 1, vec)) + [limit + vec, 12 * vec + 1]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_backward_at_every_width_of_the_fast_path(dtype):
    """Upstream gradient = signature rows (tests/ln_oracle.py: every output row carries the mean of its class, rows
    that share a wave differ by many standard deviations, so a chunk taken from the neighbouring row cannot pass),
    T = 16, 17 and 197 with class token, r = 1 and r = clamp.  sum and drop: grad_in bit-equal to the gather of the
    upstream gradient through the row map computed on the CPU from the plan's index tensors (dropped tokens: zero).
    mean / merge_wavg: RTOL / ATOL above against the fp64 autograd of oracle/torch_port.py."""
    import ln_oracle as lo
    M, _abi, torch_port = _mods()
    seed = 900
    n = 2
    for T, cls in SWEEP_SHAPES:
        for r in (1, (T - int(cls)) // 2):
            seed += 1
            merge, _ = _matching(M, n, T, cls, False, r, seed)
            drop = _matching(M, n, T, cls, False, r, seed, drop=True)
            plan = merge.plan
            tp = _cpu_plan(torch_port, plan)
            row, _ = lo.merged_row_of_token(plan.src_idx, plan.dst_idx, plan.unm_idx, T)
            drow, _ = lo.merged_row_of_token(drop.plan.src_idx, drop.plan.dst_idx, drop.plan.unm_idx, T)
            dropped = torch.zeros(n, T, dtype=torch.bool)
            dropped[torch.arange(n)[:, None], 2 * drop.plan.src_idx.cpu().reshape(n, -1)] = True
            To = T - plan.r
            size = torch.randint(1, 5, (n, T, 1), device=DEV, generator=_gen(seed)).to(dtype)
            s64 = size.double().cpu()
            for C in _sweep_widths(dtype):
                tag = f"T={T} cls={cls} r={plan.r} C={C} {dtype}"
                g = lo.signature_rows((n, To, C), torch.bfloat16, seed * 4096 + C, 1 if C % 16 else -1).to(dtype).to(DEV)
                x = torch.randn(n, T, C, device=DEV, generator=_gen(seed + C)).to(dtype)
                g64 = g.double().cpu()

                def native(fn):
                    xg = x.clone().requires_grad_(True)
                    out = fn(xg)
                    assert "Function" in type(out.grad_fn).__name__, (tag, out.grad_fn)
                    out.backward(g)
                    return xg.grad.cpu()

                gcpu = g.cpu()
                idx = torch.arange(n)[:, None]
                assert torch.equal(native(lambda t: merge(t, mode="sum")), gcpu[idx, row]), (tag, "sum")
                want = gcpu[idx, drow].masked_fill(dropped[:, :, None], 0.0)
                assert torch.equal(native(drop), want), (tag, "drop")
                x64 = x.double().cpu()
                ref = _ref_grad(lambda t: torch_port.merge(tp, t, "mean"), x64, g64)
                _assert_within(native(lambda t: merge(t, mode="mean")), ref, dtype, f"mean {tag}")
                for sz, sz64 in ((None, None), (size, s64)):
                    ref = _ref_grad(lambda t: torch_port.merge_wavg(tp, t, sz64)[0], x64, g64)
                    _assert_within(native(lambda t: M.merge_wavg(merge, t, sz)[0]), ref, dtype,
                                   f"merge_wavg size={'given' if sz is not None else None} {tag}")
