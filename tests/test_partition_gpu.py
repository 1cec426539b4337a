"""GPU tests of the partition matchings -- kth_bipartite_soft_matching (reference tome/merge.py:105-158) and
random_bipartite_soft_matching (merge.py:161-212) -- through the drop-in `tome` package (ctypes -> C ABI -> gfx950
kernels), against tests/golden/partition.npz (what the real reference answered on the CPU) and against the
framework-op evaluation of the same indices.

Indices: equal to the reference on every source row whose fp64 top-2 gap is above TAU (the fixture's certificate); an
uncertified row must still name a destination within TAU of its row's best fp64 score.
Values (fp32): BIT-EXACT for sum / mean / amax / merge_wavg / unmerge on every destination no uncertified row can
reach -- own term first, then the sources in ascending source-row order, is the order of torch's CPU scatter_reduce.
16-bit values equal the round-to-nearest of the fp32 result.

Nothing here reads the reference; every adversary is a legal input.
"""
import numpy as np
import pytest
import torch

import partition_cases as P
import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TAU = 1e-6
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def _tm():
    from tome import merge as tm
    return tm


def _abi():
    from tome import _abi
    return _abi


def closure_vars(fn):
    return dict(zip(fn.__code__.co_freevars, (c.cell_contents for c in fn.__closure__)))


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def make_pair(case, metric=None):
    """(merge, unmerge) of a fixture case: kth through the public function, random through the partition matching fed
    with the index lists the reference drew."""
    tm = _tm()
    if metric is None:
        metric = dev(P.metric_of(case), DTYPES[case["dtype"]])
    if case["fn"] == "kth":
        return tm.kth_bipartite_soft_matching(metric, case["k"])
    a, b = P.positions(case)
    plan = _abi().match_partition(metric, a_idx=dev(a, torch.int64)[..., None], b_idx=dev(b, torch.int64)[..., None])

    def merge(x, mode="mean"):
        return _abi().merge_partition(plan, x, mode)

    def unmerge(x):
        return _abi().unmerge_partition(plan, x)

    merge.plan = plan  # (what merge_wavg / merge_source look for)
    return merge, unmerge


def plan_of(pair):
    return pair[0].plan


def ref_ops(plan, x, mode):
    """The reference's op sequence on the plan's indices (framework ops on x's device)."""
    tm = _tm()
    return tm._partition_merge_with_autograd(plan, x, mode)


def compared_destinations(case):
    """[n,Nb] bool: destinations whose value no uncertified source row can change (such a row may go to either of its
    two best destinations)."""
    cert = P.array(case, "cert")
    nb = P.positions(case)[1].shape[1]
    keep = np.ones((case["n"], nb), dtype=bool)
    if cert.all():
        return keep
    s = P.scores64(case)
    for g, i in zip(*np.nonzero(~cert)):
        keep[g, np.argsort(-s[g, i])[:2]] = False
    return keep


@pytest.mark.parametrize("case", P.cases(), ids=P.ids())
def test_dst_idx_matches_the_reference(case):
    pair = make_pair(case)
    plan = plan_of(pair)
    a, b = P.positions(case)
    assert plan.dst_idx.shape == (case["n"], a.shape[1], 1) and plan.dst_idx.dtype == torch.int64
    got = plan.dst_idx[..., 0].cpu().numpy()
    want, cert = P.array(case, "dst").astype(np.int64), P.array(case, "cert")
    assert got.min() >= 0 and got.max() < b.shape[1]
    assert np.array_equal(got[cert], want[cert]), f"{(got[cert] != want[cert]).sum()} certified rows differ"
    if not cert.all():
        s = P.scores64(case)
        for g, i in zip(*np.nonzero(~cert)):
            assert s[g, i, got[g, i]] >= s[g, i].max() - TAU
    # every 16-bit / fp32 form of the same values gives the same certified rows (all go through the fp32 matrix pipe)
    if case["dtype"] != "float32":
        again = plan_of(make_pair(case, dev(P.metric_of(case)))).dst_idx[..., 0].cpu().numpy()
        assert np.array_equal(again[cert], want[cert])
    # the inverted list is the stable grouping of dst_idx
    off, src = plan.offsets.cpu().numpy(), plan.sources.cpu().numpy()
    for g in range(case["n"]):
        order = np.argsort(got[g], kind="stable")
        assert np.array_equal(src[g], order)
        assert np.array_equal(off[g], np.concatenate([[0], np.cumsum(np.bincount(got[g], minlength=b.shape[1]))]))


@pytest.mark.parametrize("case", P.cases(), ids=P.ids())
def test_fp32_values_bit_exact_against_the_reference(case):
    """sum, mean, amax, merge_wavg and unmerge reproduce the reference's CPU values bit for bit on the compared
    destinations (all five turned out reproducible: no mode needed the 1-ulp-per-term allowance)."""
    tm = _tm()
    pair = make_pair(case)
    merge, unmerge = pair[0], pair[1]
    plan = plan_of(pair)
    step = case.get("row_step", 1)
    keep = compared_destinations(case)[:, ::step]
    x, size = dev(P.x_of(case)), dev(P.size_of(case))
    for mode in ("sum", "mean", "amax"):
        got = merge(x, mode=mode)
        assert got.shape == (case["n"], plan.Nb, case["C"])
        got = got[:, ::step].cpu().numpy()
        want = P.array(case, mode)
        assert np.array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32)), mode
    carrier = merge
    gx, gs = tm.merge_wavg(carrier, x, size)
    assert gs.shape == (case["n"], plan.Nb, 1)
    gx, gs = gx[:, ::step].cpu().numpy(), gs[:, ::step].cpu().numpy()
    assert np.array_equal(gx[keep].view(np.uint32), P.array(case, "wavg_x")[keep].view(np.uint32))
    assert np.array_equal(gs[keep], P.array(case, "wavg_s")[keep])
    # size=None is the all-ones size; log_size gives log(size')
    gx1, gs1 = tm.merge_wavg(carrier, x, None, log_size=True)
    wx1 = merge(x, mode="sum") / gs1
    assert torch.equal(gx1, wx1) and torch.equal(_abi().log_of_size(gs1), gs1.log())
    # unmerge: compared where the token's destination is a compared one
    y = merge(x, mode="mean")
    un = unmerge(y)
    assert un.shape[1] == plan.tokens_out
    a, b = P.positions(case)
    dst = plan.dst_idx[..., 0].cpu().numpy()
    full_keep = compared_destinations(case)
    tok_ok = np.zeros((case["n"], plan.tokens_out), dtype=bool)
    for g in range(case["n"]):
        tok_ok[g, b[g]] = full_keep[g]
        tok_ok[g, a[g]] = full_keep[g, dst[g]]
    got = un[:, ::4 * step].cpu().numpy()
    ok = tok_ok[:, ::4 * step]
    assert np.array_equal(got[ok].view(np.uint32), P.array(case, "unmerge")[ok].view(np.uint32))
    if P.has(case, "source"):
        src = tm.merge_source(carrier, x)
        assert src.shape == (case["n"], plan.Nb, case["T"])
        assert np.array_equal(src.cpu().numpy()[full_keep], P.array(case, "source").astype(np.float32)[full_keep])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", [c for c in P.cases() if c["id"] in ("k4_1568_clustered", "k3_197_concat", "r784_1568_bf16", "k8_3137_fp16")],
                         ids=lambda c: c["id"])
def test_16bit_values_are_the_rounded_fp32_result(case, dtype):
    tm = _tm()
    pair = make_pair(case)
    merge, plan = pair[0], plan_of(pair)
    carrier = merge
    xh = dev(P.x_of(case), dtype)
    sh = dev(P.size_of(case), dtype)
    for mode in ("sum", "mean", "amax", "amin", "prod"):
        assert torch.equal(merge(xh, mode=mode), merge(xh.float(), mode=mode).to(dtype)), mode
    gx, gs = tm.merge_wavg(carrier, xh, sh)
    wx, ws = tm.merge_wavg(carrier, xh.float(), sh.float())
    assert gx.dtype == dtype and torch.equal(gx, wx.to(dtype)) and torch.equal(gs, ws.to(dtype))
    assert torch.equal(pair[1](merge(xh)), pair[1](merge(xh).float()).to(dtype))


def test_kth_with_k2_names_the_destinations_of_the_even_odd_matching():
    tm = _tm()
    n, T, D = 3, 1568, 64
    metric = dev(synth.normal_like((n, T, D), 4242))
    merge, _ = tm.kth_bipartite_soft_matching(metric, 2)
    m2, _ = tm.bipartite_soft_matching(metric, T // 2)
    cv = closure_vars(m2)
    by_row = torch.empty(n, T // 2, dtype=torch.int64, device=DEV)
    by_row.scatter_(1, cv["src_idx"][..., 0], cv["dst_idx"][..., 0])
    assert torch.equal(merge.plan.dst_idx[..., 0], by_row)


@pytest.mark.parametrize("k,T", [(2, 1568), (4, 1568), (7, 1568), (3, 197)])
def test_kth_lengths_and_unmerge_structure(k, T):
    tm = _tm()
    n, C = 2, 24
    merge, unmerge = tm.kth_bipartite_soft_matching(dev(synth.normal_like((n, T, 64), 99 + k)), k)
    x = dev(synth.normal_like((n, T, C), 7))
    y = merge(x)
    assert y.shape == (n, T // k, C)
    u = unmerge(y)
    assert u.shape == (n, (T // k) * k, C)
    ug = u.reshape(n, T // k, k, C)
    assert torch.equal(ug[:, :, k - 1], y)
    dst = merge.plan.dst_idx.expand(n, merge.plan.Na, C)
    assert torch.equal(ug[:, :, :k - 1].reshape(n, -1, C), y.gather(1, dst))


def _adversary_plan(n, T, a_pos, b_pos, metric):
    return _abi().match_partition(metric, a_idx=dev(a_pos, torch.int64)[..., None], b_idx=dev(b_pos, torch.int64)[..., None])


@pytest.mark.parametrize("name", ["all_to_one", "one_destination", "one_source", "empty_destinations"])
def test_inverted_list_adversaries(name):
    """Legal inputs that stress the list builder; the result equals the framework-op evaluation of the same indices in
    fp64 on the GPU (sum: within the fp32 rounding of the accumulation; amax / list structure: exactly) and two runs
    give identical bits."""
    A = _abi()
    n, T, D, C = 2, 3137, 64, 16
    m = synth.normal_like((n, T, D), 31337)
    if name == "all_to_one":  # every source is a copy of destination 5: Na = 3129 sources name one row
        b_pos = np.broadcast_to(np.arange(0, 8) * 392, (n, 8)).copy()
        a_pos = np.stack([np.setdiff1d(np.arange(T), b_pos[g]) for g in range(n)])
        m[:, a_pos[0]] = m[:, b_pos[0, 5]][:, None, :] * 2.0
    elif name == "one_destination":  # Nb = 1, Na = 3136
        b_pos = np.full((n, 1), 17)
        a_pos = np.stack([np.setdiff1d(np.arange(T), b_pos[g]) for g in range(n)])
    elif name == "one_source":  # Na = 1
        a_pos = np.full((n, 1), 100)
        b_pos = np.stack([np.setdiff1d(np.arange(T), a_pos[g]) for g in range(n)])
    else:  # few distinct source directions: most destinations receive nothing
        a_pos = np.broadcast_to(np.arange(0, 2000), (n, 2000)).copy()
        b_pos = np.broadcast_to(np.arange(2000, T), (n, T - 2000)).copy()
        m[:, :2000] = m[:, 2000 + (np.arange(2000) % 3) * 7] * 0.5
    metric = dev(m)
    plan = _adversary_plan(n, T, a_pos, b_pos, metric)
    plan2 = _adversary_plan(n, T, a_pos, b_pos, metric)
    for f in ("dst_idx", "offsets", "sources"):
        assert torch.equal(getattr(plan, f), getattr(plan2, f)), f
    dst = plan.dst_idx[..., 0]
    if name == "all_to_one":
        assert bool((dst == 5).all())
    if name == "empty_destinations":
        assert int((plan.offsets[:, 1:] == plan.offsets[:, :-1]).sum()) >= n * (T - 2000 - 3)
    x = dev(synth.normal_like((n, T, C), 5))
    for mode in ("sum", "amax", "mean"):
        got = A.merge_partition(plan, x, mode)
        assert torch.equal(got, A.merge_partition(plan2, x, mode))
        want = ref_ops(plan, x.double(), mode)
        if mode == "amax":
            assert torch.equal(got.double(), want)
        else:
            terms = float((plan.offsets[:, 1:] - plan.offsets[:, :-1]).max()) + 1
            scale = ref_ops(plan, x.double().abs(), "sum")
            if mode == "mean":
                scale = scale / (plan.offsets[:, 1:] - plan.offsets[:, :-1] + 1)[..., None]
            assert bool(((got.double() - want).abs() <= terms * 2.0 ** -24 * scale + 1e-30).all()), mode
    u = A.unmerge_partition(plan, A.merge_partition(plan, x, "mean"))
    assert torch.equal(u, _tm()._partition_unmerge_with_autograd(plan, A.merge_partition(plan, x, "mean")))


def test_public_random_function_properties():
    tm = _tm()
    n, N, D, C, r = 3, 197, 64, 40, 50
    metric = dev(synth.clustered((n, N, D), 77))
    x = dev(synth.normal_like((n, N, C), 78))
    torch.manual_seed(1234)
    merge, unmerge = tm.random_bipartite_soft_matching(metric, r)
    cv = closure_vars(merge)
    assert {"a_idx", "b_idx", "dst_idx", "r"} <= set(cv)
    a, b = cv["a_idx"], cv["b_idx"]
    assert a.shape == (n, r, 1) and b.shape == (n, N - r, 1) and cv["dst_idx"].shape == (n, r, 1)
    both = torch.cat([a, b], dim=1)[..., 0].sort(dim=1).values
    assert torch.equal(both, torch.arange(N, device=DEV).expand(n, N))
    y = merge(x)
    assert y.shape == (n, N - r, C) and unmerge(y).shape == (n, N, C)
    torch.manual_seed(1234)
    merge2, unmerge2 = tm.random_bipartite_soft_matching(metric, r)
    assert torch.equal(merge2(x), y) and torch.equal(unmerge2(y), unmerge(y))
    plan = _abi().match_partition(metric, a_idx=a, b_idx=b)
    assert torch.equal(plan.dst_idx, cv["dst_idx"])
    assert torch.equal(_abi().merge_partition(plan, x, "mean"), y)
    # unmerge structure: a destination's position holds its row, a source's position its destination's row
    u = unmerge(y)
    assert torch.equal(u.gather(1, b.expand(n, N - r, C)), y)
    assert torch.equal(u.gather(1, a.expand(n, r, C)), y.gather(1, cv["dst_idx"].expand(n, r, C)))
    # kth closure variables, HeadMeanKeys metrics
    mk, _ = tm.kth_bipartite_soft_matching(metric, 3)
    assert {"dst_idx", "r", "k"} <= set(closure_vars(mk)) and closure_vars(mk)["r"] == (N // 3) * 2
    keys = dev(synth.normal_like((n, 4, N, 64), 5))
    mh, _ = tm.kth_bipartite_soft_matching(tm.HeadMeanKeys(keys), 3)
    mm, _ = tm.kth_bipartite_soft_matching(keys.mean(1), 3)
    assert torch.equal(mh.plan.dst_idx, mm.plan.dst_idx)
    with pytest.raises(ValueError):
        tm.random_bipartite_soft_matching(metric, N)
    with pytest.raises(ValueError):
        tm.kth_bipartite_soft_matching(metric, N + 1)


def test_closures_are_differentiable_when_tokens_require_grad():
    """Values and gradients equal the reference's op sequence (merge.py:137-156, :198-210) on the same indices."""
    tm = _tm()
    n, T, C = 2, 197, 24
    metric = dev(synth.normal_like((n, T, 64), 11))
    x0 = dev(synth.normal_like((n, T, C), 12))
    size0 = dev(synth.small_ints((n, T, 1), 13))
    torch.manual_seed(5)
    for merge, unmerge in (tm.kth_bipartite_soft_matching(metric, 3), tm.random_bipartite_soft_matching(metric, 60)):
        plan = merge.plan
        cv = closure_vars(merge)
        dst_idx, Na, Nb = cv["dst_idx"], plan.Na, plan.Nb

        def ref_split(t):
            c = t.shape[-1]
            if plan.k:
                g = t[:, :(T // plan.k) * plan.k].view(n, -1, plan.k, c)
                return g[:, :, :plan.k - 1].contiguous().view(n, -1, c), g[:, :, plan.k - 1]
            return t.gather(1, cv["a_idx"].expand(n, Na, c)), t.gather(1, cv["b_idx"].expand(n, Nb, c))

        def ref_merge(t, mode="mean"):
            src, dst = ref_split(t)
            return dst.scatter_reduce(-2, dst_idx.expand(n, Na, t.shape[-1]), src, reduce=mode)

        def ref_unmerge(t):
            c = t.shape[-1]
            src = t.gather(-2, dst_idx.expand(n, Na, c))
            if plan.k:
                return torch.cat([src.view(n, -1, plan.k - 1, c), t.view(n, -1, 1, c)], dim=-2).contiguous().view(n, -1, c)
            out = torch.zeros(n, T, c, device=t.device, dtype=t.dtype)
            out = out.scatter(-2, cv["a_idx"].expand(n, Na, c), src)
            return out.scatter(-2, cv["b_idx"].expand(n, Nb, c), t)

        for mode in ("mean", "sum", "amax"):
            xa, xb = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
            ya, yb = unmerge(merge(xa, mode=mode)), ref_unmerge(ref_merge(xb, mode=mode))
            assert ya.requires_grad and torch.equal(ya, yb)
            w = dev(synth.normal_like(tuple(ya.shape), 14))
            (ya * w).sum().backward()
            (yb * w).sum().backward()
            assert torch.equal(xa.grad, xb.grad), mode
        # the differentiable form agrees with the kernels (sum order may differ: fp32 rounding per added term)
        with torch.no_grad():
            yk = merge(x0, mode="sum")
        assert torch.allclose(yk, ref_merge(x0, "sum"), rtol=0, atol=2.0 ** -20 * float(x0.abs().max()) * plan.Na)
        xa, xb = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        wa, sa = tm.merge_wavg(merge, xa, size0)
        wb = ref_merge(xb * size0, "sum") / ref_merge(size0, "sum")
        assert wa.requires_grad and torch.equal(wa, wb) and torch.equal(sa, ref_merge(size0, "sum"))
        wa.square().sum().backward()
        wb.square().sum().backward()
        assert torch.equal(xa.grad, xb.grad)


def test_distill_token_unmerge_is_differentiable():
    """merge.py:87-100 with distill_token=True: the reference's unmerge reads [unmerged, destinations]."""
    tm = _tm()
    n, T, C, r = 2, 50, 16, 9
    metric = dev(synth.normal_like((n, T, 32), 21))
    merge, unmerge = tm.bipartite_soft_matching(metric, r, class_token=True, distill_token=True)
    cv = closure_vars(merge)
    unm_idx, src_idx, dst_idx = cv["unm_idx"], cv["src_idx"], cv["dst_idx"]
    y0 = dev(synth.normal_like((n, T - r, C), 22))

    def ref_unmerge(x):
        unm_len = unm_idx.shape[1]
        unm, dst = x[..., :unm_len, :], x[..., unm_len:, :]
        src = dst.gather(dim=-2, index=dst_idx.expand(n, r, C))
        out = torch.zeros(n, T, C, device=x.device, dtype=x.dtype)
        out[..., 1::2, :] = dst
        out = out.scatter(-2, (2 * unm_idx).expand(n, unm_len, C), unm)
        return out.scatter(-2, (2 * src_idx).expand(n, r, C), src)

    ya, yb = y0.clone().requires_grad_(True), y0.clone().requires_grad_(True)
    ua, ub = unmerge(ya), ref_unmerge(yb)
    assert ua.requires_grad and torch.equal(ua, ub)
    with torch.no_grad():
        assert torch.equal(unmerge(y0), ub)
    w = dev(synth.normal_like((n, T, C), 23))
    (ua * w).sum().backward()
    (ub * w).sum().backward()
    assert torch.equal(ya.grad, yb.grad)


def test_strided_views_are_read_correctly():
    tm = _tm()
    n, T, D, C = 2, 197, 64, 24
    big = dev(synth.normal_like((n, T + 1, D + 8), 41))
    view = big[:, 1:, :D]          # strided rows, unit channel stride: read in place
    tview = dev(synth.normal_like((n, D, T), 42)).transpose(1, 2)  # channel stride != 1: copied by the wrapper
    for metric in (view, tview):
        m1, u1 = tm.kth_bipartite_soft_matching(metric, 4)
        m2, u2 = tm.kth_bipartite_soft_matching(metric.contiguous(), 4)
        assert torch.equal(m1.plan.dst_idx, m2.plan.dst_idx)
    xbig = dev(synth.normal_like((n, T, 2 * C), 43))
    xv = xbig[:, :, ::2]
    assert not xv.is_contiguous()
    assert torch.equal(m1(xv), m1(xv.contiguous()))
    y = m1(xv)
    yv = torch.cat([y, y], dim=2)[:, :, :C]
    assert torch.equal(u1(yv), u1(yv.contiguous()))
    with pytest.raises(_abi().TomeHipError):
        m1(xv[:, :-1])
    with pytest.raises(_abi().TomeHipError):
        m1(xv.cpu())


def test_benchmark_batch_runs():
    """n = 384 groups of 1568 tokens (the benchmark's batch), bf16, C = 768: runs, and agrees with the framework ops
    on a few groups."""
    tm = _tm()
    n, T, D, C = 384, 1568, 64, 768
    g = torch.Generator(device=DEV).manual_seed(3)
    metric = torch.randn(n, T, D, device=DEV, generator=g).bfloat16()
    x = torch.randn(n, T, C, device=DEV, generator=g).bfloat16()
    for k in (2, 4):
        merge, unmerge = tm.kth_bipartite_soft_matching(metric, k)
        y, s = tm.merge_wavg(merge, x, None)
        assert y.shape == (n, T // k, C) and s.shape == (n, T // k, 1)
        assert float(s.float().sum()) == n * (T // k) * k
        plan = merge.plan
        # (the framework's scatter_reduce on the GPU adds in no fixed order: one bf16 step of the largest value)
        sub = _abi().PartitionPlan(4, T, plan.Na, plan.Nb, plan.k, None, None, plan.dst_idx[::97].contiguous(), None, None,
                                   plan.device)
        want = ref_ops(sub, x[::97].float(), "mean")
        assert torch.allclose(y[::97].float(), want, rtol=0, atol=2.0 ** -7 * float(want.abs().max()))
        assert unmerge(y).shape == (n, (T // k) * k, C)
