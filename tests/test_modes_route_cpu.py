"""Which launch `merge_then_norm` / `merge_then_norm_regrouped` (tome/patch/_common.py) take, per reduction mode, on CPU
tensors with every launch seam replaced by a recorder: the fused reduction + LayerNorm entries (`_abi.merge_wavg_ln`,
`_abi.drop_ln`, `_abi.merge_wavg_regrouped(ln=)`, `_abi.drop_regrouped(ln=)`), the matchings, the source tracking and the
model's own (unfused) reduction function.  `_abi._ln_of` is the real predicate without its `x.is_cuda` clause; grad mode,
dtypes and the switches are the real thing.  A literal table holds (mode, grad, token dtype, autocast, trace_source,
_FUSE_LN, _FUSE_ADD, _FUSE_MODES, clamped r == 0) against (launch, whether the residual went in as addend); fc2's bias is
folded into the stream by the plain-merge launch alone."""
import types

import pytest
import torch

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
C_ = 16
MERGE_LN, DROP_LN, UNFUSED = "merge_wavg_ln", "drop_ln", "unfused"

# mode, grad, dtype, autocast, trace, FUSE_LN, FUSE_ADD, FUSE_MODES, r0 -> launch, residual fused as addend
TABLE = [
    # plain merge: as ever, whatever the new switch says
    ("merge", False, BF, False, False, True, True, True, False, MERGE_LN, True),
    ("merge", False, BF, False, False, True, True, False, False, MERGE_LN, True),
    ("merge", False, HF, False, False, True, False, True, False, MERGE_LN, False),
    ("merge", False, BF, False, True, True, True, True, False, MERGE_LN, False),
    ("merge", False, BF, False, False, False, True, True, False, UNFUSED, False),
    ("merge", True, BF, False, False, True, True, True, False, UNFUSED, False),
    ("merge", False, F32, False, False, True, True, True, False, UNFUSED, False),
    ("merge", False, BF, False, False, True, True, True, True, "nothing", False),
    # random_merge joins the merge launch; not with the switch off
    ("random_merge", False, BF, False, False, True, True, True, False, MERGE_LN, True),
    ("random_merge", False, BF, False, False, True, True, False, False, UNFUSED, False),
    ("random_merge", False, BF, False, False, False, True, True, False, UNFUSED, False),
    ("random_merge", True, BF, False, False, True, True, True, False, UNFUSED, False),
    ("random_merge", False, BF, False, False, True, True, True, True, "nothing", False),
    # hybrid: the merge entry with the plan's flags
    ("hybrid", False, BF, False, False, True, True, True, False, MERGE_LN, True),
    ("hybrid", False, HF, False, False, True, True, True, False, MERGE_LN, True),
    ("hybrid", False, BF, False, False, True, False, True, False, MERGE_LN, False),
    ("hybrid", False, BF, False, True, True, True, True, False, MERGE_LN, False),
    ("hybrid", False, BF, False, False, True, True, False, False, UNFUSED, False),
    ("hybrid", False, BF, False, False, False, True, True, False, UNFUSED, False),
    ("hybrid", True, BF, False, False, True, True, True, False, UNFUSED, False),
    ("hybrid", False, F32, False, False, True, True, True, False, UNFUSED, False),
    ("hybrid", False, BF, True, False, True, True, True, False, UNFUSED, False),
    ("hybrid", False, BF, False, False, True, True, True, True, "nothing", False),
    # drop and random_drop: the drop entry
    ("drop", False, BF, False, False, True, True, True, False, DROP_LN, True),
    ("drop", False, HF, False, False, True, True, True, False, DROP_LN, True),
    ("drop", False, BF, False, False, True, False, True, False, DROP_LN, False),
    ("drop", False, BF, False, True, True, True, True, False, DROP_LN, False),
    ("drop", False, BF, False, False, True, True, False, False, UNFUSED, False),
    ("drop", False, BF, False, False, False, True, True, False, UNFUSED, False),
    ("drop", True, BF, False, False, True, True, True, False, UNFUSED, False),
    ("drop", False, F32, False, False, True, True, True, False, UNFUSED, False),
    ("drop", False, BF, True, False, True, True, True, False, UNFUSED, False),
    ("drop", False, BF, False, False, True, True, True, True, "nothing", False),
    ("random_drop", False, BF, False, False, True, True, True, False, DROP_LN, True),
    ("random_drop", False, BF, False, False, True, True, False, False, UNFUSED, False),
    ("random_drop", True, BF, False, False, True, True, True, False, UNFUSED, False),
]
# the interleaved layouts never fuse while tracing sources, and their predicate asks for a clamped r > 0 up front
REGROUPED_DIFFERS = {"trace": UNFUSED, "r0": UNFUSED}


def _ids(table):
    return ["-".join(str(v).replace("torch.", "") for v in row[:9]) for row in table]


class Seams:
    def __init__(self, monkeypatch, r0):
        from tome import _abi, _ln
        from tome.merge import do_nothing
        from tome.patch import _common as C
        self.C, self.calls, self.r0 = C, [], r0

        def ln_of(x, norm):  # _abi._ln_of without `x.is_cuda`
            c = x.shape[-1]
            return (norm.elementwise_affine and norm.bias is not None and tuple(norm.normalized_shape) == (c,)
                    and x.dtype in _abi._HALF and norm.weight.dtype == x.dtype and c % 8 == 0 and c <= 1024)

        monkeypatch.setattr(_abi, "_ln_of", ln_of)
        plan = types.SimpleNamespace(n=2, T=8, r=2, edge_keep=None)

        def matching(name, pair):
            def match(metric, r, class_token=False, distill_token=False, mode=None, threshold=None):
                self.calls.append(("match", name, r, mode, threshold))
                if self.r0:
                    return do_nothing, do_nothing
                fn = types.SimpleNamespace(plan=plan)
                return (fn, fn) if pair else fn
            return match

        monkeypatch.setattr(C, "bipartite_soft_matching", matching("merge", True))
        monkeypatch.setattr(C, "bipartite_soft_matching_hybrid", matching("hybrid", True))
        monkeypatch.setattr(C, "bipartite_soft_matching_drop", matching("drop", False))
        monkeypatch.setattr(C, "merge_source", lambda merge, x, source: self.calls.append(("merge_source",)) or "src")
        monkeypatch.setattr(C, "_drop_source", lambda drop, source, n, t, dev: self.calls.append(("drop_source",)) or "src")

        def out(x, drop_rows=2):
            return x[:, drop_rows:].clone()

        def merge_wavg_ln(plan, x, size, w, b, eps, addend=None, log_size=False, out_bias=None):
            self.calls.append((MERGE_LN, addend is not None, out_bias is not None))
            return out(x), out(x), torch.ones(x.shape[0], x.shape[1] - 2, 1)

        def drop_ln(plan, x, w, b, eps, addend=None, out_bias=None):
            self.calls.append((DROP_LN, addend is not None, out_bias is not None))
            return out(x), out(x)

        def merge_wavg_regrouped(plan, x, size, frames, has_cls=True, ln=None, addend=None, log_size=False,
                                 addend_grouped=None, cls_addend=None, out_bias=None):
            assert ln is not None
            self.calls.append((MERGE_LN, addend is not None or addend_grouped is not None, out_bias is not None))
            return out(x, 2 * frames), out(x, 2 * frames), torch.ones(plan.n, plan.T - plan.r, 1)

        def drop_regrouped(plan, x, frames, has_cls=True, ln=None, addend=None, addend_grouped=None, cls_addend=None,
                           out_bias=None):
            assert ln is not None
            self.calls.append((DROP_LN, addend is not None or addend_grouped is not None, out_bias is not None))
            return out(x, 2 * frames), out(x, 2 * frames)

        for name, fn in (("merge_wavg_ln", merge_wavg_ln), ("drop_ln", drop_ln),
                         ("merge_wavg_regrouped", merge_wavg_regrouped), ("drop_regrouped", drop_regrouped)):
            monkeypatch.setattr(_abi, name, fn)

        def add_layernorm(x, addend, norm, skip_first=False, how=None):
            self.calls.append(("trailing_ln_kernel", how))
            return x, torch.nn.functional.layer_norm(x.float(), (x.shape[-1],)).to(x.dtype), False

        monkeypatch.setattr(_ln, "add_layernorm", add_layernorm)

    def launches(self):
        return [c for c in self.calls if c[0] in (MERGE_LN, DROP_LN, UNFUSED)]


def _reducers(seams, regrouped):
    """the model's three reduction functions: they pop r and record that the reduction ran on its own"""
    def make(name):
        if regrouped:
            def reduce(metric, x, info, frames):
                r = info["r"].pop(0)
                seams.calls.append((UNFUSED, name, x.dtype))
                return x[:, 2 * frames:] if r > 0 and not seams.r0 else x
        else:
            def reduce(metric, x, info):
                r = info["r"].pop(0)
                seams.calls.append((UNFUSED, name, x.dtype))
                return x[:, 2:] if r > 0 and not seams.r0 else x
        return reduce
    return make("merge"), make("drop"), make("hybrid")


def _fc2(dtype):
    """the Linear that finishes the block, as `foldable` hands it over"""
    return torch.nn.Linear(4 * C_, C_).requires_grad_(False).to(dtype)


def _info(mode, trace, r):
    from tome.patch import _common as C
    info = C.new_tome_info(trace, True, mode, "mean", 0.25, False, class_token=False)
    info["r"] = [r, r]
    return info


def _setup(monkeypatch, row):
    mode, grad, dtype, autocast, trace, fuse_ln, fuse_add, fuse_modes, r0 = row[:9]
    from tome import _abi
    seams = Seams(monkeypatch, r0)
    C = seams.C
    monkeypatch.setattr(C, "_FUSE_LN", fuse_ln)
    monkeypatch.setattr(C, "_FUSE_ADD", fuse_add)
    monkeypatch.setattr(C, "_FUSE_MODES", fuse_modes)
    monkeypatch.setattr(_abi, "autocast_dtype", lambda device: BF if autocast else None)
    # under autocast the model keeps fp32 master weights: the LayerNorm is not the fused launch's kind
    norm = torch.nn.LayerNorm(C_).requires_grad_(grad).to(F32 if autocast else dtype)
    return seams, C, norm


@pytest.mark.parametrize("row", TABLE, ids=_ids(TABLE))
def test_flat_layout_route(row, monkeypatch):
    mode, grad, dtype, autocast, trace, _, _, fuse_modes, r0, want, want_add = row
    seams, C, norm = _setup(monkeypatch, row)
    merge_fn, drop_fn, hybrid_fn = _reducers(seams, False)
    fn = C.pick_reduction(mode, merge_fn, drop_fn, hybrid_fn)
    info = _info(mode, trace, 2)
    x = torch.randn(2, 8, C_).to(dtype).requires_grad_(grad)
    res = torch.randn(2, 8, C_).to(dtype)
    with torch.set_grad_enabled(grad):
        xo, y = C.merge_then_norm(None, x, info, norm, fn, merge_fn, residual=res, fold=_fc2(dtype), drop_fn=drop_fn,
                                  hybrid_fn=hybrid_fn)
    got = seams.launches()
    assert info["r"] == [2], "exactly one r is consumed"
    if want == "nothing":  # the fused route found a clamped r of 0: no reduction launch, x + residual and norm(x)
        assert got == [] and xo.shape == x.shape and torch.equal(xo, x + res)
        assert torch.equal(y, norm(xo))
    else:
        assert len(got) == 1 and got[0][0] == want, got
        if want == UNFUSED:
            kind = {"random_merge": "merge", "random_drop": "drop"}.get(mode, mode)
            assert got[0][1] == kind
        else:
            assert got[0][1] is want_add, got
            # fc2's bias goes into the stream in plain 'merge' alone: the other modes keep the bits of the three steps
            assert got[0][2] is (mode == "merge") and ("_folded" in info) is (mode == "merge"), got
    matches = [c for c in seams.calls if c[0] == "match"]
    if want in (MERGE_LN, DROP_LN, "nothing"):
        # one matching, the mode's own, with the mode string (the random generator is consumed as on the unfused path)
        which = "drop" if mode in ("drop", "random_drop") else "hybrid" if mode == "hybrid" else "merge"
        assert matches == [("match", which, 2, mode, 0.25 if which == "hybrid" else None)]
        tracked = [c[0] for c in seams.calls if c[0].endswith("_source")]
        expect = [] if not trace or (want == "nothing" and mode in ("merge",)) else \
            ["drop_source" if which == "drop" else "merge_source"]
        assert tracked == expect
        if want == DROP_LN:
            assert info["size"].dtype == F32 and tuple(info["size"].shape) == (2, 6, 1) and bool((info["size"] == 1).all())
    else:
        assert matches == []


REGROUPED = [r for r in TABLE]


@pytest.mark.parametrize("grouped", [False, True], ids=["residual", "GroupedResidual"])
@pytest.mark.parametrize("row", REGROUPED, ids=_ids(REGROUPED))
def test_regrouped_layout_route(row, grouped, monkeypatch):
    mode, grad, dtype, autocast, trace, _, fuse_add, _, r0, want, want_add = row
    if trace:
        want, want_add = REGROUPED_DIFFERS["trace"], False
    seams, C, norm = _setup(monkeypatch, row)
    merge_fn, drop_fn, hybrid_fn = _reducers(seams, True)
    fn = C.pick_reduction(mode, merge_fn, drop_fn, hybrid_fn)
    B, F, P = 1, 2, 8
    r = 0 if r0 else 2  # (the interleaved predicate clamps r itself; P // 2 = 4 >= 2)
    if r0:
        want, want_add = REGROUPED_DIFFERS["r0"], False
    info = _info(mode, trace, r)
    x = torch.randn(B, 1 + P * F, C_).to(dtype).requires_grad_(grad)
    if grouped:
        res = C.GroupedResidual(torch.randn(B * F, 1 + P, C_).to(dtype), torch.randn(B, 1, C_).to(dtype), B, F, P)
    else:
        res = torch.randn(B, 1 + P * F, C_).to(dtype)
    with torch.set_grad_enabled(grad):
        C.merge_then_norm_regrouped(None, x, info, norm, lambda z: fn(None, z, info, F), fn is merge_fn, F, residual=res,
                                    fold=_fc2(dtype), is_drop=fn is drop_fn, is_hybrid=fn is hybrid_fn)
    got = seams.launches()
    assert info["r"] == [r]
    assert len(got) == 1 and got[0][0] == want, got
    if want != UNFUSED:
        assert got[0][1] is want_add
        assert got[0][2] is (mode == "merge") and ("_folded" in info) is (mode == "merge"), got
        which = "drop" if mode in ("drop", "random_drop") else "hybrid" if mode == "hybrid" else "merge"
        assert [c for c in seams.calls if c[0] == "match"] == [("match", which, 2, mode, 0.25 if which == "hybrid" else None)]


def test_positional_call_forms_behave_as_before(monkeypatch):
    """The call forms of tests/test_layernorm_backward_gpu.py and test_layernorm_regrouped_backward_gpu.py -- no new
    keyword -- know the plain merge alone: 'merge' fuses, every other mode runs the reduction on its own."""
    for mode, want in (("merge", MERGE_LN), ("drop", UNFUSED), ("hybrid", UNFUSED), ("random_merge", MERGE_LN),
                       ("random_drop", UNFUSED)):
        row = (mode, False, BF, False, False, True, True, True, False)
        seams, C, norm = _setup(monkeypatch, row)
        merge_fn, drop_fn, hybrid_fn = _reducers(seams, False)
        fn = C.pick_reduction(mode, merge_fn, drop_fn, hybrid_fn)
        x, res = torch.randn(2, 8, C_).to(BF), torch.randn(2, 8, C_).to(BF)
        with torch.no_grad():
            C.merge_then_norm(None, x, _info(mode, False, 2), norm, fn, merge_fn, res)
        assert [c[0] for c in seams.launches()] == [want], mode
        seams, C, norm = _setup(monkeypatch, row)
        merge_fn, drop_fn, hybrid_fn = _reducers(seams, True)
        fn = C.pick_reduction(mode, merge_fn, drop_fn, hybrid_fn)
        info = _info(mode, False, 2)
        xf, rf = torch.randn(1, 17, C_).to(BF), torch.randn(1, 17, C_).to(BF)
        with torch.no_grad():
            C.merge_then_norm_regrouped(None, xf, info, norm, lambda z: fn(None, z, info, 2), fn is merge_fn, 2, rf)
        assert [c[0] for c in seams.launches()] == [want], mode
    # ... and with the new switch off, 'random_merge' is the parent's three steps again
    row = ("random_merge", False, BF, False, False, True, True, False, False)
    seams, C, norm = _setup(monkeypatch, row)
    merge_fn, _, _ = _reducers(seams, False)
    with torch.no_grad():
        C.merge_then_norm(None, torch.randn(2, 8, C_).to(BF), _info("random_merge", False, 2), norm, merge_fn, merge_fn,
                          torch.randn(2, 8, C_).to(BF))
    assert [c[0] for c in seams.launches()] == [UNFUSED]


@pytest.mark.parametrize("kind, mode", [("merge", "merge"), ("merge", "random_merge"), ("hybrid", "hybrid"),
                                        ("drop", "drop"), ("drop", "random_drop")])
def test_matching_helper(kind, mode, monkeypatch):
    """`matching(kind, metric, r, info)`: the kind's own matching, looked up on the module, with info's tokens, mode and
    threshold; the callable that carries the plan, or None exactly when the matching reports a clamped r of 0 -- the
    (do_nothing, do_nothing) pair, which is also the tuple the drop matching then answers with."""
    from tome.merge import do_nothing
    for r0 in (False, True):
        seams = Seams(monkeypatch, r0)
        C = seams.C
        info = _info(mode, False, 2)
        info["class_token"], info["distill_token"] = True, False
        got = C.matching(kind, "metric", 3, info)
        assert seams.calls == [("match", kind, 3, mode, 0.25 if kind == "hybrid" else None)]
        if r0:
            assert got is None
        else:
            assert got is not None and got is not do_nothing and got.plan.r == 2
    # the answers' forms one by one, and the arguments as the matchings receive them
    seen = []
    carrier = types.SimpleNamespace(plan="plan")
    for name, answer in (("bipartite_soft_matching", (carrier, "unmerge")),
                         ("bipartite_soft_matching_hybrid", (carrier, "unmerge")),
                         ("bipartite_soft_matching_drop", carrier)):
        monkeypatch.setattr(C, name, lambda *a, _name=name, _answer=answer: seen.append((_name,) + a) or _answer)
    assert C.matching(kind, "metric", 3, info) is carrier
    which = {"merge": "bipartite_soft_matching", "hybrid": "bipartite_soft_matching_hybrid",
             "drop": "bipartite_soft_matching_drop"}[kind]
    assert seen == [(which, "metric", 3, True, False, mode) + ((0.25,) if kind == "hybrid" else ())]
    for name in ("bipartite_soft_matching", "bipartite_soft_matching_hybrid", "bipartite_soft_matching_drop"):
        monkeypatch.setattr(C, name, lambda *a: (do_nothing, do_nothing))
    assert C.matching(kind, "metric", 3, info) is None


def test_fused_kind_table():
    from tome.patch import _common as C
    assert C._FUSE_MODES is True  # the default
    kinds = {(m, f): C.fused_kind(m, f == "merge", f == "drop", f == "hybrid")
             for m in ("merge", "random_merge", "drop", "random_drop", "hybrid") for f in ("merge", "drop", "hybrid")}
    assert {k: v for k, v in kinds.items() if v} == {
        ("merge", "merge"): "merge", ("random_merge", "merge"): "merge", ("drop", "drop"): "drop",
        ("random_drop", "drop"): "drop", ("hybrid", "hybrid"): "hybrid"}
