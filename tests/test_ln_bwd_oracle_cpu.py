"""CPU side of the LayerNorm backward (tests/ln_bwd_oracle.py): the bound accepts an fp32 evaluation of the kernel's
formula and rejects the wrong answers such a kernel can give; the two new entries are exported, bound and refuse bad
arguments on the host with a message.  No kernel is launched here."""
import ctypes

import pytest
import torch

import ln_bwd_oracle as bo

DTYPES = [torch.bfloat16, torch.float16]
EPS = 1e-5
# (rows as [B, N], C): N = 16 and 128 rows per clip, 32 clips
SHAPES = [((32, 16), 8), ((32, 16), 64), ((32, 16), 96), ((32, 16), 384), ((32, 16), 768), ((32, 16), 1024),
          ((32, 128), 64), ((32, 128), 96), ((32, 128), 384), ((32, 128), 768), ((32, 128), 1024)]


def _case(shape, C, dtype, seed, **kw):
    return bo.make_inputs((*shape, C), dtype, seed, **kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_bound_accepts_an_fp32_evaluation(dtype):
    """Rows 30 standard deviations from zero and rows around zero, gradients of size 1 and 1e-3, with and without
    gx_in, plain and skip_first: every element of gx, dweight and dbias of the fp32 emulation lies inside the bound."""
    seed = 0
    for shape, C in SHAPES:
        for far, scale, with_in, skip in ((True, 1.0, True, False), (True, 1e-3, False, False), (False, 1.0, True, True),
                                          (True, 1e-3, True, True)):
            seed += 1
            gy, xs, gi, w = _case(shape, C, dtype, seed, far=far, grad_scale=scale, skip_first=skip, with_in=with_in)
            ref = bo.reference(gy, xs, gi, w, EPS, skip_first=skip)
            gx, dw, db = bo.emulate_fp32(gy, xs, gi, w, EPS, skip_first=skip)
            bo.check(f"fp32 emulation {shape} C={C} far={far} scale={scale} in={with_in} skip={skip} {dtype}", gx, dw, db,
                     ref, dtype)
            if skip:
                want = torch.zeros_like(xs[:, 0]) if gi is None else gi[:, 0]
                assert torch.equal(gx[:, 0], want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("slip", ["no_xhat_term", "neighbour_rstd", "chunk_out_of_mean"])
def test_bound_rejects_a_wrong_gx(slip, dtype):
    """At every C >= 64 of SHAPES at least 95 % of the rows hold an element outside the bound when the xhat * mean(gw xhat)
    term is left out, a row is scaled with its neighbour's rstd, or a 16-byte chunk is left out of mean(gw)."""
    seed = 100
    for shape, C in SHAPES:
        if C < 64:
            continue
        for with_in in (False, True):
            seed += 1
            gy, xs, gi, w = _case(shape, C, dtype, seed, far=True, with_in=with_in)
            ref = bo.reference(gy, xs, gi, w, EPS)
            gx, _, _ = bo.emulate_fp32(gy, xs, gi, w, EPS, slip=slip)
            bad, _ = bo.outside_gx(gx, ref, dtype)
            share = float(bad.double().mean())
            print(f"{slip} {shape} C={C} in={with_in} {dtype}: {100 * share:.1f} % of the rows rejected")
            assert share >= 0.95, (slip, shape, C, with_in, share)


def _rejected_share(slip, shape, C, dtype, seed):
    """Share of the channels of dweight and of dbias outside the bound, counted over enough seeds for 1024 channels
    (the share of 64 channels moves in steps of 1.6 %)."""
    skip = slip == "class_row_counted"
    bad = {"dw": [], "db": []}
    for k in range(-(-1024 // C)):
        gy, xs, gi, w = _case(shape, C, dtype, seed + k, far=True, skip_first=skip)
        ref = bo.reference(gy, xs, gi, w, EPS, skip_first=skip)
        _, dw, db = bo.emulate_fp32(gy, xs, gi, w, EPS, skip_first=skip, slip=slip)
        for which, got in (("dw", dw), ("db", db)):
            bad[which].append(bo.outside_param(got, ref, which, dtype)[0])
    return {which: float(torch.cat(v).double().mean()) for which, v in bad.items()}


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_bound_rejects_the_class_row_counted_in_the_parameter_gradients(dtype):
    """skip_first with the class row's share added, groups of 16 rows: at every C >= 64 of SHAPES, at 512 rows and at
    4096 rows (up to 512 partial rows), at least 95 % of the channels of dweight and of dbias fall outside the bound."""
    widths = sorted({C for _, C in SHAPES if C >= 64})
    for i, (shape, C) in enumerate([((B, 16), C) for B in (32, 256) for C in widths]):
        share = _rejected_share("class_row_counted", shape, C, dtype, 200 + 40 * i)
        print(f"class_row_counted {shape} C={C} {dtype}: rejected {share}, parts {bo.form(shape[0] * shape[1], C)[2]}")
        assert min(share.values()) >= 0.95, (shape, C, share)


# launches of at most 64 partial rows at every C >= 64 of SHAPES (C = 1024 holds four rows per partial row: 64 and
# 128 rows; C = 768 eight): tests/ln_bwd_oracle.py, "what no bound can show"
FEW_PARTS = [((32, 16), 64), ((32, 16), 96), ((32, 16), 384), ((32, 16), 768), ((4, 16), 1024), ((8, 16), 1024),
             ((32, 32), 64), ((32, 32), 96), ((32, 32), 384), ((16, 16), 768)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_bound_rejects_a_dropped_partial_row(dtype):
    """One workgroup's partial row left out of dweight / dbias: at least 95 % of the channels fall outside the bound."""
    assert {C for _, C in FEW_PARTS} >= {C for _, C in SHAPES if C >= 64}
    for i, (shape, C) in enumerate(FEW_PARTS):
        parts = bo.form(shape[0] * shape[1], C)[2]
        assert parts <= 64
        share = _rejected_share("partial_dropped", shape, C, dtype, 900 + 40 * i)
        print(f"partial_dropped {shape} C={C} {dtype}: rejected {share}, parts {parts}")
        assert min(share.values()) >= 0.95, (shape, C, share)


def test_form_walks_every_row_once():
    for rows in (1, 5, 511, 512, 4096, 100_352, 602_112):
        for C in (8, 64, 96, 384, 392, 768, 1024):
            R, spw, parts = bo.form(rows, C)
            assert 1 <= R <= 4 and R * (C // 8) <= 3 * bo.WAVE and parts <= bo.MAX_PARTS
            assert parts * spw * 4 * R >= rows > (parts - 1) * spw * 4 * R


def test_new_entries_are_listed_and_bound():
    from tome import _abi
    L = _abi.lib()
    for name in ("tome_layernorm_backward_workspace_bytes", "tome_layernorm_backward"):
        assert name in _abi.SYMBOLS and hasattr(L, name)
    assert L.tome_abi_version() == 11
    for rows, C in ((100, 64), (4096, 768), (602_112, 768)):
        assert L.tome_layernorm_backward_workspace_bytes(rows, C) >= bo.form(rows, C)[2] * 2 * C * 4
    for rows, C in ((0, 64), (10, 12), (10, 1032), (2 ** 31, 8)):
        assert L.tome_layernorm_backward_workspace_bytes(rows, C) == 0


def test_host_side_refusals():
    from tome import _abi
    L = _abi.lib()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    eps = ctypes.c_float(1e-5)

    def call(gy=p, xs=p, gi=None, dtype=1, groups=2, group_rows=4, skip=0, C=64, w=p, gx=p, dw=None, db=None, ws=None):
        return L.tome_layernorm_backward(gy, xs, gi, dtype, groups, group_rows, skip, C, w, eps, gx, dw, db, ws, None)

    for kw, word in (({"gy": None}, "null"), ({"xs": None}, "null"), ({"w": None}, "null"), ({"gx": None}, "null"),
                     ({"dtype": 0}, "16-bit"), ({"dtype": 7}, "16-bit"), ({"C": 12}, "C % 8"), ({"C": 1032}, "C <= 1024"),
                     ({"C": 0}, "C % 8"), ({"groups": 0}, "rows"), ({"skip": 1, "group_rows": 1}, "skip_first"),
                     ({"gy": p + 2}, "aligned"), ({"dw": p}, "workspace"), ({"db": p}, "workspace")):
        rc = call(**kw)
        msg = L.tome_last_error().decode()
        assert rc != 0 and "tome_layernorm_backward" in msg and word in msg, (kw, rc, msg)


def test_python_wrapper_has_no_cpu_path():
    from tome import _abi
    gy, xs, gi, w = bo.make_inputs((4, 64), torch.bfloat16, 1)
    with pytest.raises(_abi.TomeHipError, match="no CPU path"):
        _abi.layernorm_backward(gy, xs, gi, w, 1e-5)


def test_older_library_without_the_entries_says_so():
    """A v11 library built before the entries were added: a clear TomeHipError, not an AttributeError."""
    from tome import _abi

    class Old:
        pass
    with pytest.raises(_abi.TomeHipError, match="tome_layernorm_backward is missing"):
        _abi.require_symbol(Old(), "tome_layernorm_backward")


def test_ln_trainable_is_ln_fusable_without_the_grad_clause():
    from tome import _abi
    norm = torch.nn.LayerNorm(64).to(torch.bfloat16)
    x = torch.zeros(2, 3, 64, dtype=torch.bfloat16)
    assert not _abi.ln_trainable(x, norm)  # CPU tensors
    assert not _abi.ln_trainable(x.float(), norm)
