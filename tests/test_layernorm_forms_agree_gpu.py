"""The 16-bit form and the autocast form of a fused LayerNorm launch give the same bits where their contracts meet: a
16-bit stream and addend, and parameters that are 16-bit values widened to fp32.  Both forms call one body
(csrc/tome_ln_rows.h); this test holds them to it, and no forward saves mean or rstd, so it also holds the two backward
kernels to one recomputation.
Widths 8, 384, 512, 768, 1024: four, four, three, two and one row per wave, with lanes that hold no slot at 8 and
1024.  5 groups of 5 rows: the 25 rows leave a short last wave for four, three and two rows per wave.
Reference: none -- each pair is compared bit for bit (torch.equal), and the fp64 bounds of both forms are held by
tests/test_layernorm_accounting_gpu.py, test_layernorm_amp_gpu.py and test_merge_ln_amp_gpu.py."""
import pytest
import torch

import merge_ln_amp_oracle as mo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
WIDTHS = [8, 384, 512, 768, 1024]
GROUPS, GROUP_ROWS = 5, 5
N, T, R = 3, 12, 2  # the merge / drop plan
HALVES = [torch.bfloat16, torch.float16]
HALF_IDS = ["bf16", "fp16"]


def _abi():
    from tome import _abi
    return _abi


def _rand(shape, dtype, seed, scale=1.0, shift=0.0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=gen) * scale + shift).to(dtype).to(DEV)


def _params(C, half, seed):
    """weight and bias as 16-bit tensors, and the same values widened to fp32"""
    w, b = _rand((C,), half, seed, 0.5, 1.0), _rand((C,), half, seed + 1, 0.5)
    return w, b, w.float(), b.float()


@pytest.fixture(scope="module")
def plans():
    """One merge plan and one drop plan, n = 3, T = 12, r = 2, made once."""
    from tome import merge as tm
    metric = _rand((N, T, 16), torch.float32, 5)
    return {"merge": tm.bipartite_soft_matching(metric, R, False, False)[0].plan,
            "drop": tm.bipartite_soft_matching_drop(metric, R, False, False).plan}


@pytest.mark.parametrize("with_addend", [True, False], ids=["add", "ln_only"])
@pytest.mark.parametrize("skip_first", [False, True], ids=["plain", "skip_first"])
@pytest.mark.parametrize("half", HALVES, ids=HALF_IDS)
def test_add_layernorm(half, skip_first, with_addend):
    abi = _abi()
    for C in WIDTHS:
        x = _rand((GROUPS, GROUP_ROWS, C), half, 10 + C, 2.0, 0.5)
        a = _rand((GROUPS, GROUP_ROWS, C), half, 11 + C) if with_addend else None
        w, b, wf, bf = _params(C, half, 12 + C)
        x16, y16 = abi.add_layernorm(x, a, w, b, EPS, skip_first=skip_first)
        xam, yam = abi.add_layernorm_amp(x, a, wf, bf, EPS, half, skip_first=skip_first)
        assert y16.shape == yam.shape and y16.dtype == yam.dtype == half, C
        assert torch.equal(x16, xam), f"C={C}: x' differs between the 16-bit and the autocast form"
        assert torch.equal(y16, yam), f"C={C}: y differs between the 16-bit and the autocast form"


@pytest.mark.parametrize("half", HALVES, ids=HALF_IDS)
def test_drop_ln(half, plans):
    abi = _abi()
    plan = plans["drop"]
    for C in WIDTHS:
        x, a = _rand((N, T, C), half, 20 + C, 2.0, 0.5), _rand((N, T, C), half, 21 + C)
        w, b, wf, bf = _params(C, half, 22 + C)
        x16, y16 = abi.drop_ln(plan, x, w, b, EPS, addend=a)
        xam, yam = abi.drop_ln_amp(plan, x, wf, bf, EPS, half, addend=a)
        assert tuple(x16.shape) == (N, T - R, C), C
        assert torch.equal(x16, xam), f"C={C}: x_out"
        assert torch.equal(y16, yam), f"C={C}: y"


@pytest.mark.parametrize("half", HALVES, ids=HALF_IDS)
def test_merge_wavg_ln(half, plans):
    abi = _abi()
    plan = plans["merge"]
    recv = mo.received(plan.src_idx.cpu(), plan.dst_idx.cpu(), plan.unm_idx.cpu(), T, False).to(DEV)
    assert bool(recv.any()) and not bool(recv.all())
    gen = torch.Generator().manual_seed(3)
    size = torch.randint(1, 4, (N, T, 1), generator=gen).float().to(DEV)  # 1, 2 (moved as raw bits) and 3 (scaled)
    for C in WIDTHS:
        x, a = _rand((N, T, C), half, 30 + C, 2.0, 0.5), _rand((N, T, C), half, 31 + C)
        w, b, wf, bf = _params(C, half, 32 + C)
        x16, y16, s16 = abi.merge_wavg_ln(plan, x, size, w, b, EPS, addend=a, log_size=True)
        xam, yam, sam = abi.merge_wavg_ln_amp(plan, x, size, wf, bf, EPS, half, addend=a, log_size=True)
        assert torch.equal(x16, xam), f"C={C}: x_out"
        assert torch.equal(s16, sam), f"C={C}: size_out"
        assert torch.equal(s16._tome_log, sam._tome_log), f"C={C}: log(size_out)"
        # A row that receives sources is normalised by dst_row_finish in the 16-bit form (shuffle sum, division by C,
        # 1 / sqrt) and by merge_dst_row_amp in the autocast form (ln_rows' arithmetic): those rows of y may differ in
        # the last bit and are not compared here; every other row goes through ln_rows in both forms.
        assert torch.equal(y16[~recv], yam[~recv]), f"C={C}: y of the rows without sources"


@pytest.mark.parametrize("with_in", [True, False], ids=["gx_in", "no_gx_in"])
@pytest.mark.parametrize("skip_first", [False, True], ids=["plain", "skip_first"])
@pytest.mark.parametrize("half", HALVES, ids=HALF_IDS)
def test_layernorm_backward(half, skip_first, with_in):
    abi = _abi()
    for C in WIDTHS:
        xs = _rand((GROUPS, GROUP_ROWS, C), half, 40 + C, 2.0, 0.5)
        gy = _rand((GROUPS, GROUP_ROWS - 1 if skip_first else GROUP_ROWS, C), half, 41 + C)
        gi = _rand((GROUPS, GROUP_ROWS, C), half, 42 + C) if with_in else None
        w, _, wf, _ = _params(C, half, 43 + C)
        for want in (True, False):  # with the parameter gradients (slab walk) and with a frozen LayerNorm
            g16 = abi.layernorm_backward(gy, xs, gi, w, EPS, skip_first=skip_first, want_weight=want, want_bias=want)[0]
            gam = abi.layernorm_backward_amp(gy, xs, gi, wf, EPS, skip_first=skip_first, want_weight=want,
                                             want_bias=want)[0]
            assert g16.dtype == gam.dtype == half and g16.shape == gam.shape, C
            assert torch.equal(g16, gam), f"C={C} params={want}: gx differs between the 16-bit and the autocast form"
