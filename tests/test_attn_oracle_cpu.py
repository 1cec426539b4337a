"""The attention checks of tests/attn_oracle.py reject wrong answers (CPU, no GPU): outputs of deliberately wrong
attention -- a key dropped, counted twice, a tile dropped, the size bias on the neighbouring key, the TimeSformer
form's class query or class key biased, another batch's or head's values -- computed in fp64 and rounded to the
16-bit format as a kernel would, must all fail the checks the GPU tests apply (test_attention_accounting_gpu.py),
and the correct output must pass them.  So those tests catch these bug classes at the shapes they run."""
import pytest
import torch

import attn_oracle as A

B, H = 2, 3
DTYPES = (torch.bfloat16, torch.float16)


def _counting_output(mult, chan, N, dtype, denom=None):
    """What attention with q = 0 and one-hot values returns when key j is counted mult[j] times (0: dropped):
    the channel sums of mult over sum(mult) (or over `denom`: a key left in the row sum but not in the product),
    rounded to the 16-bit format.  mult [Nk]; chan [B, H, Nk].  -> [B, N, H, 64]"""
    m = mult.double().expand(chan.shape)
    cnt = torch.zeros(B, H, 64, dtype=torch.float64).scatter_add_(-1, chan, m)
    den = m.sum(-1, keepdim=True) if denom is None else float(denom)
    return (cnt / den).unsqueeze(1).expand(B, N, H, 64).to(dtype)


def _rejected_by(mult, Nk, dtype, denom=None):
    """The encodings under which check_counts rejects the output of key multiplicities `mult` (the GPU tests run
    both on every shape, so a mistake is caught when either rejects it)."""
    out = set()
    for enc in ("mod", "tile"):
        chan = A.channel_of(B, H, Nk, enc)
        try:
            A.check_counts(_counting_output(mult, chan, 3, dtype, denom), A.expected_counts(B, H, Nk, enc), Nk)
        except AssertionError:
            out.add(enc)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Nk", [2, 65, 200, 1568, 3137])
def test_counting_check_rejects_every_miscounted_key(Nk, dtype):
    """Every key position of the first and of the last (partly filled) tile dropped -- from the product and the row
    sum, or from the product only (a mask applied to P but not to l) -- or counted twice: rejected under the "mod"
    encoding (a key of its own in its channel among the nearest 64).  A whole tile dropped: rejected by the tile
    encoding -- under "mod" it takes one key from every channel, and once the row sum loses the same 64 keys the
    shares hardly move; conversely, "tile" cannot see a renormalised drop inside a channel that holds every key of a
    short row.  The GPU tests run both."""
    ones = torch.ones(Nk, dtype=torch.float64)
    assert _rejected_by(ones, Nk, dtype) == set()
    keys = sorted(set(range(0, min(64, Nk))) | set(range((Nk - 1) // 64 * 64, Nk)))
    assert Nk - 1 in keys
    for j in keys:
        for name, mult, denom in (("dropped", 0.0, None), ("masked from O only", 0.0, Nk), ("counted twice", 2.0, None)):
            m = ones.clone()
            m[j] = mult
            assert "mod" in _rejected_by(m, Nk, dtype, denom), (j, name)
    if Nk > 128:
        m = ones.clone()
        m[64:128] = 0.0
        assert "tile" in _rejected_by(m, Nk, dtype), "tile 1 dropped"
        assert _rejected_by(m, Nk, dtype, denom=Nk) == {"mod", "tile"}, "tile 1 masked from O only"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Nk", [1, 200, 1568])
def test_counting_check_rejects_another_slices_values(Nk, dtype):
    """Values read from the neighbouring batch or head (the one-hot channels rotate with b and h)."""
    counts = A.expected_counts(B, H, Nk, "mod")
    for dim in (0, 2):  # counts [B, 1, H, 64]: batch, head
        for shift in (1, -1):
            wrong = torch.roll(counts, shift, dims=dim)
            with pytest.raises(AssertionError):
                A.check_counts((wrong / Nk).expand(B, 5, H, 64).to(dtype), counts, Nk, f"dim {dim} shift {shift}")


def test_counting_check_refuses_counts_outside_its_exact_range():
    counts = torch.full((1, 1, 1, 64), 128.0, dtype=torch.float64)
    with pytest.raises(AssertionError, match="exact only below"):
        A.check_counts((counts / 8192).to(torch.bfloat16), counts, 8192)


def _inputs(N, Nk, dtype, seed, amp=0.0):
    g = torch.Generator().manual_seed(seed)
    q = (amp * torch.randn(B, H, N, 64, generator=g)).to(dtype)
    k = torch.randn(B, H, Nk, 64, generator=g).to(dtype)
    sizes = torch.randint(1, 4, (B, Nk), generator=g).float()
    sizes[:, 0] = 3.0  # (the skip form's key-0 mistake below gives key 0 this size: make it differ from weight 1)
    return q, k, sizes


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("amp", [0.0, 1.0])
@pytest.mark.parametrize("N,Nk", [(33, 200), (1, 1568), (129, 1568)])
def test_weighted_check_rejects_misplaced_bias(N, Nk, amp, dtype):
    """The size bias of key j applied to key j + 1 or j - 1, against the weight bound."""
    q, k, sizes = _inputs(N, Nk, dtype, N + Nk, amp)
    lb = sizes.log()
    ref = A.weighted_reference(q, k, lb, False, 0.125, "mod")
    assert A.check_weighted(ref.out.to(dtype), ref, "correct") <= 1.0
    if amp == 0.0:
        assert A.sensitivity(ref, dtype) > 1.0
    for shift in (1, -1):
        wrong = A.weighted_reference(q, k, torch.roll(lb, shift, dims=1), False, 0.125, "mod")
        with pytest.raises(AssertionError):
            A.check_weighted(wrong.out.to(dtype), ref, f"bias shifted by {shift}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("amp", [0.0, 1.0])
@pytest.mark.parametrize("N", [65, 225, 1568])
def test_weighted_check_rejects_skip_form_mistakes(N, amp, dtype):
    """TimeSformer's form: the class query biased like the others, key 0 given key 1's size (an unshifted index),
    the per-key form instead, the bias dropped altogether."""
    q, k, sizes = _inputs(N, N, dtype, 3 * N, amp)
    lb = sizes[:, 1:].log()
    ref = A.weighted_reference(q, k, lb, True, 0.125, "mod")
    assert A.check_weighted(ref.out.to(dtype), ref, "correct") <= 1.0
    if amp == 0.0:
        assert A.sensitivity(ref, dtype) > 1.0
    right = A.log2_bias(lb, True, N, N)
    query0 = right.clone()
    query0[:, :, 0, 1:] = lb[:, None, :] * A.LOG2E
    key0 = right.clone()
    key0[:, :, 1:, 0] = lb[:, None, :1] * A.LOG2E
    per_key = A.log2_bias(sizes.log(), False, N, N)
    for name, beta in (("query 0 biased", query0), ("key 0 biased", key0), ("per-key form", per_key),
                       ("no bias", torch.zeros_like(right))):
        wrong = A.weighted_reference(q, k, None, False, 0.125, "mod", beta=beta)
        with pytest.raises(AssertionError):
            A.check_weighted(wrong.out.to(dtype), ref, name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Nk", [449, 1568])
def test_weighted_check_rejects_dropped_doubled_keys_and_other_slices(Nk, dtype):
    """q = 0 with sizes: one key dropped or counted twice (every key of the first tile and of the last), another
    batch's or head's values -- the mistakes `sensitivity` says cannot hide in the bound."""
    N = 4
    q, k, sizes = _inputs(N, Nk, dtype, Nk)
    lb = sizes.log()
    ref = A.weighted_reference(q, k, lb, False, 0.125, "mod")
    assert A.sensitivity(ref, dtype) > 1.0
    right = A.log2_bias(lb, False, N, Nk)
    for j in sorted(set(range(64)) | set(range((Nk - 1) // 64 * 64, Nk))):
        for name, change in (("dropped", -1e9), ("counted twice", 1.0)):  # log2 units: weight 0 / twice the weight
            beta = right.clone()
            beta[..., j] += change
            wrong = A.weighted_reference(q, k, None, False, 0.125, "mod", beta=beta)
            with pytest.raises(AssertionError):
                A.check_weighted(wrong.out.to(dtype), ref, f"key {j} {name}")
    for dim in (0, 2):  # out [B, N, H, 64]: batch, head
        with pytest.raises(AssertionError):
            A.check_weighted(torch.roll(ref.out, 1, dims=dim).to(dtype), ref, f"dim {dim}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_segment_checks_reject_keys_of_the_wrong_segment(dtype):
    """Segments: every segment one key late (a segment offset off by one key) for the counts; one softmax over all
    segments instead of one per segment for the weights."""
    P, F, N = 65, 3, 6
    Nk = P * F
    q, k, sizes = _inputs(N, Nk, dtype, 9)
    counts = A.expected_counts(B, H, Nk, "mod", nseg=F)

    def seg_counts(chan):
        c = torch.zeros(B, H, F, 64, dtype=torch.float64).scatter_add_(-1, chan, torch.ones(chan.shape, dtype=torch.float64))
        return (c / P).permute(0, 2, 1, 3).unsqueeze(1).expand(B, N, F, H, 64).to(dtype)

    A.check_counts(seg_counts(A.channel_of(B, H, Nk, "mod").view(B, H, F, P)), counts, P, "correct")
    late = A.channel_of(B, H, Nk + 1, "mod")[..., 1:].reshape(B, H, F, P)
    with pytest.raises(AssertionError):
        A.check_counts(seg_counts(late), counts, P, "one key late")
    lb = sizes.log()
    ref = A.weighted_reference(q, k, lb, False, 0.125, "mod", nseg=F)
    assert A.check_weighted(ref.out.to(dtype), ref, "correct") <= 1.0
    assert A.sensitivity(ref, dtype) > 1.0
    one = A.weighted_reference(q, k, lb, False, 0.125, "mod", nseg=1)
    with pytest.raises(AssertionError):
        A.check_weighted(one.out.unsqueeze(2).expand(B, N, F, H, 64).to(dtype), ref, "one softmax")


def test_weighted_bound_floor_and_terms():
    """2u + eta relative, the fp16 floor nk * 2^-24, bf16's 1e-6."""
    r = torch.tensor([0.0, 0.5], dtype=torch.float64)
    assert torch.equal(A.weighted_bound(r, torch.bfloat16, 100, 0.0), torch.tensor([1e-6, 2 ** -8 + 1e-6], dtype=torch.float64))
    assert torch.equal(A.weighted_bound(r, torch.float16, 2 ** 10, 2 ** -16),
                       torch.tensor([2 ** -14, (2 ** -10 + 2 ** -16) * 0.5 + 2 ** -14], dtype=torch.float64))


def test_expected_form_mirrors_the_dispatcher():
    """Points of attn_form's rule (csrc/tome_kernels.hip), the dispatch of prop_attention_impl."""
    f = A.expected_form
    assert f(197, 197, 64 * 12) == "resident" and f(1568, 196, 2 * 12 * 8) == "resident"
    assert f(1, 225, 24) == "wave4" and f(1, 1569, 24) == "wave4"       # Motionformer's class query, > 224 keys
    assert f(1568, 1568, 6) == "stream" and f(1568, 1568, 8 * 12) == "stream"  # N > 128: streamed either way
    assert f(128, 1568, 6) == "wave4" and f(129, 1568, 6) == "stream"
    assert f(1568, 64, 6, {"TOME_ATTN_RESIDENT": "0"}) == "wave4"       # one tile: never streamed
    assert f(1568, 64, 1024, {"TOME_ATTN_RESIDENT": "0"}) == "wave8"
    env8 = A.FORMS["stream"]
    assert f(33, 65, 6, env8) == "stream" and f(33, 64, 6, env8) == "wave8"
    assert f(33, 700, 6, A.FORMS["wave8"]) == "wave8" and f(33, 700, 6, A.FORMS["wave4"]) == "wave4"
    assert f(100, 100, 6, off32=False) == "wave4" and f(700, 700, 6, sn_ok=False) == "wave4"
    assert f(10, 10, 6, {"TOME_ATTN_WAVES": "6"}) == "resident"
    assert f(300, 300, 6, {"TOME_ATTN_WAVES": "6"}) == "stream"         # an invalid value: the default rule


def test_gpu_grids_reach_every_launch_form():
    """The parametrisation of the GPU tests covers all four kernels (what their ids name is what the dispatcher
    picks: expected_form)."""
    import test_attention_accounting_gpu as G
    for grid in (G.COUNT_GRID, G.WEIGHT_GRID):
        assert {p.values[2] for p in grid} == set(A.FORMS)
    assert {(N, Nk) for N, Nk, _ in (p.values for p in G.COUNT_GRID)} == set(G.COUNT_SHAPES)
