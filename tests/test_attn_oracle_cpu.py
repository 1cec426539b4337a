"""The attention checks of tests/attn_oracle.py reject wrong answers (CPU, no GPU): outputs of deliberately wrong
attention -- a key dropped, counted twice, a tile dropped, the size bias on the neighbouring key, the TimeSformer
form's class query or class key biased, another batch's or head's values -- computed in fp64 and rounded to the
16-bit format as a kernel would, must all fail the checks the GPU tests apply (test_attention_accounting_gpu.py),
and the correct output must pass them.  So those tests catch these bug classes at the shapes they run.  Also here:
the mirror of the dispatcher's rule (five launch forms), the grids of the GPU tests against it, and the conditions
that make the staircase inputs (a reference point that has to move) a check and not a formality."""
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
    assert f(1568, 1568, 6) == "stream" and f(1568, 1568, 8 * 12, cus=1024) == "stream"  # N > 128: streamed either way
    assert f(1568, 1568, 8 * 12) == "pair"                              # 96 x 7 = 672 items > 256 CUs: two per CU
    assert f(128, 1568, 6) == "wave4" and f(129, 1568, 6) == "stream"
    # the persistent kernel's two forms: by the switch ...
    one, two = {"TOME_ATTN_STREAM": "1"}, {"TOME_ATTN_STREAM": "2"}
    assert f(1568, 1568, 8 * 12, one) == "stream" and f(1568, 1568, 6, two) == "pair"
    assert f(1568, 64, 6, dict(two, TOME_ATTN_RESIDENT="0")) == "wave4"  # (one tile: the switch picks no kernel)
    assert f(128, 1568, 6, two) == "wave4" and f(128, 1568, 6, dict(two, TOME_ATTN_WAVES="8")) == "pair"
    assert f(33, 700, 6, A.FORMS["pair"]) == "pair" and f(33, 700, 6, A.FORMS["stream"]) == "stream"
    # ... or by the launch size: items = slices rounded up to 8, times the 256-row query blocks, against the CUs
    # rounded down to 8
    assert f(300, 300, 128) == "stream" and f(300, 300, 129) == "pair"   # 2 x 128 = 256 items; 2 x 136
    assert f(256, 300, 256) == "stream" and f(257, 300, 256) == "pair"   # one query block of 256 rows; two
    assert f(200, 300, 249) == "stream" and f(200, 300, 250, cus=255) == "pair"   # 256 items; 255 CUs count as 248
    assert f(200, 300, 248, cus=255) == "stream" and f(200, 300, 249, cus=255) == "pair"
    assert f(200, 300, 256, cus=263) == "stream" and f(200, 300, 256, cus=264) == "stream"
    assert f(200, 300, 257, cus=263) == "pair" and f(200, 300, 257, cus=264) == "stream"   # 264 items
    off = {"TOME_ATTN_STREAM": "0"}
    assert f(300, 300, 6, off) == "wave4" and f(300, 300, 1024, off) == "wave8"
    assert f(1568, 64, 6, {"TOME_ATTN_RESIDENT": "0"}) == "wave4"       # one tile: never streamed
    assert f(1568, 64, 1024, {"TOME_ATTN_RESIDENT": "0"}) == "wave8"
    env8 = A.FORMS["stream"]
    assert f(33, 65, 6, env8) == "stream" and f(33, 64, 6, env8) == "wave8"
    assert f(33, 700, 6, A.FORMS["wave8"]) == "wave8" and f(33, 700, 6, A.FORMS["wave4"]) == "wave4"
    assert f(100, 100, 6, off32=False) == "wave4" and f(700, 700, 6, sn_ok=False) == "wave4"
    assert f(10, 10, 6, {"TOME_ATTN_WAVES": "6"}) == "resident"
    assert f(300, 300, 6, {"TOME_ATTN_WAVES": "6"}) == "stream"         # an invalid value: the default rule


def test_gpu_grids_reach_every_launch_form():
    """The parametrisation of the GPU tests covers all five launch forms (what their ids name is what the dispatcher
    picks: expected_form) in every grid; the walk grid the two persistent kernels, the only ones that walk."""
    import test_attention_accounting_gpu as G
    import test_hip_parity
    assert set(A.FORMS) == set(A.FORM_KERNEL) == {"resident", "wave4", "wave8", "stream", "pair"}
    for grid in (G.COUNT_GRID, G.WEIGHT_GRID, G.OUT_GRID, G.MOTIONFORMER_GRID, G.SEGMENT_GRID):
        assert {p.values[2] for p in grid} == set(A.FORMS)
    assert {p.values[1] for p in test_hip_parity.RERUN_GRID} == set(A.FORMS)
    assert {p.values[3] for p in G.STAIR_GRID} == set(A.FORMS)
    assert {p.values[2] for p in G.WALK_GRID} == {"stream", "pair"}
    assert {(N, Nk) for N, Nk, _ in (p.values for p in G.COUNT_GRID)} == set(G.COUNT_SHAPES)
    assert {(N, Nk) for N, Nk, _ in (p.values for p in G.WALK_GRID)} == set(G.WALK_SHAPES)
    # every form's switches pin it: no form is left to the size of the launch
    for form, env in A.FORMS.items():
        if form != "resident":
            for items in (6, 24, 4096):
                assert A.expected_form(300, 300, items, env) == form, (form, items)
    # wherever the one-workgroup-per-CU form is reachable, so is the pair form
    for grid in (G.COUNT_GRID, G.WEIGHT_GRID, G.OUT_GRID, G.MOTIONFORMER_GRID, G.SEGMENT_GRID):
        by_form = {f: {p.values[:2] for p in grid if p.values[2] == f} for f in ("stream", "pair")}
        assert by_form["stream"] == by_form["pair"] and by_form["pair"]


def test_gain_scales_the_values_not_the_weights():
    """gain = ones is the reference without it, bit for bit; a two-key case by hand."""
    q, k, sizes = _inputs(5, 200, torch.bfloat16, 77, 1.0)
    lb = sizes.log()
    plain = A.weighted_reference(q, k, lb, False, 0.125, "mod")
    ones = A.weighted_reference(q, k, lb, False, 0.125, "mod", gain=torch.ones(200, dtype=torch.float64))
    for a, b in zip(plain, ones):
        assert a == b if isinstance(a, int) else torch.equal(a, b)
    assert torch.equal(A.onehot_values(B, H, 200, "mod", torch.bfloat16),
                       A.onehot_values(B, H, 200, "mod", torch.bfloat16, gain=torch.ones(200, dtype=torch.float64)))
    # two keys, q = 0, sizes 1 and 3 (weights 1/3 and 1 against the row maximum), gains 8 and 2: channel of key 0
    # holds (1/3 * 8) / (4/3) = 2, that of key 1 (1 * 2) / (4/3) = 1.5 -- batch 0, head 0: channels 0 and 1
    q0 = torch.zeros(1, 1, 1, 64, dtype=torch.bfloat16)
    k2 = torch.randn(1, 1, 2, 64, generator=torch.Generator().manual_seed(1)).bfloat16()
    gain = torch.tensor([8.0, 2.0], dtype=torch.float64)
    ref = A.weighted_reference(q0, k2, torch.tensor([[1.0, 3.0]]).log(), False, 0.125, "mod", gain=gain)
    want = torch.zeros(64, dtype=torch.float64)
    want[0], want[1] = 2.0, 1.5
    assert torch.allclose(ref.out[0, 0, 0], want, rtol=1e-7, atol=0.0)   # (fp32 log of 3: not the exact 3)
    assert torch.allclose(ref.weights.flatten(), torch.tensor([1 / 3, 1.0], dtype=torch.float64), rtol=1e-7)
    v = A.onehot_values(1, 1, 2, "mod", torch.bfloat16, gain=gain)
    assert v[0, 0, 0, 0] == 8.0 and v[0, 0, 1, 1] == 2.0 and float(v.sum()) == 10.0
    with pytest.raises(AssertionError, match="not exact"):
        A.onehot_values(1, 1, 2, "mod", torch.float16, gain=torch.tensor([2.0 ** 30, 1.0], dtype=torch.float64))


def _stair_inputs():
    """(dtype, step, Nk, walk) of every input set test_reference_point_moves_every_form runs."""
    import test_attention_accounting_gpu as G
    return sorted({(p.values[0], p.values[1], p.values[2], bool(p.values[4])) for p in G.STAIR_GRID}, key=str)


@pytest.mark.parametrize("dtype,step,Nk,walk", _stair_inputs(),
                         ids=lambda v: {torch.bfloat16: "bf16", torch.float16: "fp16"}.get(v, str(v)))
def test_staircase_inputs_meet_their_conditions(dtype, step, Nk, walk):
    """The very tensors of the GPU test (drawn on the CPU there too), without a bias and with integer sizes:
    (a) rise > log2(AttLimit) (60 / 15: AttLimit in csrc/tome_attn_tile.h) -- the guard has to trip;
    (b) every tile's contribution to every channel it touches exceeds the channel's bound (tile_visibility > 1);
    (c) the reference rounded to the 16-bit format passes check_weighted;
    (d) rejected by check_weighted: every tile before tile T weighted by 2^0.25 against the rest (what a reference
        point that lost u |m| = 0.25 at |m| = 64 between the two sides of a move gives), T the last tile and the one
        before it; one whole tile left out, each tile in turn.
    bf16 (gains): all of it under the "mod" encoding, where every channel collects a key of every tile, and under
    "tile".  fp16 (unit values, so tile t weighs 2^(-step (ntiles - 1 - t)) of the last): (b) and (d) under "tile",
    a channel per tile, for the last three tiles -- what is more than two steps behind the last tile is below the
    format's floor nk 2^-24 whatever the encoding.  Under "mod" every channel is the same mix of tiles when the
    values are all 1, a factor between tiles cancels against the row total, and only (a) and (c) are asserted."""
    import test_attention_accounting_gpu as G
    _, _, q, k, gain, sizes = G.staircase_case(dtype, step, Nk, walk)
    ntiles = (Nk + 63) // 64
    bf16 = dtype == torch.bfloat16
    for lb in (None, sizes.log()):
        right = A.log2_bias(lb, False, G.STAIR_N, Nk)
        for enc in ("mod", "tile"):
            ref = A.weighted_reference(q, k, lb, False, 0.125, enc, gain=gain)
            assert A.rise(ref) > A.ATT_LIMIT_LOG2[dtype]                                          # (a)
            assert A.check_weighted(ref.out.to(dtype), ref, "correct") <= 1.0                     # (c)
            if not bf16 and enc == "mod":
                continue
            seen = range(ntiles) if bf16 else range(ntiles - 3, ntiles)
            assert A.tile_visibility(ref, gain, dtype, seen) > 1.0                                # (b)
            for T in (ntiles - 1, ntiles - 2):                                                    # (d)
                beta = right.clone()
                beta[..., :64 * T] += 0.25
                wrong = A.weighted_reference(q, k, None, False, 0.125, enc, beta=beta, gain=gain)
                with pytest.raises(AssertionError):
                    A.check_weighted(wrong.out.to(dtype), ref, f"tiles before {T} at 2^0.25")
            for t in seen:
                beta = right.clone()
                beta[..., 64 * t:64 * (t + 1)] -= 1e9
                wrong = A.weighted_reference(q, k, None, False, 0.125, enc, beta=beta, gain=gain)
                with pytest.raises(AssertionError):
                    A.check_weighted(wrong.out.to(dtype), ref, f"tile {t} left out")
