"""Every key accounted for in the attention kernels (tome_prop_attention / tome_prop_attention_segments and their
kernels k_resident_attention, k_prop_attention with 4 and 8 waves, k_prop_attention_stream as one workgroup per CU
and as two of 128 registers), each of the five launch forms forced through the dispatcher's measurement switches
(read per call) and checked against an exact expectation (tests/attn_oracle.py):

  * counting: q = 0 and one-hot values -- the output is count / Nk per channel, the counts are recovered exactly;
  * weighted: integer sizes or random q, the fp64 weight mass of every channel within the kernels' rounding bound;

at N == Nk around the tile edges, one query against many keys (Motionformer's class token, written through `out=`
into row 0 of the joined buffer), many queries against few keys, strided `out` and `log_bias` views, the segmented
form, a qkv buffer of more than 2^31 elements, persistent workgroups that walk from one item to the next
(TOME_ATTN_GRID=8 over 24 slices), and logits that climb from tile to tile until the reference point has to move."""
import pytest
import torch

import attn_oracle as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, H = 2, 3
DTYPES = (torch.bfloat16, torch.float16)
SWITCHES = ("TOME_ATTN_RESIDENT", "TOME_ATTN_WAVES", "TOME_ATTN_STREAM", "TOME_ATTN_GRID")

SQUARE = [1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 160, 161, 224, 225, 449, 1568, 3137]
WIDE = [(1, 2), (1, 65), (1, 217), (1, 225), (1, 801), (1, 1569), (33, 700)]
TALL = [(700, 1), (700, 32), (700, 65), (700, 200)]
COUNT_SHAPES = [(n, n) for n in SQUARE] + WIDE + TALL
WEIGHT_SHAPES = [(n, n) for n in (1, 33, 65, 97, 129, 161, 224, 225, 449, 1568)] + \
                [(1, 217), (1, 1569), (33, 700), (700, 65), (700, 200)]
OUT_SHAPES = [(1, 1), (33, 33), (65, 65), (97, 97), (225, 225), (449, 449), (1, 801), (700, 200)]
MOTIONFORMER = [(196, 8), (100, 8), (27, 8), (20, 8)]  # (P, F): the class query against 1 + P*F keys
SEGMENTS = [(196, 8), (350, 2), (65, 3), (33, 3)]     # (P, F): N = P*F queries against F segments of P keys


def _grid(shapes, items):
    """(N, Nk, form) for every form the dispatcher reaches on that shape (the others would run another form)."""
    return [pytest.param(N, Nk, form, id=f"N{N}-Nk{Nk}-{form}") for N, Nk in shapes for form, env in A.FORMS.items()
            if A.expected_form(N, Nk, items, env) == form]


COUNT_GRID = _grid(COUNT_SHAPES, B * H)
WEIGHT_GRID = _grid(WEIGHT_SHAPES, B * H)
OUT_GRID = _grid(OUT_SHAPES, B * H)
MOTIONFORMER_GRID = [pytest.param(P, F, form, id=f"P{P}F{F}-{form}") for P, F in MOTIONFORMER
                     for form, env in A.FORMS.items() if A.expected_form(1, 1 + P * F, 2 * 12, env) == form]
SEGMENT_GRID = [pytest.param(P, F, form, id=f"P{P}F{F}-{form}") for P, F in SEGMENTS
                for form, env in A.FORMS.items() if A.expected_form(P * F, P, B * H * F, env) == form]
# (the grids must reach all five launch forms: checked here, at collection, on any machine)
for _g in (COUNT_GRID, WEIGHT_GRID, OUT_GRID, MOTIONFORMER_GRID, SEGMENT_GRID):
    assert {p.values[2] for p in _g} == set(A.FORMS), "the shape grid no longer reaches every launch form"

# Workgroups that walk items: 2 x 12 slices over TOME_ATTN_GRID=8 persistent workgroups.  att_item gives workgroup w
# the query blocks of slice w, then 8 + w, then 16 + w: every switch changes the head, some the batch.  (N, Nk):
WALK_B, WALK_H, WALK_WGS = 2, 12, 8
WALK_SHAPES = [(129, 129),   # three tiles: the ring slot parity flips at every item
               (288, 288),   # a second query block of 32 rows: one computing wave, seven helpers
               (300, 96),    # the last tile holds 32 keys (last_half)
               (64, 577),    # ten tiles, three bias groups: the third takes buffer 0 again inside an item
               (1, 161)]     # one row, seven helper waves
WALK_FORMS = ("stream", "pair")  # the persistent kernels: nothing else walks
WALK_GRID = [pytest.param(N, Nk, form, id=f"N{N}-Nk{Nk}-{form}") for N, Nk in WALK_SHAPES for form in WALK_FORMS]
for _p in WALK_GRID:
    assert A.expected_form(_p.values[0], _p.values[1], WALK_B * WALK_H, A.FORMS[_p.values[2]]) == _p.values[2]
    assert _p.values[1] % 64 != 0  # ("mod": a rotation by a whole tile's worth of keys would not show in the counts)
    # more items than workgroups: every workgroup walks
    assert (WALK_B * WALK_H + 7) // 8 * 8 * ((_p.values[0] + 255) // 256) >= 3 * WALK_WGS

# The reference point moves: (dtype, step, Nk) of attn_oracle.staircase_inputs, N = 64, and the forms that run them --
# every form where the keys allow it (the resident kernel holds 224), the persistent ones also walking items.
STAIR_N = 64
STAIR_INPUTS = [(torch.bfloat16, 5, 865), (torch.bfloat16, 5, 896), (torch.float16, 5, 448), (torch.float16, 6, 224)]


def _stair_forms(dtype, Nk):
    forms = [(f, None) for f in ("wave4", "wave8", "stream", "pair")] + [(f, WALK_WGS) for f in WALK_FORMS]
    return ([("resident", None)] if Nk <= A.RES_ROWS else []) + forms


_NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}
STAIR_GRID = [pytest.param(dtype, step, Nk, form, wgs,
                           id=f"{_NAME[dtype]}-step{step}-Nk{Nk}-{form}" + ("-walk" if wgs else ""))
              for dtype, step, Nk in STAIR_INPUTS for form, wgs in _stair_forms(dtype, Nk)]
for _p in STAIR_GRID:
    _bh = WALK_B * WALK_H if _p.values[4] else B * H
    assert A.expected_form(STAIR_N, _p.values[2], _bh, A.FORMS[_p.values[3]]) == _p.values[3]
# (every form in both formats but bf16 on the resident kernel: see test_reference_point_moves_every_form)
assert {(p.values[0], p.values[3]) for p in STAIR_GRID} == \
    {(d, f) for d in DTYPES for f in A.FORMS} - {(torch.bfloat16, "resident")}


def staircase_case(dtype, step, Nk, walk):
    """The inputs of one staircase case, drawn on the CPU (so that tests/test_attn_oracle_cpu.py holds the very same
    tensors to its conditions): B, H, q, k, gain, sizes."""
    Bs, Hs = (WALK_B, WALK_H) if walk else (B, H)
    g = torch.Generator().manual_seed(1000 * step + Nk + (7 if walk else 0))
    q, k, gain = A.staircase_inputs(Bs, Hs, STAIR_N, Nk, dtype, step, g)
    sizes = torch.randint(1, 4, (Bs, Nk), generator=g).float()
    return Bs, Hs, q, k, gain, sizes


def _force(monkeypatch, form, wgs=None):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in A.FORMS[form].items():
        monkeypatch.setenv(name, value)
    if wgs:
        monkeypatch.setenv("TOME_ATTN_GRID", str(wgs))


def _abi():
    from tome import _abi
    return _abi


@pytest.mark.parametrize("N,Nk,form", COUNT_GRID)
def test_key_counts_every_form(N, Nk, form, monkeypatch):
    """q = 0: every logit 0 (or the same constant bias), every weight exactly 1, so a one-hot v makes the output the
    number of keys of each channel over Nk -- recovered exactly, both encodings (a key per channel in turn / a
    channel per 64-key tile), both 16-bit formats, without and with a constant log_bias.  Nk = 1 returns v itself."""
    _abi_ = _abi()
    _force(monkeypatch, form)
    g = torch.Generator(device=DEV).manual_seed(7919 * N + Nk)
    for dtype in DTYPES:
        q = torch.zeros(B, H, N, 64, dtype=dtype, device=DEV)
        k = torch.randn(B, H, Nk, 64, device=DEV, generator=g).to(dtype)
        for enc in ("mod", "tile"):
            v = A.onehot_values(B, H, Nk, enc, dtype, DEV)
            counts = A.expected_counts(B, H, Nk, enc, device=DEV)
            for lb in (None, torch.full((B, Nk), 0.7, device=DEV)):
                out = _abi_.prop_attention(q, k, v, None, 0.125, log_bias=lb).view(B, N, H, 64)
                A.check_counts(out, counts, Nk, f"{form} {dtype} {enc} bias={lb is not None}")
                if Nk == 1:
                    assert torch.equal(out, v[:, :, :1].permute(0, 2, 1, 3).expand(B, N, H, 64))


@pytest.mark.parametrize("P,F,form", MOTIONFORMER_GRID)
def test_motionformer_class_query_into_joined_row(P, F, form, monkeypatch):
    """The call tome/patch/motionformer.py makes for the class token: heads[0][:, :, :1] against heads[1] and
    heads[2], all views of one qkv buffer [B, 1+P*F, 3, H, 64], written through out= into row 0 of the joined
    [B, 1+P*F, H*64] buffer (its batch stride far wider than one row).  Counts exact; every other row untouched."""
    _abi_ = _abi()
    _force(monkeypatch, form)
    Bm, Hm, N = 2, 12, 1 + P * F
    g = torch.Generator(device=DEV).manual_seed(P * 100 + F)
    for dtype in DTYPES:
        qkv = torch.zeros(Bm, N, 3, Hm, 64, dtype=dtype, device=DEV)
        heads = qkv.permute(2, 0, 3, 1, 4)
        heads[1].copy_(torch.randn(Bm, Hm, N, 64, device=DEV, generator=g))
        for enc in ("mod", "tile"):
            heads[2].copy_(A.onehot_values(Bm, Hm, N, enc, dtype, DEV))
            joined = torch.full((Bm, N, Hm * 64), float("nan"), dtype=dtype, device=DEV)
            out = joined[:, :1].unflatten(2, (Hm, 64))
            res = _abi_.prop_attention(heads[0][:, :, :1], heads[1], heads[2], None, 0.125, out=out)
            assert res.data_ptr() == joined.data_ptr()
            A.check_counts(joined[:, :1].view(Bm, 1, Hm, 64), A.expected_counts(Bm, Hm, N, enc, device=DEV), N,
                           f"{form} {dtype} {enc}")
            assert bool(torch.isnan(joined[:, 1:]).all()), "rows behind the class row were written"


@pytest.mark.parametrize("N,Nk,form", OUT_GRID)
def test_out_view_and_strided_log_bias(N, Nk, form, monkeypatch):
    """out= a [B, N, H, 64] view of a wider NaN-filled buffer (a row before and after, 8 spare channels per head) and
    log_bias a [B, nb] view of a [B, nb + 16] tensor (row stride != nb): the same bits as the plain call of the same
    form, nothing outside the view written.  No bias, the per-key bias and the TimeSformer form."""
    _abi_ = _abi()
    _force(monkeypatch, form)
    g = torch.Generator(device=DEV).manual_seed(31 * N + Nk)
    for dtype in DTYPES:
        q = torch.randn(B, H, N, 64, device=DEV, generator=g).to(dtype)
        k, v = (torch.randn(B, H, Nk, 64, device=DEV, generator=g).to(dtype) for _ in range(2))
        for mode in ("none", "bias", "skip"):
            skip = mode == "skip"
            if skip and (N != Nk or Nk < 2):
                continue
            nb = Nk - (1 if skip else 0)
            wide = torch.randint(1, 30, (B, nb + 16), device=DEV, generator=g).float().log()
            lb = None if mode == "none" else wide[:, :nb]
            plain = _abi_.prop_attention(q, k, v, None, 0.125, bias_skip=skip,
                                         log_bias=None if lb is None else lb.contiguous())
            buf = torch.full((B, N + 2, H, 72), float("nan"), dtype=dtype, device=DEV)
            view = buf[:, 1:N + 1, :, :64]
            _abi_.prop_attention(q, k, v, None, 0.125, bias_skip=skip, log_bias=lb, out=view)
            assert torch.equal(view, plain.view(B, N, H, 64)), (mode, dtype)
            outside = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
            outside[:, 1:N + 1, :, :64] = False
            assert bool(torch.isnan(buf[outside]).all()), (mode, dtype, "written outside the out view")


@pytest.mark.parametrize("N,Nk,form", WEIGHT_GRID)
def test_weighted_mass_every_form(N, Nk, form, monkeypatch):
    """Weighted accounting against the fp64 reference: every channel's weight mass within weighted_bound.
    (a) q = 0, integer sizes 1..3: the weights are the sizes -- per-key bias and TimeSformer's skip form -- and the
    bound is tight enough that dropping or doubling any single key would break it (sensitivity > 1);
    (b) random q, N(0, 1) and x3 (peaky rows), no bias, per-key bias and the skip form."""
    _abi_ = _abi()
    _force(monkeypatch, form)
    g = torch.Generator(device=DEV).manual_seed(104729 * N + Nk)
    modes = ["none", "bias"] + (["skip"] if N == Nk and Nk > 1 else [])
    worst = 0.0
    for dtype in DTYPES:
        k = torch.randn(B, H, Nk, 64, device=DEV, generator=g).to(dtype)
        v = A.onehot_values(B, H, Nk, "mod", dtype, DEV)
        sizes = torch.randint(1, 4, (B, Nk), device=DEV, generator=g).float()
        cases = [(0.0, m) for m in modes if m != "none"] + [(amp, m) for amp in (1.0, 3.0) for m in modes]
        for amp, mode in cases:
            q = (amp * torch.randn(B, H, N, 64, device=DEV, generator=g)).to(dtype)
            skip = mode == "skip"
            lb = None if mode == "none" else (sizes[:, 1:] if skip else sizes).log().contiguous()
            out = _abi_.prop_attention(q, k, v, None, 0.125, bias_skip=skip, log_bias=lb).view(B, N, H, 64)
            ref = A.weighted_reference(q, k, lb, skip, 0.125, "mod")
            worst = max(worst, A.check_weighted(out, ref, f"{form} {dtype} q*{amp} {mode}"))
            if amp == 0.0 and Nk >= 2:
                assert A.sensitivity(ref, dtype) > 1.0, (dtype, mode)
    print(f"largest error / bound: {worst:.3f}")


@pytest.mark.parametrize("P,F,form", SEGMENT_GRID)
def test_segments_counts_and_mass(P, F, form, monkeypatch):
    """prop_attention_segments as Motionformer calls it (q / k / v views of one qkv buffer behind a class token):
    per segment, the key counts of q = 0 exact and the weight mass of sizes / random q within the bound."""
    _abi_ = _abi()
    _force(monkeypatch, form)
    N = P * F
    g = torch.Generator(device=DEV).manual_seed(P * 17 + F)
    for dtype in DTYPES:
        qkv = torch.randn(B, 1 + N, 3, H, 64, device=DEV, generator=g).to(dtype)
        heads = qkv.permute(2, 0, 3, 1, 4)
        q, k, v = (t[:, :, 1:] for t in heads)
        sizes = torch.randint(1, 4, (B, N), device=DEV, generator=g).float()
        for enc in ("mod", "tile"):
            v.copy_(A.onehot_values(B, H, N, enc, dtype, DEV))
            counts = A.expected_counts(B, H, N, enc, nseg=F, device=DEV)
            q0 = torch.zeros_like(q)
            for lb in (None, torch.full((B, N), 0.7, device=DEV)):
                y = _abi_.prop_attention_segments(q0, k, v, F, 0.125, log_bias=lb)
                A.check_counts(y.view(B, N, F, H, 64), counts, P, f"{form} {dtype} {enc} bias={lb is not None}")
        v.copy_(A.onehot_values(B, H, N, "mod", dtype, DEV))
        for amp, with_bias in ((0.0, True), (1.0, False), (1.0, True), (3.0, True)):
            qa = (amp * q.float()).to(dtype)
            lb = sizes.log() if with_bias else None
            y = _abi_.prop_attention_segments(qa, k, v, F, 0.125, log_bias=lb)
            ref = A.weighted_reference(qa, k, lb, False, 0.125, "mod", nseg=F)
            A.check_weighted(y.view(B, N, F, H, 64), ref, f"{form} {dtype} q*{amp} bias={with_bias}")
            if amp == 0.0:
                assert A.sensitivity(ref, dtype) > 1.0, dtype


@pytest.mark.parametrize("waves", [None, "4"])
def test_counts_beyond_2_31_elements(waves, monkeypatch):
    """A qkv buffer [640, 1568, 3, 12, 64] bf16 (2.3e9 elements: batch offsets past 2^31) with q = 0 and rotated
    one-hot values: every (batch, token, head) row of the NaN-prefilled out holds its slice's key counts -- a read or
    write at a wrapped 32-bit offset lands in another slice and shows.  Default dispatch (the persistent kernel as two
    workgroups per CU at this size: 53760 items) and TOME_ATTN_WAVES=4."""
    _abi_ = _abi()
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if waves:
        monkeypatch.setenv("TOME_ATTN_WAVES", waves)
    Bb, N, Hb = 640, 1568, 12
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert A.expected_form(N, N, Bb * Hb, {} if waves is None else {"TOME_ATTN_WAVES": waves}, cus=cus) == \
        ("pair" if waves is None else "wave4")
    qkv = torch.zeros(Bb, N, 3, Hb, 64, dtype=torch.bfloat16, device=DEV)
    assert qkv.numel() > 2 ** 31
    q, k, v = qkv.permute(2, 0, 3, 1, 4)
    k.normal_(generator=torch.Generator(device=DEV).manual_seed(11))
    v.scatter_(-1, A.channel_of(Bb, Hb, N, "mod", DEV).unsqueeze(-1), 1.0)
    out = torch.full((Bb, N, Hb, 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    _abi_.prop_attention(q, k, v, None, 0.125, out=out)
    counts = A.expected_counts(Bb, Hb, N, "mod", device=DEV)
    for lo in range(0, Bb, 64):
        A.check_counts(out[lo:lo + 64], counts[lo:lo + 64], N, f"batches {lo}..{lo + 63}")
    del qkv, out
    torch.cuda.empty_cache()


def _into_nan(call, Bs, N, Hs, dtype):
    """call(out) into a NaN-filled [Bs, N, Hs, 64]: a row or head left unwritten shows as non-finite."""
    out = torch.full((Bs, N, Hs, 64), float("nan"), dtype=dtype, device=DEV)
    res = call(out)
    assert res.data_ptr() == out.data_ptr()
    return out


@pytest.mark.parametrize("N,Nk,form", WALK_GRID)
def test_walking_workgroups_account_for_every_key(N, Nk, form, monkeypatch):
    """Eight persistent workgroups over 2 x 12 slices (TOME_ATTN_GRID=8): each walks three slices' query blocks, and
    the step between two items -- the stream already two tiles into the next item's K / V and bias row, the ring slot
    parity carried over, q_request / item_take / item_reset -- is held to the exact checks.  The one-hot channels
    rotate with batch and head and Nk is no multiple of 64, so a K, V, bias row, Q or output address left over from
    the previous item lands in the wrong channels or weights.  Per shape, both formats, into a NaN-filled out:
    (a) q = 0: key counts exact, both encodings, without and with a constant bias;
    (b) weight mass within weighted_bound: integer sizes at q = 0 (sensitivity > 1), random q x1 and x3; no bias,
        per-key bias and (N == Nk) the TimeSformer skip form."""
    _abi_ = _abi()
    _force(monkeypatch, form, WALK_WGS)
    Bw, Hw = WALK_B, WALK_H
    g = torch.Generator(device=DEV).manual_seed(15485863 + 7919 * N + Nk)
    modes = ["none", "bias"] + (["skip"] if N == Nk else [])
    worst = {}
    for dtype in DTYPES:
        k = torch.randn(Bw, Hw, Nk, 64, device=DEV, generator=g).to(dtype)
        q0 = torch.zeros(Bw, Hw, N, 64, dtype=dtype, device=DEV)
        for enc in ("mod", "tile"):
            v = A.onehot_values(Bw, Hw, Nk, enc, dtype, DEV)
            counts = A.expected_counts(Bw, Hw, Nk, enc, device=DEV)
            for lb in (None, torch.full((Bw, Nk), 0.7, device=DEV)):
                out = _into_nan(lambda o: _abi_.prop_attention(q0, k, v, None, 0.125, log_bias=lb, out=o),
                                Bw, N, Hw, dtype)
                A.check_counts(out, counts, Nk, f"{form} {dtype} {enc} bias={lb is not None}")
        v = A.onehot_values(Bw, Hw, Nk, "mod", dtype, DEV)
        sizes = torch.randint(1, 4, (Bw, Nk), device=DEV, generator=g).float()
        cases = [(0.0, m) for m in modes if m != "none"] + [(amp, m) for amp in (1.0, 3.0) for m in modes]
        for amp, mode in cases:
            q = (amp * torch.randn(Bw, Hw, N, 64, device=DEV, generator=g)).to(dtype)
            skip = mode == "skip"
            lb = None if mode == "none" else (sizes[:, 1:] if skip else sizes).log().contiguous()
            out = _into_nan(lambda o: _abi_.prop_attention(q, k, v, None, 0.125, bias_skip=skip, log_bias=lb, out=o),
                            Bw, N, Hw, dtype)
            ref = A.weighted_reference(q, k, lb, skip, 0.125, "mod")
            ratio = A.check_weighted(out, ref, f"{form} {dtype} q*{amp} {mode}")
            worst[dtype] = max(worst.get(dtype, 0.0), ratio)
            if amp == 0.0:
                assert A.sensitivity(ref, dtype) > 1.0, (dtype, mode)
    print("largest error / bound: " + ", ".join(f"{_NAME[d]} {w:.3f}" for d, w in worst.items()))


@pytest.mark.parametrize("dtype,step,Nk,form,wgs", STAIR_GRID)
def test_reference_point_moves_every_form(dtype, step, Nk, form, wgs, monkeypatch):
    """Logits that climb by `step` log2 units per 64-key tile (attn_oracle.staircase_inputs): against tile 0's
    reference point the last tile's weights are beyond the guard's limit (tests/test_attn_oracle_cpu.py asserts it
    for these very inputs), so the reference point moves at least once -- and in bf16 the values grow backwards by
    the same factor, so that what was summed BEFORE the move still makes up most of every channel: a reference point
    that differs between the two sides of a move (a factor 2^0.25 at |m| = 64 if the matrix pipe carried only the
    `hi` of hi + lo), or an O or l not rescaled, is many times the bound, where the rerun tests of test_hip_parity.py
    (a jump of 70 log2 units: nothing before it has any mass) cannot see it.  fp16 runs with unit values: its range
    cannot hold the gains, and under the "tile" encoding (a channel per tile) its 2u and floor still show the two
    tiles before the last, 7 times the bound for that factor.  No bias and integer sizes, both
    encodings, every launch form, the persistent ones also walking items (2 x 12 slices over 8 workgroups: an item
    that starts after the previous one's moves).  Left out: bf16 on the resident kernel -- its 224 keys are four
    tiles, and 60 log2 units in three steps leave nothing of the first three visible."""
    _abi_ = _abi()
    _force(monkeypatch, form, wgs)
    Bs, Hs, q, k, gain, sizes = staircase_case(dtype, step, Nk, bool(wgs))
    q, k, sizes = q.to(DEV), k.to(DEV), sizes.to(DEV)
    worst = 0.0
    for enc in ("mod", "tile"):
        v = A.onehot_values(Bs, Hs, Nk, enc, dtype, DEV, gain=gain)
        for lb in (None, sizes.log()):
            out = _into_nan(lambda o: _abi_.prop_attention(q, k, v, None, 0.125, log_bias=lb, out=o),
                            Bs, STAIR_N, Hs, dtype)
            ref = A.weighted_reference(q, k, lb, False, 0.125, enc, gain=gain)
            assert A.rise(ref) > A.ATT_LIMIT_LOG2[dtype]
            worst = max(worst, A.check_weighted(out, ref, f"{form} {dtype} step {step} {enc} bias={lb is not None}"))
    print(f"largest error / bound: {worst:.3f}")
