"""Every key accounted for in the attention kernels (tome_prop_attention / tome_prop_attention_segments and their
kernels k_resident_attention, k_prop_attention with 4 and 8 waves, k_prop_attention_stream), each launch form forced
through the dispatcher's measurement switches (read per call) and checked against an exact expectation
(tests/attn_oracle.py):

  * counting: q = 0 and one-hot values -- the output is count / Nk per channel, the counts are recovered exactly;
  * weighted: integer sizes or random q, the fp64 weight mass of every channel within the kernels' rounding bound;

at N == Nk around the tile edges, one query against many keys (Motionformer's class token, written through `out=`
into row 0 of the joined buffer), many queries against few keys, strided `out` and `log_bias` views, the segmented
form, and a qkv buffer of more than 2^31 elements."""
import pytest
import torch

import attn_oracle as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, H = 2, 3
DTYPES = (torch.bfloat16, torch.float16)
SWITCHES = ("TOME_ATTN_RESIDENT", "TOME_ATTN_WAVES", "TOME_ATTN_STREAM")

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
# (the grids must reach all four kernels: checked here, at collection, on any machine)
for _g in (COUNT_GRID, WEIGHT_GRID):
    assert {p.values[2] for p in _g} == set(A.FORMS), "the shape grid no longer reaches every launch form"


def _force(monkeypatch, form):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in A.FORMS[form].items():
        monkeypatch.setenv(name, value)


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


@pytest.mark.parametrize("P,F,form", [pytest.param(P, F, form, id=f"P{P}F{F}-{form}") for P, F in MOTIONFORMER
                                      for form, env in A.FORMS.items()
                                      if A.expected_form(1, 1 + P * F, 2 * 12, env) == form])
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


@pytest.mark.parametrize("N,Nk,form", _grid(OUT_SHAPES, B * H))
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


@pytest.mark.parametrize("P,F,form", [pytest.param(P, F, form, id=f"P{P}F{F}-{form}") for P, F in SEGMENTS
                                      for form, env in A.FORMS.items()
                                      if A.expected_form(P * F, P, B * H * F, env) == form])
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
    write at a wrapped 32-bit offset lands in another slice and shows.  Default dispatch (persistent 8-wave stream
    kernel at this size) and TOME_ATTN_WAVES=4."""
    _abi_ = _abi()
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if waves:
        monkeypatch.setenv("TOME_ATTN_WAVES", waves)
    Bb, N, Hb = 640, 1568, 12
    assert A.expected_form(N, N, Bb * Hb, {} if waves is None else {"TOME_ATTN_WAVES": waves}) == \
        ("stream" if waves is None else "wave4")
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
