"""tome_token_mean (k_token_mean): the fp32 column mean over a clip's tokens, plain and of the exact-erf GELU's stored bits.

Accounting (act = 0): small-integer tokens, so every partial sum is exact in fp32 whatever its order -- `out * tokens`
must be the integer column sums (out the correctly rounded quotient of exactly that integer: a row or channel read
twice, left out or added to a neighbour's column changes the integer), then single elements set to distinct powers of
two must show up in exactly their own outputs; the words around `out` stay untouched.  Values (act = 1): against the float64 mean of tome_gelu_erf's own output bits,
within the fp32 summation bound of ANY order, (tokens - 1) 2^-24 mean|a|, plus the one rounding of the division,
2^-24 |ref| -- derived, not measured.  Two calls give the same bits.  Every refusal returns its error and writes nothing.

Shapes: a single row; one row more and one less than a wave's stride (4 rows) and a workgroup's (32 rows: 4 waves x 8 rows
in flight), and than two of them; several steps plus a rest (257); a width below one lane-chunk row (8), one slab partly
filled (64), a width that is no multiple of the 512-channel slab (520: the second slab has one live lane), the headline
width (3072: six slabs); one group and three."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
GROUPS = [1, 3]
TOKENS = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 257]
WIDTHS = [8, 64, 520, 3072]
U = 2.0 ** -24  # unit roundoff of fp32
GUARD = 64      # fp32 words in front of and behind `out`
CODE = {torch.bfloat16: 1, torch.float16: 2}


def _abi():
    from tome import _abi
    return _abi


def _raw(x, groups, tokens, width, act, dtype_code=None, x_ptr=True, out_ptr=True):
    """The C entry on a guarded output buffer: (status, buffer [GUARD + groups * width + GUARD] as int32 words)."""
    abi = _abi()
    n = max(groups, 1) * max(width, 8)
    buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    sentinel = buf.view(torch.int32).clone()
    rc = abi.lib().tome_token_mean(x.data_ptr() if x_ptr else None, CODE[x.dtype] if dtype_code is None else dtype_code,
                                   groups, tokens, width, act, buf[GUARD:].data_ptr() if out_ptr else None,
                                   abi._stream(x.device))
    torch.cuda.synchronize()
    return rc, buf, sentinel


def _small_ints(shape, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=gen).to(dtype).to(DEV)


def _is_the_mean_of(out, sums, tokens):
    """`out * tokens` is the integer column sums: in float64 the product rounds to exactly those integers, and out is
    the correctly rounded fp32 quotient of them (the fp32 product itself need not return to the integer: 4343 / 31 * 31
    lands one ulp off; the float64 quotient of two small integers rounds to fp32 as the exact quotient does)."""
    return (torch.equal((out.double() * tokens).round(), sums) and torch.equal(out, (sums / tokens).float()))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tokens", TOKENS)
def test_every_row_and_channel_is_counted_once(tokens, dtype):
    abi = _abi()
    for groups in GROUPS:
        for width in WIDTHS:
            x = _small_ints((groups, tokens, width), dtype, 7 * tokens + width + groups)
            rc, buf, sentinel = _raw(x, groups, tokens, width, 0)
            assert rc == 0, abi.lib().tome_last_error()
            n = groups * width
            words = buf.view(torch.int32)
            assert torch.equal(words[:GUARD], sentinel[:GUARD]) and torch.equal(words[GUARD + n:], sentinel[GUARD + n:])
            out = buf[GUARD:GUARD + n].view(groups, width)
            sums = x.double().sum(1)
            assert _is_the_mean_of(out, sums, tokens), (groups, tokens, width)
            assert torch.equal(abi.token_mean(x), out)  # the wrapper: the same launch into a tensor of its own
            # distinct powers of two at distinct places: each in exactly its own output
            places = {(0, 0, 0): 8, (groups - 1, tokens - 1, width - 1): 9, (groups // 2, tokens // 2, width // 2): 10,
                      (groups - 1, 0, min(width - 1, 511)): 11, (0, tokens - 1, width - 8): 12}
            x2 = x.clone()
            for (g, t, c), p in places.items():
                x2[g, t, c] = 2.0 ** p
            out2 = abi.token_mean(x2)
            assert _is_the_mean_of(out2, x2.double().sum(1), tokens), (groups, tokens, width)
            touched = torch.zeros((groups, width), dtype=torch.bool, device=DEV)
            for (g, t, c) in places:
                touched[g, c] = True
            assert torch.equal(out2[~touched], out[~touched])


def _gelu_inputs(shape, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=gen) * 1.5).to(dtype)
    fi = torch.finfo(dtype)
    points = torch.tensor([0.0, -0.0, 9.0, -9.0, fi.max, -fi.max, fi.tiny, -fi.tiny], dtype=torch.float64).to(dtype)
    flat = x.view(-1)
    flat[:8] = points  # (every shape has at least 8 elements: width >= 8)
    return x.to(DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tokens", TOKENS)
def test_gelu_mean_against_the_stored_activation_bits(tokens, dtype):
    abi = _abi()
    for groups in GROUPS:
        for width in WIDTHS:
            h = _gelu_inputs((groups, tokens, width), dtype, 11 * tokens + width + groups)
            a = abi.gelu_erf(h, inplace=False).double()
            ref = a.mean(1)
            bound = (tokens - 1) * U * a.abs().mean(1) + U * ref.abs()
            out = abi.token_mean(h, gelu=True)
            assert out.dtype == torch.float32 and tuple(out.shape) == (groups, width)
            err = (out.double() - ref).abs()
            assert bool((err <= bound).all()), (groups, tokens, width, float((err - bound).max()))
            again = abi.token_mean(h, gelu=True)
            assert torch.equal(out.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_calls_give_the_same_bits(dtype):
    abi = _abi()
    x = _gelu_inputs((3, 257, 3072), dtype, 5)
    for gelu in (False, True):
        first, second = abi.token_mean(x, gelu=gelu), abi.token_mean(x, gelu=gelu)
        assert torch.equal(first.view(torch.int32), second.view(torch.int32))


def test_refusals_return_their_error_and_write_nothing():
    abi = _abi()
    x = _small_ints((3, 5, 64), torch.bfloat16, 3)
    bad = {
        "width % 8": dict(groups=3, tokens=5, width=60, act=0),
        "width 0": dict(groups=3, tokens=5, width=0, act=0),
        "tokens < 1": dict(groups=3, tokens=0, width=64, act=0),
        "groups < 1": dict(groups=0, tokens=5, width=64, act=0),
        "fp32": dict(groups=3, tokens=5, width=64, act=0, dtype_code=0),
        "unknown dtype": dict(groups=3, tokens=5, width=64, act=0, dtype_code=7),
        "unknown act": dict(groups=3, tokens=5, width=64, act=2),
        "negative act": dict(groups=3, tokens=5, width=64, act=-1),
        "null x": dict(groups=3, tokens=5, width=64, act=0, x_ptr=False),
        "null out": dict(groups=3, tokens=5, width=64, act=0, out_ptr=False),
    }
    for what, kw in bad.items():
        rc, buf, sentinel = _raw(x, **kw)
        assert rc == 1, what
        assert b"tome_token_mean" in abi.lib().tome_last_error(), what
        assert torch.equal(buf.view(torch.int32), sentinel), what
    with pytest.raises(abi.TomeHipError, match="token_mean"):
        abi.token_mean(x.float())
    with pytest.raises(abi.TomeHipError, match="token_mean"):
        abi.token_mean(x.transpose(0, 1))
    rc, buf, _ = _raw(x, 3, 5, 64, 0)  # ... and the legal call behind them goes through
    assert rc == 0 and bool(torch.isfinite(buf[GUARD:GUARD + 3 * 64]).all())
