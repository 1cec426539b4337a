"""The tensor-kind predicates of tome/_abi.py on a table of small views; no kernel is launched.

Every `*_ok` / `ln_fusable` is its kind's predicate and "no gradient wanted"; every `*_trainable` is that predicate with
no grad clause -- plus the three real differences: short_attention_trainable refuses aliased q, k, v, ln_trainable wants
the stock LayerNorm class and a bias of the tokens' dtype (ln_fusable takes a subclass and does not look at the bias).
The expected values are literals recorded from the commit before the predicates were folded."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


class _MyLayerNorm(torch.nn.LayerNorm):
    pass


def _heads(n=4, d=64, dtype=torch.bfloat16, pad=0, step=1, offset=0):
    """One [1, 1, n, d] head view: token stride d * step + pad elements, channel stride `step`, `offset` elements into
    its storage; head stride 64 (a single head: no element depends on it), which the short kernels ask for."""
    width = d * step + pad
    buf = torch.zeros(offset + n * width, dtype=dtype, device=DEV)
    return torch.as_strided(buf, (1, 1, n, d), (n * width, 64, width, step), offset)


def _tokens(dtype=torch.bfloat16, step=1, pad=0, offset=0):
    """64 rows of C = 64, built like _heads."""
    return _heads(64, 64, dtype, pad, step, offset)[0, 0]


def _norm(cls=torch.nn.LayerNorm, dtype=torch.bfloat16, bias_dtype=None):
    norm = cls(64).to(device=DEV, dtype=dtype)
    if bias_dtype is not None:
        norm.bias.data = norm.bias.data.to(bias_dtype)
    return norm


def _row(heads=None, x=None, norm=None, **view):
    """(q, k, v), x, norm of one table row: `view` shapes every tensor of the row alike."""
    heads = heads if heads is not None else tuple(_heads(**view) for _ in range(3))
    view = {key: value for key, value in view.items() if key not in ("n", "d")}  # (the tokens stay 64 rows of 64)
    return heads, (x if x is not None else _tokens(**view)), (norm if norm is not None else _norm())


def _aliased():
    q = _heads()
    return q, q, q


# name -> builder of the row
ROWS = {
    "good": lambda: _row(),
    "channel stride 2": lambda: _row(step=2),
    "token stride not a multiple of 8": lambda: _row(pad=4),
    "storage offset of 8 bytes": lambda: _row(offset=4),
    "fp32": lambda: _row(dtype=torch.float32, norm=_norm(dtype=torch.float32)),
    "head dim 32": lambda: _row(d=32),
    "short triple, aliased q = k = v": lambda: _row(heads=_aliased()),
    "short triple, N = 9": lambda: _row(n=9),
    "LayerNorm subclass": lambda: _row(norm=_norm(_MyLayerNorm)),
    "LayerNorm with fp32 bias": lambda: _row(norm=_norm(bias_dtype=torch.float32)),
}

# (prop_attention_ok, prop_attention_trainable, short_attention_ok, short_attention_trainable, ln_fusable, ln_trainable)
# with no gradient wanted, as the parent commit answers (tools of that commit, run on an MI355X).  With a gradient wanted
# the parent's *_ok / ln_fusable are all False and its *_trainable keep these values: asserted below for every row.
PARENT = {
    "good": (True, True, True, True, True, True),
    "channel stride 2": (False, False, False, False, True, True),
    "token stride not a multiple of 8": (False, False, False, False, True, True),
    "storage offset of 8 bytes": (False, False, False, False, True, True),
    "fp32": (False, False, False, False, False, False),
    "head dim 32": (False, False, False, False, True, True),
    "short triple, aliased q = k = v": (True, True, True, False, True, True),
    "short triple, N = 9": (True, True, False, False, True, True),
    "LayerNorm subclass": (True, True, True, True, True, False),
    "LayerNorm with fp32 bias": (True, True, True, True, True, False),
}
# the rows on which a real difference between the pair shows: there *_ok is NOT *_trainable and "no gradient wanted"
DIFFERENT = {"short triple, aliased q = k = v": "short", "LayerNorm subclass": "ln", "LayerNorm with fp32 bias": "ln"}


def evaluate(_abi, name, requires_grad):
    """The six predicates of row `name` under the current grad mode, every tensor with `requires_grad` as given."""
    (q, k, v), x, norm = ROWS[name]()
    for t in {id(t): t for t in (q, k, v, x)}.values():
        t.requires_grad_(requires_grad)
    norm.requires_grad_(requires_grad)
    return (all(_abi.prop_attention_ok(t) for t in (q, k, v)), _abi.prop_attention_trainable(q, k, v),
            _abi.short_attention_ok(q, k, v), _abi.short_attention_trainable(q, k, v),
            _abi.ln_fusable(x, norm), _abi.ln_trainable(x, norm))


@pytest.mark.parametrize("name", list(ROWS))
def test_ok_is_trainable_and_no_gradient_wanted(name):
    from tome import _abi
    assert set(ROWS) == set(PARENT)
    for requires_grad in (False, True):
        for mode in (torch.enable_grad, torch.no_grad):
            with mode():
                wanted = requires_grad and torch.is_grad_enabled()
                got = tuple(bool(b) for b in evaluate(_abi, name, requires_grad))
            print(name, "requires_grad", requires_grad, mode.__name__, got)
            p_ok, p_tr, s_ok, s_tr, l_ok, l_tr = PARENT[name]
            want = (p_ok and not wanted, p_tr, s_ok and not wanted, s_tr, l_ok and not wanted, l_tr)
            assert got == want, (name, requires_grad, mode.__name__, got, want)
            for kind, (ok, tr) in (("prop", got[0:2]), ("short", got[2:4]), ("ln", got[4:6])):
                if DIFFERENT.get(name) != kind:
                    assert ok == (tr and not wanted), (name, kind, requires_grad, mode.__name__)
