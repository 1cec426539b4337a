"""The refusals of tome_drop_ln and tome_drop_regrouped_ln, one call per refusal with exactly one fault each:
(return code, tome_last_error()) held to literals.  Every call returns before anything touches the GPU; there is no
call without a fault here, it would try to launch."""
import ctypes

import pytest

_BUF = ctypes.create_string_buffer(1024)
P = (ctypes.addressof(_BUF) + 255) & ~255  # a 256-byte aligned host address; no refused call reads it

# a call of each entry that has no fault: each row of REFUSALS replaces the arguments it names
GOOD = {
    "tome_drop_ln": dict(x=P, dtype=1, n=2, T=16, C=64, r=4, und_idx=P, distill_token=0, ln_weight=P, ln_bias=P,
                         eps=1e-6, addend=P, x_out=P, y_out=P, x_out_bias=P, stream=None),
    "tome_drop_regrouped_ln": dict(x=P, dtype=2, B=2, F=2, P=16, C=64, r=4, has_cls=1, und_idx=P, ln_weight=P,
                                   ln_bias=P, eps=1e-6, addend=P, addend_grouped=1, cls_addend=P, x_out=P, y_out=P,
                                   x_out_bias=P, stream=None),
}

REFUSALS = [
    ("tome_drop_ln", dict(x=None), 1, "tome_drop_ln: bad shape/pointer"),
    ("tome_drop_ln", dict(x_out=None), 1, "tome_drop_ln: bad shape/pointer"),
    ("tome_drop_ln", dict(n=0), 1, "tome_drop_ln: bad shape/pointer"),
    ("tome_drop_ln", dict(r=0), 1, "tome_drop_ln: r=0 outside (0, T/2]"),
    ("tome_drop_ln", dict(r=9), 1, "tome_drop_ln: r=9 outside (0, T/2]"),
    ("tome_drop_ln", dict(und_idx=None), 1, "tome_drop_ln: null index buffer"),
    ("tome_drop_ln", dict(y_out=None), 1, "tome_drop_ln: null buffer"),
    ("tome_drop_ln", dict(ln_weight=None), 1, "tome_drop_ln: null buffer"),
    ("tome_drop_ln", dict(ln_bias=None), 1, "tome_drop_ln: null buffer"),
    ("tome_drop_ln", dict(dtype=0), 1, "tome_drop_ln: 16-bit tokens only (dtype=0)"),
    ("tome_drop_ln", dict(dtype=5), 1, "tome_drop_ln: 16-bit tokens only (dtype=5)"),
    ("tome_drop_ln", dict(C=12), 1, "tome_drop_ln: C=12 must be a multiple of 8, at most 1024"),
    ("tome_drop_ln", dict(C=1032), 1, "tome_drop_ln: C=1032 must be a multiple of 8, at most 1024"),
    ("tome_drop_ln", dict(x=P + 8), 1, "tome_drop_ln: x / x_out not 16-byte aligned"),
    ("tome_drop_ln", dict(x_out=P + 2), 1, "tome_drop_ln: x / x_out not 16-byte aligned"),
    ("tome_drop_ln", dict(y_out=P + 8), 1, "tome_drop_ln: y_out not 16-byte aligned"),
    ("tome_drop_ln", dict(ln_weight=P + 4), 1, "tome_drop_ln: ln_weight / ln_bias not 16-byte aligned"),
    ("tome_drop_ln", dict(ln_bias=P + 2), 1, "tome_drop_ln: ln_weight / ln_bias not 16-byte aligned"),
    ("tome_drop_ln", dict(addend=P + 8), 1, "tome_drop_ln: addend not 16-byte aligned"),
    ("tome_drop_ln", dict(x_out_bias=P + 8), 1, "tome_drop_ln: x_out_bias not 16-byte aligned"),
    ("tome_drop_regrouped_ln", dict(B=0), 1, "tome_drop_regrouped_ln: bad shape"),
    ("tome_drop_regrouped_ln", dict(F=0), 1, "tome_drop_regrouped_ln: bad shape"),
    ("tome_drop_regrouped_ln", dict(x=None), 1, "tome_drop_regrouped_ln: bad shape/pointer"),
    ("tome_drop_regrouped_ln", dict(x_out=None), 1, "tome_drop_regrouped_ln: bad shape/pointer"),
    ("tome_drop_regrouped_ln", dict(r=0), 1, "tome_drop_regrouped_ln: r=0 outside (0, T/2]"),
    ("tome_drop_regrouped_ln", dict(r=9), 1, "tome_drop_regrouped_ln: r=9 outside (0, T/2]"),
    ("tome_drop_regrouped_ln", dict(und_idx=None), 1, "tome_drop_regrouped_ln: null index buffer"),
    ("tome_drop_regrouped_ln", dict(y_out=None), 1, "tome_drop_regrouped_ln: null buffer"),
    ("tome_drop_regrouped_ln", dict(ln_weight=None), 1, "tome_drop_regrouped_ln: null buffer"),
    ("tome_drop_regrouped_ln", dict(ln_bias=None), 1, "tome_drop_regrouped_ln: null buffer"),
    ("tome_drop_regrouped_ln", dict(dtype=0), 1, "tome_drop_regrouped_ln: 16-bit tokens only (dtype=0)"),
    ("tome_drop_regrouped_ln", dict(C=12), 1, "tome_drop_regrouped_ln: C=12 must be a multiple of 8, at most 1024"),
    ("tome_drop_regrouped_ln", dict(C=1032), 1, "tome_drop_regrouped_ln: C=1032 must be a multiple of 8, at most 1024"),
    ("tome_drop_regrouped_ln", dict(x=P + 4), 1, "tome_drop_regrouped_ln: x / x_out not 16-byte aligned"),
    ("tome_drop_regrouped_ln", dict(y_out=P + 8), 1, "tome_drop_regrouped_ln: y_out not 16-byte aligned"),
    ("tome_drop_regrouped_ln", dict(ln_weight=P + 8), 1, "tome_drop_regrouped_ln: ln_weight / ln_bias not 16-byte aligned"),
    ("tome_drop_regrouped_ln", dict(addend=P + 8), 1, "tome_drop_regrouped_ln: addend not 16-byte aligned"),
    ("tome_drop_regrouped_ln", dict(cls_addend=P + 8), 1, "tome_drop_regrouped_ln: addend not 16-byte aligned"),
    ("tome_drop_regrouped_ln", dict(x_out_bias=P + 2), 1, "tome_drop_regrouped_ln: x_out_bias not 16-byte aligned"),
    # the grouped residual is read through a layout of its own, with or without a class token (has_cls only moves its
    # rows): what is refused is the flag without the tensor
    ("tome_drop_regrouped_ln", dict(addend=None), 1, "tome_drop_regrouped_ln: addend_grouped without addend"),
]


@pytest.mark.parametrize("entry,fault,rc,text", REFUSALS, ids=[f"{e}-{i}" for i, (e, *_) in enumerate(REFUSALS)])
def test_refusal(entry, fault, rc, text):
    from tome import _abi
    L = _abi.lib()
    args = dict(GOOD[entry])
    assert set(fault) <= set(args), (entry, fault)
    args.update(fault)
    assert len(args) == len(_abi.SIGNATURES[entry][1])
    got = _abi.require_symbol(L, entry)(*args.values())
    assert (got, L.tome_last_error().decode()) == (rc, text)


def test_the_new_entries_are_flagged_as_added_later():
    """A v11 library built before them still binds (test_abi_cpu holds that for every flagged row)."""
    from tome import _abi
    assert _abi.SIGNATURES["tome_drop_ln"][2] and _abi.SIGNATURES["tome_drop_regrouped_ln"][2]
