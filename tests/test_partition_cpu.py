"""kth_bipartite_soft_matching / random_bipartite_soft_matching: what needs no device -- the fixture file and its
certificates, and the argument handling in front of any launch."""
import numpy as np
import pytest
import torch

import partition_cases as P


def _tm():
    from tome import merge as tm
    return tm


def test_fixture_loads_and_certificates_satisfy_the_cap():
    man = P.manifest()
    assert man["tau"] == 1e-6 and man["cap"] == 0.01
    assert len(man["cases"]) >= 12
    for case in man["cases"]:
        cert, dst = P.array(case, "cert"), P.array(case, "dst")
        a, b = P.positions(case)
        assert cert.shape == dst.shape == a.shape
        assert (~cert).sum() == case["uncertified"] and cert.size == case["rows"]
        assert (~cert).mean() <= man["cap"], case["id"]
        assert dst.min() >= 0 and dst.max() < b.shape[1]
        for g in range(case["n"]):  # the two sets are disjoint positions of the sequence
            both = np.concatenate([a[g], b[g]])
            assert len(set(both.tolist())) == both.size and both.min() >= 0 and both.max() < case["T"]
        for key in ("sum", "mean", "amax", "wavg_x", "wavg_s", "unmerge"):
            assert P.has(case, key), (case["id"], key)
            assert np.isfinite(P.array(case, key)).all()  # (a zero metric row makes NaN scores, never NaN tokens)


def test_fixture_certified_rows_are_the_fp64_argmax():
    for case in P.cases():
        if case.get("zero_tokens"):
            continue
        s = P.scores64(case)
        cert, dst = P.array(case, "cert"), P.array(case, "dst")
        assert np.array_equal(s.argmax(-1)[cert], dst[cert]), case["id"]


def test_trivial_arguments_give_do_nothing():
    tm = _tm()
    metric = torch.zeros(2, 10, 8)  # a CPU tensor: nothing may touch it
    for k in (1, 0, -3):
        assert tm.kth_bipartite_soft_matching(metric, k) == (tm.do_nothing, tm.do_nothing)
    for r in (0, -1):
        assert tm.random_bipartite_soft_matching(metric, r) == (tm.do_nothing, tm.do_nothing)


def test_calls_the_reference_cannot_answer_raise_value_error():
    tm = _tm()
    metric = torch.zeros(2, 10, 8)
    with pytest.raises(ValueError):
        tm.kth_bipartite_soft_matching(metric, 11)
    for r in (10, 11):
        with pytest.raises(ValueError):
            tm.random_bipartite_soft_matching(metric, r)


def test_cpu_tensors_are_refused_with_text():
    tm = _tm()
    from tome import _abi
    with pytest.raises(_abi.TomeHipError, match="HIP device"):
        tm.kth_bipartite_soft_matching(torch.zeros(2, 10, 8), 2)
    with pytest.raises(_abi.TomeHipError, match="HIP device"):
        tm.random_bipartite_soft_matching(torch.zeros(2, 10, 8), 3)


def test_partition_entry_points_validate_arguments_without_gpu():
    from tome import _abi
    L = _abi.lib()
    assert L.tome_partition_workspace_bytes(8, 784, 784, 64) % 256 == 0
    assert L.tome_partition_workspace_bytes(8, 784, 0, 64) == 0
    one = 1 << 20  # stands for a non-null pointer; every call below is refused before it is used
    rc = L.tome_match_partition(one, 0, 2, 16, 8, 128, 8, 1, None, None, 8, 8, one, one, one, one, 1 << 30, None)
    assert rc == 1 and b"k=1" in L.tome_last_error()
    rc = L.tome_match_partition(one, 0, 2, 16, 8, 128, 8, 0, one, one, 16, 0, one, one, one, one, 1 << 30, None)
    assert rc == 1 and b"empty destination set" in L.tome_last_error()
    rc = L.tome_match_partition(one, 0, 2, 16, 8, 128, 8, 0, None, None, 8, 8, one, one, one, one, 1 << 30, None)
    assert rc == 1 and b"null a_idx" in L.tome_last_error()
    rc = L.tome_match_partition(one, 0, 2, 16, 8, 128, 8, 0, one + 4, one, 8, 8, one, one, one, one, 1 << 30, None)
    assert rc == 1 and b"misaligned" in L.tome_last_error()
    rc = L.tome_match_partition(one, 0, 2, 16, 8, 128, 8, 4, None, None, 12, 4, None, one, one, one, 1 << 30, None)
    assert rc == 1 and b"null output" in L.tome_last_error()
    rc = L.tome_match_partition(one, 0, 2, 16, 8, 128, 8, 4, None, None, 12, 4, one, one, one, one, 16, None)
    assert rc == 2
    rc = L.tome_merge_partition(None, 0, 2, 16, 8, 4, None, None, 12, 4, one, one, 0, one, None)
    assert rc == 1 and b"tome_merge_partition" in L.tome_last_error()
    rc = L.tome_merge_partition(one, 0, 2, 16, 8, 4, None, None, 12, 4, one, one + 2, 0, one, None)
    assert rc == 1 and b"misaligned" in L.tome_last_error()
    rc = L.tome_merge_wavg_partition(one, 0, None, 0, 2, 16, 8, 4, None, None, 12, 4, one, one, one, None, None, None)
    assert rc == 1
    rc = L.tome_unmerge_partition(one, 0, 2, 16, 8, 4, None, None, 12, 4, None, one, None)
    assert rc == 1 and b"dst_idx" in L.tome_last_error()
