"""Access to tests/golden/partition.npz (what the reference's kth_ / random_bipartite_soft_matching answered;
tests/golden/generate_partition.py) for test_partition_cpu.py and test_partition_gpu.py."""
import functools
import json
import os

import numpy as np

import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def manifest():
    with open(os.path.join(GOLDEN, "partition_manifest.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _npz():
    return np.load(os.path.join(GOLDEN, "partition.npz"))


def cases():
    return manifest()["cases"]


def ids():
    return [c["id"] for c in cases()]


def array(case, key):
    return _npz()[f"{case['id']}/{key}"]


def has(case, key):
    return f"{case['id']}/{key}" in _npz().files


def metric_of(case) -> np.ndarray:
    """The case's metric as fp32 values that are exact in the case's dtype (generate_partition.make_metric)."""
    shape = (case["n"], case["T"], case["D"])
    m = synth.normal_like(shape, case["seed"]) if case["kind"] == "normal" else synth.clustered(shape, case["seed"])
    if case["dtype"] == "bfloat16":
        m = synth.bf16_round(m)
    elif case["dtype"] == "float16":
        m = m.astype(np.float16).astype(np.float32)
    for t in case.get("zero_tokens", ()):
        m[:, t, :] = 0.0
    return np.ascontiguousarray(m, dtype=np.float32)


def x_of(case) -> np.ndarray:
    return synth.normal_like((case["n"], case["T"], case["C"]), case["seed"] + 1)


def size_of(case) -> np.ndarray:
    return synth.small_ints((case["n"], case["T"], 1), case["seed"] + 2)


def positions(case):
    """Token positions of the source rows [n,Na] and of the destination rows [n,Nb] (int64)."""
    n, T = case["n"], case["T"]
    if case["fn"] == "kth":
        k = case["k"]
        pos = np.arange((T // k) * k, dtype=np.int64).reshape(-1, k)
        a, b = pos[:, :k - 1].reshape(-1), pos[:, k - 1]
        return np.broadcast_to(a, (n, a.size)).copy(), np.broadcast_to(b, (n, b.size)).copy()
    return array(case, "a").astype(np.int64), array(case, "b").astype(np.int64)


def scores64(case):
    """fp64 cosine similarity A.B^T per group, [n,Na,Nb] (NaN where a token has no direction)."""
    m = metric_of(case).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = m / np.linalg.norm(m, axis=-1, keepdims=True)
    a, b = positions(case)
    return np.stack([m[g, a[g]] @ m[g, b[g]].T for g in range(case["n"])])
