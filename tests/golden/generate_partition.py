#!/usr/bin/env python3
"""Golden vectors of kth_bipartite_soft_matching / random_bipartite_soft_matching (reference tome/merge.py:105-212).

Runs only where the reference checkout is available (TOME_REFERENCE, default /root/reference): it loads the
reference's own ``tome/merge.py`` by file path, feeds it the deterministic inputs of ``tests/synth.py`` and stores
what the reference answered on the CPU in ``partition.npz`` + ``partition_manifest.json``.  Only seeds and outputs
are stored -- no reference source text.

Per case:
  dst    the reference's ``dst_idx`` [n, Na]
  cert   per source row: is the fp64 gap between the two largest similarities of its row > TAU?  Rows below that
         depend on the summation order of the implementation; the tests leave them out (and, for value comparisons,
         the destinations such a row may go to).  At most CAP = 1 % of a case's rows may be uncertified: asserted
         here, with a search over a handful of seeds.
  a, b   random cases only: the ``a_idx`` / ``b_idx`` the reference drew from the CPU generator (which no device
         generator reproduces); the tests hand them to the partition matching directly
  sum, mean, amax, unmerge, wavg_x, wavg_s [, source]
         merge(x, mode) / unmerge(merge(x, "mean")) / merge_wavg / merge_source on fp32 x, rows ``row_step`` apart
         (unmerge: 4 * row_step apart)

Metrics of 16-bit cases are the synthetic values rounded to that dtype; the reference is run on those values held in
fp32 (its own 16-bit CPU arithmetic is a different computation, not the one the certificate speaks about).
The reference's merge_source asks for reduce="max", a name the installed torch's scatter_reduce does not accept: the
closure is called with "amax" there (same reduction).
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import synth  # noqa: E402

REF = os.environ.get("TOME_REFERENCE", "/root/reference")
TAU = 1e-6   # the value generate.py uses
CAP = 0.01   # largest share of uncertified source rows per case
SEED_TRIES = 5


def load_ref(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def closure_vars(fn):
    return dict(zip(fn.__code__.co_freevars, (c.cell_contents for c in fn.__closure__)))


# id, kind, n, T, D, k or r, metric kind, metric dtype, C of the values, row_step, flags
CASES = [
    dict(id="k2_1568", fn="kth", n=1, T=1568, D=64, k=2, kind="normal", dtype="float32", C=8, row_step=4),
    dict(id="k4_1568_clustered", fn="kth", n=1, T=1568, D=64, k=4, kind="clustered", dtype="float32", C=12, row_step=4),
    dict(id="k7_1568_bf16", fn="kth", n=1, T=1568, D=64, k=7, kind="normal", dtype="bfloat16", C=8, row_step=4),
    dict(id="k3_197_concat", fn="kth", n=1, T=197, D=768, k=3, kind="normal", dtype="float32", C=768, row_step=8,
         source=True),
    dict(id="k8_3137_fp16", fn="kth", n=1, T=3137, D=64, k=8, kind="clustered", dtype="float16", C=1),
    dict(id="k3_197_d20", fn="kth", n=2, T=197, D=20, k=3, kind="normal", dtype="float32", C=8),
    dict(id="k2_1568_clustered_bf16", fn="kth", n=1, T=1568, D=64, k=2, kind="clustered", dtype="bfloat16", C=8, row_step=4),
    dict(id="k4_200_zero_rows", fn="kth", n=2, T=200, D=64, k=4, kind="normal", dtype="float32", C=8,
         zero_tokens=[0, 23]),
    dict(id="r1_197", fn="random", n=2, T=197, D=64, r=1, kind="normal", dtype="float32", C=8),
    dict(id="r50_197_clustered", fn="random", n=2, T=197, D=64, r=50, kind="clustered", dtype="float32", C=12),
    dict(id="r784_1568_bf16", fn="random", n=1, T=1568, D=64, r=784, kind="normal", dtype="bfloat16", C=8, row_step=4),
    dict(id="r196_197", fn="random", n=2, T=197, D=64, r=196, kind="normal", dtype="float32", C=8, source=True),
    dict(id="r50_1568_concat_fp16", fn="random", n=1, T=1568, D=768, r=50, kind="normal", dtype="float16", C=1),
    dict(id="r98_197_d20_zero_rows", fn="random", n=2, T=197, D=20, r=98, kind="normal", dtype="float32", C=24,
         zero_tokens=[5, 100]),
]


def make_metric(case, seed) -> np.ndarray:
    shape = (case["n"], case["T"], case["D"])
    m = synth.normal_like(shape, seed) if case["kind"] == "normal" else synth.clustered(shape, seed)
    if case["dtype"] == "bfloat16":
        m = synth.bf16_round(m)
    elif case["dtype"] == "float16":
        m = m.astype(np.float16).astype(np.float32)
    for t in case.get("zero_tokens", ()):
        m[:, t, :] = 0.0
    return np.ascontiguousarray(m, dtype=np.float32)


def sets_of(case, a_idx=None, b_idx=None):
    """Token positions of the source rows and of the destination rows, [n, Na] / [n, Nb]."""
    n, T = case["n"], case["T"]
    if case["fn"] == "kth":
        k = case["k"]
        pos = np.arange((T // k) * k).reshape(-1, k)
        a, b = pos[:, :k - 1].reshape(-1), pos[:, k - 1]
        return np.broadcast_to(a, (n, a.size)), np.broadcast_to(b, (n, b.size))
    return a_idx, b_idx


def certificate(metric, a_pos, b_pos, dst):
    """fp64 top-2 gap of every source row; a row with NaN scores is decided by torch.max's NaN rule and counts as
    certified.  The reference's answer must be the fp64 argmax on every certified row."""
    m = torch.from_numpy(metric).double()
    m = m / m.norm(dim=-1, keepdim=True)
    n = m.shape[0]
    cert = np.zeros(dst.shape, dtype=bool)
    for g in range(n):
        a, b = m[g, torch.from_numpy(a_pos[g].copy())], m[g, torch.from_numpy(b_pos[g].copy())]
        s = a @ b.T
        has_nan = torch.isnan(s).any(dim=1)
        if s.shape[1] >= 2:
            top = torch.nan_to_num(s, nan=-2.0).topk(2, dim=1).values
            gap = top[:, 0] - top[:, 1]
        else:
            gap = torch.full((s.shape[0],), float("inf"), dtype=torch.float64)
        ok = (gap > TAU) | has_nan
        best = torch.nan_to_num(s, nan=-2.0).argmax(dim=1)
        first_nan = torch.isnan(s).double().argmax(dim=1)
        want = torch.where(has_nan, first_nan, best).numpy()
        assert np.array_equal(want[ok.numpy()], dst[g][ok.numpy()]), "reference disagrees with fp64 on a certified row"
        cert[g] = ok.numpy()
    return cert


def run_case(ref, case, seed):
    metric = make_metric(case, seed)
    mt = torch.from_numpy(metric)
    n, T = case["n"], case["T"]
    out = {}
    if case["fn"] == "kth":
        merge, unmerge = ref.kth_bipartite_soft_matching(mt, case["k"])
        a_pos, b_pos = sets_of(case)
    else:
        torch.manual_seed(seed)
        merge, unmerge = ref.random_bipartite_soft_matching(mt, case["r"])
        cv = closure_vars(closure_vars(merge)["split"])  # (the index lists are variables of its `split` helper)
        a_pos, b_pos = cv["a_idx"][..., 0].numpy(), cv["b_idx"][..., 0].numpy()
        out["a"], out["b"] = a_pos.astype(np.int16), b_pos.astype(np.int16)
    dst = closure_vars(merge)["dst_idx"][..., 0].numpy()
    cert = certificate(metric, a_pos, b_pos, dst)
    out["dst"], out["cert"] = dst.astype(np.int16), cert
    bad = 1.0 - cert.mean()
    if bad > CAP:
        return None, bad
    C, step = case["C"], case.get("row_step", 1)
    x = torch.from_numpy(synth.normal_like((n, T, C), seed + 1))
    size = torch.from_numpy(synth.small_ints((n, T, 1), seed + 2))
    for mode in ("sum", "mean", "amax"):
        out[mode] = merge(x, mode=mode)[:, ::step].numpy()
    out["unmerge"] = unmerge(merge(x, mode="mean"))[:, ::4 * step].numpy()  # (T rows: a quarter of them)
    wx, ws = ref.merge_wavg(merge, x, size)
    out["wavg_x"], out["wavg_s"] = wx[:, ::step].numpy(), ws[:, ::step].numpy()
    if case.get("source"):
        src = ref.merge_source(lambda t, mode: merge(t, mode="amax" if mode == "max" else mode), x)
        assert set(np.unique(src.numpy())) <= {0.0, 1.0}
        out["source"] = src.numpy().astype(np.uint8)
    return out, bad


def main():
    ref = load_ref("_ref_tome_merge", "tome/merge.py")
    arrays, manifest = {}, {"tau": TAU, "cap": CAP, "torch": torch.__version__, "cases": []}
    for ci, case in enumerate(CASES):
        for attempt in range(SEED_TRIES):
            seed = 104729 * (ci + 1) + 31 * attempt
            out, bad = run_case(ref, case, seed)
            if out is not None:
                break
        assert out is not None, f"{case['id']}: more than {CAP:.0%} uncertified rows for {SEED_TRIES} seeds ({bad:.3%})"
        entry = dict(case, seed=seed, uncertified=int((~out["cert"]).sum()), rows=int(out["cert"].size))
        manifest["cases"].append(entry)
        for key, val in out.items():
            arrays[f"{case['id']}/{key}"] = val
        print(f"{case['id']}: seed {seed}, {entry['uncertified']}/{entry['rows']} uncertified rows")
    np.savez_compressed(os.path.join(HERE, "partition.npz"), **arrays)
    with open(os.path.join(HERE, "partition_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    print(os.path.getsize(os.path.join(HERE, "partition.npz")), "bytes")


if __name__ == "__main__":
    main()
