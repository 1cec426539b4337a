"""Where does the fused add+merge+LN kernel lose time?  Same shapes, different index patterns."""
import os

import torch

import ab
from tome import _abi, merge as tm


COUNTS = dict(iters=20, warmup=3, sync=False)  # (this tool never synchronised between warm-up and timing)


def main():
    dev = torch.device(ab.DEV)
    B, T, C = int(os.environ.get("EXP_B", "64")), 1568, 768
    torch.manual_seed(0)
    x = torch.randn(B, T, C, device=dev, dtype=torch.bfloat16)
    a = torch.randn(B, T, C, device=dev, dtype=torch.bfloat16)
    w = torch.ones(C, device=dev, dtype=torch.bfloat16)
    b = torch.zeros(C, device=dev, dtype=torch.bfloat16)
    size = torch.ones(B, T, 1, device=dev, dtype=torch.bfloat16)

    def run(tag, r, sort_unm=False, sz=size, addend=a):
        metric = torch.randn(B, T, 64, device=dev)
        mg, _ = tm.bipartite_soft_matching(metric, r)
        plan = mg.plan
        if sort_unm:
            plan.unm_idx = plan.unm_idx.sort(dim=1)[0].contiguous()
        us = ab.time_us(lambda: _abi.merge_wavg_ln(plan, x, sz, w, b, 1e-6, addend=addend), **COUNTS)
        nbytes = B * ((2 if addend is not None else 1) * T * C * 2 + 2 * (T - r) * C * 2)
        us2 = ab.time_us(lambda: _abi.merge_wavg(plan, x, sz), **COUNTS)
        nb2 = B * (T * C * 2 + (T - r) * C * 2)
        print(f"{tag:34s} r={r:3d} add+merge+ln {us:7.1f} us {nbytes / us / 1e6:6.2f} TB/s | merge {us2:6.1f} us {nb2 / us2 / 1e6:5.2f} TB/s")

    run("random unm order", 16)
    run("sorted unm order", 16, sort_unm=True)
    run("r=1 random", 1)
    run("r=1 sorted", 1, sort_unm=True)
    run("size=None random", 16, sz=None)
    run("no addend random", 16, addend=None)
    run("no addend sorted", 16, sort_unm=True, addend=None)
    us = ab.time_us(lambda: _abi.add_layernorm(x, a, w, b, 1e-6), **COUNTS)
    print(f"add_layernorm same rows {us:7.1f} us {B * T * C * 2 * 4 / us / 1e6:6.2f} TB/s")

    ob = torch.randn(C, device=dev, dtype=torch.bfloat16)
    metric = torch.randn(B, T, 64, device=dev)
    plan = tm.bipartite_soft_matching(metric, 16)[0].plan
    for tag, kw in (("out_bias=None", {}), ("out_bias", {"out_bias": ob})):
        us = ab.time_us(lambda: _abi.merge_wavg_ln(plan, x, size, w, b, 1e-6, addend=a, **kw), **COUNTS)
        print(f"add+merge+ln {tag:14s} {us:7.1f} us")
    us = ab.time_us(lambda: _abi.add_layernorm(x, None, w, b, 1e-6), **COUNTS)
    print(f"layernorm only (no addend)  {us:7.1f} us {B * T * C * 2 * 2 / us / 1e6:6.2f} TB/s")
    y = torch.empty_like(x)
    us = ab.time_us(lambda: y.copy_(x), **COUNTS)
    print(f"torch copy                  {us:7.1f} us {B * T * C * 2 * 2 / us / 1e6:6.2f} TB/s")
    us = ab.time_us(lambda: torch.add(x, a, out=y), **COUNTS)
    print(f"torch add                   {us:7.1f} us {B * T * C * 2 * 3 / us / 1e6:6.2f} TB/s")


if __name__ == "__main__":
    main()
