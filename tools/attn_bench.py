#!/usr/bin/env python3
"""tome_prop_attention in isolation (HIP events, random bf16 q/k/v as strided views of one qkv buffer) next to
PyTorch-ROCm's fused attention, plain and with the per-key log(size) bias.
    python tools/attn_bench.py [--quick]"""
import sys

import torch
import torch.nn.functional as F

import ab
from tome import _abi


def main():
    dev = torch.device(ab.DEV)
    torch.manual_seed(0)
    shapes = [(128, 12, 1568), (128, 12, 1472), (8, 12, 3137), (64, 12, 197), (8, 12, 1568)]
    if "--quick" in sys.argv:
        shapes = shapes[:2]
    for arg in sys.argv[1:]:
        if arg.startswith("--shapes="):  # --shapes=128x12x1536,128x12x1600
            shapes = [tuple(int(v) for v in sh.split("x")) for sh in arg.split("=", 1)[1].split(",")]
    ours_only = "--ours" in sys.argv
    for (B, H, N) in shapes:
        qkv = torch.randn(B, N, 3, H, 64, device=dev).bfloat16()
        q, k, v = qkv.permute(2, 0, 3, 1, 4)
        size = torch.randint(1, 9, (B, N, 1), device=dev).float()
        bias = size.log()[:, None, None, :, 0].bfloat16()
        fl = 4.0 * B * H * N * N * 64
        with torch.no_grad():
            t0 = t1 = float("nan")
            if not ours_only:
                t0 = ab.time_us(lambda: F.scaled_dot_product_attention(q, k, v, scale=0.125), 20, warmup=5)
                t1 = ab.time_us(lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=bias, scale=0.125), 20, warmup=5)
            t2 = ab.time_us(lambda: _abi.prop_attention(q, k, v, None, 0.125), 20, warmup=5)
            t3 = ab.time_us(lambda: _abi.prop_attention(q, k, v, size, 0.125), 20, warmup=5)
        print(f"{(B, H, N)}: sdpa {t0:7.1f} us ({fl / t0 / 1e6:5.0f} TF/s) | sdpa+bias {t1:7.1f} ({fl / t1 / 1e6:5.0f}) | "
              f"ours {t2:7.1f} ({fl / t2 / 1e6:5.0f}) | ours+bias {t3:7.1f} ({fl / t3 / 1e6:5.0f})", flush=True)


if __name__ == "__main__":
    main()
