#!/usr/bin/env python3
"""TimeSformer's temporal attention in isolation: 64 x P sequences of 8 tokens (12 heads x 64) as strided views of
one qkv buffer -- PyTorch-ROCm's fused attention + the head transpose against tome_short_attention (HIP events).
    python tools/temporal_attn_bench.py"""
import torch
import torch.nn.functional as F

import ab
from tome import _abi


def main():
    dev = torch.device(ab.DEV)
    for ours in (False, True):
        for P in (196, 148, 100, 52, 20):
            B = 64 * P
            qkv = torch.randn(B, 8, 3, 12, 64, device=dev).bfloat16()
            q, k, v = qkv.permute(2, 0, 3, 1, 4)
            if ours:
                t = ab.time_us(lambda: _abi.short_attention(q, k, v, 0.125), 30, warmup=5)
            else:
                with torch.no_grad():
                    t = ab.time_us(lambda: F.scaled_dot_product_attention(q, k, v, scale=0.125).transpose(1, 2)
                                   .reshape(B, 8, 768), 30, warmup=5)
            byt = B * 8 * 768 * 2 * 4
            print(f"{'ours ' if ours else ''}P={P}: {B} sequences, {t:.1f} us, {byt/t/1e6:.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
