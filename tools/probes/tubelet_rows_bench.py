#!/usr/bin/env python3
"""tome_tubelet_rows against the framework's permute-copy on the four hosts' clip shapes (bf16)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # tools/, for ab
import torch  # noqa: E402

import ab  # noqa: E402
from tome import _abi  # noqa: E402


def main():
    dev = torch.device(ab.DEV)
    for name, B, T, kt, view in (("videomae 384 x 16 frames", 384, 16, 2, "plain"), ("videomae 8 x 16 frames", 8, 16, 2, "plain"),
                                 ("timesformer 384 x 8 frames (per frame)", 384, 8, 1, "plain"),
                                 ("vivit 64 x 32 frames [B,T,C,H,W]", 64, 32, 2, "btchw")):
        if view == "btchw":
            x = torch.rand(B, T, 3, 224, 224, device=dev).bfloat16().permute(0, 2, 1, 3, 4)
        else:
            x = torch.rand(B, 3, T, 224, 224, device=dev).bfloat16()
        nt = T // kt

        def by_views():
            return x.reshape(B, 3, nt, kt, 14, 16, 14, 16).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, nt * 196, 3 * kt * 256)

        t_k = ab.time_us(lambda: _abi.tubelet_rows(x, kt, 16, 16), 10, warmup=3)
        t_v = ab.time_us(by_views, 10, warmup=3)
        gb = 2 * x.numel() * 2 / 1e9
        print(f"{name:42s}: kernel {t_k:8.1f} us = {gb / t_k * 1e3:5.2f} TB/s   framework permute-copy {t_v:8.1f} us = "
              f"{gb / t_v * 1e3:5.2f} TB/s", flush=True)
        del x


if __name__ == "__main__":
    main()
