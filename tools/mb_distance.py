"""Dense pairwise distance timing: ops.pairwise_distance (dm_pairwise_distance, one fused launch) on device tensors against the
roofline bound max(4 n m B / HBM, 2 n m p / fp32 matrix peak) at nominal 8 TB/s and 157.3 TF, with torch.cdist
(compute_mode="use_mm_for_euclid_dist": norms + vendor GEMM + clamp / sqrt) on the same box as a yardstick.
Usage: python tools/mb_distance.py [--iters N]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from deepmerge_amd import ops  # noqa: E402

HBM_BPS = 8.0e12
FP32_MATRIX_FLOPS = 157.3e12
SHAPES = [(19881, 19881, 100, "config 4 superpixels"), (59600, 2000, 100, "59.6k points x 2k centres"),
          (4096, 4096, 768, "ViT width"), (19881, 19881, 3, "store-bound, p = 3")]


def time_ms(fn, iters):
    for _ in range(3):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = "cuda:0"
    print(f"device {torch.cuda.get_device_name(0)}; bound = max(4nm B / {HBM_BPS / 1e12:.0f} TB/s, 2nmp / {FP32_MATRIX_FLOPS / 1e12:.1f} TF); "
          f"{args.iters} timed calls per row, hipEvent timing, output allocated per call (caching allocator)")
    print(f"{'n':>6} {'m':>6} {'p':>4}  {'kernel':>8} {'ms':>8} {'TFLOP/s':>8} {'GB/s':>7} {'bound ms':>8} {'of bound':>8}   "
          f"{'cdist ms':>8} {'of bound':>8}  {'max|diff|':>9}  shape")
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    for n, m, p, what in SHAPES:
        X = torch.randn((n, p), device=dev, generator=g)
        Y = torch.randn((m, p), device=dev, generator=g)
        flops, nbytes = 2.0 * n * m * p, 4.0 * n * m
        bound = max(nbytes / HBM_BPS, flops / FP32_MATRIX_FLOPS) * 1e3
        t = time_ms(lambda: ops.pairwise_distance(X, Y), args.iters)
        tc = time_ms(lambda: torch.cdist(X, Y, compute_mode="use_mm_for_euclid_dist"), args.iters)
        diff = float((ops.pairwise_distance(X, Y) - torch.cdist(X, Y, compute_mode="use_mm_for_euclid_dist")).abs().max())
        kind = "matrix" if flops / FP32_MATRIX_FLOPS > nbytes / HBM_BPS else "stores"
        print(f"{n:>6} {m:>6} {p:>4}  {kind:>8} {t:8.3f} {flops / t / 1e9:8.1f} {nbytes / t / 1e6:7.0f} {bound:8.3f} {bound / t:8.2f}   "
              f"{tc:8.3f} {bound / tc:8.2f}  {diff:9.2e}  {what}")
        del X, Y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
