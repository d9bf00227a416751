#!/usr/bin/env python3
"""Train_SMT.train() throughput and the per-epoch draw.

  python tools/mb_train_smt.py draw [--pairs 1000000]     dm_pair_epoch_draw at N pairs (time it with rocprofv3 --kernel-trace --stats)
  python tools/mb_train_smt.py train [--epochs 3]        train() at the BASELINE configs[4] shape (v3 [6,4,2], 4 scales x 4 bands,
                                                          train_bs 120) on a synthetic dataset of ~20 steps per epoch; prints one JSON line
                                                          with the steady-state pairs/s (epochs after the first; no checkpoint is due)
Compare the second against `tools/train_synth.py --pairs 120` on the same box.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmerge_amd import Train_SMT, ops  # noqa: E402
from deepmerge_amd.dataset import PairDataset  # noqa: E402
from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3  # noqa: E402

DEV = "cuda:0"


def synthetic_images(n_images, bands, size, n_pairs, rng):
    """Images with 64 points per polygon-ish: windows in the ranges train_synth draws (inner 16..64, obj inner + 8..48)."""
    per = -(-n_pairs // n_images)
    ims = []
    for _ in range(n_images):
        n_poly = max(8, int(np.sqrt(2 * per)) + 2)
        n_pts = 4 * n_poly
        inner = rng.integers(16, 65, n_pts)
        flat = rng.choice(n_poly * n_poly, size=per, replace=False)
        pairs = np.stack((flat // n_poly, flat % n_poly), 1)
        ims.append({"tile": rng.integers(0, 256, size=(bands, size, size), dtype=np.uint8),
                    "xy": rng.integers(96, size - 96, (n_pts, 2)), "inner": inner, "obj": inner + rng.integers(8, 49, n_pts),
                    "region": np.exp(rng.uniform(-2.0, 3.0, (n_pts, 15))).astype(np.float32),
                    "polygon_points": [np.arange(k, n_pts, n_poly) for k in range(n_poly)],
                    "positive": pairs[: per // 2], "negative": pairs[per // 2:]})
    return ims


def run_draw(args):
    rng = np.random.default_rng(0)
    N, n_poly = args.pairs, 2048
    counts = rng.integers(1, 17, n_poly)
    n_pts = int(counts.sum())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pairs = up(rng.integers(0, n_poly, (N, 2)).astype(np.int32))
    poly_off = up(np.concatenate(([0], np.cumsum(counts))).astype(np.int32))
    poly_pts = up(rng.permutation(n_pts).astype(np.int32))
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=DEV)
    ins = (pairs, up(rng.integers(0, 2, N).astype(np.int32)), poly_off, poly_pts, up(rng.integers(0, 6, n_pts).astype(np.int32)),
           up(rng.integers(0, 1024, (n_pts, 2)).astype(np.int32)), up(rng.integers(16, 64, n_pts).astype(np.int32)),
           up(rng.integers(64, 112, n_pts).astype(np.int32)), up(rng.random((n_pts, 15), dtype=np.float32)))
    outs = (i32(2 * N), i32(2 * N, 2), i32(2 * N), i32(2 * N), torch.empty((2 * N, 15), device=DEV), torch.empty((N,), device=DEV))
    for e in range(args.reps):
        ops.pair_epoch_draw(*ins, 0, e, 120, *outs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for e in range(args.reps):
        ops.pair_epoch_draw(*ins, 0, e, 120, *outs)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.reps
    written = N * (2 * (4 + 8 + 4 + 4 + 60) + 4)
    print(json.dumps({"tool": "mb_train_smt", "what": "dm_pair_epoch_draw", "pairs": N, "host_timed_ms_per_launch": round(dt * 1e3, 4),
                      "bytes_written": written}))


def run_train(args):
    rng = np.random.default_rng(0)
    scales, bands, B = [32, 64, 128, 256], 4, 120
    N = args.steps_per_epoch * B - B // 2                    # ~20 steps per epoch, the last one partial
    ds = PairDataset.from_arrays(synthetic_images(6, bands, 1024, N, rng), seed=0, n_scales=4)
    N = len(ds)
    torch.manual_seed(0)
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=list(scales), depth=[6, 4, 2], in_c=bands, numerics="bf16")
    stamps = []
    draw = ds.epoch

    def stamped(e, batch):
        stamps.append(time.perf_counter())                 # the previous epoch ended with its loss read (a sync)
        return draw(e, batch)
    ds.epoch = stamped
    _, losses = Train_SMT.train(net, 1.0, B, 1e-4, 0.0, 0.0, 0.1, 0, dataset=ds, num_epochs=args.epochs, model_paras_path="unused")
    torch.cuda.synchronize()
    stamps.append(time.perf_counter())
    per_epoch = [b - a for a, b in zip(stamps[:-1], stamps[1:])]
    steady = per_epoch[1:]
    print(json.dumps({"tool": "mb_train_smt", "what": "train", "pairs_per_epoch": N, "train_bs": B, "steps_per_epoch": -(-N // B),
                      "epochs": args.epochs, "loss_curve": [round(x, 5) for x in losses], "epoch_s": [round(x, 4) for x in per_epoch],
                      "pairs_per_s_steady": round(len(steady) * N / sum(steady), 1) if steady else None,
                      "steady_note": "epochs after the first (the first holds the eager warm-up step and the hipGraph capture)"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["draw", "train"])
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--steps-per-epoch", type=int, default=20)
    args = ap.parse_args()
    run_draw(args) if args.what == "draw" else run_train(args)


if __name__ == "__main__":
    main()
