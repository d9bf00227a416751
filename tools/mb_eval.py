#!/usr/bin/env python3
"""Held-out pair validation throughput (evaluate.PairEvaluator) and the summary reduction.

  python tools/mb_eval.py eval [--epochs 3]     at the BASELINE configs[4] shape (v3 [6,4,2], scales [32,64,128,256] x 4 bands,
                                                bf16) on mb_train_smt's synthetic images: evaluation pairs/s at val_batch 1000 and
                                                120, then train() epoch time (train_bs 120) without and with a validation set of
                                                the same size; one JSON line each
  python tools/mb_eval.py summary [--pairs 1000000] [--thresholds 1024]
                                                dm_pair_eval_summary alone (time it with rocprofv3 --kernel-trace --stats)
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from deepmerge_amd import Train_SMT, ops  # noqa: E402
from deepmerge_amd.dataset import PairDataset  # noqa: E402
from deepmerge_amd.evaluate import PairEvaluator  # noqa: E402
from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3  # noqa: E402
from mb_train_smt import synthetic_images  # noqa: E402

DEV = "cuda:0"
SCALES, BANDS, TRAIN_BS = [32, 64, 128, 256], 4, 120


def _net():
    torch.manual_seed(0)
    return ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=list(SCALES), depth=[6, 4, 2], in_c=BANDS, numerics="bf16").to(DEV)


def _datasets(steps_per_epoch):
    N = steps_per_epoch * TRAIN_BS - TRAIN_BS // 2                 # as mb_train_smt: ~20 steps per epoch, the last one partial
    train = PairDataset.from_arrays(synthetic_images(6, BANDS, 1024, N, np.random.default_rng(0)), seed=0, n_scales=4)
    val = PairDataset.from_arrays(synthetic_images(6, BANDS, 1024, N, np.random.default_rng(1)), seed=1, n_scales=4)
    return train, val


def _train_epochs(net, ds, epochs, **kw):
    """train()'s per-epoch wall times, stamped at each epoch's draw (the previous epoch ended with its loss read, a sync)."""
    stamps, draw = [], ds.epoch

    def stamped(e, batch):
        stamps.append(time.perf_counter())
        return draw(e, batch)
    ds.epoch = stamped
    try:
        _, losses = Train_SMT.train(net, 1.0, TRAIN_BS, 1e-4, 0.0, 0.0, 0.1, 0, dataset=ds, num_epochs=epochs, model_paras_path="unused", **kw)
    finally:
        ds.epoch = draw
    torch.cuda.synchronize()
    stamps.append(time.perf_counter())
    return [b - a for a, b in zip(stamps[:-1], stamps[1:])], losses


def run_eval(args):
    train, val = _datasets(args.steps_per_epoch)
    N = len(val)
    net = _net()
    for vb in (1000, 120):
        ev = PairEvaluator(net, val, batch=vb, margin=1.0)
        ev.run()                                                    # warm-up (code objects, allocator)
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = ev.run()                                            # ends with the host read of the result block (a sync)
            times.append(time.perf_counter() - t0)
        print(json.dumps({"tool": "mb_eval", "what": "evaluate", "pairs": N, "val_batch": vb, "run_s": [round(t, 4) for t in times],
                          "pairs_per_s": round(N / float(np.median(times)), 1), "val_loss": round(r.loss, 6), "f_at_margin": round(r.f_score, 4)}),
              flush=True)
    for label, kw in (("train", {}), ("train+val", {"val_dataset": val, "val_batch": 1000})):
        per_epoch, losses = _train_epochs(_net(), train, args.epochs, **kw)
        steady = per_epoch[1:]
        print(json.dumps({"tool": "mb_eval", "what": label, "pairs_per_epoch": len(train), "val_pairs": N if kw else 0, "train_bs": TRAIN_BS,
                          "epochs": args.epochs, "loss_curve": [round(x, 5) for x in losses], "epoch_s": [round(x, 4) for x in per_epoch],
                          "steady_epoch_s": round(float(np.mean(steady)), 4) if steady else None}), flush=True)


def run_summary(args):
    rng = np.random.default_rng(0)
    N, T = args.pairs, args.thresholds
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    term, simi = up(rng.exponential(1.0, N).astype(np.float32)), up(rng.uniform(0, 2, N).astype(np.float32))
    flag = up((rng.random(N) < 0.5).astype(np.float32))
    th = up(np.linspace(2.0 / T, 2.0, T).astype(np.float32))
    out = torch.empty(2 * T + 2, dtype=torch.int64, device=DEV)
    for _ in range(3):
        ops.pair_eval_summary(term, simi, flag, th, validate=False, out=out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        ops.pair_eval_summary(term, simi, flag, th, validate=False, out=out)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.reps
    print(json.dumps({"tool": "mb_eval", "what": "dm_pair_eval_summary", "pairs": N, "thresholds": T,
                      "host_timed_ms_per_call": round(dt * 1e3, 4), "bytes_read": 12 * N}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["eval", "summary"])
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--thresholds", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--steps-per-epoch", type=int, default=20)
    args = ap.parse_args()
    if args.what == "eval":
        args.reps = min(args.reps, 5)
        run_eval(args)
    else:
        run_summary(args)


if __name__ == "__main__":
    main()
