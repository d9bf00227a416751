#!/usr/bin/env python3
"""Train_SMT counterpart on synthetic data (Train_SMT.py:212-351): epochs of steps, MultiStepLR([40, 80], 0.2) stepped per
epoch, FRESH pairs every step generated on the device -- patch pyramids cut from resident uint8 tiles by the sync-free feed
(deepmerge_amd/feed.py: one dm_pair_batch_gather launch per scale straight into the captured step's inputs), positives = two
jittered windows of the same spot, negatives = spots of different tiles -- through PairTrainer (hipGraph replay).  Prints a loss curve; BASELINE configs[4] shape by default (depth [6,4,2], 4 scales x 4 ch,
120 pairs per GPU).        python tools/train_synth.py [--epochs 3] [--steps-per-epoch 20] [--pairs 120] [--depth 6,4,2] [--augment d4] [--radiometric 0.2,0.1,0.05]
--balance P / --mining EVERY[,CAP]: instead of fresh pairs every step, a fixed pool of steps-per-epoch x pairs pairs is drawn once and
every epoch samples it with replacement by integer weights (dataset.balance_weights / hardness_weights, one
ops.pair_epoch_select launch per epoch); each step gathers its rows of the pool by index.  Mining evaluates the pool's loss terms with
the model as it stands at the first epoch and every EVERY-th.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmerge_amd import ops  # noqa: E402
from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3  # noqa: E402
from deepmerge_amd.dataset import balance_weights, hardness_weights  # noqa: E402
from deepmerge_amd.feed import PairFeed, PairTable  # noqa: E402
from deepmerge_amd.patches import point_batch  # noqa: E402
from deepmerge_amd.trainer import PairTrainer, multistep_lr  # noqa: E402

DEV = "cuda:0"


def smooth_tiles(n, bands, size, g):
    """Spatially correlated uint8 tiles (so that two nearby windows look alike and two tiles do not)."""
    low = torch.rand((n, bands, size // 32, size // 32), generator=g, device=DEV)
    t = torch.nn.functional.interpolate(low, size=(size, size), mode="bilinear", align_corners=False)
    t = t + 0.08 * torch.rand((n, bands, size, size), generator=g, device=DEV)
    return (t.clamp(0, 1) * 255).to(torch.uint8)


def draw_pairs(n_tiles, size, B, g):
    """The sample table of one batch, drawn on the device (same draws, in the same order, as the per-tile loop of rounds 1-4 --
    `make_pairs_looped` below -- so the two feeds see identical data)."""
    flag = (torch.arange(B, device=DEV) % 2 == 0).to(torch.int64)
    tl = torch.randint(0, n_tiles, (B,), generator=g, device=DEV)
    tr = torch.where(flag == 1, tl, (tl + 1 + torch.randint(0, n_tiles - 1, (B,), generator=g, device=DEV)) % n_tiles)
    xy_l = torch.randint(96, size - 96, (B, 2), generator=g, device=DEV)
    xy_r = torch.where(flag[:, None] == 1, xy_l + torch.randint(-6, 7, (B, 2), generator=g, device=DEV),
                       torch.randint(96, size - 96, (B, 2), generator=g, device=DEV))
    inner = torch.randint(16, 65, (B,), generator=g, device=DEV)
    obj = inner + torch.randint(8, 49, (B,), generator=g, device=DEV)
    feats_l = torch.exp(torch.empty((B, 15), device=DEV).uniform_(-2.0, 3.0, generator=g))
    feats_r = torch.where(flag[:, None] == 1, feats_l * 1.05, torch.exp(torch.empty((B, 15), device=DEV).uniform_(-2.0, 3.0, generator=g)))
    return tl, tr, xy_l, xy_r, inner, obj, feats_l, feats_r, flag


def pair_table(draw, orient=None, radio=None):
    """deepmerge_amd.feed.PairTable of a draw: [left rows; right rows], int32 columns -- device ops only, nothing read back.
    orient: int32 [B] dihedral orientations, one per pair (both sides get it), or None.  radio: int32 [2B, bands, 2] or None."""
    tl, tr, xy_l, xy_r, inner, obj, feats_l, feats_r, flag = draw
    i32 = lambda a, b: torch.cat((a, b), 0).to(torch.int32)
    return PairTable(tile_id=i32(tl, tr), xy=i32(xy_l, xy_r), inner=i32(inner, inner), obj=i32(obj, obj),
                     region=torch.cat((feats_l, feats_r), 0), flag=flag, orient=None if orient is None else i32(orient, orient), radio=radio)


def draw_orient(B, augment, g):
    """One orientation per pair from a generator of its own, so that the data stream is the same with and without --augment."""
    return torch.randint(0, {"flips": 4, "d4": 8}[augment], (B,), generator=g, device=DEV)


def draw_radio(B, bands, radiometric, step, out):
    """One (gain, offset) table per pair of step `step`, on both of its rows (ops.pair_epoch_radiometric with the step as the epoch:
    one step is one block of the blocked layout, [left B; right B]); a stream of its own, like the orientations."""
    ops.pair_epoch_radiometric(1, step, B, B, bands, *radiometric.spans(), out)
    return out


def pool_terms(net, feed, pool, B, margin=1.0):
    """fp32 [len(pool)]: the contrastive term of every pair of the pool in pool order, B pairs per eval forward (a feed of its own)."""
    n = pool[-1].shape[0]
    term, d2 = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    was_training = net.training
    net.eval()
    with torch.no_grad():
        for lo in range(0, n, B):
            _, _, _, _, flag = feed.fill(pair_table(tuple(t[lo:lo + B] for t in pool)))
            F = net(feed.both, feed.dboth).contiguous()
            ops.contrastive_terms(F[:B], F[B:], flag, margin, d2=d2[lo:lo + B], term=term[lo:lo + B])
    net.train(was_training)
    return term


MAX_WINDOW = [64, 112, 160, 208]       # bounds of (inner, obj, obj + interval, obj + 2 interval) for the ranges drawn above


def make_pairs_looped(tiles, B, scales, g):
    """The feed of rounds 1-4 (`--feed looped`, kept for the A/B and the bit-for-bit test): one gather launch per (tile, scale), tile
    membership by `nonzero`, window sides through the host."""
    n, bands, size, _ = tiles.shape
    tl, tr, xy_l, xy_r, inner, obj, feats_l, feats_r, flag = draw_pairs(n, size, B, g)

    def side(tid, xy, feats):
        patches = [torch.empty((B, bands, s, s), device=DEV) for s in scales]
        designed = torch.empty((B, 1, 19), device=DEV)
        for t in range(n):                                  # one gather launch per (tile, scale)
            sel = torch.nonzero(tid == t).reshape(-1)
            if sel.numel() == 0:
                continue
            p, d = point_batch(tiles[t], xy[sel].to(torch.int32), inner[sel].cpu(), obj[sel].cpu(), feats[sel], scales=scales)
            for i in range(len(scales)):
                patches[i][sel] = p[i]
            designed[sel] = d
        return patches, designed
    pl, dl = side(tl, xy_l, feats_l)
    pr, dr = side(tr, xy_r, feats_r)
    return pl, dl, pr, dr, flag


def main():  # noqa: C901
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--steps-per-epoch", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=120)
    ap.add_argument("--depth", type=str, default="6,4,2")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--numerics", type=str, default="bf16", choices=["bf16", "fp32", "bf16x3"])
    ap.add_argument("--milestones", type=str, default="40,80")
    ap.add_argument("--feed", type=str, default="rows", choices=["rows", "patches", "looped"],
                    help="rows: deepmerge_amd.feed.PairFeed writing the patch-embed operand rows (default); patches: the same feed writing "
                         "fp32 patch tensors; looped: the per-tile Python loop of rounds 1-4")
    ap.add_argument("--augment", type=str, default=None, choices=["flips", "d4"],
                    help="feed every pair at a random dihedral orientation (both sides alike; rows / patches feeds only)")
    ap.add_argument("--radiometric", type=str, default=None, metavar="C,B,K",
                    help="feed every pair under a random gain / offset per band: contrast, brightness, colour half widths, e.g. 0.2,0.1,0.05 "
                         "(both sides alike; rows / patches feeds only)")
    ap.add_argument("--balance", type=float, default=None, metavar="P",
                    help="sample a fixed pool of pairs with replacement so that a share P of what the model sees is positive pairs")
    ap.add_argument("--mining", type=str, default=None, metavar="EVERY[,CAP]",
                    help="sample the pool by loss-driven weights refreshed every EVERY epochs, saturating at a term of CAP (default 1.0)")
    ap.add_argument("--loss-every", type=int, default=0, help="read the loss back every k steps (0 = once per epoch)")
    args = ap.parse_args()
    sampled = args.balance is not None or args.mining is not None
    if sampled and args.feed == "looped":
        ap.error("--balance / --mining need the sync-free feed (--feed rows or patches)")
    try:
        mining = None
        if args.mining:
            every, _, cap = args.mining.partition(",")
            mining = ops.Mining(every=int(every), cap=float(cap) if cap else 1.0)
    except (TypeError, ValueError) as e:
        ap.error(f"--mining EVERY[,CAP]: {e}")
    if args.augment and args.feed == "looped":
        ap.error("--augment needs the sync-free feed (--feed rows or patches)")
    if args.radiometric and args.feed == "looped":
        ap.error("--radiometric needs the sync-free feed (--feed rows or patches)")
    try:
        radiometric = ops.Radiometric(*(float(v) for v in args.radiometric.split(","))) if args.radiometric else None
    except (TypeError, ValueError) as e:
        ap.error(f"--radiometric C,B,K: {e}")
    scales, bands = [32, 64, 128, 256], 4
    depth = [int(d) for d in args.depth.split(",")]
    ms = tuple(int(m) for m in args.milestones.split(","))
    g = torch.Generator(device=DEV); g.manual_seed(0)
    g_orient = torch.Generator(device=DEV); g_orient.manual_seed(1)
    torch.manual_seed(0)
    tiles = smooth_tiles(6, bands, 1024, g)
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=list(scales), depth=depth, in_c=bands, numerics=args.numerics).to(DEV)
    tr = PairTrainer(net, margin=1.0, lr=args.lr)
    tr.enable_graph(warmup=1)
    feed = None if args.feed == "looped" else PairFeed(tiles, scales, args.pairs, MAX_WINDOW, rows=args.feed == "rows", numerics=args.numerics, trainer=tr)
    radio_buf = torch.empty((2 * args.pairs, bands, 2), dtype=torch.int32, device=DEV) if radiometric else None
    pool = src = weights = class_w = eval_feed = None
    if sampled:                                              # the pool: one epoch's worth of pairs, drawn once
        n_pool = args.steps_per_epoch * args.pairs
        pool = draw_pairs(tiles.shape[0], tiles.shape[2], n_pool, g)
        src = torch.empty(n_pool, dtype=torch.int32, device=DEV)
        try:
            class_w = weights = balance_weights(pool[-1], args.balance) if args.balance is not None else None
        except ValueError as e:
            ap.error(f"--balance P: {e}")
        if mining is not None:
            if n_pool % args.pairs:
                ap.error("--mining evaluates the pool in batches of --pairs")
            eval_feed = PairFeed(tiles, scales, args.pairs, MAX_WINDOW, rows=args.feed == "rows", numerics=args.numerics)
    curve = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    WARM = 3                                                 # eager step(s) + the capturing step: not steady state (one extra sync after them)
    t_warm, done = None, 0
    for epoch in range(args.epochs):
        lr = multistep_lr(args.lr, epoch, ms)
        tot = torch.zeros((), device=DEV)
        if sampled:
            if mining is not None and epoch % mining.every == 0:
                weights = hardness_weights(pool_terms(net, eval_feed, pool, args.pairs), mining.floor_share, mining.cap, class_weights=class_w)
            ops.pair_epoch_select(torch.cumsum(weights, 0), 0, epoch, src)
        for k in range(args.steps_per_epoch):
            if done == WARM:
                torch.cuda.synchronize(); t_warm = time.perf_counter()
            done += 1
            if feed is None:
                batch = make_pairs_looped(tiles, args.pairs, scales, g)
            else:
                orient = draw_orient(args.pairs, args.augment, g_orient) if args.augment else None
                radio = draw_radio(args.pairs, bands, radiometric, done, radio_buf) if radiometric else None
                if sampled:
                    idx = src[k * args.pairs:(k + 1) * args.pairs].long()
                    draw = tuple(t[idx] for t in pool)
                else:
                    draw = draw_pairs(tiles.shape[0], tiles.shape[2], args.pairs, g)
                batch = feed.fill(pair_table(draw, orient, radio))
            tot += tr.step(*batch, lr=lr)                    # (device-side sum: the reference's per-step .item(), Train_SMT.py:301, is a sync)
            if args.loss_every and (k + 1) % args.loss_every == 0:
                float(tot)
        curve.append(round(float(tot) / args.steps_per_epoch, 5))
        if feed is not None:
            feed.check()
        print(f"epoch {epoch}: lr {lr:.2e} mean loss {curve[-1]:.5f}", flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = args.epochs * args.steps_per_epoch
    print(json.dumps({"tool": "train_synth", "feed": args.feed, "augment": args.augment, "radiometric": args.radiometric, "balance": args.balance, "mining": args.mining, "numerics": args.numerics, "depth": depth, "pairs_per_step": args.pairs, "steps": n,
                      "loss_curve": curve, "hip_graph": tr.graph_error is None, "pairs_per_s_incl_data_generation": round(n * args.pairs / dt, 1),
                      "pairs_per_s_steady_incl_data_generation": None if t_warm is None else round((n - WARM) * args.pairs / (t0 + dt - t_warm), 1),
                      "steady_note": f"after the first {WARM} steps (eager warm-up + hipGraph capture)"}))


if __name__ == "__main__":
    main()
