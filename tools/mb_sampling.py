#!/usr/bin/env python3
"""What weighted pair sampling costs.  Nothing of it is on the per-step path: a sampled epoch adds one torch.cumsum, one
dm_pair_epoch_select and one readback per EPOCH, and a mining refresh one eval pass over the training pairs every `every` epochs.

  kernels   N = M = 10^6 pairs / draws, batch 32, in one process, alternating: torch.cumsum (int64), dm_pair_epoch_select,
            dm_pair_epoch_draw_src, dm_pair_epoch_draw, and the orientation / radiometric columns in both key rules.  Call times from
            device events around each call (a launch each; cumsum is torch's own kernels).
  parent    with --parent-root DIR (a built checkout of the parent commit): dm_pair_epoch_draw / _orient / _radiometric at the same size
            from this tree and from that one, three alternating child processes each -- the templating of the kernels must cost nothing.
  train     tools/train_synth.py steady pairs/s without / with --balance 0.5, alternating child processes (and, with --parent-root, the
            parent's tool without the flag).
  mining    one refresh -- the eval pass over a pool of one epoch's pairs (tools/train_synth.py's pool_terms at the headline model:
            depth 6,4,2, 120 pairs per forward) -- against the same number of training steps.

  python tools/mb_sampling.py [--pairs 1000000] [--reps 20] [--train-rounds 2] [--parent-root DIR] [--skip train,mining] [--out profiles/sampling_mb.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, BANDS = 32, 4


def draw_inputs(torch, N, dev):
    """A synthetic pair list at N pairs: polygons of 1 .. 9 points, every point in one polygon (tools/mb_train_smt.py's shape)."""
    g = torch.Generator(device=dev); g.manual_seed(0)
    n_poly = max(4, N // 3)
    counts = torch.randint(1, 10, (n_poly,), generator=g, device=dev)
    poly_off = torch.cat((torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0))).to(torch.int32)
    n_pts = int(poly_off[-1])
    i32 = lambda t: t.to(torch.int32).contiguous()
    ins = [i32(torch.randint(0, n_poly, (N, 2), generator=g, device=dev)), i32(torch.randint(0, 2, (N,), generator=g, device=dev)), poly_off,
           i32(torch.randperm(n_pts, generator=g, device=dev)), i32(torch.randint(0, 6, (n_pts,), generator=g, device=dev)),
           i32(torch.randint(0, 4000, (n_pts, 2), generator=g, device=dev)), i32(torch.randint(1, 50, (n_pts,), generator=g, device=dev)),
           i32(torch.randint(50, 100, (n_pts,), generator=g, device=dev)), torch.rand((n_pts, 15), generator=g, device=dev)]
    e32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    outs = [e32(2 * N), e32(2 * N, 2), e32(2 * N), e32(2 * N), torch.empty((2 * N, 15), device=dev), torch.empty((N,), device=dev)]
    return ins, outs


def timed(torch, calls, reps, warm=3):
    """{name: [ms per repetition]}: the calls alternate, order rotated per repetition; device events around each call."""
    names = list(calls)
    times = {k: [] for k in names}
    for rep in range(warm + reps):
        k0 = rep % len(names)
        for name in names[k0:] + names[:k0]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            calls[name]()
            b.record()
            b.synchronize()
            if rep >= warm:
                times[name].append(a.elapsed_time(b))
    return times


def worker_kernels(root, N, reps, existing_only):
    """One process: the epoch calls at N pairs from the tree at `root`; prints one JSON line {name: [ms]}."""
    sys.path.insert(0, root)
    import torch
    from deepmerge_amd import ops
    dev = "cuda:0"
    ins, outs = draw_inputs(torch, N, dev)
    orient = torch.empty((2 * N,), dtype=torch.int32, device=dev)
    radio = torch.empty((2 * N, BANDS, 2), dtype=torch.int32, device=dev)
    spans = ops.Radiometric().spans()
    calls = {"dm_pair_epoch_draw": lambda: ops.pair_epoch_draw(*ins, 0, 1, BATCH, *outs),
             "dm_pair_epoch_orient": lambda: ops.pair_epoch_orient(0, 1, N, BATCH, 7, orient),
             "dm_pair_epoch_radiometric": lambda: ops.pair_epoch_radiometric(0, 1, N, BATCH, BANDS, *spans, radio)}
    if not existing_only:
        g = torch.Generator(device=dev); g.manual_seed(1)
        weights = torch.randint(1, 1 << 20, (N,), generator=g, device=dev)
        cum = torch.cumsum(weights, 0)
        src = torch.empty((N,), dtype=torch.int32, device=dev)
        ops.pair_epoch_select(cum, 0, 1, src)
        calls.update({"torch.cumsum (int64)": lambda: torch.cumsum(weights, 0),
                      "dm_pair_epoch_select": lambda: ops.pair_epoch_select(cum, 0, 1, src),
                      "dm_pair_epoch_draw_src": lambda: ops.pair_epoch_draw(*ins, 0, 1, BATCH, *outs, src=src),
                      "dm_pair_epoch_orient_src": lambda: ops.pair_epoch_orient(0, 1, N, BATCH, 7, orient, by_position=True),
                      "dm_pair_epoch_radiometric_src": lambda: ops.pair_epoch_radiometric(0, 1, N, BATCH, BANDS, *spans, radio, by_position=True)})
    print(json.dumps(timed(torch, calls, reps)), flush=True)


def worker_mining(steps, pairs):
    """One process: a refresh over a pool of steps x pairs pairs against `steps` training steps at the headline model."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch
    import train_synth as TS
    from deepmerge_amd.feed import PairFeed
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    from deepmerge_amd.trainer import PairTrainer
    scales, bands = [32, 64, 128, 256], 4
    g = torch.Generator(device=TS.DEV); g.manual_seed(0)
    torch.manual_seed(0)
    tiles = TS.smooth_tiles(6, bands, 1024, g)
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=scales, depth=[6, 4, 2], in_c=bands, numerics="bf16").to(TS.DEV)
    tr = PairTrainer(net, margin=1.0, lr=1e-4)
    tr.enable_graph(warmup=1)
    feed = PairFeed(tiles, scales, pairs, TS.MAX_WINDOW, numerics="bf16", trainer=tr)
    eval_feed = PairFeed(tiles, scales, pairs, TS.MAX_WINDOW, numerics="bf16")
    pool = TS.draw_pairs(6, 1024, steps * pairs, g)

    def epoch():
        for k in range(steps):
            tr.step(*feed.fill(TS.pair_table(tuple(t[k * pairs:(k + 1) * pairs] for t in pool))), lr=1e-4)

    def clock(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    epoch(); TS.pool_terms(net, eval_feed, pool, pairs)                    # warm-up: capture, code objects
    out = {"epoch_s": [], "refresh_s": []}
    for _ in range(3):
        out["epoch_s"].append(clock(epoch))
        out["refresh_s"].append(clock(lambda: TS.pool_terms(net, eval_feed, pool, pairs)))
    print(json.dumps(out), flush=True)


def child(args, limit=600):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + args, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"mb_sampling: a child process ended with {r.returncode}; nothing more is started\n{' '.join(args)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    print("mb_sampling: done:", " ".join(args[-6:]), file=sys.stderr, flush=True)
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def table(times):
    w = max(len(k) for k in times)
    med = {k: statistics.median(v) for k, v in times.items()}
    base = med.get("dm_pair_epoch_draw")
    lines = [f"  {'call':{w}s}  median ms    min ms    max ms   x dm_pair_epoch_draw   spread ms (|median even reps - median odd reps|)"]
    for k, v in times.items():
        spread = abs(statistics.median(v[0::2]) - statistics.median(v[1::2])) if len(v) > 1 else 0.0
        lines.append(f"  {k:{w}s} {med[k]:10.4f} {min(v):9.4f} {max(v):9.4f}   {med[k] / base:18.3f}   {spread:8.4f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train-rounds", type=int, default=2)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit, for the A/B of the existing entry points")
    ap.add_argument("--skip", default="", help="comma-separated: kernels, parent, train, mining")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_mb.txt"))
    ap.add_argument("--worker", default=None, choices=["kernels", "existing", "mining"])
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.worker in ("kernels", "existing"):
        return worker_kernels(a.root, a.pairs, a.reps, a.worker == "existing")
    if a.worker == "mining":
        return worker_mining(20, 120)
    skip = set(filter(None, a.skip.split(",")))
    me = os.path.abspath(__file__)
    lines = ["Weighted pair sampling (tools/mb_sampling.py), one MI355X, one session", ""]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if "kernels" not in skip:
        t = child([me, "--worker", "kernels", "--pairs", str(a.pairs), "--reps", str(a.reps)])
        lines += [f"per-epoch calls at N = M = {a.pairs} pairs / draws, batch {BATCH}, {BANDS} bands, one process, {a.reps} repetitions after 3 warm-up, "
                  "the calls alternating (order rotated per repetition); device events around each call"] + table(t) + [""]
        flush()
    if a.parent_root and "parent" not in skip:
        runs = {"this tree": [], "parent": []}
        for _ in range(3):
            for k, root in (("this tree", ROOT), ("parent", os.path.abspath(a.parent_root))):
                runs[k].append(child([me, "--worker", "existing", "--pairs", str(a.pairs), "--reps", str(a.reps), "--root", root]))
        lines += [f"the existing entry points at N = {a.pairs}, batch {BATCH}: this tree against the parent commit's build, three alternating processes "
                  f"each, median ms of {a.reps} repetitions per process"]
        for name in runs["this tree"][0]:
            row = {k: [round(statistics.median(r[name]), 4) for r in v] for k, v in runs.items()}
            lines.append(f"  {name:26s} this tree {row['this tree']}   parent {row['parent']}")
        lines.append("")
        flush()
    if "train" not in skip:
        variants = {"without": (ROOT, []), "--balance 0.5": (ROOT, ["--balance", "0.5"])}
        if a.parent_root:
            variants["parent commit, without"] = (os.path.abspath(a.parent_root), [])
        rates = {k: [] for k in variants}
        for _ in range(a.train_rounds):
            for k, (root, extra) in variants.items():
                res = child([os.path.join(root, "tools", "train_synth.py"), "--epochs", "2", "--steps-per-epoch", "20"] + extra)
                rates[k].append(res["pairs_per_s_steady_incl_data_generation"])
        w = max(len(k) for k in variants)
        lines += ["tools/train_synth.py --epochs 2 --steps-per-epoch 20 (120 pairs per step, depth 6,4,2, bf16), steady pairs/s incl. data generation, "
                  f"{a.train_rounds} runs each, alternating (with --balance each step indexes a fixed pool instead of drawing fresh pairs):"]
        lines += [f"  {k:{w}s} : {v}" for k, v in rates.items()] + [""]
        flush()
    if "mining" not in skip:
        m = child([me, "--worker", "mining"])
        e, r = statistics.median(m["epoch_s"]), statistics.median(m["refresh_s"])
        lines += ["one mining refresh (eval forward + dm_contrastive_terms over 20 x 120 pairs, depth 6,4,2, bf16) against a training epoch of the same "
                  "20 x 120 pairs (hipGraph replays), host clock around synchronised work, 3 runs each, alternating:",
                  f"  epoch s {[round(x, 4) for x in m['epoch_s']]}   refresh s {[round(x, 4) for x in m['refresh_s']]}   refresh / epoch = {r / e:.3f}", ""]
        flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
