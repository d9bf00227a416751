#!/usr/bin/env python3
"""Cost of rag.mrs from both of its starts, on the piecewise-constant tile with noise that tools/mb_slic.py makes: the SLIC
superpixels (cell 29, ~20 k labels) of a 4096 x 4096 x 4 uint8 tile, and the single pixels of a 1024 x 1024 crop of it (1 M regions,
2 M edges in round 1).

  python tools/mb_mrs.py [--out profiles/mrs_mb.txt] [--size 4096] [--pixel-size 1024] [--scale 100] [--pixel-scale 30]

hipEvent time of the stages in front of the loop (each a whole call: allocations and readbacks included), of the whole rag.mrs call,
of its first round alone (max_rounds=1: the round at full size, where the two folds' single-workgroup scans are longest) and hence
per round; rounds and regions per round.  Beside them, for orientation only, rag.merge_regions per round on the same graph in the
same process, scored on the regions' mean colours through one sample point per region.  No target time is set.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from deepmerge_amd import rag  # noqa: E402
from deepmerge_amd.workload import ev  # noqa: E402
from mb_slic import block_noise_tile  # noqa: E402


def learned_rounds(stats, edges, weights, max_rounds):
    """(seconds per scoring round, rounds) of merge_regions on the mean colours / 8 of the same regions, one point per region."""
    S = stats["count"].numel()
    feats = (stats["sum"].double() / stats["count"].double().unsqueeze(1) / 8.0).float().contiguous()
    ids = torch.arange(S + 1, dtype=torch.int32, device=edges.device)
    run = lambda: rag.merge_regions(feats, ids, ids[:-1].contiguous(), edges, margin=1.0, weights=weights, stats=stats, max_rounds=max_rounds)
    res = run()
    return ev(run, 3) / (res.rounds + 1), res


def report(name, tile, scale, start, stages, iters, learned_max_rounds):
    """start() -> (stats, edges, weights, mrs keyword arguments); stages: [(label, callable)] timed one by one."""
    stats, edges, weights, kw = start()
    run = lambda **more: rag.mrs(tile, scale, **kw, **more)
    res = run()                                                    # warm-up: allocator and code objects
    lines = [f"{name}: tile {tuple(tile.shape)} uint8, S0 = {stats['count'].numel()} regions, E = {edges.shape[0]} edges; "
             f"scale {scale}, shape 0.1, compactness 0.5"]
    lines += [f"    {label:56s} {ev(fn, iters) * 1e3:9.3f} ms" for label, fn in stages]
    t_cost = ev(lambda: rag.region_merge_cost(stats, edges, weights), iters)
    t_all, t_first = ev(run, iters), ev(lambda: run(max_rounds=1), iters)
    lines += [f"    {'rag.region_merge_cost on the start graph':56s} {t_cost * 1e3:9.3f} ms",
              f"    {'rag.mrs, whole call (its start included)':56s} {t_all * 1e3:9.3f} ms",
              f"    {'rag.mrs(max_rounds=1): start + round 1 + final scoring':56s} {t_first * 1e3:9.3f} ms",
              f"    rounds applied: {res.rounds}; whole call / (rounds + 1) = {t_all / (res.rounds + 1) * 1e3:.3f} ms per scoring round",
              f"    regions per round: {res.regions_per_round}"]
    t_learned, lres = learned_rounds(stats, edges, weights, learned_max_rounds)
    lines.append(f"    for orientation, rag.merge_regions on the same graph (mean colours / 8, margin 1, max_rounds={learned_max_rounds}): "
                 f"{t_learned * 1e3:.3f} ms per scoring round over {lres.rounds} rounds, regions {lres.regions_per_round[0]} -> {lres.regions_per_round[-1]}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mrs_mb.txt"))
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--pixel-size", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=100.0)
    ap.add_argument("--pixel-scale", type=float, default=30.0)
    a = ap.parse_args()
    tile = block_noise_tile(4, a.size, a.size)
    labels, S = rag.slic(tile, cell=29, compactness=10, iters=10)
    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}"]

    def slic_start():
        return rag.label_stats(labels, tile, S), *rag.rag_edges(labels, S), {"labels": labels, "n_labels": S}

    lines += report("SLIC start (rag.slic, cell 29)", tile, a.scale, slic_start,
                    [("rag.slic (not part of rag.mrs)", lambda: rag.slic(tile, cell=29, compactness=10, iters=10)),
                     ("rag.label_stats", lambda: rag.label_stats(labels, tile, S)),
                     ("rag.rag_edges", lambda: rag.rag_edges(labels, S))], 5, None)
    crop = tile[:, :a.pixel_size, :a.pixel_size].contiguous()
    del tile, labels

    def pixel_start():
        return *rag.pixel_regions(crop), {}

    arange = torch.arange(a.pixel_size * a.pixel_size, dtype=torch.int32, device=crop.device).view(a.pixel_size, a.pixel_size)
    lines += report("pixel start", crop, a.pixel_scale, pixel_start,
                    [("rag.pixel_regions", lambda: rag.pixel_regions(crop)),
                     ("what it replaces: rag.label_stats of the arange raster", lambda: rag.label_stats(arange, crop, arange.numel())),
                     ("what it replaces: rag.rag_edges of the arange raster", lambda: rag.rag_edges(arange, arange.numel()))], 3, 8)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
