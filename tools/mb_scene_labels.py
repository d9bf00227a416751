#!/usr/bin/env python3
"""Cost of scene.segment_labels beside scene.segment_scene on the scene of tools/mb_scene.py: a synthetic 8192 x 8192 x 3 uint8 scene
in an np.memmap on disk, four tiles of 4096, rag.slic cell 29, k = 3, the reference's encoder depth [6, 4, 2] in bf16, batch 2000.

  python tools/mb_scene_labels.py [--out profiles/scene_labels_mb.txt] [--size 8192] [--tile 4096] [--k 3]

`segment_scene` runs with SLIC and keeps its assembled raster; `segment_labels` then runs on that raster in the same session, so
both build the same graph and the same points (checked).  Wall time per stage with a device synchronisation at every stage
boundary, after a warm-up of both on a small scene and one unreported pass of both over the scene itself.  The one thing to read off: what the label-raster path pays for not knowing
which tile owns a superpixel -- the compaction (`torch.unique` per core), the fold, and the k passes over the label raster of
the points -- as the ratio of its graph + points stages to the "graph" stage of `segment_scene` (which holds the per-tile
statistics, edges and points).  No target time is set: the feature has no parent to compare with.
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from deepmerge_amd import rag, scene  # noqa: E402
from deepmerge_amd.ExtractFeatures import FeatureIO  # noqa: E402
from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3  # noqa: E402
from mb_slic import block_noise_tile  # noqa: E402

OLD = ("read + copy", "segment", "graph", "stitch", "encode", "merge", "write")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_labels_mb.txt"))
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--k", type=int, default=3)
    a = ap.parse_args()
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=[32, 64, 128], in_c=3, numerics="bf16")
    fio = FeatureIO(net, None, "cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        img = np.memmap(os.path.join(tmp, "scene.u8"), dtype=np.uint8, mode="w+", shape=(3, a.size, a.size))
        for i, (y0, y1, x0, x1) in enumerate(scene.tile_grid(a.size, a.size, a.tile)):
            img[:, y0:y1, x0:x1] = block_noise_tile(3, y1 - y0, x1 - x0, seed=i).cpu().numpy()
        img.flush()
        labels_out = np.memmap(os.path.join(tmp, "labels.i32"), dtype=np.int32, mode="w+", shape=(a.size, a.size))
        small = np.ascontiguousarray(img[:, :512, :512])
        warm = fio.segment_scene(small, tile=256, k=a.k)          # warm-up: allocator and code objects, of both paths
        fio.segment_scene(small, tile=256, k=a.k, labels=warm.labels, n_labels=warm.n_labels)
        for _ in range(2):                                        # the second pass is the one reported: tables of the scene's size exist
            old_t, new_t = {}, {}
            old = fio.segment_scene(img, tile=a.tile, k=a.k, labels_out=labels_out, stage_times=old_t)
            labels_out.flush()
            new = fio.segment_scene(img, tile=a.tile, k=a.k, labels=labels_out, n_labels=old.n_labels, stage_times=new_t)
            torch.cuda.synchronize()
    same = (torch.equal(new.edges, old.edges) and torch.equal(new.weights, old.weights) and torch.equal(new.points.xy, old.points.xy)
            and all(torch.equal(new.stats[key], old.stats[key]) for key in rag._STAT_KEYS) and torch.equal(new.result.region_of, old.result.region_of))
    rounds = [f"points round {j}" for j in range(a.k)]
    new_stages = ["read + copy", "compact", "graph"] + rounds + ["points emit", "stitch", "encode", "merge"]
    old_total, new_total = sum(old_t.values()), sum(new_t.values())
    graph_points = sum(new_t.get(s, 0.0) for s in ["compact", "graph", "points emit"] + rounds)
    reads = 1 + a.k + 1                                            # graph, k point rounds (labels only), encode (image only)
    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"scene (3, {a.size}, {a.size}) uint8 in an np.memmap, {len(old.tiles)} tiles of {a.tile}, halo {scene.halo_of(rag.MAX_WINDOW)}; "
             f"rag.slic cell 29, k = {a.k}, encoder depth [6, 4, 2] bf16, batch 2000",
             f"superpixels {old.n_labels}, sample points {old.points.xy.shape[0]}, edges {old.edges.shape[0]}; the two calls agree in "
             f"statistics, edges, weights, points and the merge: {same}",
             "segment_scene (SLIC per tile), wall time per stage, all tiles (synchronised at every stage boundary):"]
    lines += [f"    {s:40s} {old_t.get(s, 0.0) * 1e3:11.3f} ms  {100.0 * old_t.get(s, 0.0) / old_total:5.1f} %" for s in OLD]
    lines += [f"    {'total':40s} {old_total * 1e3:11.3f} ms",
              "segment_labels on the raster that call assembled (an np.memmap on disk), same session:"]
    lines += [f"    {s:40s} {new_t.get(s, 0.0) * 1e3:11.3f} ms  {100.0 * new_t.get(s, 0.0) / new_total:5.1f} %" for s in new_stages]
    lines += [f"    {'total':40s} {new_total * 1e3:11.3f} ms",
              f"read + copy covers {reads} streams: image and labels for the graph, the labels' halo windows for each of the {a.k} point "
              f"rounds, the image's halo windows for the encode",
              f"compact + graph + points of segment_labels: {graph_points * 1e3:.3f} ms = {graph_points / old_t['graph']:.2f} x the graph stage "
              f"of segment_scene ({old_t['graph'] * 1e3:.3f} ms); compact (torch.unique per core) alone: {new_t.get('compact', 0.0) * 1e3:.3f} ms; "
              f"the {a.k} point rounds (clearance + select per window, commit): {sum(new_t.get(s, 0.0) for s in rounds) * 1e3:.3f} ms",
              f"whole call: segment_labels / (segment_scene without segment and write) = "
              f"{new_total / (old_total - old_t.get('segment', 0.0) - old_t.get('write', 0.0)):.3f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
