#!/usr/bin/env python3
"""Cost of scene.trace_labels beside rag._trace of the same raster, in one process: the 8192 x 8192 scene of tools/mb_scene.py (2^26
pixels, so that it also fits ONE rag._trace), segmented by the default pipeline, then its SLIC raster and its merged raster traced
twice each -- in four 4096 tiles across the seams, and whole.

  python tools/mb_scene_vector.py [--out profiles/scene_vector_mb.txt] [--size 8192] [--tile 4096]

Per stage, with a device synchronisation at every stage boundary of the tiled trace (its `stats`) and hipEvent times between the
stages of the one-raster trace (its `stats`); both after a warm-up on a small raster.  The two are checked to be bit-equal.  No target
time is set: the feature has no parent to compare with.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from deepmerge_amd import rag, scene  # noqa: E402
from deepmerge_amd.ExtractFeatures import FeatureIO  # noqa: E402
from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3  # noqa: E402
from mb_slic import block_noise_tile  # noqa: E402

STAGES = ("read + copy", "per-tile passes", "sort + join", "rounds", "emit")
WHOLE = {"count + scan + readback of D": "per-tile passes", "emit + link": "per-tile passes", "head rounds": "rounds", "rank rounds": "rounds",
         "ring tables (sort, scans) + ring_emit": "emit", "arc tables (two sorts, scan) + arc_emit": "emit"}


def both(name: str, raster: np.ndarray, n: int, tile: int):
    """One tiled and one whole trace of `raster`, timed per stage; returns the report's lines."""
    tiled_stats, whole_stats = {}, {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tiled = scene.trace_labels(raster, n, tile, stats=tiled_stats)
    torch.cuda.synchronize()
    t_tiled = time.perf_counter() - t0
    t0 = time.perf_counter()
    on_device = torch.from_numpy(np.ascontiguousarray(raster)).to("cuda:0")
    torch.cuda.synchronize()
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    whole = rag._trace(on_device, n, whole_stats)
    torch.cuda.synchronize()
    t_whole = time.perf_counter() - t0
    for f in ("region_ptr", "ring_ptr", "xy", "ring_label", "ring_area2"):
        assert torch.equal(getattr(tiled[0], f), getattr(whole[0], f)), f
    for f in ("arc_ptr", "xy", "left", "right"):
        assert torch.equal(getattr(tiled[1], f), getattr(whole[1], f)), f
    per = {s: 0.0 for s in STAGES}
    per["read + copy"] = t_copy
    for stage, ms in whole_stats["stage_ms"]:
        per[WHOLE[stage]] += ms * 1e-3
    s = tiled_stats
    lines = [f"{name}: {n} labels, {s['D']} darts, {s['rings']} rings, {s['vertices']} ring vertices, {s['arcs']} arcs, "
             f"{s['arc_vertices']} arc vertices; rounds head {s['head_rounds']} + rank {s['rank_rounds']} (whole: "
             f"{whole_stats['head_rounds']} + {whole_stats['rank_rounds']}); {s['tiles']} tiles; bit-equal: yes",
             f"    {'stage':24s} {'trace_labels':>14s} {'rag._trace':>14s}   ratio"]
    for stage in STAGES:
        a, b = s["stage_s"].get(stage, 0.0), per[stage]
        lines.append(f"    {stage:24s} {a * 1e3:11.3f} ms {b * 1e3:11.3f} ms   {a / b if b else float('nan'):5.2f}")
    lines.append(f"    {'total (wall)':24s} {t_tiled * 1e3:11.3f} ms {(t_copy + t_whole) * 1e3:11.3f} ms   {t_tiled / (t_copy + t_whole):5.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_vector_mb.txt"))
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--tile", type=int, default=4096)
    a = ap.parse_args()
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=[32, 64, 128], in_c=3, numerics="bf16")
    fio = FeatureIO(net, None, "cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        img = np.memmap(os.path.join(tmp, "scene.u8"), dtype=np.uint8, mode="w+", shape=(3, a.size, a.size))
        for i, (y0, y1, x0, x1) in enumerate(scene.tile_grid(a.size, a.size, a.tile)):
            img[:, y0:y1, x0:x1] = block_noise_tile(3, y1 - y0, x1 - x0, seed=i).cpu().numpy()
        img.flush()
        res = fio.segment_scene(img, tile=a.tile, k=3)
        slic, merged = np.ascontiguousarray(res.labels), res.write_merged()
    warm = np.ascontiguousarray(slic[:512, :512])
    warm -= warm.min()
    scene.trace_labels(warm, int(warm.max()) + 1, 256, stats={})      # warm-up: allocator and code objects
    rag._trace(torch.from_numpy(warm).to("cuda:0"), int(warm.max()) + 1, {})
    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"scene {a.size} x {a.size} (tools/mb_scene.py's), int32 label rasters in host memory; trace_labels in {a.tile} tiles against "
             f"rag._trace of the whole raster, same process; rag._trace's read + copy is the one copy of the raster to the device",
             "trace_labels: wall time per stage, synchronised at every boundary; rag._trace: hipEvent time between its stages"]
    lines += both("SLIC raster", slic, res.n_labels, a.tile)
    lines += both("merged raster", merged, int(res.result.rep.numel()), a.tile)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
