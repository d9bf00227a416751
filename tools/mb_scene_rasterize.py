#!/usr/bin/env python3
"""Cost of scene.rasterize_rings beside rag.rasterize of the same rings, in one process: the 8192 x 8192 scene of tools/mb_scene.py
(2^26 pixels, so that it also fits ONE rag.rasterize), its scene-wide SLIC superpixels (`scene.slic_labels`) traced across the seams
(`scene.trace_labels`), and those rings rasterised back -- in four 4096 tiles through a `RingSource`, and whole.

  python tools/mb_scene_rasterize.py [--out profiles/scene_rasterize_mb.txt] [--size 8192] [--tile 4096] [--rounds 3]

The two alternate, `--rounds` times, after a warm-up of both on a small raster; every timing is a host clock around work that ends
in a device synchronisation.  The tiled call's stages come from its `stats` (a synchronisation at every stage boundary), the
whole-raster call's from its own (hipEvent times), from one extra run each.  Both results are compared with the SLIC raster before
anything is reported.  Then `scene.trace_labels` is timed twice, alternating: reading a `RingSource` (no host raster: every window is
rasterised on the device) and reading the host raster.  No target time is set: the feature has no parent to compare with.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from deepmerge_amd import rag, scene  # noqa: E402
from mb_slic import block_noise_tile  # noqa: E402


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_rasterize_mb.txt"))
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    H = W = a.size
    with tempfile.TemporaryDirectory() as tmp:
        img = np.memmap(os.path.join(tmp, "scene.u8"), dtype=np.uint8, mode="w+", shape=(3, H, W))
        for i, (y0, y1, x0, x1) in enumerate(scene.tile_grid(H, W, a.tile)):
            img[:, y0:y1, x0:x1] = block_noise_tile(3, y1 - y0, x1 - x0, seed=i).cpu().numpy()
        img.flush()
        labels, n = scene.slic_labels(img, tile=a.tile)
        del img
    polys = scene.trace_labels(labels, n, a.tile)[0]
    warm = np.ascontiguousarray(labels[:512, :512])
    warm_ids, warm = np.unique(warm, return_inverse=True)
    warm = warm.reshape(512, 512).astype(np.int32)
    warm_polys = scene.trace_labels(warm, len(warm_ids), 256)[0]           # warm-up: allocator and code objects
    scene.rasterize_rings(warm_polys, 512, 512, tile=256)
    rag.rasterize(warm_polys, 512, 512).cpu()

    out = np.empty((H, W), np.int32)
    tiled = lambda: scene.rasterize_rings(polys, H, W, tile=a.tile, labels_out=out)
    whole = lambda: rag.rasterize(polys, H, W).cpu().numpy()
    if not np.array_equal(tiled(), labels) or not np.array_equal(whole(), labels):
        raise RuntimeError("the rasterised rings differ from the raster they were traced from")
    t_tiled, t_whole = [], []
    for _ in range(a.rounds):
        t_tiled.append(wall(tiled)[0])
        t_whole.append(wall(whole)[0])
    stats, whole_stats = {}, {}
    scene.rasterize_rings(polys, H, W, tile=a.tile, labels_out=out, stats=stats)
    t_dev, on_device = wall(lambda: rag.rasterize(polys, H, W, stats=whole_stats))
    t_copy = wall(lambda: on_device.cpu().numpy())[0]

    source = scene.RingSource(polys, H, W)
    from_rings, from_raster = (lambda: scene.trace_labels(source, n, a.tile)), (lambda: scene.trace_labels(labels, n, a.tile))
    got, want = from_rings(), from_raster()
    for f in ("region_ptr", "ring_ptr", "xy", "ring_label", "ring_area2"):
        assert torch.equal(getattr(got[0], f), getattr(want[0], f)), f
    del got, want
    t_rings, t_raster = [], []
    for _ in range(a.rounds):
        t_rings.append(wall(from_rings)[0])
        t_raster.append(wall(from_raster)[0])

    ms = lambda ts: "  ".join(f"{t * 1e3:9.1f}" for t in ts) + f"   median {statistics.median(ts) * 1e3:9.1f} ms"
    events = stats["events"]
    stage_keys = [k for k, v in stats.items() if isinstance(v, float)]
    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"scene {H} x {W} (tools/mb_scene.py's): {n} SLIC superpixels across the seams, traced into {stats['rings']} rings of "
             f"{stats['vertices']} vertices; rasterised back in {stats['tiles']} tiles of {a.tile} and whole; both equal the raster: yes",
             f"wall time per call, host raster included, {a.rounds} alternating rounds:",
             f"    scene.rasterize_rings            {ms(t_tiled)}",
             f"    rag.rasterize(...).cpu().numpy() {ms(t_whole)}",
             f"    ratio of the medians {statistics.median(t_tiled) / statistics.median(t_whole):.2f}",
             f"scene.rasterize_rings, one run, synchronised at every stage boundary; events per band: "
             + ", ".join(f"rows {y0}..{y1 - 1}: {v}" for (y0, y1), v in events.items())]
    lines += [f"    {k:48s} {stats[k] * 1e3:9.3f} ms" for k in stage_keys]
    lines += [f"rag.rasterize, one run, hipEvent time between its stages (N = {whole_stats['N']}); whole call {t_dev * 1e3:.3f} ms, copy to the "
              f"host {t_copy * 1e3:.3f} ms:"]
    lines += [f"    {stage:48s} {t:9.3f} ms" for stage, t in whole_stats["stage_ms"]]
    lines += [f"scene.trace_labels in {a.tile} tiles, wall time, {a.rounds} alternating rounds; the results are equal array for array:",
              f"    from a RingSource (no host raster) {ms(t_rings)}",
              f"    from the host raster               {ms(t_raster)}",
              f"    ratio of the medians {statistics.median(t_rings) / statistics.median(t_raster):.2f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
