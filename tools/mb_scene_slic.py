#!/usr/bin/env python3
"""Cost of scene.slic_labels (superpixels that cross tile seams) on the scene of tools/mb_scene.py: a synthetic 8192 x 8192 x 3
uint8 scene in an np.memmap on disk, in four 4096 x 4096 tiles, rag.slic's defaults (cell 29, compactness 10, 10 iterations).

  python tools/mb_scene_slic.py [--out profiles/scene_slic_mb.txt] [--size 8192] [--tile 4096] [--repeats 3]

Measured, in one session:
  - wall time per stage of scene.slic_labels (its stage_times: a device synchronisation at every stage boundary), with the cores
    resident between the passes and with resident_bytes=0 (every pass reads the image again), `--repeats` runs each;
  - beside it what segment_scene's default path spends on the same pixels: per tile read + copy and rag.slic (its "segment" stage),
    `--repeats` runs: their spread is the session's run-to-run spread;
  - for one 4096 x 4096 core, hipEvent time of a round (assignment pass with sums + update) and of the labels pass: inside
    dm_slic_iterate (by difference of iters = 0, R and 2 R) and as dm_scene_slic_pass / dm_scene_slic_update on the same tile, same
    table of centres; the existing kernel is repeated to give the spread the new one is read against.
No ratio is set in advance.
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
from deepmerge_amd import _lib, rag, scene  # noqa: E402
from deepmerge_amd.ops import _stream, check  # noqa: E402
from deepmerge_amd.workload import ev  # noqa: E402
from mb_slic import block_noise_tile  # noqa: E402

STAGES = ("read + copy", "assignment passes", "components + graph", "seams", "absorption rounds", "relabel + write")
DEV = "cuda:0"


def per_tile_slic(img, tiles):
    """segment_scene's default path on the same pixels, without the graph and the encoder: (read + copy, segment) seconds and the
    superpixel count."""
    clock_into = {}
    clock = scene._Clock(clock_into, torch.device(DEV))
    n = 0
    for core in tiles:
        t = scene._read(scene._as_source(img), core, torch.uint8, 3, torch.device(DEV))
        clock.lap("read + copy")
        n += int(rag.slic(t)[1])
        clock.lap("segment")
    return clock_into["read + copy"], clock_into["segment"], n


def kernel_times(tile, cell, compactness, rounds, repeats):
    """hipEvent seconds for one core: ((round, labels pass) inside dm_slic_iterate per repeat, (round, labels pass) of the scene entries per repeat)."""
    lib = _lib.lib()
    bands, H, W = tile.shape
    K = ((H + cell - 1) // cell) * ((W + cell - 1) // cell)
    centres = torch.empty((K, 6), dtype=torch.int32, device=DEV)
    sums = torch.empty((K, 7), dtype=torch.int64, device=DEV)
    labels = torch.empty((H, W), dtype=torch.int32, device=DEV)
    it = lambda n: check(lib.dm_slic_iterate(tile.data_ptr(), bands, H, W, cell, compactness, n, centres.data_ptr(), sums.data_ptr(),
                                             labels.data_ptr(), _stream()), "dm_slic_iterate")
    place = (tile.data_ptr(), bands, H, W, 0, 0, H, W, cell)
    init = lambda: check(lib.dm_scene_slic_init(*place, centres.data_ptr(), sums.data_ptr(), _stream()), "dm_scene_slic_init")
    sum_pass = lambda: check(lib.dm_scene_slic_pass(*place, compactness, centres.data_ptr(), sums.data_ptr(), None, _stream()), "dm_scene_slic_pass")
    lab_pass = lambda: check(lib.dm_scene_slic_pass(*place, compactness, centres.data_ptr(), None, labels.data_ptr(), _stream()), "dm_scene_slic_pass")
    update = lambda: check(lib.dm_scene_slic_update(K, centres.data_ptr(), sums.data_ptr(), _stream()), "dm_scene_slic_update")

    def scene_rounds(n):
        init()
        for _ in range(n):
            sum_pass()
            update()
        lab_pass()

    old, new = [], []
    for _ in range(repeats):
        for into, run in ((old, it), (new, scene_rounds)):
            t0, t1, t2 = ev(lambda: run(0), 5), ev(lambda: run(rounds), 5), ev(lambda: run(2 * rounds), 5)
            into.append(((t2 - t1) / rounds, t0))                 # a round; init + the labels pass
    return old, new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_slic_mb.txt"))
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    tiles = scene.tile_grid(a.size, a.size, a.tile)
    with tempfile.TemporaryDirectory() as tmp:
        img = np.memmap(os.path.join(tmp, "scene.u8"), dtype=np.uint8, mode="w+", shape=(3, a.size, a.size))
        for i, (y0, y1, x0, x1) in enumerate(tiles):
            img[:, y0:y1, x0:x1] = block_noise_tile(3, y1 - y0, x1 - x0, seed=i).cpu().numpy()
        img.flush()
        labels_out = np.memmap(os.path.join(tmp, "labels.i32"), dtype=np.int32, mode="w+", shape=(a.size, a.size))
        small = np.ascontiguousarray(img[:, :512, :512])
        scene.slic_labels(small, tile=256)                          # warm-up: allocator and code objects
        per_tile_slic(small, scene.tile_grid(512, 512, 256))
        runs = {"resident": [], "streamed": []}
        stats = {}
        for _ in range(a.repeats):
            for name, budget in (("resident", 8 << 30), ("streamed", 0)):
                times = {}
                _, n = scene.slic_labels(img, tile=a.tile, labels_out=labels_out, resident_bytes=budget, stage_times=times, stats=stats)
                runs[name].append(times)
        old_path = [per_tile_slic(img, tiles) for _ in range(a.repeats)]
        y0, y1, x0, x1 = tiles[0]
        one = torch.from_numpy(np.ascontiguousarray(img[:, y0:y1, x0:x1])).to(DEV)
    k_old, k_new = kernel_times(one, 29, 10, 5, a.repeats)
    ms = lambda vs: "  ".join(f"{v * 1e3:10.3f}" for v in vs)
    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"scene (3, {a.size}, {a.size}) uint8 in an np.memmap, {len(tiles)} tiles of {a.tile}; cell 29, compactness 10, 10 iterations; "
             f"{a.repeats} runs of everything, in the order run (ms)",
             f"scene.slic_labels: superpixels {n}; tile-local components {stats['provisional']}, united across seams {stats['seam_unions']} "
             f"pairs, components {stats['components']}, absorption rounds {stats['rounds']}, picked edges {stats['picks']}"]
    for name in ("resident", "streamed"):
        reads = 1 if name == "resident" else 12
        lines.append(f"scene.slic_labels, cores {name} (image read {reads} x), wall time per stage, synchronised at every stage boundary:")
        lines += [f"    {s:28s} {ms([t.get(s, 0.0) for t in runs[name]])}" for s in STAGES]
        lines.append(f"    {'total':28s} {ms([sum(t.values()) for t in runs[name]])}")
    lines += ["segment_scene's per-tile superpixels on the same pixels (superpixels stop at the seams; " f"{old_path[0][2]} of them):",
              f"    {'read + copy':28s} {ms([r[0] for r in old_path])}",
              f"    {'segment (rag.slic per tile)':28s} {ms([r[1] for r in old_path])}",
              f"one {a.tile} x {a.tile} core, hipEvent time, same tile and table of centres:",
              f"    {'round inside dm_slic_iterate':44s} {ms([r[0] for r in k_old])}",
              f"    {'dm_scene_slic_pass (sums) + update':44s} {ms([r[0] for r in k_new])}",
              f"    {'init + labels pass, dm_slic_iterate(iters=0)':44s} {ms([r[1] for r in k_old])}",
              f"    {'dm_scene_slic_init + pass (labels)':44s} {ms([r[1] for r in k_new])}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
