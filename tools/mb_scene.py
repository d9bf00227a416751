#!/usr/bin/env python3
"""Cost of scene.segment_scene on a scene four tiles large: a synthetic 8192 x 8192 x 3 uint8 scene (the piecewise-constant tile
with noise that tools/mb_slic.py makes, tile by tile) in an np.memmap on disk, streamed in 4096 x 4096 tiles through the default
pipeline (rag.slic cell 29, k = 3, the reference's encoder depth [6, 4, 2] in bf16, batch 2000).

  python tools/mb_scene.py [--out profiles/scene_mb.txt] [--size 8192] [--tile 4096] [--k 3]

Wall time per stage with a device synchronisation at every stage boundary (segment_scene's stage_times), after a warm-up on a small
scene; superpixels, seam positions, seam edges; and the one thing to check: the stitch alone beside the edges of ONE tile, as whole calls
(hipEvent time of rag.seam_stitch / rag.rag_edges, allocations, readback and sort included) and as their launches alone.  No target time is set: the feature has no
parent to compare with.
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
from deepmerge_amd import _lib, rag, scene  # noqa: E402
from deepmerge_amd.ExtractFeatures import FeatureIO  # noqa: E402
from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3  # noqa: E402
from deepmerge_amd.ops import _stream  # noqa: E402
from deepmerge_amd.workload import ev  # noqa: E402
from mb_slic import block_noise_tile  # noqa: E402

STAGES = ("read + copy", "segment", "graph", "stitch", "encode", "merge", "write")     # write: labels_out and write_merged


def seams_of(labels: np.ndarray, tiles):
    """(a, b) on the device: the pixels either side of every seam of the scene, read back from the assembled raster."""
    xs = sorted({t[2] for t in tiles} - {0})
    ys = sorted({t[0] for t in tiles} - {0})
    a = [labels[:, x - 1] for x in xs] + [labels[y - 1, :] for y in ys]
    b = [labels[:, x] for x in xs] + [labels[y, :] for y in ys]
    to = lambda parts: torch.from_numpy(np.ascontiguousarray(np.concatenate(parts))).to("cuda:0")
    return to(a), to(b)


def launches_alone(call, max_out, iters=20):
    """hipEvent time of the three launches of a key-counting entry point (clear, count, compact) on buffers allocated once, sized as
    rag._count_keys sizes them: no allocation, no readback, no sort."""
    log2 = max(10, (4 * max_out - 1).bit_length())
    tk, ok = torch.empty(1 << log2, dtype=torch.int64, device="cuda:0"), torch.empty(max_out, dtype=torch.int64, device="cuda:0")
    tc, oc = torch.empty(1 << log2, dtype=torch.int32, device="cuda:0"), torch.empty(max_out, dtype=torch.int32, device="cuda:0")
    meta = torch.empty(2, dtype=torch.int32, device="cuda:0")
    table = (tk.data_ptr(), tc.data_ptr(), log2, ok.data_ptr(), oc.data_ptr(), max_out, meta.data_ptr(), meta[1:].data_ptr())
    return ev(lambda: _lib.check(call(*table, _stream()), "launch"), iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_mb.txt"))
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
        merged_out = np.memmap(os.path.join(tmp, "merged.i32"), dtype=np.int32, mode="w+", shape=(a.size, a.size))
        fio.segment_scene(np.ascontiguousarray(img[:, :512, :512]), tile=256, k=a.k)      # warm-up: allocator and code objects
        times = {}
        res = fio.segment_scene(img, tile=a.tile, k=a.k, labels_out=labels_out, stage_times=times)
        torch.cuda.synchronize()
        t = time.perf_counter()
        res.write_merged(merged_out)
        times["write"] = times.get("write", 0.0) + time.perf_counter() - t
        sa, sb = seams_of(res.labels, res.tiles)
        y0, y1, x0, x1 = res.tiles[0]
        one = torch.from_numpy(np.ascontiguousarray(res.labels[y0:y1, x0:x1])).to("cuda:0")
    S, n0 = res.n_labels, res.offsets[1]
    tile_of = torch.bucketize(res.edges.long(), torch.tensor(res.offsets[1:], device="cuda:0"), right=True)
    n_seam_edges = int((tile_of[:, 0] != tile_of[:, 1]).sum())
    peri = res.stats["peri"].clone()
    t_stitch = ev(lambda: rag.seam_stitch(sa, sb, S, peri, max_edges=max(1024, min(8 * S, sa.numel()))), 10)      # sized as the driver sizes it
    t_edges = ev(lambda: rag.rag_edges(one, n0), 10)
    lib, n_seam, m_seam = _lib.lib(), sa.numel(), max(1024, min(8 * S, sa.numel()))
    k_stitch = launches_alone(lambda *t: lib.dm_seam_stitch(sa.data_ptr(), sb.data_ptr(), n_seam, S, peri.data_ptr(), *t), m_seam)
    k_edges = launches_alone(lambda *t: lib.dm_rag_edges(one.data_ptr(), one.shape[0], one.shape[1], n0, *t), max(1024, 8 * n0))
    k_floor = launches_alone(lambda *t: lib.dm_seam_stitch(sa.data_ptr(), sb.data_ptr(), 1, S, peri.data_ptr(), *t), m_seam)
    total = sum(times.values())
    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"scene (3, {a.size}, {a.size}) uint8 in an np.memmap, {len(res.tiles)} tiles of {a.tile}, halo {scene.halo_of(rag.MAX_WINDOW)}; "
             f"rag.slic cell 29, k = {a.k}, encoder depth [6, 4, 2] bf16, batch 2000",
             f"superpixels {S}, sample points {res.points.xy.shape[0]}, edges {res.edges.shape[0]}, seam positions {sa.numel()}, "
             f"seam edges {n_seam_edges}; merge: {res.result.rounds} rounds, regions {res.result.regions_per_round[0]} -> "
             f"{res.result.regions_per_round[-1]}",
             "wall time per stage, all tiles (synchronised at every stage boundary):"]
    lines += [f"    {s:40s} {times.get(s, 0.0) * 1e3:11.3f} ms  {100.0 * times.get(s, 0.0) / total:5.1f} %" for s in STAGES]
    lines += [f"    {'total':40s} {total * 1e3:11.3f} ms",
              "the stitch launch alone (whole rag.seam_stitch call: table sizing, three launches, readback, sort):",
              f"    {'rag.seam_stitch, all seams of the scene':40s} {t_stitch * 1e3:11.3f} ms",
              f"    {'rag.rag_edges of ONE tile (' + str(n0) + ' labels)':40s} {t_edges * 1e3:11.3f} ms",
              f"    ratio stitch / one tile's rag_edges: {t_stitch / t_edges:.3f}  (both calls are mostly their allocations, readback and sort)",
              "the launches alone (clear, count, compact on buffers allocated once; no readback, no sort):",
              f"    {'dm_seam_stitch, all seams of the scene':40s} {k_stitch * 1e3:11.3f} ms",
              f"    {'dm_seam_stitch on ONE position (floor)':40s} {k_floor * 1e3:11.3f} ms",
              f"    {'dm_rag_edges of ONE tile':40s} {k_edges * 1e3:11.3f} ms",
              f"    ratio stitch / one tile's rag_edges: {k_stitch / k_edges:.3f}; above the floor of its three launches: "
              f"{(k_stitch - k_floor) * 1e3:.3f} ms"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
