#!/usr/bin/env python3
"""Cost of scene.simplify_labels beside its two yardsticks, in one process: the 8192 x 8192 scene of tools/mb_scene.py (2^26 pixels,
so that it also fits ONE rag.simplify), segmented by the default pipeline, then its SLIC raster and its merged raster simplified at
one tolerance -- in four 4096 tiles across the seams, and whole.

  python tools/mb_scene_simplify.py [--out profiles/scene_simplify_mb.txt] [--size 8192] [--tile 4096] [--tolerance 1.5]

The yardsticks: scene.trace_labels on the same source (the parent's cost for the same darts) and rag.simplify of the same raster
from device memory.  simplify_labels and trace_labels: wall time per stage, synchronised at every boundary (their `stats`);
rag.simplify: hipEvent time between its stages.  All after a warm-up on a small raster.  The two results are checked to be
bit-equal.  No ratio is fixed in advance: what is measured is written down.
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

TRACE_STAGES = ("read + copy", "per-tile passes", "sort + join", "rounds", "emit")
SIMPLIFY_STAGES = ("node lists + arc_keep", "chains", "kept set", "arc_count", "ring_count", "scans + readback of the totals", "arc_emit",
                   "ring_emit + area")
# rag.simplify's stages, and the stages of the sparse form that do the same work
WHOLE = (("nodes", ("node lists + arc_keep",)), ("chains", ("chains", "kept set")),
         ("arc_count + ring_count + scans + readback of the totals", ("arc_count", "ring_count", "scans + readback of the totals")),
         ("arc_emit + ring_emit + area", ("arc_emit", "ring_emit + area")))


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def both(name: str, raster: np.ndarray, n: int, tile: int, tol: float):
    """One tiled simplification, one tiled trace and one whole simplification of `raster`, timed per stage; the report's lines."""
    tiled_stats, trace_stats, whole_stats = {}, {}, {}
    tiled, t_tiled = wall(lambda: scene.simplify_labels(raster, n, tol, tile, stats=tiled_stats))
    _, t_trace = wall(lambda: scene.trace_labels(raster, n, tile, stats=trace_stats))
    on_device, t_copy = wall(lambda: torch.from_numpy(np.ascontiguousarray(raster)).to("cuda:0"))
    whole, t_whole = wall(lambda: rag.simplify(on_device, n, tol, stats=whole_stats))
    for f in ("region_ptr", "ring_ptr", "xy", "ring_label", "ring_area2"):
        assert torch.equal(getattr(tiled[0], f), getattr(whole[0], f)), f
    for f in ("arc_ptr", "xy", "left", "right"):
        assert torch.equal(getattr(tiled[1], f), getattr(whole[1], f)), f
    s, ms = tiled_stats, lambda sec: f"{sec * 1e3:11.3f} ms"
    st = s["stage_s"]
    lines = [f"{name}: {n} labels, {s['D']} darts, {s['rings']} rings, {s['arcs']} arcs, {s['tiles']} tiles; {s['nodes']} nodes, {s['kept']} kept "
             f"corners; ring vertices {s['vertices']} -> {s['kept_vertices']}, arc vertices {s['arc_vertices']} -> {s['kept_arc_vertices']}; "
             f"longest arc {s['longest_arc']} vertices; q = {s['q']}; bit-equal to rag.simplify: yes",
             f"    {'tracing stage':34s} {'simplify_labels':>15s} {'trace_labels':>14s}   ratio"]
    for stage in TRACE_STAGES:
        a, b = st.get(stage, 0.0), trace_stats["stage_s"].get(stage, 0.0)
        lines.append(f"    {stage:34s} {ms(a)}  {ms(b)}   {a / b if b else float('nan'):5.2f}")
    lines.append(f"    {'simplify stage':34s} {'simplify_labels':>15s} {'rag.simplify':>14s}   ratio   (rag.simplify's stage)")
    whole_ms = dict(whole_stats["stage_ms"])
    for theirs, ours in WHOLE:
        a, b = sum(st.get("simplify: " + o, 0.0) for o in ours), whole_ms[theirs] * 1e-3
        lines.append(f"    {' + '.join(ours)[:34]:34s} {ms(a)}  {ms(b)}   {a / b if b else float('nan'):5.2f}   ({theirs})")
    ring = st.get("simplify: ring_count", 0.0) + st.get("simplify: ring_emit + area", 0.0)
    arc = st.get("simplify: arc_count", 0.0) + st.get("simplify: arc_emit", 0.0)
    dense = (whole_ms["arc_count + ring_count + scans + readback of the totals"] + whole_ms["arc_emit + ring_emit + area"]) * 1e-3
    lines.append(f"    ring pass alone (ring_count + ring_emit + area) {ms(ring)}; arc pass alone {ms(arc)}; rag.simplify's count and emit stages, "
                 f"rings and arcs together, {ms(dense)}")
    simplify = sum(v for k, v in st.items() if k.startswith("simplify: "))
    whole_simplify = sum(whole_ms.values()) * 1e-3
    lines.append(f"    {'simplify stages, sum':34s} {ms(simplify)}  {ms(whole_simplify)}   {simplify / whole_simplify:5.2f}")
    lines.append(f"    {'total (wall)':34s} {ms(t_tiled)}  {ms(t_trace)}   {t_tiled / t_trace:5.2f}   (trace_labels)")
    lines.append(f"    {'':34s} {'':14s}  {ms(t_copy + t_whole)}   {t_tiled / (t_copy + t_whole):5.2f}   (copy + rag.simplify, its tracing included)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_simplify_mb.txt"))
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--tolerance", type=float, default=1.5)
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
    n_warm = int(warm.max()) + 1
    scene.simplify_labels(warm, n_warm, a.tolerance, 256, stats={})       # warm-up: allocator and code objects
    scene.trace_labels(warm, n_warm, 256, stats={})
    rag.simplify(torch.from_numpy(warm).to("cuda:0"), n_warm, a.tolerance, stats={})
    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"scene {a.size} x {a.size} (tools/mb_scene.py's), int32 label rasters in host memory; simplify_labels at tolerance {a.tolerance} in "
             f"{a.tile} tiles against trace_labels on the same source and rag.simplify of the whole raster from device memory, same process",
             "simplify_labels, trace_labels: wall time per stage, synchronised at every boundary; rag.simplify: hipEvent time between its stages"]
    lines += both("SLIC raster", slic, res.n_labels, a.tile, a.tolerance)
    lines += both("merged raster", merged, int(res.result.rep.numel()), a.tile, a.tolerance)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
