#!/usr/bin/env python3
"""Cost of scene.simplify_labels_topology beside the plain call of the same build, in one session: the 8192 x 8192 scene of
tools/mb_scene.py in four 4096 tiles, its SLIC raster and its merged raster, each at tolerance 1.5 and 8.

  python tools/mb_scene_simplify_topology.py [--out profiles/scene_simplify_topology_mb.txt] [--size 8192] [--tile 4096] [--tolerances 1.5 8]

Per raster and tolerance: the flagged segments of every round, the rounds taken and the grid's cell side; wall time of whole calls,
the repairing call (topology=True below) against the plain one (topology=False) alternating in one session after a warm-up, the median and the range of the windows; the stages
of the rounds of one run between events and the "simplify: topology rounds" stage of that run; the same raster through
rag.simplify(topology=True) from device memory, whose result is checked to be bit-equal and whose rounds are checked to flag the same
segments.  No ratio is fixed in advance: what is measured is written down.
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
from deepmerge_amd.ExtractFeatures import FeatureIO  # noqa: E402
from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3  # noqa: E402
from deepmerge_amd.workload import ev  # noqa: E402
from mb_slic import block_noise_tile  # noqa: E402

WINDOWS, ITERS = 5, 6


def wall_ms(call, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def report(name: str, raster: np.ndarray, n: int, tile: int, tol: float):
    plain = lambda **kw: scene.simplify_labels(raster, n, tol, tile, **kw)
    safe = lambda **kw: scene.simplify_labels_topology(raster, n, tol, tile, **kw)
    plain(), safe()                                                # warm-up of both modes at this size: allocator and code objects
    plain_ms, safe_ms = [], []
    for _ in range(WINDOWS):                                       # alternating windows: the two share whatever else the host does
        plain_ms.append(wall_ms(plain, ITERS))
        safe_ms.append(wall_ms(safe, ITERS))
    st, st0, whole_st = {}, {}, {}
    tiled = safe(stats=st)
    plain_polys, _ = plain(stats=st0)
    on_device = torch.from_numpy(np.ascontiguousarray(raster)).to("cuda:0")
    whole = rag.simplify(on_device, n, tol, stats=whole_st, topology=True)
    for f in ("region_ptr", "ring_ptr", "xy", "ring_label", "ring_area2"):
        assert torch.equal(getattr(tiled[0], f), getattr(whole[0], f)), f
    for f in ("arc_ptr", "xy", "left", "right"):
        assert torch.equal(getattr(tiled[1], f), getattr(whole[1], f)), f
    assert st["topology_flagged"] == whole_st["topology_flagged"]
    whole_ms = [ev(lambda: rag.simplify(on_device, n, tol, topology=True), 10) * 1e3 for _ in range(3)]
    whole_plain_ms = [ev(lambda: rag.simplify(on_device, n, tol), 10) * 1e3 for _ in range(3)]
    traced = rag.polygons(on_device, n)
    wrong = lambda p: int(((p.ring_area2 == 0) | (torch.sign(p.ring_area2) != torch.sign(traced.ring_area2))).sum())
    H, W = raster.shape
    assert wrong(tiled[0]) == 0 and int(tiled[0].ring_area2.sum()) == 2 * H * W
    med = statistics.median
    sec, sec0 = st["stage_s"], st0["stage_s"]
    reads = sec0.get("read + copy", 0.0) / sum(sec0.values())
    lines = [f"{name}: {H} x {W} int32 labels in host memory, n_labels = {n}, {st['tiles']} tiles of {tile}; arcs = {st['arcs']}, arc vertices "
             f"{st['arc_vertices']}, tolerance {tol} px (q = {st['q']}); bit-equal to rag.simplify(topology=True): yes",
             f"    cell side 2^{st['topology_cell_log2']} corners; segments after the repair {st['topology_segments']}; flagged per round "
             f"{st['topology_flagged']}: {st['topology_rounds']} repair round(s), {st['topology_rounds'] + 1} detection round(s); cell-list entries "
             f"in the last round {st['topology_cell_entries']}",
             f"    plain simplify_labels leaves {wrong(plain_polys)} of {st['rings']} rings with zero or wrong-signed area; topology=True leaves 0",
             f"    kept ring vertices: plain {st0['kept_vertices']}, topology {st['kept_vertices']}; kept arc vertices: plain "
             f"{st0['kept_arc_vertices']}, topology {st['kept_arc_vertices']}",
             f"(a) whole call (wall), median of {WINDOWS} windows of {ITERS} calls [min .. max]: topology=False {med(plain_ms):8.3f} ms "
             f"[{min(plain_ms):.3f} .. {max(plain_ms):.3f}]; topology=True {med(safe_ms):8.3f} ms [{min(safe_ms):.3f} .. {max(safe_ms):.3f}]; "
             f"ratio {med(safe_ms) / med(plain_ms):.2f}",
             f"    the window reads ('read + copy') are {100 * reads:.0f} % of one plain call synchronised at its stage boundaries",
             f"    the same raster from device memory, rag.simplify, median of 3 windows of 10 calls: topology=False {med(whole_plain_ms):.3f} ms, "
             f"topology=True {med(whole_ms):.3f} ms, ratio {med(whole_ms) / med(whole_plain_ms):.2f}",
             "(b) stages of the rounds of one run, between events (the scans and the host work fall into the stage they end, the readback "
             "into refine):"]
    for r, stages in enumerate(st["topology_stage_ms"]):
        lines.append(f"    round {r}: " + ", ".join(f"{k} {v:.3f}" for k, v in stages.items()) + f" = {sum(stages.values()):.3f} ms")
    total = {k: sum(s[k] for s in st["topology_stage_ms"]) for k in st["topology_stage_ms"][0]}
    lines.append("    all rounds: " + ", ".join(f"{k} {v:.3f}" for k, v in total.items()) + f" = {sum(total.values()):.3f} ms")
    lines.append(f"    the 'simplify: topology rounds' stage of that run, fixed points and allocations included: "
                 f"{sec['simplify: topology rounds'] * 1e3:.3f} ms of {sum(sec.values()) * 1e3:.3f} ms; rag.simplify's 'topology rounds' stage: "
                 f"{dict(whole_st['stage_ms'])['topology rounds']:.3f} ms")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_simplify_topology_mb.txt"))
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--tolerances", type=float, nargs="+", default=[1.5, 8.0])
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
    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"scene {a.size} x {a.size} (tools/mb_scene.py's), int32 label rasters in host memory; scene.simplify_labels in {a.tile} tiles, "
             f"topology=True against topology=False of the same build, alternating in one session"]
    for tol in a.tolerances:
        lines += report("SLIC raster", slic, res.n_labels, a.tile, tol)
        lines += report("merged raster", merged, int(res.result.rep.numel()), a.tile, tol)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
