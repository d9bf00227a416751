#!/usr/bin/env python3
"""Cost of rag.simplify(topology=True) on the two rasters of tools/mb_simplify.py: the config-4 SLIC superpixels of a 4096 x 4096
tile and their merged partition, each at tolerance 1.5 and 8.

  python tools/mb_simplify_topology.py [--out profiles/simplify_topology_mb.txt] [--size 4096] [--tolerances 1.5 8]

Per raster and tolerance: the flagged segments of every round and the rounds taken; hipEvent time over repeated whole calls of
topology=True against topology=False (today's call, the baseline), the two alternating in one session, the median and the range of
the windows; the stages of the rounds of one run between events; the kept vertices of both modes.  Both results are compared for
what must hold: every plain vertex is kept, and the repaired rings keep the traced rings' signs.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from deepmerge_amd import rag  # noqa: E402
from deepmerge_amd.workload import ev  # noqa: E402
from mb_simplify import merged_partition  # noqa: E402
from mb_slic import block_noise_tile  # noqa: E402

WINDOWS, ITERS = 5, 40


def report(name, labels, S, tol):
    H, W = labels.shape
    plain_keep = rag._simplify(labels, S, tol)[2]                  # warm-up of both modes: allocator and code objects
    safe_polys, _, safe_keep = rag._simplify(labels, S, tol, topology=True)
    plain_ms, safe_ms = [], []
    for _ in range(WINDOWS):                                       # alternating windows: the two share whatever else the host does
        plain_ms.append(ev(lambda: rag.simplify(labels, S, tol), ITERS) * 1e3)
        safe_ms.append(ev(lambda: rag.simplify(labels, S, tol, topology=True), ITERS) * 1e3)
    st, st0 = {}, {}
    rag.simplify(labels, S, tol, stats=st, topology=True)
    plain_polys, _ = rag.simplify(labels, S, tol, stats=st0)
    traced = rag.polygons(labels, S)
    wrong = lambda p: int(((p.ring_area2 == 0) | (torch.sign(p.ring_area2) != torch.sign(traced.ring_area2))).sum())
    assert bool(((safe_keep > 0) >= (plain_keep > 0)).all()) and wrong(safe_polys) == 0 and int(safe_polys.ring_area2.sum()) == 2 * H * W
    med = statistics.median
    own0 = sum(ms for _, ms in st0["stage_ms"])
    lines = [f"{name}: {H} x {W} int32 labels, n_labels = {S}; kept arcs = {st['arcs']}, arc vertices {st['arc_vertices']}, tolerance {tol} px "
             f"(q = {st['q']})",
             f"    segments after the repair {st['topology_segments']}; flagged per round {st['topology_flagged']}: {st['topology_rounds']} repair "
             f"round(s), {st['topology_rounds'] + 1} detection round(s); cell-list entries in the last round {st['topology_cell_entries']}",
             f"    plain simplify leaves {wrong(plain_polys)} of {st['rings']} rings with zero or wrong-signed area; topology=True leaves 0",
             f"    kept ring vertices: plain {st0['kept_vertices']}, topology {st['kept_vertices']}; kept arc vertices: plain "
             f"{st0['kept_arc_vertices']}, topology {st['kept_arc_vertices']}",
             f"(a) whole call, median of {WINDOWS} windows of {ITERS} calls [min .. max]: topology=False {med(plain_ms):8.3f} ms "
             f"[{min(plain_ms):.3f} .. {max(plain_ms):.3f}]; topology=True {med(safe_ms):8.3f} ms [{min(safe_ms):.3f} .. {max(safe_ms):.3f}]; "
             f"ratio {med(safe_ms) / med(plain_ms):.2f}",
             f"    the plain call's passes after the tracing: {own0:.3f} ms in one run",
             "(b) stages of the rounds of one run, between events (the scans and the host work fall into the stage they end, the readback "
             "into refine):"]
    for r, stages in enumerate(st["topology_stage_ms"]):
        lines.append(f"    round {r}: " + ", ".join(f"{k} {v:.3f}" for k, v in stages.items()) + f" = {sum(stages.values()):.3f} ms")
    total = {k: sum(s[k] for s in st["topology_stage_ms"]) for k in st["topology_stage_ms"][0]}
    lines.append("    all rounds: " + ", ".join(f"{k} {v:.3f}" for k, v in total.items()) + f" = {sum(total.values()):.3f} ms")
    rest = dict(st["stage_ms"])
    lines.append(f"    the 'topology rounds' stage of that run, fixed points and allocations included: {rest['topology rounds']:.3f} ms")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_topology_mb.txt"))
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--tolerances", type=float, nargs="+", default=[1.5, 8.0])
    a = ap.parse_args()
    H = W = a.size
    tile = block_noise_tile(4, H, W)
    labels, S = rag.slic(tile, cell=29, compactness=10, iters=10)
    merged, C = merged_partition(tile, labels, S)
    del tile
    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}"]
    for tol in a.tolerances:
        lines += report("config-4 superpixels (rag.slic, cell 29)", labels, S, tol)
        lines += report("their merged partition (rag.merge_regions on mean colours)", merged, C, tol)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
