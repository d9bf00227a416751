#!/usr/bin/env python3
"""Cost of rag.simplify on the config-4 raster and on its merged partition: the SLIC superpixels (cell 29, ~20 k labels) of a
4096 x 4096 x 4 uint8 piecewise-constant tile with noise, as tools/mb_slic.py makes it, and the regions rag.merge_regions leaves of
them on the superpixels' mean colours (the tile's blocks, a few thousand objects that keep every stair step of the cells they
swallowed).

  python tools/mb_simplify.py [--out profiles/simplify_mb.txt] [--size 4096] [--tolerance 1.5]

hipEvent time over repeated whole calls (allocations and readbacks included), the stages of one run between events, and the sizes
before and after.  Beside them, in the same process on the same raster: rag._trace, the tracing run every simplify call starts
with -- the parent's cost for the same darts.
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


def merged_partition(tile, labels, S):
    """(labels int32 [H,W], n) of mutual-best merging on the superpixels' mean colours / 8: cells of one block differ by the noise."""
    st = rag.label_stats(labels, tile[:3].contiguous(), S)
    feats = (st["sum"].double() / st["count"].double().unsqueeze(1) / 8.0).float().contiguous()
    edges, w = rag.rag_edges(labels, S)
    ids = torch.arange(S + 1, dtype=torch.int32, device=labels.device)
    res = rag.merge_regions(feats, ids, ids[:-1].contiguous(), edges, margin=1.0, weights=w)
    return res.labels(labels), int(res.rep.numel())


def report(name, labels, S, tol):
    rag._simplify(labels, S, tol)                                  # warm-up: allocator and code objects
    t_trace = ev(lambda: rag._trace(labels, S), 5)
    t_all = ev(lambda: rag.simplify(labels, S, tol), 5)
    st = {}
    rag.simplify(labels, S, tol, stats=st)
    tr = st["trace"]
    own = sum(ms for _, ms in st["stage_ms"])
    H, W = labels.shape
    lines = [f"{name}: {H} x {W} int32 labels, n_labels = {S}; darts D = {tr['D']}, rings = {st['rings']}, kept arcs = {st['arcs']}, "
             f"longest arc = {st['longest_arc']} vertices",
             f"    tolerance {tol} px (q = {st['q']}): ring vertices {st['vertices']} -> {st['kept_vertices']}, arc vertices "
             f"{st['arc_vertices']} -> {st['kept_arc_vertices']}",
             f"(a) rag.simplify, whole call: {t_all * 1e3:9.3f} ms; rag._trace alone, same raster, same session: {t_trace * 1e3:9.3f} ms; "
             f"the passes after the tracing: {own:9.3f} ms in one run",
             "(b) stages of that run after the tracing, between events (host work and the readback fall into the stage they end):"]
    lines += [f"    {stage:56s} {ms:9.3f} ms" for stage, ms in st["stage_ms"]]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_mb.txt"))
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--tolerance", type=float, default=1.5)
    a = ap.parse_args()
    H = W = a.size
    tile = block_noise_tile(4, H, W)
    labels, S = rag.slic(tile, cell=29, compactness=10, iters=10)
    merged, C = merged_partition(tile, labels, S)
    del tile
    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}"]
    lines += report("config-4 superpixels (rag.slic, cell 29)", labels, S, a.tolerance)
    lines += report("their merged partition (rag.merge_regions on mean colours)", merged, C, a.tolerance)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
