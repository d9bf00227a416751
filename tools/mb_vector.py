#!/usr/bin/env python3
"""Cost of rag.polygons / rag.boundary_arcs on the config-4 raster: the SLIC superpixels (cell 29, ~20 k labels) of a 4096 x 4096 x 4
uint8 piecewise-constant tile with noise, as tools/mb_slic.py makes it.

  python tools/mb_vector.py [--out profiles/vector_mb.txt] [--size 4096]

hipEvent time over repeated whole calls (allocations and readbacks included: the calls size their buffers from the dart count they
read back), the stages of one tracing run between events, the number of darts D, the jumping rounds and the bytes the passes
move.  Beside them, in the same process on the same raster: rag.rag_edges, the other pass over the labels.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vector_mb.txt"))
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args()
    H = W = a.size
    tile = block_noise_tile(4, H, W)
    labels, S = rag.slic(tile, cell=29, compactness=10, iters=10)
    del tile
    edges, _ = rag.rag_edges(labels, S)
    rag._trace(labels, S)                                          # warm-up: allocator and code objects
    t_edges = ev(lambda: rag.rag_edges(labels, S), 5)
    t_trace = ev(lambda: rag._trace(labels, S), 5)
    t_polys = ev(lambda: rag.polygons(labels, S), 3)
    t_arcs = ev(lambda: rag.boundary_arcs(labels, S, edges=edges), 3)
    st = {}
    rag._trace(labels, S, st)
    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"input: {H} x {W} int32 labels, n_labels = {S} (rag.slic, cell 29), E = {edges.shape[0]} edges",
             f"darts D = {st['D']}, rings = {st['rings']} with {st['vertices']} vertices, kept arcs = {st['arcs']} with {st['arc_vertices']} "
             f"vertices; jumping rounds: {st['head_rounds']} (heads) + {st['rank_rounds']} (ranks)",
             f"(a) one tracing run (rag._trace, both results): {t_trace * 1e3:9.3f} ms   {st['bytes'] / 1e6:.0f} MB moved by its passes, "
             f"{st['bytes'] / t_trace / 1e9:.1f} GB/s",
             f"    rag.polygons {t_polys * 1e3:9.3f} ms; rag.boundary_arcs(edges=) {t_arcs * 1e3:9.3f} ms (each is one run)",
             "(b) stages of one run, between events (host work and readbacks fall into the stage they end):"]
    lines += [f"    {name:48s} {ms:9.3f} ms" for name, ms in st["stage_ms"]]
    lines += [f"(c) same process, same raster: rag.rag_edges {t_edges * 1e3:9.3f} ms; one tracing run is {t_trace / t_edges:.1f} x that"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
