#!/usr/bin/env python3
"""Cost of rag.slic at the config-4 tile size: 4096 x 4096 x 4 uint8, cell 29 (~20 k superpixels), compactness 10, 10 iterations,
on a piecewise-constant image (blocks of side 97) with uniform noise of +-8.

  python tools/mb_slic.py [--out profiles/slic_mb.txt]

Per stage (hipEvent time over repeated calls on pre-allocated buffers unless said otherwise):
  iteration pass   (dm_slic_iterate with 10 iterations - with 0) / 10: one assignment pass + the centre update; the byte floor of a
                   pass is the tile itself, bands * H * W bytes.  The last pass (iters = 0: init + assignment + the label raster written)
                   is printed beside it.
  components       dm_connected_labels on the assigned raster (4 B read by the tile pass; parent written, walked and read; labels
                   written), and rag.connected_labels as a whole call (allocations + its one readback).
  absorption       every round of rag.absorb_small, wall time between synchronisations (rag_edges, the picks, merge_components,
                   relabel_raster and their readbacks).
Beside them, in the same process, on the SLIC raster: rag.rag_edges + rag.sample_points + rag.label_stats -- the rest of
merge_tile's graph stages -- and one whole rag.slic call.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmerge_amd import _lib, rag  # noqa: E402
from deepmerge_amd.ops import _stream, check  # noqa: E402
from deepmerge_amd.workload import ev  # noqa: E402

DEV = "cuda:0"


def block_noise_tile(bands, H, W, block=97, noise=8, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    by, bx = -(-H // block), -(-W // block)
    base = torch.randint(noise, 256 - noise, (bands, by, bx), device=DEV, generator=g)
    img = base.repeat_interleave(block, 1).repeat_interleave(block, 2)[:, :H, :W]
    return (img + torch.randint(-noise, noise + 1, (bands, H, W), device=DEV, generator=g)).to(torch.uint8).contiguous()


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slic_mb.txt"))
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args()
    H = W = a.size
    bands, cell, comp, iters = 4, 29, 10, 10
    px, lib, i32 = H * W, _lib.lib(), torch.int32
    tile = block_noise_tile(bands, H, W)
    K = (-(-H // cell)) * (-(-W // cell))
    centres = torch.empty((K, 6), dtype=i32, device=DEV)
    sums = torch.empty((K, 7), dtype=torch.int64, device=DEV)
    assigned = torch.empty((H, W), dtype=i32, device=DEV)

    def iterate(n):
        check(lib.dm_slic_iterate(tile.data_ptr(), bands, H, W, cell, comp, n, centres.data_ptr(), sums.data_ptr(), assigned.data_ptr(),
                                  _stream()), "dm_slic_iterate")
    t_last = ev(lambda: iterate(0), 10)
    t_loop = ev(lambda: iterate(iters), 5)
    t_pass = (t_loop - t_last) / iters

    parent = torch.empty(px, dtype=i32, device=DEV)
    chunks = torch.empty((px + 4095) // 4096 + 1, dtype=i32, device=DEV)
    frag = torch.empty((H, W), dtype=i32, device=DEV)
    n_dev = torch.empty(1, dtype=i32, device=DEV)
    t_ccl = ev(lambda: check(lib.dm_connected_labels(assigned.data_ptr(), H, W, 0, 0, parent.data_ptr(), chunks.data_ptr(), frag.data_ptr(),
                                                     n_dev.data_ptr(), _stream()), "dm_connected_labels"), 10)
    t_ccl_call = ev(lambda: rag.connected_labels(assigned), 5)
    n_frag = int(n_dev)

    min_size = max(1, cell * cell // 4)
    marks = []

    def on_round(r):
        torch.cuda.synchronize()
        marks.append(time.perf_counter())
    rag.absorb_small(frag, n_frag, min_size)                       # warm-up: allocator and code objects
    t_abs, (labels, S, rounds) = wall(lambda: rag.absorb_small(frag, n_frag, min_size, on_round=on_round))
    torch.cuda.synchronize()
    marks.append(time.perf_counter())
    t_rounds = [b - a_ for a_, b in zip(marks[:-1], marks[1:])]

    t_slic = ev(lambda: rag.slic(tile, cell=cell, compactness=comp, iters=iters), 3)
    t_edges = ev(lambda: rag.rag_edges(labels, S), 5)
    t_points = ev(lambda: rag.sample_points(labels, S, k=3), 5)
    t_stats = ev(lambda: rag.label_stats(labels, tile, S), 5)
    area = rag.label_area(labels, S)

    floor_bytes = bands * px
    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"input: {H} x {W} x {bands} uint8, blocks of side 97 + noise +-8; cell {cell}, compactness {comp}, {iters} iterations, "
             f"min_size {min_size}: K = {K} centres, {n_frag} fragments after the components, n_labels = {S} after {rounds} absorption rounds "
             f"(area min {int(area.min())}, median {int(area.median())}, max {int(area.max())})",
             f"(a) iteration pass (assignment + update, ({iters} iterations - 0) / {iters}): {t_pass * 1e6:9.1f} us   "
             f"{floor_bytes / t_pass / 1e9:7.1f} GB/s against the byte floor of {floor_bytes / 1e6:.0f} MB (the tile)",
             f"    last pass (init + assignment + labels written):                {t_last * 1e6:9.1f} us",
             f"    dm_slic_iterate, {iters} iterations:                                {t_loop * 1e6:9.1f} us",
             f"(b) components: dm_connected_labels {t_ccl * 1e6:9.1f} us; rag.connected_labels, whole call {t_ccl_call * 1e6:9.1f} us",
             f"(c) absorption: {rounds} rounds + the round that finds nothing to pick, {t_abs * 1e6:9.1f} us in all (wall, label_area included)"]
    lines += [f"    round {r}: {t * 1e6:9.1f} us" for r, t in enumerate(t_rounds)]
    rest = t_edges + t_points + t_stats
    lines += [f"(d) rag.slic, whole call: {t_slic * 1e6:9.1f} us",
              f"(e) same process, on the SLIC raster: rag_edges {t_edges * 1e6:.1f} us + sample_points {t_points * 1e6:.1f} us + "
              f"label_stats {t_stats * 1e6:.1f} us = {rest * 1e6:.1f} us; rag.slic is {t_slic / rest:.2f} x that"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
