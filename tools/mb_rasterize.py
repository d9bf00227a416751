#!/usr/bin/env python3
"""Cost of rag.rasterize on the config-4 raster: the rings rag.polygons traces from the SLIC superpixels (cell 29, ~20 k labels) of a
4096 x 4096 x 4 uint8 piecewise-constant tile with noise (as tools/mb_slic.py makes it), rasterised back; and on the truth-map shape
of input: 64 polygons of 512 x 512 pixels over the same raster.

  python tools/mb_rasterize.py [--out profiles/rasterize_mb.txt] [--size 4096]

hipEvent time over repeated whole calls (allocations and the three readbacks included), the stages of one run between events, the
number of events N, and the bytes the passes must move: 8 B per event for the emit's write, one read and one write
of the sort (the least an out-of-place sort does; the radix sort behind torch.sort makes several passes) and the fill's read, plus
4 B per raster pixel for the pre-set and 4 B per covered pixel for the integer max.  Beside them, in the same process on the same
raster: rag.polygons, the way there.  The result is compared with the input raster before anything is timed.
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

HBM_BYTES_PER_S = 8e12


def measure(name, labels, S):
    H, W = labels.shape
    polys = rag.polygons(labels, S)
    out = rag.rasterize(polys, H, W)                               # warm-up: allocator and code objects
    if not torch.equal(out, labels):
        raise RuntimeError(f"{name}: rasterize(polygons(labels)) differs from labels in {int((out != labels).sum())} pixels")
    t_polys = ev(lambda: rag.polygons(labels, S), 3)
    t_rast = ev(lambda: rag.rasterize(polys, H, W), 5)
    st = {}
    rag.rasterize(polys, H, W, stats=st)
    N, covered = st["N"], int((out >= 0).sum())
    nbytes = 8 * N * 4 + 4 * H * W + 4 * covered
    bound = nbytes / HBM_BYTES_PER_S
    staged = dict(st["stage_ms"])
    fill_ms = staged["pre-set + fill + readback of the error flag"]
    lines = [f"[{name}] {H} x {W} int32, n_labels = {S}: rings = {st['rings']}, vertices = {st['vertices']}, events N = {N} "
             f"({N / (H * W):.3f} per pixel, mean span {2 * covered / max(N, 1):.1f} px)",
             f"    rag.rasterize {t_rast * 1e3:9.3f} ms   bytes the passes must move {nbytes / 1e6:.0f} MB -> bound {bound * 1e3:.3f} ms at 8 TB/s; "
             f"achieved {nbytes / t_rast / 1e9:.1f} GB/s = {100 * bound / t_rast:.1f} % of the bound's rate",
             f"    rag.polygons  {t_polys * 1e3:9.3f} ms on the same raster (rasterize is {t_rast / t_polys:.2f} x that)",
             "    stages of one run, between events (host work and readbacks fall into the stage they end):"]
    lines += [f"      {stage:48s} {ms:9.3f} ms" for stage, ms in st["stage_ms"]]
    lines += [f"    pixel atomics: pre-set + fill take {fill_ms:.3f} ms of the {sum(staged.values()):.3f} ms staged "
              f"({100 * fill_ms / sum(staged.values()):.0f} %); their bytes ({(4 * H * W + 4 * covered + 8 * N) / 1e6:.0f} MB) at 8 TB/s: "
              f"{(4 * H * W + 4 * covered + 8 * N) / HBM_BYTES_PER_S * 1e3:.3f} ms"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rasterize_mb.txt"))
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args()
    H = W = a.size
    tile = block_noise_tile(4, H, W)
    labels, S = rag.slic(tile, cell=29, compactness=10, iters=10)
    del tile
    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}"]
    lines += measure("superpixels (rag.slic, cell 29)", labels, S)
    y, x = torch.meshgrid(torch.arange(H, device=labels.device) // 512, torch.arange(W, device=labels.device) // 512, indexing="ij")
    grid = (y * ((W + 511) // 512) + x).to(torch.int32).contiguous()
    lines += measure("truth map (512-px grid)", grid, int(grid.max()) + 1)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
