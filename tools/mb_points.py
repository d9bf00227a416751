#!/usr/bin/env python3
"""Cost of deriving sample points from a label raster at the config-4r tile size: 4096 x 4096 labels, jittered Voronoi with
cell 29 (workload.voronoi_raster, ~20 k superpixels), k = 3, max_window = 384; and the worst case for the clearance column pass,
one label filling the raster (every pixel away from the edge visits cap = 192 rows up and down).

  python tools/mb_points.py [--out profiles/points_mb.txt]

Per pass: hipEvent time over 20 calls that rotate through 4 label rasters with their own clearance rasters (256 MiB of labels
+ 128 MiB of clearance, so that no call finds its input in the 256 MiB Infinity Cache), and GB/s against the algorithmic bytes:
  clearance       4 B read + 2 B written per pixel (the bit plane and the row distances are scratch on top: 1/8 + 1 B written, 1/8 B +
                  the column pass's re-reads of 1 B rows read)
  selection round 6 B per pixel (4 B label + 2 B clearance)
  emit            independent of the raster: S * k rows
Beside them, in the same process: rag.label_stats / rag.rag_edges on the same raster (as config4r times them), the stream rate of
dm_relabel_raster (8 B per pixel), and the whole rag.sample_points call (allocations and its one readback included).
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmerge_amd import _lib, rag  # noqa: E402
from deepmerge_amd.ops import _stream, check  # noqa: E402
from deepmerge_amd.workload import ev, voronoi_raster  # noqa: E402

DEV = "cuda:0"
ENCODER_S_PER_TILE = 2.0


def ev_rot(fn, n=4, iters=20):
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i % n)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def passes(rasters, S, k, mw):
    """Per-pass seconds on pre-allocated buffers (the entry points as rag.sample_points calls them)."""
    lib = _lib.lib()
    H, W = rasters[0].shape
    dev, i32 = rasters[0].device, torch.int32
    bits = torch.empty(H * ((W + 63) // 64), dtype=torch.int64, device=dev)
    rowd = torch.empty((H, W), dtype=torch.uint8, device=dev)
    clr = [torch.empty((H, W), dtype=torch.uint16, device=dev) for _ in rasters]
    best = torch.empty(S, dtype=torch.int64, device=dev)
    pts, pclr = torch.empty((S, k, 2), dtype=i32, device=dev), torch.empty((S, k), dtype=i32, device=dev)
    cnt, bbox = torch.empty(S, dtype=i32, device=dev), torch.empty((S, 4), dtype=i32, device=dev)
    ptr, xy = torch.empty(S + 1, dtype=i32, device=dev), torch.empty((S * k, 2), dtype=i32, device=dev)
    label, inner, obj, rnd = (torch.empty(S * k, dtype=i32, device=dev) for _ in range(4))

    def clear(i):
        check(lib.dm_label_clearance(rasters[i].data_ptr(), H, W, mw, bits.data_ptr(), rowd.data_ptr(), clr[i].data_ptr(), _stream()), "clearance")

    def select(j):
        def run(i):
            check(lib.dm_point_select_round(rasters[i].data_ptr(), clr[i].data_ptr(), H, W, S, k, j, best.data_ptr(), pts.data_ptr(),
                                            pclr.data_ptr(), cnt.data_ptr(), bbox.data_ptr(), _stream()), "select")
        return run

    def emit(_i):
        check(lib.dm_point_emit(cnt.data_ptr(), pts.data_ptr(), pclr.data_ptr(), bbox.data_ptr(), S, k, mw, S * k, ptr.data_ptr(), xy.data_ptr(),
                                label.data_ptr(), inner.data_ptr(), obj.data_ptr(), rnd.data_ptr(), _stream()), "emit")
    out = {"clearance": ev_rot(clear)}
    for j in range(k):                                            # round j needs rounds < j of the same raster: the rasters are equal
        out[f"select round {j}"] = ev_rot(select(j))
    out["emit"] = ev_rot(emit)
    return out, int(ptr[S])


def report(name, t, px, k):
    lines = []
    for key, sec in t.items():
        if key == "clearance":
            lines.append(f"  {key:16s} {sec * 1e6:9.1f} us   {6.0 * px / sec / 1e9:7.1f} GB/s (6 B/pixel)")
        elif key.startswith("select"):
            lines.append(f"  {key:16s} {sec * 1e6:9.1f} us   {6.0 * px / sec / 1e9:7.1f} GB/s (6 B/pixel)")
        else:
            lines.append(f"  {key:16s} {sec * 1e6:9.1f} us")
    lines.append(f"  {'sum of passes':16s} {sum(t.values()) * 1e6:9.1f} us")
    return [name] + lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_mb.txt"))
    a = ap.parse_args()
    torch.manual_seed(0)
    H = W = 4096
    k, mw, px = 3, 384, 4096 * 4096
    lab, _cy, _cx, S = voronoi_raster(H, W, 29)
    tile = torch.randint(0, 256, (4, H, W), dtype=torch.uint8, device=DEV)
    rasters = [lab] + [lab.clone() for _ in range(3)]
    t_v, P = passes(rasters, S, k, mw)
    t_all = ev(lambda: rag.sample_points(lab, S, k=k), 10)
    t_stats = ev(lambda: rag.label_stats(lab, tile, S), 10)
    t_edges = ev(lambda: rag.rag_edges(lab, S), 10)
    ident = torch.arange(S, dtype=torch.int32, device=DEV)
    t_rel = ev_rot(lambda i: rag.relabel_raster(rasters[i], ident))
    pts = rag.sample_points(lab, S, k=k)
    c0 = (pts.inner[pts.round == 0] + 1) // 2
    flat = [torch.zeros((H, W), dtype=torch.int32, device=DEV) for _ in range(4)]
    t_w, P_w = passes(flat, 1, k, mw)

    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"input: 4096 x 4096 labels, jittered Voronoi cell 29, S = {S} superpixels, k = {k}, max_window = {mw}: P = {P} points, "
             f"clearance at point 0: median {int(c0.median())}, min {int(c0.min())}, max {int(c0.max())}"]
    lines += report("(a) per pass, 4 rasters rotated (hipEvent, 20 calls):", t_v, px, k)
    lines += [f"(b) rag.sample_points, whole call (allocations + one readback): {t_all * 1e6:.1f} us = "
              f"{100 * t_all / ENCODER_S_PER_TILE:.3f} % of the {ENCODER_S_PER_TILE:.1f} s the encoder takes per tile",
              f"(c) same process, same raster: label_stats {t_stats * 1e6:.1f} us ({7.0 * px / t_stats / 1e9:.1f} GB/s at 7 B/pixel), "
              f"rag_edges {t_edges * 1e6:.1f} us ({4.0 * px / t_edges / 1e9:.1f} GB/s at 4 B/pixel), "
              f"relabel_raster {t_rel * 1e6:.1f} us ({8.0 * px / t_rel / 1e9:.1f} GB/s at 8 B/pixel, rotated)"]
    lines += report(f"(d) worst case, one label fills the raster (S = 1, P = {P_w}; the column pass visits 2 x 191 rows per pixel):", t_w, px, k)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
