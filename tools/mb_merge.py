#!/usr/bin/env python3
"""Cost of region merging at the config-4 tile size: 4096 x 4096 labels, ~20 k superpixels, ~60 k edges and sample points,
one feature centre per 4 x 4 superpixels (+ 0.05 noise, D = 100, margin 1; tests/merge_ref.py::raster_case).

  python tools/mb_merge.py [--out profiles/merge_mb.txt]

(a) one full rag.merge_regions run (weights + statistics carried) and its mean per scoring round, best of 3;
(b) MergeResult.labels() on the 64 MiB raster: hipEvent time over 20 calls that rotate through 4 raster pairs (512 MiB, so that
    no call finds its input in the 256 MiB Infinity Cache), bytes = 8 per pixel, fraction of the 6.3 TB/s a float4 copy sustains;
(c) in the same process, one round of the threshold rule on the round-1 inputs: rag_similarity_sweep + merge_components +
    merge_partition, best of 3.
"""
import argparse
import os
import socket
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import merge_ref as M  # noqa: E402
from deepmerge_amd import rag  # noqa: E402
from deepmerge_amd.ExtractFeatures import rag_similarity_sweep  # noqa: E402

DEV = "cuda:0"
HBM_SUSTAINED = 6.3e12


def wall(fn, reps=3):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_mb.txt"))
    a = ap.parse_args()
    c = M.raster_case(4096, 4096, 29, 3, 4, 100, 2, step=17)
    S = c["S"]
    tl = torch.from_numpy(c["labels"]).to(DEV)
    tt = torch.from_numpy(c["tile"]).to(DEV)
    F, ptr, idx = (torch.from_numpy(c[k]).to(DEV) for k in ("F", "ptr", "idx"))
    edges, w = rag.rag_edges(tl, S)
    st = rag.label_stats(tl, tt, S)
    rag.merge_regions(F, ptr, idx, edges, weights=w, stats=st)                      # warm-up (allocator, sort workspaces)

    t_full, res = wall(lambda: rag.merge_regions(F, ptr, idx, edges, weights=w, stats=st))
    scored = res.rounds + 1                                                          # the last scoring round picks nothing
    rasters = [tl.clone() for _ in range(4)]
    for r in rasters:
        res.labels(r)
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for i in range(20):
        res.labels(rasters[i & 3])
    end.record()
    torch.cuda.synchronize()
    t_lab = beg.elapsed_time(end) * 1e-3 / 20
    bw = 8.0 * tl.numel() / t_lab

    def threshold_round():
        pooled, simi, merge = rag_similarity_sweep(F, ptr, idx, edges, margin=1.0)
        root = rag.merge_components(edges, merge, S)
        return rag.merge_partition(ptr, idx, edges, root)
    threshold_round()
    t_old, old = wall(threshold_round)

    lines = [
        f"box: {socket.gethostname()}  device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
        f"input: 4096 x 4096 labels, S = {S} superpixels, E = {edges.shape[0]} edges, P = {idx.numel()} points, D = 100, margin 1",
        f"(a) merge_regions: {t_full * 1e3:.2f} ms for {res.rounds} applied rounds ({S} -> {res.ptr.numel() - 1} regions), "
        f"{t_full * 1e3 / scored:.3f} ms per scoring round ({scored} of them, one readback each)",
        f"(b) labels(): {t_lab * 1e6:.1f} us per 4096 x 4096 raster = {bw / 1e12:.2f} TB/s = {100 * bw / HBM_SUSTAINED:.0f} % of the 6.3 TB/s "
        f"a float4 copy sustains",
        f"(c) threshold rule, one round on the round-1 inputs (sweep + merge_components + merge_partition): {t_old * 1e3:.3f} ms "
        f"({S} -> {old[1].numel() - 1} regions in that one round)",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
