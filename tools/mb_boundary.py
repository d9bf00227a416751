#!/usr/bin/env python3
"""Cost of rag.boundary_scores on the config-4 raster: the SLIC superpixels (cell 29, ~20 k labels) of a 4096 x 4096 x 4 uint8
piecewise-constant tile with noise (as tools/mb_slic.py makes it) against a truth raster (jittered Voronoi, cell 120, with a 40-row
unlabelled band, as tools/mb_truth.py makes it); and of scene.boundary_scores on that pair laid out 2 x 2 as an 8192 x 8192 scene
in four tiles.

  python tools/mb_boundary.py [--out profiles/boundary_mb.txt] [--size 4096]

(a) the launches alone on buffers allocated once, 40 calls that rotate through 4 raster pairs (512 MiB, more than the Infinity
    Cache) captured in one hipGraph and replayed (so that the host's enqueue rate is not in the figure): the bits pass of
    both rasters (8 H W bytes read, the rate as a fraction of 8 TB/s), with and without a mapping, and the count pass per tolerance.
(b) the whole calls, alternating in one session, the median of 5 rounds: rag.boundary_scores at d = 2 and at d = 2, 4, 8, 16
    together, beside rag.label_overlap and rag.clearance on the same rasters (the two calls that make one pass over a label raster).
(c) scene.boundary_scores on the 8192 x 8192 scene from host memory, its stages as wall time.
The whole-raster result is compared with the scene's before anything is reported.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from deepmerge_amd import _lib, rag, scene  # noqa: E402
from deepmerge_amd.ops import _stream, check  # noqa: E402
from deepmerge_amd.workload import ev, voronoi_raster  # noqa: E402
from mb_slic import block_noise_tile  # noqa: E402
from mb_truth import ev_rot  # noqa: E402

HBM_BYTES_PER_S = 8e12
DEV = "cuda:0"


def replay_time(launch, n=4, iters=40, reps=5):
    """Device time per call: launch(i % n) captured `iters` times into one hipGraph, hipEvent time of a replay, best of `reps`.
    (The launches of this file run for tens of microseconds: the replay takes the host's enqueue rate out of the figure.)"""
    for i in range(n):
        launch(i)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        launch(0)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            for i in range(iters):
                launch(i % n)
    graph.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / iters * 1e-3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_mb.txt"))
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args()
    torch.manual_seed(0)
    H = W = a.size
    px = H * W
    lab, S = rag.slic(block_noise_tile(4, H, W), cell=29, compactness=10, iters=10)
    tru, _cy, _cx, G = voronoi_raster(H, W, 120)
    tru[H // 4:H // 4 + 40, :] = -1                                # an unlabelled band
    lib, i64 = _lib.lib(), torch.int64
    labs, trus = [lab] + [lab.clone() for _ in range(3)], [tru] + [tru.clone() for _ in range(3)]
    WW = (W + 63) // 64
    le, te, tv = (torch.empty((H, WW), dtype=i64, device=DEV) for _ in range(3))
    ident = torch.arange(S, dtype=torch.int32, device=DEV)
    counts = torch.zeros(4, dtype=i64, device=DEV)

    def bits(i, mapping=None):
        check(lib.dm_boundary_bits(labs[i].data_ptr(), H, W, S, mapping.data_ptr() if mapping is not None else None, le.data_ptr(), None,
                                   _stream()), "dm_boundary_bits")
        check(lib.dm_boundary_bits(trus[i].data_ptr(), H, W, G, None, te.data_ptr(), tv.data_ptr(), _stream()), "dm_boundary_bits")

    def count(d):
        check(lib.dm_boundary_counts(le.data_ptr(), te.data_ptr(), tv.data_ptr(), H, W, d, 0, H, 0, W, counts.data_ptr(), _stream()),
              "dm_boundary_counts")

    t_bits_host = ev_rot(bits)
    t_bits = replay_time(bits)
    t_bits_map = replay_time(lambda i: bits(i, ident))
    t_count = {d: replay_time(lambda i: count(d)) for d in (0, 2, 4, 8, 16, 64)}

    calls = {"rag.boundary_scores, d = 2": lambda: rag.boundary_scores(lab, tru, S, G, 2),
             "rag.boundary_scores, d = 2, 4, 8, 16": lambda: rag.boundary_scores(lab, tru, S, G, [2, 4, 8, 16]),
             "rag.label_overlap": lambda: rag.label_overlap(lab, tru, S, G),
             "rag.clearance": lambda: rag.clearance(lab)}
    times = {k: [] for k in calls}
    for _ in range(5):                                             # alternating: every round times every call
        for k, fn in calls.items():
            times[k].append(ev(fn, 5))
    sc = rag.boundary_scores(lab, tru, S, G, [2, 4, 8, 16])

    lab2 = np.empty((2 * H, 2 * W), np.int32)
    tru2 = np.empty((2 * H, 2 * W), np.int32)
    lab_h, tru_h = lab.cpu().numpy(), tru.cpu().numpy()
    for q, (y, x) in enumerate(((0, 0), (0, W), (H, 0), (H, W))):
        lab2[y:y + H, x:x + W] = lab_h + q * S
        tru2[y:y + H, x:x + W] = np.where(tru_h >= 0, tru_h + q * G, -1)
    scene.boundary_scores(lab2, tru2, 4 * S, 4 * G, 2, tile=a.size)          # warm-up
    st = {}
    torch.cuda.synchronize()
    got = scene.boundary_scores(lab2, tru2, 4 * S, 4 * G, 2, tile=a.size, stage_times=st)
    if H * W * 4 < 1 << 31:                                        # the scene as one raster, where it fits one: the definition
        want = rag.boundary_scores(torch.from_numpy(lab2).to(DEV), torch.from_numpy(tru2).to(DEV), 4 * S, 4 * G, 2)
        if got != want:
            raise RuntimeError(f"scene.boundary_scores differs from the whole-raster call: {got} != {want}")

    bound = 8.0 * px / HBM_BYTES_PER_S
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"input: {H} x {W}, labels rag.slic cell 29 (S = {S}), truth jittered Voronoi cell 120 with a 40-row unlabelled band (G = {G})",
             "scores: " + "; ".join(f"d = {s.tolerance}: recall {s.recall:.4f} precision {s.precision:.4f} F {s.f:.4f} "
                                    f"({s.hit_truth}/{s.n_truth_b}, {s.hit_label}/{s.n_label_b})" for s in sc),
             f"(a) launches alone, 4 raster pairs rotated, 40 calls captured in one hipGraph, best of 5 replays; 8 H W = {8 * px / 1e6:.0f} MB -> "
             f"{bound * 1e6:.1f} us at 8 TB/s (enqueued from Python, hipEvent over 20 calls: {t_bits_host * 1e6:.1f} us per call):",
             f"    bits pass, both rasters             {t_bits * 1e6:9.1f} us = {8.0 * px / t_bits / 1e9:7.1f} GB/s = {100 * bound / t_bits:.1f} % of 8 TB/s",
             f"    bits pass, labels through a mapping {t_bits_map * 1e6:9.1f} us = {8.0 * px / t_bits_map / 1e9:7.1f} GB/s = "
             f"{100 * bound / t_bits_map:.1f} % of 8 TB/s"]
    lines += [f"    count pass, d = {d:2d}                    {t * 1e6:9.1f} us" for d, t in t_count.items()]
    lines += ["(b) whole calls (allocations and readbacks included), alternating, median of 5 rounds of 5 calls (min .. max):"]
    lines += [f"    {k:40s} {med[k] * 1e6:9.1f} us  ({min(times[k]) * 1e6:.1f} .. {max(times[k]) * 1e6:.1f})" for k in calls]
    lines += [f"    per byte of raster read: boundary_scores d = 2 is {med['rag.boundary_scores, d = 2'] / med['rag.label_overlap']:.2f} x "
              f"label_overlap (both read 8 B per pixel)",
              f"(c) scene.boundary_scores, {2 * H} x {2 * W} from host memory in 4 tiles of {a.size}, d = 2 (halo 3), wall time per stage:"]
    total = sum(st.values())
    lines += [f"    {stage:40s} {t * 1e3:9.3f} ms  {100 * t / total:5.1f} %" for stage, t in st.items()]
    lines += [f"    {'total':40s} {total * 1e3:9.3f} ms;  recall {got.recall:.4f} precision {got.precision:.4f} F {got.f:.4f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
