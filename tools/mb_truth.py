#!/usr/bin/env python3
"""Cost of the overlap table of a label raster with a ground-truth raster at the config-4r tile size: 4096 x 4096 labels, jittered
Voronoi with cell 29 (workload.voronoi_raster, ~20 k superpixels) against a truth raster of cell 120 (~1.2 k objects) with an
unlabelled band.

  python tools/mb_truth.py [--out profiles/truth_mb.txt]

(a) dm_label_overlap on pre-allocated buffers: hipEvent time over 20 calls that rotate through 4 (labels, truth) pairs = 512 MiB,
    so that no call finds its input in the 256 MiB Infinity Cache; GB/s against the algorithmic 8 B per pixel.
(b) in the same process, the yardsticks: rag.label_stats (7 B/pixel), rag.rag_edges (4 B/pixel) as config4r times them, and the
    stream rate of dm_relabel_raster (8 B/pixel, rotated).
(c) the small passes: dm_overlap_reduce over the K cells, dm_pair_flags over the E edges; rag.label_overlap as called (allocations,
    sort, reduce, one readback).
(d) scoring a merged partition per round: Overlap.coarsen(map).scores() against the rescan relabel_raster + label_overlap + scores,
    for maps that halve the number of regions round by round.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "truth_mb.txt"))
    a = ap.parse_args()
    torch.manual_seed(0)
    H = W = 4096
    px = H * W
    lab, _cy, _cx, S = voronoi_raster(H, W, 29)
    tru, _cy, _cx, G = voronoi_raster(H, W, 120)
    tru[1000:1040, :] = -1                                        # an unlabelled band
    tile = torch.randint(0, 256, (4, H, W), dtype=torch.uint8, device=DEV)
    labs, trus = [lab] + [lab.clone() for _ in range(3)], [tru] + [tru.clone() for _ in range(3)]
    lib, i32, i64 = _lib.lib(), torch.int32, torch.int64
    max_cells = max(1024, 8 * S)
    log2 = max(10, (4 * max_cells - 1).bit_length())
    tk, tc = torch.empty(1 << log2, dtype=i64, device=DEV), torch.empty(1 << log2, dtype=i32, device=DEV)
    ck, cc = torch.empty(max_cells, dtype=i64, device=DEV), torch.empty(max_cells, dtype=i32, device=DEV)
    meta = torch.empty(2, dtype=i32, device=DEV)

    def overlap(i):
        check(lib.dm_label_overlap(labs[i].data_ptr(), trus[i].data_ptr(), H, W, S, G, tk.data_ptr(), tc.data_ptr(), log2, ck.data_ptr(),
                                   cc.data_ptr(), max_cells, meta.data_ptr(), meta[1:].data_ptr(), _stream()), "dm_label_overlap")
    t_ov = ev_rot(overlap)
    K, overflow = meta.tolist()
    assert not overflow and K <= max_cells

    t_stats = ev(lambda: rag.label_stats(lab, tile, S), 10)
    t_edges = ev(lambda: rag.rag_edges(lab, S), 10)
    ident = torch.arange(S, dtype=i32, device=DEV)
    t_rel = ev_rot(lambda i: rag.relabel_raster(labs[i], ident))

    ov = rag.label_overlap(lab, tru, S, G)
    edges, _ = rag.rag_edges(lab, S)
    E = edges.shape[0]
    keys = ov.cells[:, 0].long() * (G + 1) + ov.cells[:, 1].long()
    best, rows, area, size, summ = (torch.empty(n, dtype=i64, device=DEV) for n in (S, S, S, G, 8))
    owner, oc, cover = (torch.empty(n, dtype=i32, device=DEV) for n in (S, S, G))
    flags = torch.empty(E, dtype=torch.int8, device=DEV)
    t_red = ev(lambda: check(lib.dm_overlap_reduce(keys.data_ptr(), ov.count.data_ptr(), K, S, G, best.data_ptr(), rows.data_ptr(), area.data_ptr(),
                                                   owner.data_ptr(), oc.data_ptr(), size.data_ptr(), cover.data_ptr(), summ.data_ptr(), _stream()),
                             "dm_overlap_reduce"), 20)
    t_fl = ev(lambda: check(lib.dm_pair_flags(edges.data_ptr(), E, area.data_ptr(), owner.data_ptr(), oc.data_ptr(), S, 600, flags.data_ptr(),
                                              _stream()), "dm_pair_flags"), 20)
    t_all = ev(lambda: rag.label_overlap(lab, tru, S, G), 10)
    f = rag.pair_flags(edges, ov, 0.6)
    sc = ov.scores()

    lines = [f"device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             f"input: 4096 x 4096, labels jittered Voronoi cell 29 (S = {S}), truth cell 120 with a 40-row unlabelled band (G = {G}): "
             f"K = {K} cells, E = {E} edges; at min_purity 0.6: {int((f == 1).sum())} merge / {int((f == 0).sum())} keep / "
             f"{int((f == -1).sum())} ambiguous; asa {sc.asa:.4f} coverage {sc.coverage:.4f} ARI {sc.adjusted_rand:.4f}",
             f"(a) dm_label_overlap, 4 raster pairs rotated (hipEvent, 20 calls): {t_ov * 1e6:.1f} us = {8.0 * px / t_ov / 1e9:.1f} GB/s at 8 B/pixel",
             f"(b) same process: label_stats {t_stats * 1e6:.1f} us ({7.0 * px / t_stats / 1e9:.1f} GB/s at 7 B/pixel), "
             f"rag_edges {t_edges * 1e6:.1f} us ({4.0 * px / t_edges / 1e9:.1f} GB/s at 4 B/pixel), "
             f"relabel_raster {t_rel * 1e6:.1f} us ({8.0 * px / t_rel / 1e9:.1f} GB/s at 8 B/pixel, rotated); "
             f"label_stats + rag_edges = {(t_stats + t_edges) * 1e6:.1f} us",
             f"(c) dm_overlap_reduce (K = {K}) {t_red * 1e6:.1f} us, dm_pair_flags (E = {E}) {t_fl * 1e6:.1f} us, "
             f"rag.label_overlap whole call (allocations, sort, reduce, one readback) {t_all * 1e6:.1f} us",
             "(d) score of a merged partition, per round (map = superpixel id // 2^r):"]
    for r in (1, 2, 4, 8):
        mapping = (ident // (1 << r)).to(i32)
        C = int(mapping.max()) + 1
        t_co = ev(lambda: ov.coarsen(mapping).scores(), 10)
        t_re = ev(lambda: rag.label_overlap(rag.relabel_raster(lab, mapping), tru, C, G, max_cells=max_cells).scores(), 10)
        got, want = ov.coarsen(mapping).scores(), rag.label_overlap(rag.relabel_raster(lab, mapping), tru, C, G, max_cells=max_cells).scores()
        assert got == want
        lines.append(f"  r = {r}: C = {C:6d}  coarsen + scores {t_co * 1e6:8.1f} us   rescan (relabel + overlap + scores) {t_re * 1e6:8.1f} us   "
                     f"asa {got.asa:.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
