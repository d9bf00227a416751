#!/usr/bin/env python3
"""Cost of the elimination rounds (merge_regions(min_area=)) beside the margin rounds, at the config-4 tile size: tools/mb_merge.py's
4096 x 4096 case (~20 k superpixels, ~60 k edges and sample points, D = 100, margin 1) with the features of 15 % of the superpixels
moved far from every block centre (tests/merge_small_ref.py::add_outliers), so that the margin rounds leave single superpixels.

  python tools/mb_merge_small.py [--out profiles/merge_small_mb.txt] [--against DIR]

All in one session, the two calls alternating, REPS times each, median and min..max of the wall time (host clock around a call that
ends in a device synchronise):
(a) A = merge_regions(min_area=0) and B = merge_regions(min_area=2 cells).  A is p + 1 margin rounds (p applied, one that picks
    nothing); B is the same p + 1 margin rounds and then s + 1 elimination rounds (s applied, one that picks nothing; the first
    reuses the scores).  margin round = A / (p + 1); elimination round = (B - A) / (s + 1): the margin rounds of the same session
    are the yardstick.  The cost falls with the partition, so B is also cut after every round (max_rounds = k, CUTS calls each,
    interleaved): the step from k to k + 1 is round k + 1, a margin or an elimination round, beside the size it worked on.
(b) the launch floor of the session: 2000 dm_merge_accept launches on one edge, back to back, one synchronise; per launch.
(c) rounds and regions for min_area of 1, 2 and 4 SLIC cells (cell = 29: 841 pixels).
(d) with --against DIR (another checkout of the project, built: the parent commit): merge_regions without the keyword there and
    merge_regions(min_area=0) here, in child processes that alternate, PAIRS times; each child reports its median of REPS calls.
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELL, REPS, PAIRS, LATE, CUTS = 29, 15, 3, 4, 7


def load(root):
    for d in (os.path.join(ROOT, "tests"), ROOT, root):            # the package from `root`; the case builders (and the oracle
        sys.path.insert(0, d)                                     # package they import) from this checkout
    import torch
    import merge_ref as M
    import merge_small_ref as MS
    from deepmerge_amd import rag
    dev = "cuda:0"
    c = M.raster_case(4096, 4096, CELL, 3, 4, 100, 2, step=17)
    F = MS.add_outliers(c, 0.15, 2)
    tl, tt = torch.from_numpy(c["labels"]).to(dev), torch.from_numpy(c["tile"]).to(dev)
    ptr, idx = (torch.from_numpy(c[k]).to(dev) for k in ("ptr", "idx"))
    edges, w = rag.rag_edges(tl, c["S"])
    st = rag.label_stats(tl, tt, c["S"])
    return torch, rag, c["S"], (torch.from_numpy(F).to(dev), ptr, idx, edges), dict(weights=w, stats=st)


def wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(ts):
    return f"{statistics.median(ts) * 1e3:.3f} ms (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f}, {len(ts)} calls)"


def child(root, keyword):
    """Median wall time of REPS merge_regions calls in the checkout `root`, as one JSON line."""
    torch, rag, S, args, kw = load(root)
    if keyword:
        kw["min_area"] = 0
    for _ in range(3):
        rag.merge_regions(*args, **kw)
    ts = [wall(torch, lambda: rag.merge_regions(*args, **kw))[0] for _ in range(REPS)]
    print(json.dumps({"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_small_mb.txt"))
    ap.add_argument("--against", default=None, help="another built checkout (the parent commit) to alternate merge_regions with")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--keyword", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.keyword)

    torch, rag, S, args, kw = load(ROOT)
    from deepmerge_amd import _lib
    from deepmerge_amd.ops import _stream, check
    area = 2 * CELL * CELL
    for _ in range(3):                                            # warm-up: allocator, sort workspaces, code objects
        rag.merge_regions(*args, **kw)
        rag.merge_regions(*args, **kw, min_area=area)
    p = rag.merge_regions(*args, **kw).rounds
    ta, tb = [], []
    for _ in range(REPS):
        t, ra = wall(torch, lambda: rag.merge_regions(*args, **kw, min_area=0))
        ta.append(t)
        t, rb = wall(torch, lambda: rag.merge_regions(*args, **kw, min_area=area))
        tb.append(t)
    print(f"(a) timed: A {spread(ta)}, B {spread(tb)}", flush=True)
    s = rb.small_rounds
    assert ra.rounds == p and rb.rounds - s == p and s >= 1 and p > LATE
    ma, mb = statistics.median(ta), statistics.median(tb)
    per_margin, per_small = ma / (p + 1), (mb - ma) / (s + 1)
    cut = [[] for _ in range(rb.rounds + 1)]                       # the same run cut after k rounds: k applied rounds + one scoring
    for _ in range(CUTS):
        for k in range(rb.rounds + 1):
            cut[k].append(wall(torch, lambda: rag.merge_regions(*args, **kw, min_area=area, max_rounds=k))[0])
    cut = [statistics.median(c) for c in cut]
    step = [cut[k + 1] - cut[k] for k in range(rb.rounds)]        # round k + 1 (step[p] also holds the margin round that picked nothing)
    late, small = step[p - LATE:p], step[p + 1:]
    print(f"(a) cut after every round: {len(cut)} x {CUTS} calls", flush=True)

    lib = _lib.lib()
    e1 = torch.tensor([[0, 1]], dtype=torch.int32, device="cuda:0")
    s1 = torch.tensor([0.5], dtype=torch.float32, device="cuda:0")
    c1 = torch.tensor([1, 9], dtype=torch.int64, device="cuda:0")
    b1 = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
    one = (e1.data_ptr(), s1.data_ptr(), 1, 2, c1.data_ptr(), 5, b1.data_ptr(), _stream())

    def launches(n=2000):
        for _ in range(n):
            check(lib.dm_merge_accept(*one), "dm_merge_accept")
    launches(200)
    floor = [wall(torch, launches)[0] / 2000 for _ in range(5)]

    lines = [
        f"box: {socket.gethostname()}  device: {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
        f"input: 4096 x 4096 labels, S = {S} superpixels, E = {args[3].shape[0]} edges, P = {args[2].numel()} points, D = 100, margin 1, "
        f"15 % outlier superpixels; min_area = {area} pixels (2 cells of {CELL} x {CELL})",
        f"(a) A = merge_regions(min_area=0): {spread(ta)}; {p} applied margin rounds ({S} -> {ra.rep.numel()} regions)",
        f"    B = merge_regions(min_area={area}): {spread(tb)}; + {s} applied elimination rounds ({ra.rep.numel()} -> {rb.rep.numel()} regions)",
        f"    margin round = A / {p + 1} = {per_margin * 1e3:.3f} ms;  elimination round = (B - A) / {s + 1} = {per_small * 1e3:.3f} ms "
        f"(the mean margin round is dearer: the early ones score and fold four times as many regions)",
        f"    the same run cut after every round (max_rounds = k, median of {CUTS} calls each; a step = one applied round):",
        "    " + "; ".join(f"{k + 1}{'e' if k >= p else 'm'} {rb.regions_per_round[k]}->{rb.regions_per_round[k + 1]} {step[k] * 1e6:.0f} us"
                           for k in range(rb.rounds)),
        f"    (m = margin round, e = elimination round; step {p + 1} also holds the margin round that picked nothing)",
        f"    last {LATE} margin rounds: {statistics.mean(late) * 1e6:.1f} us per round; elimination rounds {p + 2}..{rb.rounds}: "
        f"{statistics.mean(small) * 1e6:.1f} us per round = those {(statistics.mean(small) - statistics.mean(late)) * 1e6:+.1f} us",
        f"(b) launch floor: {statistics.median(floor) * 1e6:.2f} us per launch (min {min(floor) * 1e6:.2f}, max {max(floor) * 1e6:.2f}; "
        f"2000 one-edge dm_merge_accept launches per sample, 5 samples)",
    ]
    for cells in (1, 2, 4):
        r = rag.merge_regions(*args, **kw, min_area=cells * CELL * CELL)
        lines.append(f"(c) min_area = {cells} cell(s) = {cells * CELL * CELL} pixels: {r.rounds - r.small_rounds} margin + {r.small_rounds} elimination "
                     f"rounds, {r.regions_per_round[r.rounds - r.small_rounds]} -> {r.rep.numel()} regions, smallest region left "
                     f"{int(r.stats['count'][r.stats['count'] > 0].min())} pixels")
    if a.against:
        here, there = [], []
        for _ in range(PAIRS):
            for root, key, into in ((a.against, False, there), (ROOT, True, here)):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", root] + (["--keyword"] if key else [])
                out = subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=300).stdout.strip().splitlines()[-1]
                into.append(json.loads(out)["median_ms"])
                print(f"(d) {'here' if key else 'there'}: {into[-1]:.3f} ms", flush=True)
        lines.append(f"(d) merge_regions() in {os.path.basename(os.path.abspath(a.against))} (no min_area keyword) vs merge_regions(min_area=0) "
                     f"here, {PAIRS} alternating processes each, median of {REPS} calls per process: "
                     f"there {', '.join(f'{t:.3f}' for t in there)} ms; here {', '.join(f'{t:.3f}' for t in here)} ms")
    else:
        lines.append("(d) not run: no --against checkout given")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
