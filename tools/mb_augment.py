#!/usr/bin/env python3
"""What the feed's dihedral augmentation costs: each scale's gather at the headline batch -- 32 pairs = 64 samples, 4
bands, scales 32 / 64 / 128 / 256, window sides drawn as tools/train_synth.py draws them, patch-embed rows in bf16 -- in four forms
that alternate in one session:
  existing   dm_pair_batch_gather
  identity   dm_pair_batch_gather_oriented, every orientation 0
  d4         dm_pair_batch_gather_oriented, orientations uniform in 0..7 (equal on both sides of a pair)
  transpose  dm_pair_batch_gather_oriented, every orientation 4
Kernel times come from a `rocprofv3 --kernel-trace --stats` run of the worker below (a child process; nothing else is traced): the
worker launches the forms in a known order (rotated by one per repetition, so every form takes every position), and the trace's
dispatches are mapped back by their order.  The session's spread is the difference between the medians of the even and the odd
repetitions of the same form (identical work).

  python tools/mb_augment.py [--reps 40] [--out profiles/augment_mb.txt]      kernel times
  python tools/mb_augment.py --train [--train-rounds 2]                       also tools/train_synth.py pairs/s without / with
                                                                              --augment d4, run alternately
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("existing", "identity", "d4", "transpose")
SCALES, BANDS, PAIRS, WARM = [32, 64, 128, 256], 4, 32, 3


def rotated(rep):
    """The order of the forms in repetition `rep`: rotated by one each time, so that every form takes every position (the first gather
    after another scale's finds less of its tiles in L2 than the three that follow it)."""
    k = rep % len(FORMS)
    return FORMS[k:] + FORMS[:k]


def worker(reps):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_synth as TS
    from deepmerge_amd import ops
    g = torch.Generator(device=TS.DEV); g.manual_seed(0)
    tiles = TS.smooth_tiles(6, BANDS, 1024, g)
    table = TS.pair_table(TS.draw_pairs(6, 1024, PAIRS, g))
    P = 2 * PAIRS
    half = torch.randint(0, 8, (PAIRS,), generator=g, device=TS.DEV).to(torch.int32)
    orient = {"existing": None, "identity": torch.zeros(P, dtype=torch.int32, device=TS.DEV), "d4": torch.cat((half, half)),
              "transpose": torch.full((P,), 4, dtype=torch.int32, device=TS.DEV)}
    outs = [torch.empty((P * 64, BANDS * (s // 8) ** 2), dtype=torch.bfloat16, device=TS.DEV) for s in SCALES]
    flag = torch.zeros((1,), dtype=torch.int32, device=TS.DEV)
    torch.cuda.synchronize()
    for rep in range(WARM + reps):
        for i, s in enumerate(SCALES):
            for form in rotated(rep):
                ops.pair_batch_gather(tiles, table.tile_id, table.xy, table.inner, table.obj, i, s, TS.MAX_WINDOW[i], outs[i], grid=8,
                                      error_flag=flag, orient=orient[form])
        torch.cuda.synchronize()
    if int(flag.item()) != 0:
        sys.exit("mb_augment worker: the gather flagged a sample")
    print("WORKER done", flush=True)


def kernel_times(reps, trace_dir=None):
    """{(scale, form): [ns per repetition]} from a traced run of the worker (the trace is kept when trace_dir is given)."""
    with tempfile.TemporaryDirectory() as tmp:
        d = trace_dir or tmp
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--worker", "--reps", str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0 or "WORKER done" not in r.stdout:
            sys.exit(f"mb_augment: the traced worker ended with {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
    rows = [x for x in rows if "patch_pyramid_kernel" in x["Kernel_Name"]]
    rows.sort(key=lambda x: int(x["Dispatch_Id"]))
    per_rep = len(SCALES) * len(FORMS)
    if len(rows) != (WARM + reps) * per_rep:
        sys.exit(f"mb_augment: {len(rows)} gather dispatches in the trace, expected {(WARM + reps) * per_rep}")
    times = {(s, f): [] for s in SCALES for f in FORMS}
    names = {(s, f): set() for s in SCALES for f in FORMS}
    for k, x in enumerate(rows[WARM * per_rep:]):
        s, f = SCALES[(k % per_rep) // len(FORMS)], rotated(WARM + k // per_rep)[k % len(FORMS)]
        times[(s, f)].append(int(x["End_Timestamp"]) - int(x["Start_Timestamp"]))
        names[(s, f)].add(x["Kernel_Name"])
    for s in SCALES:            # the mapping by order holds: one instantiation per (scale, entry), the new entry's three forms share theirs
        new = names[(s, "identity")]
        if not (len(names[(s, "existing")]) == len(new) == 1 and new == names[(s, "d4")] == names[(s, "transpose")]):
            sys.exit(f"mb_augment: scale {s}: the trace's kernel names do not follow the launch order: {names}")
    return times


def report_kernels(times, reps):
    lines = [f"gather kernel times, {PAIRS} pairs = {2 * PAIRS} samples x {BANDS} bands, bf16 patch-embed rows (grid 8), {reps} repetitions after "
             f"{WARM} warm-up, the four forms alternating (order rotated per repetition); rocprofv3 --kernel-trace --stats, one traced run",
             "  scale  form        median us    min us    max us   vs existing   session spread us (|median even reps - median odd reps|)"]
    for s in SCALES:
        base = statistics.median(times[(s, "existing")])
        for f in FORMS:
            t = times[(s, f)]
            med = statistics.median(t)
            spread = abs(statistics.median(t[0::2]) - statistics.median(t[1::2]))
            lines.append(f"  {s:5d}  {f:10s} {med / 1e3:10.2f} {min(t) / 1e3:9.2f} {max(t) / 1e3:9.2f}   {med / base:10.3f}   {spread / 1e3:8.2f}")
    return lines


def train_rates(rounds):
    """tools/train_synth.py at its defaults without / with --augment d4, alternately, one child process each."""
    rates = {None: [], "d4": []}
    for _ in range(rounds):
        for aug in (None, "d4"):
            cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.join(ROOT, "tools", "train_synth.py"), "--epochs", "2", "--steps-per-epoch", "20"]
            r = subprocess.run(cmd + (["--augment", aug] if aug else []), capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit(f"mb_augment: train_synth ended with {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            rates[aug].append(res["pairs_per_s_steady_incl_data_generation"])
    return [f"tools/train_synth.py --epochs 2 --steps-per-epoch 20 (120 pairs per step, depth 6,4,2, bf16), steady pairs/s incl. data generation, "
            f"{rounds} runs each, alternating:",
            f"  without --augment : {rates[None]}",
            f"  --augment d4      : {rates['d4']}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_mb.txt"))
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--train-rounds", type=int, default=2)
    ap.add_argument("--trace-dir", default=None, help="keep rocprofv3's output there")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        worker(a.reps)
        return
    lines = ["Dihedral augmentation of the training feed (tools/mb_augment.py), one MI355X, one session", ""]
    lines += report_kernels(kernel_times(a.reps, a.trace_dir), a.reps)
    lines += [""] + (train_rates(a.train_rounds) if a.train else ["tools/train_synth.py pairs/s without / with --augment d4: not measured"])
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
