#!/usr/bin/env python3
"""What the feed's augmentations cost: each scale's gather at the headline batch -- 32 pairs = 64 samples, 4
bands, scales 32 / 64 / 128 / 256, window sides drawn as tools/train_synth.py draws them, patch-embed rows in bf16 -- in six forms
that alternate in one session:
  existing   dm_pair_batch_gather
  identity   dm_pair_batch_gather_oriented, every orientation 0
  d4         dm_pair_batch_gather_oriented, orientations uniform in 0..7 (equal on both sides of a pair)
  transpose  dm_pair_batch_gather_oriented, every orientation 4
  radio_id   dm_pair_batch_gather_augmented, the d4 orientations, the identity table (gain 256, offset 0)
  radio      dm_pair_batch_gather_augmented, the d4 orientations, a table drawn by dm_pair_epoch_radiometric at its default spans
Kernel times come from a `rocprofv3 --kernel-trace --stats` run of the worker below (a child process; nothing else is traced): the
worker launches the forms in a known order (rotated by one per repetition, so every form takes every position), and the trace's
dispatches are mapped back by their order.  The session's spread is the difference between the medians of the even and the odd
repetitions of the same form (identical work).

  python tools/mb_augment.py [--reps 40] [--out profiles/radiometric_mb.txt]  kernel times
  python tools/mb_augment.py --train [--train-rounds 2]                       also tools/train_synth.py pairs/s without / with
                                                                              --augment d4 / with --radiometric, run alternately
  python tools/mb_augment.py --train-only                                     the pairs/s alone
(profiles/augment_mb.txt is the four-form run that accepted the oriented entry.)
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
FORMS = ("existing", "identity", "d4", "transpose", "radio_id", "radio")
ORIENTED, RADIO = ("identity", "d4", "transpose"), ("radio_id", "radio")       # the forms that share an entry (one instantiation per scale)
RADIOMETRIC = "0.2,0.1,0.05"
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
    orient["radio_id"] = orient["radio"] = orient["d4"]
    drawn = torch.empty((P, BANDS, 2), dtype=torch.int32, device=TS.DEV)
    ops.pair_epoch_radiometric(0, 0, PAIRS, PAIRS, BANDS, *ops.Radiometric().spans(), drawn)
    radio = {f: None for f in FORMS}
    radio["radio_id"] = torch.tensor([256, 0], dtype=torch.int32, device=TS.DEV).repeat(P, BANDS, 1).contiguous()
    radio["radio"] = drawn
    outs = [torch.empty((P * 64, BANDS * (s // 8) ** 2), dtype=torch.bfloat16, device=TS.DEV) for s in SCALES]
    flag = torch.zeros((1,), dtype=torch.int32, device=TS.DEV)
    torch.cuda.synchronize()
    for rep in range(WARM + reps):
        for i, s in enumerate(SCALES):
            for form in rotated(rep):
                ops.pair_batch_gather(tiles, table.tile_id, table.xy, table.inner, table.obj, i, s, TS.MAX_WINDOW[i], outs[i], grid=8,
                                      error_flag=flag, orient=orient[form], radio=radio[form])
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
    for s in SCALES:            # the mapping by order holds: one instantiation per (scale, entry), the forms of one entry share theirs
        per_entry = [names[(s, "existing")]] + [set().union(*(names[(s, f)] for f in group)) for group in (ORIENTED, RADIO)]
        if not (all(len(n) == 1 for n in per_entry) and len(set().union(*per_entry)) == 3):
            sys.exit(f"mb_augment: scale {s}: the trace's kernel names do not follow the launch order: {names}")
    return times


def report_kernels(times, reps):
    lines = [f"gather kernel times, {PAIRS} pairs = {2 * PAIRS} samples x {BANDS} bands, bf16 patch-embed rows (grid 8), {reps} repetitions after "
             f"{WARM} warm-up, the {len(FORMS)} forms alternating (order rotated per repetition); rocprofv3 --kernel-trace --stats, one traced run",
             "  scale  form        median us    min us    max us   vs existing     vs d4   session spread us (|median even reps - median odd reps|)"]
    verdict = []
    for s in SCALES:
        base, d4 = statistics.median(times[(s, "existing")]), statistics.median(times[(s, "d4")])
        spreads = {}
        for f in FORMS:
            t = times[(s, f)]
            med = statistics.median(t)
            spreads[f] = abs(statistics.median(t[0::2]) - statistics.median(t[1::2]))
            lines.append(f"  {s:5d}  {f:10s} {med / 1e3:10.2f} {min(t) / 1e3:9.2f} {max(t) / 1e3:9.2f}   {med / base:10.3f} {med / d4:9.3f}   {spreads[f] / 1e3:8.2f}")
        # the yardstick of the augmented entry: the oriented entry on the same orientations, + 3 % + this session's own spread
        limit = 1.03 * d4 + max(spreads.values())
        for f in RADIO:
            med = statistics.median(times[(s, f)])
            verdict.append(f"  {s:5d}  {f:10s} {med / 1e3:8.2f} us against 1.03 x d4 + spread = {limit / 1e3:8.2f} us: {'within' if med <= limit else 'OVER'}")
    return lines + ["", "the augmented entry against the oriented entry (d4) of this session, + 3 % + the largest even/odd spread of the scale:"] + verdict


def train_rates(rounds):
    """tools/train_synth.py at its defaults without augmentation / with --augment d4 / with --radiometric, alternately, one child
    process each."""
    variants = {"without either": [], "--augment d4": ["--augment", "d4"], "--radiometric " + RADIOMETRIC: ["--radiometric", RADIOMETRIC]}
    rates = {k: [] for k in variants}
    for _ in range(rounds):
        for k, extra in variants.items():
            cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.join(ROOT, "tools", "train_synth.py"), "--epochs", "2", "--steps-per-epoch", "20"]
            r = subprocess.run(cmd + extra, capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit(f"mb_augment: train_synth ended with {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            rates[k].append(res["pairs_per_s_steady_incl_data_generation"])
            print(f"train_synth {k}: {rates[k][-1]} pairs/s", file=sys.stderr, flush=True)
    width = max(len(k) for k in variants)
    return [f"tools/train_synth.py --epochs 2 --steps-per-epoch 20 (120 pairs per step, depth 6,4,2, bf16), steady pairs/s incl. data generation, "
            f"{rounds} runs each, alternating:"] + [f"  {k:{width}s} : {v}" for k, v in rates.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiometric_mb.txt"))
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--train-only", action="store_true", help="the train_synth.py rates alone, printed and not written to --out")
    ap.add_argument("--train-rounds", type=int, default=2)
    ap.add_argument("--trace-dir", default=None, help="keep rocprofv3's output there")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        worker(a.reps)
        return
    if a.train_only:
        print("\n".join(train_rates(a.train_rounds)))
        return
    lines = ["Dihedral and radiometric augmentation of the training feed (tools/mb_augment.py), one MI355X, one session", ""]
    lines += report_kernels(kernel_times(a.reps, a.trace_dir), a.reps)
    lines += [""] + (train_rates(a.train_rounds) if a.train else ["tools/train_synth.py pairs/s without / with the augmentations: not measured"])
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
