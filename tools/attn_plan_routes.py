"""Which kernels the attention entry points launch, per environment (MI355X; the table of profiles/attn_plan_routes.txt).

    python tools/attn_plan_routes.py [--lib PATH] > routes.txt

For every environment of tools/attn_plan_queries.py ENVS, in a child process of its own (the DM_ATTN_* switches are read once), one
forward and one backward at each of CALLS run under `rocprofv3 --kernel-trace` (nothing else traced); printed per call: the kernel
names with their template arguments, grid and block sizes and LDS bytes as the trace has them.  Two libraries route alike when their
outputs are equal (`diff`).  Every child has its own time limit; the first child that fails ends the run, nothing is started again.

The worker uses the C ABI and the HIP runtime through ctypes only (no torch: a child starts in a second).  Tensors are zeros -- the
route does not depend on the data.  A one-row dm_split_bf16 launch in front of every entry-point call marks the trace.
"""
import argparse
import csv
import ctypes as C
import glob
import importlib.util
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from attn_plan_queries import ENVS, env_name  # noqa: E402

BF16, F32 = 1, 0
# (B, N, H, D, dtype, bias): table = relative-position table only, dense = [H, N, N] rows (+ transposed copy), both (backward only:
# the forward of such a module ran on the dense rows), none; split: the bf16x3 entry points, with a table or without.
CALLS = [(64, 256, 12, 64, BF16, "table"), (64, 256, 12, 64, BF16, "dense"), (64, 256, 12, 64, BF16, "both"), (64, 256, 12, 64, BF16, "none"),
         (64, 192, 12, 64, BF16, "table"), (256, 197, 12, 64, BF16, "none"), (64, 193, 12, 64, BF16, "dense"), (2, 256, 12, 64, BF16, "dense"),
         (2, 256, 12, 64, BF16, "table"), (64, 128, 12, 64, BF16, "dense"), (64, 64, 12, 64, BF16, "dense"), (64, 256, 12, 64, F32, "dense"),
         (8, 257, 16, 80, BF16, "none"), (64, 256, 12, 64, F32, "split-table"), (64, 197, 12, 64, F32, "split-none")]


def call_name(c):
    B, N, H, D, dt, bias = c
    return f"B{B}_N{N}_H{H}_D{D}_{'bf16' if dt == BF16 else 'fp32'}_{bias}"


def worker(lib_path):
    spec = importlib.util.spec_from_file_location("dm_lib", os.path.join(ROOT, "deepmerge_amd", "_lib.py"))      # (not the package: no torch)
    _lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(_lib)
    if lib_path:
        _lib.LIB_PATH = os.path.abspath(lib_path)
    lib = _lib.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes, hip.hipMemset.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_int, C.c_size_t]

    def zeros(nbytes):
        p = C.c_void_p()
        if hip.hipMalloc(C.byref(p), nbytes) != 0 or hip.hipMemset(p, 0, nbytes) != 0:
            sys.exit("attn_plan_routes worker: hipMalloc / hipMemset failed")
        return p

    MB = 1 << 20
    big = max(B * N * 3 * H * D * 4 for B, N, H, D, _, _ in CALLS)
    qkv, dqkv, hi, lo = zeros(big), zeros(big), zeros(big // 2), zeros(big // 2)
    out, dout, dhi, dlo = zeros(big // 3), zeros(big // 3), zeros(big // 6), zeros(big // 6)
    lse, delta, bias, bias_t, table, slab, mark = zeros(4 * MB), zeros(4 * MB), zeros(8 * MB), zeros(8 * MB), zeros(MB), zeros(64 * MB), zeros(4096)
    for c in CALLS:
        B, N, H, D, dt, kind = c
        scale, cube = D ** -0.5, (N // 64, 8, 8)
        want_slab = kind not in ("none", "split-none")
        chunks = lib.dm_attention_split_bwd_chunks(B, N, H) if kind.startswith("split") else lib.dm_attention_bwd_batch_chunks(B, N, H, dt)
        assert chunks * H * N * N * 4 <= 64 * MB and B * H * N * 4 <= 4 * MB and H * N * N * 4 <= 8 * MB, c
        for step in ("fwd", "bwd"):
            assert lib.dm_split_bf16(mark, 4, 1, 4, C.c_void_p(mark.value + 2048), 0, 0, None) == 0
            if kind.startswith("split"):
                tab = table if kind == "split-table" else None
                rc = (lib.dm_attention_split_fwd(qkv, hi, lo, tab, *cube, out, lse, B, N, H, D, scale, None) if step == "fwd" else
                      lib.dm_attention_split_bwd(hi, lo, tab, *cube, out, dout, dhi, dlo, lse, dqkv, delta, slab if tab else None, B, N, H, D, scale, None))
            elif step == "fwd":
                rc = (lib.dm_attention_fwd_relpos(qkv, table, *cube, out, lse, B, N, H, D, scale, dt, None) if kind == "table" else
                      lib.dm_attention_fwd(qkv, None if kind == "none" else bias, out, lse, B, N, H, D, scale, dt, None))
            else:
                b, bt = (bias, bias_t) if kind in ("dense", "both") else (None, None)
                sl = slab if want_slab else None
                rc = (lib.dm_attention_bwd_relpos(qkv, table, *cube, b, bt, out, dout, lse, dqkv, delta, sl, B, N, H, D, scale, dt, None)
                      if kind in ("table", "both") else
                      lib.dm_attention_bwd(qkv, b, bt, out, dout, lse, dqkv, delta, sl, B, N, H, D, scale, dt, None))
            if hip.hipDeviceSynchronize() != 0:
                sys.exit(f"attn_plan_routes worker: device error after {call_name(c)} {step}")
            print(f"STEP {call_name(c)} {step} rc={rc}", flush=True)


def run_env(env, lib_path):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DM_ATTN_")}
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--worker"] + (["--lib", lib_path] if lib_path else [])
        r = subprocess.run(cmd, env={**clean, **env}, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"environment {env_name(env)}: child ended with {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        steps = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("STEP ")]
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda x: int(x["Dispatch_Id"]))
    segs = []
    for x in rows:
        if "split_bf16" in x["Kernel_Name"]:
            segs.append([])
        elif segs:
            grid = "x".join(x[f"Grid_Size_{a}"] for a in "XYZ")
            block = "x".join(x[f"Workgroup_Size_{a}"] for a in "XYZ")
            segs[-1].append(f"{x['Kernel_Name']} grid {grid} block {block} lds {x.get('LDS_Block_Size', '?')}")
    if len(segs) != len(steps):
        sys.exit(f"environment {env_name(env)}: {len(segs)} marked trace segments for {len(steps)} calls")
    print(f"== {env_name(env)}")
    for (name, step, rc), ks in zip(steps, segs):
        print(f"{name} {step} {rc}: " + ("nothing launched" if not ks else ""))
        for k in ks:
            print(f"    {k}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another libdeepmerge_hip.so (default: this tree's)")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        worker(a.lib)
        return
    for env in ENVS:
        run_env(env, a.lib)


if __name__ == "__main__":
    main()
