"""GPU: the weight-gradient product of dm_gemm (DM_TN: dW = dy^T x, db = column sums of dy) on every kernel family at ragged, guarded edges,
bit for bit against the float64 spec of tests/gemm_ref.py (its weight-gradient section: WG_FAMILIES, the plan restatements, wg_data, wg_frames).

Every family (forced by the switches read_switches reads on every call, then verified from the `_t<code>` of the profiler row) runs the cases
of gemm_ref.wg_cases at the smallest shape with two tiles in M and in N, a partly filled wave block and one that starts past M, an N tail and
at least two K slices whose last is shorter and ends in a partial K step, where the family has them (the 4-wave kernel takes whole tiles and
K % 128 == 0 only: its edges are the strides, the rows behind K and the short last slice):

  split             the sliced contraction, C written (NaN before)            short_acc         one unsplit short contraction, accumulate on: straight to C
  split_acc_cs      ... accumulate on, column sums stored (NaN before)        short_acc_csadd   ... with column sums added to old db
  split_csadd       ... column sums added to old db                           fold_acc_cs       hi / lo plane pairs (t64, p256, w4): accumulate + column sums

and dm_gemm_grouped runs two products in one launch in its sliced and its one-slice form, plain and on plane pairs (gemm_ref.WG_GROUP).

The data makes every partial sum a float32 in any order and any slicing (tests/test_gemm_host.py), so dW and db are compared BIT FOR BIT.
Every tensor a call touches is a view 8 elements into a larger allocation (16-byte, not 256-byte aligned) whose rest is NaN: dy has
lda = M + 8, x has ldb = N + 16, and below row K lie at least one whole k_per_split of NaN rows, so a slice that reads past K poisons the
result and still stays inside the allocation; C has ldc = N + 8 and 256 rows below M; db is M floats in a NaN frame.  Plane pairs are dense
[2, K, M] blocks (ops.gemm: lda = M), framed as a whole.  After the call every byte outside the windows of C and db is the prefill, dy and
x are unchanged.  The workspace is filled with NaN before the call; afterwards exactly the planned number of M x N slab slices and of rows
[M] of the column-sum region are finite and every other float of the buffer still holds the prefill -- so the slice structure the host test
derives from the restated plans is the one the kernels used, and nothing was written past the byte count the call declared.

ops.gemm declares the whole buffer of its workspace slot (>= 1 MiB), which would put the column-sum region at the buffer's end; here the
DmGemmArgs come from ops._gemm_args and declare exactly dm_gemm_workspace_bytes (asserted equal to its restatement), so that there IS room
behind the declared size.  dm_gemm_grouped is called through ops.gemm_grouped, whose slots are sized for 16 slices; their sizes are read back.

DM_PROF_SHAPES is read once per process, so each family is one fresh child process; the child sets the family's switches before every call,
prints one JSON `CASE` line per product and the parent asserts on the lines: exactly the documented cases ran, each on its family (the
generic fp32 path leaves no row; a grouped call that fell back to separate launches leaves rows without `grouped`).  After a child that ended
at its timeout, on a signal or on a HIP error no further child is started and every later case fails at once.

Findings.  test_gemm_skinny_fp32_k_slices[TN-100-52-2050] (tests/test_gpu_kernels.py) never ran on the generic path: 100 and 52 are multiples
of 4 and gemm_prepare's "fewer than 16 tiles" rule excludes DM_TN, so it runs on 64 x 64 MFMA tiles (`probe` line of the generic child: code
64); its docstring says so now.  sgemm_small_kernel<DM_TN> with gridDim.z > 1 is reached by the `generic` family here (M = 102).  The 64 /
128 tiles bound their m-contiguous loads by a buffer descriptor that ends at row K, so dropping the `min(K, ...)` of gemm_kernel's slice end
changes nothing for DM_TN: that fault is tried on the kernels whose slice end IS the bound.

The net is tight (single-line faults, each on a scratch copy of the library and run against this module; none is committed):
  dm_gemm256.hip gemm256_kernel: `kend = kbeg + p.k_per_split`       caught by p256: split, split_acc_cs, split_csadd, short_acc, short_acc_csadd (dW and db not the spec's bits,
  (the `min(p.K, ...)` of the slice end dropped)                      a planned slab slice not finite: 56 of the NaN rows below K were read).  The other seven children pass.  Not run
                                                                      against the older tests: their dense operands end at row K, the read would leave the allocation.
  dm_gemm.hip splitk_reduce_kernel: `f32x4 v = {0, 0, 0, 0}`         caught by t64, t128, f32_t64, f32_t128, p256, w4: split_acc_cs (and fold_acc_cs where the family has it)
  (the slab reduction ignores `accumulate`)                           and by grouped: sliced_acc, fold_sliced -- dW not the spec's bits.  generic passes (its slices are summed
                                                                      by sgemm_small_reduce_kernel).  Also caught by 12 of the older weight-gradient tests.
  dm_gemm.hip gemm_kernel: `row = p.colsum_slab + (z + 1) * p.M`     caught by t64: split_acc_cs, split_csadd, short_acc_csadd, fold_acc_cs (db not the spec's bits; column-sum
  (the fused column-sum rows indexed by the slice, off by one)        row 0 not written and a row outside the planned ones written).  The other seven children pass.  Also
                                                                      caught by test_gemm_wgrad_with_fused_column_sums and two grouped tests of tests/test_gpu_kernels.py.
"""
import json
import os
import subprocess
import sys

import pytest

import gemm_ref as G
from test_gpu_gemm_epilogues import ONCE_PER_PROCESS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 60           # a few dozen sub-millisecond products; the process start dominates.  Not a measurement.
_DEAD = []             # a child ended at its timeout, on a signal or on a HIP error: nothing more is started on the GPU by this module
SKINNY_TN = (100, 52, 2050)      # the TN case of test_gemm_skinny_fp32_k_slices: which family runs it (the generic child probes it)

CHILD = r"""
import ctypes as C
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import torch
import gemm_ref as G
from deepmerge_amd import _lib, ops
from deepmerge_amd._lib import DM_TN, DM_EPI_NONE

family = sys.argv[2]
grouped = family == "grouped"
fam = G.WG_GROUP if grouped else G.WG_FAMILIES[family]
dev, lib = "cuda:0", _lib.lib()
ab = {G.F32: torch.float32, G.BF16: torch.bfloat16}[fam["ab"]]
OFF = G.VIEW_OFFSET
NAN = float("nan")
HIP_WORDS = ("hip", "illegal", "launch failed", "memory access", "out of memory")


def set_env(extra=None):                                 # read_switches reads the environment on every call
    for k, v in dict(fam["env"], **(extra or {})).items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(got, want64):
    return bool(torch.equal(bits(got), bits(torch.from_numpy(np.array(want64)).to(got.dtype))))


def outside_changed(before, after, idx):
    keep = torch.ones(before.numel(), dtype=torch.bool)
    if idx is not None:
        keep[torch.from_numpy(idx).reshape(-1)] = False
    return int((bits(before)[keep] != bits(after)[keep]).sum()) * before.element_size()


def product(M, N, K, fold, acc, cs, kps):
    # the framed operands of one product on the host and on the device
    d = G.wg_data(M, N, K, fold)
    fr = G.wg_frames(M, N, K, kps, fold)
    host = {}
    for nm in ("dy", "x"):
        flat = torch.full((fr[nm]["elems"],), NAN, dtype=ab)
        idx = torch.from_numpy(fr[nm]["idx"])
        if fold:
            flat[idx[0]] = torch.from_numpy(np.array(d[nm + "_hi"])).to(ab)
            flat[idx[1]] = torch.from_numpy(np.array(d[nm + "_lo"])).to(ab)
        else:
            flat[idx] = torch.from_numpy(np.array(d[nm])).to(ab)
        host[nm] = flat
    host["c"] = torch.full((fr["c"]["elems"],), NAN)
    if acc:
        host["c"][torch.from_numpy(fr["c"]["idx"])] = torch.from_numpy(np.array(d["old_c"])).float()
    host["db"] = torch.full((fr["db"]["elems"],), NAN)
    if cs == "add":
        host["db"][torch.from_numpy(fr["db"]["idx"])] = torch.from_numpy(np.array(d["old_db"])).float()
    on = {k: v.clone().to(dev) for k, v in host.items()}
    if fold:
        A = ops.Planes(on["dy"][OFF:OFF + 2 * K * M].view(2, K, M))
        B = ops.Planes(on["x"][OFF:OFF + 2 * K * N].view(2, K, N))
    else:
        A, B = on["dy"][OFF:], on["x"][OFF:]
    return dict(d=d, fr=fr, host=host, on=on, A=A, B=B, Cv=on["c"][OFF:], dbv=on["db"][OFF:OFF + M] if cs else None,
                ref=G.wg_ref(d, acc, cs, fold))


def fill_ws(nbytes, slot):
    ws = ops.workspace(nbytes, dev, slot)
    ws.view(torch.float32).fill_(NAN)
    return ws


def check_ws(ws, writes, M, N, cs_first):
    # the planned writes are finite, every other float of the buffer is the prefill; slab slices and column-sum rows counted from their starts
    fl = ws.view(torch.float32).cpu()
    mask = torch.zeros(fl.numel(), dtype=torch.bool)
    for first, count in writes:
        mask[first:first + count] = True
    fin = torch.isfinite(fl)
    slices = 0
    while (slices + 1) * M * N <= fl.numel() and slices < 40 and bool(fin[slices * M * N:(slices + 1) * M * N].all()):
        slices += 1
    rows = 0
    while cs_first is not None and cs_first + (rows + 1) * M <= fl.numel() and rows < 200 and bool(fin[cs_first + rows * M:cs_first + (rows + 1) * M].all()):
        rows += 1
    return dict(written_finite=bool(fin[mask].all()), outside_changed=int((~torch.isnan(fl[~mask])).sum()), slab_slices=slices, cs_rows=rows)


def check_product(pr, M, N, cs):
    after = {k: v.cpu() for k, v in pr["on"].items()}
    fr, host = pr["fr"], pr["host"]
    out = {"exact": {"c": same_bits(after["c"][torch.from_numpy(fr["c"]["idx"])], pr["ref"][0])},
           "sentinel": {"c": outside_changed(host["c"], after["c"], fr["c"]["idx"]), "db": outside_changed(host["db"], after["db"], fr["db"]["idx"] if cs else None),
                        "dy": outside_changed(host["dy"], after["dy"], None), "x": outside_changed(host["x"], after["x"], None)}}
    if cs:
        out["exact"]["db"] = same_bits(after["db"][torch.from_numpy(fr["db"]["idx"])], pr["ref"][1])
    return out


def collect():
    rows = (_lib.DmProfRow * 64)()
    n = lib.dm_prof_collect(rows, 64)
    return [rows[i].name.decode() for i in range(n) for _ in range(rows[i].launches)]      # one entry per launch


def refuse(line, e):
    # exit status 3 = the library refused the arguments before any launch; anything that names the runtime ends the child with another
    # status, after which the parent starts nothing more
    line["error"] = "%s: %s" % (type(e).__name__, e)
    print("CASE " + json.dumps(line), flush=True)
    sys.exit(4 if any(w in line["error"].lower() for w in HIP_WORDS) else 3)


if not grouped:
    for case in G.wg_cases(family):
        M, N, K, fold, acc, cs = (case[k] for k in ("M", "N", "K", "fold", "acc", "cs"))
        k_all = 3 * K if fold else K
        set_env()
        declared = int(lib.dm_gemm_workspace_bytes(DM_TN, M, N, k_all))
        plan = G.wg_plan(family, case)
        line = {"family": family, "case": case["name"], "ws_bytes": [declared, plan["ws_bytes"]], "split": plan["split"], "kps": plan["kps"], "cs": plan["cs"]}
        pr = product(M, N, K, fold, acc, cs, plan["kps"])
        ws = fill_ws(declared, "gemm")
        if fold:
            A, B, lda, ldb, foldarg = pr["A"].t, pr["B"].t, M, N, (K, pr["A"].t.stride(0), pr["B"].t.stride(0))
        else:
            A, B, lda, ldb, foldarg = pr["A"], pr["B"], pr["fr"]["dy"]["ld"], pr["fr"]["x"]["ld"], None
        a = ops._gemm_args(DM_TN, A, B, pr["Cv"], M, N, k_all, lda, ldb, pr["fr"]["c"]["ld"], None, None, None, DM_EPI_NONE, None, None, acc, 0, 0, 0,
                           pr["dbv"], cs == "add", "gemm", None, foldarg)
        assert a.workspace == ws.data_ptr() and a.workspace_bytes == ws.numel() >= declared
        a.workspace_bytes = declared                      # exactly what dm_gemm_workspace_bytes asks for: the rest of the buffer is the guard
        set_env()
        lib.dm_prof_enable(1)
        try:
            ops.check(lib.dm_gemm(C.byref(a), ops._stream()), "dm_gemm")
        except Exception as e:
            refuse(line, e)
        torch.cuda.synchronize()
        lib.dm_prof_enable(0)
        line["rows"] = collect()
        line.update(check_product(pr, M, N, cs))
        cs_first = G.cut_workspace(declared, M, True)[1] // 4 if cs else None
        line["ws"] = check_ws(ws, plan["writes"], M, N, cs_first)
        line["ws"]["planned"] = [plan["split"] if plan["split"] > 1 else 0, plan["cs_rows"]]
        print("CASE " + json.dumps(line), flush=True)
    if family == "generic":                               # which family runs the TN case of test_gemm_skinny_fp32_k_slices (dense operands, as there)
        M, N, K = json.loads(sys.argv[3])
        for k in fam["env"]:
            os.environ.pop(k, None)
        g = torch.Generator(device=dev); g.manual_seed(M * N + K)
        A = torch.randint(-2, 3, (K, M), device=dev, generator=g).float()
        B = torch.randint(-2, 3, (K, N), device=dev, generator=g).float()
        probe = []
        for kw in (dict(bias=torch.zeros(N, device=dev), residual=torch.zeros(M, N, device=dev)), dict(accumulate=True)):
            Cm = torch.zeros(M, N, device=dev)
            lib.dm_prof_enable(1)
            ops.gemm(DM_TN, A, B, Cm, M, N, K, **kw)
            torch.cuda.synchronize()
            lib.dm_prof_enable(0)
            probe.append({"rows": collect(), "exact": bool(torch.equal(Cm, A.t() @ B))})
        print("PROBE " + json.dumps(probe), flush=True)
else:
    for case in fam["cases"]:
        K, fold, acc, cs = case["K"], case["fold"], case["acc"], case["cs"]
        k_all = 3 * K if fold else K
        set_env({"DM_GEMM_GROUPED": str(case["mode"])})
        wss = [fill_ws(int(lib.dm_gemm_workspace_bytes(DM_TN, M, N, k_all)) + G.GROUP_MIN_SLABS * M * N * 4, "gemm.g%d" % i) for i, (M, N) in enumerate(fam["shapes"])]
        plan = G.wg_group_plan(case, [w.numel() for w in wss])
        line = {"family": family, "case": case["name"], "form": plan["form"], "split": plan["split"], "kps": plan["kps"]}
        prs, calls = [], []
        for M, N in fam["shapes"]:
            pr = product(M, N, K, fold, acc, cs, plan["kps"])
            prs.append(pr)
            calls.append(((DM_TN, pr["A"], pr["B"], pr["Cv"], M, N, K),
                          dict(lda=pr["fr"]["dy"]["ld"], ldb=pr["fr"]["x"]["ld"], ldc=pr["fr"]["c"]["ld"], accumulate=acc, colsum_out=pr["dbv"], colsum_accumulate=cs == "add")))
        set_env({"DM_GEMM_GROUPED": str(case["mode"])})
        lib.dm_prof_enable(1)
        try:
            ops.gemm_grouped(calls)
        except Exception as e:
            refuse(line, e)
        torch.cuda.synchronize()
        lib.dm_prof_enable(0)
        line["rows"] = collect()
        line["products"] = []
        for i, ((M, N), pr, pp) in enumerate(zip(fam["shapes"], prs, plan["products"])):
            one = check_product(pr, M, N, cs)
            one["ws"] = check_ws(wss[i], pp["writes"], M, N, G.cut_workspace(wss[i].numel(), M, True)[1] // 4)
            one["ws"]["planned"] = [plan["split"] if plan["form"] == "sliced" else 0, max([c // M for f, c in pp["writes"] if f > 0] + [0])]
            line["products"].append(one)
        print("CASE " + json.dumps(line), flush=True)
print("DONE", flush=True)
"""


def _codes(rows):
    return [int(r.rsplit("_t", 1)[1]) for r in rows if r.startswith("gemm_") and "_t" in r and "grouped" not in r]


def _bad_product(tag, l, cs):
    bad = []
    want = {"c"} | ({"db"} if cs else set())
    if set(l.get("exact", {})) != want:
        bad.append((tag, "checks missing", l.get("exact")))
    for op, ok in l.get("exact", {}).items():
        if not ok:
            bad.append((tag, f"{op}: not bit-identical to the spec"))
    if set(l.get("sentinel", {})) != {"c", "db", "dy", "x"}:
        bad.append((tag, "sentinel counts missing", l.get("sentinel")))
    for op, nbytes in l.get("sentinel", {}).items():
        if nbytes != 0:
            bad.append((tag, f"{op}: {nbytes} bytes outside the written window changed"))
    ws = l.get("ws", {})
    if not ws.get("written_finite"):
        bad.append((tag, "a planned slab slice or column-sum row was not written"))
    if ws.get("outside_changed") != 0:
        bad.append((tag, f"workspace: {ws.get('outside_changed')} floats outside the planned slab slices and column-sum rows changed"))
    if [ws.get("slab_slices"), ws.get("cs_rows")] != ws.get("planned"):
        bad.append((tag, "slab slices / column-sum rows written differ from the plan", ws))
    return bad


def _run(family, *extra):
    if _DEAD:
        pytest.fail(f"not started: an earlier child ended abnormally ({_DEAD[0]})")
    env = dict(os.environ, DM_PROF_SHAPES="1")
    for k in ONCE_PER_PROCESS:
        env.pop(k, None)
    try:
        run = subprocess.run([sys.executable, "-c", CHILD, ROOT, family, *extra], env=env, cwd=ROOT, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _DEAD.append(f"{family}: no end after {TIMEOUT} s")
        pytest.fail(f"{family}: the child did not end within {TIMEOUT} s\n{(e.stdout or b'')[-2000:]}\n{(e.stderr or b'')[-2000:]}")
    if run.returncode not in (0, 3):        # 3: the library refused a product before any launch (the child says so); anything else may be a fault
        _DEAD.append(f"{family}: exit status {run.returncode}")
    lines = [json.loads(l[len("CASE "):]) for l in run.stdout.splitlines() if l.startswith("CASE ")]
    for l in lines:
        print(f"  [gemm_wgrad] {json.dumps(l)}")
    assert run.returncode == 0 and run.stdout.rstrip().endswith("DONE"), (run.returncode, run.stdout[-1500:], run.stderr[-3000:])
    return lines, run.stdout


@pytest.mark.parametrize("family", list(G.WG_FAMILIES))
def test_gemm_wgrad_family(family):
    fam = G.WG_FAMILIES[family]
    lines, out = _run(family, json.dumps(SKINNY_TN))
    cases = G.wg_cases(family)
    assert [l["case"] for l in lines] == [c["name"] for c in cases]          # exactly the documented cases ran
    bad = []
    for l, case in zip(lines, cases):
        tag = l["case"]
        plan = G.wg_plan(family, case)
        if l["ws_bytes"][0] != l["ws_bytes"][1]:
            bad.append((tag, "dm_gemm_workspace_bytes differs from its restatement", l["ws_bytes"]))
        codes = _codes(l["rows"])
        if fam["codes"]:
            if len(codes) != 1 or codes[0] not in fam["codes"] or len(l["rows"]) != 1:
                bad.append((tag, "ran on another family", l["rows"]))
        elif l["rows"]:
            bad.append((tag, "left a profiler row: not the generic path", l["rows"]))
        if (l["split"], l["kps"], l["cs"]) != (plan["split"], plan["kps"], plan["cs"]):
            bad.append((tag, "the child planned something else", l))
        bad += _bad_product(tag, l, case["cs"])
    if family == "generic":
        # the finding recorded at the top and in test_gemm_skinny_fp32_k_slices' docstring: its TN case runs on 64 x 64 MFMA tiles
        probe = json.loads([l for l in out.splitlines() if l.startswith("PROBE ")][-1][len("PROBE "):])
        print(f"  [gemm_wgrad] probe TN {SKINNY_TN}: {probe}")
        assert [_codes(p["rows"]) for p in probe] == [[64], [64]] and all(p["exact"] for p in probe), probe
    assert not bad, bad


def test_gemm_wgrad_grouped():
    lines, _ = _run("grouped")
    cases = G.WG_GROUP["cases"]
    assert [l["case"] for l in lines] == [c["name"] for c in cases]
    bad = []
    for l, case in zip(lines, cases):
        tag = l["case"]
        want_form = "sliced" if case["mode"] == 4 else "one_slice"
        row_form = "sliced" if case["mode"] == 4 else "1slice"
        # launches counted as tests/test_gpu_gemm_route.py does: ONE profiler record, the grouped one, in the form asked for
        if l["form"] != want_form or len(l["rows"]) != 1 or "grouped2" not in l["rows"][0] or not l["rows"][0].endswith(row_form):
            bad.append((tag, "fell back to separate launches or took the other form", l["form"], l["rows"]))
        if len(l["products"]) != len(G.WG_GROUP["shapes"]):
            bad.append((tag, "products missing"))
        for i, p in enumerate(l["products"]):
            bad += _bad_product(f"{tag}[{i}]", p, case["cs"])
    assert not bad, bad
