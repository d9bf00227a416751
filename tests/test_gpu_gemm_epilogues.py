"""GPU: the fused epilogue of dm_gemm on every kernel family at ragged edges, against the float64 spec of tests/gemm_ref.py.

Every family (forced by the switches read_switches reads on every call) runs the 14 operand configurations of gemm_ref.CONFIGS, in NT and
NN where it has both (and none_f32 once more per layout with A and B as framed views too: gemm_ref.FRAMED_AB, lda = K + 8, NaN pads and pad rows), at the smallest shape whose last row of tiles holds a partially filled wave block and one that starts past M, with an
N tail inside a wave's columns.  C, aux and residual are views 8 elements into larger allocations with leading dimensions N + 8 / N + 16 /
N + 24 and 256 rows below M; everything outside the M x N windows is NaN (also in the operands that are only read, so that a read outside
the window poisons the result), and after the call every byte outside the written windows must still be the prefill.

DM_PROF_SHAPES is read once per process and is the only way to learn which family ran a product, so each family is one fresh child
process (as in tests/test_gpu_gemm_route.py).  The child sets the family's switches before every call, reads the `_t<code>` of the one
profiler row the call leaves (the generic fp32 path leaves none), compares in-process and prints one JSON line per (layout, configuration);
the parent asserts on those lines.  A product that ran on another family is a failure.  After a child that ended at its timeout or with any status other than 0 or a
plain refusal of dm_gemm (a signal, a HIP error) no further child is started: every later case fails at once.

EXACT results (none / bias / residual / accumulate in any combination, MUL, the saved pre-activation of GELU, in fp32 and bf16) are compared
bit for bit (the sign of a zero set aside only for gemm_ref.STRIP_ZERO_SIGN, a recorded finding).  BOUNDED results against the bounds of gemm_ref.bounds, with D = E_AS / 2 + U for the fast GELU parts (E_AS = 1.5e-7, the
Abramowitz-Stegun error; U = 2^-24) and D = U for erff / expf (fp32 operands); each constant is the smallest integer for which the float32
restatement of the kernel's arithmetic stays at or below half the bound on exactly these inputs (tests/test_gemm_host.py):

  constant          bound                                                       worst err/tol   CPU restatement   GPU (MI355X), worst over the families
  C_G  fast 3       C_G D |x|                         gelu(x) -> fp32                            0.432             0.432
       erff 3                                                                                    0.487             0.487
                    ... + C_BF16 2^-8 (|y| + tol)     gelu(x) -> bf16 (C_BF16 = 2, rows_ref)     0.498 / 0.494     0.498 (w4; 0.494 elsewhere) / 0.494
                    ... + 2^-16 |y|                   gelu(x) -> hi + lo of a plane pair         0.462             0.462
  C_D  fast 1       C_D D + C_BF16 2^-8 (|g| + tol)   saved gelu'(x) -> bf16                     0.491             0.491
       erff 1                                                                                    0.491             0.491
  C_DG fast 4       C_DG (D |acc| + U |result|)       acc gelu'(aux) + residual -> fp32          0.399             0.399 (w4; 0.366 .. 0.383 elsewhere)
       erff 5                                                                                    0.479             0.441 (f32_t128; 0.431 f32_t64, generic)
  (the hardware's v_exp_f32 / v_rcp_f32 and the library's erff / expf used none of the spare factor 2: no extra term was needed)

The net is tight (three single-line changes on a scratch copy of the library, each run against these tests and against test_gemm_epilogues):
  dm_gemm_emit8 reads the residual at rb.c       caught by w4 and kslices: bias_res_f32, bias_res_acc_f32 (bits), dgelu_f32_res (inf of the bound);
                                                 test_gemm_epilogues and its ring / w4 forms pass.  (Not by grouped41: its shared ld makes rb.c == rb.r.)
  dm_gemm_strip_store adds pre.res before the    caught by t64 and f32_t64: dgelu_f32_res (> 10^6 of the bound); test_gemm_epilogues passes
  multiply
  dm_gelu_parts_fast drops the copysignf         caught by every bf16-operand family (8 of 11) in every GELU-type configuration (> 10^6 of the bound);
                                                 here test_gemm_epilogues[bf16] and its ring / w4 forms fail too: 1.6e-2 does catch a lost sign

Skipped configurations, each with the line of the plan that refuses it: gemm_ref.FAMILIES[family]["skips"] (q4: everything without a
straight-line epilogue instance; t96: everything with an epilogue or accumulate, or whose lean key is not 0, 1 << 3 or 1 | 1 << 3 -- none_f32,
none_bf16 and bias_res_f32 remain; fp32 operands: the plane pair; the generic path: everything that is not fp32 throughout, and grouped rows).
The t96 family (dm_gemm_t96.hip, code 12896; 128 x 96 tiles, a wave owns 64 x 48) joined after the table and the mutation record above were
made: it runs at 320 x 200 x 192 (M % 64 == 0 as its plan demands, three column tiles, the 8-column tail inside a wave's 48 columns).
The K loops of all these families are pinned by tests/test_gpu_gemm_mainloop.py.
The parent asserts that exactly the remaining cases ran.  Run with -s for one line per product with its family code.
"""
import json
import os
import subprocess
import sys

import pytest

import gemm_ref as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 60           # a few hundred sub-millisecond products; the process start dominates.  Not a measurement.
# switches the library reads once per process (or that this module does not set per call): an inherited value would silently change which
# kernel or epilogue form runs.  tests/test_gemm_host.py holds this list against the library's getenv calls.
ONCE_PER_PROCESS = ("DM_GEMM_ROUTE", "DM_GEMM_W4_TN", "DM_GEMM_EPI_LEAN", "DM_GEMM_T128_ROWS", "DM_GEMM_T128_TOUCH", "DM_GEMM_FWD_SPLIT",
                    "DM_GEMM_GROUP_M", "DM_GEMM_256_GROUP_M", "DM_GEMM_SKINNY", "DM_GEMM_FOLD_ROUTES",
                    "DM_GEMM_CUS_RESERVED", "DM_GEMM_256_NT_LONGK", "DM_GEMM_256_TN_MINK", "DM_GEMM_GROUPED")
_DEAD = []             # a child ended at its timeout, on a signal or on a HIP error: nothing more is started on the GPU by this module

CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import torch
import gemm_ref as G
from deepmerge_amd import _lib, ops
from deepmerge_amd._lib import DM_NN, DM_NT, DM_EPI_NONE, DM_EPI_GELU, DM_EPI_GELU_GRAD, DM_EPI_DGELU, DM_EPI_MUL

family = sys.argv[2]
fam = G.FAMILIES[family]
M, N, K = fam["shape"]
d = G.operands(M, N, K)
dev, lib = "cuda:0", _lib.lib()
TD = {G.F32: torch.float32, G.BF16: torch.bfloat16}
EPI = {"none": DM_EPI_NONE, "gelu": DM_EPI_GELU, "gelu_grad": DM_EPI_GELU_GRAD, "dgelu": DM_EPI_DGELU, "mul": DM_EPI_MUL}
ab = TD[fam["ab"]]
A = torch.from_numpy(d["a"]).to(ab).to(dev)
B = {"NT": torch.from_numpy(d["b"]).to(ab).to(dev), "NN": torch.from_numpy(np.ascontiguousarray(d["b"].T)).to(ab).to(dev)}
bias = torch.from_numpy(d["bias"]).float().to(dev)


def alloc(o, window):
    flat = torch.full((o["elems"],), float("nan"), dtype=TD[o["dtype"]])
    if window is not None:
        flat[torch.from_numpy(o["idx"])] = torch.from_numpy(np.array(window)).to(flat.dtype)
    return flat


def changed_bytes(before, after, o, written):
    size = before.element_size()
    diff = before.view(torch.uint8).reshape(-1, size) != after.view(torch.uint8).reshape(-1, size)
    keep = torch.ones(before.numel(), dtype=torch.bool)
    if written:
        keep[torch.from_numpy(o["idx"]).reshape(-1)] = False
        if "plane" in o:
            keep[torch.from_numpy(o["idx"] + o["plane"]).reshape(-1)] = False
    return int(diff[keep].sum())


def same_bits(got, want64, dtype, zero_sign_apart):
    # bit for bit; the sign of a zero is set aside only for the recorded pairs of gemm_ref.STRIP_ZERO_SIGN
    want = torch.from_numpy(np.array(want64)).to(dtype)
    it = torch.int32 if dtype == torch.float32 else torch.int16
    if zero_sign_apart:
        got, want = torch.where(got == 0, torch.zeros_like(got), got), torch.where(want == 0, torch.zeros_like(want), want)
    return bool(torch.equal(got.contiguous().view(it), want.contiguous().view(it)))


HIP_WORDS = ("hip", "illegal", "launch failed", "memory access", "out of memory")

def framed(values, rows, cols):
    # a read-only operand as a view VIEW_OFFSET elements into a NaN allocation with a padded leading dimension (gemm_ref.framed_operand)
    elems, ld, idx = G.framed_operand(rows, cols)
    flat = torch.full((elems,), float("nan"), dtype=ab)
    flat[torch.from_numpy(idx)] = values.cpu()
    return flat, ld


for layout, name in G.family_cases(family) + G.family_framed_cases(family):
    cfg = G.CONFIG["none_f32" if name == G.FRAMED_AB else name]
    c = G.case(cfg, M, N, K)
    ref = G.epilogue_ref(d["acc"], c)
    b = G.buffers(cfg, M, N)
    host = {"c": alloc(b["c"], c["old_c"])}
    if "aux" in b:
        host["aux"] = alloc(b["aux"], c["aux_v"])
    if "res" in b:
        host["res"] = alloc(b["res"], c["res_v"])
    on = {k: v.clone().to(dev) for k, v in host.items()}
    off = G.VIEW_OFFSET
    if cfg["c"] == G.PAIR:
        c_arg, ldc = ops.Planes(on["c"][off:off + 2 * M * N].view(2, M, N)), None
    else:
        c_arg, ldc = on["c"][off:], b["c"]["ld"]
    a_arg, b_arg, lda, ldb = A, B[layout], K, K if layout == "NT" else N
    if name == G.FRAMED_AB:
        host["a"], lda = framed(A, M, K)
        host["b"], ldb = framed(B[layout], *((N, K) if layout == "NT" else (K, N)))
        on["a"], on["b"] = host["a"].clone().to(dev), host["b"].clone().to(dev)
        a_arg, b_arg = on["a"][off:], on["b"][off:]
    kw = dict(lda=lda, ldb=ldb, ldc=ldc, bias=bias if cfg["bias"] else None, epilogue=EPI[cfg["epi"]],
              accumulate=cfg["acc"], rows_per_group=b["rows_per_group"], group_stride=b["group_stride"])
    if "aux" in b:
        kw.update(aux=on["aux"][off:], ldaux=b["aux"]["ld"])
    if "res" in b:
        kw.update(residual=on["res"][off:], ldr=b["res"]["ld"])
    for k, v in fam["env"].items():                      # read_switches reads the environment on every call
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    line = {"family": family, "layout": layout, "config": name}
    slab = None
    if family == "kslices":                               # the call's split-K slab (ops.gemm takes it from workspace slot "gemm"): NaN before
        slab = ops.workspace(lib.dm_gemm_workspace_bytes(DM_NT if layout == "NT" else DM_NN, M, N, K), dev, "gemm")
        slab.view(torch.float32).fill_(float("nan"))
    lib.dm_prof_enable(1)
    try:
        ops.gemm(DM_NT if layout == "NT" else DM_NN, a_arg, b_arg, c_arg, M, N, K, **kw)
    except Exception as e:
        # exit status 3 = dm_gemm refused the arguments before any launch; anything that names the runtime, and anything raised later
        # (the synchronize below is outside this block), ends the child with another status, after which the parent starts nothing more
        line["error"] = "%s: %s" % (type(e).__name__, e)
        print("CASE " + json.dumps(line), flush=True)
        sys.exit(4 if any(w in line["error"].lower() for w in HIP_WORDS) else 3)
    torch.cuda.synchronize()
    if slab is not None:                                  # two slices of M x N partial sums were written, the rest of the slab was not
        fl = slab.view(torch.float32)
        line["slab"] = [bool(torch.isfinite(fl[:2 * M * N]).all()), bool(torch.isnan(fl[2 * M * N:4 * M * N]).all())]
    lib.dm_prof_enable(0)
    rows = (_lib.DmProfRow * 64)()
    n = lib.dm_prof_collect(rows, 64)
    line["rows"] = [rows[i].name.decode() for i in range(n)]
    after = {k: v.cpu() for k, v in on.items()}
    line["sentinel"] = {k: changed_bytes(host[k], after[k], b[k], b[k]["written"]) for k in ("c", "aux", "res") if k in b}
    line["sentinel"].update({k: changed_bytes(host[k], after[k], None, False) for k in ("a", "b") if k in host})

    c_exact, aux_exact = G.is_exact(cfg)
    apart = (family, name) in G.STRIP_ZERO_SIGN
    tol = G.bounds(cfg, ref, d["acc"], fam["fast"])
    idx = torch.from_numpy(b["c"]["idx"])
    got = after["c"][idx]
    line["exact"], line["ratio"] = {}, {}
    if c_exact:
        line["exact"]["c"] = same_bits(got, ref["c"], got.dtype, apart)
    elif cfg["c"] == G.PAIR:
        s = got.double() + after["c"][idx + b["c"]["plane"]].double()
        line["ratio"]["c"] = G.worst((s - torch.from_numpy(ref["v"])).abs(), tol["c"])
    else:
        line["ratio"]["c"] = G.worst((got.double() - torch.from_numpy(ref["v"])).abs(), tol["c"])
    if "aux" in b and b["aux"]["written"]:
        gx = after["aux"][torch.from_numpy(b["aux"]["idx"])]
        if aux_exact:
            line["exact"]["aux"] = same_bits(gx, ref["aux"], gx.dtype, False)
        else:
            line["ratio"]["aux"] = G.worst((gx.double() - torch.from_numpy(ref["aux_v"])).abs(), tol["aux"])
    print("CASE " + json.dumps(line), flush=True)
print("DONE", flush=True)
"""


def _code(rows):
    assert len(rows) == 1, rows
    return int(rows[0].rsplit("_t", 1)[1])


def _kind(cfg, op, fast):
    """The row of the table at the top a bounded result belongs to."""
    who = "fast" if fast else "erff"
    if op == "aux":
        return f"{who} gelu' -> bf16"
    if cfg["epi"] == "dgelu":
        return f"{who} acc gelu' + res -> f32"
    return f"{who} gelu -> {cfg['c']}"


@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_gemm_epilogue_family(family):
    if _DEAD:
        pytest.fail(f"not started: an earlier child ended abnormally ({_DEAD[0]})")
    fam = G.FAMILIES[family]
    env = dict(os.environ, DM_PROF_SHAPES="1")
    for k in ONCE_PER_PROCESS:
        env.pop(k, None)
    try:
        run = subprocess.run([sys.executable, "-c", CHILD, ROOT, family], env=env, cwd=ROOT, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _DEAD.append(f"{family}: no end after {TIMEOUT} s")
        pytest.fail(f"{family}: the child did not end within {TIMEOUT} s\n{(e.stdout or b'')[-2000:]}\n{(e.stderr or b'')[-2000:]}")
    lines = [json.loads(l[len("CASE "):]) for l in run.stdout.splitlines() if l.startswith("CASE ")]
    if run.returncode not in (0, 3):        # 3: dm_gemm refused a product before any launch (the child says so); anything else may be a fault
        _DEAD.append(f"{family}: exit status {run.returncode}")
    worst = {}
    for l in lines:
        print(f"  [gemm_epi] {family:<8s} {l['layout']} {l['config']:<20s} rows={l.get('rows')} exact={l.get('exact')} "
              f"ratio={ {k: round(v, 3) for k, v in l.get('ratio', {}).items()} } sentinel={l.get('sentinel')} {l.get('error', '')}")
    assert run.returncode == 0 and run.stdout.rstrip().endswith("DONE"), (run.returncode, run.stdout[-1500:], run.stderr[-3000:])

    # exactly the documented cases ran
    assert [(l["layout"], l["config"]) for l in lines] == G.family_cases(family) + G.family_framed_cases(family)
    bad = []
    for l in lines:
        cfg = G.CONFIG["none_f32" if l["config"] == G.FRAMED_AB else l["config"]]
        tag = (l["layout"], l["config"])
        # the family: the code of the one profiler row; the generic path leaves none
        if fam["codes"]:
            if len(l["rows"]) != 1 or _code(l["rows"]) not in fam["codes"]:
                bad.append((tag, "ran on another family", l["rows"]))
        elif l["rows"]:
            bad.append((tag, "left a profiler row: not the generic path", l["rows"]))
        if family == "kslices" and l.get("slab") != [True, True]:
            bad.append((tag, "the split-K slab was not written by exactly two slices: not the K-slice path", l.get("slab")))
        c_exact, aux_exact = G.is_exact(cfg)
        saves = isinstance(cfg["aux"], tuple) and cfg["aux"][1] == "save"
        want_exact = {"c"} if c_exact else set()
        want_ratio = set() if c_exact else {"c"}
        if saves:
            (want_exact if aux_exact else want_ratio).add("aux")
        if set(l["exact"]) != want_exact or set(l["ratio"]) != want_ratio:
            bad.append((tag, "checks missing", l["exact"], l["ratio"]))
        for op, ok in l["exact"].items():
            if not ok:
                bad.append((tag, f"{op}: not bit-identical to the spec"))
        for op, r in l["ratio"].items():
            k = _kind(cfg, op, fam["fast"])
            worst[k] = max(worst.get(k, 0.0), r)
            if not r <= 1.0:
                bad.append((tag, f"{op}: {r:.3f} of the bound"))
        want_ops = {"c"} | ({"aux"} if isinstance(cfg["aux"], tuple) else set()) | ({"res"} if cfg["res"] else set())
        if l["config"] == G.FRAMED_AB:
            want_ops |= {"a", "b"}
        if set(l["sentinel"]) != want_ops:
            bad.append((tag, "sentinel counts missing", l["sentinel"]))
        for op, nbytes in l["sentinel"].items():
            if nbytes != 0:
                bad.append((tag, f"{op}: {nbytes} bytes outside the written window changed"))
    for k, r in sorted(worst.items()):
        print(f"  [gemm_epi] {family:<8s} worst err/tol  {k:<28s} {r:.3f}")
    assert not bad, bad
