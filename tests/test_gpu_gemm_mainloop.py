"""GPU: the K loop of dm_gemm's forward / dgrad products (NT, NN) on every kernel family, bit for bit against the float64 spec of
tests/gemm_ref.py: every K-step count from one to the pipeline's depth + 2, K tails, hi / lo plane pairs with one, two and three K tiles
per segment in two placements, and the tile walk.

Structure as in tests/test_gpu_gemm_epilogues.py: one fresh child process per family (DM_PROF_SHAPES is read once per process and the
`_t<code>` of the profiler row is the only way to learn which family ran), the epilogue module's ONCE_PER_PROCESS switches removed from its environment,
the family's switches set before every call, one JSON line per product, all assertions in the parent, which also requires that exactly the
documented products ran.  After a child that ended at its timeout or with a status other than 0 or 3 no further child is started.

Every product checks
  family     one profiler row whose code is the family's (generic: none); kslices: the NaN-prefilled slab holds exactly the planned slices;
  result     C (both planes of pair_none) bit-identical to gemm_ref.epilogue_ref; gemm_ref.STRIP_ZERO_SIGN names no pair of these tests;
  sentinels  C in its NaN frame (ldc = N + 8, 256 rows below M), A and B in NaN frames (plain: gemm_ref.framed_operand, lda = K + 8; pairs:
             gemm_ref.pair_frame), the residual in its own; no byte outside C's window changes and the operands are unchanged;
  placement  plane pairs run "dense" (planes rows * cols apart) and "far" (rows * cols + 8 * 37, NaN between: a weight's mirror pair; ops.gemm
             takes the stride from Planes.t.stride(0) and accepts the strided view as it is); the two C are bit-identical.

Case table (gemm_ref.ML_K, ML_FOLD, ML_WALK; M, N of gemm_ref.FAMILIES; NT and NN where the family has both; plain: none_f32, none_bf16,
bias_res_f32; pairs: those and pair_none):
  family      code    K (plain)                          k_fold (pairs)   walk M x N x K
  t64         64      8 64 72 128 136 192 256 320        64 128 192       648 x 136 x 64
  t128        128     8 64 72 128 136 192 256 320        64 128 192       1352 x 264 x 64
  f32_t64     64      4 32 36 64 96 128 160              refused          648 x 264 x 32   (N: 16 tiles of 128 x 128 keep it off the generic path)
  f32_t128    128     4 32 36 64 96 128 160              refused          1352 x 264 x 32
  ring8       2568    64 128 192 256 320                 64 128 192       2760 x 264 x 64
  ring4       1288    64 128 192 256 320                 64 128 192       1352 x 264 x 64
  q4          1284    64 128 192 256 320                 declined         1344 x 264 x 64
  t96         12896   64 128 192 256 320 384             declined         1344 x 200 x 64
  w4          1924    128 256 384 512                    64 128 192       (256 (cus + cus / 2 + 1) - 56) x 192 x {128, 256}: its own test
  p256        256     64 128 192 256 320                 64 128 192       2760 x 520 x 64
  kslices     64      1536 1600 2048 (2, 2, 4 slices)    512 576          648 x 136 x 1536 (a one-step product has no slices)
  generic     -       1 19 33 (no none_bf16: fp32 only)  refused          171 x 40 x 19    (2-D grid: no remap, no bands)

Skips and refusals, each with its line of the plan in gemm_ref: no listed K is refused by any plan (ML_K_SKIPS is empty;
tests/test_gemm_host.py restates the K rules).  Plane pairs (ML_FOLD_REFUSED): fp32 operands and the generic path are refused by dm_gemm
itself (k_fold_fault, "k_fold needs bf16 operands"): the child ends with status 3.  q4 and t96 differ from what the issue expected: their
plans return false for k_fold > 0 and gemm_plan goes on to the register-staged tiles, so dm_gemm does NOT refuse -- the product runs under
code 64.  The child requires exactly that (one row, not the family's code) and then ends with status 3 as for a refusal; a q4 / t96 row for
a folded product would be a failure.

The net is tight (three single-line changes on a scratch copy of the library, one at a time, each run once on an MI355X against this
module and against tests/test_gpu_kernels.py::test_folded_split_product_equals_the_image_product; each only changes which in-bounds data
is read or how many steps run):
  gemm_ring_kernel's k_off picks b_fold by the   caught by ring8 and ring4: all 24 plane-pair products each (k_fold 64, 128, 192; four configurations;
  A pattern (B read as hi, hi, lo)               dense and far), bits of C and of both planes; every plain product, the walks and the eleven other
                                                 tests pass.  The older test fails too: its three lds-NT cases, at `torch.equal(outs[0], outs[1])`
  gemm_kernel runs nk - 1 steps when nk > 4      caught by t64 and t128: K = 320 (six products each) and k_fold = 128, 192 (6 and 9 steps; 32 products each;
                                                 k_fold = 64 and every K <= 256 pass: nk <= 4); f32_t64 and f32_t128: K = 160; kslices: all 50 products
                                                 and both walks.  The older test fails too: all nine tiles cases and two w4 cases, which therefore ran on gemm_kernel
  dm_gemm256.hip takes segment 2's A offset      caught by p256: all 48 plane-pair products; everything else passes.  The older test fails too: its
  from a_fold[1]                                 nine lds cases (the NT ones through the weight gradient it runs behind the product)
  So these three are gross enough for the older test as well: a change confined to the FOLD instances breaks its bit comparison of the plane
  pairs with the three-piece images on the same kernel, and a lost K tile is far outside 3e-5.  What it cannot see, and tests/test_gemm_host.py
  shows this module does (test_mainloop_net_is_tight: every restated fault differs from the spec in every 16 x 16 block): a fault both of its
  runs share inside 3e-5 of the result's scale, which family ran (DM_GEMM_RING and DM_GEMM_256 are both set for "lds"), a seam at one, two or
  three K tiles, a ragged M or N tail, planes that are not rows * cols apart, and anything outside the written window.

Findings: none.  Every family matched the spec bit for bit at every listed K, k_fold, placement and walk on the first run.

Run with -s for one line per product: family, layout, K or k_fold, placement, code, verdict.
"""
import json
import os
import subprocess
import sys

import pytest

import gemm_ref as G
from test_gpu_gemm_epilogues import ONCE_PER_PROCESS, TIMEOUT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DEAD = []             # a child ended at its timeout, on a signal or on a HIP error: nothing more is started on the GPU by this module

CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import torch
import gemm_ref as G
from deepmerge_amd import _lib, ops
from deepmerge_amd._lib import DM_NN, DM_NT

family, part = sys.argv[2], sys.argv[3]
fam = G.FAMILIES[family]
dev, lib = "cuda:0", _lib.lib()
TD = {G.F32: torch.float32, G.BF16: torch.bfloat16}
ab = TD[fam["ab"]]
off = G.VIEW_OFFSET
HIP_WORDS = ("hip", "illegal", "launch failed", "memory access", "out of memory")
NAN = float("nan")


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
    # bit for bit; the sign of a zero is set aside only for the recorded pairs of gemm_ref.STRIP_ZERO_SIGN (none of them is run here)
    want = torch.from_numpy(np.array(want64)).to(dtype)
    it = torch.int32 if dtype == torch.float32 else torch.int16
    if zero_sign_apart:
        got, want = torch.where(got == 0, torch.zeros_like(got), got), torch.where(want == 0, torch.zeros_like(want), want)
    return bool(torch.equal(got.contiguous().view(it), want.contiguous().view(it)))


def framed(values, dtype):
    # a plain operand as a view VIEW_OFFSET elements into a NaN allocation with a padded leading dimension (gemm_ref.framed_operand)
    rows, cols = values.shape
    elems, ld, idx = G.framed_operand(rows, cols)
    flat = torch.full((elems,), NAN, dtype=dtype)
    flat[torch.from_numpy(idx)] = torch.from_numpy(np.ascontiguousarray(values)).to(dtype)
    return flat, ld


def pair(hi, lo, placement, dtype=torch.bfloat16):
    # a plane pair inside one flat NaN allocation (gemm_ref.pair_frame); the Planes view is built on the device copy
    rows, cols = hi.shape
    fr = G.pair_frame(rows, cols, placement)
    flat = torch.full((fr["elems"],), NAN, dtype=dtype)
    flat[torch.from_numpy(fr["idx"])] = torch.from_numpy(np.stack([hi, lo])).to(dtype)
    return flat, fr


def planes(flat_dev, fr, rows, cols):
    return ops.Planes(torch.as_strided(flat_dev, (2, rows, cols), (fr["plane"], cols, 1), off))


def set_switches():
    for k, v in fam["env"].items():                      # read_switches reads the environment on every call
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


_OPS = {}

def operands_on_device(kind, layout, M, N, K, placement, d):
    # (host copies, device copies, A argument, B argument, lda, ldb), built once per (kind, layout, K, placement)
    key = (kind, layout, M, N, K, placement)
    if key in _OPS:
        return _OPS[key]
    _OPS.clear()
    host = {}
    if kind == "fold":
        host["a"], fa = pair(d["a_hi"], d["a_lo"], placement)
        bh, bl = (d["b_hi"], d["b_lo"]) if layout == "NT" else (d["b_hi"].T, d["b_lo"].T)
        host["b"], fb = pair(bh, bl, placement)
        on = {k: v.clone().to(dev) for k, v in host.items()}
        out = (host, on, planes(on["a"], fa, M, K), planes(on["b"], fb, *bh.shape), None, None)
    else:
        host["a"], lda = framed(d["a"], ab)
        host["b"], ldb = framed(d["b"] if layout == "NT" else d["b"].T, ab)
        on = {k: v.clone().to(dev) for k, v in host.items()}
        out = (host, on, on["a"][off:], on["b"][off:], lda, ldb)
    _OPS[key] = out
    return out


_DENSE_C = {}

def run(kind, layout, M, N, K, placement, name, d, line):
    cfg = G.ML_CONFIG[name]
    fold = kind == "fold"
    ref = G.epilogue_ref(d["acc"], G.ml_case(cfg, d)) if "bias" in d else G.epilogue_ref(d["acc"], dict(cfg, bias_v=None, res_v=None, old_c=None, aux_v=None))
    b = G.buffers(cfg, M, N)
    host, on, a_arg, b_arg, lda, ldb = operands_on_device(kind, layout, M, N, K, placement, d)
    host, on = dict(host), dict(on)
    host["c"] = torch.full((b["c"]["elems"],), NAN, dtype=TD[b["c"]["dtype"]])
    if "res" in b:
        host["res"] = torch.full((b["res"]["elems"],), NAN, dtype=torch.float32)
        host["res"][torch.from_numpy(b["res"]["idx"])] = torch.from_numpy(np.array(d["res"])).float()
    for k in ("c", "res"):
        if k in host:
            on[k] = host[k].clone().to(dev)
    if cfg["c"] == G.PAIR:
        c_arg, ldc = ops.Planes(on["c"][off:off + 2 * M * N].view(2, M, N)), None
    else:
        c_arg, ldc = on["c"][off:], b["c"]["ld"]
    kw = dict(lda=lda, ldb=ldb, ldc=ldc, bias=torch.from_numpy(np.array(d["bias"])).float().to(dev) if cfg["bias"] else None)
    if "res" in b:
        kw.update(residual=on["res"][off:], ldr=b["res"]["ld"])
    set_switches()
    lay = DM_NT if layout == "NT" else DM_NN
    slab = None
    k_all = 3 * K if fold else K
    if family == "kslices":                               # the call's split-K slab (ops.gemm takes it from workspace slot "gemm"): NaN before
        slab = ops.workspace(lib.dm_gemm_workspace_bytes(lay, M, N, k_all), dev, "gemm")
        slab.view(torch.float32).fill_(NAN)
    lib.dm_prof_enable(1)
    try:
        ops.gemm(lay, a_arg, b_arg, c_arg, M, N, K, **kw)
    except Exception as e:
        # exit status 3 = dm_gemm refused the arguments before any launch; anything that names the runtime, and anything raised later
        # (the synchronize below is outside this block), ends the child with another status, after which the parent starts nothing more
        line["error"] = "%s: %s" % (type(e).__name__, e)
        print("CASE " + json.dumps(line), flush=True)
        sys.exit(4 if any(w in line["error"].lower() for w in HIP_WORDS) else 3)
    torch.cuda.synchronize()
    if slab is not None:                                  # how many whole M x N slices of partial sums were written, and nothing behind them
        fl = slab.view(torch.float32)[:4 * M * N].view(4, M * N)
        fin, nan = torch.isfinite(fl).all(1).tolist(), torch.isnan(fl).all(1).tolist()
        n = sum(fin)
        line["slab"] = n if (fin[:n] == [True] * n and nan[n:] == [True] * (4 - n)) else -1
    lib.dm_prof_enable(0)
    rows = (_lib.DmProfRow * 64)()
    n = lib.dm_prof_collect(rows, 64)
    line["rows"] = [rows[i].name.decode() for i in range(n)]
    after = {k: v.cpu() for k, v in on.items()}
    line["sentinel"] = {k: changed_bytes(host[k], after[k], b[k], b[k]["written"]) for k in ("c", "res") if k in b}
    line["sentinel"].update({k: changed_bytes(host[k], after[k], None, False) for k in ("a", "b")})
    apart = (family, name) in G.STRIP_ZERO_SIGN
    idx = torch.from_numpy(b["c"]["idx"])
    got = after["c"][idx]
    line["exact"] = {"c": same_bits(got, ref["c"], got.dtype, apart)}
    if cfg["c"] == G.PAIR:
        got_lo = after["c"][idx + b["c"]["plane"]]
        line["exact"]["c_lo"] = same_bits(got_lo, ref["c_lo"], got_lo.dtype, False)
        got = torch.stack([got, got_lo])
    if not line["exact"]["c"]:
        bad = (got if cfg["c"] != G.PAIR else got[0]).double() != torch.from_numpy(np.array(ref["c"]))
        line["wrong"] = int(bad.sum())
    if fold:                                              # the two placements give the same bits
        key = (layout, K, name)
        if placement == "dense":
            _DENSE_C.clear()
            _DENSE_C[key] = got.clone()
        else:
            it = torch.int32 if got.dtype == torch.float32 else torch.int16
            line["same_as_dense"] = key in _DENSE_C and bool(torch.equal(_DENSE_C[key].contiguous().view(it), got.contiguous().view(it)))
    print("CASE " + json.dumps(line), flush=True)


if part == "walk_w4":
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, N = G.ml_walk_w4(cus)
    for K in G.ML_WALK_W4_K:
        for layout in fam["layouts"]:
            run("plain", layout, M, N, K, None, "none_f32", G.ml_walk_data(M, N, K), {"family": family, "kind": "walk", "layout": layout, "K": K, "M": M, "N": N, "cus": cus})
    print("DONE", flush=True)
    sys.exit(0)

M, N, _ = fam["shape"]
for c in G.ml_cases(family):
    fold = c["kind"] == "fold"
    run(c["kind"], c["layout"], M, N, c["K"], c["placement"], c["config"], G.ml_data(M, N, c["K"], fold), {"family": family, **c})
if family in G.ML_WALK:
    WM, WN, WK = G.ML_WALK[family]
    for layout in fam["layouts"]:
        run("plain", layout, WM, WN, WK, None, "none_f32", G.ml_walk_data(WM, WN, WK), {"family": family, "kind": "walk", "layout": layout, "K": WK, "M": WM, "N": WN})
print("DONE", flush=True)

if family in G.ML_FOLD_REFUSED:
    # a plane-pair product on a family without a FOLD instance; fp32 families hand over fp32 planes
    how, _ = G.ML_FOLD_REFUSED[family]
    kf, layout = G.ML_REFUSED_K_FOLD, fam["layouts"][0]
    d = G.ml_data(M, N, kf, True)
    line = {"family": family, "kind": "refused", "layout": layout, "K": kf, "how": how}
    fa, fra = pair(d["a_hi"], d["a_lo"], "dense", ab)
    bh, bl = (d["b_hi"], d["b_lo"]) if layout == "NT" else (d["b_hi"].T, d["b_lo"].T)
    fb, frb = pair(bh, bl, "dense", ab)
    fa, fb = fa.to(dev), fb.to(dev)
    b = G.buffers(G.CONFIG["none_f32"], M, N)
    c = torch.full((b["c"]["elems"],), NAN, dtype=torch.float32, device=dev)
    set_switches()
    lib.dm_prof_enable(1)
    try:
        ops.gemm(DM_NT if layout == "NT" else DM_NN, planes(fa, fra, M, kf), planes(fb, frb, *bh.shape), c[off:], M, N, kf, ldc=b["c"]["ld"])
    except Exception as e:
        line["error"] = "%s: %s" % (type(e).__name__, e)
        print("CASE " + json.dumps(line), flush=True)
        sys.exit(4 if any(w in line["error"].lower() for w in HIP_WORDS) else 3)
    torch.cuda.synchronize()
    lib.dm_prof_enable(0)
    rows = (_lib.DmProfRow * 64)()
    n = lib.dm_prof_collect(rows, 64)
    line["rows"] = [rows[i].name.decode() for i in range(n)]
    codes = [int(r.rsplit("_t", 1)[1]) for r in line["rows"]]
    ref = G.ml_ref(d, G.CONFIG["none_f32"])
    got = c.cpu()[torch.from_numpy(b["c"]["idx"])]
    line["exact"] = {"c": same_bits(got, ref["c"], got.dtype, False)}
    line["declined"] = how == "plan" and len(codes) == 1 and codes[0] not in fam["codes"]
    print("CASE " + json.dumps(line), flush=True)
    sys.exit(3 if line["declined"] else 0)
"""


def _code(rows):
    assert len(rows) == 1, rows
    return int(rows[0].rsplit("_t", 1)[1])


def _child(family, part):
    if _DEAD:
        pytest.fail(f"not started: an earlier child ended abnormally ({_DEAD[0]})")
    env = dict(os.environ, DM_PROF_SHAPES="1")
    for k in ONCE_PER_PROCESS:
        env.pop(k, None)
    try:
        run = subprocess.run([sys.executable, "-c", CHILD, ROOT, family, part], env=env, cwd=ROOT, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _DEAD.append(f"{family}: no end after {TIMEOUT} s")
        pytest.fail(f"{family}: the child did not end within {TIMEOUT} s\n{(e.stdout or b'')[-2000:]}\n{(e.stderr or b'')[-2000:]}")
    if run.returncode not in (0, 3):        # 3: a plain refusal before any launch (the child says so); anything else may be a fault
        _DEAD.append(f"{family}: exit status {run.returncode}")
    lines = [json.loads(l[len("CASE "):]) for l in run.stdout.splitlines() if l.startswith("CASE ")]
    return run, lines


def _check(family, l, bad, slices=None):
    """The four checks of one product's line."""
    fam = G.FAMILIES[family]
    cfg = G.ML_CONFIG[l.get("config", "none_f32")]
    tag = (l["kind"], l["layout"], l["K"], l.get("placement"), l.get("config", "none_f32"))
    code = "-"
    if fam["codes"]:
        if len(l["rows"]) != 1 or _code(l["rows"]) not in fam["codes"]:
            bad.append((tag, "ran on another family", l["rows"]))
        else:
            code = _code(l["rows"])
    elif l["rows"]:
        bad.append((tag, "left a profiler row: not the generic path", l["rows"]))
    if family == "kslices" and l.get("slab") != slices:
        bad.append((tag, f"the split-K slab was not written by exactly {slices} slices", l.get("slab")))
    if set(l["exact"]) != ({"c", "c_lo"} if cfg["c"] == G.PAIR else {"c"}):
        bad.append((tag, "checks missing", l["exact"]))
    for op, ok in l["exact"].items():
        if not ok:
            bad.append((tag, f"{op}: not bit-identical to the spec", l.get("wrong")))
    if set(l["sentinel"]) != {"c", "a", "b"} | ({"res"} if cfg["res"] else set()):
        bad.append((tag, "sentinel counts missing", l["sentinel"]))
    for op, nbytes in l["sentinel"].items():
        if nbytes != 0:
            bad.append((tag, f"{op}: {nbytes} bytes outside the written window changed"))
    if l.get("placement") == "far" and l.get("same_as_dense") is not True:
        bad.append((tag, "the far placement's C differs from the dense one's"))
    ok = not bad or bad[-1][0] != tag
    print(f"  [gemm_ml] {family:<8s} {l['kind']:<5s} {l['layout']} {'k_fold' if l['kind'] == 'fold' else 'K'}={l['K']:<5d} {str(l.get('placement') or '-'):<5s} "
          f"{l.get('config', 'none_f32'):<13s} code={code} {'ok' if ok else 'FAILED'}")


@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_gemm_mainloop_family(family):
    fam = G.FAMILIES[family]
    run, lines = _child(family, "cases")
    refused = G.ML_FOLD_REFUSED.get(family)
    assert run.returncode == (3 if refused else 0) and "\nDONE" in "\n" + run.stdout, (run.returncode, run.stdout[-1500:], run.stderr[-3000:])

    # exactly the documented products ran: the cases, the walk, the refusal
    want = [dict(c) for c in G.ml_cases(family)]
    if family in G.ML_WALK:
        WM, WN, WK = G.ML_WALK[family]
        want += [dict(kind="walk", layout=lay, K=WK, M=WM, N=WN) for lay in fam["layouts"]]
    if refused:
        want.append(dict(kind="refused", layout=fam["layouts"][0], K=G.ML_REFUSED_K_FOLD, how=refused[0]))
    ident = lambda l: {k: l[k] for k in ("kind", "layout", "K", "placement", "config", "M", "N", "how") if k in l}
    assert [ident(l) for l in lines] == want
    assert set(G.ML_FOLD) | set(G.ML_FOLD_REFUSED) == set(G.FAMILIES)

    bad = []
    M, N, _ = fam["shape"]
    for l in lines:
        if l["kind"] == "refused":
            # dm_gemm refused (its message names k_fold), or the family's plan declined and another family's row was left
            if l["how"] == "dm_gemm":
                if "k_fold" not in l.get("error", "") or "rows" in l:
                    bad.append(("refused", "dm_gemm did not refuse the plane pair", l))
            elif l.get("declined") is not True or l.get("exact") != {"c": True}:
                bad.append(("refused", "the family's plan did not hand the plane pair to another family", l))
            print(f"  [gemm_ml] {family:<8s} fold  {l['layout']} k_fold={l['K']:<5d} dense refused ({l['how']}): {l.get('error') or l.get('rows')}")
            continue
        k_all = 3 * l["K"] if l["kind"] == "fold" else l["K"]
        _check(family, l, bad, len(G.ml_slices(family, k_all, l.get("M"), l.get("N"))) if family == "kslices" else None)
    assert not bad, bad


def test_gemm_mainloop_walk_w4():
    """The persistent 4-wave kernel: cus + cus / 2 + 1 row tiles on cus workgroups, a tile boundary after two and after four K steps."""
    family = "w4"
    run, lines = _child(family, "walk_w4")
    assert run.returncode == 0 and run.stdout.rstrip().endswith("DONE"), (run.returncode, run.stdout[-1500:], run.stderr[-3000:])
    assert [(l["K"], l["layout"]) for l in lines] == [(K, lay) for K in G.ML_WALK_W4_K for lay in G.FAMILIES[family]["layouts"]]
    bad = []
    for l in lines:
        cus = l["cus"]
        assert (l["M"], l["N"]) == G.ml_walk_w4(cus) and cus < (l["M"] + 255) // 256 < 2 * cus and l["M"] % 256 != 0      # two tiles or one; the last ragged
        _check(family, l, bad)
    assert not bad, bad
