"""GPU: the one-round 128 x 96 DMA-ring bf16 GEMM (dm_gemm_t96.hip) through the C-ABI.

Every case is one dm_gemm call routed twice with DM_GEMM_ROUTE, once to `t96` and once to `64` (the register-staged 64 x 64 tiles, which
run the same MFMAs in the same K order).  The variable is read once per process, so the two routes run in two child processes (started
together, once per module); each child reads the family that ran from the `_t<code>` suffix of the product's DM_PROF_SHAPES=1 row and
saves every output buffer.  The tests compare the two runs bit for bit and the t96 run against a float64 product of the same bf16 data.

Buffers: every operand and result lives in a larger allocation (one more row, `pad` more columns) filled with NaN (operands) or a
sentinel (results): a DMA that reads the row past M / N or the column past K, or an epilogue that writes past the logical block, shows.

Tolerance against float64 (derived, not measured): the bf16 operands are exact and so is every product in fp32; the fp32 accumulation
of K terms, the bias and the residual add err at most (K + 2) 2^-24 S with S = sum_k |a||b| + |bias| + |residual|; an fp32 result adds
its own rounding 2^-24 |ref|, a bf16 result 2^-8 |ref| (bf16's unit roundoff: half an ulp of 8 significant bits; the fp32 error in
front of that rounding is scaled by 1 + 2^-7).
"""
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T96_CODE = 12896

# name -> (layout, M, N, K, epilogue, pad, taken): epilogue h = bf16 C, f = fp32 C, rf = fp32 C + fp32 residual, each with bias;
# pad > 0: lda / ldb / ldc larger than the logical width by pad, ldr by 2 pad; taken = the t96 plan takes the product
CASES = {
    # one tile, one K tile
    "one_nt": ("NT", 128, 96, 64, "h", 0, True),
    "one_nn": ("NN", 128, 96, 64, "f", 0, True),
    # ring of four stages: shorter than, equal to, longer than the stage count, uneven wrap (17 K tiles); 2 x 2 tiles
    "ring_k128": ("NT", 256, 192, 128, "rf", 8, True),
    "ring_k192": ("NN", 256, 192, 192, "h", 8, True),
    "ring_k256": ("NT", 256, 192, 256, "f", 8, True),
    "ring_k320": ("NN", 256, 192, 320, "rf", 8, True),
    "ring_k1088_nt": ("NT", 256, 192, 1088, "h", 8, True),
    "ring_k1088_nn": ("NN", 256, 192, 1088, "f", 8, True),
    # ragged rows (second row tile half full) and columns (last column tile 8 wide: one and three column tiles)
    "rows192_nt": ("NT", 192, 96, 192, "rf", 8, True),
    "rows192_nn": ("NN", 192, 96, 192, "h", 8, True),
    "cols104_nt": ("NT", 128, 104, 192, "h", 8, True),
    "cols104_nn": ("NN", 128, 104, 192, "rf", 8, True),
    "cols200_nt": ("NT", 192, 200, 320, "f", 16, True),
    "cols200_nn": ("NN", 192, 200, 320, "h", 16, True),
    # refused by the plan: the product falls through to the register-staged tiles and is still right
    "refused_n100": ("NT", 128, 100, 128, "f", 8, False),          # N % 8 != 0
    "refused_k96": ("NT", 128, 96, 96, "h", 8, False),             # K % 64 != 0
    "refused_m200": ("NN", 200, 96, 128, "rf", 8, False),          # M % 64 != 0: the store guard is a route rule
    # the step's fc2 forward
    "fc2_fwd": ("NT", 4096, 768, 3072, "rf", 0, True),
}

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import torch
from deepmerge_amd import _lib, ops
from deepmerge_amd._lib import DM_NN, DM_NT

dev, lib = "cuda:0", _lib.lib()
cases, out_path = json.loads(sys.argv[2]), sys.argv[3]
SENTINEL = 777.0
out = {}
for name, (lay, M, N, K, epi, pad, _taken) in cases.items():
    g = torch.Generator().manual_seed(sum(map(ord, name)) + M + N + K)
    a = torch.randn(M, K, generator=g).bfloat16()
    b = (torch.randn(N, K, generator=g) * 0.25).bfloat16()
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    lda = K + pad
    A = torch.full((M + 1, lda), float("nan"), dtype=torch.bfloat16)
    A[:M, :K] = a
    if lay == "NT":
        ldb = K + pad
        B = torch.full((N + 1, ldb), float("nan"), dtype=torch.bfloat16)
        B[:N, :K] = b
    else:
        ldb = N + pad
        B = torch.full((K + 1, ldb), float("nan"), dtype=torch.bfloat16)
        B[:K, :N] = b.T
    ldc, ldr = N + pad, N + 2 * pad
    C = torch.full((M + 1, ldc), SENTINEL, dtype=torch.bfloat16 if epi == "h" else torch.float32)
    R = torch.full((M + 1, ldr), float("nan"))
    R[:M, :N] = res
    A, B, C, R, bias_d = A.to(dev), B.to(dev), C.to(dev), R.to(dev), bias.to(dev)
    kw = dict(lda=lda, ldb=ldb, ldc=ldc, bias=bias_d)
    if epi == "rf":
        kw.update(residual=R, ldr=ldr)
    lib.dm_prof_enable(1)
    ops.gemm(DM_NT if lay == "NT" else DM_NN, A, B, C, M, N, K, **kw)
    torch.cuda.synchronize()
    lib.dm_prof_enable(0)
    rows = (_lib.DmProfRow * 64)()
    n = lib.dm_prof_collect(rows, 64)
    out[name] = {"rows": [rows[i].name.decode() for i in range(n)], "C": C.cpu(), "a": a, "b": b, "bias": bias, "res": res}
torch.save(out, out_path)
print("DONE")
"""


def _key(lay, M, N, K):
    return "%s:%dx%dx%d" % (lay, M, N, K)


@pytest.fixture(scope="module")
def runs():
    """{"t96": ..., "64": ...}: every case's output under each route, from two child processes started together."""
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        procs = {}
        for fam in ("t96", "64"):
            route = ",".join(f"{_key(*c[:4])}={fam}" for c in CASES.values())
            env = {k: v for k, v in os.environ.items() if not k.startswith("DM_GEMM_")}
            env.update(DM_GEMM_ROUTE=route, DM_PROF_SHAPES="1")
            path = os.path.join(tmp, fam + ".pt")
            procs[fam] = (subprocess.Popen([sys.executable, "-c", CHILD, ROOT, json.dumps(CASES), path], env=env, cwd=ROOT,
                                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), path)
        for fam, (proc, path) in procs.items():
            so, se = proc.communicate(timeout=300)
            assert proc.returncode == 0 and "DONE" in so, (fam, so[-2000:], se[-4000:])
            got[fam] = torch.load(path)
    return got


def _code(rows):
    assert len(rows) == 1, rows
    return int(rows[0].rsplit("_t", 1)[1])


@pytest.mark.parametrize("name", list(CASES))
def test_gemm_t96_case(runs, name):
    lay, M, N, K, epi, pad, taken = CASES[name]
    new, old = runs["t96"][name], runs["64"][name]
    # which family ran
    assert (_code(new["rows"]) == T96_CODE) == taken, new["rows"]
    assert _code(old["rows"]) == 64, old["rows"]
    c_new, c_old = new["C"], old["C"]
    # nothing written outside the logical block (the row past M, the columns past N), under either route
    for c in (c_new, c_old):
        assert bool((c[M:, :] == 777.0).all()) and bool((c[:, N:] == 777.0).all()), name
    got = c_new[:M, :N]
    assert bool(torch.isfinite(got.float()).all()), f"{name}: a NaN / inf reached the output (operand rows past M / N or columns past K are NaN)"
    # bit for bit the register-staged 64 x 64 tiles' result
    assert torch.equal(got, c_old[:M, :N]), f"{name}: max diff to the 64 route {(got.double() - c_old[:M, :N].double()).abs().max()}"
    # float64 product of the same bf16 data
    a, b = new["a"].double(), new["b"].double()
    ref = a @ b.T + new["bias"].double()
    mag = a.abs() @ b.abs().T + new["bias"].double().abs()
    if epi == "rf":
        ref = ref + new["res"].double()
        mag = mag + new["res"].double().abs()
    tol = (K + 2) * 2.0 ** -24 * mag
    tol = tol * (1 + 2.0 ** -7) + 2.0 ** -8 * ref.abs() if epi == "h" else tol + 2.0 ** -24 * ref.abs()
    err = (got.double() - ref).abs()
    worst = float((err / tol.clamp_min(1e-30)).max())
    print(f"  [gemm_t96] {name:<14s} worst err/tol {worst:.3f}")
    assert worst <= 1.0, f"{name}: err/tol {worst}"


# (layout, M, N, K, epilogue): the step's products and whether the routing rule (DM_GEMM_T96 unset) sends them to this family
RULE = [
    ("NT", 4096, 768, 3072, "rf", True),       # fc2 forward
    ("NN", 4096, 768, 3072, "h", True),        # fc1 dgrad
    ("NN", 4096, 768, 2304, "h", True),        # qkv dgrad
    ("NT", 4096, 768, 768, "rf", True),        # proj forward
    ("NN", 4096, 768, 768, "h", True),         # proj / fc2 dgrad
    ("NT", 4096, 768, 512, "f", False),        # a contraction shorter than the output is wide
    ("NT", 1024, 2304, 768, "h", False),       # one round (192 tiles), but a wide output: not measured, not routed
    ("NT", 1024, 768, 3072, "rf", False),      # the 1024-token stage: 64 tiles
    ("NT", 16384, 768, 3072, "rf", False),     # the 16384-token stage: four rounds
]


@pytest.mark.parametrize("lay,M,N,K,epi,routed", RULE)
def test_gemm_t96_routing_rule(monkeypatch, lay, M, N, K, epi, routed):
    from torch.profiler import ProfilerActivity, profile

    from deepmerge_amd import ops
    from deepmerge_amd._lib import DM_NN, DM_NT
    for k in [k for k in os.environ if k.startswith("DM_GEMM_")]:
        monkeypatch.delenv(k, raising=False)
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    A = torch.randn(M, K, device=dev, generator=g).bfloat16()
    B = (torch.randn(N, K, device=dev, generator=g) if lay == "NT" else torch.randn(K, N, device=dev, generator=g)).bfloat16()
    C = torch.empty(M, N, device=dev, dtype=torch.bfloat16 if epi == "h" else torch.float32)
    kw = dict(bias=torch.randn(N, device=dev, generator=g))
    if epi == "rf":
        kw["residual"] = torch.randn(M, N, device=dev, generator=g)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        ops.gemm(DM_NT if lay == "NT" else DM_NN, A, B, C, M, N, K, **kw)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name == "CUDA"]
    assert any("gemm_t96_kernel" in n for n in names) == routed, names
