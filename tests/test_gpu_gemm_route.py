"""GPU: DM_GEMM_ROUTE, the per-product kernel-family override of dm_gemm, pinned.

The variable is read once per process, so every case runs in a fresh child process whose environment names one product per family
in DM_GEMM_ROUTE and sets the per-family variables to the OPPOSITE of each route.  The child reads the family each product ran on
from the `_t<code>` suffix of its DM_PROF_SHAPES=1 profiler row (the method of tools/which_kernel.py), compares every result with
an exact small-integer product, and finally asks libc (not os.environ, a Python-side copy) what the six variables hold.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# family -> (layout, M, N, K) of the product routed to it, and the `_t<code>` values that family prints
ROUTED = {
    "ring": (("NT", 2048, 2304, 768), (2568, 1288)),
    "q4": (("NT", 2048, 3072, 768), (1284,)),
    "w4": (("NT", 2048, 768, 768), (1924,)),
    "256": (("NN", 1024, 512, 512), (256,)),
    "128": (("NN", 256, 256, 512), (128,)),          # 4 tiles of 128 x 128: the tile rule alone picks 64
    "64": (("NT", 2048, 2048, 256), (64,)),          # 256 tiles of 128 x 128: the tile rule alone picks 128
}
ROUTED_TN = (("TN", 768, 768, 2048), (1924,))       # a second w4 product: the weight-gradient form (DM_GEMM_W4_TN)
UNNAMED = ("NT", 2048, 2304, 512)                   # legal for the ring kernel, not in DM_GEMM_ROUTE
KEYS = ("DM_GEMM_W4", "DM_GEMM_W4_TN", "DM_GEMM_Q4", "DM_GEMM_RING", "DM_GEMM_256", "DM_GEMM_FORCE_TILE")

CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from deepmerge_amd import _lib, ops
from deepmerge_amd._lib import DM_NN, DM_NT, DM_TN

dev, lib = "cuda:0", _lib.lib()
out = {"products": {}}
for spec in json.loads(sys.argv[2]):
    lay, M, N, K = spec
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    a = torch.from_numpy(rng.integers(-3, 4, size=(M, K)).astype(np.float32))
    b = torch.from_numpy(rng.integers(-3, 4, size=(N, K)).astype(np.float32))
    want = a.double() @ b.double().T
    A = (a.T.contiguous() if lay == "TN" else a).to(dev).bfloat16()
    B = (b if lay == "NT" else b.T.contiguous()).to(dev).bfloat16()
    C = torch.full((M, N), float("nan"), device=dev)
    lib.dm_prof_enable(1)
    ops.gemm({"NT": DM_NT, "NN": DM_NN, "TN": DM_TN}[lay], A, B, C, M, N, K)
    torch.cuda.synchronize()
    lib.dm_prof_enable(0)
    rows = (_lib.DmProfRow * 64)()
    n = lib.dm_prof_collect(rows, 64)
    out["products"]["%s:%dx%dx%d" % (lay, M, N, K)] = {"rows": [rows[i].name.decode() for i in range(n)],
                                                      "exact": bool(torch.equal(C.cpu().double(), want))}
getenv = ctypes.CDLL(None).getenv
getenv.restype, getenv.argtypes = ctypes.c_char_p, [ctypes.c_char_p]
out["env"] = {k: (lambda v: None if v is None else v.decode())(getenv(k.encode())) for k in json.loads(sys.argv[3])}
print("RESULT " + json.dumps(out))
"""


def _key(spec):
    return "%s:%dx%dx%d" % spec


def _family_code(rows):
    """The `_t<code>` of the one profiler row a dm_gemm call leaves."""
    assert len(rows) == 1, rows
    return int(rows[0].rsplit("_t", 1)[1])


@pytest.mark.parametrize("force_tile", ["64", "128"])
def test_gemm_route_overrides_per_product_and_leaves_the_environment(force_tile):
    route = ",".join(f"{_key(spec)}={fam}" for fam, (spec, _) in ROUTED.items()) + f",{_key(ROUTED_TN[0])}=w4"
    # the plain variables say the opposite of every route: all families off, and a forced tile (both values are run, so that the
    # `128` and the `64` route each meet the other one)
    plain = {"DM_GEMM_W4": "0", "DM_GEMM_W4_TN": "0", "DM_GEMM_Q4": "0", "DM_GEMM_RING": "0", "DM_GEMM_256": "0",
             "DM_GEMM_FORCE_TILE": force_tile}
    env = dict(os.environ, DM_GEMM_ROUTE=route, DM_PROF_SHAPES="1", **plain)
    specs = [spec for spec, _ in ROUTED.values()] + [ROUTED_TN[0], UNNAMED]
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(specs), json.dumps(KEYS)], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    got = json.loads([l for l in run.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    print(json.dumps(got, indent=1))

    for fam, (spec, codes) in list(ROUTED.items()) + [("w4", ROUTED_TN)]:
        p = got["products"][_key(spec)]
        assert _family_code(p["rows"]) in codes, (fam, p)
        assert p["exact"], (fam, p)
    # not named in DM_GEMM_ROUTE: the plain variables hold (ring, q4, w4 and the pipeline off, the forced tile)
    p = got["products"][_key(UNNAMED)]
    assert _family_code(p["rows"]) == int(force_tile), p
    assert p["exact"], p
    # the process environment is what the child was started with
    assert got["env"] == plain


# ---- dm_gemm_grouped: the one launch honours the family switches and DM_GEMM_ROUTE ----------------------------------------------------
# The smallest legal group: two bf16 DM_TN products of one 256 x 192 tile and two K steps each, both with column sums.  The rule leaves
# so small a group to the separate calls; DM_GEMM_GROUPED=2 takes the one-slice form whenever it is legal.
GROUP_SPEC = ("TN", 256, 192, 128)

GROUP_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import torch
from deepmerge_amd import _lib, ops
from deepmerge_amd._lib import DM_TN

dev, lib = "cuda:0", _lib.lib()
_, M, N, K = json.loads(sys.argv[2])
g = torch.Generator(device=dev); g.manual_seed(M + N + K)
calls, want = [], []
for i in range(2):
    dy = torch.randint(-1, 2, (K, M), device=dev, generator=g).to(torch.bfloat16)
    x = torch.randint(-1, 2, (K, N), device=dev, generator=g).to(torch.bfloat16)
    dw = torch.full((M, N), float("nan"), device=dev)
    db = torch.full((M,), float("nan"), device=dev)
    calls.append(((DM_TN, dy, x, dw, M, N, K), dict(lda=M, ldb=N, ldc=N, colsum_out=db)))
    want.append((dy.float().T @ x.float(), dy.float().sum(0), dw, db))
lib.dm_prof_enable(1)
ops.gemm_grouped(calls)
torch.cuda.synchronize()
lib.dm_prof_enable(0)
rows = (_lib.DmProfRow * 64)()
n = lib.dm_prof_collect(rows, 64)
# dm_prof_collect sums the launches of one name into one row: one entry per launch here
names = [rows[i].name.decode() for i in range(n) for _ in range(rows[i].launches)]
print("RESULT " + json.dumps({"rows": names, "exact": [bool(torch.equal(dw, w_dw) and torch.equal(db, w_db)) for w_dw, w_db, dw, db in want]}))
"""


@pytest.mark.parametrize("extra,n_rows,grouped,codes", [
    ({}, 1, True, None),                                            # the one-slice form, one launch
    ({"DM_GEMM_W4_TN": "0"}, 2, False, "not1924"),                  # the 4-wave weight-gradient form off: the separate calls, elsewhere
    ({"DM_GEMM_W4": "0"}, 2, False, "not1924"),                     # the 4-wave family off: the same
    ({"DM_GEMM_ROUTE": "TN:256x192x128=64"}, 2, False, 64),         # a member is routed: the separate calls, each routed by dm_gemm
], ids=["grouped", "w4_tn_off", "w4_off", "routed"])
def test_gemm_grouped_honours_family_switches_and_route(extra, n_rows, grouped, codes):
    """Before ABI 7 the grouped fast path ignored DM_GEMM_W4 / DM_GEMM_W4_TN / DM_GEMM_ROUTE, so an A/B run of the grouped products
    measured the 4-wave kernel whatever it had asked for.  A "row" is one profiler record (one launch scope)."""
    env = {k: v for k, v in os.environ.items() if k not in KEYS + ("DM_GEMM_ROUTE", "DM_GEMM_GROUPED")}
    env.update(DM_GEMM_GROUPED="2", DM_PROF_SHAPES="1", **extra)
    run = subprocess.run([sys.executable, "-c", GROUP_CHILD, ROOT, json.dumps(GROUP_SPEC)], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    got = json.loads([l for l in run.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    print(json.dumps(got, indent=1))
    rows = got["rows"]
    assert len(rows) == n_rows, rows
    if grouped:
        assert "grouped2" in rows[0] and "1slice" in rows[0], rows
    else:
        assert not any("grouped" in r for r in rows), rows
        got_codes = [int(r.rsplit("_t", 1)[1]) for r in rows]
        assert all(c != 1924 for c in got_codes) if codes == "not1924" else got_codes == [codes, codes], rows
    assert got["exact"] == [True, True], got
