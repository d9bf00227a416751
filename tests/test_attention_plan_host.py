"""CPU: the four attention routing queries answer from the plan (csrc/dm_attention_plan.h) exactly as the routing did before the plan
existed.  The expected values were taken from the library of the commit before the plan (4150e6c), not from the plan; every rule of
the routing that a query can see decides at least one row (reference shapes: nets/ShfitScaleFormer.py:84-156 token cubes (S, 8, 8) of
64 S tokens, v5's 64 S + 1, vit_model.py N = 197, ViT-H/14 N = 257 / D = 80)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


# (environment, [((B, N, H, D, dtype (1 = bf16, 0 = fp32), token cube or None),
#                 (dm_attention_relpos_inkernel, dm_attention_bwd_batch_chunks, dm_attention_split_ok, dm_attention_split_bwd_chunks))])
# What decides the rows, in order.  No switches: the two table cubes; N != 64 S; not an (S, 8, 8) cube; fp32 (register kernels, their
# batch_chunk; the split entries take it); D = 80 (generic); B * H = 24 < 96 (the split entries take any batch); B * H = 96; v5's 193
# (ragged with a slab: register kernels); 197 (the same; split: no table needed); N = 128 (pipeline, not the 32-row kernels); N = 64;
# N = 257 (generic); fp32 again without a cube; ragged 160; a small ragged fp32 batch; the 32-bit DMA offset limit at H = 21845 |
# 21846; H * blocks = 32 per sample.  DM_ATTN_PIPE=0: the 32-row BACKWARD sits behind the pipeline's gate, the slab falls to the
# register kernels' chunks, the split entries do not care.  =2 lifts only its own B * H rule.  DM_ATTN_Q32=0 | DM_ATTN_Q32_BWD=0 | 3 |
# DM_ATTN_Q32_TABKV=0: no table in the kernel, the slab's chunks stay the pipeline's.  DM_ATTN_X3=0: the split entries only.
# All three =2: the small batch is taken, also 1 sample x 1 head; ragged N stays refused.
CASES = [
    ({}, [
        ((64, 256, 12, 64, 1, (4, 8, 8)), (1, 10, 1, 10)),
        ((64, 192, 12, 64, 1, (3, 8, 8)), (1, 10, 1, 10)),
        ((64, 192, 12, 64, 1, (4, 8, 8)), (0, 10, 0, 10)),
        ((64, 256, 12, 64, 1, (4, 4, 16)), (0, 10, 0, 10)),
        ((64, 256, 12, 64, 0, (4, 8, 8)), (0, 8, 1, 10)),
        ((64, 256, 12, 80, 1, (4, 8, 8)), (0, 10, 0, 10)),
        ((2, 256, 12, 64, 1, (4, 8, 8)), (0, 2, 1, 2)),
        ((8, 256, 12, 64, 1, (4, 8, 8)), (1, 8, 1, 8)),
        ((64, 193, 12, 64, 1, (3, 8, 8)), (0, 8, 0, 10)),
        ((256, 197, 12, 64, 1, None), (0, 32, 1, 10)),
        ((64, 128, 12, 64, 1, None), (0, 16, 0, 16)),
        ((64, 64, 12, 64, 1, None), (0, 32, 0, 16)),
        ((64, 257, 12, 64, 1, None), (0, 8, 0, 7)),
        ((64, 256, 12, 64, 0, None), (0, 8, 1, 10)),
        ((64, 160, 12, 64, 1, None), (0, 16, 1, 10)),
        ((3, 197, 12, 64, 0, None), (0, 3, 1, 3)),
        ((1, 256, 21845, 64, 1, (4, 8, 8)), (1, 1, 1, 1)),
        ((1, 256, 21846, 64, 1, (4, 8, 8)), (0, 1, 0, 1)),
        ((256, 256, 16, 64, 1, (4, 8, 8)), (1, 8, 1, 8)),
    ]),
    ({'DM_ATTN_PIPE': '0'}, [
        ((64, 256, 12, 64, 1, (4, 8, 8)), (0, 8, 1, 10)),
        ((64, 192, 12, 64, 1, (3, 8, 8)), (0, 16, 1, 10)),
        ((2, 256, 12, 64, 1, (4, 8, 8)), (0, 2, 1, 2)),
    ]),
    ({'DM_ATTN_PIPE': '2'}, [
        ((2, 256, 12, 64, 1, (4, 8, 8)), (0, 2, 1, 2)),
        ((64, 256, 12, 64, 1, (4, 8, 8)), (1, 10, 1, 10)),
    ]),
    ({'DM_ATTN_Q32': '0'}, [
        ((64, 256, 12, 64, 1, (4, 8, 8)), (0, 10, 1, 10)),
    ]),
    ({'DM_ATTN_Q32': '2'}, [
        ((2, 256, 12, 64, 1, (4, 8, 8)), (0, 2, 1, 2)),
    ]),
    ({'DM_ATTN_Q32_BWD': '0'}, [
        ((64, 256, 12, 64, 1, (4, 8, 8)), (0, 10, 1, 10)),
    ]),
    ({'DM_ATTN_Q32_BWD': '2'}, [
        ((2, 256, 12, 64, 1, (4, 8, 8)), (0, 2, 1, 2)),
    ]),
    ({'DM_ATTN_Q32_BWD': '3'}, [
        ((64, 256, 12, 64, 1, (4, 8, 8)), (0, 10, 1, 10)),
        ((64, 192, 12, 64, 1, (3, 8, 8)), (0, 10, 1, 10)),
    ]),
    ({'DM_ATTN_Q32_TABKV': '0'}, [
        ((64, 256, 12, 64, 1, (4, 8, 8)), (0, 10, 1, 10)),
    ]),
    ({'DM_ATTN_X3': '0'}, [
        ((64, 256, 12, 64, 1, (4, 8, 8)), (1, 10, 0, 10)),
        ((256, 197, 12, 64, 1, None), (0, 32, 0, 10)),
    ]),
    ({'DM_ATTN_PIPE': '2', 'DM_ATTN_Q32': '2', 'DM_ATTN_Q32_BWD': '2'}, [
        ((2, 256, 12, 64, 1, (4, 8, 8)), (1, 2, 1, 2)),
        ((1, 192, 1, 64, 1, (3, 8, 8)), (1, 1, 1, 1)),
        ((2, 193, 12, 64, 1, None), (0, 2, 1, 2)),
    ]),
]


@pytest.mark.parametrize("env,rows", CASES, ids=[",".join(f"{k}={v}" for k, v in e.items()) or "none" for e, _ in CASES])
def test_queries_answer_as_before_the_plan(built_lib, env, rows):
    """One child process per environment: the DM_ATTN_* switches are read once per process."""
    code = ("import sys, json; sys.path.insert(0, %r); from deepmerge_amd import _lib; l = _lib.lib(); out = []\n"
            "for (B, N, H, D, dt, cube), _ in %r:\n"
            "    s, h, w = cube or (0, 0, 0)\n"
            "    out.append((l.dm_attention_relpos_inkernel(B, N, H, D, s, h, w, dt), l.dm_attention_bwd_batch_chunks(B, N, H, dt),\n"
            "                l.dm_attention_split_ok(B, N, H, D, int(cube is not None), s, h, w), l.dm_attention_split_bwd_chunks(B, N, H)))\n"
            "print(json.dumps(out))" % (ROOT, rows))
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DM_ATTN_")}
    got = json.loads(subprocess.run([sys.executable, "-c", code], env={**clean, **env}, capture_output=True, text=True, check=True).stdout)
    for (call, want), have in zip(rows, got):
        assert tuple(have) == want, (env, call)
