"""CPU side of the GEMM epilogue tests: the float64 spec of dm_gemm's fused epilogue, the data, the error bounds and the case table.

Shared by tests/test_gemm_host.py (no GPU: pins the spec, the exactness of the data and the constants of the bounds) and
tests/test_gpu_gemm_epilogues.py (every kernel family's epilogue against the spec).  numpy / torch float64 only.
The weight gradient (DM_TN) has its own section below FAMILIES: families and shapes, the library's split rules restated, data, spec and
frames of tests/test_gpu_gemm_wgrad.py.  The K loop of the forward / dgrad products (NT, NN) has the last section: contraction lengths per family,
plane-pair products and their frames, the tile walk -- the case table of tests/test_gpu_gemm_mainloop.py.

Spec (the order of dm_gemm_emit, deepmerge_amd/csrc/dm_gemm_common.h): v = acc + bias; GELU (the pre-activation v is saved first), GELU_GRAD (gelu'(v)
is saved), DGELU (v *= gelu'(aux)) or MUL (v *= aux); + residual; + old C; rounding to c_dtype (DM_BF16_PAIR: hi = bf16(v),
lo = bf16(v - hi)).  Row m of C / residual / aux lives at (m / rows_per_group) * group_stride + (m % rows_per_group) * ld (dm_gemm_row).

Two classes of check.  EXACT: every configuration without a transcendental, and the saved pre-activation of GELU -- the data is built
so that every intermediate is a float32 whatever the order of the additions and with or without fused multiply-add, so the kernel's
result is compared bit for bit.  BOUNDED: GELU output, saved GELU' and DGELU, inside a bound derived below.
"""
import math

import numpy as np
import torch

from rows_ref import C_BF16, U, UB, worst  # noqa: F401  (the rounding model and err / tol reduction of the row-kernel tests)

F32, BF16, PAIR = "f32", "bf16", "pair"
PAD_ROWS = 256          # rows of sentinel below M in every allocation
VIEW_OFFSET = 8         # every view starts this many elements into its allocation
GROUP_ROWS = 41         # rows_per_group of the grouped configurations: divides no tile, no 16-row MFMA tile, no 8-row item
E_AS = 1.5e-7           # |erf error| of Abramowitz-Stegun 7.1.26 (the comment of dm_gelu_parts_fast, deepmerge_amd/csrc/dm_common.h)

# ---- configurations --------------------------------------------------------------------------------------------------------------
# aux: None (no operand), "null" (GELU without a saved operand: inference), or (dtype, "save" | "read")
CONFIGS = (
    dict(id=1, name="none_f32", epi="none", bias=False, res=False, aux=None, c=F32, acc=False, grouped=False),              # lean key 0,0,1,0
    dict(id=2, name="none_bf16", epi="none", bias=False, res=False, aux=None, c=BF16, acc=False, grouped=False),            # 0,0,0,0
    dict(id=3, name="bias_res_f32", epi="none", bias=True, res=True, aux=None, c=F32, acc=False, grouped=False),            # 1,0,1,0
    dict(id=4, name="acc_f32", epi="none", bias=False, res=False, aux=None, c=F32, acc=True, grouped=False),                # 0,1,1,0
    dict(id=5, name="bias_res_acc_f32", epi="none", bias=True, res=True, aux=None, c=F32, acc=True, grouped=False),         # run-time lean form
    dict(id=6, name="gelu_bf16_nosave", epi="gelu", bias=True, res=False, aux="null", c=BF16, acc=False, grouped=False),    # 0,0,0,0 + GELU
    dict(id=7, name="gelu_save_bf16", epi="gelu", bias=True, res=False, aux=(BF16, "save"), c=BF16, acc=False, grouped=False),          # 0,0,0,1
    dict(id=8, name="gelugrad_save_bf16", epi="gelu_grad", bias=True, res=False, aux=(BF16, "save"), c=BF16, acc=False, grouped=False),  # 0,0,0,1
    dict(id=9, name="gelu_save_f32", epi="gelu", bias=True, res=False, aux=(F32, "save"), c=F32, acc=False, grouped=False),  # run-time lean form
    dict(id=10, name="mul_bf16", epi="mul", bias=False, res=False, aux=(BF16, "read"), c=BF16, acc=False, grouped=False),    # 0,2,0,0
    dict(id=11, name="dgelu_f32_res", epi="dgelu", bias=False, res=True, aux=(F32, "read"), c=F32, acc=False, grouped=False),  # run-time lean form
    dict(id=12, name="pair_gelu", epi="gelu", bias=True, res=False, aux=(BF16, "save"), c=PAIR, acc=False, grouped=False),   # run-time lean form
    dict(id=13, name="grouped41", epi="none", bias=True, res=True, aux=None, c=F32, acc=False, grouped=True),                # lean form refused
    dict(id=14, name="grouped41_gelugrad", epi="gelu_grad", bias=False, res=False, aux=(BF16, "save"), c=BF16, acc=False, grouped=True),
)
CONFIG = {c["name"]: c for c in CONFIGS}
ALL = tuple(c["name"] for c in CONFIGS)


def lean_key(cfg):
    """dm_epi_lean_key restated: RES | YL << 1 | C32 << 3 | XS << 4, -1 for grouped rows, 1 << 8 for plane pairs."""
    if cfg["grouped"]:
        return -1
    if cfg["c"] == PAIR:
        return 1 << 8
    aux = cfg["aux"] if isinstance(cfg["aux"], tuple) else None
    c32 = cfg["c"] == F32
    yl = 1 if (c32 and cfg["acc"]) else ((3 if aux[0] == F32 else 2) if aux and aux[1] == "read" else 0)
    xs = (2 if aux[0] == F32 else 1) if aux and aux[1] == "save" else 0
    return int(cfg["res"]) | (yl << 1) | (int(c32) << 3) | (xs << 4)


SPECIALISED_KEYS = (0, 1 | (1 << 3), 1 << 3, (1 << 1) | (1 << 3), 1 << 4, 2 << 1)      # dm_epi_key_specialised

# ---- families --------------------------------------------------------------------------------------------------------------------
# The proposed shape is M, N, K = 328, 200, 192: 328 = 8 * 41 = 2 * 128 + 72 = 256 + 72 = 5 * 64 + 8, 200 = 128 + 72 = 192 + 8, three K steps
# of 64.  Every family needs two tiles in M and in N, a last row of tiles with a partially filled wave block AND a wave block that starts
# past M, an N tail (N % 8 == 0) that ends inside a wave's columns, and two or three K steps; where the proposal cannot give that, the
# nearest shape that does is taken and the reason stands next to it.  `wave` = (rows, columns) of a wave's block, `tile` = (rows, columns)
# of the workgroup's tile, `bk` = the K step.  `env`: the switches read_switches (deepmerge_amd/csrc/dm_gemm.hip) reads on every call; a key set to
# None is removed from the environment.  `codes`: the `_t<code>` of the family's profiler row (prof_family_code), () = no row at all.
_OFF = {"DM_GEMM_W4": "0", "DM_GEMM_Q4": "0", "DM_GEMM_T96": "0", "DM_GEMM_RING": "0", "DM_GEMM_256": "0", "DM_GEMM_FORCE_TILE": "0", "DM_GEMM_RING_WM": None}
_Q4_SKIPS = {
    "bias_res_acc_f32": "dm_gemm_q4.hip dm_gemm_q4_plan: `if (!dm_epi_key_specialised(dm_epi_lean_key(p, 64))) return false` (residual + accumulate has no straight-line instance)",
    "gelu_save_f32": "dm_gemm_q4.hip dm_gemm_q4_plan: `if (!dm_epi_key_specialised(...)) return false` (fp32 aux written)",
    "dgelu_f32_res": "dm_gemm_q4.hip dm_gemm_q4_plan: `if (!dm_epi_key_specialised(...)) return false` (fp32 aux read + residual)",
    "pair_gelu": "dm_gemm_q4.hip dm_gemm_q4_plan: `... || p.c_dtype == DM_BF16_PAIR) return false`",
    "grouped41": "dm_gemm_q4.hip dm_gemm_q4_plan: `if (!dm_epi_key_specialised(...)) return false` (grouped rows: dm_epi_lean_key is -1)",
    "grouped41_gelugrad": "dm_gemm_q4.hip dm_gemm_q4_plan: `if (!dm_epi_key_specialised(...)) return false` (grouped rows: dm_epi_lean_key is -1)",
}
_T96_EPI = "dm_gemm_t96.hip dm_gemm_t96_plan: `if (p.epilogue != DM_EPI_NONE || p.accumulate) return false`"
_T96_KEY = "dm_gemm_t96.hip dm_gemm_t96_plan: `if (!(key == 0 || key == (1 << 3) || key == (1 | (1 << 3)))) return false`"
_T96_SKIPS = {
    "acc_f32": _T96_EPI + " (accumulate)",
    "bias_res_acc_f32": _T96_EPI + " (accumulate)",
    "gelu_bf16_nosave": _T96_EPI + " (GELU; its lean key is 0)",
    "gelu_save_bf16": _T96_EPI + " (GELU)",
    "gelugrad_save_bf16": _T96_EPI + " (GELU_GRAD)",
    "gelu_save_f32": _T96_EPI + " (GELU)",
    "mul_bf16": _T96_EPI + " (MUL)",
    "dgelu_f32_res": _T96_EPI + " (DGELU)",
    "pair_gelu": "dm_gemm_t96.hip dm_gemm_t96_plan: `... || p.k_fold > 0 || p.c_dtype == DM_BF16_PAIR) return false`",
    "grouped41": _T96_KEY + " (grouped rows: dm_epi_lean_key is -1)",
    "grouped41_gelugrad": _T96_EPI + " (GELU_GRAD; grouped rows: dm_epi_lean_key is -1)",
}
_PAIR_F32 = {"pair_gelu": "dm_gemm.hip gemm_prepare: `a plane-pair result needs an NT / NN bf16 product ...` (ab_dtype == DM_BF16)"}
_GENERIC_SKIPS = {name: "dm_gemm.hip gemm_generic: `a->ab_dtype == DM_F32 && a->c_dtype == DM_F32 && (a->aux == nullptr || a->aux_dtype == DM_F32)` (the generic path is fp32-only)"
                  for name in ("none_bf16", "gelu_bf16_nosave", "gelu_save_bf16", "gelugrad_save_bf16", "mul_bf16", "pair_gelu", "grouped41_gelugrad")}
_GENERIC_SKIPS["grouped41"] = "dm_gemm.hip gemm_generic: `DM_REQUIRE(a->rows_per_group == 0, ...)` (grouped rows need the MFMA path)"

FAMILIES = {
    # 64 x 64 tiles, a wave owns 32 x 32: rows 320 .. 351 are partially filled (8 rows), 352 .. 383 start past M
    "t64": dict(ab=BF16, shape=(328, 200, 192), layouts=("NT", "NN"), tile=(64, 64), wave=(32, 32), bk=64, codes=(64,), fast=True,
                env=dict(_OFF, DM_GEMM_FORCE_TILE="64"), skips={}),
    # 128 x 128 tiles, a wave owns 64 x 64.  M = 328 leaves rows 256 .. 319 full and 320 .. 383 partial: no wave block starts past M.
    # M = 296 = 2 * 128 + 40 = 7 * 41 + 9 is the nearest M (in steps of 8, towards fewer rows) whose last tile has both: 256 .. 319 partial, 320 .. 383 past M
    "t128": dict(ab=BF16, shape=(296, 200, 192), layouts=("NT", "NN"), tile=(128, 128), wave=(64, 64), bk=64, codes=(128,), fast=True,
                 env=dict(_OFF, DM_GEMM_FORCE_TILE="128"), skips={}),
    # fp32 operands (exact erff GELU, dm_gemm_emit / the strips with FAST = false).  gemm_prepare sends fp32 products with fewer than 16 tiles
    # of 128 x 128 to the generic path (`((M + BM - 1) / BM) * ((N + BN - 1) / BN) < 16`): N = 712 = 5 * 128 + 72 = 11 * 64 + 8 gives 18 and keeps
    # the same N tail; the K step of the fp32 tiles is 32, so K = 96 is three steps
    "f32_t64": dict(ab=F32, shape=(328, 712, 96), layouts=("NT", "NN"), tile=(64, 64), wave=(32, 32), bk=32, codes=(64,), fast=False,
                    env=dict(_OFF, DM_GEMM_FORCE_TILE="64"), skips=_PAIR_F32),
    "f32_t128": dict(ab=F32, shape=(296, 712, 96), layouts=("NT", "NN"), tile=(128, 128), wave=(64, 64), bk=32, codes=(128,), fast=False,
                     env=dict(_OFF, DM_GEMM_FORCE_TILE="128"), skips=_PAIR_F32),     # M = 296: as for t128
    # ring kernel (NT only), WM 8: 256 x 128 tiles, a wave owns 128 x 64: rows 256 .. 383 partial, 384 .. 511 past M
    "ring8": dict(ab=BF16, shape=(328, 200, 192), layouts=("NT",), tile=(256, 128), wave=(128, 64), bk=64, codes=(2568,), fast=True,
                  env=dict(_OFF, DM_GEMM_RING="2", DM_GEMM_RING_WM="8"), skips={}),
    # WM 4: 128 x 128 tiles, a wave owns 64 x 64: M = 296 as for t128
    "ring4": dict(ab=BF16, shape=(296, 200, 192), layouts=("NT",), tile=(128, 128), wave=(64, 64), bk=64, codes=(1288,), fast=True,
                  env=dict(_OFF, DM_GEMM_RING="2", DM_GEMM_RING_WM="4"), skips={}),
    # four workgroups per CU, 128 x 128 tiles, a wave owns 64 x 64; dm_gemm_q4_plan: `if (p.M % 64 != 0) return false` -> M = 320: rows 256 .. 319
    # full, 320 .. 383 past M; only the straight-line epilogues
    "q4": dict(ab=BF16, shape=(320, 200, 192), layouts=("NT", "NN"), tile=(128, 128), wave=(64, 64), bk=64, codes=(1284,), fast=True,
               env=dict(_OFF, DM_GEMM_Q4="2"), skips=_Q4_SKIPS),
    # one-round DMA-ring tiles, 128 x 96, a wave owns 64 x 48 (STAGES = 4 K tiles in LDS).  dm_gemm_t96_plan: `if (p.M % 64 != 0) return false` -> the
    # proposal's M = 320 = 2 * 128 + 64: rows 256 .. 319 full, 320 .. 383 past M; N = 200 = 2 * 96 + 8: three column tiles, the tail inside the
    # first wave's 48 columns.  Only none_f32, none_bf16 and bias_res_f32 have an instance (lean keys 1 << 3, 0 and 1 | 1 << 3)
    "t96": dict(ab=BF16, shape=(320, 200, 192), layouts=("NT", "NN"), tile=(128, 96), wave=(64, 48), bk=64, codes=(12896,), fast=True,
                env=dict(_OFF, DM_GEMM_T96="2"), skips=_T96_SKIPS),
    # 4-wave persistent kernel, 256 x 192 tiles, a wave pair owns 128 rows x 192 columns.  dm_gemm_w4_plan: `k_eff % (2 * bk_eff) != 0 || p.N % TN != 0`
    # return 0 -> N = 384 (two tiles, no N tail exists for this family), K = 256 (four K steps, the smallest even count above two)
    "w4": dict(ab=BF16, shape=(328, 384, 256), layouts=("NT", "NN"), tile=(256, 192), wave=(128, 192), bk=64, codes=(1924,), fast=True,
               env=dict(_OFF, DM_GEMM_W4="2"), skips={}),
    # 256 x 256 pipeline (one tile per workgroup), a wave owns 128 x 64: N = 200 is one tile, N = 328 = 256 + 72 is two with the same tail
    "p256": dict(ab=BF16, shape=(328, 328, 192), layouts=("NT", "NN"), tile=(256, 256), wave=(128, 64), bk=64, codes=(256,), fast=True,
                 env=dict(_OFF, DM_GEMM_256="2"), skips={}),
    # forward / dgrad K slices.  plan_fwd_split(M = 328, N = 200, K = 1536): N % 8 == 0 and K >= 1536; 3 * 2 = 6 tiles of 128 x 128 < 256; split = 4 gives
    # K / 4 = 384 < 8 * 64, split = 2 gives 768 >= 512; 6 * 2 < 512 -> two slices on 64 x 64 tiles, summed and emitted by splitk_epilogue_kernel (dm_gemm_emit8).
    # DM_GEMM_FORCE_TILE must be absent (`!sw.force_tile_set`); the row carries the tile, 64 -- the same code as unsplit 64 x 64 tiles, so the
    # GPU test also prefills the call's split-K slab (workspace slot "gemm") with NaN and requires both slices of it to have been written
    "kslices": dict(ab=BF16, shape=(328, 200, 1536), layouts=("NT", "NN"), tile=(64, 64), wave=(32, 32), bk=64, codes=(64,), fast=True,
                    env=dict(_OFF, DM_GEMM_FORCE_TILE=None), skips={}),
    # generic fp32 path by shape (K = 19: K % 4 != 0): 16 x 16 outputs per workgroup, one output per thread, no profiler row
    "generic": dict(ab=F32, shape=(328, 200, 19), layouts=("NT", "NN"), tile=(16, 16), wave=(16, 16), bk=32, codes=(), fast=False,
                    env=dict(_OFF), skips=_GENERIC_SKIPS),
}


# A finding of these tests, recorded rather than hidden: the 64 x 64 strips (dm_gemm_strip_load / dm_gemm_strip_store) add a ZERO vector for an
# absent residual, so MUL's -0 (a zero accumulator times a negative aux) is stored as +0; every other form adds nothing and keeps -0, as the
# spec does.  Numerically equal; only for these (family, configuration) pairs the bit comparison maps -0 to +0 first.  Everywhere else it
# is strict.
STRIP_ZERO_SIGN = (("t64", "mul_bf16"), ("f32_t64", "mul_bf16"))


def plan_fwd_split(M, N, K):
    """deepmerge_amd/csrc/dm_gemm.hip plan_fwd_split restated for NT / NN: (slices, tile)."""
    if N % 8 != 0 or K < 1536:
        return 1, 0
    t128 = ((M + 127) // 128) * ((N + 127) // 128)
    if t128 >= 256:
        return 1, 0
    split = 4
    while split > 1 and K // split < 8 * 64:
        split >>= 1
    if split <= 1 or t128 * split >= 512:
        return 1, 0
    return split, 64


def family_configs(family):
    return tuple(n for n in ALL if n not in FAMILIES[family]["skips"])


# The operand side of NT / NN: in the 14 configurations above A and B are dense (lda = K) and unguarded.  Every family also runs none_f32
# once more per layout with A and B as views VIEW_OFFSET elements into NaN allocations: lda = K + 8, ldb = K + 8 (NT: B is [N, K]) or N + 8
# (NN: B is [K, N]), OPERAND_PAD_ROWS rows of NaN below the last row.  A read outside the window poisons the result.
FRAMED_AB = "none_f32+framed_ab"
OPERAND_PAD_ROWS = 64


def family_framed_cases(family):
    return [(lay, FRAMED_AB) for lay in FAMILIES[family]["layouts"]]


def framed_operand(rows, cols):
    """A read-only operand [rows, cols] as a framed view: (elements of the allocation, leading dimension, idx [rows, cols])."""
    ld = cols + 8
    idx = VIEW_OFFSET + np.arange(rows, dtype=np.int64)[:, None] * ld + np.arange(cols, dtype=np.int64)[None, :]
    return VIEW_OFFSET + (rows + OPERAND_PAD_ROWS) * ld, ld, idx


# ---- the weight gradient (DM_TN): families, plans, data, frames ------------------------------------------------------------------------
# dW [M, N] = dy^T x (+ old dW), db [M] = column sums of dy (+ old db); dy [K, M] and x [K, N] are row-per-k.  tests/test_gpu_gemm_wgrad.py
# runs every family at the smallest shape with two tiles in M and in N, a partly filled wave block and one that starts past M, an N tail,
# and at least two K slices whose last is shorter and ends in a partial K step -- where the family has them.  The split rules of the library
# are restated below, each with its source line; tests/test_gemm_host.py pins the slice structure of every shape, the GPU test checks it
# against the split-K slab.
CUS = 256                # compute units of the MI355X (dm_gemm_cu_count)
WG_PER_CU = 3            # dm_gemm.hip: `constexpr int WG_PER_CU = (LDS_STAGES == 1) ? 3 : 2` with DM_GEMM_LDS_STAGES 1
CS_MAX_SLICES = 64       # dm_rows.hip


def choose_split(tiles, K, bk):
    """dm_gemm.hip choose_split: `while (tiles * s < 256 * WG_PER_CU && s < 32 && K / (s * 2) >= 8 * bk) s *= 2`."""
    s = 1
    while tiles * s < 256 * WG_PER_CU and s < 32 and K // (s * 2) >= 8 * bk:
        s *= 2
    return s


def pick_tile_tn(M, N, K, force_tile):
    """dm_gemm.hip pick_tile for DM_TN."""
    if force_tile in (64, 128):
        return force_tile
    t128 = ((M + 127) // 128) * ((N + 127) // 128)
    if t128 >= 256:
        return 128
    return 128 if (K > 4096 and t128 >= 64) else 64


def colsum_region_floats(M):
    """dm_gemm.hip colsum_region_floats: `(fused > alone ? fused : alone) + 64`, fused = 128 M, alone = dm_colsum_partial_floats(M) = 64 M."""
    return max(128 * M, CS_MAX_SLICES * M) + 64


def tn_workspace_bytes(M, N, K, force_tile=0):
    """dm_gemm.hip dm_gemm_workspace_bytes for DM_TN: `(s > 1 ? s * M * N * 4 : 0) + colsum_region_floats(M) * 4`, s = choose_split(tiles, K, 32)."""
    tile = pick_tile_tn(M, N, K, force_tile)
    s = choose_split(((M + tile - 1) // tile) * ((N + tile - 1) // tile), K, 32)
    return (s * M * N * 4 if s > 1 else 0) + colsum_region_floats(M) * 4


def cut_workspace(nbytes, M, colsum):
    """dm_gemm.hip cut_workspace: (bytes of the split-K slab, byte offset of the column-sum region or None)."""
    if not colsum:
        return nbytes, None
    need = colsum_region_floats(M) * 4
    assert nbytes >= need
    slab = (nbytes - need) & ~15
    return slab, slab


def _slices(K, split, bk):
    """`kps = ((K + split - 1) / split + bk - 1) / bk * bk; split = (K + kps - 1) / kps` (gemm_plan, dm_gemm256_plan)."""
    kps = ((K + split - 1) // split + bk - 1) // bk * bk
    return (K + kps - 1) // kps, kps


def plan_tile_tn(M, N, K, tile, bk, slab_bytes):
    """dm_gemm.hip gemm_plan, the TILE branch for a weight gradient without a caller's split_k: `split = can_split ? choose_split(tiles_m *
    tiles_n, K, bk) : 1; while (split > 1 && split * M * N * 4 > slab_bytes) split >>= 1`.  Returns (slices, k_per_split)."""
    split = choose_split(((M + tile - 1) // tile) * ((N + tile - 1) // tile), K, bk) if slab_bytes > 0 else 1
    while split > 1 and split * M * N * 4 > slab_bytes:
        split >>= 1
    return _slices(K, split, bk)


def plan_p256_tn(M, N, K, slab_bytes):
    """dm_gemm256.hip dm_gemm256_plan, the slice loop: `for (sp = 1; sp <= 32; ++sp) { if (sp > 1 && (K / sp < 8 * BK256 || sp * M * N * 4 >
    workspace_bytes)) break; eff = wg / (((wg + 255) / 256) * 256); if (eff > best + 0.04) { best = eff; split = sp; } }`."""
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    split, best = 1, 0.0
    if slab_bytes > 0:
        for sp in range(1, 33):
            if sp > 1 and (K // sp < 8 * 64 or sp * M * N * 4 > slab_bytes):
                break
            wg = tiles * sp
            eff = wg / (((wg + 255) // 256) * 256)
            if eff > best + 0.04:
                best, split = eff, sp
    return _slices(K, split, 64)


def plan_w4_tn(M, N, k_eff, bk_eff, slab_bytes, cus=CUS):
    """dm_gemm_w4.hip dm_gemm_w4_plan, DM_TN: `split = cus / tiles; if (split > 16) split = 16; per = (steps + split - 1) / split; per += per & 1;
    if (per < 16) per = 16; split = (steps + per - 1) / per; while (split > 1 && split * M * N * 4 > workspace_bytes) { per += 2; ... }`.
    k_eff, bk_eff: K and 64, or for plane pairs k_fold and 32 (slices in contraction positions of ONE piece)."""
    assert M % 256 == 0 and N % 192 == 0 and k_eff % (2 * bk_eff) == 0
    tiles = (M // 256) * (N // 192)
    steps = k_eff // bk_eff
    split = min(cus // tiles, 16)
    per = (steps + split - 1) // split
    per += per & 1
    per = max(per, 16)
    split = (steps + per - 1) // per
    while split > 1 and split * M * N * 4 > slab_bytes:
        per += 2
        split = (steps + per - 1) // per
    return split, per * bk_eff


def plan_generic_tn(M, N, K, slab_bytes, colsum, skinny_on=True):
    """dm_gemm.hip gemm_generic, the skinny rule: `if (skinny_on && a->workspace && !a->colsum_a && a->K >= 1024 && tiles16 <= 128) { slices =
    512 / tiles16; if (slices > K / 128) slices = K / 128; if (slices > 32) slices = 32; while (slices > 1 && slices * M * N * 4 > slab_bytes)
    slices >>= 1; }` and `k_per_split = ((K + slices - 1) / slices + 31) / 32 * 32`."""
    tiles16 = ((N + 15) // 16) * ((M + 15) // 16)
    slices = 1
    if skinny_on and slab_bytes > 0 and not colsum and K >= 1024 and tiles16 <= 128:
        slices = min(512 // tiles16, K // 128, 32)
        while slices > 1 and slices * M * N * 4 > slab_bytes:
            slices >>= 1
    if slices > 1:
        return _slices(K, slices, 32)
    return 1, K


def plan_grouped(shapes, k_eff, bk_eff, mode, cus=CUS):
    """dm_gemm_w4.hip dm_gemm_w4_grouped_plan for products of one contraction length: ("one_slice", 1, k_eff), ("sliced", S, k_per_split) or
    None.  one_slice: `n >= 2 && same_acc && tiles <= cus && (mode == 2 || (tiles / cus >= 0.4 && k_max <= 12288))`; sliced: `S = cus / tiles;
    if (S > 16) S = 16; per = (steps + S - 1) / S; per += per & 1; if (per < 16) per = 16; S = (steps + per - 1) / per` with `S >= 2 && mode != 2`
    and `mode == 4 || (k_max > 12288 && tiles * S / cus >= 0.85)` (the slabs fit: ops.gemm_grouped asks for 16 slices of room)."""
    tiles = sum((M // 256) * (N // 192) for M, N in shapes)
    steps = k_eff // bk_eff
    if len(shapes) >= 2 and tiles <= cus and (mode == 2 or (tiles / cus >= 0.4 and k_eff <= 12288)):
        return "one_slice", 1, k_eff
    S = min(cus // tiles, 16)
    per = (steps + S - 1) // S
    per += per & 1
    per = max(per, 16)
    S = (steps + per - 1) // per
    if len(shapes) >= 2 and S >= 2 and mode != 2 and (mode == 4 or (k_eff > 12288 and tiles * S / cus >= 0.85)):
        return "sliced", S, per * bk_eff
    return None


def colsum_rows_alone(K, M, lda):
    """dm_rows.hip dm_colsum on dy [K, M]: the rows [M] it leaves in its scratch.  `slices = (M + 255) / 256` (M there = K here), capped at 64,
    evened out; one slice in the vector form (`(N % 4 == 0) && (ldx % 4 == 0)`, 16-byte aligned) goes straight to the destination."""
    slices = min((K + 255) // 256, CS_MAX_SLICES)
    rps = (K + slices - 1) // slices
    slices = (K + rps - 1) // rps
    vec = M % 4 == 0 and lda % 4 == 0
    return 0 if (slices == 1 and vec) else slices


def k_slices(K, split, kps):
    return [(z * kps, min(K, (z + 1) * kps)) for z in range(split)]


# env: as for FAMILIES (read_switches reads it on every call).  shapes: (M, N, K of the sliced cases, K of the unsplit short case).  fold:
# (M, N, k_fold) of the plane-pair case.  cs: how the column sums of dy come about -- "fused" (rows [M] per K slice from the product's own
# kernel: gemm_plan `pl.cs_fused`, `cs_rows_per_slice`) or "alone" (dm_colsum).  The shapes are the proposal's except where noted.
_WOFF = dict(_OFF, DM_GEMM_T96="0", DM_GEMM_W4_TN=None, DM_GEMM_GROUPED=None)
WG_FAMILIES = {
    # 64 x 64 tiles (a wave owns 32 x 32): 328 = 5 * 64 + 8, 200 = 3 * 64 + 8.  choose_split(24 tiles, 1100, 64) = 2 -> slices of 576 and 524 = 8 * 64 + 12
    "t64": dict(ab=BF16, codes=(64,), env=dict(_WOFF, DM_GEMM_FORCE_TILE="64"), kind="tile", tile=64, bk=64, cs="fused", cs_rows=1,
                shapes=((328, 200, 1100, 76),), fold=(328, 200, 384)),
    # 128 x 128 tiles (a wave owns 64 x 64): M = 296 as in FAMILIES.  The column sums come from dm_colsum (cs_t64 needs tile == 64)
    "t128": dict(ab=BF16, codes=(128,), env=dict(_WOFF, DM_GEMM_FORCE_TILE="128"), kind="tile", tile=128, bk=64, cs="alone", cs_rows=0,
                 shapes=((296, 200, 1100, 76),), fold=None),
    # fp32 operands, K step 32 (for DM_TN gemm_prepare's "fewer than 16 tiles" rule does not apply): choose_split(.., 1100, 32) = 4 -> 288, 288, 288, 236 = 7 * 32 + 12
    "f32_t64": dict(ab=F32, codes=(64,), env=dict(_WOFF, DM_GEMM_FORCE_TILE="64"), kind="tile", tile=64, bk=32, cs="alone", cs_rows=0,
                    shapes=((328, 200, 1100, 44),), fold=None),
    "f32_t128": dict(ab=F32, codes=(128,), env=dict(_WOFF, DM_GEMM_FORCE_TILE="128"), kind="tile", tile=128, bk=32, cs="alone", cs_rows=0,
                     shapes=((296, 200, 1100, 44),), fold=None),
    # 256 x 256 pipeline.  The proposal expected 4 slices of 576 for K = 2056; the slice loop of dm_gemm256_plan takes a slice count only when it
    # fills the 256 CUs better by MORE than 0.04 (`eff > best + 0.04`): 4 tiles x 3 slices = 12 / 256 = 0.047 is taken, x 4 = 0.0625 is not.  So
    # K = 2056 gives 3 slices of 704, 704 and 648 = 10 * 64 + 8: two slices or more, the last shorter and ending in a partial K step -- the
    # structure asked for, so the shape stays.  The plane-pair case (k_fold = 704, K = 2112) has one slice per K segment.
    "p256": dict(ab=BF16, codes=(256,), env=dict(_WOFF, DM_GEMM_256="2"), kind="p256", tile=256, bk=64, cs="fused", cs_rows=4,
                 shapes=((328, 328, 2056, 72),), fold=(328, 328, 704)),
    # 4-wave kernel: whole 256 x 192 tiles and K % 128 == 0 only, so the edges are the strides, the rows behind K and the short last slice:
    # 34 K steps -> per = 16 -> slices of 1024, 1024 and 128.  Plane pairs: 34 steps of 32 -> 512, 512, 64 positions of each piece
    "w4": dict(ab=BF16, codes=(1924,), env=dict(_WOFF, DM_GEMM_W4="2", DM_GEMM_W4_TN="2"), kind="w4", tile=(256, 192), bk=64, cs="fused", cs_rows=1,
               shapes=((256, 192, 2176, 1024), (512, 384, 2176, 1024)), fold=(256, 192, 1088)),
    # generic fp32 path (M % 4 != 0): no profiler row.  28 tiles of 16 x 16 -> 16 slices by the rule, 8 inside the slab dm_gemm_workspace_bytes
    # declares: 7 of 288 and one of 34 (wave 0 gets 32 of it, wave 1 two, the others none), then sgemm_small_reduce_kernel.  With column sums
    # wanted the rule leaves the product unsliced (`!a->colsum_a`)
    "generic": dict(ab=F32, codes=(), env=dict(_WOFF), kind="generic", tile=16, bk=32, cs="alone", cs_rows=0,
                    shapes=((102, 50, 2050, 19),), fold=None),
}
# dm_gemm_grouped: two products in one launch of the 4-wave kernel.  DM_GEMM_GROUPED = 4: the sliced form (3 slices, as w4 alone), = 2: the
# one-slice form; the rule itself leaves so small a group (3 tiles) to the separate calls, which here is a failure.
WG_GROUP = dict(ab=BF16, env=dict(_WOFF, DM_GEMM_W4="2", DM_GEMM_W4_TN="2"), shapes=((256, 192), (512, 192)), cs_rows=1,
                cases=(dict(name="sliced", K=2176, mode=4, fold=False, acc=False, cs="store"),
                       dict(name="sliced_acc", K=2176, mode=4, fold=False, acc=True, cs="add"),
                       dict(name="one_slice", K=1024, mode=2, fold=False, acc=False, cs="store"),
                       dict(name="one_slice_acc", K=1024, mode=2, fold=False, acc=True, cs="add"),
                       dict(name="fold_sliced", K=1088, mode=4, fold=True, acc=True, cs="store"),
                       dict(name="fold_one_slice", K=512, mode=2, fold=True, acc=False, cs="add")))
WG_ALL = tuple(WG_FAMILIES) + ("grouped",)
GROUP_MIN_SLABS = 16     # deepmerge_amd/ops.py gemm_grouped: `min_slabs=16 if layout == DM_TN else 0`


def wg_cases(family):
    """The products a weight-gradient family runs: dict(name, M, N, K, fold, acc, cs) with cs = None | "store" | "add" (colsum_accumulate).
    Per shape: the sliced contraction plain, with accumulate + column sums, and with added column sums; the unsplit short contraction with
    accumulate on (straight to C), without and with column sums.  Plane pairs (K = k_fold): accumulate and column sums."""
    f = WG_FAMILIES[family]
    out = []
    for si, (M, N, K, Ks) in enumerate(f["shapes"]):
        tag = "" if len(f["shapes"]) == 1 else f"@{M}x{N}"
        for name, k, acc, cs in (("split", K, False, None), ("split_acc_cs", K, True, "store"), ("split_csadd", K, False, "add"),
                                 ("short_acc", Ks, True, None), ("short_acc_csadd", Ks, True, "add")):
            out.append(dict(name=name + tag, M=M, N=N, K=k, fold=False, acc=acc, cs=cs))
    if f["fold"]:
        M, N, kf = f["fold"]
        out.append(dict(name="fold_acc_cs", M=M, N=N, K=kf, fold=True, acc=True, cs="store"))
    return out


def wg_plan(family, case, ws_bytes=None):
    """What the library does with a case: dict(split, kps, ws_bytes (the workspace the call declares), cs ("fused" | "alone" | None), cs_rows
    (rows [M] written to the column-sum region), writes = [(first float, floats)] of the workspace that are written)."""
    f = WG_FAMILIES[family]
    M, N, K = case["M"], case["N"], case["K"]
    k_all = 3 * K if case["fold"] else K
    force = int(f["env"].get("DM_GEMM_FORCE_TILE") or 0)
    if ws_bytes is None:
        ws_bytes = tn_workspace_bytes(M, N, k_all, force)
    slab, cs_off = cut_workspace(ws_bytes, M, case["cs"] is not None)
    if f["kind"] == "tile":
        split, kps = plan_tile_tn(M, N, k_all, f["tile"], f["bk"], slab)
    elif f["kind"] == "p256":
        split, kps = plan_p256_tn(M, N, k_all, slab)
    elif f["kind"] == "w4":
        split, kps = plan_w4_tn(M, N, K, 32 if case["fold"] else 64, slab)
    else:
        split, kps = plan_generic_tn(M, N, K, slab, case["cs"] is not None)
    cs, rows = None, 0
    if case["cs"] is not None:
        cs = f["cs"]
        rows = split * f["cs_rows"] if cs == "fused" else colsum_rows_alone(K, M, M if case["fold"] else M + 8)
        if cs == "alone" and case["fold"]:
            raise AssertionError("no family sums the planes of a pair with dm_colsum in these cases")
    writes = [(0, split * M * N)] if split > 1 else []
    if rows:
        writes.append((cs_off // 4, rows * M))
    return dict(split=split, kps=kps, ws_bytes=ws_bytes, cs=cs, cs_rows=rows, writes=writes)


def wg_group_plan(case, numels=None):
    """The grouped launch of a case: dict(form, split, kps, per product: ws_bytes, writes).  numels: the sizes of the products' workspace
    buffers where they are known (ops.gemm_grouped declares the whole buffer of slot "gemm.g<i>", which only grows)."""
    g = WG_GROUP
    bk = 32 if case["fold"] else 64
    form, S, kps = plan_grouped(g["shapes"], case["K"], bk, case["mode"])
    k_all = 3 * case["K"] if case["fold"] else case["K"]
    prods = []
    for i, (M, N) in enumerate(g["shapes"]):
        nbytes = max(tn_workspace_bytes(M, N, k_all) + GROUP_MIN_SLABS * M * N * 4, 1 << 20)      # ops._gemm_args / ops.workspace
        if numels is not None:
            assert numels[i] >= nbytes
            nbytes = numels[i]
        slab, cs_off = cut_workspace(nbytes, M, True)
        writes = []
        if form == "sliced":
            writes = [(0, S * M * N), (cs_off // 4, S * M)]
        elif case["cs"] == "add":           # dm_gemm_grouped: one row for the reduction that ADDS it to colsum_a; a first write goes straight there
            writes = [(cs_off // 4, M)]
        prods.append(dict(M=M, N=N, ws_bytes=nbytes, writes=writes))
    return dict(form=form, split=S, kps=kps, products=prods)


def wg_data(M, N, K, fold=False):
    """float64 arrays, all exact in bf16 and in fp32 (cached per shape).  Plain: dy [K, M] integers in [-2, 2], x [K, N] on the 2^-6 grid with
    |x| <= 2: every product is a multiple of 2^-6 and |sum| <= 4 K, so for K <= 2304 every partial sum in any order and slicing is a float32.
    Plane pairs: +-(i + j / 1024), i in {1, 2}, j in 0 .. 3 -> hi = +-i, lo = +-j / 1024 (dy_hi, dy_lo, x_hi, x_lo): multiples of 2^-10 with
    |sum| < 4.02 K.  old_c [M, N] and old_db [M] on the 2^-6 grid."""
    key = (M, N, K, fold)
    if key in _WG_DATA:
        return _WG_DATA[key]
    rng = np.random.default_rng(7 + 1000003 * M + 1009 * N + 2 * K + int(fold))
    grid = lambda shape, lim: rng.integers(-lim, lim + 1, size=shape).astype(np.float64) / 64.0
    d = {}
    if fold:
        for nm, cols in (("dy", M), ("x", N)):
            sign = rng.integers(0, 2, size=(K, cols)).astype(np.float64) * 2 - 1
            d[nm + "_hi"] = sign * rng.integers(1, 3, size=(K, cols)).astype(np.float64)
            d[nm + "_lo"] = sign * rng.integers(0, 4, size=(K, cols)).astype(np.float64) / 1024.0
    else:
        d["dy"] = rng.integers(-2, 3, size=(K, M)).astype(np.float64)
        d["x"] = grid((K, N), 128)
    d["old_c"] = grid((M, N), 128)
    d["old_db"] = grid((M,), 128)
    for v in d.values():
        v.setflags(write=False)
    _WG_DATA[key] = d
    return d


_WG_DATA = {}


def wg_ref(d, acc, cs, fold=False, k0=0, k1=None):
    """The float64 spec over contraction rows [k0, k1): (dW, db).  Plane pairs: dW = hi^T hi + hi^T lo + lo^T hi, db = colsum(hi) + colsum(lo)."""
    sl = slice(k0, k1)
    if fold:
        ah, al, bh, bl = d["dy_hi"][sl], d["dy_lo"][sl], d["x_hi"][sl], d["x_lo"][sl]
        dw = ah.T @ bh + ah.T @ bl + al.T @ bh
        db = ah.sum(0) + al.sum(0)
    else:
        dw = d["dy"][sl].T @ d["x"][sl]
        db = d["dy"][sl].sum(0)
    if acc:
        dw = dw + d["old_c"]
    if cs == "add":
        db = db + d["old_db"]
    return dw, db


def wg_frames(M, N, K, kps, fold=False):
    """The allocations of a weight-gradient product, every view VIEW_OFFSET elements in: {"dy" | "x" | "c" | "db": dict(elems, ld, idx)}.
    dy: lda = M + 8, x: ldb = N + 16, and below row K at least one whole k_per_split of rows, so that a slice that forgets its
    `min(K, ...)` still reads inside the allocation.  Plane pairs are dense [2, K, cols] blocks (ops.gemm: lda = M), framed as a whole: idx is
    [2, K, cols].  C: ldc = N + 8 and PAD_ROWS rows below M; db: M floats and 64 behind them."""
    rows_below = max(kps, 64)
    out = {}
    for nm, cols, pad in (("dy", M, 8), ("x", N, 16)):
        k = np.arange(K, dtype=np.int64)[:, None]
        c = np.arange(cols, dtype=np.int64)[None, :]
        if fold:
            idx = VIEW_OFFSET + np.stack([k * cols + c, K * cols + k * cols + c])
            out[nm] = dict(elems=VIEW_OFFSET + (2 * K + rows_below) * cols, ld=cols, idx=idx, plane=K * cols)
        else:
            ld = cols + pad
            out[nm] = dict(elems=VIEW_OFFSET + (K + rows_below) * ld, ld=ld, idx=VIEW_OFFSET + k * ld + c)
    ldc = N + 8
    out["c"] = dict(elems=VIEW_OFFSET + (M + PAD_ROWS) * ldc, ld=ldc,
                    idx=VIEW_OFFSET + np.arange(M, dtype=np.int64)[:, None] * ldc + np.arange(N, dtype=np.int64)[None, :])
    out["db"] = dict(elems=VIEW_OFFSET + M + 64, ld=M, idx=VIEW_OFFSET + np.arange(M, dtype=np.int64))
    return out


# ---- addressing and buffers --------------------------------------------------------------------------------------------------------
def row_offsets(M, ld, rows_per_group=0, group_stride=0):
    """dm_gemm_row restated: element offset of every output row."""
    m = np.arange(M, dtype=np.int64)
    if rows_per_group > 0:
        return (m // rows_per_group) * group_stride + (m % rows_per_group) * ld
    return m * ld


def buffers(cfg, M, N):
    """The allocation of every operand a configuration has: {"c" | "aux" | "res": dict(dtype, ld, elems, idx, written)} plus the grouped-row
    arguments.  idx [M, N] = flat element index of output (m, n) inside the allocation (plane pairs: idx of the hi plane, "plane" = the lo
    plane's distance).  Plain rows: ldc = N + 8, ldaux = N + 16, ldr = N + 24 (plane pairs: ldc = N, as gemm_prepare demands).  Grouped rows:
    one leading dimension N + 8 for all three, because dm_gemm_row gives them one group_stride = 41 * ld + 64."""
    out = {"rows_per_group": 0, "group_stride": 0}
    if cfg["grouped"]:
        ld = N + 8
        rpg, gs = GROUP_ROWS, GROUP_ROWS * ld + 64
        out.update(rows_per_group=rpg, group_stride=gs)
        lds = {"c": ld, "aux": ld, "res": ld}
        extent = ((M + rpg - 1) // rpg) * gs
    else:
        rpg = gs = 0
        lds = {"c": N if cfg["c"] == PAIR else N + 8, "aux": N + 16, "res": N + 24}
        extent = None
    cols = np.arange(N, dtype=np.int64)[None, :]

    def one(dtype, ld, written, pair=False):
        ro = row_offsets(M, ld, rpg, gs)
        if pair:
            elems = VIEW_OFFSET + 2 * M * N + PAD_ROWS * ld
        else:
            elems = VIEW_OFFSET + (extent if extent is not None else M * ld) + PAD_ROWS * ld
        d = dict(dtype=dtype, ld=ld, elems=int(elems), idx=VIEW_OFFSET + ro[:, None] + cols, written=written)
        if pair:
            d["plane"] = M * N
        return d

    out["c"] = one(BF16 if cfg["c"] == PAIR else cfg["c"], lds["c"], True, pair=cfg["c"] == PAIR)
    if isinstance(cfg["aux"], tuple):
        out["aux"] = one(cfg["aux"][0], lds["aux"], cfg["aux"][1] == "save")
    if cfg["res"]:
        out["res"] = one(F32, lds["res"], False)
    return out


# ---- data --------------------------------------------------------------------------------------------------------------------------
def k_shift(K):
    """Operands are integers in [-2, 2] (variance 2 each); A is scaled by 2^-shift so that the accumulator's spread is between 1 and 2."""
    return max(0, math.ceil(math.log2(math.sqrt(4.0 * K) / 2.0)))


_PLANT = (0.0, 6.0, -6.0, 5.5, -5.5, 0.015625, -0.015625, 1.0)      # bias of the first and the last eight columns


def operands(M, N, K):
    """Everything a case reads, as float64 numpy arrays (all exactly representable in bf16 resp. fp32; cached per shape):
    a [M, K], b [N, K] small integers (a times 2^-shift), acc = a b^T; bias, res, old_c, aux_mul on the 2^-6 grid with |.| <= 2;
    aux_dgelu on the 2^-6 grid over [-6.5, 6.5].  Rows 0 and M - 1 of a are zero, so those rows of the pre-activation are the bias, which
    carries exact zeros, both signs and +-5.5 / +-6 (erf saturated in fp32) in its first and last eight columns."""
    key = (M, N, K)
    if key in _OPERANDS:
        return _OPERANDS[key]
    rng = np.random.default_rng(1000003 * M + 1009 * N + K)
    a = rng.integers(-2, 3, size=(M, K)).astype(np.float64) * 2.0 ** -k_shift(K)
    b = rng.integers(-2, 3, size=(N, K)).astype(np.float64)
    a[0] = 0.0
    a[M - 1] = 0.0
    grid = lambda shape, lim: rng.integers(-lim, lim + 1, size=shape).astype(np.float64) / 64.0
    bias = grid((N,), 128)
    bias[:8] = _PLANT
    bias[N - 8:] = _PLANT[::-1]
    d = dict(a=a, b=b, acc=a @ b.T, bias=bias, res=grid((M, N), 128), old_c=grid((M, N), 128), aux_mul=grid((M, N), 128),
             aux_dgelu=grid((M, N), 416))
    d["aux_dgelu"][0, :8] = _PLANT
    d["aux_dgelu"][M - 1, N - 8:] = _PLANT
    for v in d.values():
        v.setflags(write=False)
    _OPERANDS[key] = d
    return d


_OPERANDS = {}


def case(cfg, M, N, K):
    """A configuration with the operand values it reads (the argument of epilogue_ref)."""
    d = operands(M, N, K)
    c = dict(cfg)
    c["bias_v"] = d["bias"] if cfg["bias"] else None
    c["res_v"] = d["res"] if cfg["res"] else None
    c["old_c"] = d["old_c"] if cfg["acc"] else None
    c["aux_v"] = None
    if isinstance(cfg["aux"], tuple) and cfg["aux"][1] == "read":
        c["aux_v"] = d["aux_mul"] if cfg["epi"] == "mul" else d["aux_dgelu"]
    return c


# ---- the spec ------------------------------------------------------------------------------------------------------------------------
def gelu64(x):
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x * (1.0 + torch.special.erf(torch.from_numpy(x / math.sqrt(2.0))).numpy())


def dgelu64(x):
    x = np.asarray(x, dtype=np.float64)
    cdf = 0.5 * (1.0 + torch.special.erf(torch.from_numpy(x / math.sqrt(2.0))).numpy())
    return cdf + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def round_bf16(x):
    """float64 -> nearest bf16 (ties to even), returned as float64.  Exact for the EXACT class, whose values are float32 already."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def round_to(x, dtype):
    if dtype == BF16:
        return round_bf16(x)
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def epilogue_ref(acc, cfg):
    """What dm_gemm leaves in C and in aux for accumulator `acc` (float64) under `cfg` (see case()).  Returns a dict:
    v     the unrounded result, float64                          c     v rounded to c_dtype (plane pairs: the hi plane)
    c_lo  plane pairs: bf16(v - hi)                              pre   the pre-activation acc + bias (GELU-type epilogues)
    aux_v the unrounded saved operand (saving epilogues)         aux   aux_v rounded to the aux dtype"""
    v = np.array(acc, dtype=np.float64)
    out = {}
    if cfg["bias_v"] is not None:
        v = v + cfg["bias_v"][None, :]
    epi = cfg["epi"]
    if epi == "gelu":
        out["pre"] = v
        if isinstance(cfg["aux"], tuple):
            out["aux_v"] = v
        v = gelu64(v)
    elif epi == "gelu_grad":
        out["pre"] = v
        out["aux_v"] = dgelu64(v)
        v = gelu64(v)
    elif epi == "dgelu":
        v = v * dgelu64(cfg["aux_v"])
    elif epi == "mul":
        v = v * cfg["aux_v"]
    if cfg["res_v"] is not None:
        v = v + cfg["res_v"]
    if cfg["old_c"] is not None:
        v = v + cfg["old_c"]
    out["v"] = v
    if cfg["c"] == PAIR:
        out["c"] = round_bf16(v)
        out["c_lo"] = round_bf16(v - out["c"])
    else:
        out["c"] = round_to(v, cfg["c"])
    if "aux_v" in out:
        out["aux"] = round_to(out["aux_v"], cfg["aux"][0])
    return out


def is_exact(cfg):
    """(C exact, saved aux exact): compared bit for bit."""
    return cfg["epi"] in ("none", "mul"), cfg["epi"] == "gelu"


# ---- float32 restatements of the kernels' arithmetic ---------------------------------------------------------------------------------
f32 = np.float32


def _fma(a, b, c):
    """fl32(a * b + c) with one rounding: the product of two float32 is exact in float64; the sum's float64 rounding is far below a float32 ulp."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def gelu_parts_fast32(x):
    """dm_gelu_parts_fast (deepmerge_amd/csrc/dm_common.h) operation by operation in float32; a correctly rounded exp2 and 1 / x stand in for v_exp_f32 and
    v_rcp_f32 (__expf(x) is exp2(x * log2 e))."""
    x = np.asarray(x, dtype=f32)
    z = np.abs(x) * f32(0.70710678118654752440)
    arg = (-(z * z)) * f32(1.4426950408889634)
    e = np.exp2(arg.astype(np.float64)).astype(f32)
    t = (1.0 / _fma(f32(0.3275911), z, f32(1.0)).astype(np.float64)).astype(f32)
    poly = _fma(t, f32(1.061405429), f32(-1.453152027))
    poly = _fma(t, poly, f32(1.421413741))
    poly = _fma(t, poly, f32(-0.284496736))
    poly = _fma(t, poly, f32(0.254829592))
    poly = t * poly
    erf_abs = _fma(-poly, e, f32(1.0))
    cdf = f32(0.5) * (f32(1.0) + np.copysign(erf_abs, x))
    pdf = f32(0.39894228040143267794) * e
    return cdf, pdf


def _erf32(x):
    """A correctly rounded erff."""
    return torch.special.erf(torch.from_numpy(np.asarray(x, dtype=f32).astype(np.float64))).numpy().astype(f32)


def gelu32(x, fast):
    x = np.asarray(x, dtype=f32)
    if fast:
        return x * gelu_parts_fast32(x)[0]                                            # dm_gelu_fast
    return (f32(0.5) * x) * (f32(1.0) + _erf32(x * f32(0.70710678118654752440)))      # dm_gelu


def dgelu32(x, fast):
    x = np.asarray(x, dtype=f32)
    if fast:
        cdf, pdf = gelu_parts_fast32(x)
        return _fma(x, pdf, cdf)                                                      # dm_dgelu_fast
    cdf = f32(0.5) * (f32(1.0) + _erf32(x * f32(0.70710678118654752440)))
    pdf = f32(0.39894228040143267794) * np.exp(((f32(-0.5) * x) * x).astype(np.float64)).astype(f32)
    return cdf + x * pdf                                                              # dm_dgelu


def restate32(acc, cfg, fast, order="left", fma=False):
    """The epilogue in float32, operation by operation (unrounded-to-c_dtype result `v`, saved operand `aux_v`, both float32).
    order = "left": ((acc + bias) ... + residual) + old C, the kernels' order; "right": the additive operands are summed first and joined
    to the accumulator last (bias + (residual + old C) where no multiply stands between them).  fma: multiply-adds fused (one rounding)."""
    v = np.asarray(acc, dtype=np.float64).astype(f32)
    assert np.array_equal(v.astype(np.float64), acc), "the accumulator must be a float32"
    g = lambda k: None if cfg[k] is None else np.asarray(cfg[k], dtype=np.float64).astype(f32)
    bias, res, old, aux = g("bias_v"), g("res_v"), g("old_c"), g("aux_v")
    out = {}
    epi = cfg["epi"]
    tail = [t for t in (res, old) if t is not None]
    if epi == "none" and order == "right":
        adds = ([np.broadcast_to(bias[None, :], v.shape)] if bias is not None else []) + tail
        if adds:
            s = adds[-1]
            for t in adds[-2::-1]:
                s = t + s
            v = v + s
        out["v"] = v
        return out
    if bias is not None:
        v = v + bias[None, :]
    if epi == "gelu":
        out["aux_v"] = v
        v = gelu32(v, fast)
    elif epi == "gelu_grad":
        out["aux_v"] = dgelu32(v, fast)
        v = gelu32(v, fast)
    mult = None
    if epi == "dgelu":
        mult = dgelu32(aux, fast)
    elif epi == "mul":
        mult = aux
    if order == "right" and len(tail) == 2:
        tail = [tail[0] + tail[1]]
    if mult is not None:
        if fma and tail:
            v = _fma(v, mult, tail[0])
            tail = tail[1:]
        else:
            v = v * mult
    for t in tail:
        v = v + t
    out["v"] = v
    return out


# ---- bounds --------------------------------------------------------------------------------------------------------------------------
# GELU, its derivative and DGELU are the only inexact steps.  With the fast parts (bf16-operand kernels) the error of the CDF is E_AS / 2 from
# the polynomial plus about one U of rounding (the last fma and the halving are the only roundings at unit scale: t, the polynomial and
# exp(-x^2 / 2) carry relative errors of a few U into a product poly * e <= 1); with erff (fp32 operands) it is the roundings alone.
#     gelu(x)  = x cdf                      |error| <= C_G  D |x|                  D = E_AS / 2 + U  (fast)   or   U  (erff)
#     gelu'(x) = cdf + x pdf                |error| <= C_D  D                      (|x pdf| <= 0.25 and its relative error (1 + x^2) U stay inside D)
#     acc gelu'(aux) + res                  |error| <= C_DG (D |acc| + U |result|) (the factor's error scaled by |acc|; product and sum rounded once each)
# A bf16 destination adds one rounding to 8 bits: tol + C_BF16 2^-8 (|value| + tol), the form of rows_ref.  Each constant is the smallest integer
# for which the float32 restatement above stays at or below HALF the bound on the data of every case (tests/test_gemm_host.py asserts both
# directions), so a correct kernel has a factor 2 to spare for the 1-ulp v_exp_f32 / v_rcp_f32 and the library's erff / expf.
C = {(True, "gelu"): 3, (True, "dgelu"): 1, (True, "muld"): 4,           # fast parts: C_G, C_D, C_DG
     (False, "gelu"): 3, (False, "dgelu"): 1, (False, "muld"): 5}        # erff / expf
# (C_D: the derivative is only ever SAVED as bf16 in these configurations, so the rounding to 8 bits dominates its bound)


def unit(fast):
    return E_AS / 2 + U if fast else U


def with_bf16(tol, value, dtype):
    return tol + C_BF16 * UB * (np.abs(value) + tol) if dtype == BF16 else tol


def bounds(cfg, ref, acc, fast, consts=None):
    """{"c": tol or None, "aux": tol or None}: None where the class is EXACT (or nothing is stored)."""
    k = dict(C) if consts is None else consts
    D = unit(fast)
    out = {"c": None, "aux": None}
    epi = cfg["epi"]
    cdt = BF16 if cfg["c"] == PAIR else cfg["c"]
    if epi in ("gelu", "gelu_grad"):
        tol = k[(fast, "gelu")] * D * np.abs(ref["pre"])
        # plane pairs: hi + lo restores the fp32 result to 2^-16 relative (two roundings to 8 bits); the GPU test compares the SUM of the planes
        out["c"] = tol + UB * UB * np.abs(ref["v"]) if cfg["c"] == PAIR else with_bf16(tol, ref["v"], cdt)
        if epi == "gelu_grad":
            out["aux"] = with_bf16(k[(fast, "dgelu")] * D * np.ones_like(ref["v"]), ref["aux_v"], cfg["aux"][0])
    elif epi == "dgelu":
        out["c"] = with_bf16(k[(fast, "muld")] * (D * np.abs(acc) + U * np.abs(ref["v"])), ref["v"], cdt)
    return out


def family_cases(family):
    """(layout, config name) of everything a family runs."""
    return [(lay, n) for lay in FAMILIES[family]["layouts"] for n in family_configs(family)]


# ---- the main loop of the forward / dgrad products (NT, NN): K-step counts and plane pairs ------------------------------------------------
# tests/test_gpu_gemm_mainloop.py runs every family of FAMILIES at M, N of its shape over a list of contraction lengths (ML_K), the families
# with a FOLD instance over hi / lo plane pairs with one, two and three K tiles per segment (ML_FOLD), and once on a tile walk of eleven row
# tiles (ML_WALK).  Everything is EXACT: the data of operands() / wg_data() sums exactly in float32 in any order (tests/test_gemm_host.py),
# so C is compared bit for bit.
ML_K = {
    # one to five K steps of 64: touch_at = max(0, nk - 4) of gemm_kernel on both sides of nk - 4 (bias_res_f32 has the residual that arms it);
    # an 8-wide K tail alone (8), behind one (72) and behind two (136) full steps
    "t64": (8, 64, 72, 128, 136, 192, 256, 320),
    "t128": (8, 64, 72, 128, 136, 192, 256, 320),
    # fp32 operands: the K step is 32, the tail 4 wide
    "f32_t64": (4, 32, 36, 64, 96, 128, 160),
    "f32_t128": (4, 32, 36, 64, 96, 128, 160),
    # dm_gemm_ring.hip: two A buffers, one B buffer, the `more` branch -> 1 .. 5 steps (depth 2 + 3)
    "ring8": (64, 128, 192, 256, 320),
    "ring4": (64, 128, 192, 256, 320),
    # dm_gemm_q4.hip: "one LDS stage" -> depth 1
    "q4": (64, 128, 192, 256, 320),
    # dm_gemm256.hip: `LDS256 = 2 * BUF_BYTES`: two K-tile buffers, the prologue stages tile 0 and most of tile 1 -> depth 2
    "p256": (64, 128, 192, 256, 320),
    # dm_gemm_t96.hip: `STAGES = 4` -> 1 .. STAGES + 2 steps
    "t96": (64, 128, 192, 256, 320, 384),
    # dm_gemm_w4.hip: `LDS_BYTES = 2 * BUF_BYTES + ...`: two buffers; dm_gemm_w4_plan: `k_eff % (2 * bk_eff) != 0 ... return 0` -> K % 128 == 0:
    # 2, 4, 6, 8 steps
    "w4": (128, 256, 384, 512),
    # plan_fwd_split: 1536 -> two slices of 768; 1600 -> 832 + 768; 2048 -> four slices of 512
    "kslices": (1536, 1600, 2048),
    # sgemm_small_kernel: four waves share K in pieces of 32: one wave with one product, one wave short, two waves (32 + 1)
    "generic": (1, 19, 33),
}
ML_DEPTH = {"t64": 2, "t128": 2, "f32_t64": 2, "f32_t128": 2, "ring8": 2, "ring4": 2, "q4": 1, "p256": 2, "t96": 4, "w4": 2}   # K tiles in flight / in LDS
# (family, K) a plan refuses, with the refusing line: none of the listed K is refused (tests/test_gemm_host.py restates each plan's K rule)
ML_K_SKIPS = {}

# plane pairs: k_fold = 64, 128, 192 -> one, two, three K tiles per segment, the seams at K tiles 1|2, 2|4, 3|6: both buffer parities
# (4-wave kernel: 2, 4, 6 steps of 32 positions per segment).  kslices: k_fold = 512 -> K = 1536, slices [0, 768) and [768, 1536): the seam at
# 512 inside slice 0, the one at 1024 inside slice 1; k_fold = 576 -> K = 1728, slices [0, 896) and [896, 1728), seams at 576 and 1152
ML_FOLD = {"t64": (64, 128, 192), "t128": (64, 128, 192), "ring8": (64, 128, 192), "ring4": (64, 128, 192), "p256": (64, 128, 192),
           "w4": (64, 128, 192), "kslices": (512, 576)}
# The families without a FOLD instance.  "dm_gemm": the call is refused before any launch (status 3 of the child).  "plan": the family's plan
# returns false and dm_gemm_plan goes on to the register-staged tiles, which do have one -- dm_gemm itself does not refuse; the child
# requires the row of another family and then ends with status 3 like a refusal.
ML_FOLD_REFUSED = {
    "q4": ("plan", "dm_gemm_q4.hip dm_gemm_q4_plan: `if (p.K % dmq4::BK != 0 || p.N % 8 != 0 || p.k_fold > 0 || p.c_dtype == DM_BF16_PAIR) return false`"),
    "t96": ("plan", "dm_gemm_t96.hip dm_gemm_t96_plan: `if (p.K % dmt96::BK != 0 || p.N % 8 != 0 || p.k_fold > 0 || p.c_dtype == DM_BF16_PAIR) return false`"),
    "f32_t64": ("dm_gemm", "dm_gemm.hip k_fold_fault: `if (!(a.ab_dtype == DM_BF16 && a.K == 3 * a.k_fold && a.k_fold % 64 == 0)) return 1`"),
    "f32_t128": ("dm_gemm", "dm_gemm.hip k_fold_fault: `if (!(a.ab_dtype == DM_BF16 && a.K == 3 * a.k_fold && a.k_fold % 64 == 0)) return 1`"),
    "generic": ("dm_gemm", "dm_gemm.hip k_fold_fault: `if (!(a.ab_dtype == DM_BF16 && a.K == 3 * a.k_fold && a.k_fold % 64 == 0)) return 1` (gemm_prepare asks it before the generic path is chosen)"),
}
ML_REFUSED_K_FOLD = 64
PLACEMENTS = ("dense", "far")
FAR_GAP = 8 * 37        # elements of NaN between the planes of a "far" pair: a weight's mirror pair (Planes.t.stride(0) is not rows * cols)

PAIR_NONE = dict(id=15, name="pair_none", epi="none", bias=False, res=False, aux=None, c=PAIR, acc=False, grouped=False)   # lean key 1 << 8
ML_CONFIG = {n: CONFIG[n] for n in ("none_f32", "none_bf16", "bias_res_f32")}
ML_CONFIG["pair_none"] = PAIR_NONE
ML_PLAIN_CONFIGS = ("none_f32", "none_bf16", "bias_res_f32")
ML_FOLD_CONFIGS = ("none_f32", "none_bf16", "bias_res_f32", "pair_none")     # gemm_prepare allows a pair result for every NT / NN bf16 product


def ml_configs(family, fold):
    """The configurations a family runs in the main-loop tests (the generic path is fp32 throughout: no none_bf16)."""
    names = ML_FOLD_CONFIGS if fold else ML_PLAIN_CONFIGS
    return tuple(n for n in names if n not in FAMILIES[family]["skips"] or n == "pair_none")


def ml_cases(family):
    """Every product of a family, in the order the child runs them: dict(kind = "plain" | "fold", layout, K (plain) or k_fold, placement
    (None for plain), config)."""
    f = FAMILIES[family]
    out = []
    for K in ML_K[family]:
        if (family, K) in ML_K_SKIPS:
            continue
        for lay in f["layouts"]:
            for name in ml_configs(family, False):
                out.append(dict(kind="plain", layout=lay, K=K, placement=None, config=name))
    for kf in ML_FOLD.get(family, ()):
        for lay in f["layouts"]:
            for name in ml_configs(family, True):
                for pl in PLACEMENTS:
                    out.append(dict(kind="fold", layout=lay, K=kf, placement=pl, config=name))
    return out


def ml_slices(family, K, M=None, N=None):
    """The K slices of a product of the kslices family: [(k0, k1)]; [(0, K)] for every other family.  M, N: the family's unless given (the walk)."""
    if family != "kslices":
        return [(0, K)]
    if M is None:
        M, N, _ = FAMILIES[family]["shape"]
    split, tile = plan_fwd_split(M, N, K)
    return k_slices(K, *_slices(K, split, 64))


def ml_data(M, N, K, fold=False):
    """Plain: operands(M, N, K) as it is.  Plane pairs (K = k_fold): as wg_data -- a_hi, a_lo [M, K], b_hi, b_lo [N, K] with hi = +-i, i in {1, 2}
    and lo = +-j / 1024, j in 0 .. 3, the lo planes of A and B drawn independently; acc = Ah Bh^T + Ah Bl^T + Al Bh^T (the order of the
    segments: left operand hi, hi, lo, right operand hi, lo, hi).  The omitted Al Bl^T is a multiple of 2^-20, off the 2^-10 grid of the spec.
    bias [N] and res [M, N] on the 2^-6 grid.  The planes go to the kernel as given (ops.Planes): they are not the split of anything."""
    if not fold:
        return operands(M, N, K)
    key = (M, N, K)
    if key in _ML_DATA:
        return _ML_DATA[key]
    rng = np.random.default_rng(11 + 1000003 * M + 1009 * N + K)
    d = {}
    for nm, rows in (("a", M), ("b", N)):
        sign = rng.integers(0, 2, size=(rows, K)).astype(np.float64) * 2 - 1
        d[nm + "_hi"] = sign * rng.integers(1, 3, size=(rows, K)).astype(np.float64)
        d[nm + "_lo"] = sign * rng.integers(0, 4, size=(rows, K)).astype(np.float64) / 1024.0
    d["acc"] = d["a_hi"] @ d["b_hi"].T + d["a_hi"] @ d["b_lo"].T + d["a_lo"] @ d["b_hi"].T
    d["bias"] = rng.integers(-128, 129, size=(N,)).astype(np.float64) / 64.0
    d["res"] = rng.integers(-128, 129, size=(M, N)).astype(np.float64) / 64.0
    for v in d.values():
        v.setflags(write=False)
    _ML_DATA[key] = d
    return d


_ML_DATA = {}
FOLD_SEGMENTS = (("a_hi", "b_hi"), ("a_hi", "b_lo"), ("a_lo", "b_hi"))      # a_fold = (0, 0, plane), b_fold = (0, plane, 0): ops._gemm_args


def ml_case(cfg, d):
    """A main-loop configuration with the operand values it reads (the argument of epilogue_ref)."""
    c = dict(cfg)
    c["bias_v"] = d["bias"] if cfg["bias"] else None
    c["res_v"] = d["res"] if cfg["res"] else None
    c["old_c"] = None
    c["aux_v"] = None
    return c


def ml_ref(d, cfg):
    """The float64 spec of a main-loop product: epilogue_ref on the data's accumulator."""
    return epilogue_ref(d["acc"], ml_case(cfg, d))


def ml_terms(d, fold):
    """The contraction as a list of terms, in the kernel's K order: [(A [M, k], B [N, k])] -- one term for a plain product, three for a pair."""
    if not fold:
        return [(d["a"], d["b"])]
    return [(d[a], d[b]) for a, b in FOLD_SEGMENTS]


def pair_frame(rows, cols, placement):
    """A plane pair [2, rows, cols] inside one flat bf16 allocation, VIEW_OFFSET elements in, NaN before, behind and (far) between the planes:
    dict(elems, ld, idx [2, rows, cols], plane).  dense: the planes rows * cols apart; far: rows * cols + FAR_GAP."""
    plane = rows * cols + (FAR_GAP if placement == "far" else 0)
    r = np.arange(rows, dtype=np.int64)[:, None]
    c = np.arange(cols, dtype=np.int64)[None, :]
    idx = VIEW_OFFSET + np.stack([r * cols + c, plane + r * cols + c])
    return dict(elems=VIEW_OFFSET + plane + rows * cols + OPERAND_PAD_ROWS * cols, ld=cols, idx=idx, plane=plane)


# The tile walk (dm_xcd_remap, bands of group_m = 8 row tiles): one K step, tiles_m = group_m + 3 = 11 with a ragged last tile (a last band
# of three), three column tiles (the last 8 wide), none_f32.  The grid has exactly tiles_m * tiles_n workgroups, so a tile visited twice
# leaves another unvisited: C is prefilled with NaN, and every element must be the spec's.  M = 11 * tile - 56; where the plan asks for
# M % 64 == 0 (q4, t96) 11 * tile - 64.  Exceptions, each with its reason:
#   f32_t64   gemm_prepare sends fp32 products with fewer than 16 tiles of 128 x 128 to the generic path: 6 x 2 = 12 at N = 136 -> N = 264
#             (five column tiles of 64), 6 x 3 = 18
#   kslices   a one-step product has no slices (plan_fwd_split: K >= 1536): K = 1536, two slices of twelve steps
#   generic   16 x 16 outputs on a 2-D grid (no remap, no bands); K = 19
#   w4        persistent: its own case, the shape depends on the CU count (ml_walk_w4)
GROUP_M = 8             # dm_gemm.hip gemm_plan: `p.group_m = dm_gemm_tuning().group_m >= 0 ? ... : 8`


def _walk(family):
    f = FAMILIES[family]
    tm, tn = f["tile"]
    M = (GROUP_M + 3) * tm - (64 if family in ("q4", "t96") else 56)
    N = 2 * tn + 8
    K = f["bk"]
    if family == "f32_t64":
        N = 4 * tn + 8
    if family == "kslices":
        K = 1536
    if family == "generic":
        M, K = (GROUP_M + 3) * tm - 5, 19
    return (M, N, K)


ML_WALK = {fam: _walk(fam) for fam in FAMILIES if fam != "w4"}
ML_WALK_W4_K = (128, 256)       # two and four K steps: the persistent pipeline crosses a tile boundary after two steps and after four


def ml_walk_w4(cus):
    """(M, N) of the 4-wave kernel's walk: cus + cus // 2 + 1 row tiles of 256 (the last ragged) in one column tile of 192, on min(tiles, cus)
    persistent workgroups -> workgroups run two tiles or one."""
    return 256 * (cus + cus // 2 + 1) - 56, 192


def ml_walk_data(M, N, K):
    """a [M, K], b [N, K] and acc of a walk: the integers of operands() without the M x N epilogue operands (the 4-wave walk is 98 504 rows)."""
    key = (M, N, K)
    if key not in _ML_WALK_DATA:
        rng = np.random.default_rng(5 + 1000003 * M + 1009 * N + K)
        a = rng.integers(-2, 3, size=(M, K)).astype(np.float64) * 2.0 ** -k_shift(K)
        b = rng.integers(-2, 3, size=(N, K)).astype(np.float64)
        d = dict(a=a, b=b, acc=a @ b.T)
        for v in d.values():
            v.setflags(write=False)
        _ML_WALK_DATA.clear()           # one at a time: the large ones are used once
        _ML_WALK_DATA[key] = d
    return _ML_WALK_DATA[key]


_ML_WALK_DATA = {}
