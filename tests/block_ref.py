"""fp64 restatement of the fused transformer block (ops.BlockFn) with the bf16 mode's rounding points -- plain CPU torch + autograd.

Two switches of ONE graph:
  * truth  (points=False): fp64 throughout.  The op sequence is oracle.s2former.cross_scale_block's, so on the same parameters the two
    agree to the last bit (tests/test_block_ref_host.py); with table=None it is the ViT block (vit_model.Block).
  * points (points=True): the same graph with identity nodes where the fused block rounds in "bf16" mode.  A FORWARD node (`rf`) rounds a
    value to bf16 and back and passes the gradient through; a BACKWARD node (`rb`) is the identity forward and rounds the gradient that
    flows through it.  The residual stream (x, x1, x2) and the residual gradient (dres) carry no node: they stay fp32 in the kernels.

The distance of the points run to truth is the YARDSTICK of the GPU test (tests/test_gpu_block_oracle.py): what the bf16 mode's own
rounding costs each tensor.  What separates the kernels from the points run is fp32 accumulation order and sparse one-ulp flips.

Where each point comes from (deepmerge_amd/ops.py = ops, deepmerge_amd/csrc/... = csrc); DESIGN.md "Numerics contract of the fused
block in bf16 mode" has the same list as a table.

forward
  F1 the four weights as operands        ops:1621-1622 lp_weight -> ops:1508 cast (csrc/dm_rows.hip:368 cast_bf16_kernel) or the trainer's mirror
  F2 y1 = LN1(x), y2 = LN2(x1)           ops:1634 / ops:1660, out dtype bf16: csrc/dm_rows.hip:87 dm_store4 of (v - mean) * rstd * g + b
  F3 qkv                                 ops:1639, bf16 C: csrc/dm_gemm_common.h:172 (bias added in fp32 first, :132)
  F4 probabilities before P.V            csrc/dm_attention.hip:273 (s *= inv, fp32) -> :278 contract_tokens -> :113 acc_frag (bf16_t) casts.
                                         (The persistent kernels round exp(s - max) <= 1 and divide O by the row sum afterwards,
                                         csrc/dm_attention_pipe.hip:323, csrc/dm_attention_q32.hip:578-608: the same relative rounding.)
  F5 o                                   csrc/dm_attention.hip:282 dm_store4 into the bf16 out rows
  F6 h = GELU(pre)                       ops:1664 DM_EPI_GELU_GRAD: csrc/dm_gemm_common.h:148 v * cdf -> :172 bf16 C (pre itself is never stored)
  F7 the saved GELU' image               csrc/dm_gemm_common.h:147 d = fma(v, pdf, cdf) -> :155 bf16 aux; read back by DM_EPI_MUL at :158-160
backward
  B1 operand copy of the incoming dx2    ops:1704 _operand_grad (the previous block's copy, csrc/dm_rows.hip:168, or ops:1022 cast); feeds
                                         dW2, db2 (column sums of the COPY ride on the weight gradient, ops:1730-1739) and dpre
  B2 dpre = (dy W2) * GELU'              ops:1741 DM_EPI_MUL, bf16 C: csrc/dm_gemm_common.h:160 -> :172; feeds dW1, db1, dy2
  B3 dy2                                 ops:1747, bf16 C
  B4 operand copy of dx1                 ops:1754 want_lp: csrc/dm_rows.hip:168 (dx1 itself stays fp32: :156); feeds dWp, dbp, do
  B5 do                                  ops:1763, bf16 C
  B6 dS before dQ = dS K, dK = dS^T Q    csrc/dm_attention.hip:372 / :484 pack_tiles -> :204 (bf16_t) casts.  The table gradient sums the
                                         fp32 dS (:369 hacc += dsv) in the register kernels; the table-reading dK / dV kernel sums the bf16
                                         operand (csrc/dm_attention_q32_bwd.hip:677-680) -- over hundreds of entries per bin the difference
                                         is far below the yardstick, and the restatement keeps the fp32 form.
     P^T before dV = P^T dO              csrc/dm_attention.hip:483 pack_tiles(tp); autograd's P.V node holds the F4-rounded P: the same values
  B7 dqkv                                csrc/dm_attention.hip:386 / :498 / :505 dm_store4 into the bf16 dqkv rows; feeds dWqkv, dbqkv, dy1
  B8 dy1                                 ops:1788, bf16 C
  not rounded: x1 / x2 (fp32 C + fp32 residual, ops:1659 / ops:1669), dx1 / dx (csrc/dm_rows.hip:154-156: rs * (...) + dres in fp32), every
  parameter gradient (fp32 C of the DM_TN products; LayerNorm partial rows, csrc/dm_rows.hip:140-141), biases, gamma / beta, the table.

The separate-node forms (LinearFn, AttentionFn, MlpFn behind CrossScaleAttention / Mlp with numerics="bf16") round at the same places:
`attention_branch` / `mlp_branch` are their sub-graphs, the module input cast (ops:1016 _as_operand in _CastFn, nets/ShfitScaleFormer.py
:135-144) standing where F2 stands in the block and the bf16 dx of the first product (ops:1034-1035) where B8 / B3 stand.
"""
import math

import torch
import torch.nn.functional as F

GRAD_NAMES = ("norm1.weight", "norm1.bias", "attn.relative_position_bias_table", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight",
              "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
EPS = 1e-5


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


class _RoundFwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return bf16_round(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return bf16_round(g)


class _GeluSavedImage(torch.autograd.Function):
    """GELU whose backward multiplies by the bf16 image of GELU'(pre) saved in the forward pass (F7), not by GELU' of the fp32 value."""

    @staticmethod
    def forward(ctx, pre):
        cdf = 0.5 * (1.0 + torch.erf(pre * math.sqrt(0.5)))
        pdf = torch.exp(-0.5 * pre * pre) / math.sqrt(2.0 * math.pi)
        ctx.save_for_backward(bf16_round(cdf + pre * pdf))
        return F.gelu(pre)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0]


def rf(t, points):
    return _RoundFwd.apply(t) if points else t


def rb(t, points):
    return _RoundBwd.apply(t) if points else t


def operand(t, points):
    """A value the kernels hold in bf16 and whose gradient they write in bf16 (F2 + B8 / B3; the module input of the separate nodes)."""
    return rb(rf(t, points), points)


def attention_branch(p, pre, y, heads, points):
    """proj(attention(qkv(y))) of nets/ShfitScaleFormer.py CrossScaleAttention / vit_model.Attention; y = operand(...) of its input.
    The gradient arriving at the result is rounded (B4: the operand copy of dx1; LinearFn: ops:1079)."""
    B, N, C = y.shape
    d = C // heads
    qkv = F.linear(y, rf(p[pre + "qkv.weight"], points), p[pre + "qkv.bias"])                 # F1
    qkv = rb(rf(qkv, points), points)                                                         # F3, B7
    qkv = qkv.reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    q = q * (d ** -0.5)                               # (the kernels scale the fp32 score instead; d = 64: a power of two, no rounding either way)
    attn = rb(q @ k.transpose(-2, -1), points)                                                # B6 (in front of the bias add: its gradient stays fp32)
    if pre + "relative_position_bias_table" in p:
        table, index = p[pre + "relative_position_bias_table"], p[pre + "relative_position_index"]
        attn = attn + table[index.reshape(-1)].reshape(N, N, -1).permute(2, 0, 1).contiguous().unsqueeze(0)
    attn = torch.softmax(attn, dim=-1)
    out = (rf(attn, points) @ v).transpose(1, 2).reshape(B, N, C)                             # F4
    out = rb(rf(out, points), points)                                                         # F5, B5
    return rb(F.linear(out, rf(p[pre + "proj.weight"], points), p[pre + "proj.bias"]), points)    # F1, B4


def mlp_branch(p, pre, y, points):
    """fc2(GELU(fc1(y))) of Mlp; y = operand(...) of its input.  The gradient arriving at the result is rounded (B1)."""
    a = rb(F.linear(y, rf(p[pre + "fc1.weight"], points), p[pre + "fc1.bias"]), points)       # F1, B2 (the fp32 accumulator goes into GELU)
    h = rf(_GeluSavedImage.apply(a) if points else F.gelu(a), points)                         # F6, F7
    return rb(F.linear(h, rf(p[pre + "fc2.weight"], points), p[pre + "fc2.bias"]), points)    # F1, B1


def block(p, x, heads, points, eps=EPS, pre=""):
    """x + attn(LN1(x)), then + mlp(LN2(.)): oracle.s2former.cross_scale_block (no table keys in p: the ViT block)."""
    C = x.shape[-1]
    y1 = operand(F.layer_norm(x, (C,), p[pre + "norm1.weight"], p[pre + "norm1.bias"], eps), points)      # F2, B8
    x = x + attention_branch(p, pre + "attn.", y1, heads, points)
    y2 = operand(F.layer_norm(x, (C,), p[pre + "norm2.weight"], p[pre + "norm2.bias"], eps), points)      # F2, B3
    return x + mlp_branch(p, pre + "mlp.", y2, points)


def attention_module(p, x, heads, points):
    """CrossScaleAttention.forward as separate nodes (keys without the "attn." prefix)."""
    return attention_branch(p, "", operand(x, points), heads, points)


def mlp_module(p, x, points):
    """Mlp.forward as a separate node (keys "fc1.*", "fc2.*")."""
    return mlp_branch(p, "", operand(x, points), points)


def two_blocks(p, x, heads, points, side=None, shared=False):
    """b2(b1(x)) with parameters under "b1." / "b2." (shared=True: b1 twice).  side = c: the middle activation also feeds (x_mid * c).sum();
    returns (y, that extra loss term)."""
    mid = block(p, x, heads, points, pre="b1.")
    y = block(p, mid, heads, points, pre="b1." if shared else "b2.")
    return y, (None if side is None else (mid * side).sum())


def evaluate(forward, params, x, go):
    """Run `forward(P, X)` (-> y or (y, extra loss term)) in fp64 on fresh leaves, loss = (y * go).sum() [+ extra]; returns
    {"y", "dx", "d_<key>" for every floating-point parameter that got a gradient} as detached fp64 tensors."""
    P = {k: (v.detach().double().requires_grad_(True) if v.is_floating_point() else v) for k, v in params.items()}
    X = x.detach().double().requires_grad_(True)
    out = forward(P, X)
    y, extra = out if isinstance(out, tuple) else (out, None)
    loss = (y * go.double()).sum()
    if extra is not None:
        loss = loss + extra
    loss.backward()
    res = {"y": y.detach(), "dx": X.grad}
    for k, v in P.items():
        if v.is_floating_point() and v.grad is not None:
            res["d_" + k] = v.grad
    return res


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    """|| a - b || / || b ||, in fp64."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


# ---- the cases of the GPU test: the smallest shapes that still reach each route -----------------------------------------------------------
# id -> (kind, C, heads, token cube or token count, B).  "s*" / "n*": CrossScaleBlock (table), "v*": vit_model.Block (no table).
# The two "b8" cases have B * heads >= 96, the batch rule of the persistent bf16 attention kernels (csrc/dm_attention.hip persistent_gate):
# below it a bf16 block never reaches the table-reading or the pipelined kernels the training step runs on.
CASES = {
    "s256": ("cross", 768, 12, (4, 8, 8), 2),
    "s192": ("cross", 768, 12, (3, 8, 8), 3),
    "s48": ("cross", 768, 12, (3, 4, 4), 2),
    "n256": ("cross", 256, 4, (4, 8, 8), 1),
    "v197": ("vit", 768, 12, 197, 3),
    "v50": ("vit", 192, 3, 50, 5),
    "s256b8": ("cross", 768, 12, (4, 8, 8), 8),
    "v197b8": ("vit", 768, 12, 197, 8),
}
SEEDS = {name: 1000 + i for i, name in enumerate(CASES)}


def case_tokens(name):
    t = CASES[name][3]
    return t if isinstance(t, int) else t[0] * t[1] * t[2]


def relpos_index(cube):
    """idx[i, j] = (zi-zj+S-1)(2H-1)(2W-1) + (yi-yj+H-1)(2W-1) + (xi-xj+W-1), tokens scale-major then row-major (oracle.s2former.relpos_index)."""
    S, H, W = cube
    t = torch.arange(S * H * W)
    z, y, x = t // (H * W), (t // W) % H, t % W
    d = lambda a, n: a[:, None] - a[None, :] + (n - 1)
    return d(z, S) * ((2 * H - 1) * (2 * W - 1)) + d(y, H) * (2 * W - 1) + d(x, W)


def block_params(C, heads, cube, gen, pre=""):
    """Random block parameters as fp32 tensors: weights ~ N(0, 1 / fan_in) and exactly representable in bf16 (the mode rounds them anyway),
    biases and beta ~ 0.1 N, gamma = 1 + 0.1 N, table ~ 0.5 N.  Keys are the modules' state_dict keys."""
    Hd = 4 * C
    n = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    p = {}
    p[pre + "norm1.weight"], p[pre + "norm1.bias"] = 1 + 0.1 * n(C), 0.1 * n(C)
    if cube is not None:
        S, H, W = cube
        p[pre + "attn.relative_position_bias_table"] = 0.5 * n((2 * S - 1) * (2 * H - 1) * (2 * W - 1), heads)
        p[pre + "attn.relative_position_index"] = relpos_index(cube)
    p[pre + "attn.qkv.weight"], p[pre + "attn.qkv.bias"] = bf16_round(n(3 * C, C) / math.sqrt(C)), 0.1 * n(3 * C)
    p[pre + "attn.proj.weight"], p[pre + "attn.proj.bias"] = bf16_round(n(C, C) / math.sqrt(C)), 0.1 * n(C)
    p[pre + "norm2.weight"], p[pre + "norm2.bias"] = 1 + 0.1 * n(C), 0.1 * n(C)
    p[pre + "mlp.fc1.weight"], p[pre + "mlp.fc1.bias"] = bf16_round(n(Hd, C) / math.sqrt(C)), 0.1 * n(Hd)
    p[pre + "mlp.fc2.weight"], p[pre + "mlp.fc2.bias"] = bf16_round(n(C, Hd) / math.sqrt(Hd)), 0.1 * n(C)
    return p


def case_data(name, blocks=("",)):
    """(params, x, go) of a case: one parameter set per prefix in `blocks`, x and the output gradient ~ N(0, 1), all from the case's seed."""
    kind, C, heads, tok, B = CASES[name]
    gen = torch.Generator().manual_seed(SEEDS[name])
    cube = tok if kind == "cross" else None
    p = {}
    for pre in blocks:
        p.update(block_params(C, heads, cube, gen, pre))
    N = case_tokens(name)
    x = torch.randn(B, N, C, generator=gen, dtype=torch.float32)
    go = torch.randn(B, N, C, generator=gen, dtype=torch.float32)
    return p, x, go


def strip(p, pre):
    """The parameters under prefix `pre`, without it."""
    return {k[len(pre):]: v for k, v in p.items() if k.startswith(pre)}
