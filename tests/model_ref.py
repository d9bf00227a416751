"""fp64 restatement of the ShfitScaleFormer_v3 training step (pair forward + Loss(1.0, 0.1, 0) + backward) with the bf16 mode's rounding
points -- plain CPU torch + autograd, built on tests/block_ref.py.

Two switches of ONE graph, as in block_ref:
  * truth  (points=False): fp64 throughout.  The op sequence is oracle.s2former.forward_pair's followed by oracle.losses.contrastive_loss,
    so on the same parameters the two agree to rounding (tests/test_model_ref_host.py);
  * points (points=True): the same graph with `rf` / `rb` identity nodes where the model rounds in "bf16" mode.  The blocks are
    block_ref.block(p, x, heads, points, pre=...), unchanged; this file adds what rounds AROUND them.
The distance of the points run to truth is the yardstick of tests/test_gpu_model_oracle.py.

Where each point outside the block comes from (deepmerge_amd/ops.py = ops, deepmerge_amd/nets/ShfitScaleFormer.py = nets,
deepmerge_amd/csrc/... = csrc); DESIGN.md "Numerics contract of the fused block in bf16 mode" has the same list as rows M1 - M3.

  M1 the patch embeds' operand rows      nets:99 ops.patchify(x.float(), patch, act_dtype) -> ops:762-763 bf16 rows: csrc/dm_rows.hip:625
                                         dm_store4 of the fp32 pixels into bf16_t cols
  M2 the patch embeds' weights           ops:1333 lp_weight in PatchEmbedCatFn.forward -> ops:1780 cast (csrc/dm_rows.hip:528 cast_bf16_kernel)
                                         or the trainer's mirror (ops:1777-1779).  C (the token cube) and the bias stay fp32: ops:1327, ops:1335
  M3 the gradient rows of the token cube ops:1355 the `_dm_lp_regrouped` rider block 0's LayerNorm backward wrote (ops:1991-1998,
                                         csrc/dm_rows.hip:302 dm_store4 of the fp32 dx into bf16 rows) or ops:1359 the strided cast-copy;
                                         feeds dW = dy^T cols and db = the column sums of the COPY (ops:1365 -> ops:1275-1276)
  no point:
     the stage transitions               ops:1586-1587 pooled rows and y in fp32 (PoolNormFn.forward); ops:1546 / ops:1571 the separate
                                         TokenPoolFn + LayerNormFn(..., torch.float32); dgamma / dbeta from fp32 partial rows (ops:1610-1617)
     the final norm, the designed norm   nets:320-321 _ln: out_dtype torch.float32
     the per-scale token mean            ops:1630 GroupMeanFn: fp32 in, fp32 out
     FeatureEmbed                        nets:162-164 x.float() rows: MlpFn / LinearFn cast their weights to x.dtype = fp32 (ops:1382-1383,
                                         ops:1295 -> ops:1775-1776)
     the final Linear                    nets:355 LinearFn on the fp32 rows of torch.cat: lp_weight(..., fp32) is the master (ops:1775-1776),
                                         its backward's operand is the fp32 dy (ops:1309 -> ops:1195-1196)
     the loss                            ops:1652-1655 / ops:1714-1717 dm_contrastive_loss on fp32 rows
  the block's own B1, not a second rounding:
     the bf16 copies of dx that a stage transition (ops:1607, ops:1619; csrc/dm_rows.hip:271) and the final norm (nets:347 grad_lp ->
     ops:1423, ops:1432-1433; csrc/dm_rows.hip:302) leave on the gradient are what the block below takes as the operand copy of its
     incoming gradient (ops:1957-1959): block_ref's `rb` at the result of mlp_branch.  The fp32 dx itself goes on as the residual gradient.

The shared `norm.weight` / `norm.bias` enter the graph as four leaf copies, one per writer (WRITERS); `d_norm.*` is their sum and
`parts` keeps each writer's share.  Under the contrastive loss the output gradients of the two sides of a pair are equal and opposite,
so everything the pair's output depends on through a term that is the SAME for both sides has an exactly zero gradient: the bias of
the final Linear, and the shares of `norm.bias` that come from the final norm and from the designed-feature norm (beta passes
linearly through the token mean and the Linear).  ZERO_BY_SYMMETRY names them; `cancel_scale` gives the size of what cancels.
"""
import time

import torch
import torch.nn.functional as F

import block_ref as R
from oracle import losses as OL
from oracle import s2former as O
from util import MODEL_CASES, model_inputs, model_params

WRITERS = ("pool0", "pool1", "final", "designed")      # the two stage transitions, the final norm, the designed-feature norm
NO_GRAD = ("final_features.bias", "final_features.weight", "head.bias", "head.weight")       # the fixtures' grad_none
MARGIN = 1.0
# tensors (and writer shares) that are zero in exact arithmetic, see the header
ZERO_BY_SYMMETRY = ("d_final_features_with_design.bias",)
ZERO_SHARES = (("norm.bias", "final"), ("norm.bias", "designed"))

# id -> (config, tag of the recipe inputs, pairs drawn, pairs used)
CASES = {
    "m3b4": (MODEL_CASES["v3_3s3c_111"], "v3_3s3c_111", 4, 4),
    "m4b4": (O.S2Config(scales=(32, 64, 128, 256), in_c=4, depth=(2, 1, 1)), "m4b4", 4, 4),
    "m3b2": (MODEL_CASES["v3_3s3c_111"], "v3_3s3c_111", 4, 2),      # pairs 0 (flag 1) and 1 (flag 0, inside the margin) of m3b4
}


def case_data(name):
    """(cfg, params, (left, ld, right, rd, flag)): the recipe's weights by state_dict key and its inputs, fp32."""
    cfg, tag, drawn, used = CASES[name]
    p = model_params(cfg, requires_grad=False)
    left, ld, right, rd, flag = model_inputs(tag, cfg.scales, cfg.in_c, drawn)
    cut = lambda t: t[:used].contiguous()
    return cfg, p, ([cut(t) for t in left], cut(ld), [cut(t) for t in right], cut(rd), cut(flag))


def _norm(p, writer, x, cfg):
    return F.layer_norm(x, (cfg.dim,), p["norm.weight@" + writer], p["norm.bias@" + writer], cfg.ln_eps)


def forward_once(p, patches, designed, cfg, points):
    """oracle.s2former.forward_once with the designed-feature branch; p holds `norm.*@<writer>` for the four uses of the shared norm."""
    ys = []
    for i in range(cfg.n_scales):
        pre = f"patch_embed_blocks.{i}.proj."
        y = F.conv2d(R.rf(patches[i], points), R.rf(p[pre + "weight"], points), p[pre + "bias"], stride=cfg.patch_size(i))    # M1, M2
        ys.append(y.flatten(2).transpose(1, 2))
    x = R.rb(torch.cat(ys, dim=1), points)                                                                                   # M3
    for stage in range(3):
        for j in range(cfg.depth[stage]):
            x = R.block(p, x, cfg.heads, points, cfg.ln_eps, pre=f"blocks{stage}.{j}.")
        if stage < 2:
            x = _norm(p, f"pool{stage}", O.token_pool2x2(x, cfg.n_scales, cfg.grid >> stage), cfg)
    x = _norm(p, "final", x, cfg)
    B = x.shape[0]
    x = x.reshape(B, cfg.n_scales, -1, cfg.dim).mean(dim=2).reshape(B, cfg.n_scales * cfg.dim)
    f = _norm(p, "designed", O.feature_embed(p, "feature_embed.", designed).squeeze(1), cfg)
    return F.linear(torch.cat((x, f), dim=1), p["final_features_with_design.weight"], p["final_features_with_design.bias"])


def evaluate(cfg, params, inputs, points):
    """One training step in fp64 on fresh leaves.  Returns (res, parts, cancel_scale):
    res   {"out_a", "out_b", "loss", "d_<name>" for every parameter of net.named_parameters() that gets a gradient};
    parts {"norm.weight" / "norm.bias": {writer: that writer's share of the gradient}};
    cancel_scale {name in ZERO_BY_SYMMETRY: || sum of |contributions| ||, the size of the terms that cancel to zero}."""
    left, ld, right, rd, flag = inputs
    P = {}
    for k, v in params.items():
        if not v.is_floating_point():
            P[k] = v
        elif k in ("norm.weight", "norm.bias"):
            for w in WRITERS:
                P[k + "@" + w] = v.detach().double().requires_grad_(True)
        else:
            P[k] = v.detach().double().requires_grad_(True)
    dd = lambda t: t.detach().double()
    # both sides as ONE batch [left; right], as the model runs them (no op mixes samples: the same values as two passes)
    both = [torch.cat((dd(l), dd(r)), 0) for l, r in zip(left, right)]
    f = forward_once(P, both, torch.cat((dd(ld), dd(rd)), 0), cfg, points)
    f.retain_grad()
    n = flag.shape[0]
    fa, fb = f[:n], f[n:]
    loss = OL.contrastive_loss(fa, fb, flag, MARGIN)
    loss.backward()
    res = {"out_a": fa.detach(), "out_b": fb.detach(), "loss": loss.detach()}
    parts = {}
    for k in ("norm.weight", "norm.bias"):
        parts[k] = {w: P[k + "@" + w].grad for w in WRITERS}
        res["d_" + k] = sum(parts[k][w] for w in WRITERS)
    none = []
    for k, v in P.items():
        if "@" in k or not v.is_floating_point():
            continue
        if v.grad is None:
            none.append(k)
        else:
            res["d_" + k] = v.grad
    assert sorted(none) == sorted(NO_GRAD), none
    cancel_scale = {"d_final_features_with_design.bias": float(f.grad.abs().sum(0).norm())}
    return res, parts, cancel_scale


def rel_err(got, truth, scale=None):
    """|| got - truth || / || truth ||, in fp64; `scale` replaces the denominator for a tensor whose truth is zero by symmetry."""
    got, truth = got.detach().double().cpu(), truth.detach().double().cpu()
    return float((got - truth).norm() / (truth.norm() if scale is None else scale))


_ref = {}


def reference(name):
    """Truth and points runs of a case, computed once per process and shared: a dict with cfg, params, inputs, truth, parts, scale
    (cancel_scale of the truth run), yard {tensor: distance of the points run to truth} and seconds (host time of the two runs)."""
    if name not in _ref:
        cfg, p, inputs = case_data(name)
        t0 = time.perf_counter()
        truth, parts, scale = evaluate(cfg, p, inputs, False)
        pts, _, _ = evaluate(cfg, p, inputs, True)
        dt = time.perf_counter() - t0
        yard = {k: rel_err(pts[k], truth[k], scale.get(k)) for k in truth}
        _ref[name] = dict(cfg=cfg, params=p, inputs=inputs, truth=truth, parts=parts, scale=scale, yard=yard, seconds=dt)
    return _ref[name]


def gate(yard):
    """The bf16 bound of one tensor: twice what the mode's own roundings cost it, and never below the fp32 parity gate."""
    return max(2.0 * yard, 1e-3)
