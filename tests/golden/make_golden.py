#!/usr/bin/env python3
"""Generate the committed golden vectors by running the UNMODIFIED reference modules on CPU.

Run in the build container only (needs /root/reference; the GPU box never sees it):

    python tests/golden/make_golden.py            # writes tests/golden/*.npz

What is imported from the reference: `vit_model`, `Losses`, `nets.ShfitScaleFormer`
(nets/ShfitScaleFormer.py:9 imports two symbols from `timm`, which is not installed; as
SURVEY.md section 8c records, an in-process module object provides
`trunc_normal_ = torch.nn.init.trunc_normal_` and `DropPath = vit_model.DropPath` -- both only
touch initialisation / a never-instantiated identity, and every weight used in a fixture is
overwritten by tests/golden/recipe.py anyway).

Fixtures hold data only: seeds/recipes for inputs and weights, and the reference's outputs,
losses, gradients and post-Adam weights (as compact summaries, see recipe.summarize).
No reference source text is stored.
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import recipe  # noqa: E402

REF = os.environ.get("DEEPMERGE_REFERENCE", "/root/reference")


def import_reference():
    sys.path.insert(0, REF)
    import vit_model  # noqa
    layers = types.ModuleType("timm.models.layers")
    layers.trunc_normal_ = torch.nn.init.trunc_normal_
    layers.DropPath = vit_model.DropPath
    for name, mod in (("timm", types.ModuleType("timm")), ("timm.models", types.ModuleType("timm.models")),
                      ("timm.models.layers", layers)):
        sys.modules[name] = mod
    from nets import ShfitScaleFormer as S2F  # noqa
    import Losses  # noqa
    return S2F, vit_model, Losses


def load_det_weights(module: torch.nn.Module, prefix: str = ""):
    """Overwrite every float tensor of module.state_dict() with the name-keyed recipe."""
    sd = module.state_dict()
    new = {}
    for k, v in sd.items():
        if v.dtype.is_floating_point:
            new[k] = torch.from_numpy(recipe.det_weight(prefix + k, v.shape))
        else:
            new[k] = v
    module.load_state_dict(new, strict=True)


def t(name, shape, kind="normal"):
    return torch.from_numpy(recipe.det_input(name, shape, kind))


def add(fx, name, tensor, k=2048):
    fx.update(recipe.summarize(name, tensor.detach().cpu().numpy(), k))


# ------------------------------------------------------------------------------------------
def gen_relpos(S2F):
    fx = {}
    for cube in ([2, 2, 2], [3, 8, 8], [3, 4, 4], [3, 2, 2], [4, 8, 8], [4, 4, 4], [4, 2, 2], [1, 3, 5]):
        attn = S2F.CrossScaleAttention(dim=768, num_heads=12, cube_size=list(cube), qkv_bias=True)
        idx = attn.relative_position_index.numpy()
        assert idx.dtype == np.int64
        key = "x".join(map(str, cube))
        fx["index/" + key] = idx.astype(np.int32)
        fx["table_rows/" + key] = np.int64(attn.relative_position_bias_table.shape[0])
    np.savez_compressed(os.path.join(HERE, "relpos_index.npz"), **fx)
    print("relpos_index.npz", len(fx))


def gen_ops(S2F, Losses):
    fx = {}
    # ---- PatchEmbed -----------------------------------------------------------------
    for tag, img, patch, in_c in (("pe32", 32, 4, 3), ("pe64", 64, 8, 3), ("pe128", 128, 16, 3), ("pe256c4", 256, 32, 4)):
        m = S2F.PatchEmbed(img_size=img, patch_size=patch, in_c=in_c, out_c=768)
        load_det_weights(m, tag + ".")
        x = t(tag + ".x", (2, in_c, img, img), "unit").requires_grad_(True)
        y = m(x)
        go = t(tag + ".go", y.shape)
        (y * go).sum().backward()
        add(fx, tag + "/y", y)
        add(fx, tag + "/dx", x.grad)
        add(fx, tag + "/dw", m.proj.weight.grad)
        add(fx, tag + "/db", m.proj.bias.grad)
    # ---- Mlp ------------------------------------------------------------------------
    m = S2F.Mlp(in_features=768, hidden_features=3072)
    load_det_weights(m, "mlp.")
    x = t("mlp.x", (2, 12, 768)).requires_grad_(True)
    y = m(x)
    (y * t("mlp.go", y.shape)).sum().backward()
    add(fx, "mlp/y", y); add(fx, "mlp/dx", x.grad)
    for n, p in m.named_parameters():
        add(fx, "mlp/d_" + n, p.grad)
    # config-1 style 2-linear block on 128-d pair features
    m = S2F.Mlp(in_features=128, hidden_features=128, out_features=128)
    load_det_weights(m, "mlp128.")
    x = t("mlp128.x", (64, 128)).requires_grad_(True)
    y = m(x)
    (y * t("mlp128.go", y.shape)).sum().backward()
    add(fx, "mlp128/y", y); add(fx, "mlp128/dx", x.grad)
    for n, p in m.named_parameters():
        add(fx, "mlp128/d_" + n, p.grad)
    # ---- FeatureEmbed ---------------------------------------------------------------
    m = S2F.FeatureEmbed(feature_size=19, embed_dim=768)
    load_det_weights(m, "fe.")
    x = t("fe.x", (3, 1, 19), "designed").requires_grad_(True)
    y = m(x)
    (y * t("fe.go", y.shape)).sum().backward()
    add(fx, "fe/y", y); add(fx, "fe/dx", x.grad)
    for n, p in m.named_parameters():
        add(fx, "fe/d_" + n, p.grad)
    # ---- CrossScaleAttention / CrossScaleBlock ----------------------------------------
    for cube in ([3, 2, 2], [3, 4, 4], [3, 8, 8], [4, 8, 8], [4, 4, 4], [4, 2, 2]):
        tag = "attn" + "x".join(map(str, cube))
        n = cube[0] * cube[1] * cube[2]
        m = S2F.CrossScaleAttention(dim=768, num_heads=12, cube_size=list(cube), qkv_bias=True)
        load_det_weights(m, tag + ".")
        x = t(tag + ".x", (2, n, 768)).requires_grad_(True)
        y = m(x)
        (y * t(tag + ".go", y.shape)).sum().backward()
        add(fx, tag + "/y", y); add(fx, tag + "/dx", x.grad)
        for pn, p in m.named_parameters():
            add(fx, tag + "/d_" + pn, p.grad)
    for cube in ([3, 4, 4], [4, 8, 8]):
        tag = "block" + "x".join(map(str, cube))
        n = cube[0] * cube[1] * cube[2]
        m = S2F.CrossScaleBlock(dim=768, num_heads=12, cube_size=list(cube))
        load_det_weights(m, tag + ".")
        x = t(tag + ".x", (2, n, 768)).requires_grad_(True)
        y = m(x)
        (y * t(tag + ".go", y.shape)).sum().backward()
        add(fx, tag + "/y", y); add(fx, tag + "/dx", x.grad)
        for pn, p in m.named_parameters():
            add(fx, tag + "/d_" + pn, p.grad)
    # ---- Loss -----------------------------------------------------------------------
    crit = Losses.Loss(margin=1.0, lamda=0.1, belta=0)
    a = t("loss.a", (16, 100)) * 0.2
    b = a + t("loss.b", (16, 100)) * np.linspace(0.01, 0.25, 16, dtype=np.float32)[:, None]  # d from << 1 to >> 1
    flag_i = torch.tensor([1, 0] * 8, dtype=torch.int64)
    for tag, flag in (("loss_i64", flag_i), ("loss_f32", flag_i.to(torch.float32))):
        aa = a.clone().requires_grad_(True); bb = b.clone().requires_grad_(True)
        val = crit(aa, bb, flag)
        val.backward()
        fx[tag + "/value"] = np.float64(val.item())
        add(fx, tag + "/da", aa.grad); add(fx, tag + "/db", bb.grad)
    d = (a - b).pow(2).sum(1)
    fx["loss/n_below_margin"] = np.int64((d < 1.0).sum().item())
    fx["loss/n_above_margin"] = np.int64((d > 1.0).sum().item())
    fx["loss/a"] = a.numpy(); fx["loss/b"] = b.numpy(); fx["loss/flag"] = flag_i.numpy()
    # MultiLoss / ClassLoss
    ll = t("loss.ll", (16, 11)); rl = t("loss.rl", (16, 11))
    lt = torch.arange(16) % 11; rt = (torch.arange(16) * 3) % 11
    fx["multiloss/value"] = np.float64(Losses.MultiLoss(1.0, 0.1, 0)(a, b, flag_i, ll, lt, rl, rt).item())
    fx["classloss/value"] = np.float64(Losses.ClassLoss(1.0, 0.1, 0)(ll, lt, rl, rt).item())
    np.savez_compressed(os.path.join(HERE, "ops_s2former.npz"), **fx)
    print("ops_s2former.npz", len(fx))


def model_inputs(tag, scales, in_c, B=4):
    """Pair batch of 4: (unrelated, flag 1), (near-identical, flag 0: hinge branch d < margin
    live, SURVEY 8a L1 note), (near-identical, flag 1), (unrelated, flag 0: hinge dead)."""
    assert B == 4
    left = [t(f"{tag}.left{i}", (B, in_c, s, s), "unit") for i, s in enumerate(scales)]
    right = [t(f"{tag}.right{i}", (B, in_c, s, s), "unit") for i, s in enumerate(scales)]
    ld = t(tag + ".ld", (B, 1, 19), "designed")
    rd = t(tag + ".rd", (B, 1, 19), "designed")
    eps = 0.2
    for i in range(len(scales)):
        for b in (1, 2):
            right[i][b] = left[i][b] * (1 - eps) + eps * right[i][b]
    for b in (1, 2):
        rd[b] = ld[b] * (1 + eps)
    flag = torch.tensor([1, 0, 1, 0], dtype=torch.int64)
    return left, ld, right, rd, flag


def gen_model(S2F, Losses):
    fx = {}
    for tag, scales, in_c, depth in (("v3_3s3c_642", [32, 64, 128], 3, [6, 4, 2]),
                                     ("v3_4s4c_321", [32, 64, 128, 256], 4, [3, 2, 1]),
                                     ("v3_3s3c_111", [32, 64, 128], 3, [1, 1, 1]),
                                     ("v3_4s4c_642", [32, 64, 128, 256], 4, [6, 4, 2])):      # BASELINE configs[4]'s model
        PE = S2F.PatchEmbed if in_c == 3 else (
            lambda img_size, patch_size, in_c, out_c, _c=in_c: S2F.PatchEmbed(img_size=img_size, patch_size=patch_size, in_c=_c, out_c=out_c))
        net = S2F.ShfitScaleFormer_v3(is_designed_feature_embedding=True, PatchEmbed=PE, cube_size=[8, 8],
                                      input_image_scales=list(scales), embed_dim=768, depth=list(depth))
        load_det_weights(net, "")
        sd = net.state_dict()
        fx[tag + "/manifest_keys"] = np.array(list(sd.keys()))
        fx[tag + "/manifest_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        fx[tag + "/manifest_dtypes"] = np.array([str(v.dtype).replace("torch.", "") for v in sd.values()])
        fx[tag + "/name"] = np.array(net.name)
        fx[tag + "/n_params"] = np.int64(sum(p.numel() for p in net.parameters()))
        left, ld, right, rd, flag = model_inputs(tag, scales, in_c, 4)
        crit = Losses.Loss(margin=1.0, lamda=0.1, belta=0)
        net.train()
        opt = torch.optim.Adam(filter(lambda p: p.requires_grad, net.parameters()), lr=1e-4)
        watch = ["blocks0.0.attn.qkv.weight", "blocks2.0.mlp.fc2.bias", "norm.weight",
                 "blocks1.0.attn.relative_position_bias_table", "patch_embed_blocks.0.proj.weight",
                 "final_features_with_design.weight", "feature_embed.proj0.weight"]
        named = dict(net.named_parameters())
        for step in range(1, 4):
            out_a, out_b = net(left, ld, right, rd)
            loss = crit(out_a, out_b, flag)
            opt.zero_grad()
            loss.backward()
            if step == 1:
                add(fx, tag + "/out_a", out_a); add(fx, tag + "/out_b", out_b)
                fx[tag + "/loss"] = np.float64(loss.item())
                fx[tag + "/dist"] = (out_a - out_b).pow(2).sum(1).detach().numpy().astype(np.float64)
                none = []
                for n, p in named.items():
                    if p.grad is None:
                        none.append(n)
                    else:
                        add(fx, tag + "/grad/" + n, p.grad, k=1024)
                fx[tag + "/grad_none"] = np.array(none)
                net.eval()
                ev = net(left, ld)
                net.train()
                fx[tag + "/eval_equals_train"] = np.bool_(torch.equal(ev, out_a))
            opt.step()
            fx[tag + f"/loss_step{step}"] = np.float64(loss.item())
            if step in (1, 3):
                for n in watch:
                    add(fx, tag + f"/adam{step}/" + n, named[n], k=1024)
        print(tag, "loss", fx[tag + "/loss"], "dist", fx[tag + "/dist"], "none", list(fx[tag + "/grad_none"]))
    # (the values after three Adam steps move by ~3e-5 relative from run to run: CPU reductions are thread-order dependent.
    # Keys already committed keep their committed values, so re-running this script only ADDS cases.)
    path = os.path.join(HERE, "model_v3.npz")
    if os.path.exists(path):
        old = np.load(path)
        fx.update({k: old[k] for k in old.files})
    np.savez_compressed(path, **fx)
    print("model_v3.npz", len(fx))


def gen_model_f64(S2F, Losses):
    """gen_model's three Adam steps with the reference modules, weights and inputs in float64 (model_v3_f64.npz, keys `<tag>/f64/...`).  In fp32 the
    post-Adam values depend on the host's CPU code paths (noise-level gradients move their entries by O(lr)); in float64 they do not."""
    fx = {}
    for tag, scales, in_c, depth in (("v3_3s3c_642", [32, 64, 128], 3, [6, 4, 2]),
                                     ("v3_4s4c_321", [32, 64, 128, 256], 4, [3, 2, 1]),
                                     ("v3_3s3c_111", [32, 64, 128], 3, [1, 1, 1]),
                                     ("v3_4s4c_642", [32, 64, 128, 256], 4, [6, 4, 2])):
        PE = S2F.PatchEmbed if in_c == 3 else (
            lambda img_size, patch_size, in_c, out_c, _c=in_c: S2F.PatchEmbed(img_size=img_size, patch_size=patch_size, in_c=_c, out_c=out_c))
        net = S2F.ShfitScaleFormer_v3(is_designed_feature_embedding=True, PatchEmbed=PE, cube_size=[8, 8],
                                      input_image_scales=list(scales), embed_dim=768, depth=list(depth))
        load_det_weights(net, "")
        net.double().train()
        left, ld, right, rd, flag = model_inputs(tag, scales, in_c, 4)
        left, ld, right, rd = [x.double() for x in left], ld.double(), [x.double() for x in right], rd.double()
        crit = Losses.Loss(margin=1.0, lamda=0.1, belta=0)
        opt = torch.optim.Adam(filter(lambda p: p.requires_grad, net.parameters()), lr=1e-4)
        watch = [k[len(tag + "/adam1/"):-len("/shape")] for k in np.load(os.path.join(HERE, "model_v3.npz")).files
                 if k.startswith(tag + "/adam1/") and k.endswith("/shape")]
        named = dict(net.named_parameters())
        for step in range(1, 4):
            out_a, out_b = net(left, ld, right, rd)
            loss = crit(out_a, out_b, flag)
            opt.zero_grad()
            loss.backward()
            opt.step()
            fx[tag + f"/f64/loss_step{step}"] = np.float64(loss.item())
            if step in (1, 3):
                for n in watch:
                    add(fx, tag + f"/f64/adam{step}/" + n, named[n], k=1024)
        print(tag, "f64 losses", [fx[tag + f"/f64/loss_step{s}"] for s in (1, 2, 3)])
    np.savez_compressed(os.path.join(HERE, "model_v3_f64.npz"), **fx)      # (host-independent: regenerated whole)
    print("model_v3_f64.npz", len(fx))


def gen_variants(S2F, Losses):
    """Single-stage variants v1 / v2 (cube [4,7,7], N = 196) and the designed-features-only v6."""
    fx = {}
    crit = Losses.Loss(margin=1.0, lamda=0.1, belta=0)
    scales = [28, 56, 112, 224]
    for tag, ctor, kw in (("v1_d2", S2F.ShfitScaleFormer, dict(depth=2)), ("v2", S2F.ShfitScaleFormer_v2, {})):
        net = ctor(is_designed_feature_embedding=True, cube_size=[7, 7], input_image_scales=list(scales), **kw)
        load_det_weights(net, "")
        sd = net.state_dict()
        fx[tag + "/manifest_keys"] = np.array(list(sd.keys()))
        fx[tag + "/manifest_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        fx[tag + "/n_params"] = np.int64(sum(p.numel() for p in net.parameters()))
        left, ld, right, rd, flag = model_inputs(tag, scales, 3, 4)
        net.train()
        fa, fb = net(left, ld, right, rd)
        loss = crit(fa, fb, flag)
        loss.backward()
        add(fx, tag + "/out_a", fa); add(fx, tag + "/out_b", fb)
        fx[tag + "/loss"] = np.float64(loss.item())
        none = []
        for n, p in net.named_parameters():
            if p.grad is None:
                none.append(n)
            else:
                add(fx, tag + "/grad/" + n, p.grad, k=512)
        fx[tag + "/grad_none"] = np.array(none)
        net.eval()
        with torch.no_grad():
            single = net(left, ld)
        fx[tag + "/single_equals_left"] = np.bool_(torch.equal(single, fa))
        print(tag, "loss", fx[tag + "/loss"], "params", int(fx[tag + "/n_params"]), "none", none)
    net = S2F.ShfitScaleFormer_v6()
    load_det_weights(net, "")
    fx["v6/manifest_keys"] = np.array(list(net.state_dict().keys()))
    da = t("v6.da", (4, 1, 19), "designed"); db = t("v6.db", (4, 1, 19), "designed")
    db[1] = da[1] * 1.05
    flag = torch.tensor([1, 0, 1, 0], dtype=torch.int64)
    fa, fb = net(None, da, None, db)
    loss = crit(fa, fb, flag)
    loss.backward()
    add(fx, "v6/out_a", fa); add(fx, "v6/out_b", fb)
    fx["v6/loss"] = np.float64(loss.item())
    for n, p in net.named_parameters():
        if p.grad is not None:
            add(fx, "v6/grad/" + n, p.grad, k=512)
    np.savez_compressed(os.path.join(HERE, "model_variants.npz"), **fx)
    print("model_variants.npz", len(fx))


def gen_aux(S2F, Losses):
    """v4 (aux heads) and v5 (designed-feature token + extended bias table), SURVEY 8a M14 / M15.  Dropout2d in the aux
    heads is set to p = 0 on the instance (its RNG stream is not reproducible by an independent implementation); everything
    else, including BatchNorm2d batch statistics and running-statistic updates, is pinned."""
    fx = {}
    crit = Losses.Loss(margin=1.0, lamda=0.1, belta=0)
    scales = [32, 64, 128]
    for tag, ctor, kw in (("v4_111", S2F.ShfitScaleFormer_v4, dict(is_designed_feature_embedding=True)),
                          ("v5_111", S2F.ShfitScaleFormer_v5, {})):
        net = ctor(cube_size=[8, 8], input_image_scales=list(scales), depth=[1, 1, 1], **kw)
        load_det_weights(net, "")
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout2d):
                m.p = 0.0
        sd = net.state_dict()
        fx[tag + "/manifest_keys"] = np.array(list(sd.keys()))
        fx[tag + "/manifest_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        fx[tag + "/manifest_dtypes"] = np.array([str(v.dtype).replace("torch.", "") for v in sd.values()])
        if hasattr(net, "name"):
            fx[tag + "/name"] = np.array(net.name)
        fx[tag + "/n_params"] = np.int64(sum(p.numel() for p in net.parameters()))
        for k, v in sd.items():
            if k.endswith("relative_position_index"):
                fx[tag + "/index/" + k] = v.numpy().astype(np.int64)
        left, ld, right, rd, flag = model_inputs(tag, scales, 3, 4)
        net.train()
        (xa, a0a, a1a), (xb, a0b, a1b) = net(left, ld, right, rd)
        loss = crit(xa, xb, flag) + 0.1 * crit(a0a, a0b, flag) + 0.2 * crit(a1a, a1b, flag)
        loss.backward()
        for n_, v in (("out_a", xa), ("out_b", xb), ("aux0_a", a0a), ("aux0_b", a0b), ("aux1_a", a1a), ("aux1_b", a1b)):
            add(fx, f"{tag}/{n_}", v)
        fx[tag + "/loss"] = np.float64(loss.item())
        none = []
        for n, p in net.named_parameters():
            if p.grad is None:
                none.append(n)
            else:
                add(fx, tag + "/grad/" + n, p.grad, k=512)
        fx[tag + "/grad_none"] = np.array(none)
        for k, v in net.state_dict().items():
            if "running_" in k:
                add(fx, tag + "/after/" + k, v, k=768)
            if k.endswith("num_batches_tracked"):
                fx[tag + "/after/" + k] = np.int64(v.item())
        net.eval()
        with torch.no_grad():
            ev = net(left, ld)
        add(fx, tag + "/eval_out", ev)
        print(tag, "loss", fx[tag + "/loss"], "params", int(fx[tag + "/n_params"]), "none", none)
    np.savez_compressed(os.path.join(HERE, "model_aux.npz"), **fx)
    print("model_aux.npz", len(fx))


def gen_vit(vit_model, Losses):
    """vit_model.py pair encoders (BASELINE configs[2])."""
    fx = {}
    path = os.path.join(HERE, "model_vit.npz")
    old = np.load(path) if os.path.exists(path) else None       # cases already committed are kept as they are (only ADD)
    have = (lambda tag: old is not None and tag + "/loss" in old.files)
    crit = Losses.Loss(margin=1.0, lamda=0.1, belta=0)
    flag = torch.tensor([1, 0], dtype=torch.int64)
    # ---- VisionTransformer ViT-B/16 (num_classes=100, has_logits=False), depth 12 and a 2-block cut;
    #      ViT-H/14 geometry (vit_model.py:649-662: dim 1280, 16 heads of 80, 14-pixel patches, 257 tokens), 2 blocks ----
    for tag, depth in (("vitb16_d12", 12), ("vitb16_d2", 2), ("vith14_d2", 2)):
        if have(tag):
            continue
        if tag == "vith14_d2":
            net = vit_model.VisionTransformer(img_size=224, patch_size=14, embed_dim=1280, depth=depth, num_heads=16,
                                              representation_size=None, num_classes=100)
        elif depth == 12:
            net = vit_model.vit_base_patch16_224_in21k(num_classes=100, has_logits=False)
        else:
            net = vit_model.VisionTransformer(img_size=224, patch_size=16, embed_dim=768, depth=depth, num_heads=12,
                                              representation_size=None, num_classes=100)
        load_det_weights(net, "")
        sd = net.state_dict()
        fx[tag + "/manifest_keys"] = np.array(list(sd.keys()))
        fx[tag + "/manifest_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        fx[tag + "/n_params"] = np.int64(sum(p.numel() for p in net.parameters()))
        x1 = t(tag + ".x1", (2, 3, 224, 224), "unit"); x2 = t(tag + ".x2", (2, 3, 224, 224), "unit")
        x2[1] = x1[1] * 0.8 + 0.2 * x2[1]
        net.train()
        ya, yb = net(x1, x2)
        loss = crit(ya, yb, flag)
        loss.backward()
        add(fx, tag + "/out_a", ya); add(fx, tag + "/out_b", yb)
        fx[tag + "/loss"] = np.float64(loss.item())
        fx[tag + "/dist"] = (ya - yb).pow(2).sum(1).detach().numpy().astype(np.float64)
        for n, p in net.named_parameters():
            assert p.grad is not None, n
            add(fx, tag + "/grad/" + n, p.grad, k=512)
        one = net(x1)
        fx[tag + "/single_equals_pair"] = np.bool_(torch.equal(one, ya))
        try:
            net(x1, x1, x1, x1)
            fx[tag + "/four_args_raise"] = np.bool_(False)
        except ValueError:
            fx[tag + "/four_args_raise"] = np.bool_(True)
        print(tag, "loss", fx[tag + "/loss"], "dist", fx[tag + "/dist"], "params", int(fx[tag + "/n_params"]))
    # ---- ScaleEmbedTransformer (multi-scale + designed-feature token) --------------------------------
    for tag, depth in (("vitscale_d12", 12), ("vitscale_d2", 2)):
        if have(tag):
            continue
        if depth == 12:
            net = vit_model.vit_base_patch_scales_224_in21k(num_classes=512, has_logits=False)
        else:
            net = vit_model.ScaleEmbedTransformer(img_size=224, patch_size=16, embed_dim=768, depth=depth, num_heads=12,
                                                  representation_size=None, num_classes=512)
        load_det_weights(net, "")
        sd = net.state_dict()
        fx[tag + "/manifest_keys"] = np.array(list(sd.keys()))
        fx[tag + "/manifest_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        fx[tag + "/n_params"] = np.int64(sum(p.numel() for p in net.parameters()))
        sizes = (28, 56, 112, 224)
        xa = [t(f"{tag}.xa{i}", (2, 3, s, s), "unit") for i, s in enumerate(sizes)]
        xb = [t(f"{tag}.xb{i}", (2, 3, s, s), "unit") for i, s in enumerate(sizes)]
        fa = t(tag + ".fa", (2, 1, 19), "designed"); fb = t(tag + ".fb", (2, 1, 19), "designed")
        for i in range(4):
            xb[i][1] = xa[i][1] * 0.8 + 0.2 * xb[i][1]
        fb[1] = fa[1] * 1.2
        net.train()
        ya, yb = net(xa, fa, xb, fb)
        loss = crit(ya, yb, flag)
        loss.backward()
        add(fx, tag + "/out_a", ya); add(fx, tag + "/out_b", yb)
        fx[tag + "/loss"] = np.float64(loss.item())
        fx[tag + "/dist"] = (ya - yb).pow(2).sum(1).detach().numpy().astype(np.float64)
        none = []
        for n, p in net.named_parameters():
            if p.grad is None:
                none.append(n)
            else:
                add(fx, tag + "/grad/" + n, p.grad, k=512)
        fx[tag + "/grad_none"] = np.array(none)
        two = net(xa, fa)                      # 2 args = (patches, designed), NOT a pair (:544-545)
        fx[tag + "/two_args_equals_left"] = np.bool_(torch.equal(two, ya))
        print(tag, "loss", fx[tag + "/loss"], "dist", fx[tag + "/dist"], "none", none)
    # ---- ScaleEmbedTransformer with is_label_embed=True (vit_model.py:369-371, :408-432, :480-483, :503-506): label token,
    #      my_class_head / class_logits, 3-tuple result.  Dropout(0.3) of my_class_head is set to p = 0 on the instance (its RNG
    #      stream is not reproducible); loss = contrastive(embeddings) + cross entropy of both sides' class logits
    #      + 0.01 * sum(x_class^2), so every returned value carries gradient ------------------------------------------------
    tag = "vitscale_label_d2"
    if not have(tag):
        net = vit_model.ScaleEmbedTransformer(img_size=224, patch_size=16, embed_dim=768, depth=2, num_heads=12,
                                              representation_size=None, num_classes=512, is_label_embed=True)
        net.my_class_head[2].p = 0.0
        load_det_weights(net, "")
        sd = net.state_dict()
        fx[tag + "/manifest_keys"] = np.array(list(sd.keys()))
        fx[tag + "/manifest_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        fx[tag + "/n_params"] = np.int64(sum(p.numel() for p in net.parameters()))
        sizes = (28, 56, 112, 224)
        xa = [t(f"{tag}.xa{i}", (2, 3, s, s), "unit") for i, s in enumerate(sizes)]
        xb = [t(f"{tag}.xb{i}", (2, 3, s, s), "unit") for i, s in enumerate(sizes)]
        fa = t(tag + ".fa", (2, 1, 19), "designed"); fb = t(tag + ".fb", (2, 1, 19), "designed")
        for i in range(4):
            xb[i][1] = xa[i][1] * 0.8 + 0.2 * xb[i][1]
        fb[1] = fa[1] * 1.2
        la, lb = torch.tensor([3, 7]), torch.tensor([0, 10])
        net.train()
        ra, rb = net(xa, fa, xb, fb)
        assert len(ra) == 3 and len(rb) == 3
        ce = torch.nn.functional.cross_entropy
        loss = crit(ra[0], rb[0], flag) + ce(ra[1], la) + ce(rb[1], lb) + 0.01 * (ra[2].pow(2).sum() + rb[2].pow(2).sum())
        loss.backward()
        for side, r in (("a", ra), ("b", rb)):
            add(fx, f"{tag}/out_{side}", r[0]); add(fx, f"{tag}/logits_{side}", r[1]); add(fx, f"{tag}/class_{side}", r[2])
        fx[tag + "/loss"] = np.float64(loss.item())
        fx[tag + "/tokens"] = np.int64(201)
        none = []
        for n, p in net.named_parameters():
            if p.grad is None:
                none.append(n)
            else:
                add(fx, tag + "/grad/" + n, p.grad, k=512)
        fx[tag + "/grad_none"] = np.array(none)
        two = net(xa, fa)
        fx[tag + "/two_args_equals_left"] = np.bool_(all(torch.equal(u, v) for u, v in zip(two, ra)))
        print(tag, "loss", fx[tag + "/loss"], "none", none, "params", int(fx[tag + "/n_params"]))
    # ---- VisionTransformer with distilled=True (vit_model.py:217, :225, :250-253, :270, :277-291): DeiT distillation token and
    #      head_dist; training mode returns (x, x_dist) per input, eval mode their average ---------------------------------------
    tag = "vitb16_dist_d2"
    if not have(tag):
        net = vit_model.VisionTransformer(img_size=224, patch_size=16, embed_dim=768, depth=2, num_heads=12,
                                          representation_size=None, num_classes=100, distilled=True)
        load_det_weights(net, "")
        sd = net.state_dict()
        fx[tag + "/manifest_keys"] = np.array(list(sd.keys()))
        fx[tag + "/manifest_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        fx[tag + "/n_params"] = np.int64(sum(p.numel() for p in net.parameters()))
        x1 = t(tag + ".x1", (2, 3, 224, 224), "unit"); x2 = t(tag + ".x2", (2, 3, 224, 224), "unit")
        x2[1] = x1[1] * 0.8 + 0.2 * x2[1]
        net.train()
        (ya, da), (yb, db) = net(x1, x2)
        loss = crit(ya, yb, flag) + crit(da, db, flag)
        loss.backward()
        add(fx, tag + "/out_a", ya); add(fx, tag + "/out_b", yb); add(fx, tag + "/dist_a", da); add(fx, tag + "/dist_b", db)
        fx[tag + "/loss"] = np.float64(loss.item())
        for n, p in net.named_parameters():
            assert p.grad is not None, n
            add(fx, tag + "/grad/" + n, p.grad, k=512)
        net.eval()
        with torch.no_grad():
            add(fx, tag + "/eval_a", net(x1))
        print(tag, "loss", fx[tag + "/loss"], "params", int(fx[tag + "/n_params"]))
    if old is not None:
        fx.update({k: old[k] for k in old.files})
    np.savez_compressed(path, **fx)
    print("model_vit.npz", len(fx))


def gen_nets():
    """Nets.MLP / Nets.FC (MNIST sandbox); Nets.py only needs torch."""
    sys.path.insert(0, REF)
    import Nets  # noqa
    fx = {}
    m = Nets.MLP()
    load_det_weights(m, "nets.mlp.")
    x = t("nets.x", (37, 784), "unit").requires_grad_(True)
    a, b = m(x)
    (a.sum() * 1.5 + (b * b).sum()).backward()
    add(fx, "mlp/fc3_map", a); add(fx, "mlp/fc2_map", b); add(fx, "mlp/dx", x.grad)
    for n, p in m.named_parameters():
        add(fx, "mlp/grad/" + n, p.grad)
    fx["mlp/keys"] = np.array(list(m.state_dict().keys()))
    f = Nets.FC()
    load_det_weights(f, "nets.fc.")
    y = t("nets.y", (37, 250), "normal").requires_grad_(True)
    o = f(y)
    (o * o).sum().backward()
    add(fx, "fc/out", o); add(fx, "fc/dy", y.grad)
    for n, p in f.named_parameters():
        add(fx, "fc/grad/" + n, p.grad)
    # ---- RNN (4-layer bidirectional GRU + attention pooling, Nets.py:48-111); eval mode: its Dropout(0.5) draws from torch's RNG ----
    import contextlib, io
    r = Nets.RNN()
    load_det_weights(r, "nets.rnn.")
    r.eval()
    xr = t("nets.rnn.x", (9, 28, 28), "unit").requires_grad_(True)
    with contextlib.redirect_stdout(io.StringIO()):           # the reference prints tensor sizes
        o = r(xr)
    (o * o).sum().backward()
    add(fx, "rnn/out", o); add(fx, "rnn/dx", xr.grad)
    for n, p in r.named_parameters():
        add(fx, "rnn/grad/" + n, p.grad)
    fx["rnn/keys"] = np.array(list(r.state_dict().keys()))
    path = os.path.join(HERE, "model_nets.npz")
    if os.path.exists(path):                                   # committed cases keep their values: re-running only ADDS
        old = np.load(path)
        fx.update({k: old[k] for k in old.files})
    np.savez_compressed(path, **fx)
    print("model_nets.npz", len(fx))


def import_sweep_reference():
    """ExtractFeatures.py / MyUtils1.py import h5py, osgeo (gdal, ogr) and cv2 at module level (storage, GIS I/O and
    the band resize: none installed here).  Same mechanism as the timm entry above: empty in-process module objects
    satisfy the import statements; no function of those packages is ever called by what the fixtures exercise
    (Euclidean_distance, MC_Lyu_2020, get_scales, calculate_left_top_point_and_size, cut_image, get_designed_features,
    get_all_features with duck-typed feature / raster objects).  cv2.resize is NOT emulated: the resize stays unpinned."""
    for name in ("h5py", "cv2", "osgeo", "osgeo.gdal", "osgeo.ogr", "osgeo.osr"):
        sys.modules.setdefault(name, types.ModuleType(name))
    for sub in ("gdal", "ogr", "osr"):
        setattr(sys.modules["osgeo"], sub, sys.modules["osgeo." + sub])
    sys.path.insert(0, REF)
    import ExtractFeatures  # noqa
    import MyUtils1  # noqa
    return ExtractFeatures, MyUtils1


class _Raster:
    """Duck-typed stand-in for the gdal.Dataset METHODS cut_image / get_all_features call (data holder, no arithmetic)."""

    def __init__(self, img, gt):
        self.img = img
        self.gt = gt
        self.RasterCount, self.RasterYSize, self.RasterXSize = img.shape

    def ReadAsArray(self, x, y, w, h):
        assert 0 <= x and 0 <= y and w >= 0 and h >= 0 and x + w <= self.RasterXSize and y + h <= self.RasterYSize, (x, y, w, h)
        return self.img[:, y:y + h, x:x + w]

    def GetGeoTransform(self):
        return self.gt


class _Point:
    """Duck-typed ogr.Feature: attribute table row + point geometry."""

    def __init__(self, fields, x, y):
        self.fields, self.x, self.y = fields, x, y

    def GetField(self, k):
        return self.fields[k]

    def GetGeometryRef(self):
        return self

    def GetX(self):
        return self.x

    def GetY(self):
        return self.y


def gen_sweep():
    """ExtractFeatures sweep arithmetic and loader window arithmetic from the reference's own functions
    (VERDICT r1 item 1)."""
    EF, MU1 = import_sweep_reference()
    fx = {}
    rng = np.random.default_rng(20240)
    # ---- Euclidean_distance / MC_Lyu_2020 on float32 rows, D = 100 (the feature store's row width) ---------------
    cases = {}
    cases["n1m1"] = (rng.normal(size=(1, 100)) * 0.08, rng.normal(size=(1, 100)) * 0.08)
    cases["n5m7"] = (rng.normal(size=(5, 100)) * 0.1, rng.normal(size=(7, 100)) * 0.1)
    x = rng.normal(size=(6, 100)) * 0.3
    cases["cancel"] = (x, x + rng.normal(size=(6, 100)) * 1e-4)               # x ~ y: expanded form is cancellation noise
    cases["self"] = (x, x.copy())
    a = rng.normal(size=(64, 100)); b = rng.normal(size=(64, 100))
    a /= np.linalg.norm(a, axis=1, keepdims=True); b /= np.linalg.norm(b, axis=1, keepdims=True)
    # distances laid on both sides of the margin 1.0: |a - t*b| swept through 1 (unit vectors, random angle)
    tt = np.linspace(0.0, 1.6, 64)[:, None]
    cases["near_margin"] = (a * 0.75, a * 0.75 - tt * b * 0.9)
    cases["p3"] = (rng.normal(size=(4, 3)), rng.normal(size=(2, 3)))
    for tag, (X, Y) in cases.items():
        X = np.ascontiguousarray(X, np.float32); Y = np.ascontiguousarray(Y, np.float32)
        D1 = EF.Euclidean_distance(X.copy(), Y.copy())
        D2 = EF.MC_Lyu_2020(X.copy(), Y.copy())
        assert D1.dtype == np.float32 and np.array_equal(D1, D2)
        fx[f"dist/{tag}/X"] = X; fx[f"dist/{tag}/Y"] = Y; fx[f"dist/{tag}/D"] = D1
    fx["dist/tags"] = np.array(list(cases.keys()))
    # ---- the per-edge loop body of test_for_shp (ExtractFeatures.py:188-216) on an in-memory feature store ----------
    # rows fetched one by one and np.concatenate'd, np.mean(axis=0), [np.newaxis,:], Euclidean_distance, .max();
    # edges with LEFT_FID/RIGHT_FID == -1 never reach the loop (MyUtils2.py:184-186).
    S, Dm = 60, 100
    counts = rng.integers(1, 6, size=S)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    P = int(ptr[-1])
    idx = rng.permutation(P).astype(np.int32)
    base = rng.normal(size=(S, Dm)) * 0.05
    # neighbouring polygons share a slowly varying component so simi straddles the margin
    drift = np.cumsum(rng.normal(size=(S, Dm)) * 0.055, axis=0)
    F = np.zeros((P, Dm), np.float32)
    for s in range(S):
        F[idx[ptr[s]:ptr[s + 1]]] = (base[s] + drift[s] + rng.normal(size=(counts[s], Dm)) * 0.02).astype(np.float32)
    E = 400
    edges = np.stack([rng.integers(0, S, size=E), rng.integers(0, S, size=E)], 1).astype(np.int32)
    near = rng.random(E) < 0.7
    edges[near, 1] = np.clip(edges[near, 0] + rng.integers(1, 4, size=int(near.sum())), 0, S - 1)
    same = edges[:, 0] == edges[:, 1]
    edges[same, 1] = (edges[same, 0] + 1) % S
    edges[::19, 0] = -1
    edges[7::29, 1] = -1
    simi = np.full(E, np.nan, np.float32)
    pooled = np.zeros((S, Dm), np.float32)
    for e in range(E):
        L, R = int(edges[e, 0]), int(edges[e, 1])
        if L == -1 or R == -1:
            continue
        sides = []
        for poly in (L, R):
            out = []
            for m, pid in enumerate(idx[ptr[poly]:ptr[poly + 1]]):
                row = F[int(pid)][np.newaxis, :]
                out = row if m == 0 else np.concatenate((out, row), axis=0)
            out = np.mean(out, axis=0)
            pooled[poly] = out
            sides.append(out[np.newaxis, :])
        simi[e] = EF.Euclidean_distance(sides[0], sides[1]).max()
    live = ~np.isnan(simi)
    fx["sweep/F"] = F; fx["sweep/ptr"] = ptr; fx["sweep/idx"] = idx; fx["sweep/edges"] = edges
    fx["sweep/simi"] = simi; fx["sweep/pooled"] = pooled
    fx["sweep/pooled_valid"] = np.isin(np.arange(S), edges[live].ravel())
    print("sweep: live", int(live.sum()), "merge fraction", float((simi[live] < 1.0).mean()),
          "min |simi-1|", float(np.abs(simi[live] - 1).min()))
    # ---- loader window arithmetic (MyUtils1.py): get_scales, calculate_left_top_point_and_size, cut_image, and the whole
    # get_all_features chain (designed-feature order, geo -> pixel, windows) with resize_data replaced ON THE INSTANCE by a
    # pass-through so the zero-padded uint8 crops are observable (cv2 is absent; the resize itself stays unpinned) -----
    ds = object.__new__(MU1.MergingSegmensPairDataset)
    io = np.array([[16, 24], [24, 48], [64, 112], [20, 21], [33, 90], [50, 50]], np.int64)
    fx["win/inner_object"] = io
    sc, fc = zip(*(ds.get_scales(int(i), int(o)) for i, o in io))
    fx["win/scales"] = np.array(sc, np.int64); fx["win/factors"] = np.array(fc, np.float64)
    mids = np.array([[10, 10, 8], [10, 10, 7], [2, 1, 7], [0, 0, 1], [5, 9, 24], [100, 3, 33], [0, 0, 6]], np.int64)
    fx["win/mid_len"] = mids
    fx["win/left_top"] = np.array([ds.calculate_left_top_point_and_size(int(a), int(b), int(c)) for a, b, c in mids], np.int64)
    img = rng.integers(0, 256, size=(4, 37, 53), dtype=np.uint8)
    gt = (500000.0, 0.5, 0.0, 4100000.0, 0.0, -0.5)
    raster = _Raster(img, gt)
    fx["crop/img"] = img; fx["crop/gt"] = np.array(gt, np.float64)
    boxes = np.array([[-3, -2, 8], [0, 0, 5], [48, 30, 9], [50, 35, 6], [-10, 10, 12], [20, -4, 11], [-5, -5, 70], [30, 20, 1]], np.int64)
    fx["crop/boxes"] = boxes
    for k, (x0, y0, L) in enumerate(boxes):
        fx[f"crop/out{k}"] = ds.cut_image(raster, (int(x0), int(y0), int(L), int(L)))
    # identity-size windows (L == target, so the resize is the identity whatever its rule): mid-point -> crop, what the GPU
    # gather must reproduce exactly through calculate_left_top_point_and_size + cut_image
    ident = np.array([[3, 3, 32], [50, 35, 32], [26, 18, 32], [0, 36, 64], [52, 0, 64], [26, 18, 64], [-2, 40, 32]], np.int64)
    fx["ident/mid_len"] = ident
    for k, (mx, my, L) in enumerate(ident):
        fx[f"ident/out{k}"] = ds.cut_image(raster, ds.calculate_left_top_point_and_size(int(mx), int(my), int(L)))
    names = ["area", "peri", "len", "width", "smooth", "std0", "std1", "std2", "mean0", "mean1", "mean2", "shapeness", "compact", "bright", "border"]
    fx["point/field_order"] = np.array(names)
    ds.resize_data = lambda region, h, w: region
    pts = []
    for k, (inner, obj, gx, gy) in enumerate(((16, 24, 500003.3, 4099995.2), (24, 48, 500020.75, 4099983.0), (8, 40, 500000.1, 4099999.9))):
        fields = {n: str(round(float(v), 4)) for n, v in zip(names, np.exp(rng.uniform(np.log(1e-2), np.log(1e3), 15)))}
        fields.update(inner=str(inner), object=str(obj))
        designed, scales_t, patches = ds.get_all_features(raster, _Point(fields, gx, gy))
        fx[f"point/{k}/fields"] = np.array([float(fields[n]) for n in names], np.float64)
        fx[f"point/{k}/inner_object_xy"] = np.array([inner, obj, gx, gy], np.float64)
        fx[f"point/{k}/designed"] = designed.numpy()
        fx[f"point/{k}/scales"] = scales_t.numpy()
        for i, p in enumerate(patches):
            fx[f"point/{k}/crop{i}"] = p
        pts.append(k)
    fx["point/n"] = np.int64(len(pts))
    np.savez_compressed(os.path.join(HERE, "sweep.npz"), **fx)
    print("sweep.npz", len(fx))


def main():
    warnings.filterwarnings("ignore")
    torch.manual_seed(0)
    torch.set_num_threads(8)
    S2F, vit_model, Losses = import_reference()
    which = sys.argv[1:] or ["relpos", "ops", "model", "vit", "variants", "aux", "nets", "sweep"]
    if "relpos" in which:
        gen_relpos(S2F)
    if "ops" in which:
        gen_ops(S2F, Losses)
    if "model" in which:
        gen_model(S2F, Losses)
    if "model" in which or "model_f64" in which:
        gen_model_f64(S2F, Losses)
    if "vit" in which:
        gen_vit(vit_model, Losses)
    if "variants" in which:
        gen_variants(S2F, Losses)
    if "aux" in which:
        gen_aux(S2F, Losses)
    if "nets" in which:
        gen_nets()
    if "sweep" in which:
        gen_sweep()


if __name__ == "__main__":
    main()

