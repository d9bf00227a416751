"""GPU: held-out pair validation.  dm_contrastive_terms against a numpy restatement of its pinned order (bit for bit),
dm_pair_eval_summary against numpy counts and math.fsum, PairEvaluator.run() against a hand-written loop over the same draw, and
train(..., val_dataset=) against train() without it (bit for bit), with the reference's LossHistory files."""
import glob
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALES = [32, 64, 128]
F32 = np.float32


# ---- numpy restatements -----------------------------------------------------------------------------------------------------
def terms_ref(a, b, flag, margin):
    """lane l sums (a - b)^2 over columns l, l+64, ... in order, xor butterfly 32 .. 1, then
    f*d2 + (1-f)*max(margin - d2, 0) left to right -- every operation a rounded float32 one."""
    a, b, flag = a.astype(F32), b.astype(F32), flag.astype(F32)
    B, D = a.shape
    d = a - b
    sq = d * d
    part = np.zeros((B, 64), F32)
    for c0 in range(0, D, 64):
        w = min(64, D - c0)
        part[:, :w] = part[:, :w] + sq[:, c0:c0 + w]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lanes ^ o]
    d2 = part[:, 0]
    m = F32(margin) - d2
    h = np.where(m < 0, F32(0), m).astype(F32)
    return d2, (flag * d2 + (F32(1) - flag) * h).astype(F32)


def counts_ref(simi, flag, th):
    """merged[c][j] = #{class c : simi < th[j]} by sorting (NaN sorts last and is never below a threshold)."""
    pos, neg = np.sort(simi[flag == 1]), np.sort(simi[flag != 1])
    return np.searchsorted(pos, th, side="left"), np.searchsorted(neg, th, side="left"), int((flag == 1).sum())


def _bits_equal(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ---- 1. dm_contrastive_terms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 7, 3000])
@pytest.mark.parametrize("D", [64, 100, 130])
def test_contrastive_terms_match_restatement_bit_for_bit(B, D):
    from deepmerge_amd import ops
    rng = np.random.default_rng(B * 1000 + D)
    a = rng.standard_normal((B, D)).astype(F32)
    spread = rng.uniform(0.005, 0.3, (B, 1))
    spread[-1], spread[0] = 0.3, 0.005                          # d2 ~ 2 D spread^2: one row each side of the hinge at least
    b = (a + rng.standard_normal((B, D)) * spread).astype(F32)
    flag = (rng.random(B) < 0.5).astype(F32)
    flag[0] = 1.0
    if B > 1:
        flag[1] = 0.0
    for margin in (1.0, 0.7):
        d2, term = ops.contrastive_terms(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), torch.from_numpy(flag).to(DEV), margin)
        want_d2, want_term = terms_ref(a, b, flag, margin)
        assert _bits_equal(d2.cpu().numpy(), want_d2)
        assert _bits_equal(term.cpu().numpy(), want_term)
    # both branches of the hinge are exercised
    assert (want_d2 < 0.7).any() and (B == 1 or (want_d2 > 1.0).any())


def test_contrastive_terms_write_into_views_and_refuse_bad_shapes():
    from deepmerge_amd import ops
    a = torch.randn(10, 100, device=DEV)
    flag = torch.ones(5, device=DEV)
    buf = torch.full((12,), 7.0, device=DEV)
    d2 = torch.empty(12, device=DEV)
    ops.contrastive_terms(a[:5], a[5:], flag, 1.0, d2=d2[3:8], term=buf[3:8])
    torch.cuda.synchronize()
    assert buf[:3].eq(7).all() and buf[8:].eq(7).all() and torch.equal(buf[3:8], d2[3:8])      # flag 1: term = d2
    with pytest.raises(ValueError):
        ops.contrastive_terms(a[:5], a[:4], flag, 1.0)
    with pytest.raises(ValueError):
        ops.contrastive_terms(a[:5].double(), a[5:].double(), flag, 1.0)
    with pytest.raises(ValueError):
        ops.contrastive_terms(a[:5], a[5:], flag[:4], 1.0)


# ---- 2. dm_pair_eval_summary ------------------------------------------------------------------------------------------------
def _summary(term, simi, flag, th):
    from deepmerge_amd import ops
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    block = ops.pair_eval_summary(up(term), up(simi), up(flag), up(th)).cpu()
    T = len(th)
    return float(block[:1].view(torch.float64)[0]), int(block[1]), block[2:].view(2, T).numpy()


@pytest.mark.parametrize("N", [1, 1000, 10 ** 6])
@pytest.mark.parametrize("T", [1, 17, 1024])
def test_pair_eval_summary_counts_and_loss(N, T):
    rng = np.random.default_rng(N + T)
    th = np.sort(rng.choice(np.arange(1, 4 * T + 1), T, replace=False)).astype(F32) / F32(2 * T)
    simi = rng.uniform(0, 2.2, N).astype(F32)
    k = min(N, max(1, N // 4))
    simi[:k] = th[rng.integers(0, T, k)]                       # exactly on a threshold: not merged there
    if N > 2:
        simi[rng.integers(0, N, max(1, N // 50))] = np.nan     # never merged
    term = (rng.exponential(1.0, N) * (rng.random(N) < 0.9)).astype(F32)
    for flag in ((rng.random(N) < 0.4).astype(F32), np.ones(N, F32), np.zeros(N, F32)):   # both classes, then each one empty
        loss, n_pos, merged = _summary(term, simi, flag, th)
        mp, mn, want_pos = counts_ref(simi, flag, th)
        assert n_pos == want_pos
        assert np.array_equal(merged[0], mp) and np.array_equal(merged[1], mn)
        want = math.fsum(term.astype(np.float64))
        assert abs(loss - want) <= 1e-12 * abs(want) + 1e-300
        again, _, merged2 = _summary(term, simi, flag, th)
        assert np.float64(again).tobytes() == np.float64(loss).tobytes() and np.array_equal(merged, merged2)


def test_pair_eval_summary_refuses_bad_arguments():
    from deepmerge_amd import ops
    t = torch.zeros(10, device=DEV)
    ok = torch.tensor([0.5, 1.0], device=DEV)
    with pytest.raises(ValueError, match="N"):
        ops.pair_eval_summary(t[:0], t[:0], t[:0], ok)
    with pytest.raises(ValueError, match="thresholds"):
        ops.pair_eval_summary(t, t, t, ok[:0])
    with pytest.raises(ValueError, match="thresholds"):
        ops.pair_eval_summary(t, t, t, torch.linspace(0, 1, 1025, device=DEV))
    with pytest.raises(ValueError, match="ascending"):
        ops.pair_eval_summary(t, t, t, torch.tensor([1.0, 0.5], device=DEV))
    with pytest.raises(ValueError, match="finite"):
        ops.pair_eval_summary(t, t, t, torch.tensor([0.5, float("inf")], device=DEV))
    with pytest.raises(ValueError, match="simi"):
        ops.pair_eval_summary(t, t[:9], t, ok)


# ---- a small synthetic dataset (as tests/test_gpu_train_smt.py builds it) -------------------------------------------------
def _images(seed=0, n_pos=6, n_neg=4):
    rng = np.random.default_rng(seed)
    ims = []
    for i, (h, w) in enumerate(((150, 180), (210, 170))):
        n = 24
        xy = np.stack((rng.integers(0, w, n), rng.integers(0, h, n)), 1)
        inner = rng.integers(8, 30, n)
        ims.append({"tile": rng.integers(0, 256, size=(3, h, w), dtype=np.uint8), "xy": xy, "inner": inner,
                    "obj": inner + rng.integers(4, 40, n), "region": rng.random((n, 15), dtype=np.float32),
                    "polygon_points": [" ".join(str(q) for q in range(k, n, 8)) for k in range(8)]})
    ims[0]["positive"], ims[1]["positive"] = np.array([[0, 1], [2, 3], [4, 5]]), np.array([[1, 2], [3, 4], [6, 7]])[: n_pos - 3]
    ims[0]["negative"], ims[1]["negative"] = np.array([[0, 7], [5, 6]]), np.array([[0, 5], [2, 7]])[: n_neg - 2]
    return ims


def _net(seed=3):
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    torch.manual_seed(seed)
    return ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=list(SCALES), depth=[1, 1, 1], in_c=3, numerics="bf16").to(DEV)


def _v2_net(seed=0):
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v2
    torch.manual_seed(seed)
    return ShfitScaleFormer_v2(cube_size=[8, 8], input_image_scales=list(SCALES), numerics="bf16").to(DEV)


# ---- 3. PairEvaluator against a hand-written loop ---------------------------------------------------------------------------
def _hand_eval(net, ds, batch, margin, draw_key=0):
    """The composition PairEvaluator promises, written out: the draw, feeds, eval forwards, the sweep with one point per polygon,
    the restated terms."""
    from deepmerge_amd.ExtractFeatures import rag_similarity_sweep
    from deepmerge_amd.feed import PairFeed
    from deepmerge_amd.trainer import stacked_pair_inputs
    table = ds.epoch(draw_key, batch)
    feeds, simi, merge, terms, flags = {}, [], [], [], []
    net.eval()
    with torch.no_grad():
        for s in range(len(table)):
            b = table.pairs_in_step(s)
            if b not in feeds:
                feeds[b] = PairFeed(ds.tiles, SCALES, b, ds.max_window(len(SCALES)), rows=stacked_pair_inputs(net), numerics="bf16")
            f = feeds[b]
            _, _, _, _, flag = f.fill(table.step(s))
            F = net(f.both, f.dboth)
            i = torch.arange(b, dtype=torch.int32, device=DEV)
            ptr = torch.arange(2 * b + 1, dtype=torch.int32, device=DEV)
            _, sm, mg = rag_similarity_sweep(F, ptr, ptr[:-1], torch.stack((i, i + b), 1), margin=margin)
            Fh = F.cpu().numpy()
            fl = flag.cpu().numpy()
            terms.append(terms_ref(Fh[:b], Fh[b:], fl, margin)[1])
            simi.append(sm.cpu().numpy())
            merge.append(mg.cpu().numpy())
            flags.append(fl)
    for f in feeds.values():
        f.check()
    return np.concatenate(simi), np.concatenate(merge), np.concatenate(terms), np.concatenate(flags)


@pytest.mark.parametrize("kind", ["v3", "v2"])
def test_evaluator_equals_hand_loop(kind):
    from deepmerge_amd.dataset import PairDataset
    from deepmerge_amd.evaluate import PairEvaluator, threshold_set
    from deepmerge_amd.trainer import stacked_pair_inputs
    ds = PairDataset.from_arrays(_images(6), seed=4)
    assert len(ds) == 10
    net = _net(1) if kind == "v3" else _v2_net(1)
    assert stacked_pair_inputs(net) == (kind == "v3")
    margin, batch = 0.05, 4                                     # 2 full batches + a tail of 2
    th = [0.01, 0.02, 0.04, 0.08, 0.5]
    net.train()
    ev = PairEvaluator(net, ds, batch=batch, margin=margin, thresholds=th, draw_key=3)
    r = ev.run()
    assert net.training                                         # the mode is restored
    simi, term = ev.simi.cpu().numpy(), ev.term.cpu().numpy()
    want_simi, want_merge, want_term, flag = _hand_eval(net, ds, batch, margin, draw_key=3)
    net.train()
    assert _bits_equal(simi, want_simi) and np.array_equal(simi < F32(margin), want_merge)
    assert _bits_equal(term, want_term)
    full = threshold_set(th, margin)
    assert r.thresholds == tuple(float(x) for x in full)
    mp, mn, n_pos = counts_ref(want_simi, flag, full)
    assert (r.n_pairs, r.n_pos, r.n_neg) == (10, n_pos, 10 - n_pos) and n_pos == ds.positive_pair_number
    assert r.merged_pos == tuple(int(x) for x in mp) and r.merged_neg == tuple(int(x) for x in mn)
    j = list(full).index(F32(margin))
    assert (r.tp, r.fp) == (mp[j], mn[j])
    assert abs(r.loss - math.fsum(want_term.astype(np.float64)) / 10) <= 1e-12 * abs(r.loss)
    net.eval()
    assert ev.run() == r and not net.training                  # a second run: same result, eval mode kept


# ---- 4./5. train() with validation ------------------------------------------------------------------------------------------
def _last_checkpoint(path):
    files = glob.glob(os.path.join(path, "*_3epochs.pth"))
    assert len(files) == 1
    return torch.load(files[0], weights_only=False)


def test_train_with_validation_is_bit_identical_and_logs(tmp_path, monkeypatch):
    from deepmerge_amd import Train_SMT
    from deepmerge_amd.dataset import PairDataset
    from deepmerge_amd.evaluate import PairEvaluator
    monkeypatch.setattr(Train_SMT, "checkpoint_due", lambda e: e == 2)        # the last epoch's state, Adam moments included
    ds = PairDataset.from_arrays(_images(), seed=11)
    val = PairDataset.from_arrays(_images(7, n_pos=6, n_neg=3), seed=5)
    assert len(ds) == 10 and len(val) == 9
    args = (1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0)
    net_a, net_b = _net(), _net()
    it_a, loss_a = Train_SMT.train(net_a, *args, dataset=ds, num_epochs=3, milestones=(1, 2), model_paras_path=str(tmp_path / "plain"))
    hist = []
    it_b, loss_b = Train_SMT.train(net_b, *args, dataset=ds, num_epochs=3, milestones=(1, 2), model_paras_path=str(tmp_path / "val"),
                                   val_dataset=val, val_batch=4, log_dir=str(tmp_path / "logs"), val_history=hist)
    assert it_a == it_b == [0, 1, 2] and loss_a == loss_b
    for (k, a), (k2, b) in zip(net_a.state_dict().items(), net_b.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    x, y = _last_checkpoint(str(tmp_path / "plain")), _last_checkpoint(str(tmp_path / "val"))
    assert x["optimizer"]["param_groups"] == y["optimizer"]["param_groups"]
    for i in x["optimizer"]["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(x["optimizer"]["state"][i][k], y["optimizer"]["state"][i][k]), (i, k)
    # one entry per epoch; the last equals a standalone evaluation of the final weights
    assert [e for e, _ in hist] == [0, 1, 2] and all(np.isfinite(r.loss) for _, r in hist)
    assert hist[-1][1] == PairEvaluator(net_b, val, batch=4, margin=1.0).run()
    # the reference's three files, one line per epoch
    d = glob.glob(str(tmp_path / "logs" / "loss_*"))
    assert len(d) == 1
    t = os.path.basename(d[0])[len("loss_"):]
    read = lambda kind: open(os.path.join(d[0], f"epoch_{kind}_{t}.txt")).read().splitlines()
    assert read("loss") == [str(v) for v in loss_b]
    assert read("val_loss") == [str(r.loss) for _, r in hist]
    assert read("f_score") == [str(r.f_score) for _, r in hist]
    with pytest.raises(ValueError, match="val_dataset"):
        Train_SMT.train(_net(), *args, dataset=ds, num_epochs=1, val_dataset=ds)


def test_train_log_dir_without_validation_writes_upstream_stand_ins(tmp_path):
    from deepmerge_amd import Train_SMT
    from deepmerge_amd.dataset import PairDataset
    ds = PairDataset.from_arrays(_images(2), seed=1)
    _, losses = Train_SMT.train(_net(), 1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0, dataset=ds, num_epochs=2, model_paras_path="unused",
                                log_dir=str(tmp_path))
    d = glob.glob(str(tmp_path / "loss_*"))
    assert len(d) == 1
    t = os.path.basename(d[0])[len("loss_"):]
    read = lambda kind: open(os.path.join(d[0], f"epoch_{kind}_{t}.txt")).read().splitlines()
    assert read("loss") == read("val_loss") == [str(v) for v in losses]
    elapsed = [float(v) for v in read("f_score")]
    assert len(elapsed) == 2 and 0 <= elapsed[0] <= elapsed[1] and all(round(v, 2) == v for v in elapsed)
