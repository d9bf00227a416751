"""GPU: dm_pair_epoch_draw against the numpy restatement (bit for bit), and Train_SMT.train: equal to a hand-written loop, resume
equal to an uninterrupted run, the padded tile canvas, the reference's checkpoint cadence / dict, and which models it takes."""
import glob
import os

import numpy as np
import pytest
import torch

import train_smt_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALES = [32, 64, 128]


# ---- 1. the kernel against the restatement --------------------------------------------------------------------------------
def _draw_inputs(rng, N):
    """Polygons of 1 or 9 points (every point in exactly one polygon, ids shuffled), N distinct pairs, random flags."""
    n_poly = max(4, int(np.sqrt(2 * N)) + 2)
    counts = np.where(rng.random(n_poly) < 0.5, 1, 9)
    n_pts = int(counts.sum())
    poly_off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    poly_pts = rng.permutation(n_pts).astype(np.int32)
    flat = rng.choice(n_poly * n_poly, size=N, replace=False)
    pairs = np.stack((flat // n_poly, flat % n_poly), 1).astype(np.int32)
    pts = {"tile": rng.integers(0, 5, n_pts).astype(np.int32), "xy": rng.integers(0, 4000, (n_pts, 2)).astype(np.int32),
           "inner": rng.integers(1, 50, n_pts).astype(np.int32), "obj": rng.integers(50, 100, n_pts).astype(np.int32),
           "region": rng.standard_normal((n_pts, 15)).astype(np.float32)}
    return pairs, rng.integers(0, 2, N).astype(np.int32), poly_off, poly_pts, pts


def _kernel_table(pairs, flag, poly_off, poly_pts, pts, seed, epoch, batch):
    from deepmerge_amd import ops
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    N = len(pairs)
    out = {"tile_id": torch.full((2 * N,), 7, dtype=torch.int32, device=DEV), "xy": torch.full((2 * N, 2), 7, dtype=torch.int32, device=DEV),
           "inner": torch.full((2 * N,), 7, dtype=torch.int32, device=DEV), "obj": torch.full((2 * N,), 7, dtype=torch.int32, device=DEV),
           "region": torch.full((2 * N, 15), 7.0, device=DEV), "flag": torch.full((N,), 7.0, device=DEV),
           "point_id": torch.full((2 * N,), 7, dtype=torch.int32, device=DEV)}
    ops.pair_epoch_draw(up(pairs), up(flag), up(poly_off), up(poly_pts), up(pts["tile"]), up(pts["xy"]), up(pts["inner"]), up(pts["obj"]),
                        up(pts["region"]), seed, epoch, batch, out["tile_id"], out["xy"], out["inner"], out["obj"], out["region"], out["flag"],
                        point_id=out["point_id"])
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("N", [1, 10, 1000, 70000])
def test_epoch_draw_matches_restatement_bit_for_bit(N):
    rng = np.random.default_rng(N)
    pairs, flag, poly_off, poly_pts, pts = _draw_inputs(rng, N)
    owner = np.empty(len(poly_pts), np.int64)
    for p in range(len(poly_off) - 1):
        owner[poly_pts[poly_off[p]:poly_off[p + 1]]] = p
    pair_index = {(int(a), int(b)): k for k, (a, b) in enumerate(pairs)}
    for seed in (0, 0x9E3779B97F4A7C15):
        for epoch in (0, 3):
            for batch in (1, 4, 7, 120):
                got = _kernel_table(pairs, flag, poly_off, poly_pts, pts, seed, epoch, batch)
                want = R.epoch_table(pts, pairs, flag, poly_off, poly_pts, seed, epoch, batch)
                for k in want:
                    assert got[k].dtype == want[k].dtype and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (k, seed, epoch, batch)
                # structure: each pair exactly once, its points drawn from its own polygons, flags following their pairs
                rl, rr = R.blocked_rows(N, batch)
                pl, pr = owner[got["point_id"][rl]], owner[got["point_id"][rr]]
                ks = np.asarray([pair_index[(int(a), int(b))] for a, b in zip(pl, pr)])
                assert np.array_equal(np.sort(ks), np.arange(N))
                assert np.array_equal(got["flag"], flag[ks].astype(np.float32))
    if N >= 1000:
        assert not np.array_equal(_kernel_table(pairs, flag, poly_off, poly_pts, pts, 0, 0, 7)["point_id"],
                                  _kernel_table(pairs, flag, poly_off, poly_pts, pts, 0, 1, 7)["point_id"])


def test_epoch_draw_rejects_bad_arguments():
    from deepmerge_amd import ops
    rng = np.random.default_rng(5)
    pairs, flag, poly_off, poly_pts, pts = _draw_inputs(rng, 10)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    o = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device=DEV)
    args = [up(pairs), up(flag), up(poly_off), up(poly_pts), up(pts["tile"]), up(pts["xy"]), up(pts["inner"]), up(pts["obj"]), up(pts["region"])]
    outs = [o(20), o(20, 2), o(20), o(20), o(20, 15, dt=torch.float32), o(10, dt=torch.float32)]
    with pytest.raises(ValueError, match="batch"):
        ops.pair_epoch_draw(*args, 0, 0, 0, *outs)
    with pytest.raises(ValueError, match="xy"):
        ops.pair_epoch_draw(*args, 0, 0, 4, outs[0], o(20, 3), *outs[2:])
    bad = list(args)
    bad[0] = up(pairs.astype(np.int64))
    with pytest.raises(ValueError, match="pairs"):
        ops.pair_epoch_draw(*bad, 0, 0, 4, *outs)


# ---- a small synthetic dataset: two images of different sizes --------------------------------------------------------------
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


def _hand_loop(net, ds, batch, epochs, lr_init, milestones, margin=1.0, lamda=0.1, belta=0):
    """The composition train() promises, written out: the restatement's tables, PairFeed, eager PairTrainer steps."""
    from deepmerge_amd import Train_SMT
    from deepmerge_amd.feed import PairFeed, PairTable
    from deepmerge_amd.trainer import PairTrainer
    h = ds.host
    pts = {"tile": h.pt_tile, "xy": h.pt_xy, "inner": h.pt_inner, "obj": h.pt_obj, "region": h.pt_region}
    tr = PairTrainer(net, margin=margin, lr=lr_init, lamda=lamda, belta=belta)
    N = len(h.pairs)
    mw = ds.max_window(len(SCALES))
    feeds = {}
    means = []
    for e in range(epochs):
        lr = Train_SMT.epoch_lr(lr_init, e, milestones, 0.2)
        tab = R.epoch_table(pts, h.pairs, h.flag, h.poly_off, h.poly_pts, ds.seed, e, batch)
        total = torch.zeros((), dtype=torch.float32, device=DEV)
        steps = -(-N // batch)
        for s in range(steps):
            b = min(batch, N - s * batch)
            lo = 2 * s * batch
            up = lambda k: torch.from_numpy(np.ascontiguousarray(tab[k][lo:lo + 2 * b])).to(DEV)
            table = PairTable(tile_id=up("tile_id"), xy=up("xy"), inner=up("inner"), obj=up("obj"), region=up("region"),
                              flag=torch.from_numpy(tab["flag"][s * batch:s * batch + b]).to(DEV))
            if b not in feeds:
                feeds[b] = PairFeed(ds.tiles, SCALES, b, mw, numerics="bf16")
            total += tr.step(*feeds[b].fill(table), lr=lr)
        means.append(float(total) / steps)
        for f in feeds.values():
            f.check()
    return means, tr


def test_train_equals_hand_loop_bit_for_bit(tmp_path):
    """3 epochs of N = 10 pairs at train_bs = 4: two graph-replayed steps and one eager tail step per epoch in train(), all eager
    in the hand loop -- same per-epoch losses and weights, bit for bit."""
    from deepmerge_amd import Train_SMT
    from deepmerge_amd.dataset import PairDataset
    ds = PairDataset.from_arrays(_images(), seed=11)
    assert len(ds) == 10 and (ds.positive_pair_number, ds.negative_pair_number) == (6, 4)
    net_a = _net()
    net_b = _net()
    it, losses = Train_SMT.train(net_a, 1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0, dataset=ds, num_epochs=3, milestones=(1, 2),
                                 model_paras_path=str(tmp_path))
    assert it == [0, 1, 2] and all(np.isfinite(losses))
    want, _ = _hand_loop(net_b, ds, 4, 3, 1e-3, (1, 2))
    assert losses == want
    for (k, a), (k2, b) in zip(net_a.state_dict().items(), net_b.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    assert glob.glob(os.path.join(str(tmp_path), "*.pth")) == []         # epochs 1..3: no checkpoint due


def test_train_replays_stay_correct_after_eager_tail_steps():
    """trainer.step(eager=True) between replays: the replays after it still equal eager steps (a full epoch of 3 graph steps + a
    tail on both sides of it)."""
    from deepmerge_amd import Train_SMT
    from deepmerge_amd.dataset import PairDataset
    ds = PairDataset.from_arrays(_images(1, n_pos=6, n_neg=3), seed=2)
    assert len(ds) == 9
    net_a, net_b = _net(5), _net(5)
    _, losses = Train_SMT.train(net_a, 1.0, 2, 1e-3, 0.0, 0.0, 0.1, 0, dataset=ds, num_epochs=2, model_paras_path="unused")
    want, _ = _hand_loop(net_b, ds, 2, 2, 1e-3, (40, 80))
    assert losses == want
    assert all(torch.equal(a, b) for a, b in zip(net_a.state_dict().values(), net_b.state_dict().values()))


def test_resume_equals_uninterrupted(tmp_path, monkeypatch):
    """6 epochs straight == 5 epochs, checkpoint, fresh net resumed from `..._5epochs.pth`: same weights and Adam state after epoch
    index 5.  milestones (2, 4) make the saved lr differ from lr_init."""
    from deepmerge_amd import Train_SMT
    from deepmerge_amd.dataset import PairDataset
    monkeypatch.setattr(Train_SMT, "checkpoint_due", lambda e: e in (4, 5))       # also write the last epoch, to compare its state
    ds = PairDataset.from_arrays(_images(2), seed=7)
    a, b = tmp_path / "straight", tmp_path / "resumed"
    _, straight = Train_SMT.train(_net(), 1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0, dataset=ds, num_epochs=6, milestones=(2, 4), model_paras_path=str(a))
    five = glob.glob(os.path.join(str(a), "*_5epochs.pth"))
    assert len(five) == 1
    saved = torch.load(five[0], weights_only=False)
    assert saved["epoch"] == 4 and saved["optimizer"]["param_groups"][0]["lr"] == Train_SMT.epoch_lr(1e-3, 4, (2, 4), 0.2) != 1e-3
    it, resumed = Train_SMT.train(_net(99), 1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0, True, five[0], dataset=ds, num_epochs=6, milestones=(2, 4),
                                  model_paras_path=str(b))
    assert it == [5] and resumed == straight[5:]
    x = torch.load(glob.glob(os.path.join(str(a), "*_6epochs.pth"))[0], weights_only=False)
    y = torch.load(glob.glob(os.path.join(str(b), "*_6epochs.pth"))[0], weights_only=False)
    assert x["epoch"] == y["epoch"] == 5
    for k in x["net"]:
        assert torch.equal(x["net"][k], y["net"][k]), k
    ox, oy = x["optimizer"], y["optimizer"]
    assert ox["param_groups"] == oy["param_groups"] and sorted(ox["state"]) == sorted(oy["state"])
    for i in ox["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(ox["state"][i][k], oy["state"][i][k]), (i, k)
    with pytest.raises(ValueError, match="start_epoch"):
        Train_SMT.train(_net(), 1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0, True, five[0], dataset=ds, num_epochs=5)


def test_padded_canvas_patches_equal_the_unpadded_image():
    """A point at the right / bottom edge of the SMALLER image: its patches from the dataset's zero-padded canvas equal
    patches.point_batch on that image alone."""
    from deepmerge_amd.dataset import PairDataset
    from deepmerge_amd.feed import PairFeed
    from deepmerge_amd.patches import point_batch
    ims = _images(4)
    small = ims[0]                                     # 150 x 180 against 210 x 170: padded on both axes
    small["xy"][0] = (178, 148)
    small["inner"][0], small["obj"][0] = 30, 70
    small["polygon_points"][0] = "0"
    ds = PairDataset.from_arrays(ims, seed=1, n_scales=3)
    assert tuple(ds.tiles.shape) == (2, 3, 210, 180)
    table = ds.epoch(0, len(ds))
    rows = np.nonzero(table.cols["point_id"].cpu().numpy() == 0)[0]
    assert rows.size >= 1
    feed = PairFeed(ds.tiles, SCALES, len(ds), ds.max_window(3), rows=False)
    left, ld, right, rd, _ = feed.fill(table.step(0))
    feed.check()
    P = len(ds)
    tile = torch.from_numpy(small["tile"]).to(DEV)
    want, wd = point_batch(tile, torch.tensor([[178, 148]], dtype=torch.int32, device=DEV), torch.tensor([30]), torch.tensor([70]),
                           torch.from_numpy(small["region"][:1]).to(DEV), scales=SCALES)
    for r in rows:
        for i in range(len(SCALES)):
            got = left[i][r] if r < P else right[i][r - P]
            assert torch.equal(got, want[i][0]), (r, i)
        got_d = ld[r] if r < P else rd[r - P]
        assert torch.equal(got_d, wd[0])


def test_checkpoint_cadence_keys_and_reference_format_resume(tmp_path):
    """A 10-epoch run writes exactly the reference's `_5epochs` and `_10epochs` files with its dict; a checkpoint in the reference's
    own format (torch.optim.Adam state, test_checkpoint.py's layout) resumes."""
    from deepmerge_amd import Train_SMT
    from deepmerge_amd.dataset import PairDataset
    ds = PairDataset.from_arrays(_images(3), seed=0)
    net = _net()
    Train_SMT.train(net, 1.0, 4, 1e-4, 0.0, 0.0, 0.1, 0, dataset=ds, num_epochs=10, model_paras_path=str(tmp_path / "run"))
    files = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "run" / "*.pth")))
    assert len(files) == 2 and files[0].endswith("_10epochs.pth") and files[1].endswith("_5epochs.pth"), files
    for f, epoch in zip(files, (9, 4)):
        st = torch.load(str(tmp_path / "run" / f), weights_only=False)
        assert list(st.keys()) == ["net", "optimizer", "epoch", "time", "scales", "depth", "name"] and st["epoch"] == epoch
        assert st["scales"] == SCALES and st["depth"] == [1, 1, 1] and st["name"] == net.name
    # the reference's own writer: torch.optim.Adam over filter(requires_grad), a few steps on CPU
    ref = _net(8).cpu()
    pg = [p for p in ref.parameters() if p.requires_grad]
    opt = torch.optim.Adam(pg, lr=2e-4)
    g = torch.Generator().manual_seed(0)
    for _ in range(2):
        for p in pg:
            p.grad = 1e-3 * torch.randn(p.shape, generator=g)
        opt.step()
    path = str(tmp_path / "reference.pth")
    torch.save({"net": ref.state_dict(), "optimizer": opt.state_dict(), "epoch": 7, "time": 1.0, "scales": SCALES, "depth": [1, 1, 1],
                "name": ref.name}, path)
    it, losses = Train_SMT.train(_net(9), 1.0, 4, 1e-4, 0.0, 0.0, 0.1, 0, is_retrained=True, checkpoint_path=path, dataset=ds,
                                 num_epochs=10, model_paras_path=str(tmp_path / "resumed"))
    assert it == [8, 9] and all(np.isfinite(losses))
    st = torch.load(glob.glob(str(tmp_path / "resumed" / "*_10epochs.pth"))[0], weights_only=False)
    assert st["optimizer"]["param_groups"][0]["lr"] == 2e-4 and float(st["optimizer"]["state"][0]["step"]) == 2 + 2 * 3


def test_v2_trains_through_fp32_patches():
    """Models without forward_pair_batched (ShfitScaleFormer_v2) are fed fp32 patch tensors by the same draw."""
    from deepmerge_amd import Train_SMT
    from deepmerge_amd.dataset import PairDataset
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v2
    from deepmerge_amd.trainer import stacked_pair_inputs
    ds = PairDataset.from_arrays(_images(5), seed=0)
    torch.manual_seed(0)
    net = ShfitScaleFormer_v2(cube_size=[8, 8], input_image_scales=list(SCALES), numerics="bf16")
    assert not stacked_pair_inputs(net)
    before = net.state_dict()["final_features_with_design.weight"].clone()
    it, losses = Train_SMT.train(net, 1.0, 4, 1e-4, 0.0, 0.0, 0.1, 0, dataset=ds, num_epochs=1, model_paras_path="unused")
    assert it == [0] and np.isfinite(losses[0])
    assert not torch.equal(net.state_dict()["final_features_with_design.weight"].cpu(), before)
