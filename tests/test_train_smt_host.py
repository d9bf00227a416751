"""CPU: the per-epoch draw's RNG contract (numpy restatement), the pair-list reader, PairDataset's host validation,
and Train_SMT's schedule and checkpoint file names against the reference's torch objects."""
import time

import numpy as np
import pytest
import torch

import train_smt_ref as R
from deepmerge_amd import Train_SMT
from deepmerge_amd.dataset import build_host, read_pair_list


def test_philox_known_answers():
    assert [int(x) for x in R.philox4x32_10((0, 0, 0, 0), (0, 0))] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    m = 0xFFFFFFFF
    assert [int(x) for x in R.philox4x32_10((m, m, m, m), (m, m))] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert R.seed_key(0x0123456789ABCDEF) == (0x89ABCDEF, 0x01234567)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 1000, 65537])
def test_feistel_shuffle_is_a_permutation(n):
    for seed, epoch in ((0, 0), (12345, 7)):
        src = R.epoch_perm(n, seed, epoch)
        assert np.array_equal(np.sort(src), np.arange(n))
    if n >= 64:
        assert not np.array_equal(R.epoch_perm(n, 0, 0), R.epoch_perm(n, 0, 1))      # a new order every epoch


def test_blocked_rows_layout():
    left, right = R.blocked_rows(10, 4)
    assert left.tolist() == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17]
    assert right.tolist() == [4, 5, 6, 7, 12, 13, 14, 15, 18, 19]
    assert sorted(left.tolist() + right.tolist()) == list(range(20))


def test_read_pair_list(tmp_path):
    p = tmp_path / "image_a.txt"
    p.write_text("0,3,5\n1,7,2,9,9\n\n2,11,4\n")
    got = read_pair_list(str(p))
    assert got.dtype == np.int32 and got.tolist() == [[3, 5], [7, 2], [11, 4]]
    (tmp_path / "empty.txt").write_text("")
    assert read_pair_list(str(tmp_path / "empty.txt")).shape == (0, 2)


def _image(h=64, w=80, n=6, bands=3):
    rng = np.random.default_rng(h * w + n)
    return {"tile": rng.integers(0, 256, size=(bands, h, w), dtype=np.uint8),
            "xy": np.stack((rng.integers(0, w, n), rng.integers(0, h, n)), 1), "inner": np.full(n, 8), "obj": np.full(n, 20),
            "region": rng.random((n, 15), dtype=np.float32), "polygon_points": [[0, 1], "2 3", np.array([4, 5])],
            "positive": np.array([[0, 1]]), "negative": np.array([[1, 2], [0, 2]])}


def test_host_build_joins_images():
    a, b = _image(), _image(h=40, w=96, n=4)
    b["polygon_points"] = ["0", "1 2 3"]
    b["positive"], b["negative"] = np.array([[0, 1]]), np.zeros((0, 2))
    h = build_host([a, b], n_scales=3)
    assert h.tiles.shape == (2, 3, 64, 96) and h.tiles[1, :, 40:, :].max() == 0 and h.tiles[0, :, :, 80:].max() == 0
    assert np.array_equal(h.tiles[1, :, :40, :96], b["tile"])
    assert h.pairs.tolist() == [[0, 1], [3, 4], [1, 2], [0, 2]] and h.flag.tolist() == [1, 1, 0, 0]
    assert (h.positive_pair_number, h.negative_pair_number) == (2, 2)
    assert h.poly_off.tolist() == [0, 2, 4, 6, 7, 10] and h.poly_pts.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert h.pt_tile.tolist() == [0] * 6 + [1] * 4
    assert h.max_windows == [8, 20, 32]
    gt = (1000.0, 0.5, 0.0, 2000.0, 0.0, -0.5)                     # map coordinates -> pixels like MyUtils1.py:67-73
    c = dict(a)
    del c["xy"]
    c["geo"], c["geotransform"] = np.stack((1000.0 + 0.5 * a["xy"][:, 0], 2000.0 - 0.5 * a["xy"][:, 1]), 1), gt
    assert np.array_equal(build_host([c]).pt_xy, a["xy"] + 1)


def test_host_validation_errors():
    def bad(mutate, match, **kw):
        im = _image()
        mutate(im)
        with pytest.raises(ValueError, match=match):
            build_host([_image(), im], **kw)
    bad(lambda im: im.update(positive=np.array([[0, 3]])), r"image 1, positive pair 0 \(0, 3\), right polygon 3: polygon id out of range")
    bad(lambda im: im.update(negative=np.array([[1, 2], [-1, 0]])), r"image 1, negative pair 1 .*left polygon -1: polygon id out of range")
    bad(lambda im: im["polygon_points"].__setitem__(1, ""), r"image 1, positive pair 0 \(0, 1\), right polygon 1: the polygon has no sample points")
    bad(lambda im: im["polygon_points"].__setitem__(2, [4, 6]), r"image 1, negative pair 0 .*polygon 2: point id 6 out of range")
    bad(lambda im: im["inner"].__setitem__(3, 0), r"image 1, .*point 3 has window side 0 at scale 0, outside 1..384")
    bad(lambda im: im["obj"].__setitem__(5, 200), r"point 5 has window side 392 at scale 2, outside 1..384")
    build_host([_image(), _image()], n_scales=3)
    big = _image()
    big["obj"][5] = 200
    build_host([big], n_scales=2)                                   # 392 is only the third scale's side
    bad(lambda im: im["obj"].__setitem__(5, 140), r"window side 404 at scale 3", n_scales=4)
    with pytest.raises(ValueError, match="empty dataset"):
        e = _image()
        e["positive"], e["negative"] = np.zeros((0, 2)), np.zeros((0, 2))
        build_host([e])


def test_epoch_lr_matches_torch_multistep_fresh_and_resumed():
    """Fresh run and a resume across a milestone: the lr of each epoch equals torch.optim.Adam + MultiStepLR, with the resumed
    optimizer restored through load_state_dict and a NEW scheduler (Train_SMT.py:192-197, :351)."""
    for lr_init, milestones in ((1e-4, (40, 80)), (1e-3, (40, 80)), (3e-4, (2, 4)), (0.01, (3, 3, 6))):
        p = [torch.nn.Parameter(torch.zeros(2))]
        opt = torch.optim.Adam(p, lr=lr_init)
        sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=list(milestones), gamma=0.2)
        ref = []
        for epoch in range(100):
            ref.append(opt.param_groups[0]["lr"])
            opt.step(); sch.step()
            if epoch == 4:
                saved = opt.state_dict()
        assert [Train_SMT.epoch_lr(lr_init, e, milestones, 0.2) for e in range(100)] == ref
        # resume from the checkpoint written after epoch index 4: start_epoch 5, milestones counted again from there
        opt2 = torch.optim.Adam(p, lr=lr_init)
        sch2 = torch.optim.lr_scheduler.MultiStepLR(opt2, milestones=list(milestones), gamma=0.2)
        opt2.load_state_dict(saved)
        lr0 = opt2.param_groups[0]["lr"]
        got = []
        for epoch in range(5, 100):
            got.append(opt2.param_groups[0]["lr"])
            opt2.step(); sch2.step()
        assert [Train_SMT.epoch_lr(lr0, e - 5, milestones, 0.2) for e in range(5, 100)] == got


def test_checkpoint_cadence_and_names():
    t = time.struct_time((2026, 3, 7, 9, 5, 0, 5, 66, 0))
    assert Train_SMT.checkpoint_name(4, 100, "S2Former_v3-3CH-3DP-SEF-642", t) == "model-2026-3-7_9-5_5epochs.pth"
    assert Train_SMT.checkpoint_name(89, 100, "S2Former_v3-3CH-3DP-SEF-642", t) == "model-2026-3-7_9-5_90epochs.pth"
    assert Train_SMT.checkpoint_name(99, 100, "S2Former_v3-3CH-3DP-SEF-642", t) == "model-2026-3-7_9-5-S2Former_v3-3CH-3DP-SEF-642_100epochs.pth"
    assert [e for e in range(100) if Train_SMT.checkpoint_due(e)] == [4, 9, 14, 19, 24, 29, 34, 39, 44, 49, 54, 59, 64, 69, 74, 79, 84] + list(range(89, 100))


def test_train_refuses_without_a_dataset_or_with_several_ranks(monkeypatch):
    with pytest.raises(ValueError, match="dataset"):
        Train_SMT.train(torch.nn.Linear(2, 2), 1.0, 4, 1e-4, 0.0, 0.0, 0.1, 0)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError):
        Train_SMT.train(torch.nn.Linear(2, 2), 1.0, 4, 1e-4, 0.0, 0.0, 0.1, 0, dataset=object())
    assert Train_SMT.Euclidean_distance is not None
