"""GPU: rag.slic / rag.connected_labels (csrc/dm_slic.hip) against the numpy spec tests/slic_ref.py -- labels and counts are
bit-equal -- and the two chains that start from them: FeatureIO.segment_tile and PairDataset.from_rasters without `labels`."""
import numpy as np
import pytest
import torch

import points_ref as P
import slic_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def image(kind, bands, H, W, seed=0):
    if kind == "constant":
        return np.full((bands, H, W), 93, np.uint8)
    if kind == "noise":
        return R.noise_image(bands, H, W, seed)
    return R.block_image(bands, H, W, 37, seed)


CASES = {  # kind, bands, H, W, cell, compactness, iters, min_size
    "vec_3_bands": ("blocks", 3, 96, 128, 8, 10, 3, None),                 # W % 16 == 0: the 16-byte loads and stores
    "odd_4_bands": ("blocks", 4, 257, 301, 13, 10, 3, None),               # no multiple of the tile, odd width
    "odd_1_band": ("blocks", 1, 257, 301, 13, 10, 3, None),
    "odd_2_bands": ("blocks", 2, 257, 301, 13, 10, 2, None),
    "odd_5_bands": ("blocks", 5, 257, 301, 13, 10, 3, None),               # only four are used
    "one_pixel": ("noise", 3, 1, 1, 4, 10, 2, None),
    "flat_wide": ("noise", 3, 5, 700, 8, 10, 2, None),
    "flat_tall": ("noise", 3, 700, 6, 8, 10, 2, None),
    "one_centre": ("blocks", 3, 33, 17, 40, 10, 2, None),
    "most_centres": ("blocks", 3, 130, 130, 4, 10, 3, None),               # 18 x 18 centres staged per tile
    "wide_distance": ("blocks", 4, 130, 130, 129, 255, 2, None),           # cell^2 (4 * 255^2 + 18 * 255^2) > 2^32: 64-bit D
    "wide_distance_vec": ("noise", 4, 144, 160, 130, 200, 2, 50),
    "compactness_0": ("blocks", 3, 96, 128, 11, 0, 3, None),
    "compactness_255": ("blocks", 3, 96, 128, 11, 255, 3, None),
    "iters_0": ("blocks", 3, 131, 150, 11, 10, 0, None),
    "iters_1": ("blocks", 3, 131, 150, 11, 10, 1, None),
    "min_size_1": ("blocks", 3, 131, 150, 11, 10, 2, 1),                   # no absorption
    "min_size_huge": ("blocks", 3, 131, 150, 6, 10, 2, 4 * 36),            # many rounds
    "constant": ("constant", 3, 131, 150, 9, 10, 2, None),                 # all ties
    "noise": ("noise", 4, 257, 301, 13, 10, 2, None),                      # tens of thousands of fragments
    "defaults": ("blocks", 3, 200, 260, 29, 10, 10, None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_slic_equals_the_spec(name):
    from deepmerge_amd import rag
    kind, bands, H, W, cell, comp, iters, min_size = CASES[name]
    tile = image(kind, bands, H, W, seed=len(name))
    want, n_want, rounds = R.slic(tile, cell, comp, iters, min_size, return_rounds=True)
    t = dev(tile)
    # the stages first, so that a mismatch names the kernel
    assigned, centres = rag.slic_assign(t, cell, comp, iters)
    lab_ref, centres_ref = R.iterate(tile, cell, comp, iters)
    frag_ref, n_frag = R.connected_labels(lab_ref)
    print(f"{name}: K = {centres_ref.shape[0]}, fragments = {n_frag}, n = {n_want}, absorption rounds = {rounds}")
    assert np.array_equal(centres.cpu().numpy(), centres_ref.astype(np.int32)), "centres"
    assert np.array_equal(assigned.cpu().numpy(), lab_ref.astype(np.int32)), "assignment"
    frag, n = rag.connected_labels(assigned)
    assert n == n_frag and np.array_equal(frag.cpu().numpy(), frag_ref), "components"
    labels, n = rag.slic(t, cell=cell, compactness=comp, iters=iters, min_size=min_size)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (H, W)
    assert n == n_want and np.array_equal(labels.cpu().numpy(), want)
    assert torch.equal(t.cpu(), torch.from_numpy(tile))            # the input is not modified
    if name == "noise":
        assert n_frag > 20000
    if name == "min_size_1":
        assert rounds == 0
    if name == "min_size_huge":
        assert rounds >= 2


def test_two_runs_are_identical_and_defaults_are_the_documented_ones():
    from deepmerge_amd import rag
    tile = R.noise_image(3, 257, 301, 9)
    t = dev(tile)
    a, na = rag.slic(t, cell=13)
    b, nb = rag.slic(t, cell=13, compactness=10, iters=10, min_size=13 * 13 // 4)
    assert na == nb and torch.equal(a, b)
    area = torch.bincount(a.reshape(-1).long(), minlength=na)
    assert int(area.min()) >= 13 * 13 // 4 and torch.equal(rag.label_area(a, na).long(), area)


def test_slic_rejects_bad_arguments():
    from deepmerge_amd import rag
    t = torch.zeros((3, 16, 16), dtype=torch.uint8, device=DEV)
    for bad in (t.float(), t[0], torch.zeros((3, 0, 16), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError, match="tile must be uint8"):
            rag.slic(bad)
    for kw, msg in (({"cell": 3}, "cell"), ({"cell": 257}, "cell"), ({"compactness": -1}, "compactness"), ({"compactness": 256}, "compactness"),
                    ({"iters": -1}, "iters"), ({"min_size": 0}, "min_size")):
        with pytest.raises(ValueError, match=msg):
            rag.slic(t, **kw)
    r = torch.zeros((4, 4), dtype=torch.int32, device=DEV)
    for bad in (r.long(), r[0], r[:0]):
        with pytest.raises(ValueError, match="raster must be int32"):
            rag.connected_labels(bad)
    with pytest.raises(ValueError, match="background"):
        rag.connected_labels(r, background=1 << 31)


def class_raster(H, W, seed, values=3):
    return np.random.default_rng(seed).integers(0, values, (H, W)).astype(np.int32)


RASTERS = {  # raster, background
    "serpentine": (lambda: R.serpentine(130, 130), None),                  # one path that crosses every tile border many times
    "serpentine_background": (lambda: R.serpentine(130, 130), 0),
    "serpentine_columns": (lambda: np.ascontiguousarray(R.serpentine(130, 130).T), None),
    "checkerboard": (lambda: (np.indices((130, 130)).sum(0) % 2).astype(np.int32), None),      # H*W components
    "checkerboard_vec": (lambda: (np.indices((66, 144)).sum(0) % 2).astype(np.int32), None),
    "single_value": (lambda: np.full((131, 70), -5, np.int32), None),
    "all_background": (lambda: np.full((70, 131), -5, np.int32), -5),
    "classes": (lambda: class_raster(257, 301, 1), None),
    "classes_background": (lambda: class_raster(257, 301, 2), 1),
    "classes_vec": (lambda: class_raster(192, 256, 3, values=2), None),
    "blobs_negative_background": (lambda: (P.voronoi_labels(200, 170, 31, 4)[0] % 3 - 1).astype(np.int32), -1),
    "one_pixel": (lambda: np.zeros((1, 1), np.int32), None),
    "one_row": (lambda: class_raster(1, 500, 5, values=2), None),
    "one_column": (lambda: class_raster(500, 1, 6, values=2), 0),
}


@pytest.mark.parametrize("name", list(RASTERS))
def test_connected_labels_equals_the_spec(name):
    from deepmerge_amd import rag
    make, background = RASTERS[name]
    r = make()
    want, n_want = R.connected_labels(r, background)
    t = dev(r)
    got, n = rag.connected_labels(t, background)
    assert got.dtype == torch.int32 and n == n_want and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(t.cpu(), torch.from_numpy(r))
    again, m = rag.connected_labels(t, background)
    assert m == n and torch.equal(again, got)
    if name == "checkerboard":
        assert n == r.size
    if name == "serpentine":
        assert n < 80 and (want[r == 1] == 0).all()                # the path is ONE component, the first in scan order


def test_segment_tile_equals_slic_then_merge_tile():
    from deepmerge_amd import rag
    from deepmerge_amd.ExtractFeatures import FeatureIO
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    torch.manual_seed(1)
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, (3, 4, 4)).astype(np.uint8)        # coarse colour blocks + noise, as the merge_tile test uses
    tile = np.clip(np.kron(base, np.ones((64, 64), np.uint8)).astype(np.int64) + rng.integers(-8, 9, (3, 256, 256)), 0, 255).astype(np.uint8)
    tt = dev(tile)
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=[32, 64, 128], depth=[1, 1, 1], in_c=3, numerics="fp32")
    fio = FeatureIO(net, None, DEV)
    kw = dict(cell=23, compactness=12, iters=4, min_size=100)
    labels, S = rag.slic(tt, **kw)
    want_labels, want_S = R.slic(tile, **kw)
    assert S == want_S and np.array_equal(labels.cpu().numpy(), want_labels)
    want, wpts = fio.merge_tile(tt, labels, S, k=3, margin=1.0, batch_size=100, max_rounds=3)
    got, gpts, glabels, gS = fio.segment_tile(tt, k=3, margin=1.0, batch_size=100, max_rounds=3, **kw)
    assert gS == S and torch.equal(glabels, labels)
    for f in ("xy", "label", "inner", "obj", "ptr", "idx", "bbox", "round"):
        assert torch.equal(getattr(gpts, f), getattr(wpts, f)), f
    for f in ("region_of", "ptr", "idx", "edges", "weights", "rep", "history"):
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    for f in ("pooled", "simi", "history_simi"):
        assert torch.equal(getattr(got, f).view(torch.int32), getattr(want, f).view(torch.int32)), f
    for key in ("count", "sum", "sumsq", "bbox", "peri"):
        assert torch.equal(got.stats[key], want.stats[key]), key
    assert (got.rounds, got.regions_per_round, got.merges_per_round) == (want.rounds, want.regions_per_round, want.merges_per_round)
    assert got.regions_per_round[0] == S


def test_from_rasters_without_labels_segments_with_slic():
    from deepmerge_amd import rag
    from deepmerge_amd.dataset import PairDataset
    images = []
    for H, W, seed in ((96, 128, 1), (120, 100, 2)):
        truth, G = P.voronoi_labels(H, W, 30, seed)
        rng = np.random.default_rng(seed)
        colour = rng.integers(8, 248, (3, G))                      # the image follows the truth: superpixels are mostly pure
        tile = (colour[:, truth] + rng.integers(-8, 9, (3, H, W))).astype(np.uint8)
        images.append({"tile": tile, "truth": truth, "n_truth": G, "slic": {"cell": 9, "iters": 3}})
    with_labels = []
    for im in images:
        labels, S = rag.slic(dev(im["tile"]), **im["slic"])
        with_labels.append({"tile": im["tile"], "truth": im["truth"], "n_truth": im["n_truth"], "labels": labels, "n_labels": S})
    got = PairDataset.from_rasters(images, k=3, seed=5, device=DEV)
    want = PairDataset.from_rasters(with_labels, k=3, seed=5, device=DEV)
    assert len(got) == len(want) > 50 and got.positive_pair_number > 0 and got.negative_pair_number > 0
    for f in ("tiles", "pairs", "flag", "poly_off", "poly_pts", "pt_tile", "pt_xy", "pt_inner", "pt_obj", "pt_region"):
        assert np.array_equal(getattr(got.host, f), getattr(want.host, f)), f
