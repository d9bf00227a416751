"""CPU: the point-sampling rule (tests/points_ref.py, the spec of rag.clearance / rag.sample_points) -- known answers on
hand-drawn rasters, the 8-neighbour-boundary identity against the brute-force definition, that the dataset builder accepts what
the rule produces -- and the library's side without a GPU: header / SIGNATURES / exported symbols, argument validation."""
import os

import numpy as np
import pytest

import points_ref as R


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    from oracle import sweep as OS
    strict = os.path.join(os.path.dirname(os.path.abspath(OS.__file__)), "_ref", "liboracle_sweep.so")
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(strict):
        g.build()
    return _lib


def block_raster(H, W, y0, x0, h, w):
    """Superpixel 1 = an h x w block at (y0, x0) on a background of superpixel 0."""
    lab = np.zeros((H, W), np.int32)
    lab[y0:y0 + h, x0:x0 + w] = 1
    return lab


def test_five_by_five_block_is_sampled_at_its_centre():
    lab = block_raster(11, 12, 3, 4, 5, 5)
    c = R.clearance(lab)
    assert np.array_equal(c, R.clearance_brute(lab))
    assert c[5, 6] == 3 and R.clearance_at(lab, 5, 6) == 3
    assert np.array_equal(c[3:8, 4:9], [[1, 1, 1, 1, 1], [1, 2, 2, 2, 1], [1, 2, 3, 2, 1], [1, 2, 2, 2, 1], [1, 1, 1, 1, 1]])
    r = R.sample_points(lab, 2, k=1)
    at = r["ptr"][1]
    assert r["ptr"].tolist() == [0, 1, 2] and r["xy"][at].tolist() == [6, 5] and r["inner"][at] == 5 and r["obj"][at] == 5
    assert r["label"].tolist() == [0, 1] and r["round"].tolist() == [0, 0] and r["bbox"][1].tolist() == [4, 3, 8, 7]
    assert r["idx"].tolist() == [0, 1]


def test_one_pixel_wide_strip_has_clearance_one_and_lines_its_points_up():
    """On a one-pixel-wide strip c = 1 everywhere, so score_j = min(c, distance) is 1 on every pixel not yet chosen and the tie
    rule decides: the points are the strip's first k pixels in linear order.  (The rule as specified cannot spread points along a
    strip of clearance 1; it does from clearance 2 on, second half of this test.)"""
    lab = block_raster(5, 21, 2, 2, 1, 17)                       # superpixel 1: row 2, x = 2..18
    c = R.clearance(lab)
    assert (c[2, 2:19] == 1).all() and np.array_equal(c, R.clearance_brute(lab))
    r = R.sample_points(lab, 2, k=3)
    mine = slice(r["ptr"][1], r["ptr"][2])
    # round 0: all scores 1, the smallest linear index; round 1: scores min(1, distance) = 1 everywhere else, again the smallest
    # index: clearance 1 cannot tell far from near, so a strip's points line up from its first pixel
    assert r["xy"][mine].tolist() == [[2, 2], [3, 2], [4, 2]]
    assert r["inner"][mine].tolist() == [1, 1, 1] and r["obj"][mine].tolist() == [17, 17, 17] and r["round"][mine].tolist() == [0, 1, 2]
    # a 3-pixel-wide strip has clearance 2 on its middle row: there the later points do move away from the first
    lab3 = block_raster(9, 25, 3, 2, 3, 21)                      # rows 3..5, x = 2..22
    r3 = R.sample_points(lab3, 2, k=3)
    mine = slice(r3["ptr"][1], r3["ptr"][2])
    assert r3["xy"][mine].tolist() == [[3, 4], [5, 4], [7, 4]] and r3["inner"][mine].tolist() == [3, 3, 3]


def test_two_pixel_superpixel_with_k_3_gets_two_points_and_a_missing_id_none():
    lab = np.zeros((6, 7), np.int32)
    lab[2, 3] = lab[2, 4] = 2                                     # id 1 and id 3 never occur
    r = R.sample_points(lab, 4, k=3)
    assert np.diff(r["ptr"]).tolist() == [3, 0, 2, 0]
    mine = slice(r["ptr"][2], r["ptr"][3])
    assert r["xy"][mine].tolist() == [[3, 2], [4, 2]] and r["round"][mine].tolist() == [0, 1]
    assert r["inner"][mine].tolist() == [1, 1] and r["obj"][mine].tolist() == [2, 2]
    assert r["bbox"][1].tolist() == [R.INT_MAX, R.INT_MAX, -1, -1] and r["bbox"][2].tolist() == [3, 2, 4, 2]
    assert len(set(map(tuple, r["xy"].tolist()))) == r["xy"].shape[0]       # no duplicates


def test_ties_go_to_the_smaller_linear_index():
    lab = block_raster(8, 9, 2, 2, 4, 4)                          # 4 x 4 block: four centre pixels of clearance 2
    c = R.clearance(lab)
    assert (c[3:5, 3:5] == 2).all() and c.max() == 2
    r = R.sample_points(lab, 2, k=4)
    mine = slice(r["ptr"][1], r["ptr"][2])
    assert r["xy"][mine][0].tolist() == [3, 3]                   # y*W + x smallest among (3,3), (4,3), (3,4), (4,4)
    # round 1: every other pixel scores 1 (adjacent to the point or clearance 1) except none at 2 -> smallest linear index of score 1
    assert r["xy"][mine][1].tolist() == [2, 2]


def test_cap_on_one_label_filling_the_raster():
    lab = np.zeros((400, 400), np.int32)
    c = R.clearance(lab)
    assert c.max() == 192 and R.clearance_at(lab, 200, 200) == 192 and R.clearance_at(lab, 191, 191) == 192
    assert R.clearance_at(lab, 190, 200) == 191 and c[190, 200] == 191 and c[190, 300] == 100
    r = R.sample_points(lab, 1, k=2, clr=c)
    assert r["xy"][0].tolist() == [191, 191]                      # the first pixel at the cap
    assert r["inner"][0] == 383 and r["obj"][0] == 383 and 3 * r["obj"][0] - 2 * r["inner"][0] <= 384
    assert ((3 * r["obj"].astype(np.int64) - 2 * r["inner"]) <= 384).all() and (r["inner"] <= r["obj"]).all()
    small = R.sample_points(lab, 1, k=1, max_window=31)
    assert small["inner"][0] == 31 and small["obj"][0] == 31 and R.clearance(lab, 31).max() == 16


@pytest.mark.parametrize("seed", range(6))
def test_boundary_identity_equals_the_brute_force_definition(seed):
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    if seed % 2:
        lab, _ = R.voronoi_labels(H, W, int(rng.integers(3, 12)), seed)
        lab[rng.random((H, W)) < 0.02] = -1                       # ids out of range are labels like any other here
    else:
        lab = rng.integers(0, 3, (H // 4 + 1, W // 4 + 1)).astype(np.int32).repeat(4, 0).repeat(4, 1)[:H, :W]
    for mw in (384, 31, 5, 1):
        assert np.array_equal(R.clearance(lab, mw), R.clearance_brute(lab, mw)), (H, W, mw)
    big = np.zeros((70, 90), np.int32)
    big[10:60, 5:80] = 7
    assert np.array_equal(R.clearance(big, 384), R.clearance_brute(big, 384)) and R.clearance(big, 384).max() == 25


def test_spec_properties_on_a_voronoi_raster():
    lab, S = R.voronoi_labels(150, 170, 13, 4)
    lab[40:43, 50:90] = S + 5                                     # out of range: never sampled, another label to its neighbours
    r = R.sample_points(lab, S + 2, k=3)
    area = np.bincount(lab[(lab >= 0) & (lab < S + 2)], minlength=S + 2)
    assert np.array_equal(np.diff(r["ptr"]), np.minimum(3, area))
    assert np.array_equal(lab[r["xy"][:, 1], r["xy"][:, 0]], r["label"])
    assert (r["inner"] >= 1).all() and (r["inner"] <= r["obj"]).all() and ((3 * r["obj"] - 2 * r["inner"]) <= 384).all()
    for (x, y), i, s in zip(r["xy"], r["inner"], r["label"]):
        h = i // 2
        assert (lab[y - h:y + h + 1, x - h:x + h + 1] == s).all() and lab[y - h:y + h + 1, x - h:x + h + 1].shape == (i, i)


def test_dataset_builder_accepts_the_points_the_rule_produces():
    from deepmerge_amd import dataset
    lab, S = R.voronoi_labels(96, 128, 17, 2)
    big = np.zeros((400, 400), np.int32)
    images = []
    for labels, n in ((lab, S), (big, 1)):
        r = R.sample_points(labels, n, k=3)
        polys = [list(range(r["ptr"][s], r["ptr"][s + 1])) for s in range(n)]
        occupied = [s for s in range(n) if polys[s]]
        pairs = [(occupied[0], occupied[-1])] if len(occupied) > 1 else [(0, 0)]
        images.append({"tile": np.zeros((3,) + labels.shape, np.uint8), "xy": r["xy"], "inner": r["inner"], "obj": r["obj"],
                       "region": np.zeros((r["xy"].shape[0], 15), np.float32), "polygon_points": polys, "positive": pairs})
    host = dataset.build_host(images, n_scales=4)
    assert host.pt_xy.shape[0] == sum(im["xy"].shape[0] for im in images) and max(host.max_windows) <= dataset.MAX_WINDOW
    w = dataset.window_sides(np.concatenate([im["inner"] for im in images]), np.concatenate([im["obj"] for im in images]), 4)
    assert w.min() >= 1 and w.max() <= dataset.MAX_WINDOW


# ---- the library's side, without a GPU ------------------------------------------------------------------------------------------
NEW = ("dm_label_clearance", "dm_point_select_round", "dm_point_emit")


def test_header_signatures_and_exports_agree_and_abi_is_still_6(built):
    import ctypes
    lib = built.lib()
    assert lib.dm_abi_version() == 7
    declared = built.declared_symbols()
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW:
        assert name in declared and name in built.SIGNATURES and hasattr(raw, name), name
    assert sorted(built.SIGNATURES) == declared
    text = open(built.HEADER_PATH).read()
    for name, nargs in zip(NEW, (8, 13, 15)):
        proto = text[text.index("int " + name + "("):]
        proto = proto[:proto.index(";")]
        assert proto.count(",") + 1 == nargs == len(built.SIGNATURES[name][1]), name


def test_point_entry_points_validate_before_any_launch(built):
    lib = built.lib()
    p = 4096                                                       # any non-null address: validation never dereferences
    cases = [
        (lambda: lib.dm_label_clearance(None, 8, 8, 384, p, p, p, None), b"dm_label_clearance: null pointer"),
        (lambda: lib.dm_label_clearance(p, 8, 8, 384, p, None, p, None), b"dm_label_clearance: null pointer"),
        (lambda: lib.dm_label_clearance(p, 0, 8, 384, p, p, p, None), b"dm_label_clearance: bad sizes"),
        (lambda: lib.dm_label_clearance(p, 1 << 16, 1 << 15, 384, p, p, p, None), b"dm_label_clearance: bad sizes"),
        (lambda: lib.dm_label_clearance(p, 8, 8, 0, p, p, p, None), b"max_window = 0 outside 1..384"),
        (lambda: lib.dm_label_clearance(p, 8, 8, 385, p, p, p, None), b"max_window = 385 outside 1..384"),
        (lambda: lib.dm_point_select_round(p, None, 8, 8, 4, 3, 0, p, p, p, p, p, None), b"dm_point_select_round: null pointer"),
        (lambda: lib.dm_point_select_round(p, p, 8, 8, 4, 3, 0, p, p, p, p, None, None), b"dm_point_select_round: null pointer"),
        (lambda: lib.dm_point_select_round(p, p, 8, -1, 4, 3, 0, p, p, p, p, p, None), b"dm_point_select_round: bad sizes"),
        (lambda: lib.dm_point_select_round(p, p, 8, 8, 0, 3, 0, p, p, p, p, p, None), b"dm_point_select_round: bad sizes"),
        (lambda: lib.dm_point_select_round(p, p, 8, 8, 4, 0, 0, p, p, p, p, p, None), b"k = 0 outside 1..16"),
        (lambda: lib.dm_point_select_round(p, p, 8, 8, 4, 17, 0, p, p, p, p, p, None), b"k = 17 outside 1..16"),
        (lambda: lib.dm_point_select_round(p, p, 8, 8, 4, 3, 3, p, p, p, p, p, None), b"round = 3 outside"),
        (lambda: lib.dm_point_emit(p, p, p, None, 4, 3, 384, 12, p, p, p, p, p, p, None), b"dm_point_emit: null pointer"),
        (lambda: lib.dm_point_emit(p, p, p, p, 0, 3, 384, 12, p, p, p, p, p, p, None), b"dm_point_emit: bad sizes"),
        (lambda: lib.dm_point_emit(p, p, p, p, 4, 3, 384, 0, p, p, p, p, p, p, None), b"dm_point_emit: bad sizes"),
        (lambda: lib.dm_point_emit(p, p, p, p, 4, 17, 384, 12, p, p, p, p, p, p, None), b"k = 17 outside 1..16"),
        (lambda: lib.dm_point_emit(p, p, p, p, 4, 3, 400, 12, p, p, p, p, p, p, None), b"max_window = 400 outside 1..384"),
    ]
    for call, msg in cases:
        assert call() == -1, msg
        assert msg in lib.dm_last_error(), (msg, lib.dm_last_error())


def test_point_sampling_has_no_cpu_fallback_and_checks_its_arguments_on_the_host(built):
    import torch
    from deepmerge_amd import rag
    lab = torch.zeros((8, 8), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag.clearance(lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag.sample_points(lab, 1)
    ps = rag.PointSamples(xy=torch.zeros((2, 2), dtype=torch.int32), label=torch.tensor([1, 0], dtype=torch.int32), inner=None, obj=None,
                          ptr=None, idx=None, bbox=torch.zeros((2, 4), dtype=torch.int32), round=None)
    designed = torch.arange(30, dtype=torch.float32).reshape(2, 15)
    assert torch.equal(ps.region_features(designed), designed[[1, 0]])
    with pytest.raises(ValueError, match="designed must be"):
        ps.region_features(designed[:1])
