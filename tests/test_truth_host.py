"""CPU: the overlap / pair-flag / partition-score rule (tests/truth_ref.py, the spec of rag.label_overlap, rag.pair_flags,
Overlap.coarsen and Overlap.scores) -- known answers on hand-drawn rasters, the sparse spec against its dense brute force, the
scores against an O(n^2) pair count, that the dataset builder accepts what the spec chain produces -- and the library's side
without a GPU: header / SIGNATURES / exported symbols, argument validation."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import points_ref as P
import truth_ref as T


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    from oracle import sweep as OS
    strict = os.path.join(os.path.dirname(os.path.abspath(OS.__file__)), "_ref", "liboracle_sweep.so")
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(strict):
        g.build()
    return _lib


def rows_raster(*rows):
    return np.array(rows, np.int32)


def assert_same(a, b):
    for k in T.FIELDS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


# ---- the rule on hand-drawn rasters -------------------------------------------------------------------------------------------
def test_four_by_six_two_regions_two_objects():
    lab = rows_raster([0, 0, 0, 1, 1, 1], [0, 0, 0, 1, 1, 1], [0, 0, 0, 1, 1, 1], [0, 0, 0, 1, 1, 1])
    tru = rows_raster([0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 1, 1], [0, 0, 1, 1, 1, 1], [0, 0, 1, 1, 1, 1])
    ov = T.label_overlap(lab, tru, 2, 2)
    assert ov["cells"].tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]] and ov["count"].tolist() == [10, 2, 2, 10]
    assert ov["area"].tolist() == [12, 12] and ov["owner"].tolist() == [0, 1] and ov["owner_count"].tolist() == [10, 10]
    assert ov["size"].tolist() == [12, 12] and ov["cover"].tolist() == [10, 10]
    assert ov["summary"].tolist() == [24, 208, 288, 288, 20, 20, 2, 2]
    assert_same(ov, T.label_overlap_dense(lab, tru, 2, 2))
    for k, dt in (("cells", np.int32), ("count", np.int32), ("area", np.int64), ("owner", np.int32), ("owner_count", np.int32),
                  ("size", np.int64), ("cover", np.int32), ("summary", np.int64)):
        assert ov[k].dtype == dt, k
    # a third region id and a third object that never occur: empty rows / columns
    ov = T.label_overlap(lab, tru, 3, 3)
    assert ov["cells"].tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]] and ov["area"].tolist() == [12, 12, 0]
    assert ov["owner"].tolist() == [0, 1, -1] and ov["owner_count"].tolist() == [10, 10, 0] and ov["size"].tolist() == [12, 12, 0]
    assert ov["summary"].tolist() == [24, 208, 288, 288, 20, 20, 2, 2]


def test_a_tie_in_owner_goes_to_the_smaller_object_id():
    lab = rows_raster([0, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1])
    tru = rows_raster([2, 2, 2, 1, 1, 1, 0], [0, 2, 2, 2, 2, 1, 1])
    ov = T.label_overlap(lab, tru, 2, 3)
    assert ov["owner"].tolist() == [1, 2] and ov["owner_count"].tolist() == [3, 4]
    assert_same(ov, T.label_overlap_dense(lab, tru, 2, 3))


def purity_case():
    """Four regions of 10 pixels, one per row: 6/10, 5/10, 10/10 of object 0, and 10/10 of object 1."""
    lab = np.repeat(np.arange(4, dtype=np.int32)[:, None], 10, 1)
    tru = rows_raster([0] * 6 + [1] * 4, [0] * 5 + [1] * 4 + [2], [0] * 10, [1] * 10)
    return lab, tru


def test_purity_exactly_at_the_threshold_is_pure_and_one_pixel_fewer_is_not():
    lab, tru = purity_case()
    ov = T.label_overlap(lab, tru, 4, 3)
    assert ov["owner"].tolist() == [0, 0, 0, 1] and ov["owner_count"].tolist() == [6, 5, 10, 10] and ov["area"].tolist() == [10] * 4
    edges = np.array([[0, 2], [0, 1], [1, 2], [0, 3], [2, 3], [1, 3]], np.int32)
    assert T.purity_pm(0.6) == 600 and T.purity_pm(0.5996) == 600 and T.purity_pm(1.0) == 1000 and T.purity_pm(0) == 0
    assert T.pair_flags(edges, ov, 600).tolist() == [1, -1, -1, 0, 0, -1]       # 1000 * 6 == 600 * 10: pure; 1000 * 5 < 6000: not
    assert T.pair_flags(edges, ov, 601).tolist() == [-1, -1, -1, -1, 0, -1]
    assert T.pair_flags(edges, ov, 500).tolist() == [1, 1, 1, 0, 0, 0]
    assert T.pair_flags(edges, ov, 1000).tolist() == [-1, -1, -1, -1, 0, -1]
    assert T.pair_flags(edges, ov, 0).tolist() == [1, 1, 1, 0, 0, 0]
    assert T.pair_flags(edges, ov, 600).dtype == np.int8


def test_an_unlabelled_band_lowers_purity_through_the_area():
    lab = np.repeat(np.arange(3, dtype=np.int32)[:, None], 10, 1)
    tru = rows_raster([0] * 6 + [-1] * 4, [0] * 5 + [-1] * 3 + [7, 2], [0] * 10)     # 7 and 2 = G: not object ids
    ov = T.label_overlap(lab, tru, 3, 2)
    assert ov["cells"].tolist() == [[0, 0], [0, 2], [1, 0], [1, 2], [2, 0]] and ov["count"].tolist() == [6, 4, 5, 5, 10]
    assert ov["area"].tolist() == [10, 10, 10] and ov["owner_count"].tolist() == [6, 5, 10] and ov["size"].tolist() == [21, 0]
    assert ov["summary"].tolist() == [21, 36 + 25 + 100, 36 + 25 + 100, 441, 21, 10, 3, 1]
    # every labelled pixel of region 1 belongs to object 0, yet half its area is unlabelled: not pure at 0.6
    assert T.pair_flags([[0, 2], [1, 2]], ov, 600).tolist() == [1, -1]
    assert_same(ov, T.label_overlap_dense(lab, tru, 3, 2))


def test_an_edge_with_an_endpoint_outside_the_regions_is_ambiguous_and_such_pixels_are_ignored():
    lab, tru = purity_case()
    lab = lab.copy()
    lab[3, :4] = -1
    lab[3, 4:6] = 9
    ov = T.label_overlap(lab, tru, 4, 3)
    assert ov["area"].tolist() == [10, 10, 10, 4] and ov["summary"][0] == 34
    assert T.pair_flags([[-1, 2], [2, -1], [2, 4], [9, 0], [2, 3]], ov, 600).tolist() == [-1, -1, -1, -1, 0]
    assert_same(ov, T.label_overlap_dense(lab, tru, 4, 3))


@pytest.mark.parametrize("seed", range(4))
def test_sparse_spec_equals_the_dense_brute_force(seed):
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(1, 40)), int(rng.integers(1, 50))
    lab, S = P.voronoi_labels(H, W, int(rng.integers(3, 9)), seed)
    tru, G = P.voronoi_labels(H, W, int(rng.integers(6, 20)), seed + 10)
    lab[rng.random((H, W)) < 0.05] = -1
    lab[rng.random((H, W)) < 0.02] = S + 3
    tru[rng.random((H, W)) < 0.1] = -1
    tru[rng.random((H, W)) < 0.05] = G + 2
    assert_same(T.label_overlap(lab, tru, S + 1, G + 1), T.label_overlap_dense(lab, tru, S + 1, G + 1))


# ---- scores ---------------------------------------------------------------------------------------------------------------------
def product_scores(summary):
    from deepmerge_amd import rag
    s = rag.partition_scores(summary)
    ref = T.scores(summary)
    assert (s.n, s.sum_cells, s.sum_regions, s.sum_objects, s.sum_owner, s.sum_cover, s.n_regions, s.n_objects) == tuple(int(v) for v in summary)
    for k in ("asa", "coverage", "rand", "adjusted_rand"):
        a, b = getattr(s, k), ref[k]
        assert a == b or (math.isnan(a) and math.isnan(b)), k
    return s


def test_identical_partitions_score_one():
    lab, S = P.voronoi_labels(40, 50, 9, 3)
    s = product_scores(T.label_overlap(lab, lab, S, S)["summary"])
    assert s.rand == 1.0 and s.adjusted_rand == 1.0 and s.asa == 1.0 and s.coverage == 1.0
    assert s.n == 2000 and s.n_regions == s.n_objects == len(np.unique(lab))


def test_one_region_over_two_equal_objects():
    lab = np.zeros((6, 8), np.int32)
    tru = np.zeros((6, 8), np.int32)
    tru[:, 4:] = 1
    s = product_scores(T.label_overlap(lab, tru, 1, 2)["summary"])
    assert s.asa == 0.5 and s.coverage == 1.0 and s.n_regions == 1 and s.n_objects == 2
    assert s.adjusted_rand == 0.0 and s.rand == (2 * 24 * 23 // 2) / (48 * 47 // 2)
    # the other way round: two regions inside one object
    s = product_scores(T.label_overlap(tru, lab, 2, 1)["summary"])
    assert s.asa == 1.0 and s.coverage == 0.5


def test_rand_figures_equal_an_independent_pair_count():
    rng = np.random.default_rng(5)
    lab, S = P.voronoi_labels(12, 12, 4, 7)
    tru, G = P.voronoi_labels(12, 12, 6, 8)
    tru[rng.random((12, 12)) < 0.1] = -1
    lab[0, :3] = -1
    ov = T.label_overlap(lab, tru, S, G)
    s = product_scores(ov["summary"])
    c = T.pair_counts_brute(lab, tru, S, G)
    assert c["total"] == s.n * (s.n - 1) // 2 and 0 < c["both"] < c["same_region"] < c["total"]
    assert s.rand == float(Fraction(c["both"] + c["neither"], c["total"]))
    expected = Fraction(c["same_region"] * c["same_object"], c["total"])
    ari = (c["both"] - expected) / (Fraction(c["same_region"] + c["same_object"], 2) - expected)
    assert s.adjusted_rand == float(ari) and 0.0 < s.adjusted_rand < 1.0
    # asa / coverage from the dense table
    n = np.zeros((S, G), np.int64)
    keep = (lab >= 0) & (tru >= 0)
    np.add.at(n, (lab[keep], tru[keep]), 1)
    assert s.asa == n.max(1).sum() / n.sum() and s.coverage == n.max(0).sum() / n.sum()


def test_degenerate_summaries_give_nan_not_an_exception():
    s = product_scores([0, 0, 0, 0, 0, 0, 0, 0])
    assert all(math.isnan(v) for v in (s.asa, s.coverage, s.rand, s.adjusted_rand))
    s = product_scores([1, 1, 1, 1, 1, 1, 1, 1])
    assert s.asa == 1.0 and s.coverage == 1.0 and math.isnan(s.rand) and math.isnan(s.adjusted_rand)
    s = product_scores([2, 4, 4, 4, 2, 2, 1, 1])                   # two pixels, one region, one object
    assert s.rand == 1.0 and s.adjusted_rand == 1.0


def test_coarsen_equals_recomputing_on_the_relabelled_raster():
    rng = np.random.default_rng(9)
    lab, S = P.voronoi_labels(60, 70, 7, 1)
    tru, G = P.voronoi_labels(60, 70, 20, 2)
    tru[20:23, :] = -1
    lab[rng.random(lab.shape) < 0.02] = -1
    mapping = rng.integers(0, 12, S + 2)                           # ids S, S + 1 never occur
    mapping[S + 1] = 13                                            # C = 14: regions 12 and 13 stay empty
    ov = T.label_overlap(lab, tru, S + 2, G)
    merged = np.where(lab >= 0, mapping[np.maximum(lab, 0)], -1).astype(np.int32)
    want = T.label_overlap(merged, tru, 14, G)
    got = T.coarsen(ov, mapping)
    assert_same(got, want)
    assert got["n_labels"] == 14 and got["owner"][12:].tolist() == [-1, -1]
    assert_same(T.coarsen(ov, np.arange(S + 2)), ov)
    # the unlabelled column stays apart and column facts do not depend on the partition's granularity beyond `cover`
    assert np.array_equal(got["size"], ov["size"]) and (got["cover"] >= ov["cover"]).all()


# ---- the dataset builder takes what the spec chain produces -------------------------------------------------------------------------
def spec_image(H, W, cell, tcell, min_purity=0.6, k=3):
    from oracle import rag as OR
    lab, S = P.voronoi_labels(H, W, cell, 1)
    tru, G = P.voronoi_labels(H, W, tcell, 2)
    pts = P.sample_points(lab, S, k)
    edges, _ = OR.rag_edges(lab, S)
    flags = T.pair_flags(edges, T.label_overlap(lab, tru, S, G), T.purity_pm(min_purity))
    tile = np.random.default_rng(H).integers(0, 256, (3, H, W), dtype=np.uint8)
    return {"tile": tile, "labels": lab, "n_labels": S, "truth": tru, "n_truth": G, "xy": pts["xy"], "inner": pts["inner"], "obj": pts["obj"],
            "region": np.zeros((pts["xy"].shape[0], 15), np.float32), "label": pts["label"],
            "polygon_points": [np.arange(pts["ptr"][s], pts["ptr"][s + 1]) for s in range(S)],
            "positive": edges[flags == 1], "negative": edges[flags == 0], "edges": edges, "flags": flags}


def test_every_class_of_pair_is_populated_and_build_host_accepts_the_chain():
    from deepmerge_amd import dataset
    a, b = spec_image(257, 301, 13, 40), spec_image(96, 128, 9, 30)
    count = lambda im: [int((im["flags"] == v).sum()) for v in (1, 0, -1)]
    assert count(a) == [658, 312, 348] and count(b) == [232, 99, 100]
    host = dataset.build_host([a, b], n_scales=3)
    assert (host.positive_pair_number, host.negative_pair_number) == (658 + 232, 312 + 99)
    assert host.pairs.shape == (890 + 411, 2) and host.flag.tolist() == [1] * 890 + [0] * 411
    n_poly_a = a["n_labels"]
    want = np.concatenate((a["positive"], b["positive"] + n_poly_a, a["negative"], b["negative"] + n_poly_a))
    assert np.array_equal(host.pairs, want) and max(host.max_windows) <= dataset.MAX_WINDOW


def test_holdout_hash_is_fixed_and_spreads():
    from deepmerge_amd.dataset import holdout_hash
    a, b = np.arange(1000), np.arange(1000) + 1
    h = holdout_hash(3, 0, a, b)
    assert h.dtype == np.uint64 and np.array_equal(h, holdout_hash(3, 0, a, b)) and np.unique(h).size == 1000
    assert not np.array_equal(h, holdout_hash(4, 0, a, b)) and not np.array_equal(h, holdout_hash(3, 1, a, b))
    assert not np.array_equal(h, holdout_hash(3, 0, b, a))
    share = float((h % np.uint64(1000000) < np.uint64(250000)).mean())
    assert 0.2 < share < 0.3                                       # 1000 draws at p = 1/4: 0.25 +- 3.7 sigma
    m = (1 << 64) - 1                                              # the arithmetic, restated with Python integers
    k = (((3 * 0x9E3779B97F4A7C15) ^ (1 * 0xC2B2AE3D27D4EB4F)) & m) ^ ((5 << 32) | 6)
    for mul in (0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53):
        k = ((k ^ (k >> 33)) * mul) & m
    assert int(holdout_hash(3, 0, np.array([5]), np.array([6]))[0]) == k ^ (k >> 33)


# ---- the library's side, without a GPU ------------------------------------------------------------------------------------------
NEW = ("dm_label_overlap", "dm_overlap_reduce", "dm_pair_flags")


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
    for name, nargs in zip(NEW, (15, 14, 9)):
        proto = text[text.index("int " + name + "("):]
        proto = proto[:proto.index(";")]
        assert proto.count(",") + 1 == nargs == len(built.SIGNATURES[name][1]), name


def test_truth_entry_points_validate_before_any_launch(built):
    lib = built.lib()
    p = 4096                                                       # any non-null address: validation never dereferences
    ov = lambda *, labels=p, truth=p, H=8, W=8, S=4, G=3, log2=10, cells=p, max_cells=16, n=p: \
        lib.dm_label_overlap(labels, truth, H, W, S, G, p, p, log2, cells, p, max_cells, n, p, None)
    red = lambda *, keys=p, K=4, S=4, G=3, owner=p, summary=p: lib.dm_overlap_reduce(keys, p, K, S, G, p, p, p, owner, p, p, p, summary, None)
    fl = lambda *, edges=p, E=4, area=p, S=4, pm=600, flags=p: lib.dm_pair_flags(edges, E, area, p, p, S, pm, flags, None)
    cases = [
        (lambda: ov(labels=None), b"dm_label_overlap: null pointer"),
        (lambda: ov(truth=None), b"dm_label_overlap: null pointer"),
        (lambda: ov(n=None), b"dm_label_overlap: null pointer"),
        (lambda: ov(H=0), b"dm_label_overlap: bad sizes"),
        (lambda: ov(H=1 << 16, W=1 << 15), b"dm_label_overlap: bad sizes"),
        (lambda: ov(S=0), b"dm_label_overlap: bad sizes"),
        (lambda: ov(G=0), b"dm_label_overlap: bad sizes"),
        (lambda: ov(G=1 << 31), b"dm_label_overlap: bad sizes"),
        (lambda: ov(log2=31), b"dm_label_overlap: bad sizes"),
        (lambda: ov(max_cells=0), b"dm_label_overlap: bad sizes"),
        (lambda: ov(S=1 << 61, G=1), b"dm_label_overlap: key bound exceeded"),
        (lambda: ov(S=1 << 32, G=(1 << 30) - 1), b"dm_label_overlap: key bound exceeded"),
        (lambda: red(keys=None), b"dm_overlap_reduce: null pointer"),
        (lambda: red(owner=None), b"dm_overlap_reduce: null pointer"),
        (lambda: red(summary=None), b"dm_overlap_reduce: null pointer"),
        (lambda: red(K=-1), b"dm_overlap_reduce: bad sizes"),
        (lambda: red(S=0), b"dm_overlap_reduce: bad sizes"),
        (lambda: red(G=1 << 31), b"dm_overlap_reduce: bad sizes"),
        (lambda: red(S=1 << 61, G=1), b"dm_overlap_reduce: key bound exceeded"),
        (lambda: fl(area=None), b"dm_pair_flags: null pointer"),
        (lambda: fl(edges=None), b"dm_pair_flags: null pointer"),
        (lambda: fl(flags=None), b"dm_pair_flags: null pointer"),
        (lambda: fl(E=-1), b"dm_pair_flags: bad sizes"),
        (lambda: fl(S=0), b"dm_pair_flags: bad sizes"),
        (lambda: fl(pm=1001), b"dm_pair_flags: purity_pm = 1001 outside 0..1000"),
        (lambda: fl(pm=-1), b"dm_pair_flags: purity_pm = -1 outside 0..1000"),
    ]
    for call, msg in cases:
        assert call() == -1, msg
        assert msg in lib.dm_last_error(), (msg, lib.dm_last_error())


def test_overlap_has_no_cpu_fallback_and_checks_its_arguments_on_the_host(built):
    import torch
    from deepmerge_amd import rag
    from deepmerge_amd.dataset import PairDataset
    lab = torch.zeros((8, 8), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag.label_overlap(lab, lab, 1, 1)
    ov = rag.Overlap(cells=torch.zeros((1, 2), dtype=torch.int32), count=torch.ones(1, dtype=torch.int32), area=torch.ones(1, dtype=torch.int64),
                     owner=torch.zeros(1, dtype=torch.int32), owner_count=torch.ones(1, dtype=torch.int32), size=torch.ones(1, dtype=torch.int64),
                     cover=torch.ones(1, dtype=torch.int32), summary=torch.tensor([64, 4096, 4096, 4096, 64, 64, 1, 1]), n_labels=1, n_truth=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag.pair_flags(torch.zeros((1, 2), dtype=torch.int32), ov)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ov.coarsen(torch.zeros(1, dtype=torch.int32))
    s = ov.scores()                                                # pure host arithmetic on the eight integers
    assert s.n == 64 and s.asa == 1.0 and s.adjusted_rand == 1.0
    with pytest.raises(ValueError, match="holdout"):
        PairDataset.from_rasters([], holdout=1.0)
