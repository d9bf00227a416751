"""CPU: the boundary-score rule (include/deepmerge_hip.h).  The numpy spec tests/boundary_ref.py against a
brute-force double loop and against hand cases whose counts are written out here; the library's argument errors, which need no GPU."""
import math

import numpy as np
import pytest

import boundary_ref as B


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


# ---- the spec against the rule pixel by pixel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_spec_equals_the_double_loop(seed):
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(1, 10)), int(rng.integers(1, 12))                # up to 9 x 11
    S, G = 5, 3
    coarse = lambda n, lo, hi: np.kron(rng.integers(lo, hi, ((H + n - 1) // n, (W + n - 1) // n)), np.ones((n, n), np.int64))[:H, :W]
    labels = coarse(2, -1, S + 2).astype(np.int32)                           # ids -1, S and S + 1 are out of range
    truth = coarse(3, -2, G + 1).astype(np.int32)
    mapping = rng.integers(0, 3, S).astype(np.int32)
    y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
    box = (y0, int(rng.integers(y0 + 1, H + 1)), x0, int(rng.integers(x0 + 1, W + 1)))
    for d in (0, 1, 2, 5, 12):
        for m in (None, mapping):
            for b in (None, box):
                assert B.counts(labels, truth, S, G, d, m, b) == B.brute(labels, truth, S, G, d, m, b), (seed, d, m is None, b)


def test_counts_of_disjoint_boxes_add():
    labels, S, truth, G = B.scene_pair(40, 50)
    whole = B.counts(labels, truth, S, G, 3)
    parts = [B.counts(labels, truth, S, G, 3, box=(y, min(40, y + 17), x, min(50, x + 21))) for y in range(0, 40, 17) for x in range(0, 50, 21)]
    assert whole == tuple(sum(p[i] for p in parts) for i in range(4))


# ---- hand cases ----------------------------------------------------------------------------------------------------------------------
def halves(H, W, x):
    """0 left of column x, 1 from column x on."""
    r = np.zeros((H, W), np.int32)
    r[:, x:] = 1
    return r


def test_one_vertical_edge_at_the_word_seam():
    labels = truth = halves(3, 130, 64)                                      # the boundary pixels are column 63, three rows
    assert np.array_equal(np.argwhere(B.edge_bits(B.canonical(labels, 2))), [[0, 63], [1, 63], [2, 63]])
    for d in (0, 1, 64):
        assert B.counts(labels, truth, 2, 2, d) == (3, 3, 3, 3)
    assert B.counts(labels, truth, 2, 2, 0, box=(0, 3, 64, 130)) == (0, 0, 0, 0)      # the box starts behind the boundary column
    assert B.counts(labels, truth, 2, 2, 0, box=(1, 2, 0, 64)) == (1, 1, 1, 1)


def test_truth_edge_two_pixels_from_a_label_edge():
    labels, truth = halves(4, 20, 10), halves(4, 20, 12)                     # boundary columns 9 and 11
    assert B.counts(labels, truth, 2, 2, 1) == (4, 0, 4, 0)
    assert B.counts(labels, truth, 2, 2, 2) == (4, 4, 4, 4)
    s = B.scores(B.counts(labels, truth, 2, 2, 1))
    assert s["recall"] == 0.0 and s["precision"] == 0.0 and math.isnan(s["f"])
    assert B.scores(B.counts(labels, truth, 2, 2, 2)) == {"recall": 1.0, "precision": 1.0, "f": 1.0}


def test_label_boundary_inside_unlabelled_truth_is_not_counted():
    labels = halves(4, 20, 10)                                               # boundary column 9
    truth = np.full((4, 20), -1, np.int32)
    truth[:, :3] = 0                                                         # truth boundary column 2: 0 | unlabelled
    assert B.counts(labels, truth, 2, 1, 2) == (4, 0, 0, 0)                  # column 9 is unlabelled and 7 pixels from column 2
    assert B.counts(labels, truth, 2, 1, 7) == (4, 4, 4, 4)
    truth[:, :] = 0                                                          # the same boundary on labelled truth is held against it
    assert B.counts(labels, truth, 2, 1, 2) == (0, 0, 4, 0)


def test_two_out_of_range_values_side_by_side_are_no_boundary():
    labels = np.array([[7, 9, -3, 0]], np.int32)                             # 7, 9, -3 are all outside 0..1: one value
    truth = np.array([[5, -1, 6, 6]], np.int32)                              # all outside 0..1
    assert np.array_equal(B.edge_bits(B.canonical(labels, 2)), [[False, False, True, False]])
    assert not B.edge_bits(B.canonical(truth, 2)).any()
    assert B.counts(labels, truth, 2, 2, 1) == (0, 0, 0, 0)


def test_one_label_raster_has_no_figures():
    labels, truth = np.zeros((5, 7), np.int32), halves(5, 7, 3)
    c = B.counts(labels, truth, 1, 2, 2)
    assert c == (5, 0, 0, 0)
    s = B.scores(c)
    assert s["recall"] == 0.0 and math.isnan(s["precision"]) and math.isnan(s["f"])
    c = B.counts(labels, labels, 1, 1, 2)
    assert c == (0, 0, 0, 0) and all(math.isnan(v) for v in B.scores(c).values())


def test_mapping_folds_regions_and_negative_entries_mean_no_region():
    labels = np.array([[0, 1, 2, 3]], np.int32)
    assert B.edge_bits(B.canonical(labels, 4)).sum() == 3
    assert B.edge_bits(B.canonical(labels, 4, np.array([0, 0, 1, 1], np.int32))).tolist() == [[False, True, False, False]]
    assert B.edge_bits(B.canonical(labels, 4, np.array([0, -5, -1, 0], np.int32))).tolist() == [[True, False, True, False]]


def test_the_scene_pair_is_not_degenerate():
    labels, S, truth, G = B.scene_pair()
    assert labels.shape == truth.shape == (200, 232) and len(np.unique(labels)) >= 50
    assert (truth < 0).any() and (truth >= G).any() and len(np.unique(truth[(truth >= 0) & (truth < G)])) >= 10
    for d in (1, 2, 3):
        n_t, h_t, n_l, h_l = B.counts(labels, truth, S, G, d)
        assert 0 < h_t < n_t and 0 < h_l < n_l, (d, n_t, h_t, n_l, h_l)


# ---- the Python side of the derived figures, without a GPU ------------------------------------------------------------------------
def test_scores_from_counts_match_the_spec():
    from deepmerge_amd import rag
    for c in ((4, 0, 4, 0), (4, 4, 4, 4), (5, 0, 0, 0), (0, 0, 0, 0), (10, 3, 7, 2), (0, 0, 3, 1)):
        s, ref = rag.boundary_scores_of(2, c), B.scores(c)
        assert (s.tolerance, s.n_truth_b, s.hit_truth, s.n_label_b, s.hit_label) == (2, *c)
        for k in ("recall", "precision", "f"):
            a, b = getattr(s, k), ref[k]
            assert a == b or (math.isnan(a) and math.isnan(b)), (c, k)


def test_cpu_tensors_and_bad_arguments_raise():
    import torch
    from deepmerge_amd import rag, scene
    z = torch.zeros((4, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag.boundary_scores(z, z, 1, 1)
    for bad in (-1, 65, 2.0, True, [], [1, 65]):
        with pytest.raises(ValueError, match="tolerance"):
            rag._tolerances(bad)
    assert rag._tolerances(3) == ([3], True) and rag._tolerances((0, 64)) == ([0, 64], False)
    with pytest.raises(ValueError, match="tolerance"):
        scene.boundary_scores(z, z, 1, 1, tolerance=65)
    with pytest.raises(ValueError, match="must cover the scene"):
        scene.boundary_scores(z, torch.zeros((4, 5), dtype=torch.int32), 1, 1)
    with pytest.raises(ValueError, match="mapping"):
        scene.boundary_scores(z, z, 3, 1, mapping=torch.zeros(2, dtype=torch.int32))

    class Wide:                                                    # a source whose windows cannot be indexed in int32
        shape = (1 << 16, 1 << 16)

        def read(self, *box):
            raise AssertionError("nothing is read before the limits are checked")

    with pytest.raises(ValueError, match="fewer than 2\\^31 pixels"):
        scene.boundary_scores(Wide(), Wide(), 1, 1, tile=1 << 16)

    class Long(Wide):
        shape = (1 << 31, 4)

    with pytest.raises(ValueError, match="H, W < 2\\^31"):
        scene.boundary_scores(Long(), Long(), 1, 1)


# ---- the library's side, without a GPU ----------------------------------------------------------------------------------------------
NEW = ("dm_boundary_bits", "dm_boundary_counts")


def test_header_signatures_and_exports_agree_and_abi_is_still_7(built):
    import ctypes
    lib = built.lib()
    assert lib.dm_abi_version() == 7
    declared = built.declared_symbols()
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW:
        assert name in declared and name in built.SIGNATURES and hasattr(raw, name), name
    assert sorted(built.SIGNATURES) == declared
    text = open(built.HEADER_PATH).read()
    for name, nargs in zip(NEW, (8, 12)):
        proto = text[text.index("int " + name + "("):]
        proto = proto[:proto.index(";")]
        assert proto.count(",") + 1 == nargs == len(built.SIGNATURES[name][1]), name


def test_boundary_entry_points_validate_before_any_launch(built):
    lib = built.lib()
    p = 4096                                                       # any non-null address: validation never dereferences
    bits = lambda *, raster=p, H=8, W=8, n=4, edge=p: lib.dm_boundary_bits(raster, H, W, n, None, edge, None, None)
    cnt = lambda *, le=p, te=p, tv=p, H=8, W=8, d=2, box=(0, 8, 0, 8), counts=p: lib.dm_boundary_counts(le, te, tv, H, W, d, *box, counts, None)
    cases = [
        (lambda: bits(raster=None), b"dm_boundary_bits: null pointer"),
        (lambda: bits(edge=None), b"dm_boundary_bits: null pointer"),
        (lambda: bits(H=0), b"dm_boundary_bits: bad sizes"),
        (lambda: bits(W=0), b"dm_boundary_bits: bad sizes"),
        (lambda: bits(H=1 << 16, W=1 << 15), b"dm_boundary_bits: bad sizes"),
        (lambda: bits(n=0), b"dm_boundary_bits: bad sizes"),
        (lambda: cnt(le=None), b"dm_boundary_counts: null pointer"),
        (lambda: cnt(te=None), b"dm_boundary_counts: null pointer"),
        (lambda: cnt(tv=None), b"dm_boundary_counts: null pointer"),
        (lambda: cnt(counts=None), b"dm_boundary_counts: null pointer"),
        (lambda: cnt(H=0), b"dm_boundary_counts: bad sizes"),
        (lambda: cnt(W=-1), b"dm_boundary_counts: bad sizes"),
        (lambda: cnt(H=1 << 16, W=1 << 15), b"dm_boundary_counts: bad sizes"),
        (lambda: cnt(d=-1), b"dm_boundary_counts: tolerance = -1 outside 0..64"),
        (lambda: cnt(d=65), b"dm_boundary_counts: tolerance = 65 outside 0..64"),
        (lambda: cnt(box=(3, 3, 0, 8)), b"dm_boundary_counts: bad box"),         # empty
        (lambda: cnt(box=(5, 3, 0, 8)), b"dm_boundary_counts: bad box"),         # inverted
        (lambda: cnt(box=(0, 8, 6, 2)), b"dm_boundary_counts: bad box"),
        (lambda: cnt(box=(0, 9, 0, 8)), b"dm_boundary_counts: bad box"),         # outside the raster
        (lambda: cnt(box=(0, 8, -1, 8)), b"dm_boundary_counts: bad box"),
    ]
    for call, msg in cases:
        assert call() == -1, msg
        assert msg in lib.dm_last_error(), (msg, lib.dm_last_error())
