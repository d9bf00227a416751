"""GPU: rag.boundary_scores / MergeResult.boundary_scores (csrc/dm_boundary.hip) against the numpy spec
tests/boundary_ref.py -- every comparison is an exact equality of the four integers."""
import functools
import math

import numpy as np
import pytest
import torch

import boundary_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = (1, 63, 64, 65, 129, 257, 300)           # word seams, the 256-pixel workgroup seam, ragged tails
HEIGHTS = (1, 2, 67)                              # 67: two row tiles of the count kernel, nine row groups of the bits kernel
TOLERANCES = [0, 1, 2, 31, 63, 64]                # 64 is larger than H and, for most widths, than W


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def four(s):
    return s.n_truth_b, s.hit_truth, s.n_label_b, s.hit_label


def assert_equals_spec(got, labels, truth, S, G, d, mapping=None, box=None):
    ref = B.counts(labels, truth, S, G, d, mapping, box)
    print(f"d = {d}: got {four(got)}, spec {ref}")
    assert got.tolerance == d and four(got) == ref, (d, four(got), ref)
    for k, v in B.scores(ref).items():
        a = getattr(got, k)
        assert a == v or (math.isnan(a) and math.isnan(v)), (d, k, a, v)


def score(labels, truth, S, G, tolerance, mapping=None, box=None):
    from deepmerge_amd import rag
    return rag.boundary_scores(dev(labels), dev(truth), S, G, tolerance, mapping=None if mapping is None else dev(mapping), box=box)


@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("W", WIDTHS)
def test_every_width_height_and_tolerance(H, W):
    labels, S, truth, G = B.small_pair(H, W, 100 * H + W)
    got = score(labels, truth, S, G, TOLERANCES)
    assert isinstance(got, list) and len(got) == len(TOLERANCES)
    for d, s in zip(TOLERANCES, got):
        assert_equals_spec(s, labels, truth, S, G, d)


def test_a_list_of_tolerances_equals_the_single_calls():
    labels, S, truth, G = B.small_pair(67, 300, 5)
    many = score(labels, truth, S, G, (3, 0, 17))
    assert [s.tolerance for s in many] == [3, 0, 17]
    for s in many:
        one = score(labels, truth, S, G, s.tolerance)
        assert not isinstance(one, list) and one == s


def test_boundary_in_the_last_row_and_the_last_column():
    H, W = 70, 130
    labels = np.zeros((H, W), np.int32)
    labels[H - 1, :] = 1                                            # boundary pixels: row H - 2 ...
    labels[H - 1, 100:] = 2                                         # ... and (H - 1, 99), in the last row
    truth = np.zeros((H, W), np.int32)
    truth[:, W - 1] = 1                                             # boundary pixels: column W - 2 down to row H - 2 ...
    truth[H - 1, W - 1] = 0                                         # ... and (H - 2, W - 1), in the last column
    for d in (0, 1, 64):
        assert_equals_spec(score(labels, truth, 3, 2, d), labels, truth, 3, 2, d)
    assert four(score(labels, truth, 3, 2, 0)) == (H, 2, W + 1, 2)  # they share (H - 2, W - 2) and (H - 2, W - 1)


def test_checkerboard_every_pixel_is_a_boundary():
    H, W = 67, 129
    y, x = np.mgrid[0:H, 0:W]
    board = ((y + x) % 2).astype(np.int32)
    got = score(board, board, 2, 2, 0)
    assert four(got) == (H * W - 1,) * 4                            # all but the last pixel, which has no right or lower neighbour
    assert got.recall == got.precision == got.f == 1.0
    assert_equals_spec(score(board, np.zeros_like(board), 2, 1, 2), board, np.zeros_like(board), 2, 1, 2)


@pytest.mark.parametrize("what", ["constant", "truth unlabelled", "ids outside the range"])
def test_degenerate_rasters(what):
    H, W = 67, 257
    labels, S, truth, G = B.small_pair(H, W, 9)
    if what == "constant":
        labels, truth = np.full((H, W), 3, np.int32), np.full((H, W), 1, np.int32)
    elif what == "truth unlabelled":
        truth = np.where(truth % 2 == 0, -1, G + 5).astype(np.int32)          # two different out-of-range values: one value
    else:
        labels[10:30, 60:70], labels[10:30, 70:80] = -4, S + 9                 # side by side: no boundary between them
        truth[40:50, :], truth[50:60, :] = G, -1
    for d in (0, 2):
        got = score(labels, truth, S, G, d)
        assert_equals_spec(got, labels, truth, S, G, d)
        if what != "ids outside the range":
            assert got.n_truth_b == 0 and got.n_label_b == 0 and math.isnan(got.recall) and math.isnan(got.precision) and math.isnan(got.f)


def test_mappings():
    labels, S, truth, G = B.small_pair(67, 300, 21)
    one = np.zeros(S, np.int32)                                      # folds every region into one: no label boundary but the holes'
    ident = np.arange(S, dtype=np.int32)
    fold = (np.arange(S) // 2).astype(np.int32)
    gaps = np.where(np.arange(S) % 3 == 0, -2, np.arange(S)).astype(np.int32)    # negative entries: "no region"
    for d in (0, 2, 31):
        plain = score(labels, truth, S, G, d)
        assert score(labels, truth, S, G, d, mapping=ident) == plain
        for m in (one, fold, gaps):
            assert_equals_spec(score(labels, truth, S, G, d, mapping=m), labels, truth, S, G, d, mapping=m)
    filled = np.where((labels >= 0) & (labels < S), labels, 0).astype(np.int32)
    assert four(score(filled, truth, S, G, 2, mapping=one))[2:] == (0, 0)


def test_box_whose_nearest_boundary_lies_outside_it():
    H, W = 40, 300
    labels, truth = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    labels[:, 101:] = 1                                             # label boundary: column 100, outside the box
    truth[:, 104:] = 1                                              # truth boundary: column 103, inside
    box = (10, 30, 102, 200)
    assert four(score(labels, truth, 2, 2, 2, box=box)) == (20, 0, 0, 0)
    assert four(score(labels, truth, 2, 2, 3, box=box)) == (20, 20, 0, 0)
    assert four(score(labels, truth, 2, 2, 3, box=(10, 30, 64, 103))) == (0, 0, 20, 20)
    lab, S, tru, G = B.small_pair(67, 300, 33)
    for b in ((1, 66, 1, 299), (64, 67, 63, 65), (20, 21, 128, 257), (0, 67, 256, 300)):
        for d in (0, 2, 64):
            assert_equals_spec(score(lab, tru, S, G, d, box=b), lab, tru, S, G, d, box=b)


@functools.lru_cache(maxsize=None)
def scene_pair():
    return B.scene_pair()


@pytest.mark.parametrize("d", [1, 2, 3])
def test_the_scene_pair(d):
    labels, S, truth, G = scene_pair()
    n_t, h_t, n_l, h_l = B.counts(labels, truth, S, G, d)
    assert 0 < h_t < n_t and 0 < h_l < n_l                          # the case is not degenerate
    assert_equals_spec(score(labels, truth, S, G, d), labels, truth, S, G, d)


def test_merge_result_boundary_scores_round_by_round():
    from deepmerge_amd import rag
    labels, S, truth, G = scene_pair()
    labels = labels.copy()
    labels[5:9, 7:30] = -1                                          # ids outside [0, S0) stay what they are through a merge
    rounds = [[(2 * k, 2 * k + 1) for k in range(S // 2)], [(4 * k, 4 * k + 2) for k in range(S // 4)]]
    res = B.hand_merge(S, rounds, DEV)
    tl, tt = dev(labels), dev(truth)
    before = tl.clone()
    got = res.boundary_scores(tl, tt, G, tolerance=2)
    assert len(got) == 3 and torch.equal(tl, before)
    for r, s in enumerate(got):
        m = B.region_of_at(S, rounds, r)
        assert np.array_equal(res.region_of_at(r).cpu().numpy(), m)
        assert s == rag.boundary_scores(rag.relabel_raster(tl, res.region_of_at(r)), tt, S, G, 2)
        assert_equals_spec(s, labels, truth, S, G, 2, mapping=m)
    assert got[0].n_label_b > got[1].n_label_b > got[2].n_label_b   # merging removes boundary
    assert res.boundary_scores(tl, tt, G, tolerance=1, rounds=[2, 0]) == [rag.boundary_scores(tl, tt, S, G, 1, mapping=res.region_of),
                                                                          rag.boundary_scores(tl, tt, S, G, 1)]
    with pytest.raises(ValueError):
        res.boundary_scores(tl, tt, G, rounds=[3])


def test_bad_arguments_raise():
    from deepmerge_amd import rag
    z = torch.zeros((4, 4), dtype=torch.int32, device=DEV)
    for call in (lambda: rag.boundary_scores(z, z, 1, 1, 65), lambda: rag.boundary_scores(z, z, 1, 1, -1),
                 lambda: rag.boundary_scores(z, z[:3], 1, 1), lambda: rag.boundary_scores(z.long(), z, 1, 1),
                 lambda: rag.boundary_scores(z, z, 0, 1), lambda: rag.boundary_scores(z, z, 2, 1, mapping=z[0, :3].contiguous()),
                 lambda: rag.boundary_scores(z, z, 1, 1, box=(0, 5, 0, 4)), lambda: rag.boundary_scores(z, z, 1, 1, box=(2, 2, 0, 4))):
        with pytest.raises(ValueError):
            call()
