"""GPU: scene.boundary_scores / SceneResult.boundary_scores (deepmerge_amd/scene.py, csrc/dm_boundary.hip).  The
definition is the test: the four integers equal rag.boundary_scores on the assembled rasters, whatever the tile size."""
import functools

import numpy as np
import pytest
import torch

import boundary_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILES = [(96, 112), (200, 232), (37, 41), (64, 64)]
TOLERANCES = [0, 2, 40]                           # 40: the halo of 41 pixels is wider than the smallest tile
LABELS, S, TRUTH, G = B.scene_pair()
MAPPING = (np.arange(S) // 3).astype(np.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def whole(d, mapped):
    """The reference, once per case: rag.boundary_scores on the whole rasters, itself checked against the spec."""
    from deepmerge_amd import rag
    m = MAPPING if mapped else None
    got = rag.boundary_scores(dev(LABELS), dev(TRUTH), S, G, d, mapping=None if m is None else dev(m))
    assert (got.n_truth_b, got.hit_truth, got.n_label_b, got.hit_label) == B.counts(LABELS, TRUTH, S, G, d, m)
    assert got.n_truth_b > 0 and got.n_label_b > 0
    return got


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("d", TOLERANCES)
@pytest.mark.parametrize("tile", TILES)
def test_every_tiling_equals_the_whole_raster(tile, d, mapped):
    from deepmerge_amd import scene
    got = scene.boundary_scores(LABELS, TRUTH, S, G, tolerance=d, tile=tile, mapping=dev(MAPPING) if mapped else None)
    print(f"tile {tile}, d = {d}, mapping {mapped}: {got}")
    assert got == whole(d, mapped)


def test_a_list_of_tolerances_and_the_kinds_of_source():
    from deepmerge_amd import scene
    want = [whole(d, False) for d in TOLERANCES]
    stage_times = {}
    assert scene.boundary_scores(LABELS, TRUTH, S, G, tolerance=TOLERANCES, tile=(96, 112), stage_times=stage_times) == want
    assert {"read + copy", "bits", "counts", "readback"} <= set(stage_times)
    assert scene.boundary_scores(torch.from_numpy(LABELS), scene.ArraySource(TRUTH), S, G, tolerance=tuple(TOLERANCES), tile=64) == want


def test_a_ring_source_as_the_truth():
    from deepmerge_amd import rag, scene
    polys = rag.polygons(dev(np.where((TRUTH >= 0) & (TRUTH < G), TRUTH, G).astype(np.int32)), G + 1)     # unlabelled traced as id G ...
    R = int(polys.region_ptr[G])                                                                          # ... and its rings, the last, dropped
    rings = rag.Rings(polys.ring_ptr[:R + 1].clone(), polys.xy[:int(polys.ring_ptr[R])].double(), polys.ring_label[:R].clone())
    source = scene.RingSource(rings, *TRUTH.shape)
    raster = source.read(0, TRUTH.shape[0], 0, TRUTH.shape[1])
    print("pixels where the rings' raster differs from the truth's canonical values:", int((raster.cpu().numpy() != B.canonical(TRUTH, G)).sum()))
    want = rag.boundary_scores(dev(LABELS), raster, S, G, 2)
    assert want.n_truth_b > 0 and want.hit_truth > 0 and (raster < 0).any()
    for tile in ((96, 112), (37, 41)):
        assert scene.boundary_scores(LABELS, source, S, G, tolerance=2, tile=tile) == want


def test_scene_result_scores_its_merged_partition_or_a_round():
    from deepmerge_amd import rag, scene
    rounds = [[(2 * k, 2 * k + 1) for k in range(S // 2)], [(4 * k, 4 * k + 2) for k in range(S // 4)]]
    res = B.hand_merge(S, rounds, DEV)
    none = torch.empty(0, device=DEV)
    sr = scene.SceneResult(result=res, n_labels=S, tiles=scene.tile_grid(*LABELS.shape, (96, 112)), offsets=None, stats={}, designed=none,
                           edges=none, weights=none, points=None, features=none, labels=LABELS)
    curve = res.boundary_scores(dev(LABELS), dev(TRUTH), G, tolerance=2)
    assert sr.boundary_scores(TRUTH, G) == curve[2] == rag.boundary_scores(dev(LABELS), dev(TRUTH), S, G, 2, mapping=res.region_of)
    assert sr.boundary_scores(TRUTH, G, tolerance=2, round=1) == curve[1]
    assert sr.boundary_scores(TRUTH, G, tolerance=[2], round=0) == [whole(2, False)]
