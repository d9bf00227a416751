"""CPU: the spec of the label-raster chain stated twice.  oracle/rag.py against tests/rag_ref.py's per-pixel loop on thin, tiny and
dirty rasters, the strict sweep oracle against numpy's float32 sum for every D in 1..128, and the references the GPU pins use
(components, point lists, merged partition) on known answers."""
import numpy as np
import pytest

import rag_ref as R
from oracle import rag as OR
from oracle import sweep as OS


def assert_same_rag(lab, tile, S):
    edges, weights, stats, feats = R.brute_rag(lab, tile, S)
    want_e, want_w = OR.rag_edges(lab, S)
    assert want_e.shape == edges.shape and np.array_equal(want_e, edges) and np.array_equal(want_w, weights)
    want_st = OR.label_stats(lab, tile, S)
    for k in R.STAT_KEYS:
        assert want_st[k].shape == stats[k].shape and want_st[k].dtype == stats[k].dtype, k
        assert np.array_equal(want_st[k], stats[k]), k
    want_f = OR.designed_features(want_st)
    assert np.array_equal(want_f.view(np.uint32), feats.view(np.uint32))
    return stats


@pytest.mark.parametrize("H", [1, 2, 3, 17])
@pytest.mark.parametrize("W", [1, 2, 15, 16, 17, 33])
def test_brute_rag_equals_the_oracle(H, W):
    rng = np.random.default_rng(100 * H + W)
    lab, S = R.superpixels(H, W, 3, 100 * H + W)
    S += 2
    bad = R.dirty(lab, S, rng)
    assert ((bad < 0) | (bad >= S)).any()
    for bands in (1, 2, 3, 4):
        tile = rng.integers(0, 256, (bands, H, W), dtype=np.uint8)
        for raster in (lab, bad):
            st = assert_same_rag(raster, tile, S)
            assert st["sum"].shape == (S, min(bands, 3))
            assert int(st["count"].sum()) == int(((raster >= 0) & (raster < S)).sum())


def test_dirty_draws_every_id_outside_the_range():
    lab, S = R.superpixels(40, 40, 5, 0)
    bad = R.dirty(lab, S, np.random.default_rng(0))
    changed = bad != lab
    assert changed.sum() == round(0.03 * lab.size)
    assert set(bad[changed].tolist()) == {-1, -7, S, S + 7, 2 ** 31 - 1, -2 ** 31}
    assert np.array_equal(bad, R.dirty(lab, S, np.random.default_rng(0)))


def test_reserved_id_counts_as_outside():
    """The id -2 is the pass's marker for "outside the raster" (oracle/rag.py, include/deepmerge_hip.h): the four neighbours of
    pixel (1, 1) count their side towards it as border.
        0  0  1  1
        0 -2  1  1        label 0: (0,0) 2 border; (0,1) 2 border + right; (1,0) 2 border + below        -> inner 2, border 6
        2  2  2  1        label 1: (0,2) 1 + left; (0,3) 2; (1,2) 1 border + below; (1,3) 1; (2,3) 2 + left -> inner 3, border 7
                          label 2: (2,0) 2 + above; (2,1) 2 border; (2,2) 1 + above + right              -> inner 3, border 5"""
    tile = np.arange(12, dtype=np.uint8).reshape(1, 3, 4)
    for got in (OR.label_stats(R.RESERVED, tile, R.RESERVED_S), R.brute_rag(R.RESERVED, tile, R.RESERVED_S)[2]):
        assert got["count"].tolist() == R.RESERVED_COUNT
        assert got["peri"].tolist() == R.RESERVED_PERI
    edges, w = OR.rag_edges(R.RESERVED, R.RESERVED_S)
    assert edges.tolist() == R.RESERVED_EDGES and w.tolist() == R.RESERVED_WEIGHTS
    assert_same_rag(R.RESERVED, tile, R.RESERVED_S)
    # any other id outside the range is "a different id": the same raster with -1 has the four sides in the inner column
    other = np.where(R.RESERVED == -2, -1, R.RESERVED).astype(np.int32)
    st = assert_same_rag(other, tile, R.RESERVED_S)
    assert st["peri"].tolist() == [[4, 4], [4, 6], [4, 4]]


def test_case_generators_hold_what_the_gpu_tests_need():
    lab, S = R.big_key_case()
    edges, _ = OR.rag_edges(lab, S)
    assert lab.shape == (32, 48) and len(edges) == 38
    assert int((edges[:, 0].astype(np.int64) * S + edges[:, 1]).max()) > 2 ** 32
    lab, S = R.refusal_case()
    assert len(OR.rag_edges(lab, S)[0]) == 112
    for H, W in ((264, 256), (263, 257)):
        lab, S, tile = R.one_label_case(H, W)
        assert 255 * 255 * H * W > 2 ** 32 and (tile[0] == 255).all() and not lab.any()
    for H, W, S, pairs in ((65, 130, 4096, 16670), (128, 128, 8192, 32471)):
        lab, S, _ = R.noise_case(H, W, S)
        assert len(OR.rag_edges(lab, S)[0]) == pairs < max(1024, 8 * S)
        most_l, most_p = R.max_per_tile(lab, S)
        assert most_l > 64 and most_p > 128


@pytest.mark.parametrize("lo", [1, 33, 65, 97])
def test_strict_sweep_oracle_is_numpy_float32_for_every_dim(lo):
    """|a|^2, |b|^2 and a.b of the pinned order equal numpy's float32 sum of the rounded products for every D in 1..128, so
    simi does bit for bit; equal rows give exactly 0.0."""
    for D in range(lo, lo + 32):
        rng = np.random.default_rng(D)
        pooled = rng.normal(size=(4, D)).astype(np.float32)
        pooled[3] = pooled[2]
        edges = np.array([[0, 1], [1, 2], [2, 3], [3, 0]], np.int32)
        simi, merge = OS.strict_edge_similarity(pooled, edges, 1.0)
        for e, (l, r) in enumerate(edges.tolist()):
            a, b = pooled[l], pooled[r]
            d = (np.sum(a * a) + np.sum(b * b)) - np.float32(2) * np.sum(a * b)
            assert d.dtype == np.float32
            want = np.sqrt(d if d > 0 else np.float32(0))
            assert simi[e].view(np.uint32) == want.view(np.uint32), (D, e)
            assert bool(merge[e]) == bool(want < np.float32(1.0))
        assert simi[2] == 0.0 and not np.signbit(simi[2])


@pytest.mark.parametrize("S,E,frac", [(50, 120, 0.3), (5000, 20000, 0.2), (20000, 60000, 0.05), (300, 0, 0.5)])
def test_components_ref_matches_scipy(S, E, frac):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    rng = np.random.default_rng(S + E)                      # the draw of test_gpu_rag.test_merge_components_matches_scipy
    edges = rng.integers(0, S, size=(max(E, 1), 2)).astype(np.int32)[:E].reshape(E, 2)
    merge = (rng.random(E) < frac)
    ea, eb = edges[merge, 0], edges[merge, 1]
    _, comp = connected_components(coo_matrix((np.ones(len(ea)), (ea, eb)), shape=(S, S)), directed=False)
    first = {}
    want = np.array([first.setdefault(comp[s], s) for s in range(S)], np.int64)
    assert np.array_equal(R.components_ref(edges, merge, S), want)


def test_components_ref_on_paths_stars_and_junk():
    for order in ("identity", "zigzag", "bitrev"):
        edges, merge, n = R.path_graph(6, order)
        root = R.components_ref(edges, merge, n)
        assert len(set(root.tolist())) == 2                 # 63 edges, the 37th unflagged: two pieces
        assert np.array_equal(root, R.components_ref(*R.with_junk(edges, merge, n)))
    assert [R.bit_reverse(p, 3) for p in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7]
    assert R.path_graph(3, "zigzag", 0)[0].max() == 7
    for big in (True, False):
        edges, merge, n = R.star_graph(big)
        assert n == 301 and not R.components_ref(edges, merge, n).any()
    e, m, _ = R.with_junk(*R.random_graph(100, 50, 0.5, 0))
    assert len(e) == 65 and (e[:, 0] == e[:, 1]).sum() >= 5 and ((e[:, 0] == -1) & ~m).sum() == 5


def test_points_to_csr_ref_known_answer():
    lab = np.array([[0, 0, 2],
                    [3, 2, 2]], np.int32)
    xy = np.array([[2, 1], [0, 0], [1, 1], [1, 0], [2, 0]], np.int32)         # (x, y): labels 2, 0, 2, 0, 2
    ptr, idx = R.points_to_csr_ref(lab, xy, 5)
    assert ptr.tolist() == [0, 2, 2, 5, 5, 5] and idx.tolist() == [1, 3, 0, 2, 4]


def test_merge_partition_ref_known_answer():
    # six superpixels; components {0, 2, 5}, {1}, {3, 4}
    ptr = [0, 2, 3, 3, 5, 6, 8]
    idx = [7, 1, 4, 0, 6, 2, 5, 3]
    root = [0, 1, 0, 3, 3, 0]
    edges = [[0, 1], [0, 2], [1, 2], [2, 3], [4, 5], [-1, 3], [3, 4], [1, -1], [1, 5]]
    new_id, new_ptr, new_idx, new_edges = R.merge_partition_ref(ptr, idx, edges, root)
    assert new_id.tolist() == [0, 1, 0, 2, 2, 0]
    assert new_ptr.tolist() == [0, 4, 5, 8] and new_idx.tolist() == [7, 1, 5, 3, 4, 0, 6, 2]
    assert new_edges.tolist() == [[0, 1], [0, 2]]          # (0,1), (1,2), (1,5) fold into one; (2,3), (4,5) into the other
    none = R.merge_partition_ref(ptr, idx, [[-1, 2]], list(range(6)))
    assert none[0].tolist() == list(range(6)) and none[1].tolist() == ptr and none[2].tolist() == idx and none[3].shape == (0, 2)
