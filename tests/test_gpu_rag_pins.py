"""GPU: the label-raster chain of csrc/dm_rag.hip at its edges -- every width and height class of the 64x64 tile walk and its
16-pixel strips, ids outside [0, S), accumulators and keys beyond 2^32, full LDS tables on both load instantiations, both
refusals -- and the merge step (merge_components, points_to_csr, merge_partition) against plain references (tests/rag_ref.py).
Every comparison is exact."""
import numpy as np
import pytest
import torch

import rag_ref as R
from oracle import rag as OR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_raster(lab, tile, S, tl=None, stats=True, **kw):
    """rag_edges (twice), label_stats and designed_features of one raster against oracle/rag.py; returns the oracle's results."""
    from deepmerge_amd import rag
    tl = dev(lab) if tl is None else tl
    want_e, want_w = OR.rag_edges(lab, S)
    edges, w = rag.rag_edges(tl, S, **kw)
    assert edges.dtype == torch.int32 and w.dtype == torch.int32 and tuple(edges.shape) == want_e.shape and tuple(w.shape) == want_w.shape
    assert np.array_equal(edges.cpu().numpy(), want_e) and np.array_equal(w.cpu().numpy(), want_w)
    edges2, w2 = rag.rag_edges(tl, S, **kw)                 # insertion order varies; the result must not
    assert torch.equal(edges, edges2) and torch.equal(w, w2)
    if not stats:
        return want_e, want_w, None
    want_st = OR.label_stats(lab, tile, S)
    st = rag.label_stats(tl, dev(tile), S)
    for k in R.STAT_KEYS:
        assert np.array_equal(st[k].cpu().numpy(), want_st[k]), k
    f = rag.designed_features(st).cpu().numpy()
    assert np.array_equal(f.view(np.uint32), OR.designed_features(want_st).view(np.uint32))
    return want_e, want_w, want_st


@pytest.mark.parametrize("H", R.HEIGHTS)
def test_every_width_and_height_class(H):
    """Rows without a neighbour row (H = 1), strips shorter than 16, widths on and next to the 64-pixel tile seams, heights on and
    next to them, 3 % of the pixels outside [0, S).  Widths that are multiples of 16 run on both load instantiations."""
    for W in R.WIDTHS:
        lab, S, tile = R.width_case(H, W)
        assert ((lab < 0) | (lab >= S)).any()
        check_raster(lab, tile, S)
        if W % 16 == 0:
            check_raster(lab, tile, S, tl=R.offset_view(lab, 1))


def test_one_two_three_and_four_bands_through_the_scalar_loads():
    for bands in (1, 2, 3, 4):
        lab, S, tile = R.width_case(65, 65, bands)
        _, _, st = check_raster(lab, tile, S)
        assert st["sum"].shape[1] == min(bands, 3)


@pytest.mark.parametrize("H,W", [(264, 256), (263, 257)])       # 16-byte loads / scalar loads
def test_sum_of_squares_beyond_32_bits(H, W):
    """One label over the whole raster: the tile's LDS accumulators are 32-bit, the global ones must carry 64."""
    from deepmerge_amd import rag
    lab, S, tile = R.one_label_case(H, W)
    want_e, _, want_st = check_raster(lab, tile, S)
    assert want_e.shape == (0, 2)
    assert int(want_st["sumsq"][0, 0]) == 255 * 255 * H * W > 2 ** 32
    st = rag.label_stats(dev(lab), dev(tile), S)
    assert st["count"].tolist() == [H * W, 0]
    assert st["sumsq"][0, 0].item() == 255 * 255 * H * W and st["sum"][0, 0].item() == 255 * H * W
    assert st["peri"].tolist() == [[0, 2 * (H + W)], [0, 0]]
    assert st["bbox"].tolist() == [[0, 0, W - 1, H - 1], [2 ** 31 - 1, 2 ** 31 - 1, -1, -1]]
    f = rag.designed_features(st)
    assert f[0, 5].item() == 0.0 and f[0, 8].item() == 255.0          # var = 65025 - 255^2, clamped: std0 exactly 0
    assert not f[1].any()


@pytest.mark.parametrize("H,W,S", [(65, 130, 4096), (128, 128, 8192)])     # scalar loads, 2x3 tiles / 16-byte loads, 4 tiles
def test_full_lds_tables_across_tile_seams(H, W, S):
    lab, S, tile = R.noise_case(H, W, S)
    most_labels, most_pairs = R.max_per_tile(lab, S)
    assert most_labels > 64 and most_pairs > 128
    want_e, _, _ = check_raster(lab, tile, S)
    assert len(want_e) < max(1024, 8 * S)


def test_edge_keys_beyond_32_bits():
    lab, S = R.big_key_case()
    want_e, _, _ = check_raster(lab, None, S, stats=False, max_edges=1024)
    assert len(want_e) == 38 and int((want_e[:, 0].astype(np.int64) * S + want_e[:, 1]).max()) > 2 ** 32
    check_raster(lab, None, S, tl=R.offset_view(lab, 1), stats=False, max_edges=1024)


def test_more_edges_than_max_edges_is_refused_with_room_in_the_table():
    from deepmerge_amd import rag
    lab, S = R.refusal_case()
    tl = dev(lab)
    with pytest.raises(RuntimeError, match=r"found 112, table overflow=False"):
        rag.rag_edges(tl, S, max_edges=50)
    want_e, _, _ = check_raster(lab, None, S, tl=tl, stats=False)
    assert len(want_e) == 112


def test_table_overflow_is_refused_and_the_next_call_is_exact():
    from deepmerge_amd import rag
    lab, S = R.superpixels(128, 128, 5, 3)
    tl = dev(lab)
    with pytest.raises(RuntimeError, match=r"table overflow=True"):
        rag.rag_edges(tl, S, max_edges=16)
    check_raster(lab, None, S, tl=tl, stats=False)


def test_reserved_id_counts_as_outside():
    from deepmerge_amd import rag
    tile = np.arange(12, dtype=np.uint8).reshape(1, 3, 4)
    check_raster(R.RESERVED, tile, R.RESERVED_S)
    st = rag.label_stats(dev(R.RESERVED), dev(tile), R.RESERVED_S)
    assert st["count"].tolist() == R.RESERVED_COUNT and st["peri"].tolist() == R.RESERVED_PERI
    edges, w = rag.rag_edges(dev(R.RESERVED), R.RESERVED_S)
    assert edges.tolist() == R.RESERVED_EDGES and w.tolist() == R.RESERVED_WEIGHTS


# ---- the merge step ---------------------------------------------------------------------------------------------------------
def check_components(edges, merge, S):
    from deepmerge_amd import rag
    want = R.components_ref(edges, merge, S)
    te = dev(edges) if len(edges) else torch.zeros((0, 2), dtype=torch.int32, device=DEV)
    tm = dev(merge) if len(edges) else torch.zeros((0,), dtype=torch.bool, device=DEV)
    got = rag.merge_components(te, tm, S)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy().astype(np.int64), want)
    return want


def test_merge_components_beyond_one_grid_of_edges():
    """600000 edges: the hook kernel's launch is capped at 2048 x 256 threads, so its stride loop takes a second trip."""
    edges, merge, S = R.random_graph(200000, 600000, 0.3, 7)
    assert len(edges) > 2048 * 256 and merge[2048 * 256:].any()
    want = check_components(edges, merge, S)
    assert 1 < len(set(want.tolist())) < S
    check_components(*R.with_junk(edges, merge, S))


@pytest.mark.parametrize("k", [4, 10, 14])
def test_merge_components_on_paths(k):
    for order in ("identity", "zigzag", "bitrev"):
        edges, merge, n = R.path_graph(k, order)
        want = check_components(edges, merge, n)
        assert len(set(want.tolist())) == 1 + (n - 1) // 37
        check_components(*R.with_junk(edges, merge, n))


def test_merge_components_on_stars_and_a_single_node():
    from deepmerge_amd import rag
    for centre_is_largest in (True, False):
        edges, merge, n = R.star_graph(centre_is_largest)
        assert not check_components(edges, merge, n).any()
        check_components(*R.with_junk(edges, merge, n))
    none = rag.merge_components(torch.zeros((0, 2), dtype=torch.int32, device=DEV), torch.zeros((0,), dtype=torch.bool, device=DEV), 1)
    assert none.tolist() == [0]


def test_merge_components_refusals():
    from deepmerge_amd import rag
    edges = torch.tensor([[0, 1], [2, 3], [3, 4]], dtype=torch.int32, device=DEV)
    one = torch.tensor([False, True, False], device=DEV)
    with pytest.raises(RuntimeError):                       # the round that hooks sets `changed`: one round cannot confirm
        rag.merge_components(edges, one, 5, max_rounds=1)
    assert rag.merge_components(edges, one, 5, max_rounds=2).tolist() == [0, 1, 2, 2, 4]
    with pytest.raises(ValueError):
        rag.merge_components(torch.tensor([[-1, 1], [2, 3]], dtype=torch.int32, device=DEV), torch.tensor([True, False], device=DEV), 5)
    with pytest.raises(ValueError):
        rag.merge_components(edges, one, 4)
    unflagged = rag.merge_components(torch.tensor([[-1, 1], [2, 3]], dtype=torch.int32, device=DEV), torch.tensor([False, True], device=DEV), 5)
    assert unflagged.tolist() == [0, 1, 2, 2, 4]


def test_points_to_csr_and_merge_partition_match_their_references():
    from deepmerge_amd import rag
    lab, S = R.superpixels(96, 96, 5, 5)
    S += 3
    ys, xs = np.mgrid[2:96:4, 2:96:4]
    xy = np.stack((xs.reshape(-1), ys.reshape(-1)), 1).astype(np.int32)
    rng = np.random.default_rng(9)
    xy = xy[rng.permutation(len(xy))]                       # points keep their order inside a superpixel, whatever it is
    tl = dev(lab)
    ptr, idx = rag.points_to_csr(tl, dev(xy), S)
    want_ptr, want_idx = R.points_to_csr_ref(lab, xy, S)
    assert (np.diff(want_ptr) == 0).sum() > 3 and np.diff(want_ptr).max() > 1
    assert ptr.dtype == torch.int32 and idx.dtype == torch.int32
    assert np.array_equal(ptr.cpu().numpy(), want_ptr) and np.array_equal(idx.cpu().numpy(), want_idx)

    edges, _ = rag.rag_edges(tl, S)
    e = edges.cpu().numpy()
    merge = rng.random(len(e)) < 0.3
    root = rag.merge_components(edges, dev(merge), S)
    assert np.array_equal(root.cpu().numpy(), R.components_ref(e, merge, S))
    dead = np.stack((np.full(20, -1), rng.integers(0, S, 20)), 1).astype(np.int32)
    dead[::2] = dead[::2, ::-1]
    rows = np.concatenate((e, dead, e[::3, ::-1]))          # -1 rows on either side, repeated and swapped rows
    rows = rows[rng.permutation(len(rows))]
    got = rag.merge_partition(ptr, idx, dev(rows), root)
    want = R.merge_partition_ref(want_ptr, want_idx, rows, root.cpu().numpy())
    assert 1 < len(want[1]) - 1 < S and 0 < len(want[3]) < len(e)
    for g, w, name in zip(got, want, ("new_id", "ptr", "idx", "edges")):
        assert g.dtype == torch.int32 and tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w), name
