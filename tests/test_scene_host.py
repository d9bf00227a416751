"""CPU: the host side of the scene driver (deepmerge_amd/scene.py) and of dm_seam_stitch -- the tile grid, the sources, every
limit, the declaration / binding / export of the new entry point and its validation before any launch, the numpy spec itself."""
import os
import re
import subprocess

import numpy as np
import pytest

import scene_ref as R


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


# ---- tile_grid ----------------------------------------------------------------------------------------------------------------------
def covers_exactly(tiles, H, W):
    seen = np.zeros((H, W), np.int32)
    for y0, y1, x0, x1 in tiles:
        assert 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W
        seen[y0:y1, x0:x1] += 1
    return bool((seen == 1).all())


def test_tile_grid_covers_the_scene_exactly_once_in_row_major_order():
    from deepmerge_amd.scene import tile_grid
    assert tile_grid(8, 12, 4) == [(0, 4, 0, 4), (0, 4, 4, 8), (0, 4, 8, 12), (4, 8, 0, 4), (4, 8, 4, 8), (4, 8, 8, 12)]
    for H, W, tile in ((200, 232, (96, 112)), (7, 5, 3), (64, 64, 64), (100, 1, (7, 9)), (1, 1, 1)):
        tiles = tile_grid(H, W, tile)
        assert covers_exactly(tiles, H, W)
        assert tiles == sorted(tiles, key=lambda t: (t[0], t[2]))
    tiles = tile_grid(200, 232, (96, 112))                         # ragged last row and column: 8-pixel slivers
    assert len(tiles) == 9 and tiles[-1] == (192, 200, 224, 232) and tiles[2] == (0, 96, 224, 232) and tiles[6] == (192, 200, 0, 112)
    tiles = tile_grid(9, 17, (4, 8))                               # a 1-pixel sliver on both axes
    assert tiles[-1] == (8, 9, 16, 17) and covers_exactly(tiles, 9, 17)
    assert tile_grid(10, 20, 4096) == [(0, 10, 0, 20)]             # a tile larger than the scene
    assert tile_grid(10, 20, (3, 4096)) == [(0, 3, 0, 20), (3, 6, 0, 20), (6, 9, 0, 20), (9, 10, 0, 20)]
    for bad in (0, -1, (0, 4), (4, 0)):
        with pytest.raises(ValueError, match="tile must be >= 1"):
            tile_grid(10, 10, bad)
    with pytest.raises(ValueError, match="at least one pixel"):
        tile_grid(0, 10, 4)


def test_halo_and_window_clip_to_the_scene():
    from deepmerge_amd.scene import halo_of, window_of
    assert [halo_of(m) for m in (1, 2, 63, 64, 383, 384)] == [1, 1, 32, 32, 192, 192]
    assert window_of((96, 192, 112, 224), 200, 232, 32) == (64, 200, 80, 232)
    assert window_of((0, 96, 0, 112), 200, 232, 32) == (0, 128, 0, 144)
    assert window_of((0, 5, 0, 5), 5, 5, 192) == (0, 5, 0, 5)


# ---- sources --------------------------------------------------------------------------------------------------------------------------
def test_array_source_on_an_array_a_memmap_and_a_tensor(tmp_path):
    import torch
    from deepmerge_amd.scene import ArraySource
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (3, 40, 50), dtype=np.uint8)
    path = tmp_path / "scene.u8"
    mm = np.memmap(path, dtype=np.uint8, mode="w+", shape=img.shape)
    mm[:] = img
    mm.flush()
    for src in (ArraySource(img), ArraySource(np.memmap(path, dtype=np.uint8, mode="r", shape=img.shape)), ArraySource(torch.from_numpy(img))):
        assert src.shape == (3, 40, 50)
        got = src.read(7, 31, 45, 50)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (3, 24, 5) and got.flags.c_contiguous
        assert np.array_equal(got, img[:, 7:31, 45:50])
        got[:] = 0                                                 # a copy: the scene is untouched
        assert np.array_equal(src.read(0, 40, 0, 50), img)
    truth = rng.integers(0, 9, (40, 50)).astype(np.int32)
    src = ArraySource(truth)
    assert src.shape == (40, 50) and np.array_equal(src.read(1, 3, 2, 9), truth[1:3, 2:9])
    for bad in (np.zeros(5, np.uint8), np.zeros((1, 2, 3, 4), np.uint8), [[1, 2]]):
        with pytest.raises(ValueError, match="ArraySource takes"):
            ArraySource(bad)


class Shape:
    """A source of a given shape whose pixels are never read (the limits are checked before the first read)."""

    def __init__(self, *shape):
        self.shape = shape

    def read(self, y0, y1, x0, x1):
        raise AssertionError("read before the limits were checked")


# ---- limits -----------------------------------------------------------------------------------------------------------------------------
def test_every_limit_is_a_value_error_before_any_device_work():
    import torch
    from deepmerge_amd import rag, scene
    img = np.zeros((3, 20, 30), np.uint8)
    graph = lambda src=img, **kw: scene._scene_graph(src, device="cpu", **kw)
    for tile in (0, -4, (8, 0)):
        with pytest.raises(ValueError, match="tile must be >= 1"):
            graph(tile=tile)
    for mw in (0, -1, rag.MAX_WINDOW + 1):
        with pytest.raises(ValueError, match="max_window must be in 1..384"):
            graph(tile=8, max_window=mw)
    for out in (np.zeros((20, 30), np.int64), np.zeros((20, 31), np.int32), np.zeros((1, 20, 30), np.int32), torch.zeros(20, 30, dtype=torch.int32)):
        with pytest.raises(ValueError, match="labels_out must be a writable int32"):
            graph(tile=8, labels_out=out)
    frozen = np.zeros((20, 30), np.int32)
    frozen.flags.writeable = False
    with pytest.raises(ValueError, match="labels_out must be a writable int32"):
        graph(tile=8, labels_out=frozen)
    for shape in ((20, 30), (0, 20, 30), (3, 0, 30)):
        with pytest.raises(ValueError, match="source.shape must be"):
            graph(Shape(*shape), tile=8)
    # every window below 2^31 pixels: 46000^2 < 2^31 <= (46000 + 2 * 192)^2 inside a larger scene; 46384^2 > 2^31 as a whole scene
    with pytest.raises(ValueError, match="fewer than 2\\^31 pixels, got 46384 x 46384"):
        graph(Shape(3, 200000, 200000), tile=46000)
    with pytest.raises(ValueError, match="fewer than 2\\^31 pixels"):
        graph(Shape(1, 46384, 46384), tile=1 << 20)
    with pytest.raises(AssertionError, match="read before"):      # a scene within every limit goes on to read
        graph(Shape(3, 300, 300), tile=100, max_window=64)
    # total superpixels <= MAX_REGIONS: counted as the tiles come in, refused before the tile's kernels run
    calls = []

    def many(core_tile):
        calls.append(tuple(core_tile.shape))
        return torch.zeros(core_tile.shape[1:], dtype=torch.int32), rag.MAX_REGIONS + 1

    with pytest.raises(ValueError, match="more than 2\\^24 superpixels"):
        graph(tile=16, segmenter=many)
    assert calls == [(3, 16, 16)]
    with pytest.raises(ValueError, match="segmenter must return"):
        graph(tile=16, segmenter=lambda t: (torch.zeros(t.shape[1:], dtype=torch.int64), 1))
    with pytest.raises(ValueError, match="segmenter must return"):
        graph(tile=16, segmenter=lambda t: (torch.zeros((4, 4), dtype=torch.int32), 1))
    with pytest.raises(ValueError, match="source.read.* must return torch.uint8"):
        graph(img.astype(np.int16), tile=16)


def test_cpu_tensors_have_no_fallback():
    import torch
    from deepmerge_amd import rag, scene
    a = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag.seam_stitch(a, a, 3, torch.zeros((3, 2), dtype=torch.int64))
    one = lambda t: (torch.zeros(t.shape[1:], dtype=torch.int32), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):    # the driver has none either: its first kernel refuses
        scene._scene_graph(np.zeros((3, 8, 8), np.uint8), tile=4, segmenter=one, device="cpu")


# ---- the library's side, without a GPU ----------------------------------------------------------------------------------------------------
def test_seam_stitch_is_declared_bound_and_exported(built):
    text = re.sub(r"/\*.*?\*/", "", open(built.HEADER_PATH).read(), flags=re.S)
    decl = re.search(r"\bint\s+dm_seam_stitch\s*\(([^)]*)\)\s*;", text)
    assert decl
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert len(args) == 14 == len(built.SIGNATURES["dm_seam_stitch"][1])
    # the trailing eight are the ones rag._count_keys passes, as dm_rag_edges declares them; then the stream
    rag_decl = re.search(r"\bint\s+dm_rag_edges\s*\(([^)]*)\)\s*;", text)
    rag_args = [" ".join(a.split()) for a in rag_decl.group(1).split(",")]
    assert args[5:] == rag_args[4:]
    assert built.SIGNATURES["dm_seam_stitch"][1][5:] == built.SIGNATURES["dm_rag_edges"][1][4:]
    nm = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T dm_seam_stitch\b", nm)
    assert built.lib().dm_abi_version() == 7                       # additive


def test_seam_stitch_refuses_bad_arguments_before_any_launch(built):
    lib = built.lib()
    p = 4096                                                       # any non-null address: validation never dereferences
    ok = dict(a=p, b=p, n=5, S=3, peri=p, table_keys=p, table_counts=p, capacity_log2=10, edge_keys=p, edge_counts=p, max_edges=16,
              n_edges=p, overflow=p)
    cases = [(dict(**{k: None}), b"null pointer") for k in ("a", "b", "peri", "table_keys", "table_counts", "edge_keys", "edge_counts",
                                                           "n_edges", "overflow")]
    cases += [(dict(n=0), b"bad sizes"), (dict(n=-1), b"bad sizes"), (dict(S=0), b"bad sizes"), (dict(S=(1 << 24) + 1), b"bad sizes"),
              (dict(S=1 << 40), b"bad sizes"), (dict(capacity_log2=7), b"bad sizes"), (dict(capacity_log2=31), b"bad sizes"),
              (dict(max_edges=0), b"bad sizes")]
    for change, msg in cases:
        args = {**ok, **change}
        assert lib.dm_seam_stitch(*args.values(), None) == -1, change
        assert b"dm_seam_stitch" in lib.dm_last_error() and msg in lib.dm_last_error(), (change, lib.dm_last_error())


# ---- the spec ---------------------------------------------------------------------------------------------------------------------------
def test_the_spec_on_a_case_worked_by_hand():
    S = 5
    #            0  1  2  3   4   5  6  7
    a = np.array([0, 0, 1, 1, -1, 2, 3, -2], np.int32)
    b = np.array([4, 4, 4, 1, 3, -1, -2, -1], np.int32)
    peri = np.tile(np.array([[10, 20]], np.int64), (S, 1))
    edges, weights, out = R.seam_stitch(a, b, S, peri)
    assert edges.tolist() == [[0, 4], [1, 4]] and weights.tolist() == [2, 1]
    # 0: two edges move.  1: one moves (faces 4), two only leave the border (1 faces 1, on both sides).  2: faces -1, "another label": moves.
    # 3: position 4 faces -1 (moves), position 6 faces -2 (stays border).  4: three edges move.
    assert out.tolist() == [[12, 18], [11, 17], [11, 19], [11, 19], [13, 17]]
    assert peri.tolist() == [[10, 20]] * S                         # the spec does not write its input
    e, w, out = R.seam_stitch(np.zeros(0, np.int32), np.zeros(0, np.int32), S, peri)
    assert e.shape == (0, 2) and w.shape == (0,) and np.array_equal(out, peri)


def test_the_spec_is_what_label_stats_and_rag_edges_of_the_oracle_say_about_a_cut_raster():
    """Cut a raster in two, run the oracle's label_stats / rag_edges on the halves and on the whole: the spec's stitch of the
    halves is the whole.  This ties the numpy spec to the definition (the per-tile results + the stitch = the one-raster results),
    ids outside [0, S) included."""
    from oracle import rag as OR
    rng = np.random.default_rng(5)
    H, W, S = 24, 30, 12
    lab = np.repeat(np.repeat(rng.integers(0, S, (6, 6)), 4, 0), 5, 1).astype(np.int32)
    lab[10:14, 13:17] = -1                                         # a hole that touches the seam
    lab[3, 14] = S + 3                                             # an id outside [0, S) on the seam
    img = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    # make the ids of the two halves disjoint, as a scene's are: right-half superpixel s becomes S + s
    cut = 15
    scene = lab.copy()
    right = scene[:, cut:]
    right[(right >= 0) & (right < S)] += S
    scene[3, 14] = -1                                              # the driver writes ids outside a tile's range as -1
    whole = OR.label_stats(scene, img, 2 * S)
    we, ww = OR.rag_edges(scene, 2 * S)
    left_l, right_l = scene[:, :cut].copy(), scene[:, cut:].copy()
    right_l[right_l >= 0] -= S
    ls, rs = OR.label_stats(left_l, img[:, :, :cut], S), OR.label_stats(right_l, img[:, :, cut:], S)
    peri = np.concatenate((ls["peri"], rs["peri"]))
    se, sw, fixed = R.seam_stitch(scene[:, cut - 1], scene[:, cut], 2 * S, peri)
    assert np.array_equal(fixed, whole["peri"])
    le, lw = OR.rag_edges(left_l, S)
    re_, rw = OR.rag_edges(right_l, S)
    edges = np.concatenate((le, re_ + S, se))
    weights = np.concatenate((lw, rw, sw))
    order = np.argsort(edges[:, 0].astype(np.int64) * 2 * S + edges[:, 1])
    assert np.array_equal(edges[order], we) and np.array_equal(weights[order], ww)
    assert len(se) >= 3 and (scene[:, cut - 1] == -1).any()
