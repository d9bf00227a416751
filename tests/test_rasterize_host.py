"""CPU: the rasterize spec (tests/rasterize_ref.py) against its own division-free predicate and against the tracing spec
(tests/vector_ref.py), shpstore.geo_to_corner / read_rings, and the argument checks of the C entries and of rag.rasterize that need
no GPU."""
import functools

import numpy as np
import pytest

import rasterize_ref as Z
import vector_ref as V

CASES = Z.cases()
NORTH_UP = (500000.0, 0.5, 0.0, 4100000.0, 0.0, -0.5)
ROTATED = (1200.0, 0.8, 0.3, -350.0, 0.25, -0.9)


@pytest.mark.parametrize("name", list(CASES))
def test_spec_equals_the_per_pixel_predicate(name):
    (ptr, xy, label), H, W = CASES[name]
    q = Z.quantise(xy)
    got = Z.rasterize(ptr, q, label, H, W)
    assert got.dtype == np.int32 and got.shape == (H, W)
    assert np.array_equal(got, Z.rasterize_by_predicate(ptr, q, label, H, W))
    assert np.array_equal(Z.rasterize(ptr, q, label, H, W, fill=-7), np.where(got < 0, -7, got))


def test_cases_are_what_their_names_say():
    r = {name: Z.rasterize(ptr, Z.quantise(xy), label, H, W) for name, ((ptr, xy, label), H, W) in CASES.items()}
    assert (r["fractional_triangle"] == 0).sum() > 20
    assert r["pentagram"][10, 10] == -1 and r["pentagram"][3, 10] == 0             # even-odd: the centre is left out
    hole = np.full((12, 13), -1, np.int32)
    hole[1:11, 1:11] = 2
    hole[4:8, 4:8] = -1
    assert np.array_equal(r["hole_same_orientation"], hole) and np.array_equal(r["hole_opposite_orientation"], hole)
    assert (r["half_outside"] == 0).any() and (r["half_outside"] == 1).any()
    assert (r["entirely_outside"] == -1).all() and (r["only_degenerate_rings"] == -1).all()
    # half-open rows: a vertex on a centre row counts once, a horizontal edge on one not at all
    # (the top vertex sits on the centre of row 0: both of its edges cross there at the same column, an empty span)
    assert np.array_equal(np.nonzero((r["vertex_on_centre_row"] == 0).any(1))[0], np.arange(1, 8))
    assert np.array_equal(np.nonzero(r["vertex_on_centre_row"][4] == 0)[0], np.arange(1, 9))      # the side vertices count once each
    rect = np.full((9, 9), -1, np.int32)
    rect[2:6, 1:7] = 0
    assert np.array_equal(r["horizontal_edge_on_centre_row"], rect)
    # the tie rule: column c is right of a crossing iff 256 c + 128 >= X, so a centre exactly on the shared diagonal (x == y) is right
    # of it and goes to label 1, the triangle on that side
    y, x = np.mgrid[0:9, 0:9]
    diag = np.where((x < 8) & (y < 8), np.where(x < y, 0, 1), -1)
    assert np.array_equal(r["diagonal_through_centres"], diag)
    only = np.full((9, 10), -1, np.int32)
    only[5:8, 6:9] = 5
    assert np.array_equal(r["degenerate_rings"], only)
    sq = np.full((10, 11), -1, np.int32)
    sq[3:8, 2:9] = 0
    assert np.array_equal(r["closing_vertex_repeated"], sq)
    assert np.array_equal(r["overlap_ab"], r["overlap_ba"]) and r["overlap_ab"][5, 5] == 5 and r["overlap_ab"][2, 2] == 3
    (ptr, xy, label), H, W = CASES["abutting_slanted"]
    assert (Z.claims(ptr, Z.quantise(xy), label, H, W) == 1).all()               # no gap, no double claim
    (ptr, xy, label), H, W = CASES["diagonal_through_centres"]
    assert (Z.claims(ptr, Z.quantise(xy), label, H, W)[:8, :8] == 1).all()
    (ptr, xy, label), H, W = CASES["sliver_tall"]
    q = Z.quantise(xy)
    assert len(Z.edge_events(*q[0], *q[1], H, W)[0]) == 700                    # one edge with an event in every row
    assert (r["sliver_tall"] == 0).any(1).sum() > 500 and np.array_equal(r["sliver_wide"], r["sliver_tall"].T)
    (ptr, xy, label), H, W = CASES["random_300"]
    outside = ((xy < 0) | (xy > (W, H))).any(1).mean()
    assert len(label) == 300 and 0.25 < outside < 0.45 and np.array_equal(np.round(xy * 256), xy * 256)
    assert len(np.unique(r["random_300"])) > 50


@functools.lru_cache(maxsize=None)
def _traced(name):
    labels, n = (V.comb_of_combs(130), 2) if name == "comb" else V.host_cases()[name]
    return labels, n, V.trace(labels, n)


@pytest.mark.parametrize("name", list(V.host_cases()) + ["comb"])
def test_spec_inverts_the_tracing_spec(name):
    labels, n, t = _traced(name)
    H, W = labels.shape
    got = Z.rasterize(t["ring_ptr"], 256 * t["xy"].astype(np.int64), t["ring_label"], H, W)
    assert np.array_equal(got, labels)
    assert np.array_equal(got, V.rasterise(t, H, W))
    assert np.array_equal(Z.quantise(t["xy"].astype(np.float64)), 256 * t["xy"].astype(np.int64))


def test_quantise():
    v = np.array([0.0, 1.0, -1.0, 0.5 / 256, -0.5 / 256, 1.49 / 256, -1.51 / 256, 3.25, 2.0 ** 20, -2.0 ** 20])
    assert Z.quantise(v).tolist() == [0, 256, -256, 1, 0, 1, -2, 832, 1 << 28, -(1 << 28)]


@pytest.mark.parametrize("gt", [None, NORTH_UP, ROTATED])
def test_geo_to_corner_inverts_corner_to_geo(gt):
    from deepmerge_amd import shpstore
    rng = np.random.default_rng(3)
    xy = np.concatenate((rng.integers(0, 5000, (200, 2)).astype(np.float64), np.round(rng.uniform(-50, 5000, (200, 2)) * 256) / 256))
    back = shpstore.geo_to_corner(gt, shpstore.corner_to_geo(gt, xy))
    assert back.dtype == np.float64 and back.shape == xy.shape
    assert np.array_equal(Z.quantise(back), np.round(256 * xy).astype(np.int64))


def test_geo_to_corner_refuses_a_singular_transform():
    from deepmerge_amd import shpstore
    with pytest.raises(ValueError, match="singular"):
        shpstore.geo_to_corner((0.0, 1.0, 2.0, 0.0, 2.0, 4.0), np.zeros((1, 2)))
    with pytest.raises(ValueError):
        shpstore.geo_to_corner((0.0, 1.0, 0.0), np.zeros((1, 2)))


class _Polys:                                                   # what write_polygons reads of a rag.Polygons
    def __init__(self, t):
        self.region_ptr, self.ring_ptr, self.xy = t["region_ptr"], t["ring_ptr"], t["xy"]


@pytest.mark.parametrize("gt", [None, NORTH_UP])
def test_read_rings_reads_what_write_polygons_wrote(tmp_path, gt):
    from deepmerge_amd import shpstore
    labels, n, t = _traced("absent_ids")                        # ids 0 and 3 of 6: four null shapes; label 0 has two rings
    H, W = labels.shape
    field = np.array([7, 1, 2, 0, 4, 5], np.int32)
    path = shpstore.write_polygons(str(tmp_path / "p.shp"), _Polys(t), [("LBL", field), ("w", np.arange(6.0))], gt)
    ptr, xy, label = shpstore.read_rings(path, gt)
    assert ptr.dtype == np.int64 and xy.dtype == np.float64 and label.dtype == np.int32
    assert label.tolist() == t["ring_label"].tolist() == [0, 0, 3]
    # every ring comes back with its closing vertex repeated
    assert np.array_equal(np.diff(ptr), np.diff(t["ring_ptr"]) + 1)
    for r in range(3):
        want = t["xy"][t["ring_ptr"][r]:t["ring_ptr"][r + 1]]
        assert np.array_equal(Z.quantise(xy[ptr[r]:ptr[r + 1]]), 256 * np.concatenate((want, want[:1])).astype(np.int64))
    assert np.array_equal(Z.rasterize(ptr, Z.quantise(xy), label, H, W), np.where(labels == 0, 0, 3))
    ptr2, xy2, label2 = shpstore.read_rings(path, gt, label_field="LBL")
    assert np.array_equal(ptr2, ptr) and np.array_equal(xy2, xy) and label2.tolist() == [7, 7, 0]
    assert shpstore._read_rings(path, gt, None)[3] == 6 and shpstore._read_rings(path, gt, "LBL")[3] == 8


def test_read_rings_errors(tmp_path):
    import struct
    from deepmerge_amd import shpstore
    labels, n, t = _traced("frame_island")
    polys = _Polys(t)
    lines = type("A", (), {"arc_ptr": t["arc_ptr"], "xy": t["arc_xy"]})()
    with pytest.raises(ValueError, match="not polygon"):
        shpstore.read_rings(shpstore.write_lines(str(tmp_path / "l.shp"), lines, []))
    path = shpstore.write_polygons(str(tmp_path / "p.shp"), polys, [("neg", np.array([0, -1])), ("big", np.array([0, (1 << 31) - 1], np.int64)),
                                                                    ("flt", np.array([0.0, 1.0])), ("txt", ["a", "b"])])
    with pytest.raises(ValueError, match="no field"):
        shpstore.read_rings(path, label_field="missing")
    for name, what in (("flt", "not an integer"), ("txt", "not an integer"), ("neg", "record 2"), ("big", "record 2")):
        with pytest.raises(ValueError, match=what):
            shpstore.read_rings(path, label_field=name)
    # a polygon part of one vertex, and a part of none
    one = struct.pack("<i4dii", shpstore.POLYGON, 0, 0, 0, 0, 1, 1) + struct.pack("<i", 0) + struct.pack("<2d", 1.0, 2.0)
    shpstore._write_shapes(str(tmp_path / "one.shp"), shpstore.POLYGON, [shpstore._multipart(shpstore.POLYGON, [np.zeros((4, 2))]), one], np.zeros((1, 2)))
    shpstore._write_dbf(str(tmp_path / "one.dbf"), [], 2, "regions")
    with pytest.raises(ValueError, match="record 2"):
        shpstore.read_rings(str(tmp_path / "one.shp"))
    none = struct.pack("<i4dii", shpstore.POLYGON, 0, 0, 0, 0, 1, 0) + struct.pack("<i", 0)
    shpstore._write_shapes(str(tmp_path / "none.shp"), shpstore.POLYGON, [none], np.zeros((1, 2)))
    shpstore._write_dbf(str(tmp_path / "none.dbf"), [], 1, "regions")
    with pytest.raises(ValueError, match="record 1"):
        shpstore.read_rings(str(tmp_path / "none.shp"))


@pytest.fixture(scope="module")
def built_lib():
    import os
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


def test_entries_validate_before_any_launch(built_lib):
    lib = built_lib.lib()
    p = 16                                                      # a non-null pointer that is never followed
    assert lib.dm_rasterize_count(None, p, p, 4, 1, 8, 8, p, None) == -1 and b"dm_rasterize_count: null pointer" in lib.dm_last_error()
    assert lib.dm_rasterize_count(p, p, p, 4, 1, 0, 8, p, None) == -1 and b"H=0" in lib.dm_last_error()
    assert lib.dm_rasterize_count(p, p, p, 4, 1, 8, 0, p, None) == -1 and b"W=0" in lib.dm_last_error()
    assert lib.dm_rasterize_emit(p, p, p, p, None, 4, 1, 6, 8, 8, 3, p, None) == -1 and b"dm_rasterize_emit: null pointer" in lib.dm_last_error()
    assert lib.dm_rasterize_emit(p, p, p, p, p, 4, 1, 6, 0, 8, 3, p, None) == -1 and b"H=0" in lib.dm_last_error()
    assert lib.dm_rasterize_emit(p, p, p, p, p, 4, 1, (1 << 30) + 1, 8, 8, 3, p, None) == -1 and b"2^30" in lib.dm_last_error()
    assert lib.dm_rasterize_emit(p, p, p, p, p, 4, 1, 6, 1 << 16, 1 << 15, 3, p, None) == -1          # H * W = 2^31
    assert b"H*W < 2^31" in lib.dm_last_error()
    assert lib.dm_rasterize_emit(p, p, p, p, p, 4, 1, 6, 8, 8, 1 << 31, p, None) == -1 and b"n_labels" in lib.dm_last_error()
    assert lib.dm_rasterize_fill(p, 6, 8, 8, -1, None, p, None) == -1 and b"dm_rasterize_fill: null pointer" in lib.dm_last_error()
    assert lib.dm_rasterize_fill(None, 6, 8, 8, -1, p, p, None) == -1 and b"null pointer" in lib.dm_last_error()
    assert lib.dm_rasterize_fill(p, 6, 0, 8, -1, p, p, None) == -1 and b"H=0" in lib.dm_last_error()
    assert lib.dm_rasterize_fill(p, 5, 8, 8, -1, p, p, None) == -1 and b"N even" in lib.dm_last_error()
    assert lib.dm_rasterize_fill(p, 6, 8, 8, 0, p, p, None) == -1 and b"fill < 0" in lib.dm_last_error()
    assert lib.dm_abi_version() == 7                            # the new symbols are additive


def test_rasterize_has_no_cpu_fallback(built_lib):
    import torch
    from deepmerge_amd import rag
    (ptr, xy, label), H, W = CASES["fractional_triangle"]
    rings = rag.Rings(torch.from_numpy(ptr), torch.from_numpy(xy), torch.from_numpy(label))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag.rasterize(rings, H, W)
