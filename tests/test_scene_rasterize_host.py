"""CPU: the band and window form of the rasterisation rule (tests/scene_rasterize_ref.py) against the rule on the whole raster
(tests/rasterize_ref.py), whatever the tile and for unaligned boxes; the new C-ABI entry points refuse bad arguments before any
launch (csrc/dm_scene_rasterize.hip)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import rasterize_ref as Z
import scene_rasterize_ref as S

CASES = Z.cases()
WINDOW_CASES = S.window_cases()


@functools.lru_cache(maxsize=None)
def whole(name, fill=-1):
    (ptr, xy, label), H, W = CASES[name] if name in CASES else WINDOW_CASES[name][:3]
    return Z.rasterize(ptr, Z.quantise(xy), label, H, W, fill)


@pytest.mark.parametrize("name", list(CASES))
def test_every_tiling_equals_the_whole_raster(name):
    (ptr, xy, label), H, W = CASES[name]
    q = Z.quantise(xy)
    for tile in S.tilings(H, W):
        got = S.rasterize_tiled(ptr, q, label, H, W, tile)
        assert got.dtype == np.int32 and np.array_equal(got, whole(name)), (name, tile)


@pytest.mark.parametrize("name", list(CASES))
def test_unaligned_boxes_equal_the_slice_and_the_translated_rings(name):
    (ptr, xy, label), H, W = CASES[name]
    q = Z.quantise(xy)
    for box in S.boxes(H, W):
        y0, y1, x0, x1 = box
        got = S.read(ptr, q, label, H, W, box, fill=-4)
        assert np.array_equal(got, whole(name, -4)[y0:y1, x0:x1]), (name, box)
        assert np.array_equal(got, S.translated(ptr, q, label, box, fill=-4)), (name, box)


@pytest.mark.parametrize("name", list(WINDOW_CASES))
def test_where_a_window_can_go_wrong(name):
    (ptr, xy, label), H, W, tiles = WINDOW_CASES[name]
    q = Z.quantise(xy)
    for tile in tiles:
        assert np.array_equal(S.rasterize_tiled(ptr, q, label, H, W, tile), whole(name)), (name, tile)
    for box in S.boxes(H, W, n=3):
        y0, y1, x0, x1 = box
        assert np.array_equal(S.read(ptr, q, label, H, W, box), whole(name)[y0:y1, x0:x1]), (name, box)


def test_the_window_cases_hold_what_they_are_for():
    w = whole("three_columns")
    assert (w[10, 50:100] == 4).all() and (w[10, 100:131] == 4).all() and w[10, 0] == -1        # inside columns 1 and 2, the edge in column 0
    (ptr, xy, label), H, W, _ = WINDOW_CASES["events_on_window_edges"]
    cx = [S.edge_band_events(*e, 0, H, W)[1] for e in ((12928, 768, 12928, 5120), (12800, 9728, 12800, 11264), (25728, 6400, 25728, 8960))]
    assert [set(c.tolist()) for c in cx] == [{50}, {50}, {100}]
    w = whole("overlap_ab_across_seam")
    assert np.array_equal(w, whole("overlap_ba_across_seam")) and w[12, 49] == 5 and w[12, 50] == 5 and w[5, 50] == 3
    assert (whole("band_without_event")[16:] == -1).all() and (whole("no_rings") == -1).all() and (whole("empty_rings") == -1).all()
    w = whole("vertices_on_band_edge_rows")
    # a top vertex on a row centre gives that row two events at one column (an empty span), a bottom vertex gives its row none
    assert (w[8] != 0).all() and w[9, 20] == 0 and w[14, 20] == 0 and (w[15] != 0).all()
    assert (w[7] != 1).all() and w[8, 45] == 1 and w[15, 45] == 1 and (w[16] != 1).all()
    (ptr, xy, label), H, W, _ = WINDOW_CASES["vertices_on_band_edge_rows"]
    first = S.band_keys(ptr[:2], Z.quantise(xy[:4]), label[:1], H, W, 8, 16)       # the diamond from 8.5 to 15.5 in the band 8..15
    assert first.size == 2 * 7 and first[0] // (W + 1) == 0 and first[-1] // (W + 1) == 6        # rows 8..14: the first has its pair, the last none
    assert (w[7, 80:90] == 3).all() and (w[8, 80:90] == -1).all() and (w[15, 80:90] == 4).all() and (w[16, 80:90] == -1).all()
    w = whole("long_spans")
    assert (w[2, 1100:2300] == 9).all() and (w[2, 10:1100] == 6).all()


def test_an_unclosed_band_is_an_error_for_every_window():
    ptr, xy, label = Z.pack([(1, Z._square(2, 2, 8, 8))])
    keys = S.band_keys(ptr, Z.quantise(xy), label, 10, 40, 0, 10)
    assert keys.size == 12
    broken = np.sort(np.concatenate((keys[:-2], [keys[-2] + 41, keys[-1] + 2 * 41])))         # the last pair now names two rows
    for x0, x1 in ((0, 40), (0, 5), (20, 40)):                    # the last window meets no span of the band
        assert S.fill_window(keys, 0, 10, 40, x0, x1)[1] is False
        assert S.fill_window(broken, 0, 10, 40, x0, x1)[1] is True
    assert S.fill_window(np.array([-1, 5], np.int64), 0, 10, 40, 20, 40)[1] is True


def test_the_big_scene_stays_inside_the_spec_asserts():
    """H = W = 2^20: the products of the rule stay below 2^60 (the spec asserts it) for rings with vertices at +-2^20, in scene
    coordinates and translated to every box, and both formulations agree."""
    (ptr, xy, label), H, W, bx = S.big_scene()
    q = Z.quantise(xy)
    assert int(np.abs(q).max()) == 1 << 28 and int(label.max()) == (1 << 31) - 2
    seen = set()
    for box in bx:
        got = S.read(ptr, q, label, H, W, box)
        assert np.array_equal(got, S.translated(ptr, q, label, box)), box
        seen |= set(np.unique(got).tolist())
    assert seen == {-1, 3, 5, 7, 11, (1 << 31) - 2}


# ---- the entry points' refusals: no GPU, nothing is launched --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


def test_the_entry_points_refuse_before_any_launch(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                                     # non-null; never dereferenced: every call below is refused
    M = (1 << 31) - 1
    BAD = -1                                                      # DM_ERR_BAD_SHAPE

    def refused(code, *words):
        assert code == BAD
        msg = lib.dm_last_error()
        for w in words:
            assert w in msg, (w, msg)

    count = lambda **k: lib.dm_rasterize_count_rows(k.get("xy", p), p, p, k.get("V", 4), 1, k.get("H", 10), 10, k.get("r0", 0), k.get("r1", 10),
                                                    k.get("count", p), None)
    emit = lambda **k: lib.dm_rasterize_emit_rows(p, p, p, p, p, 4, 1, k.get("N", 8), k.get("H", 10), k.get("W", 10), k.get("r0", 0),
                                                  k.get("r1", 10), k.get("n_labels", 3), k.get("keys", p), None)
    fill = lambda **k: lib.dm_rasterize_fill_window(k.get("keys", p), k.get("N", 8), k.get("H", 10), k.get("W", 10), k.get("r0", 0), k.get("r1", 10),
                                                    k.get("x0", 0), k.get("x1", 10), k.get("fill", -1), k.get("out", p), k.get("error", p), None)
    refused(count(xy=None), b"dm_rasterize_count_rows", b"null pointer")
    refused(count(count=None), b"dm_rasterize_count_rows", b"null pointer")
    refused(emit(keys=None), b"dm_rasterize_emit_rows", b"null pointer")
    refused(fill(out=None), b"dm_rasterize_fill_window", b"null pointer")
    refused(fill(error=None), b"dm_rasterize_fill_window", b"null pointer")
    refused(fill(keys=None), b"dm_rasterize_fill_window", b"null pointer")             # N > 0 needs keys
    for call, name in ((count, b"dm_rasterize_count_rows"), (emit, b"dm_rasterize_emit_rows"), (fill, b"dm_rasterize_fill_window")):
        refused(call(r0=5, r1=5), name, b"bad band", b"r0 < r1")
        refused(call(r0=6, r1=5), name, b"bad band")
        refused(call(r0=-1, r1=5), name, b"bad band")
        refused(call(r0=0, r1=11), name, b"bad band")
        refused(call(H=0), name, b"bad band")
    refused(count(V=0), b"bad sizes")
    refused(count(V=(1 << 30) + 1), b"bad sizes", b"2^30")
    refused(emit(H=M, W=M, r0=0, r1=M, n_labels=M), b"key bound exceeded", b"2^63")
    refused(emit(H=M, W=M, r0=0, r1=1 << 12, n_labels=M), b"key bound exceeded")        # 2^31 2^12 2^31 > 2^63
    refused(emit(N=(1 << 30) + 1), b"bad sizes", b"2^30 events per band")
    refused(emit(N=0), b"bad sizes")
    refused(emit(n_labels=1 << 31), b"bad sizes", b"n_labels")
    refused(fill(N=(1 << 30) + 2), b"bad arguments", b"2^30")
    refused(fill(N=7), b"bad arguments", b"N even")
    refused(fill(fill=0), b"bad arguments", b"fill < 0")
    refused(fill(x0=4, x1=4), b"bad window", b"x0 < x1")
    refused(fill(x0=5, x1=4), b"bad window")
    refused(fill(x0=-1, x1=4), b"bad window")
    refused(fill(x0=0, x1=11), b"bad window")
    refused(fill(H=M, W=M, r0=0, r1=1 << 16, x0=0, x1=1 << 15), b"bad window", b"fewer than 2^31 pixels")
    refused(fill(H=M, W=M, r0=0, r1=M, x0=0, x1=M), b"bad window", b"fewer than 2^31 pixels")
