"""CPU: the host side of scene.simplify_labels_topology.  Numpy only, against the ref modules: the facts
the sparse form of `keep` rests on still hold on REPAIRED flags, so the ring pass of 3.5.11 runs unchanged after a repair; the
sparse emit of the repaired flags is the spec's result; the flags do not depend on the cell side of the search grid; the driver's
choice of the cell side; then the validation of the eight new entries, which returns before any launch and needs no GPU."""
import ctypes
import functools
import os

import numpy as np
import pytest

import scene_simplify_topology_ref as G
import simplify_ref as S
import simplify_topology_ref as T
import vector_ref as V

CASES = T.cases()
CONFLICTED = ["bay", "long_bay", "noise32_7", "noise32_11", "noise48_7", "noise48_11", "noise24_23"]


@functools.lru_cache(maxsize=None)
def traced(name):
    return V.trace(*CASES[name])


@functools.lru_cache(maxsize=None)
def repaired(name, tol):
    labels, _ = CASES[name]
    keep, flagged, _ = T.repair(labels, traced(name), S.quantise(tol))
    return keep, flagged


@pytest.mark.parametrize("name", list(CASES))
def test_facts_1_and_3_hold_on_repaired_flags_and_the_sparse_emit_is_the_spec(name):
    labels, n = CASES[name]
    H, W = labels.shape
    t = traced(name)
    arc_ids = t["arc_xy"].astype(np.int64)[:, 1] * (W + 1) + t["arc_xy"].astype(np.int64)[:, 0]
    below = G.below_len(t)
    for tol in T.TOLERANCES:
        keep, flagged = repaired(name, tol)
        flat = keep.reshape(-1)
        plain = S.keep_flags(labels, t, S.quantise(tol)).reshape(-1)
        assert np.array_equal(flat == 2, plain == 2) and not ((plain == 1) & (flat != 1)).any()       # a repair only restores
        assert (len(flagged) > 1) == bool((flat != plain).any())
        # fact 1: a corner with keep == 1, restored ones included, is a stored vertex of exactly one arc, once below len
        arc_keep = G.arc_keep_of(t, keep, W)
        for corner in np.flatnonzero(flat == 1):
            at = np.flatnonzero((arc_ids == corner) & below)
            assert len(at) == 1 and arc_keep[at[0]] == 1, (tol, corner)
        assert int((arc_keep == 1).sum()) == int((flat == 1).sum())
        # fact 3: on a ring's run from v to its successor the kept corners strictly inside are exactly the nodes there
        nodes = set(np.flatnonzero(flat == 2).tolist())
        for r in range(len(t["ring_label"])):
            pts = t["xy"][t["ring_ptr"][r]:t["ring_ptr"][r + 1]].astype(np.int64)
            for (x0, y0), (x1, y1) in zip(pts, np.roll(pts, -1, 0)):
                sx, sy = np.sign(x1 - x0), np.sign(y1 - y0)
                for s in range(1, abs(x1 - x0) + abs(y1 - y0)):
                    corner = (y0 + s * sy) * (W + 1) + x0 + s * sx
                    assert (flat[corner] != 0) == (corner in nodes), (tol, r, corner)
        # so the sparse emit of the repaired flags is the spec's result, array for array
        want = T.emit(t, keep)
        got = G.emit(labels, t, keep, (37, 41))
        for key in ("arc_ptr", "arc_xy", "left", "right", "region_ptr", "ring_ptr", "xy", "ring_label", "ring_area2"):
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (tol, key)
        assert np.array_equal(got["kept_row"], np.flatnonzero(flat != 0))


def test_the_cases_hold_conflicts_and_several_rounds():
    assert all(len(repaired(name, 0)[1]) == 1 for name in CASES)                  # tolerance 0: one detection round, nothing flagged
    assert all(len(repaired(name, 20)[1]) > 1 for name in CONFLICTED)
    assert max(len(repaired(name, 20)[1]) - 1 for name in CONFLICTED) >= 2


@pytest.mark.parametrize("name", CONFLICTED)
def test_the_flags_do_not_depend_on_the_cell_side(name):
    """The spec tests every pair and every point.  Through a grid of 32-, 64- and 4096-corner cells the same segments are flagged
    with the same kinds: two segments that share a point share the cell of that point, and a fixed point inside a sub-chain's box
    is in a cell under the box."""
    labels, _ = CASES[name]
    t = traced(name)
    for tol in (1, 20):
        keep = S.keep_flags(labels, t, S.quantise(tol)).reshape(labels.shape[0] + 1, labels.shape[1] + 1)
        segments, fixed = T.scene_of(t, keep)
        want = T.kinds(segments, fixed)
        assert want.any()
        for log2 in (5, 6, 12):
            assert np.array_equal(G.grid_kinds(segments, fixed, log2), want), (tol, log2)


def test_the_walk_covers_the_cell_of_every_point_at_every_cell_side():
    rng = np.random.default_rng(5)
    far = (1 << 31) - 2
    for n in range(300):
        span = (40, 200, 2000, 32768)[n % 4]
        bx, by = ((0, 0), (far - span, far - span), (far - span, 0))[n % 3]
        x0, y0, x1, y1 = (int(v) for v in rng.integers(0, span + 1, 4))
        if n % 7 == 0:
            x1 = span                                            # ends at x = 2^31 - 2 when the base is far
        for log2 in (5, 6, 12, 20, 24):
            walked = G.walk_cells(bx + x0, by + y0, bx + x1, by + y1, log2)
            assert len(walked) == len(set(walked))
            if span <= 2000:
                assert G.cells_of_points(bx + x0, by + y0, bx + x1, by + y1, log2) <= set(walked), (n, log2)
            cols = {c[0] for c in walked}
            assert cols == set(range(min(bx + x0, bx + x1) >> log2, (max(bx + x0, bx + x1) >> log2) + 1))


def test_the_choice_of_the_cell_side():
    """The smallest log2 >= 5 at which ((H >> log2) + 1) ((W >> log2) + 1) <= 2^22.  Corner coordinates run to H and W included, so
    a side of exactly 65536 has 2049 cells of 32 corners and 2049^2 = 4198401 > 2^22 = 4194304: the 32-corner grid reaches
    65535 x 65535 and the 64-corner grid 131071 x 131071, one pixel short of the round figures; at the round figures the bound on
    the product, which the entries enforce, asks for the next side."""
    from deepmerge_amd import scene
    assert scene.MAX_TOPOLOGY_CELLS == G.MAX_CELLS == 1 << 22
    want = {(32768, 32768): 5, (65535, 65535): 5, (65536, 65536): 6, (131071, 131071): 6, (131072, 131072): 7, (1 << 29, (1 << 31) - 2): 20,
            (1, 1): 5, (7, 200): 5, ((1 << 31) - 2, 1): 9, ((1 << 31) - 2, 1 << 29): 20}
    for (H, W), log2 in want.items():
        got = scene.topology_cell_log2(H, W)
        assert got == log2 == G.cell_log2(H, W), (H, W, got)
        assert scene.topology_cells(H, W, got) == ((H >> got) + 1) * ((W >> got) + 1) <= 1 << 22
        assert got == 5 or scene.topology_cells(H, W, got - 1) > 1 << 22
    rng = np.random.default_rng(9)
    for _ in range(2000):
        H, W = (int(v) for v in 1 + rng.integers(0, 1 << int(rng.integers(1, 32)), 2) % ((1 << 31) - 2))
        if H * W > 1 << 60:
            continue
        got = scene.topology_cell_log2(H, W)
        assert 5 <= got <= 24 and got == G.cell_log2(H, W) and scene.topology_cells(H, W, got) <= 1 << 22


# ---- the entries: declared, bound, exported, and validating before any launch ---------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


ENTRIES = ("point_count", "point_fill", "segments", "bin_count", "bin_fill", "pairs", "jumps", "refine")
BAD_SHAPE = -1


def test_the_struct_binding_has_the_layout_of_the_header(built):
    t, d = built.DmSceneSimplifyTopology, built.DmSimplifyTopology
    assert [f[0] for f in t._fields_] == [("arc_keep" if f[0] == "keep" else f[0]) for f in d._fields_] + ["cell_log2"]
    assert [f[1] for f in t._fields_[:-1]] == [f[1] for f in d._fields_] and t._fields_[-1][1] is ctypes.c_int32
    assert ctypes.sizeof(t) == 16 * 8 + 2 * 8 + 6 * 4 and t.cell_log2.offset == 16 * 8 + 2 * 8 + 4 * 4
    header = open(built.HEADER_PATH).read()
    body = header[header.index("typedef struct DmSceneSimplifyTopology {"):header.index("} DmSceneSimplifyTopology;")]
    for name, _ in t._fields_:
        assert name in body, name
    assert built.lib().dm_abi_version() == 7


def test_every_entry_refuses_a_bad_struct_before_any_launch(built):
    lib = built.lib()
    i32, i64, u8 = (ctypes.c_int32 * 8)(), (ctypes.c_int64 * 8)(), (ctypes.c_uint8 * 8)()
    a32, a64, a8 = ctypes.addressof(i32), ctypes.addressof(i64), ctypes.addressof(u8)

    def struct(**kw):
        t = built.DmSceneSimplifyTopology(arc_xy=a32, arc_ptr=a64, new_ptr=a64, arc_keep=a8, point_count=a32, point_fill=a32, point_ptr=a64,
                                          point_xy=a32, seg=a32, kind=a32, cell_count=a32, cell_fill=a32, cell_ptr=a64, cell_seg=a32, stack=a64,
                                          status=a32, Va=9, cap=64, A=3, H=8, W=8, q=256, cell_log2=5)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def call(name, t):
        fn = getattr(lib, "dm_scene_simplify_topology_" + name)
        rc = fn(ctypes.byref(t), 1, None) if name == "refine" else fn(ctypes.byref(t), None)
        return rc, lib.dm_last_error().decode()

    side = (1 << 31) - 2
    bad = [(dict(arc_xy=None), "null pointer"), (dict(arc_ptr=None), "null pointer"), (dict(arc_keep=None), "null pointer"),
           (dict(point_count=None), "null pointer"), (dict(point_fill=None), "null pointer"),
           (dict(H=0), "H=0"), (dict(W=-1), "W=-1"), (dict(H=side + 1, cell_log2=24), "H=2147483647"), (dict(W=side + 1, cell_log2=24), "W=2147483647"),
           (dict(cell_log2=4), "cell_log2=4"), (dict(cell_log2=25), "cell_log2=25"), (dict(cell_log2=-1), "cell_log2=-1"),
           (dict(H=65536, W=65536), "cells=4198401"),                                   # 2049^2: one cell row and column too many
           (dict(H=side, W=side, cell_log2=5), f"cells={1 << 52}"),                      # (2^26)^2: only a 64-bit product sees it
           (dict(H=side, W=side, cell_log2=19), f"cells={4096 * 4096}"),
           (dict(A=0), "A=0"), (dict(A=1 << 30), "A=1073741824"), (dict(A=-5), "A=-5"), (dict(Va=1), "Va=1"), (dict(Va=(1 << 30) + 1), "2^30"),
           (dict(q=-1), "q=-1"), (dict(q=(1 << 20) + 1), "2^20")]
    tables = [(dict(cap=0), "cap=0"), (dict(cap=1 << 31), "cap=2147483648"), (dict(new_ptr=None), "null pointer"), (dict(seg=None), "null pointer"),
              (dict(kind=None), "null pointer"), (dict(cell_count=None), "null pointer"), (dict(cell_fill=None), "null pointer"),
              (dict(status=None), "null pointer")]
    own = {"point_fill": ("point_ptr", "point_xy"), "bin_fill": ("cell_ptr", "cell_seg"), "pairs": ("cell_ptr", "cell_seg"),
           "jumps": ("point_ptr", "point_xy"), "refine": ("stack",)}
    for name in ENTRIES:
        fn = getattr(lib, "dm_scene_simplify_topology_" + name)
        assert (fn(None, 1, None) if name == "refine" else fn(None, None)) == BAD_SHAPE
        for kw, text in bad + (tables if name not in ("point_count", "point_fill") else []):
            rc, message = call(name, struct(**kw))
            assert rc == BAD_SHAPE and text in message and "dm_scene_simplify_topology_" + name in message, (name, kw, message)
        for field in own.get(name, ()):
            rc, message = call(name, struct(**{field: None}))
            assert rc == BAD_SHAPE and "null pointer" in message, (name, field)
    # the widest scene is accepted by the arithmetic of the check itself at a side that fits: 2^29 x (2^31 - 2) at 2^20-corner cells
    from deepmerge_amd import scene
    assert scene.topology_cells(1 << 29, side, 20) == 513 * 2048 and scene.topology_cells(side, side, 20) == 2048 * 2048
