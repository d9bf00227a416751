"""CPU: the topology spec (tests/simplify_topology_ref.py) on hand-drawn rasters with known answers, its predicates on every
configuration the rule names, the properties the repair was observed to keep over small rasters, and the header / SIGNATURES /
argument checks of the dm_simplify_topology_* entries that need no GPU."""
import ctypes
import functools

import numpy as np
import pytest

import simplify_ref as S
import simplify_topology_ref as T
import vector_ref as V

CASES = T.cases()
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def traced(name):
    return V.trace(*CASES[name])


@functools.lru_cache(maxsize=None)
def plain(name, tol):
    labels, n = CASES[name]
    return S.simplify(labels, n, tol, traced(name))


@functools.lru_cache(maxsize=None)
def safe(name, tol):
    labels, n = CASES[name]
    return T.simplify(labels, n, tol, traced(name))


def arcs_of(r):
    return [[tuple(p) for p in r["arc_xy"][r["arc_ptr"][a]:r["arc_ptr"][a + 1]].tolist()] for a in range(len(r["left"]))]


def arc_between(r, right, left):
    return arcs_of(r)[[(int(a), int(b)) for a, b in zip(r["right"], r["left"])].index((right, left))]


def flagged(c):
    return {(int(a), tuple(int(v) for v in xy)): int(k) for a, xy, k in zip(c["arc"], c["xy"], c["kind"])}


# ---- known answers ---------------------------------------------------------------------------------------------------------------------
def test_bay_by_hand():
    # label 1 is a bar along the bottom and a 3 x 3 bay hanging into label 0, label 2 a one-pixel island in the bay's middle.  The
    # 0|1 chain is (5,4) (4,4) (4,1) (1,1) (1,4) (0,4).  (4,1) is 3 px from the chord (5,4)-(0,4): at tolerance 2.5 it stays, (1,1)
    # is 1.8 px from (4,1)-(0,4) and goes, and that segment's triangle (4,1) (1,1) (1,4) holds the island's anchor (2,2): kind 2.
    # From 3 px on the whole chain is the one segment (5,4)-(0,4), and the bay it cut off holds the island: kind 2 again.
    labels, n = T.bay()
    assert arc_between(plain("bay", 0), 0, 1) == [(5, 4), (4, 4), (4, 1), (1, 1), (1, 4), (0, 4)]
    assert arc_between(plain("bay", 2.5), 0, 1) == [(5, 4), (4, 1), (0, 4)]
    a01 = [(int(a), int(b)) for a, b in zip(traced("bay")["right"], traced("bay")["left"])].index((0, 1))
    a12 = [(int(a), int(b)) for a, b in zip(traced("bay")["right"], traced("bay")["left"])].index((1, 2))
    c = T.conflicts(labels, n, 2.5, traced("bay"))
    assert flagged(c) == {(a01, (4, 1, 0, 4)): 2, (a12, (2, 2, 2, 2)): 1} and c["n_segments"] == 9      # the island is degenerate
    for tol in (3.5, 5, 20):
        assert arc_between(plain("bay", tol), 0, 1) == [(5, 4), (0, 4)]
        assert flagged(T.conflicts(labels, n, tol, traced("bay"))) == {(a01, (5, 4, 0, 4)): 2, (a12, (2, 2, 2, 2)): 1}
    r = safe("bay", 2.5)
    assert r["rounds"] == 2 and r["flagged"] == [2, 2, 0]
    assert arc_between(r, 0, 1) == [(5, 4), (4, 1), (1, 1), (0, 4)]
    assert arc_between(r, 1, 2) == [(3, 2), (2, 2), (2, 3), (3, 3), (3, 2)]                            # the island is whole again


def test_bump_and_frame_island_by_hand():
    # bump at 1.0: the arc 0|1 (1,0) (1,1) (2,1) (2,0) loses both interior vertices (each 1 px from the chord) and lands on the frame
    # arc (1,0)-(2,0): the same two ends.  The frame arc has no interior vertex; the 0|1 segment gets (1,1) back (ties to the
    # smallest k), and (2,1), 1/sqrt(2) px from (1,1)-(2,0), stays out.
    labels, n = CASES["bump"]
    c = flagged(T.conflicts(labels, n, 1.0, traced("bump")))
    assert sorted(c.values()) == [1, 1] and {xy for _, xy in c} == {(1, 0, 2, 0)}
    r = safe("bump", 1.0)
    assert r["rounds"] == 1 and r["flagged"] == [2, 0] and arc_between(r, 0, 1) == [(1, 0), (1, 1), (2, 0)]
    assert r["ring_area2"].tolist() == [11, 1]
    # frame_island at 2.5: the island (1,1) (1,3) (3,3) (3,1) keeps (1,1) and (3,3), 2.83 px away: two segments with the same two
    # ends.  Both get their farthest vertex back: the island is whole.
    labels, n = CASES["frame_island"]
    c = flagged(T.conflicts(labels, n, 2.5, traced("frame_island")))
    assert c == {(1, (1, 1, 3, 3)): 1, (1, (3, 3, 1, 1)): 1}
    r = safe("frame_island", 2.5)
    assert r["rounds"] == 1 and r["flagged"] == [2, 0] and arcs_of(r)[1] == [(1, 1), (1, 3), (3, 3), (3, 1), (1, 1)]
    assert r["ring_area2"].tolist() == plain("frame_island", 0)["ring_area2"].tolist()
    r = safe("frame_island", 20)                                  # collapsed to its anchor: degenerate first, then as above
    assert r["flagged"] == [1, 2, 0] and arcs_of(r)[1] == [(1, 1), (1, 3), (3, 3), (3, 1), (1, 1)]


def test_meets_on_every_configuration_of_the_rule():
    m = T.meets
    assert m((0, 0), (4, 4), (0, 0), (4, 4)) and m((0, 0), (4, 4), (4, 4), (0, 0))                     # the same two ends, either order
    assert m((0, 0), (4, 4), (0, 4), (4, 0))                                                           # a proper crossing
    assert not m((0, 0), (4, 4), (0, 4), (1, 3))                                                       # the lines cross, the segments do not
    assert m((0, 0), (4, 4), (2, 2), (5, 0)) and m((2, 2), (5, 0), (0, 0), (4, 4))                     # an end inside the other (a T)
    assert not m((0, 0), (4, 4), (4, 4), (8, 0)) and not m((0, 0), (4, 4), (8, 0), (0, 0))             # a shared end alone
    assert not m((0, 0), (4, 4), (4, 4), (8, 8))                                                       # collinear, end to end
    assert m((0, 0), (4, 4), (2, 2), (8, 8)) and m((0, 0), (8, 8), (2, 2), (4, 4))                     # collinear overlap, containment
    assert m((0, 0), (4, 4), (0, 0), (2, 2)) and m((0, 0), (2, 2), (4, 4), (0, 0))                     # a shared end and the other end on it
    assert not m((0, 0), (4, 4), (6, 6), (8, 8)) and not m((0, 0), (4, 0), (0, 1), (4, 1))             # collinear apart, parallel
    assert not m((0, 0), (4, 4), (5, 5), (5, 0))                                                       # on the line, outside the box
    big = 32768
    assert m((0, 0), (big, big), (0, big), (big, 0)) and not m((0, 0), (big, 0), (big, 0), (big, big))
    assert m((0, 0), (big, big), (big // 2, big // 2), (big, 0)) and T.orient((0, 0), (big, 0), (0, big)) == 1 << 30


def test_even_odd_at_a_vertex_own_y():
    diamond = [(2, 0), (4, 2), (2, 4), (0, 2)]
    assert T.inside(diamond, (2, 2)) and T.inside(diamond, (1, 2)) and T.inside(diamond, (3, 2))       # y of the left and right vertices
    assert not T.inside(diamond, (5, 2)) and not T.inside(diamond, (-1, 2))
    assert not T.inside(diamond, (5, 0)) and not T.inside(diamond, (5, 4)) and not T.inside(diamond, (-1, 0))       # y of the top, the bottom
    square = [(0, 0), (4, 0), (4, 4), (0, 4)]                                                          # horizontal edges never count
    assert T.inside(square, (2, 2)) and not T.inside(square, (2, 4)) and T.inside(square, (2, 0)) and not T.inside(square, (4, 2))
    assert T.inside(square, (0, 2))                                                                    # half-open: the left side is in
    spike = [(0, 0), (6, 0), (6, 4), (3, 2), (0, 4)]                                                   # a reflex vertex at the point's own y
    assert T.inside(spike, (1, 2)) and T.inside(spike, (5, 2)) and not T.inside(spike, (3, 3)) and T.inside(spike, (3, 1))
    assert sorted(T.inside(spike, (x, 2)) for x in (-1, 7)) == [False, False]


# ---- the properties, on every raster and tolerance ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_repair_keeps_its_properties(name):
    labels, n = CASES[name]
    H, W = labels.shape
    t = traced(name)
    for tol in T.TOLERANCES:
        q, p, r = S.quantise(tol), plain(name, tol), safe(name, tol)
        keep = r["keep"].reshape(H + 1, W + 1)
        segments, fixed = T.scene_of(t, keep)
        assert not T.kinds(segments, fixed).any() and r["flagged"][-1] == 0                          # zero flags at the end
        assert ((r["keep"] > 0) >= (p["keep"] > 0)).all() and np.array_equal(r["keep"] == 2, p["keep"] == 2)     # kept(topology) >= kept(plain)
        for s in segments:                                                                           # removed vertices stay within the tolerance
            v = np.asarray(s["chain"], np.int64)
            e = v[s["j"]] - v[s["i"]]
            len2 = int(e[0] * e[0] + e[1] * e[1])
            for k in range(s["i"] + 1, s["j"]):
                rel = v[k] - v[s["i"]]
                d = int(rel[0] * rel[0] + rel[1] * rel[1]) if len2 == 0 else abs(int(e[0] * rel[1] - e[1] * rel[0]))
                assert not S.exceeds(d, len2, q), (tol, s["chain"][s["i"]], s["chain"][k], s["chain"][s["j"]])
        assert int(r["ring_area2"].sum()) == 2 * H * W
        assert (np.sign(r["ring_area2"]) == np.sign(t["ring_area2"])).all() and (r["ring_area2"] != 0).all()
        if r["rounds"] == 0:                                                                         # no conflict: the plain result, bit for bit
            assert len(r["conflicts"]["kind"]) == 0
            for key in p:
                assert np.array_equal(r[key], p[key]), key
        else:
            assert len(r["conflicts"]["kind"]) == r["flagged"][0] > 0 and r["rounds"] <= 4
        if tol == 0:
            assert r["rounds"] == 0
        print(f"{name} t={tol}: {len(segments)} segments, flagged per round {r['flagged']}, kept {int((p['keep'] > 0).sum())} -> {int((r['keep'] > 0).sum())}")


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("noise")] + ["bay"])
def test_the_cases_do_have_conflicts(name):
    for tol in T.TOLERANCES[1:]:
        assert len(safe(name, tol)["conflicts"]["kind"]) > 0, tol


def test_the_bays_carry_a_jump():
    for name in ("bay", "long_bay"):
        labels, n = CASES[name]
        for tol in (5, 20):
            assert (T.conflicts(labels, n, tol, traced(name))["kind"] & T.JUMPS).any()


def test_the_table_of_plain_failures():
    # what plain simplify leaves: (flagged segments, all segments, rings with zero or wrong-signed area, all rings)
    def row(name, tol):
        c, p, t = safe(name, tol)["conflicts"], plain(name, tol), traced(name)
        wrong = int(((p["ring_area2"] == 0) | (np.sign(p["ring_area2"]) != np.sign(t["ring_area2"]))).sum())
        return len(c["kind"]), c["n_segments"], wrong, len(p["ring_area2"])
    assert row("frame_island", 2.5)[2:] == (2, 3) and row("diagonal_holes", 1)[2:] == (3, 4) and row("bump", 1)[2:] == (1, 2)
    assert row("smooth", 1)[:3] == (4, 120, 2)
    assert row("noise32_7", 1) == (108, 438, 58, 164)


# ---- bindings ----------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("dm_simplify_topology_point_count", "dm_simplify_topology_point_fill", "dm_simplify_topology_segments",
           "dm_simplify_topology_bin_count", "dm_simplify_topology_bin_fill", "dm_simplify_topology_pairs", "dm_simplify_topology_jumps",
           "dm_simplify_topology_refine")


@pytest.fixture(scope="module")
def built_lib():
    import os
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


def test_header_signatures_and_exports_agree(built_lib):
    import re
    declared = built_lib.declared_symbols()
    lib = built_lib.lib()
    header = open(built_lib.HEADER_PATH).read()
    for name in ENTRIES:
        assert name in declared and name in built_lib.SIGNATURES and hasattr(lib, name)
        decl = header[header.index(f"int {name}("):]
        assert len(decl[decl.index("(") + 1:decl.index(")")].split(",")) == len(built_lib.SIGNATURES[name][1]), name
    body = header[header.index("typedef struct DmSimplifyTopology {"):header.index("} DmSimplifyTopology;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip(" *") for line in body.split("{")[1].split(";") for f in line.split(",") if f.strip()]
    names = [f.split()[-1].strip("*") for f in fields]
    assert names == [f[0] for f in built_lib.DmSimplifyTopology._fields_]                              # the struct, field for field
    assert ctypes.sizeof(built_lib.DmSimplifyTopology) == 16 * 8 + 2 * 8 + 4 * 4
    assert "#define DM_SIMPLIFY_TOPOLOGY_CELL_LOG2 5" in header
    assert lib.dm_abi_version() == 7                                                                   # the new symbols are additive
    from deepmerge_amd import rag
    assert callable(rag.simplify_conflicts) and rag.Conflicts.__dataclass_fields__.keys() == {"arc", "xy", "kind", "n_segments"}
    import inspect
    assert inspect.signature(rag.simplify).parameters["topology"].default is False
    assert inspect.signature(rag.simplify).parameters["max_rounds"].default == 64
    assert inspect.signature(rag.MergeResult.simplified).parameters["topology"].default is False
    from deepmerge_amd.ExtractFeatures import FeatureIO
    assert inspect.signature(FeatureIO.save_shapefiles).parameters["topology"].default is False


def test_entries_validate_before_any_launch(built_lib):
    lib = built_lib.lib()
    err = lib.dm_last_error
    p = 16                                                        # a non-null pointer that is never followed

    def table(**kw):
        t = built_lib.DmSimplifyTopology(**{f[0]: p for f in built_lib.DmSimplifyTopology._fields_[:16]}, Va=9, cap=64, A=3, H=8, W=8, q=256)
        for k, v in kw.items():
            setattr(t, k, v)
        return ctypes.byref(t)
    for name in ENTRIES:
        fn = getattr(lib, name)
        extra = (1,) if name.endswith("refine") else ()
        what = name.encode()
        assert fn(None, *extra, None) == -1 and what + b": null pointer" in err()
        assert fn(table(arc_xy=None), *extra, None) == -1 and what + b": null pointer" in err()
        assert fn(table(keep=None), *extra, None) == -1 and what + b": null pointer" in err()
        assert fn(table(H=0), *extra, None) == -1 and b"H=0" in err()
        assert fn(table(W=32769), *extra, None) == -1 and b"W=32769" in err() and b"32768" in err()
        assert fn(table(A=0), *extra, None) == -1 and b"A=0" in err()
        assert fn(table(Va=1), *extra, None) == -1 and b"Va=1" in err()
        assert fn(table(Va=(1 << 30) + 1), *extra, None) == -1 and b"2^30" in err()
        assert fn(table(q=-1), *extra, None) == -1 and b"q=-1" in err()
        assert fn(table(q=(1 << 20) + 1), *extra, None) == -1 and b"2^20" in err()
        if "point" not in name:
            assert fn(table(cap=0), *extra, None) == -1 and b"cap=0" in err()
            assert fn(table(cap=1 << 31), *extra, None) == -1 and b"cap=2147483648" in err()
            for field in ("new_ptr", "seg", "kind", "cell_count", "cell_fill", "status"):
                assert fn(table(**{field: None}), *extra, None) == -1 and what + b": null pointer" in err(), field
    for name, fields in (("point_fill", ("point_ptr", "point_xy")), ("bin_fill", ("cell_ptr", "cell_seg")), ("pairs", ("cell_ptr", "cell_seg")),
                         ("jumps", ("point_ptr", "point_xy"))):
        for field in fields:
            assert getattr(lib, "dm_simplify_topology_" + name)(table(**{field: None}), None) == -1 and b"null pointer" in err(), (name, field)
    assert lib.dm_simplify_topology_refine(table(stack=None), 1, None) == -1 and b"dm_simplify_topology_refine: null pointer" in err()


def test_topology_has_no_cpu_fallback(built_lib):
    import torch
    from deepmerge_amd import rag
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag.simplify(torch.zeros((4, 4), dtype=torch.int32), 1, 1.0, topology=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag.simplify_conflicts(torch.zeros((4, 4), dtype=torch.int32), 1, 1.0)
