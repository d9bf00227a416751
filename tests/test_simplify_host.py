"""CPU: the simplify spec (tests/simplify_ref.py) on hand-drawn rasters with known answers and on its invariants over the rasters of
tests/vector_ref.py, and the header / SIGNATURES / argument checks of the dm_simplify_* entries that need no GPU."""
import functools

import numpy as np
import pytest

import simplify_ref as S
import vector_ref as V

TOLERANCES = (0, 0.5, 0.75, 1.5, 4, 4096)


def _random4(H, W, seed):
    return np.random.default_rng(seed).integers(0, 4, (H, W)).astype(np.int32), 4


@functools.lru_cache(maxsize=None)
def raster(name):
    for cases in (V.host_cases(), S.drawn_cases()):
        if name in cases:
            return cases[name]
    return {"comb": lambda: (V.comb_of_combs(), 2), "random_a": lambda: _random4(9, 11, 1), "random_b": lambda: _random4(17, 13, 2),
            "random_c": lambda: _random4(24, 24, 3)}[name]()


NAMES = list(V.host_cases()) + list(S.drawn_cases()) + ["comb", "random_a", "random_b", "random_c"]


@functools.lru_cache(maxsize=None)
def traced(name):
    labels, n = raster(name)
    return V.trace(labels, n)


@functools.lru_cache(maxsize=None)
def simplified(name, t):
    labels, n = raster(name)
    return S.simplify(labels, n, t, traced(name))


def arcs_of(r):
    return [[tuple(p) for p in r["arc_xy"][r["arc_ptr"][a]:r["arc_ptr"][a + 1]].tolist()] for a in range(len(r["left"]))]


def rings_of(r, key="xy"):
    return [[tuple(p) for p in r[key][r["ring_ptr"][a]:r["ring_ptr"][a + 1]].tolist()] for a in range(len(r["ring_label"]))]


def kept_at(r, name, x, y):
    return int(r["keep"][y * (raster(name)[0].shape[1] + 1) + x])


# ---- hand-drawn known answers -------------------------------------------------------------------------------------------------------
def test_quantise():
    assert [S.quantise(t) for t in (0, 0.5 / 256, 0.49 / 256, 0.7, 0.75, 1.5, 4096)] == [0, 1, 0, 179, 192, 384, 1 << 20]
    for bad in (-1e-9, float("nan"), float("inf"), 4096.01):
        with pytest.raises(ValueError):
            S.quantise(bad)


def test_one_step_stair_survives_0_7_and_goes_at_0_75():
    # the arc 0|1 is (1,0) (1,1) (2,1) between two frame nodes; its middle vertex sits 1/sqrt(2) = 0.7071 px from the chord
    for t, middle in ((0.7, [(1, 1)]), (0.75, [])):
        r = simplified("stair", t)
        a = [(int(x), int(y)) for x, y in zip(r["right"], r["left"])].index((0, 1))
        assert arcs_of(r)[a] == [(1, 0)] + middle + [(2, 1)]
        assert kept_at(r, "stair", 1, 1) == len(middle)
        assert rings_of(r)[1] == [(1, 0), (2, 0), (2, 1)] + middle           # label 1 sees the same vertices as label 0
        assert rings_of(r)[0] == [(0, 0), (1, 0)] + middle + [(2, 1), (2, 2), (0, 2)]
    assert simplified("stair", 0.75)["ring_area2"].tolist() == [7, 1]


def test_arg_max_ties_go_to_the_smallest_k():
    # the arc 0|1 is (1,0) (1,1) (2,1) (2,0): both interior vertices are 1 px from the chord.  The first is split off; the second
    # is then 1/sqrt(2) px from the chord (1,1) - (2,0) and goes at 0.75.  Ties to the greatest k would keep (2,1) and drop (1,1).
    assert S.farthest(np.array([(1, 0), (1, 1), (2, 1), (2, 0)], np.int64), 0, 3) == (1, 1)
    r = simplified("bump", 0.75)
    assert arcs_of(r)[1] == [(1, 0), (1, 1), (2, 0)]
    assert kept_at(r, "bump", 1, 1) == 1 and kept_at(r, "bump", 2, 1) == 0
    assert arcs_of(simplified("bump", 0.7))[1] == [(1, 0), (1, 1), (2, 1), (2, 0)]
    assert arcs_of(simplified("bump", 1.5))[1] == [(1, 0), (2, 0)]            # both within 1 px: the bump is gone
    assert rings_of(simplified("bump", 1.5))[1] == [(1, 0), (2, 0)] and simplified("bump", 1.5)["ring_area2"].tolist() == [12, 0]


def test_closed_island_collapses():
    # the island's arc is closed and has no node: it is anchored at (1,1), the smallest in (y, x); its stored start (2,1) lies inside
    # a straight run and is rotated away.  The farthest vertex (3,3) is sqrt(8) = 2.83 px from the anchor.
    assert arcs_of({k: traced("frame_island")[k] for k in ("arc_xy", "arc_ptr", "left")})[1][0] == (2, 1)
    assert arcs_of(simplified("frame_island", 0))[1] == [(1, 1), (1, 3), (3, 3), (3, 1), (1, 1)]
    assert kept_at(simplified("frame_island", 0), "frame_island", 2, 1) == 0 and kept_at(simplified("frame_island", 0), "frame_island", 1, 1) == 1
    assert arcs_of(simplified("frame_island", 1.5))[1] == [(1, 1), (3, 3), (1, 1)]
    r = simplified("frame_island", 4)
    assert arcs_of(r)[1] == [(1, 1), (1, 1)]
    assert rings_of(r) == [[(0, 0), (5, 0), (5, 4), (0, 4)], [(1, 1)], [(1, 1)]] and r["ring_area2"].tolist() == [40, 0, 0]


def test_t_junction_is_inserted_into_a_straight_ring_side():
    assert rings_of(traced("tee"))[0] == [(0, 0), (2, 0), (2, 1), (0, 1)]
    for t in TOLERANCES:
        r = simplified("tee", t)
        assert kept_at(r, "tee", 1, 1) == 2
        assert rings_of(r)[0] == [(0, 0), (2, 0), (2, 1), (1, 1), (0, 1)] and r["ring_area2"].tolist() == [4, 2, 2]


@pytest.mark.parametrize("name", ["diagonal_holes", "hole_meets_outside"])
def test_degree_four_corner_is_kept(name):
    for t in TOLERANCES:
        r = simplified(name, t)
        assert kept_at(r, name, 2, 2) == 2
        assert sum(p == (2, 2) for arc in arcs_of(r) for p in arc) >= 2
    if name == "diagonal_holes":                               # the kept arc runs through the corner unbroken and is cut there: two loops
        assert arcs_of(simplified(name, 0))[1] == [(2, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 2), (2, 2), (2, 1)]
        assert arcs_of(simplified(name, 4))[1] == [(2, 2), (2, 2), (2, 2)]


@pytest.mark.parametrize("name", NAMES)
def test_raster_corners_are_kept_at_4096(name):
    H, W = raster(name)[0].shape
    r = simplified(name, 4096)
    assert all(kept_at(r, name, x, y) == 2 for x in (0, W) for y in (0, H))
    frame = {p for ring in rings_of(r) for p in ring}
    assert {(x, y) for x in (0, W) for y in (0, H)} <= frame


# ---- properties -----------------------------------------------------------------------------------------------------------------------
def _turning(ring):
    n = len(ring)
    return [p for k, p in enumerate(ring) if not S._collinear(ring[k - 1], p, ring[(k + 1) % n])]


@pytest.mark.parametrize("name", NAMES)
def test_tolerance_zero_changes_nothing_but_starts_and_nodes(name):
    t, r = traced(name), simplified(name, 0)
    W = raster(name)[0].shape[1]
    node = lambda p: r["keep"][p[1] * (W + 1) + p[0]] == 2
    for before, after in zip(arcs_of(t), arcs_of(r)):
        if before[0] == before[-1] and not node(before[0]) and S._collinear(before[-2], before[0], before[1]):
            assert after == before[1:-1] + before[1:2]           # a non-turning closed-arc start is rotated away
        else:
            assert after == before
    for before, after in zip(rings_of(t), rings_of(r)):
        assert _turning(after) == before                        # the input ring, plus vertices inside its straight runs ...
        assert all(node(p) for p in set(after) - set(before))   # ... which are nodes
    assert np.array_equal(r["ring_area2"], t["ring_area2"])
    for key in ("left", "right", "ring_label", "region_ptr"):
        assert np.array_equal(r[key], t[key])


@pytest.mark.parametrize("name", NAMES)
def test_areas_sum_to_the_raster_for_every_tolerance(name):
    H, W = raster(name)[0].shape
    for t in TOLERANCES:
        r = simplified(name, t)
        assert r["ring_area2"].dtype == np.int64 and int(r["ring_area2"].sum()) == 2 * H * W, t
        assert [S.area2(ring) for ring in rings_of(r)] == r["ring_area2"].tolist()


@pytest.mark.parametrize("name", NAMES)
def test_removed_vertices_lie_within_the_tolerance(name):
    labels, n = raster(name)
    W = labels.shape[1]
    for t in TOLERANCES:
        q, r = S.quantise(t), simplified(name, t)
        keep = r["keep"].reshape(labels.shape[0] + 1, W + 1)
        for arc in arcs_of(traced(name)):
            for chain in S.chains_of(arc, keep)[0]:
                ends = [k for k, p in enumerate(chain) if keep[p[1], p[0]]]
                assert ends[0] == 0 and ends[-1] == len(chain) - 1
                v = np.asarray(chain, np.int64)
                for i, j in zip(ends[:-1], ends[1:]):           # every removed vertex against the kept pair that encloses it
                    e = v[j] - v[i]
                    len2 = int(e[0] * e[0] + e[1] * e[1])
                    for k in range(i + 1, j):
                        rel = v[k] - v[i]
                        d = int(rel[0] * rel[0] + rel[1] * rel[1]) if len2 == 0 else abs(int(e[0] * rel[1] - e[1] * rel[0]))
                        assert not S.exceeds(d, len2, q), (t, chain[i], chain[k], chain[j])


@pytest.mark.parametrize("name", NAMES)
def test_every_arc_vertex_is_in_the_rings_of_both_labels(name):
    for t in TOLERANCES:
        r = simplified(name, t)
        of_label = {}
        for label, ring in zip(r["ring_label"].tolist(), rings_of(r)):
            of_label.setdefault(label, set()).update(ring)
        for left, right, arc in zip(r["left"].tolist(), r["right"].tolist(), arcs_of(r)):
            assert set(arc) <= of_label[right] and (left < 0 or set(arc) <= of_label[left]), t
        n_arc = sum(len(a) - (a[0] == a[-1]) for a in arcs_of(r))
        assert all(len(a) >= 2 for a in arcs_of(r)) and all(len(g) >= 1 for g in rings_of(r))
        assert np.array_equal(np.nonzero(r["keep"] == 2)[0], np.nonzero(simplified(name, 0)["keep"] == 2)[0])      # nodes stay put
        assert n_arc >= 1


def test_splitting_order_does_not_matter():
    labels, n = raster("comb")
    chain = max(arcs_of(traced("comb")), key=len)
    assert len(chain) > 8192
    v = np.asarray(chain[:-1] if chain[0] == chain[-1] else chain, np.int64)
    for q in (192, 1024):
        kept, todo = [], [(0, len(v) - 1)]
        while todo:                                             # breadth first, where the spec goes depth first
            i, j = todo.pop(0)
            if j <= i + 1:
                continue
            k, d = S.farthest(v, i, j)
            e = v[j] - v[i]
            if S.exceeds(d, int(e[0] * e[0] + e[1] * e[1]), q):
                kept.append(k)
                todo += [(i, k), (k, j)]
        assert sorted(kept) == S.douglas_peucker([tuple(p) for p in v.tolist()], q)


def test_exceeds_is_exact_beyond_64_bits():
    d, len2, q = (1 << 30) - 1, (1 << 31) - 1, 1 << 20            # 65536 d^2 is about 2^76
    assert S.exceeds(d, len2, q) == (65536 * d * d > q * q * len2)
    assert S.exceeds(1 << 12, 1, 1 << 20) is False and S.exceeds((1 << 12) + 1, 1, 1 << 20) is True          # 2^16 d^2 against 2^40
    assert S.exceeds(1 << 24, 0, 1 << 20) is False and S.exceeds((1 << 24) + 1, 0, 1 << 20) is True          # coinciding ends: 2^16 d against 2^40


# ---- bindings ----------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("dm_simplify_nodes", "dm_simplify_chains", "dm_simplify_arc_count", "dm_simplify_arc_emit", "dm_simplify_ring_count",
           "dm_simplify_ring_emit")


@pytest.fixture(scope="module")
def built_lib():
    import os
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


def test_header_signatures_and_exports_agree(built_lib):
    declared = built_lib.declared_symbols()
    lib = built_lib.lib()
    for name in ENTRIES:
        assert name in declared and name in built_lib.SIGNATURES and hasattr(lib, name)
    header = open(built_lib.HEADER_PATH).read()
    for name in ENTRIES:                                        # one ctypes argument per declared parameter
        decl = header[header.index(f"int {name}("):]
        assert len(decl[decl.index("(") + 1:decl.index(")")].split(",")) == len(built_lib.SIGNATURES[name][1]), name
    assert "#define DM_SIMPLIFY_MAX_SIDE 32768" in header and "#define DM_SIMPLIFY_MAX_Q (1 << 20)" in header
    assert lib.dm_abi_version() == 7                            # the new symbols are additive
    from deepmerge_amd import rag
    assert callable(rag.simplify) and callable(rag.MergeResult.simplified)
    assert rag.MAX_SIMPLIFY_SIDE == S.MAX_SIDE == 32768 and rag.MAX_SIMPLIFY_Q == S.MAX_Q == 1 << 20


def test_entries_validate_before_any_launch(built_lib):
    lib = built_lib.lib()
    p = 16                                                      # a non-null pointer that is never followed
    err = lib.dm_last_error
    assert lib.dm_simplify_nodes(None, 8, 8, p, None) == -1 and b"dm_simplify_nodes: null pointer" in err()
    assert lib.dm_simplify_nodes(p, 0, 8, p, None) == -1 and b"H=0" in err()
    assert lib.dm_simplify_nodes(p, 8, 32769, p, None) == -1 and b"W=32769" in err() and b"32768" in err()
    assert lib.dm_simplify_chains(p, p, 3, 9, 8, 8, 256, p, None, None) == -1 and b"dm_simplify_chains: null pointer" in err()
    assert lib.dm_simplify_chains(p, p, 0, 9, 8, 8, 256, p, p, None) == -1 and b"A=0" in err()
    assert lib.dm_simplify_chains(p, p, 3, 1, 8, 8, 256, p, p, None) == -1 and b"Va=1" in err()
    assert lib.dm_simplify_chains(p, p, 3, (1 << 30) + 1, 8, 8, 256, p, p, None) == -1 and b"2^30" in err()
    assert lib.dm_simplify_chains(p, p, 3, 9, 32769, 8, 256, p, p, None) == -1 and b"H=32769" in err()
    assert lib.dm_simplify_chains(p, p, 3, 9, 8, 8, -1, p, p, None) == -1 and b"q=-1" in err()
    assert lib.dm_simplify_chains(p, p, 3, 9, 8, 8, (1 << 20) + 1, p, p, None) == -1 and b"2^20" in err()
    assert lib.dm_simplify_arc_count(p, p, 3, 9, 8, 8, None, p, None) == -1 and b"dm_simplify_arc_count: null pointer" in err()
    assert lib.dm_simplify_arc_count(p, p, 3, 9, 8, 0, p, p, None) == -1 and b"W=0" in err()
    assert lib.dm_simplify_arc_emit(p, p, None, 3, 9, 6, 8, 8, p, p, None) == -1 and b"dm_simplify_arc_emit: null pointer" in err()
    assert lib.dm_simplify_arc_emit(p, p, p, 3, 9, 0, 8, 8, p, p, None) == -1 and b"Vn=0" in err()
    assert lib.dm_simplify_arc_emit(p, p, p, 3, 9, 10, 8, 8, p, p, None) == -1 and b"Vn=10" in err()       # simplifying adds no vertex
    assert lib.dm_simplify_ring_count(p, p, None, 12, 3, 8, 8, p, p, None) == -1 and b"dm_simplify_ring_count: null pointer" in err()
    assert lib.dm_simplify_ring_count(p, p, p, 0, 3, 8, 8, p, p, None) == -1 and b"V=0" in err()
    assert lib.dm_simplify_ring_count(p, p, p, 2, 3, 8, 8, p, p, None) == -1 and b"R=3" in err()
    assert lib.dm_simplify_ring_emit(p, p, p, p, p, 12, 3, 12, 8, 8, p, p, None, None) == -1 and b"dm_simplify_ring_emit: null pointer" in err()
    assert lib.dm_simplify_ring_emit(p, p, p, None, p, 12, 3, 12, 8, 8, p, p, p, None) == -1 and b"null pointer" in err()
    assert lib.dm_simplify_ring_emit(p, p, p, p, p, 12, 3, 0, 8, 8, p, p, p, None) == -1 and b"Vn=0" in err()
    assert lib.dm_simplify_ring_emit(p, p, p, p, p, 12, 3, 12, 8, 40000, p, p, p, None) == -1 and b"W=40000" in err()


def test_simplify_has_no_cpu_fallback(built_lib):
    import torch
    from deepmerge_amd import rag
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag.simplify(torch.zeros((4, 4), dtype=torch.int32), 1, 1.0)
