"""GPU: rag.simplify(topology=True) and rag.simplify_conflicts (csrc/dm_simplify_topology.hip) against the numpy / Python-int spec
tests/simplify_topology_ref.py -- the flagged segments, the keep flags, every array of the repaired rings and arcs and the round
counts are bit-equal --, topology=False against today's rag.simplify, MergeResult.simplified and FeatureIO.save_shapefiles."""
import functools

import numpy as np
import pytest
import torch

import simplify_ref as S
import simplify_topology_ref as T
import vector_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = T.cases()
NAMES = list(CASES)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def traced(name):
    return V.trace(*CASES[name])


@functools.lru_cache(maxsize=None)
def spec(name, tol):
    labels, n = CASES[name]
    return T.simplify(labels, n, tol, traced(name))


def spec_conflicts(name, tol):
    return spec(name, tol)["conflicts"]


def assert_equals_spec(polys, arcs, keep, want):
    pairs = (("keep", keep, torch.uint8), ("region_ptr", polys.region_ptr, torch.int32), ("ring_ptr", polys.ring_ptr, torch.int64),
             ("xy", polys.xy, torch.int32), ("ring_label", polys.ring_label, torch.int32), ("ring_area2", polys.ring_area2, torch.int64),
             ("arc_ptr", arcs.arc_ptr, torch.int64), ("arc_xy", arcs.xy, torch.int32), ("left", arcs.left, torch.int32),
             ("right", arcs.right, torch.int32))
    for key, got, dtype in pairs:
        assert got.dtype == dtype, key
        g = got.cpu().numpy()
        assert g.shape == want[key].shape and np.array_equal(g, want[key]), key


@pytest.mark.parametrize("name", NAMES)
def test_conflicts_equal_the_spec(name):
    from deepmerge_amd import rag
    labels, n = CASES[name]
    t = dev(labels)
    for tol in T.TOLERANCES:
        want = spec_conflicts(name, tol)
        got = rag.simplify_conflicts(t, n, tol)
        print(f"{name} t={tol}: {labels.shape}, {want['n_segments']} segments, {len(want['kind'])} flagged, kinds {np.bincount(want['kind'], minlength=4).tolist()}")
        assert got.n_segments == want["n_segments"]
        for key, dtype in (("arc", torch.int32), ("xy", torch.int32), ("kind", torch.uint8)):
            g = getattr(got, key)
            assert g.dtype == dtype and g.shape == want[key].shape and np.array_equal(g.cpu().numpy(), want[key]), (tol, key)
    assert torch.equal(t.cpu(), torch.from_numpy(labels))


@pytest.mark.parametrize("name", NAMES)
def test_repaired_keep_rings_arcs_and_rounds_equal_the_spec(name):
    from deepmerge_amd import rag
    labels, n = CASES[name]
    t = dev(labels)
    for tol in T.TOLERANCES:
        want = spec(name, tol)
        stats = {}
        polys, arcs, keep = rag._simplify(t, n, tol, stats, topology=True)
        print(f"{name} t={tol}: rounds {stats['topology_rounds']}, flagged {stats['topology_flagged']}, kept arc vertices {stats['kept_arc_vertices']}")
        assert stats["topology_rounds"] == want["rounds"] and stats["topology_flagged"] == want["flagged"], tol
        assert_equals_spec(polys, arcs, keep, want)
    assert torch.equal(t.cpu(), torch.from_numpy(labels))


def test_a_cell_holds_more_segments_than_a_workgroup_and_a_segment_crosses_four_cells():
    # what the two cases are in the list for: 48 x 48 lies in four 32 x 32 cells, the first of them holds over 256 segments at
    # tolerance 1; long_bay's 0|1 segment at tolerance 20 is 198 corners long
    for name in ("noise48_7", "noise48_11"):
        labels, n = CASES[name]
        keep = S.keep_flags(labels, traced(name), S.quantise(1)).reshape(49, 49)
        segments, _ = T.scene_of(traced(name), keep)
        inside = sum(1 for s in segments if max(s["chain"][s["i"]] + s["chain"][s["j"]]) < 32)
        assert inside > 256
    want = spec_conflicts("long_bay", 20)
    assert max(abs(int(x1) - int(x0)) for x0, _, x1, _ in want["xy"]) >= 4 * 32 and (want["kind"] & 2).any()


@pytest.mark.parametrize("name", ["noise32_7", "long_bay", "smooth"])
def test_topology_false_is_todays_simplify_and_tolerance_zero_takes_no_round(name):
    from deepmerge_amd import rag
    labels, n = CASES[name]
    t = dev(labels)
    for tol in (0, 2.5):
        want = S.simplify(labels, n, tol, traced(name))
        polys, arcs, keep = rag._simplify(t, n, tol, topology=False)
        assert_equals_spec(polys, arcs, keep, want)
        polys, arcs = rag.simplify(t, n, tol)
        assert np.array_equal(polys.xy.cpu().numpy(), want["xy"]) and np.array_equal(arcs.xy.cpu().numpy(), want["arc_xy"])
    stats = {}
    polys, arcs, keep = rag._simplify(t, n, 0, stats, topology=True)
    assert stats["topology_rounds"] == 0 and stats["topology_flagged"] == [0]
    assert_equals_spec(polys, arcs, keep, S.simplify(labels, n, 0, traced(name)))
    assert rag.simplify_conflicts(t, n, 0).kind.numel() == 0


def test_max_rounds_raises():
    from deepmerge_amd import rag
    labels, n = CASES["noise32_7"]
    assert spec("noise32_7", 2.5)["rounds"] == 3
    with pytest.raises(RuntimeError, match="repair rounds"):
        rag.simplify(dev(labels), n, 2.5, topology=True, max_rounds=2)
    rag.simplify(dev(labels), n, 2.5, topology=True, max_rounds=3)
    with pytest.raises(ValueError, match="max_rounds"):
        rag.simplify(dev(labels), n, 2.5, topology=True, max_rounds=0)


@functools.lru_cache(maxsize=None)
def merged_case():
    """Pixels of a two-level noise tile merged by rag.mrs into blobs: (the start raster, the MergeResult, the merged labels)."""
    from deepmerge_amd import rag
    tile = (np.random.default_rng(31).integers(0, 2, (1, 24, 28)) * 200).astype(np.uint8).repeat(3, 0)
    start = dev(np.arange(24 * 28, dtype=np.int32).reshape(24, 28))
    res = rag.mrs(dev(tile), 20, labels=start, n_labels=24 * 28)
    return start, res, res.labels(start).cpu().numpy()


def test_merge_result_simplified_with_topology():
    from deepmerge_amd import rag
    start, res, merged = merged_case()
    C = int(res.rep.numel())
    assert 8 < C < 24 * 28
    want = T.simplify(merged, C, 2.5)
    assert want["rounds"] >= 1                                    # the plain result has conflicts here
    polys, arcs = res.simplified(start, 2.5, topology=True)
    for key, got in (("xy", polys.xy), ("ring_ptr", polys.ring_ptr), ("ring_area2", polys.ring_area2), ("arc_xy", arcs.xy), ("arc_ptr", arcs.arc_ptr)):
        assert np.array_equal(got.cpu().numpy(), want[key]), key
    assert np.array_equal(arcs.edge.cpu().numpy(), V.arc_edge(want["left"], want["right"], res.edges.cpu().numpy()))
    plain = res.simplified(start, 2.5)
    assert np.array_equal(plain[0].xy.cpu().numpy(), S.simplify(merged, C, 2.5)["xy"])
    traced_sign = np.sign(V.trace(merged, C)["ring_area2"])
    assert np.array_equal(np.sign(polys.ring_area2.cpu().numpy()), traced_sign) and int(polys.ring_area2.sum()) == 2 * 24 * 28


def test_save_shapefiles_with_topology_round_trips(tmp_path):
    from deepmerge_amd import rag, shpstore
    from deepmerge_amd.ExtractFeatures import FeatureIO
    labels, n = CASES["noise24_23"]
    H, W = labels.shape
    t = dev(labels)
    designed = rag.designed_features(rag.label_stats(t, torch.zeros((1, H, W), dtype=torch.uint8, device=DEV), n))
    pts = rag.sample_points(t, n, k=1)
    paths = FeatureIO.save_shapefiles(str(tmp_path / "safe"), t, n, pts, designed, tolerance=2.5, topology=True)
    want = spec("noise24_23", 2.5)
    assert want["rounds"] >= 1
    polys, lines = shpstore.ShapeReader(paths[0]), shpstore.ShapeReader(paths[1])
    assert len(polys) == n and len(lines) == len(want["left"])
    for l in range(n):                                           # X = x, Y = -y without a transform; a ring is closed by its first vertex
        rings = [want["xy"][want["ring_ptr"][r]:want["ring_ptr"][r + 1]] for r in range(want["region_ptr"][l], want["region_ptr"][l + 1])]
        assert len(polys.shapes[l]) == len(rings)
        for part, ring in zip(polys.shapes[l], rings):
            assert np.array_equal(part * (1, -1), np.concatenate((ring, ring[:1])).astype(np.float64))
    for a in range(len(lines)):
        assert np.array_equal(lines.shapes[a][0] * (1, -1), want["arc_xy"][want["arc_ptr"][a]:want["arc_ptr"][a + 1]].astype(np.float64))
    plain = FeatureIO.save_shapefiles(str(tmp_path / "plain"), t, n, pts, designed, tolerance=2.5)
    default = FeatureIO.save_shapefiles(str(tmp_path / "default"), t, n, pts, designed, tolerance=2.5, topology=False)
    for a, b in zip(plain, default):
        for ext in (".shp", ".shx", ".dbf"):
            assert open(a[:-4] + ext, "rb").read() == open(b[:-4] + ext, "rb").read(), (a, ext)
