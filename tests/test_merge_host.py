"""CPU: the mutual-best-neighbour merge rule (tests/merge_ref.py, the spec of rag.merge_regions) -- known answers, invariants
and self-consistency on rasters -- and the argument validation of the merge entry points, which needs no GPU."""
import ctypes
import os

import numpy as np
import pytest

import merge_ref as M
from oracle import rag as OR


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    from oracle import sweep as OS
    strict = os.path.join(os.path.dirname(os.path.abspath(OS.__file__)), "_ref", "liboracle_sweep.so")
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(strict):
        g.build()
    return _lib


def line_graph(positions, edges, D=3):
    """One sample point per region on the first feature axis: simi of an edge = distance of its regions' positions."""
    S = len(positions)
    F = np.zeros((S, D), np.float32)
    F[:, 0] = positions
    return F, np.arange(S + 1, dtype=np.int32), np.arange(S, dtype=np.int32), np.asarray(edges, np.int32).reshape(-1, 2)


def test_path_merges_only_its_best_edge(built):
    """A-B-C with simi(A,B) < simi(B,C) < margin: round 1 merges (A,B) only -- the threshold rule would take all three at once."""
    F, ptr, idx, edges = line_graph([0.0, 0.25, 0.75], [(0, 1), (1, 2)])
    one = M.merge_regions_ref(F, ptr, idx, edges, 1.0, max_rounds=1)
    assert one["rounds"] == 1 and one["history"].tolist() == [[0, 0, 1]] and one["history_simi"].tolist() == [0.25]
    assert one["region_of"].tolist() == [0, 0, 1] and one["ptr"].tolist() == [0, 2, 3] and one["idx"].tolist() == [0, 1, 2]
    assert one["edges"].tolist() == [[0, 1]] and one["rep"].tolist() == [0, 2]
    assert one["simi"].tolist() == [0.625]                       # (A,B) pooled to 0.125, re-scored against C
    full = M.merge_regions_ref(F, ptr, idx, edges, 1.0)
    assert full["rounds"] == 2 and full["history"].tolist() == [[0, 0, 1], [1, 0, 2]] and full["regions_per_round"] == [3, 2, 1]
    assert full["edges"].shape == (0, 2) and full["simi"].shape == (0,)


def test_ties_go_to_the_smaller_neighbour_id(built):
    # region 1 sits exactly between 0 and 2: equal simi, its best neighbour is 0
    F, ptr, idx, edges = line_graph([0.0, 0.5, 1.0], [(0, 1), (1, 2)])
    r = M.merge_regions_ref(F, ptr, idx, edges, 1.0, max_rounds=1)
    assert r["history"].tolist() == [[0, 0, 1]]
    simi = np.array([0.5, 0.5, 0.5], np.float32)
    picked, best = M.pick_edges(simi, np.array([[0, 3], [1, 3], [2, 3]], np.int32), 4, 1.0)
    assert picked.tolist() == [True, False, False] and int(best[3]) & 0xFFFFFFFF == 0


def test_star_centre_takes_one_leaf_per_round(built):
    # centre 0 is every leaf's only (hence best) neighbour; it merges exactly one of them: its own best
    F, ptr, idx, edges = line_graph([0.0, 0.5, -0.25, 0.75], [(0, 1), (0, 2), (0, 3)])
    r = M.merge_regions_ref(F, ptr, idx, edges, 1.0, max_rounds=1)
    assert r["history"].tolist() == [[0, 0, 2]] and r["regions_per_round"] == [4, 3]
    assert r["edges"].tolist() == [[0, 1], [0, 2]]


def test_nan_edge_never_merges(built):
    F, ptr, idx, edges = line_graph([0.0, 0.25, 0.5], [(0, 1), (1, 2)])
    F[2, 1] = np.nan
    r = M.merge_regions_ref(F, ptr, idx, edges, 1.0)
    assert r["history"].tolist() == [[0, 0, 1]] and r["rounds"] == 1 and np.isnan(r["simi"]).all() and r["edges"].tolist() == [[0, 1]]
    picked, best = M.pick_edges(np.array([np.nan], np.float32), np.array([[0, 1]], np.int32), 2, 1.0)
    assert not picked.any() and (best == M.NO_BEST).all()


def test_duplicate_edges_fold_with_weights_added(built):
    # triangle 0-1-2 plus 3: merging (0,1) folds edges (0,2) and (1,2) into one with weight 5 + 7
    F, ptr, idx, edges = line_graph([0.0, 0.125, 5.0, 9.0], [(0, 1), (0, 2), (1, 2), (2, 3)])
    r = M.merge_regions_ref(F, ptr, idx, edges, 1.0, weights=np.array([3, 5, 7, 11], np.int32))
    assert r["edges"].tolist() == [[0, 1], [1, 2]] and r["weights"].tolist() == [12, 11] and r["rounds"] == 1


def test_min_regions_stops_before_the_round_and_history_is_a_prefix(built):
    F, ptr, idx, edges, w = M.random_graph(400, 1200, 8, 7)
    full = M.merge_regions_ref(F, ptr, idx, edges, 1.0, w)
    assert full["rounds"] >= 3
    for keep in (full["regions_per_round"][1], full["regions_per_round"][2] + 1, full["regions_per_round"][-1], 1):
        part = M.merge_regions_ref(F, ptr, idx, edges, 1.0, w, min_regions=keep)
        C = len(part["ptr"]) - 1
        assert C >= keep and C in full["regions_per_round"]
        k = part["rounds"]
        assert k == full["regions_per_round"].index(C)
        assert k == full["rounds"] or full["regions_per_round"][k + 1] < keep       # the next round would have gone below
        m = len(part["history"])
        assert np.array_equal(part["history"], full["history"][:m]) and np.array_equal(part["history_simi"], full["history_simi"][:m])
        assert np.array_equal(part["region_of"], full["maps"][k])
    capped = M.merge_regions_ref(F, ptr, idx, edges, 1.0, w, max_rounds=2)
    assert capped["rounds"] == 2 and np.array_equal(capped["region_of"], full["maps"][2])


@pytest.mark.parametrize("S,E,D", [(50, 120, 3), (700, 2500, 8), (3000, 9000, 100), (40, 0, 128)])
def test_spec_invariants_on_random_graphs(built, S, E, D):
    F, ptr, idx, edges, w = M.random_graph(S, E, D, S + E + D)
    r = M.merge_regions_ref(F, ptr, idx, edges, 1.0, w)
    assert all(M.is_matching(m) for m in r["matchings"])
    assert np.array_equal(np.sort(r["idx"]), np.arange(len(idx))) and r["ptr"][-1] == len(idx)
    with np.errstate(invalid="ignore"):
        assert not (r["simi"] < np.float32(1.0)).any()
    assert r["rounds"] == len(r["merges_per_round"]) and S - sum(r["merges_per_round"]) == len(r["ptr"]) - 1
    assert int(r["weights"].astype(np.int64).sum()) <= int(w.astype(np.int64).sum())
    for k in range(r["rounds"] + 1):
        assert np.array_equal(M.region_of_at(r["history"], r["merges_per_round"], S, k), r["maps"][k])
    assert np.array_equal(r["maps"][-1], r["region_of"])
    # rep = smallest original id of every region, regions numbered in that order
    first = np.full(len(r["rep"]), S, np.int64)
    np.minimum.at(first, r["region_of"], np.arange(S))
    assert np.array_equal(first, r["rep"]) and (np.diff(r["rep"]) > 0).all()
    if E:
        assert r["rounds"] >= 1


@pytest.mark.parametrize("H,W,cell,block", [(128, 128, 8, 4), (257, 301, 13, 3), (512, 512, 8, 8)])
def test_folded_graph_and_statistics_equal_those_of_the_relabelled_raster(built, H, W, cell, block):
    c = M.raster_case(H, W, cell, 3, block, 100, H + W)
    edges, w = OR.rag_edges(c["labels"], c["S"])
    st = OR.label_stats(c["labels"], c["tile"], c["S"])
    r = M.merge_regions_ref(c["F"], c["ptr"], c["idx"], edges, 1.0, w, st)
    C = len(r["ptr"]) - 1
    assert r["rounds"] >= 3 and C < c["S"] // 2                   # the inputs really iterate
    merged = r["region_of"][c["labels"]]
    e2, w2 = OR.rag_edges(merged, C)
    assert np.array_equal(e2, r["edges"]) and np.array_equal(w2, r["weights"])
    st2 = OR.label_stats(merged, c["tile"], C)
    for k in M.STAT_KEYS:
        assert np.array_equal(st2[k], r["stats"][k]), k
    assert all(M.is_matching(m) for m in r["matchings"])


# ---- the library's side, without a GPU ------------------------------------------------------------------------------------------
def test_merge_entry_points_validate_before_any_launch(built):
    from deepmerge_amd._lib import DmMergeFold
    lib = built.lib()
    assert lib.dm_abi_version() == 7
    p = 4096                                                       # any non-null address: validation never dereferences
    cases = [
        (lambda: lib.dm_merge_best(None, p, 4, 4, 1.0, p, None), b"dm_merge_best: null pointer"),
        (lambda: lib.dm_merge_best(p, p, 0, 4, 1.0, p, None), b"dm_merge_best: bad sizes"),
        (lambda: lib.dm_merge_best(p, p, 4, (1 << 24) + 1, 1.0, p, None), b"dm_merge_best: bad sizes"),
        (lambda: lib.dm_merge_match(p, p, 4, 4, p, None, p, p, None), b"dm_merge_match: null pointer"),
        (lambda: lib.dm_merge_match(p, p, 4, -1, p, p, p, p, None), b"dm_merge_match: bad sizes"),
        (lambda: lib.dm_merge_fold_regions(None, None), b"dm_merge_fold_regions: null argument"),
        (lambda: lib.dm_merge_fold_regions(ctypes.byref(DmMergeFold()), None), b"dm_merge_fold_regions: null pointer"),
        (lambda: lib.dm_merge_edge_keys(p, p, None, 4, 4, p, None), b"dm_merge_edge_keys: null pointer"),
        (lambda: lib.dm_merge_edge_keys(p, p, p, 0, 4, p, None), b"dm_merge_edge_keys: bad sizes"),
        (lambda: lib.dm_merge_fold_edges(None, p, p, 4, p, p, p, None), b"dm_merge_fold_edges: null pointer"),
        (lambda: lib.dm_merge_fold_edges(p, None, p, 4, p, p, p, None), b"dm_merge_fold_edges: weights need"),
        (lambda: lib.dm_merge_fold_edges(p, p, p, 0, p, p, p, None), b"dm_merge_fold_edges: bad size"),
        (lambda: lib.dm_relabel_raster(p, None, p, 16, 4, None), b"dm_relabel_raster: null pointer"),
        (lambda: lib.dm_relabel_raster(p, p, p, 0, 4, None), b"dm_relabel_raster: bad sizes"),
        (lambda: lib.dm_relabel_raster(p, p, p, 16, 0, None), b"dm_relabel_raster: bad sizes"),
    ]
    for call, msg in cases:
        assert call() == -1, msg
        assert msg in lib.dm_last_error(), (msg, lib.dm_last_error())
    f = DmMergeFold()
    for name, _ in DmMergeFold._fields_[:28]:
        setattr(f, name, p)
    f.count = None                                                 # no statistics
    f.C, f.P, f.E, f.S0, f.bands, f.round, f.hist_base, f.hist_cap = 0, 4, 4, 4, 0, 0, 0, 4
    assert lib.dm_merge_fold_regions(ctypes.byref(f), None) == -1 and b"bad sizes" in lib.dm_last_error()
    f.C, f.count, f.bands, f.new_sum = 4, p, 3, None
    assert lib.dm_merge_fold_regions(ctypes.byref(f), None) == -1 and b"statistics need" in lib.dm_last_error()


def test_merge_regions_has_no_cpu_fallback(built):
    import torch
    from deepmerge_amd import rag
    F, ptr, idx, edges, w = M.random_graph(20, 40, 8, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag.merge_regions(torch.from_numpy(F), torch.from_numpy(ptr), torch.from_numpy(idx), torch.from_numpy(edges))
    res = rag.MergeResult(region_of=torch.arange(4, dtype=torch.int32), ptr=None, idx=None, edges=None, weights=None, stats=None, pooled=None,
                          simi=None, rep=None, rounds=0, history=torch.zeros((0, 3), dtype=torch.int32),
                          history_simi=torch.zeros(0), regions_per_round=[4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        res.labels(torch.zeros((4, 4), dtype=torch.int32))
    assert res.region_of_at(0).tolist() == [0, 1, 2, 3]           # the replay is index arithmetic on whatever device holds the history
    with pytest.raises(ValueError):
        res.region_of_at(1)
