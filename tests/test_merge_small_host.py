"""CPU: the minimum-region-area rule of the merge (tests/merge_small_ref.py, the spec of `merge_regions(min_area=)` and
`mrs(min_area=)`) -- known answers on hand-made graphs, invariants on random graphs and rasters -- and the argument validation
of the Python and C entry points, which needs no GPU."""
import os

import numpy as np
import pytest

import merge_ref as M
import merge_small_ref as MS
import mrs_ref as R
from oracle import rag as OR

ALL_ONES = MS.NO_BEST


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    from oracle import sweep as OS
    strict = os.path.join(os.path.dirname(os.path.abspath(OS.__file__)), "_ref", "liboracle_sweep.so")
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(strict):
        g.build()
    return _lib


def name(best, r):
    return -1 if best[r] == ALL_ONES else int(best[r] & np.uint64(0xFFFFFFFF))


def pick(simi, edges, count, min_area):
    edges = np.asarray(edges, np.int32).reshape(-1, 2)
    return MS.pick_small(np.asarray(simi, np.float32), edges, len(count), np.asarray(count, np.int64), min_area)


def points_graph(positions, lens, edges, count):
    """Region r has lens[r] sample points at positions[r] on the first feature axis (simi of an edge = distance of the pooled
    positions) and count[r] pixels; the other statistics are any consistent integers."""
    S = len(positions)
    ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    F = np.zeros((int(ptr[-1]), 3), np.float32)
    F[:, 0] = np.repeat(np.asarray(positions, np.float32), lens)
    edges = np.asarray(edges, np.int32).reshape(-1, 2)
    return F, ptr, np.arange(int(ptr[-1]), dtype=np.int32), edges, np.ones(len(edges), np.int32), MS.graph_stats(S, 1, count=count)


def small_with_usable_edge(r, min_area):
    """Small regions of the result r that still have an edge with a score."""
    small = r["stats"]["count"] < min_area
    usable = r["simi"] == r["simi"]
    e = r["edges"][usable]
    return np.unique(np.concatenate((e[small[e[:, 0]], 0], e[small[e[:, 1]], 1])))


# ---- hand-made graphs ---------------------------------------------------------------------------------------------------------------
def test_chain_small_small_large_the_outer_one_waits_a_round(built):
    # 0 (small) - 1 (small) - 2 (large): 1 resembles 2 more than 0, so 0's proposal to 1 is not returned in round 1
    picked, best = pick([0.5, 0.25], [(0, 1), (1, 2)], [1, 1, 10], 5)
    assert picked.tolist() == [False, True] and [name(best, r) for r in range(3)] == [1, 2, 1]
    F, ptr, idx, edges, w, st = points_graph([0.0, 0.5, 0.75], [1, 1, 1], [(0, 1), (1, 2)], [1, 1, 10])
    r = MS.merge_regions_ref(F, ptr, idx, edges, 0.01, w, st, min_area=5)
    assert r["rounds"] == 2 and r["small_rounds"] == 2 and r["history"].tolist() == [[0, 1, 2], [1, 0, 1]]
    assert r["history_simi"].tolist() == [0.25, 0.625]            # (1, 2) pooled to 0.625: above the margin of 0.01, as allowed
    assert r["regions_per_round"] == [3, 2, 1] and r["stats"]["count"].tolist() == [12]


def test_large_hub_takes_one_small_leaf_per_round_smallest_key_first(built):
    picked, best = pick([4.0, 2.0, 3.0, 1.0], [(0, 1), (0, 2), (0, 3), (0, 4)], [100, 1, 1, 1, 1], 5)
    assert picked.tolist() == [False, False, False, True] and name(best, 0) == 4
    assert [name(best, r) for r in range(1, 5)] == [0, 0, 0, 0]   # every leaf proposed; the hub accepted one
    F, ptr, idx, edges, w, st = points_graph([0.0, 4.0, 2.0, 3.0, 1.0], [64, 1, 1, 1, 1], [(0, 1), (0, 2), (0, 3), (0, 4)],
                                             [100, 1, 1, 1, 1])
    r = MS.merge_regions_ref(F, ptr, idx, edges, 0.01, w, st, min_area=5)
    assert r["history"].tolist() == [[0, 0, 4], [1, 0, 2], [2, 0, 3], [3, 0, 1]] and r["small_rounds"] == 4 == r["rounds"]
    assert all(M.is_matching(m) for m in r["matchings"]) and r["merges_per_round"] == [1, 1, 1, 1]


def test_two_small_regions_that_propose_to_each_other_merge(built):
    picked, best = pick([0.125, 0.5], [(0, 1), (1, 2)], [1, 1, 10], 5)
    assert picked.tolist() == [True, False]
    assert name(best, 0) == 1 and name(best, 1) == 0 and best[2] == ALL_ONES     # nobody proposed to the large region
    # a small region that proposes to a small region which proposes to a third small one waits
    picked, best = pick([0.5, 0.25, 0.125], [(0, 1), (1, 2), (2, 3)], [1, 1, 1, 1], 5)
    assert picked.tolist() == [False, False, True] and [name(best, r) for r in range(4)] == [1, 2, 3, 2]


def test_ties_go_to_the_smaller_id_on_both_sides(built):
    # propose: small 3 has three equal edges to large regions and names 0; accept: large 0 has three equal proposers and names 1
    picked, best = pick([0.5, 0.5, 0.5], [(0, 3), (1, 3), (2, 3)], [9, 9, 9, 1], 5)
    assert name(best, 3) == 0 and picked.tolist() == [True, False, False]
    assert best[1] == ALL_ONES and best[2] == ALL_ONES
    picked, best = pick([0.5, 0.5, 0.5], [(0, 1), (0, 2), (0, 3)], [9, 1, 1, 1], 5)
    assert name(best, 0) == 1 and picked.tolist() == [True, False, False]
    # the key orders by simi first: a smaller simi beats a smaller id, on both sides
    picked, best = pick([0.5, 0.25], [(0, 2), (1, 2)], [9, 9, 1], 5)
    assert name(best, 2) == 1 and picked.tolist() == [False, True]
    picked, best = pick([0.5, 0.25], [(0, 1), (0, 2)], [9, 1, 1], 5)
    assert name(best, 0) == 2 and picked.tolist() == [False, True]


def test_count_equal_to_min_area_is_not_small(built):
    picked, best = pick([0.5], [(0, 1)], [5, 9], 5)
    assert not picked.any() and (best == ALL_ONES).all()
    picked, best = pick([0.5], [(0, 1)], [4, 9], 5)
    assert picked.tolist() == [True]
    picked, best = pick([0.5], [(0, 1)], [(1 << 40) - 1, 1 << 41], 1 << 40)      # int64 all the way
    assert picked.tolist() == [True]
    picked, best = pick([0.5], [(0, 1)], [1 << 40, 1 << 41], 1 << 40)
    assert not picked.any()


def test_scores_of_zero_and_infinity_are_usable_nan_is_not(built):
    picked, best = pick([np.inf, 0.0, np.nan], [(0, 1), (0, 2), (0, 3)], [9, 1, 1, 1], 5)
    assert picked.tolist() == [False, True, False] and name(best, 1) == 0 and best[3] == ALL_ONES
    picked, best = pick([np.inf], [(0, 1)], [9, 1], 5)
    assert picked.tolist() == [True]


def test_small_region_whose_only_edge_is_nan_and_empty_region_without_edges_stay(built):
    # 0 large - 1 small (scored), 2 small with a NaN feature (its only edge scores NaN), 3: no pixels, no points, no edges
    F, ptr, idx, edges, w, st = points_graph([0.0, 0.5, 0.75, 0.0], [1, 1, 1, 0], [(0, 1), (0, 2)], [10, 1, 1, 0])
    F[2, 1] = np.nan
    r = MS.merge_regions_ref(F, ptr, idx, edges, 0.01, w, st, min_area=5)
    assert r["history"].tolist() == [[0, 0, 1]] and r["small_rounds"] == 1 and r["rep"].tolist() == [0, 2, 3]
    assert r["stats"]["count"].tolist() == [11, 1, 0] and np.isnan(r["simi"]).all() and r["edges"].tolist() == [[0, 1]]
    assert len(small_with_usable_edge(r, 5)) == 0


def test_min_regions_drops_the_elimination_round_that_would_go_below_it(built):
    F, ptr, idx, edges, w, st = points_graph([0.0, 4.0, 2.0, 3.0, 1.0], [64, 1, 1, 1, 1], [(0, 1), (0, 2), (0, 3), (0, 4)],
                                             [100, 1, 1, 1, 1])
    r = MS.merge_regions_ref(F, ptr, idx, edges, 0.01, w, st, min_area=5, min_regions=3)
    assert r["rounds"] == 2 == r["small_rounds"] and r["regions_per_round"] == [5, 4, 3] and len(small_with_usable_edge(r, 5)) == 2
    # a round is dropped whole: two disjoint pairs would take 6 regions to 4, below 5
    F, ptr, idx, edges, w, st = points_graph([0.0, 1.0, 10.0, 11.0, 20.0, 30.0], [1] * 6, [(0, 1), (2, 3), (3, 4), (4, 5)],
                                             [9, 1, 9, 1, 9, 9])
    r = MS.merge_regions_ref(F, ptr, idx, edges, 0.01, w, st, min_area=5, min_regions=5)
    assert r["rounds"] == 0 and r["small_rounds"] == 0 and r["regions_per_round"] == [6]
    r = MS.merge_regions_ref(F, ptr, idx, edges, 0.01, w, st, min_area=5, min_regions=4)
    assert r["rounds"] == 1 and r["history"].tolist() == [[0, 0, 1], [0, 2, 3]]


def test_max_rounds_counts_both_phases_and_phase_one_ending_there_means_no_phase_two(built):
    F, ptr, idx, edges, w = M.random_graph(400, 1200, 8, 7)
    st = MS.graph_stats(400, 7)
    full = MS.merge_regions_ref(F, ptr, idx, edges, 1.0, w, st, min_area=30)
    p1 = full["rounds"] - full["small_rounds"]
    assert p1 >= 3 and full["small_rounds"] >= 2
    for cap in (0, 2, p1):                                        # p1: the round that would have found nothing is not run
        r = MS.merge_regions_ref(F, ptr, idx, edges, 1.0, w, st, min_area=30, max_rounds=cap)
        assert r["rounds"] == cap and r["small_rounds"] == 0 and np.array_equal(r["region_of"], full["maps"][cap])
    r = MS.merge_regions_ref(F, ptr, idx, edges, 1.0, w, st, min_area=30, max_rounds=p1 + 1)
    assert r["rounds"] == p1 + 1 and r["small_rounds"] == 1 and np.array_equal(r["region_of"], full["maps"][p1 + 1])
    # min_regions reached in phase 1: no phase 2 either
    keep = full["regions_per_round"][2]
    r = MS.merge_regions_ref(F, ptr, idx, edges, 1.0, w, st, min_area=30, min_regions=keep)
    assert r["rounds"] == 2 and r["small_rounds"] == 0


# ---- invariants -----------------------------------------------------------------------------------------------------------------------
def check_invariants(r, base, S0, min_area):
    p1 = r["rounds"] - r["small_rounds"]
    assert p1 == base["rounds"] and np.array_equal(r["maps"][p1], base["region_of"])
    m = len(base["history"])
    assert np.array_equal(r["history"][:m], base["history"]) and np.array_equal(r["history_simi"][:m], base["history_simi"])
    assert r["regions_per_round"][:p1 + 1] == base["regions_per_round"] and r["merges_per_round"][:p1] == base["merges_per_round"]
    assert all(M.is_matching(e) for e in r["matchings"])
    assert len(small_with_usable_edge(r, min_area)) == 0
    for k in range(r["rounds"] + 1):                               # the replay crosses the phase boundary
        assert np.array_equal(M.region_of_at(r["history"], r["merges_per_round"], S0, k), r["maps"][k])
    assert S0 - sum(r["merges_per_round"]) == len(r["ptr"]) - 1 and int(r["stats"]["count"].sum()) == int(base["stats"]["count"].sum())


@pytest.mark.parametrize("S,E,D", [(50, 120, 8), (700, 2500, 8), (3000, 9000, 16)])
def test_spec_invariants_on_random_graphs(built, S, E, D):
    F, ptr, idx, edges, w = M.random_graph(S, E, D, S + E + D)
    st = MS.graph_stats(S, S)
    base = M.merge_regions_ref(F, ptr, idx, edges, 1.0, w, st)
    zero = MS.merge_regions_ref(F, ptr, idx, edges, 1.0, w, st, min_area=0)
    assert zero.pop("small_rounds") == 0 and sorted(zero) == sorted(base)
    for k in base:                                                # min_area = 0 is merge_ref's run, field for field
        if k == "stats":
            assert all(np.array_equal(zero[k][s], base[k][s]) for s in M.STAT_KEYS)
        elif k in ("maps", "matchings"):
            assert len(zero[k]) == len(base[k]) and all(np.array_equal(x, y) for x, y in zip(zero[k], base[k]))
        elif isinstance(base[k], np.ndarray):
            assert zero[k].dtype == base[k].dtype and np.array_equal(zero[k], base[k], equal_nan=base[k].dtype.kind == "f"), k
        else:
            assert zero[k] == base[k], k
    for min_area in (1, 30, 10 ** 9):
        r = MS.merge_regions_ref(F, ptr, idx, edges, 1.0, w, st, min_area=min_area)
        check_invariants(r, base, S, min_area)
        if min_area == 1:
            assert r["small_rounds"] == 0                         # no region has count < 1 here
        if min_area == 30:
            assert r["small_rounds"] >= 1


@pytest.mark.parametrize("H,W,cell,block", [(96, 112, 8, 3), (200, 232, 13, 3)])
def test_spec_invariants_on_rasters_with_outlier_superpixels(built, H, W, cell, block):
    c = M.raster_case(H, W, cell, 3, block, 16, H + W)
    F = MS.add_outliers(c, 0.15, H)
    edges, w = OR.rag_edges(c["labels"], c["S"])
    st = OR.label_stats(c["labels"], c["tile"], c["S"])
    base = M.merge_regions_ref(F, c["ptr"], c["idx"], edges, 1.0, w, st)
    left = int((base["stats"]["count"] < 2 * cell * cell).sum())
    assert left > c["S"] // 20                                    # the outliers are still single superpixels after the margin rounds
    for min_area in (1, 2 * cell * cell, 10 ** 9):
        r = MS.merge_regions_ref(F, c["ptr"], c["idx"], edges, 1.0, w, st, min_area=min_area)
        check_invariants(r, base, c["S"], min_area)
        C = len(r["ptr"]) - 1
        merged = r["region_of"][c["labels"]]
        e2, w2 = OR.rag_edges(merged, C)
        assert np.array_equal(e2, r["edges"]) and np.array_equal(w2, r["weights"])
        st2 = OR.label_stats(merged, c["tile"], C)
        assert all(np.array_equal(st2[k], r["stats"][k]) for k in M.STAT_KEYS)
    assert r["small_rounds"] >= 3 and np.sum(r["stats"]["count"] > 0) == 1        # min_area = 10^9: one region holds every pixel


def test_mrs_spec_with_min_area(built):
    tile = R.quadrant_tile()
    base = R.mrs_ref(tile, 5.0)
    zero = MS.mrs_ref(tile, 5.0)
    assert zero["small_rounds"] == 0 and np.array_equal(zero["region_of"], base["region_of"]) and zero["rounds"] == base["rounds"]
    assert np.array_equal(zero["history"], base["history"]) and np.array_equal(zero["simi"], base["simi"])
    assert (base["stats"]["count"] < 12).sum() >= 10              # the pixel start leaves single pixels and specks
    r = MS.mrs_ref(tile, 5.0, min_area=12)
    check_invariants(r, base, tile.shape[1] * tile.shape[2], 12)
    assert r["small_rounds"] >= 2 and int(r["stats"]["count"].min()) >= 12


# ---- the product's side, without a GPU ---------------------------------------------------------------------------------------------
def test_min_area_is_checked_before_any_device_work(built):
    import torch
    from deepmerge_amd import rag
    F, ptr, idx, edges, w = M.random_graph(20, 40, 8, 1)
    t = [torch.from_numpy(x) for x in (F, ptr, idx, edges)]       # CPU tensors: anything that got past the check would raise
    st = {k: torch.from_numpy(v) for k, v in MS.graph_stats(20, 1).items()}       # RuntimeError("... no CPU fallback")
    st["bands"] = 3
    for bad in (-1, 2.0, 1.5, "4", None, 1 << 63):
        with pytest.raises(ValueError, match="min_area"):
            rag.merge_regions(*t, weights=torch.from_numpy(w), stats=st, min_area=bad)
        with pytest.raises(ValueError, match="min_area"):
            rag.mrs(torch.zeros((3, 8, 8), dtype=torch.uint8), 10.0, min_area=bad)
        with pytest.raises(ValueError, match="min_area"):
            rag.mrs_graph(st, t[3], torch.from_numpy(w), 10.0, min_area=bad)
    with pytest.raises(ValueError, match="min_area needs stats"):
        rag.merge_regions(*t, min_area=4)
    with pytest.raises(ValueError, match="min_area needs stats"):
        rag.merge_regions(*t, weights=torch.from_numpy(w), min_area=np.int64(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # a good value gets as far as min_area = 0 does
        rag.merge_regions(*t, weights=torch.from_numpy(w), stats=st, min_area=4)
    res = rag.MergeResult(region_of=torch.arange(4, dtype=torch.int32), ptr=None, idx=None, edges=None, weights=None, stats=None, pooled=None,
                          simi=None, rep=None, rounds=0, history=torch.zeros((0, 3), dtype=torch.int32),
                          history_simi=torch.zeros(0), regions_per_round=[4])
    assert res.small_rounds == 0


def test_small_entry_points_validate_before_any_launch(built):
    lib = built.lib()
    assert lib.dm_abi_version() == 7
    p = 4096                                                       # any non-null address: validation never dereferences
    for fn, tag in ((lib.dm_merge_best_small, b"dm_merge_best_small"), (lib.dm_merge_accept, b"dm_merge_accept")):
        cases = [((None, p, 4, 4, p, 5, p, None), b"null pointer"), ((p, None, 4, 4, p, 5, p, None), b"null pointer"),
                 ((p, p, 4, 4, None, 5, p, None), b"null pointer"), ((p, p, 4, 4, p, 5, None, None), b"null pointer"),
                 ((p, p, 0, 4, p, 5, p, None), b"bad sizes"), ((p, p, 4, 0, p, 5, p, None), b"bad sizes"),
                 ((p, p, 4, (1 << 24) + 1, p, 5, p, None), b"bad sizes"), ((p, p, 4, 4, p, 0, p, None), b"min_area"),
                 ((p, p, 4, 4, p, -3, p, None), b"min_area")]
        for args, msg in cases:
            assert fn(*args) == -1, (tag, msg)
            assert tag in lib.dm_last_error() and msg in lib.dm_last_error(), (tag, msg, lib.dm_last_error())
