"""GPU: the minimum region area of the merge -- dm_merge_best_small, dm_merge_accept (csrc/dm_merge.hip) and the elimination rounds
of rag.merge_regions / rag.mrs / FeatureIO.merge_tile / scene.segment_scene -- against the numpy spec tests/merge_small_ref.py.
Every comparison is bit for bit, with tests/test_gpu_merge.py's comparison."""
import functools

import numpy as np
import pytest
import torch

import merge_ref as M
import merge_small_ref as MS
import mrs_ref as R
import scene_labels_ref as SR
from test_gpu_merge import assert_equals_spec, assert_raster_consistent

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
STAT_KEYS = M.STAT_KEYS


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_stats(st, bands=3):
    out = {k: dev(st[k]) for k in STAT_KEYS}
    out["bands"] = bands
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def equals_spec(res, ref):
    assert_equals_spec(res, ref)
    assert res.small_rounds == ref["small_rounds"]
    for k in range(res.rounds + 1):                               # the replay from the history, across the phase boundary
        assert np.array_equal(res.region_of_at(k).cpu().numpy(), ref["maps"][k]), k


# ---- the two kernels alone ----------------------------------------------------------------------------------------------------------
def run_kernels(edges, simi, C, count, min_area):
    """(best uint64 [C], picked bool [E]) of dm_merge_best_small -> dm_merge_accept -> dm_merge_match."""
    from deepmerge_amd import _lib
    from deepmerge_amd.ops import _stream, check
    lib, E = _lib.lib(), len(edges)
    te, ts, tc = dev(edges), dev(simi), dev(count)
    keep = [t.clone() for t in (te, ts, tc)]
    best = torch.full((C + 3,), 7, dtype=torch.int64, device=DEV)                # stale values, and a guard behind the C entries
    picked = torch.empty(E, dtype=torch.uint8, device=DEV)
    root, pick = (torch.empty(C, dtype=torch.int32, device=DEV) for _ in range(2))
    n = torch.zeros(1, dtype=torch.int32, device=DEV)
    args = (te.data_ptr(), ts.data_ptr(), E, C, tc.data_ptr(), int(min_area), best.data_ptr(), _stream())
    check(lib.dm_merge_best_small(*args), "dm_merge_best_small")
    proposals = best.clone()
    check(lib.dm_merge_accept(*args), "dm_merge_accept")
    check(lib.dm_merge_match(te.data_ptr(), best.data_ptr(), E, C, picked.data_ptr(), root.data_ptr(), pick.data_ptr(), n.data_ptr(),
                             _stream()), "dm_merge_match")
    assert best[C:].tolist() == [7, 7, 7]
    for before, after in zip(keep, (te, ts, tc)):
        assert torch.equal(bits(before), bits(after))
    got = picked.cpu().numpy().astype(bool)
    assert int(n) == int(got.sum())
    return best[:C].cpu().numpy().view(np.uint64), got, proposals[:C].cpu().numpy().view(np.uint64)


def check_kernels(edges, simi, C, count, min_area):
    edges, simi, count = np.asarray(edges, np.int32).reshape(-1, 2), np.asarray(simi, np.float32), np.asarray(count, np.int64)
    want_picked, want_best = MS.pick_small(simi, edges, C, count, min_area)
    best, picked, proposals = run_kernels(edges, simi, C, count, min_area)
    assert np.array_equal(best, want_best) and np.array_equal(picked, want_picked)
    small = count < min_area
    assert (proposals[~small] == ALL_ONES).all() and np.array_equal(proposals[small], want_best[small])    # accept leaves the small alone
    assert M.is_matching(edges[picked])
    return want_picked, want_best


SCORES = np.array([0.0, 0.25, 0.25, 0.5, 0.5, 0.5, 1.0, 3.0, np.inf, np.nan], np.float32)       # ties, +0, +inf, NaN


def exact_graph(C, E, seed):
    """Exactly E edges over C regions, canonical, with scores drawn from SCORES."""
    rng = np.random.default_rng(seed)
    a, b = np.triu_indices(C, 1)
    take = np.sort(rng.choice(len(a), E, replace=False))          # (a, b) pairs in row-major order stay sorted and unique
    edges = np.stack((a[take], b[take]), 1).astype(np.int32)
    return edges, rng.choice(SCORES, E), rng.integers(0, 10, C).astype(np.int64)


@pytest.mark.parametrize("E", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_kernels_equal_the_spec_at_every_edge_count(E):
    C = 2 if E == 1 else 70
    edges, simi, count = exact_graph(C, E, E)
    if E == 1:
        simi, count = np.array([0.5], np.float32), np.array([1, 9], np.int64)
    picked, best = check_kernels(edges, simi, C, count, 5)
    if E >= 255:
        assert picked.sum() >= 3 and np.isnan(simi).any() and (simi == 0).any() and np.isinf(simi).any()
    if E == 1000:                                                  # sparser: most regions have a few edges, runs of `a` are short
        edges, simi, count = exact_graph(900, E, 5)
        assert check_kernels(edges, simi, 900, count, 5)[0].sum() >= 50


@pytest.mark.parametrize("hub_small", [True, False])
@pytest.mark.parametrize("hub_low", [True, False])
def test_hub_of_degree_300(hub_small, hub_low):
    """Hub as the lowest id: a run of 300 equal `a` across wave and workgroup boundaries; as the highest id: 300 atomics on one
    `b`.  A small hub proposes once; a non-small hub has 300 proposers and accepts one."""
    rng = np.random.default_rng(int(hub_small) * 2 + int(hub_low))
    C, hub = 301, 0 if hub_low else 300
    leaves = np.arange(1, 301) if hub_low else np.arange(300)
    star = np.stack((np.minimum(hub, leaves), np.maximum(hub, leaves)), 1)
    ring = np.stack((leaves[:-1], leaves[1:]), 1)[::3]            # some edges among the leaves
    edges = M.canonical_edges(np.concatenate((star, ring)), C)
    simi = rng.choice(SCORES[:8], len(edges)).astype(np.float32)
    at_hub = (edges == hub).any(1)
    simi[at_hub] = rng.choice(np.array([0.5, 0.5, 0.75, 2.0], np.float32), int(at_hub.sum()))      # the hub's best is a many-way tie
    if not hub_small:
        simi[~at_hub] = rng.choice(SCORES[7:], int((~at_hub).sum()))          # 3, +inf, NaN: every leaf resembles the hub most
    count = np.full(C, 1, np.int64) if not hub_small else rng.integers(0, 10, C).astype(np.int64)
    count[hub] = 1 if hub_small else 100
    picked, best = check_kernels(edges, simi, C, count, 5)
    other = int(best[hub] & np.uint64(0xFFFFFFFF))
    ties = edges[at_hub & (simi == 0.5)]
    assert best[hub] != ALL_ONES and other == ties[ties != hub].min()        # the smallest id among the tied neighbours
    if not hub_small:
        assert picked[at_hub].sum() == 1                          # 300 proposers, one accepted


def test_every_region_small_no_region_small_and_counts_beyond_2_to_the_32():
    edges, simi, count = exact_graph(70, 600, 11)
    picked, best = check_kernels(edges, simi, 70, count, 10 ** 9)            # every region small: mutual proposals only
    assert picked.any()
    picked, best = check_kernels(edges, simi, 70, count + 5, 5)              # no region small
    assert not picked.any() and (best == ALL_ONES).all()
    picked, best = check_kernels(edges, simi, 70, count, 1)                  # only the empty regions are small
    assert (count == 0).any() and picked.any()
    big = (np.int64(1) << 32) + count * ((np.int64(1) << 30) + 1)            # 2^32 .. 2^32 + 9 (2^30 + 1): the low words alone mislead
    picked, best = check_kernels(edges, simi, 70, big, (1 << 32) + 5 * ((1 << 30) + 1))
    want, _ = MS.pick_small(simi, edges, 70, count, 5)
    assert np.array_equal(picked, want) and picked.any()
    low = big & np.int64(0xFFFFFFFF)                               # what a 32-bit compare would see
    assert not np.array_equal(low < (((1 << 32) + 5 * ((1 << 30) + 1)) & 0xFFFFFFFF), count < 5)


# ---- merge_regions(min_area=) ---------------------------------------------------------------------------------------------------------
def untouched(before, after):
    for x, y in zip(before, after):
        assert torch.equal(bits(x), bits(y))


@functools.lru_cache(maxsize=None)
def graph_case(S, E, D):
    from deepmerge_amd import rag
    F, ptr, idx, edges, w = M.random_graph(S, E, D, S + E + D)
    count = np.random.default_rng(S).integers(1, 60, S).astype(np.int64)
    count[::17] = 0                                               # regions without pixels are small at every min_area
    st = MS.graph_stats(S, S, count=count)
    t = [dev(F), dev(ptr), dev(idx), dev(edges), dev(w)]
    dst = dev_stats(st)
    return (F, ptr, idx, edges, w, st), t, dst, rag.merge_regions(*t[:4], weights=t[4], stats=dst)


@pytest.mark.parametrize("min_area", [0, 1, 30, 10 ** 9])
@pytest.mark.parametrize("S,E,D", [(50, 120, 8), (5000, 20000, 100)])
def test_random_graphs_equal_the_spec(S, E, D, min_area):
    """Synthetic statistics: random counts (30 is the middle of their range, where a raster has "two cells").  At 10^9 every region
    is small: only mutual proposals merge, and the larger graph takes some 1700 rounds."""
    from deepmerge_amd import rag
    (F, ptr, idx, edges, w, st), t, dst, plain = graph_case(S, E, D)
    keep = [x.clone() for x in t] + [dst[k].clone() for k in STAT_KEYS]
    ref = MS.merge_regions_ref(F, ptr, idx, edges, 1.0, w, st, min_area=min_area)
    res = rag.merge_regions(*t[:4], weights=t[4], stats=dst, min_area=min_area)
    equals_spec(res, ref)
    if min_area == 0:                                             # equals the call without the keyword on every field
        assert res.small_rounds == 0 and res.rounds == plain.rounds and res.regions_per_round == plain.regions_per_round
        for k in ("region_of", "ptr", "idx", "edges", "weights", "rep", "history", "history_simi", "pooled", "simi"):
            assert torch.equal(bits(getattr(res, k)), bits(getattr(plain, k))), k
        assert all(torch.equal(res.stats[k], plain.stats[k]) for k in STAT_KEYS) and res.merges_per_round == plain.merges_per_round
    else:
        assert res.small_rounds >= 1 and res.rounds - res.small_rounds == plain.rounds
        assert torch.equal(res.region_of_at(plain.rounds), plain.region_of)
    if min_area == 30:                                            # the limits, counted over both phases
        last = ref["regions_per_round"][-1]
        for kw in ({"max_rounds": plain.rounds}, {"max_rounds": plain.rounds + 2}, {"min_regions": last + 1}):
            lim = MS.merge_regions_ref(F, ptr, idx, edges, 1.0, w, st, min_area=30, **kw)
            assert lim["rounds"] < ref["rounds"]
            equals_spec(rag.merge_regions(*t[:4], weights=t[4], stats=dst, min_area=30, **kw), lim)
    untouched(keep, t + [dst[k] for k in STAT_KEYS])


@pytest.mark.parametrize("H,W,cell,bands,block", [(64, 80, 9, 3, 3), (257, 301, 13, 4, 3)])
def test_rasters_with_outlier_superpixels_equal_the_spec_and_stay_consistent(H, W, cell, bands, block):
    from deepmerge_amd import rag
    c = M.raster_case(H, W, cell, bands, block, 100, H + W)
    F = MS.add_outliers(c, 0.15, H)
    lab, S, tile = c["labels"], c["S"], c["tile"]
    tl, tt = dev(lab), dev(tile)
    edges, w = rag.rag_edges(tl, S)
    st = rag.label_stats(tl, tt, S)
    args = [dev(F), dev(c["ptr"]), dev(c["idx"]), edges]
    keep = [x.clone() for x in args] + [w.clone()] + [st[k].clone() for k in STAT_KEYS]
    np_st = {k: st[k].cpu().numpy() for k in STAT_KEYS}
    for min_area in (1, 2 * cell * cell, 10 ** 9):
        ref = MS.merge_regions_ref(F, c["ptr"], c["idx"], edges.cpu().numpy(), 1.0, w.cpu().numpy(), np_st, min_area=min_area)
        res = rag.merge_regions(*args, margin=1.0, weights=w, stats=st, min_area=min_area)
        equals_spec(res, ref)
        merged = res.labels(tl)
        assert np.array_equal(merged.cpu().numpy(), ref["region_of"][lab])
        assert_raster_consistent(res, lab, tile, merged.cpu().numpy())
        if min_area > 1:                                          # guards the inputs: the outliers are there and get absorbed
            assert res.small_rounds >= 2 and res.regions_per_round[-1] < res.regions_per_round[res.rounds - res.small_rounds] - S // 20
    assert int((res.stats["count"] > 0).sum()) == 1                # min_area = 10^9: one region holds every pixel
    untouched(keep, args + [w] + [st[k] for k in STAT_KEYS])


# ---- mrs(min_area=) -----------------------------------------------------------------------------------------------------------------------
def test_mrs_from_pixels_and_from_labels_equals_the_spec():
    from deepmerge_amd import rag
    tile = R.quadrant_tile()
    tt = dev(tile)
    ref = MS.mrs_ref(tile, 5.0, min_area=12)
    assert ref["small_rounds"] >= 2
    res = rag.mrs(tt, 5.0, min_area=12)
    equals_spec(res, ref)
    assert int(res.stats["count"].min()) >= 12
    plain = rag.mrs(tt, 5.0)
    zero = rag.mrs(tt, 5.0, min_area=0)
    assert zero.small_rounds == 0 and torch.equal(zero.region_of, plain.region_of) and torch.equal(zero.history, plain.history)
    raster, n = rag.mrs_segment(tt, 5.0, min_area=12)
    assert n == res.rep.numel() and torch.equal(raster, res.region_of.view(tile.shape[1], tile.shape[2]))
    lab, gy, gx = M.superpixels(48, 64, 6, 1)
    big = R.quadrant_tile(48, 64, 3)
    tb, tl = dev(big), dev(lab)
    for min_area in (100, 10 ** 9):
        ref = MS.mrs_ref(big, 20.0, labels=lab, n_labels=gy * gx, min_area=min_area)
        assert ref["small_rounds"] >= 1 and ref["rounds"] > ref["small_rounds"]
        res = rag.mrs(tb, 20.0, labels=tl, n_labels=gy * gx, min_area=min_area)
        equals_spec(res, ref)
    st = rag.label_stats(tl, tb, gy * gx)
    e, w = rag.rag_edges(tl, gy * gx)
    graph = rag.mrs_graph(st, e, w, 20.0, min_area=10 ** 9)
    assert graph.small_rounds == res.small_rounds and torch.equal(graph.region_of, res.region_of)
    assert torch.equal(tt.cpu(), torch.from_numpy(tile)) and torch.equal(tl.cpu(), torch.from_numpy(lab))


# ---- the pipeline: merge_tile and a scene ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fio():
    from deepmerge_amd.ExtractFeatures import FeatureIO
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    torch.manual_seed(1)
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=[32, 64, 128], depth=[1, 1, 1], in_c=3, numerics="fp32")
    return FeatureIO(net, None, DEV)


@functools.lru_cache(maxsize=None)
def scene_case():
    return SR.scene_image(), SR.raster_a()


def equal_results(got, want):
    assert torch.equal(got.region_of, want.region_of) and torch.equal(got.history, want.history)
    assert torch.equal(bits(got.history_simi), bits(want.history_simi))
    assert got.rounds == want.rounds and got.small_rounds == want.small_rounds and got.regions_per_round == want.regions_per_round
    assert torch.equal(got.edges, want.edges) and torch.equal(got.weights, want.weights)
    for key in STAT_KEYS:
        assert torch.equal(got.stats[key], want.stats[key]), key


@pytest.fixture(scope="module")
def whole_scene(fio):
    """merge_tile on the whole 200 x 232 scene, with and without min_area: (margin, min_area, plain, with min_area, its points, features)."""
    image, (lab, S) = scene_case()
    whole, raster = dev(image), dev(lab)
    first, _ = fio.merge_tile(whole, raster, S, k=1, margin=1.0, batch_size=1, max_rounds=0)
    margin = float(first.simi.float().median())                    # inside the spread of the edge scores: rounds merge and stop
    plain, _ = fio.merge_tile(whole, raster, S, k=1, margin=margin, batch_size=1)
    min_area = int(plain.stats["count"].median()) + 1              # about half of what the margin rounds left is small
    want, pts = fio.merge_tile(whole, raster, S, k=1, margin=margin, batch_size=1, min_area=min_area)
    return margin, min_area, plain, want, pts, fio.features.clone()


def test_merge_tile_passes_min_area_to_merge_regions(whole_scene):
    from deepmerge_amd import rag
    image, (lab, S) = scene_case()
    margin, min_area, plain, want, pts, features = whole_scene
    whole, raster = dev(image), dev(lab)
    assert plain.small_rounds == 0 and want.small_rounds >= 1 and want.rounds - want.small_rounds == plain.rounds
    assert torch.equal(want.region_of_at(plain.rounds), plain.region_of) and want.rep.numel() < plain.rep.numel()
    edges, weights = rag.rag_edges(raster, S)
    res = rag.merge_regions(features, pts.ptr, pts.idx, edges, margin=margin, weights=weights, stats=rag.label_stats(raster, whole, S),
                            min_area=min_area)
    equal_results(res, want)
    small = want.stats["count"] < min_area                         # what is left below the area has no scored edge
    e = want.edges[want.simi == want.simi].long()
    assert not small[e].any()


def test_mrs_labels_passes_min_area_to_the_scene_graph():
    from deepmerge_amd import rag, scene
    image, (lab, S) = scene_case()
    whole, raster = dev(image), dev(lab)
    st = rag.label_stats(raster, whole, S)
    edges, weights = rag.rag_edges(raster, S)
    scale = float(rag.region_merge_cost(st, edges, weights).median().sqrt())       # inside the spread of the costs
    plain = rag.mrs(whole, scale, labels=raster, n_labels=S)
    min_area = int(plain.stats["count"].median()) + 1
    want = rag.mrs(whole, scale, labels=raster, n_labels=S, min_area=min_area)
    assert want.small_rounds >= 1 and want.rounds - want.small_rounds == plain.rounds and int(want.stats["count"].min()) >= min_area
    got = scene.mrs_labels(image, lab, S, scale, tile=SR.TILE, device=DEV, min_area=min_area)
    equal_results(got, want)
    assert torch.equal(bits(got.simi), bits(want.simi)) and torch.equal(got.rep, want.rep)


def test_segment_scene_passes_min_area_on_the_labels_and_the_cross_seams_paths(fio, whole_scene):
    from deepmerge_amd import scene
    image, (lab, S) = scene_case()
    margin, min_area, plain, want, pts, features = whole_scene
    res = fio.segment_scene(image, tile=SR.TILE, k=1, margin=margin, batch_size=1, labels=lab, n_labels=S, min_area=min_area)
    assert torch.equal(bits(res.features), bits(features))
    equal_results(res.result, want)
    assert np.array_equal(res.write_merged(), want.labels(dev(lab)).cpu().numpy())
    made = fio.segment_scene(image, tile=SR.TILE, k=1, margin=margin, batch_size=1, cross_seams=True, slic={"cell": 24},
                             min_area=10 ** 9)
    again = scene.segment_labels(fio, image, made.labels, made.n_labels, tile=SR.TILE, k=1, margin=margin, batch_size=1, min_area=10 ** 9)
    equal_results(made.result, again.result)
    p1 = made.result.rounds - made.result.small_rounds
    assert made.result.small_rounds >= 1 and made.result.regions_per_round[-1] < made.result.regions_per_round[p1]
