"""GPU: rag.region_merge_cost, rag.pixel_regions, rag.mrs and rag.mrs_segment (csrc/dm_mrs.hip + the merge loop) against the numpy
spec tests/mrs_ref.py -- every comparison is bit for bit."""
import functools

import numpy as np
import pytest
import torch

import merge_ref as M
import mrs_ref as R
from oracle import rag as OR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("region_of", "ptr", "idx", "edges", "weights", "rep", "history", "history_simi", "pooled", "simi")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_stats(st, nb):
    out = {k: dev(st[k]) for k in M.STAT_KEYS}
    out["bands"] = nb
    return out


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_equals_spec(res, ref):
    for k in FIELDS:
        got, want = getattr(res, k).cpu().numpy(), ref[k]
        assert got.dtype == want.dtype and got.shape == want.shape, (k, got.dtype, got.shape, want.dtype, want.shape)
        assert np.array_equal(bits(got), bits(want)), k
    for k in M.STAT_KEYS:
        got, want = res.stats[k].cpu().numpy(), ref["stats"][k]
        assert got.dtype == want.dtype and np.array_equal(got, want), k
    assert res.rounds == ref["rounds"] and res.regions_per_round == ref["regions_per_round"]
    assert res.merges_per_round == ref["merges_per_round"]


@functools.lru_cache(maxsize=None)
def quadrants(H=24, W=40, bands=3):
    return R.quadrant_tile(H, W, bands)


@functools.lru_cache(maxsize=None)
def superpixel_case():
    lab, gy, gx = M.superpixels(48, 64, 6, 1)
    return lab, gy * gx


@functools.lru_cache(maxsize=None)
def pixel_ref(scale, shape, max_rounds=None, min_regions=0):
    return R.mrs_ref(quadrants(), scale, shape, max_rounds=max_rounds, min_regions=min_regions)


@functools.lru_cache(maxsize=None)
def label_ref(scale, shape):
    lab, S = superpixel_case()
    return R.mrs_ref(quadrants(48, 64), scale, shape, labels=lab, n_labels=S)


# ---- the cost ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cost_case(H, W, cell, bands):
    lab, gy, gx = M.superpixels(H, W, cell, 1)
    S = gy * gx
    ids = np.unique(lab)
    lab = np.searchsorted(ids, lab).astype(np.int32)              # dense: a region without pixels has no cost
    S = len(ids)
    tile = np.random.default_rng(H + W + bands).integers(0, 256, (bands, H, W), dtype=np.uint8)
    tile[:, :H // 2] //= 3                                        # two populations, so that V differs between neighbours
    st = OR.label_stats(lab, tile, S)
    e, w = OR.rag_edges(lab, S)
    return st, e, w, S


@pytest.mark.parametrize("H,W,cell", [(48, 64, 6), (200, 300, 5)])
@pytest.mark.parametrize("bands", [1, 3, 4])
def test_region_merge_cost_equals_the_spec(H, W, cell, bands):
    from deepmerge_amd import rag
    st, e, w, S = cost_case(H, W, cell, bands)
    nb = min(bands, 3)
    if (H, W) == (48, 64):
        assert S == 88
    else:
        assert len(e) > 3000 and len(e) % 256 != 0               # more than one workgroup, a ragged last one
    dst, de, dw = dev_stats(st, nb), dev(e), dev(w)
    weights = [None, [0.5, 2.0, 1.25][:nb], [0.0, 3.0, 1e-3][:nb]]
    for shape in (0.0, 0.1, 0.9):
        for comp in (0.0, 0.5, 1.0):
            for bw in weights:
                got = rag.region_merge_cost(dst, de, dw, shape, comp, bw).cpu().numpy()
                want = R.cost(st, e, w, shape, comp, bw)
                assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), (shape, comp, bw)
    assert (R.cost(st, e, w, 0.9, 1.0) == 0).any() and (R.cost(st, e, w, 0.9, 1.0) > 0).any()      # the clamp is reached


def test_region_merge_cost_with_counts_of_2_to_the_30():
    from deepmerge_amd import rag
    st, e, w = R.big_count_stats()
    for shape, comp, bw in ((0.1, 0.5, None), (0.0, 0.5, [1.0, 0.25]), (0.9, 1.0, None), (0.5, 0.0, [3.0, 0.0])):
        got = rag.region_merge_cost(dev_stats(st, 2), dev(e), dev(w), shape, comp, bw).cpu().numpy()
        assert np.array_equal(bits(got), bits(R.cost(st, e, w, shape, comp, bw))), (shape, comp, bw)


# ---- the pixel start ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (5, 1), (3, 4), (7, 9), (33, 65), (64, 257)])
@pytest.mark.parametrize("bands", [1, 3, 4])
def test_pixel_regions_equals_the_arange_raster_and_the_spec(H, W, bands):
    from deepmerge_amd import rag
    tile = np.random.default_rng(H * 1000 + W + bands).integers(0, 256, (bands, H, W), dtype=np.uint8)
    dt = dev(tile)
    st, e, w = rag.pixel_regions(dt)
    E = H * (W - 1) + (H - 1) * W
    assert st["bands"] == min(bands, 3) and tuple(e.shape) == (E, 2) and tuple(w.shape) == (E,)
    assert e.dtype == torch.int32 and w.dtype == torch.int32
    rst, re_, rw = R.pixel_regions_ref(tile)
    assert np.array_equal(e.cpu().numpy(), re_) and np.array_equal(w.cpu().numpy(), rw)
    lab = torch.arange(H * W, dtype=torch.int32, device=DEV).view(H, W)
    lst = rag.label_stats(lab, dt, H * W)
    for k in M.STAT_KEYS:
        assert st[k].dtype == lst[k].dtype and st[k].shape == lst[k].shape, k
        assert torch.equal(st[k], lst[k]) and np.array_equal(st[k].cpu().numpy(), rst[k]), k
    if E:
        le, lw = rag.rag_edges(lab, H * W)
        assert torch.equal(e, le) and torch.equal(w, lw)
    assert torch.equal(dt.cpu(), torch.from_numpy(tile))


# ---- the merge -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,shape", [(10, 0.1), (10, 0.9), (5, 0.1)])
def test_pixel_start_equals_the_spec(scale, shape):
    from deepmerge_amd import rag
    res = rag.mrs(dev(quadrants()), scale, shape=shape)
    assert_equals_spec(res, pixel_ref(scale, shape))


def test_planted_quadrants_are_recovered():
    from deepmerge_amd import rag
    res = rag.mrs(dev(quadrants()), 10, shape=0.1)
    lab = res.region_of.view(24, 40).cpu().numpy()
    assert res.rep.numel() == 4 and len(np.unique(lab)) == 4
    for ys in (slice(0, 12), slice(12, 24)):
        for xs in (slice(0, 20), slice(20, 40)):
            assert len(np.unique(lab[ys, xs])) == 1


def test_constant_tile_is_decided_by_ids_alone():
    from deepmerge_amd import rag
    tile = np.full((3, 16, 16), 77, np.uint8)
    ref = R.mrs_ref(tile, 3.0, 0.1)
    assert ref["rounds"] >= 2 and ref["regions_per_round"][-1] < 256
    assert_equals_spec(rag.mrs(dev(tile), 3.0), ref)


@pytest.mark.parametrize("scale,shape", [(60, 0.1), (150, 0.5)])
def test_label_start_equals_the_spec(scale, shape):
    from deepmerge_amd import rag
    lab, S = superpixel_case()
    res = rag.mrs(dev(quadrants(48, 64)), scale, shape=shape, labels=dev(lab), n_labels=S)
    assert_equals_spec(res, label_ref(scale, shape))
    assert res.regions_per_round[-1] == {60: 6, 150: 3}[scale]


def test_max_rounds_and_min_regions_equal_the_spec():
    from deepmerge_amd import rag
    dt = dev(quadrants())
    res = rag.mrs(dt, 10, max_rounds=3)
    assert res.rounds == 3
    assert_equals_spec(res, pixel_ref(10, 0.1, 3, 0))
    res = rag.mrs(dt, 10, min_regions=10)
    assert res.rep.numel() >= 10
    assert_equals_spec(res, pixel_ref(10, 0.1, None, 10))
    assert_equals_spec(rag.mrs(dt, 10, max_rounds=0), pixel_ref(10, 0.1, 0, 0))


def test_starts_without_an_edge_return_at_once():
    from deepmerge_amd import rag
    tile = np.array([[[9]], [[200]]], np.uint8)                    # one pixel: S0 = 1, E = 0
    res = rag.mrs(dev(tile), 10)
    assert_equals_spec(res, R.mrs_ref(tile, 10))
    assert res.rounds == 0 and res.region_of.tolist() == [0] and res.simi.numel() == 0
    tile, lab = quadrants(), np.zeros((24, 40), np.int32)          # one label over the whole raster
    assert_equals_spec(rag.mrs(dev(tile), 10, labels=dev(lab), n_labels=1), R.mrs_ref(tile, 10, labels=lab, n_labels=1))


def test_band_weights_and_compactness_reach_the_merge():
    from deepmerge_amd import rag
    tile = quadrants(24, 40, 4)
    ref = R.mrs_ref(tile, 8, 0.3, 0.8, [2.0, 0.0, 0.5])
    assert_equals_spec(rag.mrs(dev(tile), 8, shape=0.3, compactness=0.8, band_weights=[2.0, 0.0, 0.5]), ref)


# ---- interop ---------------------------------------------------------------------------------------------------------------------------
def test_result_works_as_any_merge_result():
    from deepmerge_amd import rag
    lab, S = superpixel_case()
    dl, dt = dev(lab), dev(quadrants(48, 64))
    res = rag.mrs(dt, 60, labels=dl, n_labels=S)
    C = res.rep.numel()
    merged = res.labels(dl)
    want = label_ref(60, 0.1)["region_of"][lab]
    assert np.array_equal(merged.cpu().numpy(), want) and len(np.unique(want)) == C
    poly = res.polygons(dl)
    assert poly.region_ptr.numel() == C + 1 and torch.unique(poly.ring_label).tolist() == list(range(C))
    yy, xx = np.mgrid[0:48, 0:64]
    truth = ((yy >= 24) * 2 + (xx >= 32)).astype(np.int32)
    ov = rag.label_overlap(dl, dev(truth), S, 4)
    sc = res.scores(ov)
    direct = rag.label_overlap(merged, dev(truth), C, 4).scores()
    assert sc == direct
    assert torch.equal(res.region_of_at(res.rounds), res.region_of)
    polys, arcs = res.simplified(dl, 1.0)
    assert polys.region_ptr.numel() == C + 1 and int(arcs.edge.max()) == res.edges.shape[0] - 1
    assert sc.n == 48 * 64 and sc.n_regions == C


def test_mrs_segment_returns_dense_labels():
    from deepmerge_amd import rag
    dt = dev(quadrants())
    labels, n = rag.mrs_segment(dt, 5)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (24, 40) and n == 62
    assert torch.unique(labels).tolist() == list(range(n))
    st = rag.label_stats(labels, dt, n)
    assert int(st["count"].sum()) == 960 and int(st["count"].min()) >= 1
    lab, S = superpixel_case()
    labels, n = rag.mrs_segment(dev(quadrants(48, 64)), 60, labels=dev(lab), n_labels=S)
    assert n == 6 and torch.unique(labels).tolist() == list(range(6))


# ---- same-input checks ---------------------------------------------------------------------------------------------------------------
def test_runs_are_deterministic_and_leave_inputs_alone():
    from deepmerge_amd import rag
    lab, S = superpixel_case()
    tile = quadrants(48, 64)
    dl, dt = dev(lab), dev(tile)
    a = rag.mrs(dt, 60, labels=dl, n_labels=S)
    b = rag.mrs(dt, 60, labels=dl, n_labels=S)
    for k in FIELDS:
        assert torch.equal(getattr(a, k).view(torch.int32) if getattr(a, k).dtype == torch.float32 else getattr(a, k),
                           getattr(b, k).view(torch.int32) if getattr(b, k).dtype == torch.float32 else getattr(b, k)), k
    for k in M.STAT_KEYS:
        assert torch.equal(a.stats[k], b.stats[k]), k
    assert np.array_equal(dl.cpu().numpy(), lab) and np.array_equal(dt.cpu().numpy(), tile)
    dp = dev(quadrants())
    a, b = rag.mrs(dp, 10), rag.mrs(dp, 10)
    assert torch.equal(a.region_of, b.region_of) and torch.equal(a.history, b.history)
    assert torch.equal(a.history_simi.view(torch.int32), b.history_simi.view(torch.int32))
    assert np.array_equal(dp.cpu().numpy(), quadrants())


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_bad_inputs_raise_before_any_kernel():
    from deepmerge_amd import rag
    lab, S = superpixel_case()
    dt, dl = dev(quadrants(48, 64)), dev(lab)
    bad = [dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")), dict(shape=1.0), dict(shape=-0.1),
           dict(compactness=1.5), dict(band_weights=[1.0, -1.0, 1.0]), dict(band_weights=[1.0, 1.0]),
           dict(band_weights=[1.0, float("nan"), 1.0]), dict(labels=dl.long(), n_labels=S), dict(labels=dl), dict(labels=dl[:, :60], n_labels=S),
           dict(labels=dl.cpu(), n_labels=S), dict(n_labels=S), dict(max_rounds=-1)]
    for kw in bad:
        args = {"scale": 10.0, **kw}
        with pytest.raises(ValueError):
            rag.mrs(dt, **args)
    with pytest.raises(ValueError, match="no CPU fallback"):
        rag.mrs(dt.cpu(), 10.0)
    with pytest.raises(ValueError):
        rag.mrs(dt.float(), 10.0)
    with pytest.raises(ValueError, match="every id"):
        rag.mrs(dt, 10.0, labels=dl, n_labels=S + 2)               # ids S and S + 1 never occur
    gap = dl.clone()
    gap[gap == 5] = 6
    with pytest.raises(ValueError, match="every id"):
        rag.mrs(dt, 10.0, labels=gap, n_labels=S)
    big = torch.zeros((1, 4100, 4100), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="2\\^24"):
        rag.mrs(big, 10.0)
    with pytest.raises(ValueError, match="2\\^24"):
        rag.pixel_regions(big)
    st, e, w = R.big_count_stats()
    with pytest.raises(ValueError):
        rag.region_merge_cost(dev_stats(st, 2), dev(e), dev(w).long())
    with pytest.raises(ValueError):
        rag.region_merge_cost(dev_stats(st, 2), dev(e), dev(w), shape=1.0)
