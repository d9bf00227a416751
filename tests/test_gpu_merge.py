"""GPU: rag.merge_regions (csrc/dm_merge.hip) against the numpy spec tests/merge_ref.py -- every comparison is bit for bit."""
import time

import numpy as np
import pytest
import torch

import merge_ref as M
from oracle import rag as OR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("region_of", "ptr", "idx", "edges", "rep", "history", "history_simi", "pooled", "simi")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_stats(st, bands):
    out = {k: dev(st[k]) for k in M.STAT_KEYS}
    out["bands"] = min(bands, 3)
    return out


def assert_equals_spec(res, ref):
    for k in FIELDS:
        got, want = getattr(res, k).cpu().numpy(), ref[k]
        assert got.dtype == want.dtype and got.shape == want.shape, (k, got.dtype, got.shape, want.dtype, want.shape)
        assert np.array_equal(got.view(np.int32) if got.dtype == np.float32 else got,
                              want.view(np.int32) if want.dtype == np.float32 else want), k      # floats: same bits, NaN included
    assert res.rounds == ref["rounds"] and res.regions_per_round == ref["regions_per_round"]
    assert res.merges_per_round == ref["merges_per_round"]
    if ref["weights"] is None:
        assert res.weights is None
    else:
        assert np.array_equal(res.weights.cpu().numpy(), ref["weights"]) and res.weights.dtype == torch.int32
    if ref["stats"] is None:
        assert res.stats is None
    else:
        for k in M.STAT_KEYS:
            assert np.array_equal(res.stats[k].cpu().numpy(), ref["stats"][k]), k


def assert_raster_consistent(res, lab, tile, merged):
    """The folded graph and statistics are those of the relabelled raster, recomputed from scratch by the oracle."""
    C = res.ptr.numel() - 1
    e2, w2 = OR.rag_edges(merged, C)
    assert np.array_equal(e2, res.edges.cpu().numpy()) and np.array_equal(w2, res.weights.cpu().numpy())
    st2 = OR.label_stats(merged, tile, C)
    for k in M.STAT_KEYS:
        assert np.array_equal(st2[k], res.stats[k].cpu().numpy()), k
    return st2


@pytest.mark.parametrize("S,E,D", [(50, 120, 3), (50, 120, 128), (5000, 20000, 8), (5000, 20000, 100), (20000, 60000, 100),
                                   (20000, 60000, 128), (300, 0, 8)])
def test_random_graphs_match_the_spec(S, E, D):
    from deepmerge_amd import rag
    F, ptr, idx, edges, w = M.random_graph(S, E, D, S + E + D)
    assert (np.diff(ptr) == 0).any()                              # some regions have no points
    ref = M.merge_regions_ref(F, ptr, idx, edges, 1.0, w)
    assert E == 0 or ref["rounds"] >= 2
    res = rag.merge_regions(dev(F), dev(ptr), dev(idx), dev(edges), margin=1.0, weights=dev(w))
    assert_equals_spec(res, ref)
    bare = rag.merge_regions(dev(F), dev(ptr), dev(idx), dev(edges))                 # without weights: the same partition
    assert bare.weights is None and torch.equal(bare.region_of, res.region_of) and torch.equal(bare.edges, res.edges)
    assert torch.equal(bare.history, res.history)


RASTERS = [(64, 80, 9, 3, 3), (257, 301, 13, 4, 3), (1024, 1024, 29, 1, 4), (33, 17, 40, 2, 2)]


@pytest.mark.parametrize("H,W,cell,bands,block", RASTERS)
def test_rasters_match_the_spec_and_stay_consistent(H, W, cell, bands, block):
    from deepmerge_amd import rag
    c = M.raster_case(H, W, cell, bands, block, 100, H + W)
    lab, S, tile = c["labels"], c["S"], c["tile"]
    tl, tt = dev(lab), dev(tile)
    edges, w = rag.rag_edges(tl, S)
    st = rag.label_stats(tl, tt, S)
    ref = M.merge_regions_ref(c["F"], c["ptr"], c["idx"], edges.cpu().numpy(), 1.0, w.cpu().numpy(),
                              {k: st[k].cpu().numpy() for k in M.STAT_KEYS})
    if S >= 256:                                                  # guards the inputs, not the code under test
        assert ref["rounds"] >= 3 and len(ref["ptr"]) - 1 < S // 2
    res = rag.merge_regions(dev(c["F"]), dev(c["ptr"]), dev(c["idx"]), edges, margin=1.0, weights=w, stats=st)
    assert_equals_spec(res, ref)
    merged = res.labels(tl)
    assert merged.dtype == torch.int32 and np.array_equal(merged.cpu().numpy(), ref["region_of"][lab])
    st2 = assert_raster_consistent(res, lab, tile, merged.cpu().numpy())
    assert np.array_equal(rag.designed_features(res.stats).cpu().numpy(), OR.designed_features(st2))
    for k in range(res.rounds + 1):
        assert np.array_equal(res.region_of_at(k).cpu().numpy(), ref["maps"][k]), k
    assert torch.equal(res.region_of_at(res.rounds), res.region_of)


def test_relabel_raster_paths():
    """16-byte path, its scalar tail, a raster that is not 16-byte aligned, and ids outside [0, S) copied through."""
    from deepmerge_amd import rag
    rng = np.random.default_rng(5)
    S = 1000
    mapping = rng.integers(0, 77, S).astype(np.int32)
    tm = dev(mapping)
    for H, W, off in [(64, 64, 0), (37, 53, 0), (37, 53, 1), (1, 3, 0), (128, 96, 3), (515, 1031, 2)]:
        lab = rng.integers(-3, S + 3, (H, W)).astype(np.int32)
        want = np.where((lab >= 0) & (lab < S), mapping[np.clip(lab, 0, S - 1)], lab)
        buf = torch.zeros(H * W + 8, dtype=torch.int32, device=DEV)
        view = buf[off:off + H * W].view(H, W)
        view.copy_(dev(lab))
        assert view.data_ptr() % 16 == (4 * off) % 16
        assert np.array_equal(rag.relabel_raster(view, tm).cpu().numpy(), want), (H, W, off)
    with pytest.raises(ValueError):
        rag.relabel_raster(dev(lab).long(), tm)


def test_runs_are_deterministic_and_leave_inputs_alone():
    from deepmerge_amd import rag
    c = M.raster_case(257, 301, 13, 3, 3, 100, 9)
    tl, tt = dev(c["labels"]), dev(c["tile"])
    edges, w = rag.rag_edges(tl, c["S"])
    st = rag.label_stats(tl, tt, c["S"])
    args = [dev(c["F"]), dev(c["ptr"]), dev(c["idx"]), edges]
    keep = [t.clone() for t in args] + [w.clone()] + [st[k].clone() for k in M.STAT_KEYS]
    a = rag.merge_regions(*args, weights=w, stats=st)
    b = rag.merge_regions(*args, weights=w, stats=st)
    assert a.rounds == b.rounds >= 3 and a.regions_per_round == b.regions_per_round
    for k in FIELDS + ("weights",):
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), k
    for k in M.STAT_KEYS:
        assert torch.equal(a.stats[k], b.stats[k]), k
    for before, after in zip(keep, args + [w] + [st[k] for k in M.STAT_KEYS]):
        assert torch.equal(before, after)


def test_max_rounds_and_min_regions_match_the_spec():
    from deepmerge_amd import rag
    F, ptr, idx, edges, w = M.random_graph(400, 1200, 8, 7)
    full = M.merge_regions_ref(F, ptr, idx, edges, 1.0, w)
    t = [dev(F), dev(ptr), dev(idx), dev(edges)]
    for kw in ({"max_rounds": 0}, {"max_rounds": 2}, {"min_regions": full["regions_per_round"][2] + 1},
               {"min_regions": full["regions_per_round"][1]}, {"min_regions": 400}, {"min_regions": 1},
               {"max_rounds": 3, "min_regions": full["regions_per_round"][2]}):
        ref = M.merge_regions_ref(F, ptr, idx, edges, 1.0, w, **kw)
        res = rag.merge_regions(*t, weights=dev(w), **kw)
        assert_equals_spec(res, ref)
        m = res.history.shape[0]
        assert np.array_equal(res.history.cpu().numpy(), full["history"][:m])
    for margin in (0.0, -1.0, float("nan"), 1e9):                 # no candidates at all / every edge a candidate
        assert_equals_spec(rag.merge_regions(*t, weights=dev(w), margin=margin), M.merge_regions_ref(F, ptr, idx, edges, margin, w))


def test_nan_features_never_merge():
    from deepmerge_amd import rag
    F, ptr, idx, edges, w = M.random_graph(300, 900, 8, 21)
    F[idx[ptr[5]:ptr[6]]] = np.nan
    F[::17] = np.nan
    ref = M.merge_regions_ref(F, ptr, idx, edges, 1.0, w)
    assert np.isnan(ref["simi"]).any() and ref["rounds"] >= 2
    assert_equals_spec(rag.merge_regions(dev(F), dev(ptr), dev(idx), dev(edges), weights=dev(w)), ref)


def test_bad_inputs_raise_before_any_merge_kernel():
    from deepmerge_amd import rag
    F, ptr, idx, edges, w = M.random_graph(60, 150, 8, 3)
    good = [dev(F), dev(ptr), dev(idx), dev(edges)]
    with pytest.raises(ValueError, match="sorted"):
        rag.merge_regions(good[0], good[1], good[2], dev(edges[::-1].copy()))
    with pytest.raises(ValueError, match="sorted"):
        rag.merge_regions(good[0], good[1], good[2], dev(np.concatenate((edges[:1], edges))))
    with pytest.raises(ValueError, match="a < b"):
        rag.merge_regions(good[0], good[1], good[2], dev(edges[:, ::-1].copy()))
    holes = edges.copy()
    holes[0, 0] = -1
    with pytest.raises(ValueError, match="no polygon"):
        rag.merge_regions(good[0], good[1], good[2], dev(holes))
    with pytest.raises(ValueError, match="a < b"):
        big = edges.copy()
        big[-1, 1] = 60
        rag.merge_regions(good[0], good[1], good[2], dev(big))
    with pytest.raises(ValueError, match="int32"):
        rag.merge_regions(good[0], good[1], good[2], good[3].long())
    with pytest.raises(ValueError, match="int32"):
        rag.merge_regions(good[0], good[1].long(), good[2], good[3])
    with pytest.raises(ValueError, match="weights"):
        rag.merge_regions(*good, weights=dev(w[:-1]))
    with pytest.raises(ValueError, match="ptr must"):
        rag.merge_regions(good[0], dev(ptr[:-1]), good[2], dev(M.canonical_edges(edges[edges.max(1) < 59], 59)))
    with pytest.raises(ValueError, match="rows of features"):
        rag.merge_regions(good[0][:-1], good[1], good[2], good[3])
    lab, gy, gx = M.superpixels(64, 64, 8, 1)
    st = rag.label_stats(dev(lab), dev(np.zeros((3, 64, 64), np.uint8)), 60)
    with pytest.raises(ValueError, match="need weights"):
        rag.merge_regions(*good, stats=st)
    with pytest.raises(ValueError, match="float32"):
        rag.merge_regions(good[0].double(), good[1], good[2], good[3])


def test_full_size_tile():
    """4096 x 4096 labels, ~20 k superpixels, ~3 sample points each, one feature centre per 4 x 4 superpixels.  Done here: the run
    to termination under a time limit (a guard against a loop that does not end: tens of rounds of a few launches each take
    milliseconds, the limit is 60 s), the matching property of every round (no original superpixel's region is absorbed twice in a
    round), the raster self-consistency, AND the comparison with the numpy spec (it takes about a second at this size)."""
    from deepmerge_amd import rag
    c = M.raster_case(4096, 4096, 29, 3, 4, 100, 2, step=17)
    lab, S, tile = c["labels"], c["S"], c["tile"]
    assert 19000 <= S <= 21000 and 55000 <= c["xy"].shape[0] <= 65000
    tl, tt = dev(lab), dev(tile)
    edges, w = rag.rag_edges(tl, S)
    st = rag.label_stats(tl, tt, S)
    args = [dev(c["F"]), dev(c["ptr"]), dev(c["idx"]), edges]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = rag.merge_regions(*args, weights=w, stats=st)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    print(f"full size: {S} -> {res.ptr.numel() - 1} regions in {res.rounds} rounds, {elapsed * 1e3:.1f} ms")
    assert elapsed < 60.0
    assert 3 <= res.rounds < 100 and res.ptr.numel() - 1 < S // 2
    assert float(res.simi.min()) >= 1.0
    h = res.history.cpu().numpy()
    for r in range(res.rounds):
        assert M.is_matching(h[h[:, 0] == r][:, 1:]), r
    merged = res.labels(tl)
    assert torch.equal(merged, res.region_of[tl.long()])
    assert_raster_consistent(res, lab, tile, merged.cpu().numpy())
    ref = M.merge_regions_ref(c["F"], c["ptr"], c["idx"], edges.cpu().numpy(), 1.0, w.cpu().numpy(),
                              {k: st[k].cpu().numpy() for k in M.STAT_KEYS})
    assert_equals_spec(res, ref)
