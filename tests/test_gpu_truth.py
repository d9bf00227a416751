"""GPU: rag.label_overlap / Overlap.coarsen / Overlap.scores / rag.pair_flags (csrc/dm_truth.hip) and PairDataset.from_rasters
against the numpy spec tests/truth_ref.py -- every comparison is an exact integer equality."""
import math

import numpy as np
import pytest
import torch

import merge_ref as M
import points_ref as P
import truth_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assert_equals_spec(got, ref):
    for f in T.FIELDS:
        g, w = getattr(got, f).cpu().numpy(), ref[f]
        assert g.dtype == w.dtype and g.shape == w.shape, (f, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), f
    assert (got.n_labels, got.n_truth) == (ref["n_labels"], ref["n_truth"])


def assert_scores_equal(s, summary):
    ref = T.scores(summary)
    assert (s.n, s.sum_cells, s.sum_regions, s.sum_objects, s.sum_owner, s.sum_cover, s.n_regions, s.n_objects) == tuple(int(v) for v in summary)
    for k in ("asa", "coverage", "rand", "adjusted_rand"):
        a, b = getattr(s, k), ref[k]
        assert a == b or (math.isnan(a) and math.isnan(b)), k


def voronoi_pair(H, W, cell, tcell, holes=False):
    """Labels from seed 1, truth from seed 2 (the pair the CPU tests count the flag classes of)."""
    lab, S = P.voronoi_labels(H, W, cell, 1)
    tru, G = P.voronoi_labels(H, W, tcell, 2)
    if holes:                                                     # ids outside [0,S) in labels; -1 and G + 3 patches in truth
        lab[H // 3:H // 3 + 2, :] = -1
        lab[H // 2:H // 2 + 9, W // 4:W // 4 + 11] = S + 7
        tru[H // 4:H // 4 + 7, W // 3:W // 3 + 40] = -1
        tru[2 * H // 3:2 * H // 3 + 5, :W // 2] = G + 3
        tru[H // 3 - 3:H // 3 + 4, W // 2:] = -1                   # across the labels' -1 band
    return lab, S, tru, G


def noise_pair():
    """Per-pixel random labels 0..4095 against random truth 0..63: thousands of distinct cells in the one 64 x 64 tile, so the 128
    LDS slots fill up and most adds go to the global table directly."""
    rng = np.random.default_rng(4)
    return rng.integers(0, 4096, (64, 64)).astype(np.int32), 4096, rng.integers(0, 64, (64, 64)).astype(np.int32), 64


CASES = {
    "257x301 scalar path": lambda: voronoi_pair(257, 301, 13, 40),          # not multiples of the tile, odd width
    "96x128 vector path": lambda: voronoi_pair(96, 128, 9, 30),
    "1x1": lambda: voronoi_pair(1, 1, 3, 3),
    "5x700": lambda: voronoi_pair(5, 700, 9, 30),
    "700x6": lambda: voronoi_pair(700, 6, 9, 30),
    "64x64 noise": noise_pair,
    "256x256 one cell": lambda: (np.zeros((256, 256), np.int32), 1, np.zeros((256, 256), np.int32), 1),     # every add on one word
    "257x301 holes": lambda: voronoi_pair(257, 301, 13, 40, holes=True),
    "96x128 holes": lambda: voronoi_pair(96, 128, 9, 30, holes=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_label_overlap_matches_the_spec(name):
    from deepmerge_amd import rag
    lab, S, tru, G = CASES[name]()
    tl, tt = dev(lab), dev(tru)
    max_cells = 8192 if "noise" in name else 0
    got = rag.label_overlap(tl, tt, S, G, max_cells=max_cells)
    ref = T.label_overlap(lab, tru, S, G)
    assert_equals_spec(got, ref)
    assert_scores_equal(got.scores(), ref["summary"])
    if "noise" in name:
        assert ref["count"].size > 3000                            # guards the input: far more cells than LDS slots
    if "holes" in name:
        assert (ref["cells"][:, 1] == G).any() and ref["area"].sum() < lab.size
    if lab.size <= 4096 and S * G <= 1 << 16:
        dense = T.label_overlap_dense(lab, tru, S, G)
        assert all(np.array_equal(ref[f], dense[f]) for f in T.FIELDS)
    assert np.array_equal(tl.cpu().numpy(), lab) and np.array_equal(tt.cpu().numpy(), tru)      # the inputs are untouched
    again = rag.label_overlap(tl, tt, S, G, max_cells=max_cells)
    for f in T.FIELDS:
        assert torch.equal(getattr(again, f), getattr(got, f)), f


def test_small_max_cells_raises_cleanly_and_the_next_call_is_exact():
    from deepmerge_amd import rag
    lab, S, tru, G = noise_pair()
    tl, tt = dev(lab), dev(tru)
    with pytest.raises(RuntimeError, match="larger max_cells"):
        rag.label_overlap(tl, tt, S, G, max_cells=1024)            # ~4000 cells: the compacted output is truncated
    with pytest.raises(RuntimeError, match="larger max_cells"):
        rag.label_overlap(tl, tt, S, G, max_cells=64)              # a 1024-slot table: it overflows as well
    assert_equals_spec(rag.label_overlap(tl, tt, S, G, max_cells=8192), T.label_overlap(lab, tru, S, G))
    lab, S, tru, G = voronoi_pair(96, 128, 9, 30)
    assert_equals_spec(rag.label_overlap(dev(lab), dev(tru), S, G), T.label_overlap(lab, tru, S, G))


def test_unaligned_and_non_contiguous_rasters():
    """A raster view that is not 16-byte aligned takes the scalar loads although W % 16 == 0; a strided view is made contiguous."""
    from deepmerge_amd import rag
    lab, S, tru, G = voronoi_pair(96, 128, 9, 30, holes=True)
    ref = T.label_overlap(lab, tru, S, G)
    for off_l, off_t in ((1, 0), (0, 3), (2, 2)):
        views = []
        for a, off in ((lab, off_l), (tru, off_t)):
            buf = torch.zeros(a.size + 8, dtype=torch.int32, device=DEV)
            v = buf[off:off + a.size].view(*a.shape)
            v.copy_(dev(a))
            assert v.data_ptr() % 16 == (4 * off) % 16
            views.append(v)
        assert_equals_spec(rag.label_overlap(views[0], views[1], S, G), ref)
    wide_l, wide_t = torch.full((96, 256), -1, dtype=torch.int32, device=DEV), torch.full((96, 256), -1, dtype=torch.int32, device=DEV)
    wide_l[:, ::2], wide_t[:, 1::2] = dev(lab), dev(tru)
    assert not wide_l[:, ::2].is_contiguous()
    assert_equals_spec(rag.label_overlap(wide_l[:, ::2], wide_t[:, 1::2], S, G), ref)


def test_bad_arguments_raise_on_the_host():
    from deepmerge_amd import rag
    tl = torch.zeros((16, 16), dtype=torch.int32, device=DEV)
    ov = rag.label_overlap(tl, tl, 1, 1)
    e = torch.zeros((1, 2), dtype=torch.int32, device=DEV)
    for bad in (lambda: rag.label_overlap(tl, tl.long(), 1, 1), lambda: rag.label_overlap(tl, tl[:8], 1, 1), lambda: rag.label_overlap(tl, tl, 0, 1),
                lambda: rag.label_overlap(tl, tl, 1, 0), lambda: rag.label_overlap(tl, tl, 1 << 61, 1), lambda: rag.label_overlap(tl[0], tl[0], 1, 1),
                lambda: rag.pair_flags(e, ov, 1.5), lambda: rag.pair_flags(e, ov, -0.1), lambda: rag.pair_flags(e.long(), ov),
                lambda: ov.coarsen(torch.zeros(2, dtype=torch.int32, device=DEV)), lambda: ov.coarsen(torch.zeros(1, dtype=torch.int64, device=DEV)),
                lambda: ov.coarsen(torch.full((1,), -1, dtype=torch.int32, device=DEV))):
        with pytest.raises(ValueError):
            bad()
    assert rag.pair_flags(e[:0], ov).shape == (0,)


# ---- pair flags ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,cell,tcell,counts", [(257, 301, 13, 40, (658, 312, 348)), (96, 128, 9, 30, (232, 99, 100))])
def test_pair_flags_match_the_spec(H, W, cell, tcell, counts):
    from deepmerge_amd import rag
    for holes in (False, True):
        lab, S, tru, G = voronoi_pair(H, W, cell, tcell, holes)
        tl = dev(lab)
        edges, _ = rag.rag_edges(tl, S)
        ov = rag.label_overlap(tl, dev(tru), S, G)
        ref = T.label_overlap(lab, tru, S, G)
        e = edges.cpu().numpy()
        for purity in (0.5, 0.6, 0.8, 1.0):
            got = rag.pair_flags(edges, ov, purity)
            want = T.pair_flags(e, ref, T.purity_pm(purity))
            assert got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), want), purity
            if purity == 0.6 and not holes:
                assert tuple(int((want == v).sum()) for v in (1, 0, -1)) == counts
        # endpoints outside [0,S) (the reference's -1 = "no polygon") are ambiguous
        odd = np.concatenate((e[:5], [[-1, 3], [3, -1], [S, 0], [0, S + 9]])).astype(np.int32)
        assert np.array_equal(rag.pair_flags(dev(odd), ov, 0.6).cpu().numpy(), T.pair_flags(odd, ref, 600))


# ---- coarsen ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def merged_case():
    """A real merge_regions run on a 257 x 301 raster and its overlap with a truth raster."""
    from deepmerge_amd import rag
    c = M.raster_case(257, 301, 13, 3, 3, 100, 558)
    lab, S = c["labels"], c["S"]
    tru, G = P.voronoi_labels(257, 301, 40, 2)
    tru[100:104, :] = -1
    tl, tt = dev(lab), dev(tru)
    edges, w = rag.rag_edges(tl, S)
    res = rag.merge_regions(dev(c["F"]), dev(c["ptr"]), dev(c["idx"]), edges, margin=1.0, weights=w)
    assert res.rounds >= 3 and res.ptr.numel() - 1 < S // 2        # guards the inputs
    return {"lab": lab, "S": S, "tru": tru, "G": G, "tl": tl, "tt": tt, "res": res, "ov": rag.label_overlap(tl, tt, S, G)}


def test_coarsen_equals_label_overlap_on_the_merged_raster(merged_case):
    from deepmerge_amd import rag
    m = merged_case
    res, ov = m["res"], m["ov"]
    assert_equals_spec(ov, T.label_overlap(m["lab"], m["tru"], m["S"], m["G"]))
    C = res.ptr.numel() - 1
    merged = res.labels(m["tl"])
    got = ov.coarsen(res.region_of)
    want = rag.label_overlap(merged, m["tt"], C, m["G"])
    for f in T.FIELDS:
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    assert_equals_spec(got, T.label_overlap(merged.cpu().numpy(), m["tru"], C, m["G"]))
    assert_equals_spec(got, T.coarsen(T.label_overlap(m["lab"], m["tru"], m["S"], m["G"]), res.region_of.cpu().numpy()))
    ident = torch.arange(m["S"], dtype=torch.int32, device=DEV)
    for f in T.FIELDS:
        assert torch.equal(getattr(ov.coarsen(ident), f), getattr(ov, f)), f


def test_merge_result_scores_every_round(merged_case):
    m = merged_case
    res, ov = m["res"], m["ov"]
    ref = T.label_overlap(m["lab"], m["tru"], m["S"], m["G"])
    per_round = []
    for r in range(res.rounds + 1):
        want = T.coarsen(ref, res.region_of_at(r).cpu().numpy())
        s = res.scores(ov, round=r)
        assert_scores_equal(s, want["summary"])
        per_round.append(s)
    assert_scores_equal(res.scores(ov), T.coarsen(ref, res.region_of.cpu().numpy())["summary"])
    assert res.scores(ov).sum_cells == per_round[-1].sum_cells
    # merging can only lose purity and only gain coverage; the pixel count never changes
    assert all(a.sum_owner >= b.sum_owner and a.sum_cover <= b.sum_cover and a.n == b.n for a, b in zip(per_round, per_round[1:]))
    assert per_round[0].n_regions > per_round[-1].n_regions


# ---- from_rasters ---------------------------------------------------------------------------------------------------------------------
def raster_image(H, W, cell, tcell):
    lab, S, tru, G = voronoi_pair(H, W, cell, tcell)
    rng = np.random.default_rng(H + W)
    base = rng.integers(0, 256, (3, (H + 31) // 32, (W + 31) // 32)).astype(np.uint8)
    tile = np.kron(base, np.ones((32, 32), np.uint8))[:, :H, :W].copy()
    return {"tile": tile, "labels": lab, "n_labels": S, "truth": tru, "n_truth": G}


@pytest.fixture(scope="module")
def images():
    return [raster_image(96, 128, 9, 30), raster_image(120, 100, 11, 35)]


@pytest.fixture(scope="module")
def spec_lists(images):
    """Per image, from the spec chain alone: edges, flags, points."""
    from oracle import rag as OR
    out = []
    for im in images:
        edges, _ = OR.rag_edges(im["labels"], im["n_labels"])
        flags = T.pair_flags(edges, T.label_overlap(im["labels"], im["truth"], im["n_labels"], im["n_truth"]), 600)
        out.append({"edges": edges, "flags": flags, "points": P.sample_points(im["labels"], im["n_labels"], 3)})
    return out


def global_pairs(images, spec_lists, flag, keep=None):
    off, rows = 0, []
    for t, (im, sp) in enumerate(zip(images, spec_lists)):
        sel = sp["flags"] == flag
        if keep is not None:
            sel &= keep[t]
        rows.append(sp["edges"][sel] + off)
        off += im["n_labels"]
    return np.concatenate(rows)


def test_from_rasters_builds_the_spec_pair_lists(images, spec_lists):
    from deepmerge_amd.dataset import PairDataset
    ds = PairDataset.from_rasters(images, k=3, min_purity=0.6, seed=5, device=DEV)
    pos, neg = global_pairs(images, spec_lists, 1), global_pairs(images, spec_lists, 0)
    assert len(pos) > 50 and len(neg) > 50 and all((sp["flags"] == -1).any() for sp in spec_lists)
    assert (ds.positive_pair_number, ds.negative_pair_number) == (len(pos), len(neg)) and len(ds) == len(pos) + len(neg)
    assert np.array_equal(ds.host.pairs, np.concatenate((pos, neg))) and ds.host.flag.tolist() == [1] * len(pos) + [0] * len(neg)
    # points, windows and point lists are sample_points'
    for f, key in (("pt_xy", "xy"), ("pt_inner", "inner"), ("pt_obj", "obj")):
        assert np.array_equal(getattr(ds.host, f), np.concatenate([sp["points"][key] for sp in spec_lists])), f
    ptr = np.concatenate([[0]] + [sp["points"]["ptr"][1:].astype(np.int64) + sum(len(q["points"]["xy"]) for q in spec_lists[:t])
                                  for t, sp in enumerate(spec_lists)])
    assert np.array_equal(ds.host.poly_off, ptr) and np.array_equal(ds.host.poly_pts, np.arange(ptr[-1]))
    assert ds.host.pt_tile.tolist() == [0] * len(spec_lists[0]["points"]["xy"]) + [1] * len(spec_lists[1]["points"]["xy"])
    assert ds.host.tiles.shape == (2, 3, 120, 128) and np.array_equal(ds.host.tiles[0, :, :96, :128], images[0]["tile"])
    from oracle import rag as OR
    designed = OR.designed_features(OR.label_stats(images[1]["labels"], images[1]["tile"], images[1]["n_labels"]))
    n0 = len(spec_lists[0]["points"]["xy"])
    assert np.array_equal(ds.host.pt_region[n0:], designed[spec_lists[1]["points"]["label"]])
    # an epoch draws, and its flags are a permutation of the spec's
    table = ds.epoch(0, 16)
    assert len(table) == -(-len(ds) // 16)
    flag = table.cols["flag"].cpu().numpy()
    assert flag.shape == (len(ds),) and sorted(flag.tolist()) == [0.0] * len(neg) + [1.0] * len(pos)
    assert (flag[:64] != flag[0]).any()                            # shuffled, not the build order
    # every drawn pair is a listed pair with its own flag: the drawn points' polygons and flags, sorted, are the pair table's
    import train_smt_ref as TR
    rl, rr = TR.blocked_rows(len(ds), 16)
    pid = table.cols["point_id"].cpu().numpy()
    poly_of = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    drawn = np.stack((poly_of[pid[rl]], poly_of[pid[rr]], flag.astype(np.int64)), 1)
    listed = np.concatenate((ds.host.pairs, ds.host.flag[:, None]), 1)
    assert np.array_equal(drawn[np.lexsort(drawn.T[::-1])], listed[np.lexsort(listed.T[::-1])])


def test_from_rasters_holdout_is_a_reproducible_disjoint_split(images, spec_lists):
    from deepmerge_amd.dataset import PairDataset
    train, val = PairDataset.from_rasters(images, holdout=0.25, seed=5, device=DEV)
    full = {tuple(p) for p in np.concatenate((global_pairs(images, spec_lists, 1), global_pairs(images, spec_lists, 0))).tolist()}
    a, b = {tuple(p) for p in train.host.pairs.tolist()}, {tuple(p) for p in val.host.pairs.tolist()}
    assert len(a) == len(train) and len(b) == len(val) and not (a & b) and (a | b) == full
    assert 0.15 * len(full) < len(b) < 0.35 * len(full)            # ~650 pairs at p = 1/4: 0.25 +- 6 sigma
    assert train.positive_pair_number + val.positive_pair_number == len(global_pairs(images, spec_lists, 1))
    # which pair goes where is dataset.holdout_hash's decision (tests/test_truth_host.py restates its arithmetic)
    from deepmerge_amd.dataset import holdout_hash
    to_val = [holdout_hash(5, t, sp["edges"][:, 0], sp["edges"][:, 1]) % np.uint64(1000000) < np.uint64(250000) for t, sp in enumerate(spec_lists)]
    for ds, keep in ((train, [~v for v in to_val]), (val, to_val)):
        assert np.array_equal(ds.host.pairs, np.concatenate((global_pairs(images, spec_lists, 1, keep), global_pairs(images, spec_lists, 0, keep))))
    again_t, again_v = PairDataset.from_rasters(images, holdout=0.25, seed=5, device=DEV)
    assert np.array_equal(again_t.host.pairs, train.host.pairs) and np.array_equal(again_v.host.pairs, val.host.pairs)
    other_t, _ = PairDataset.from_rasters(images, holdout=0.25, seed=6, device=DEV)
    assert not np.array_equal(other_t.host.pairs, train.host.pairs)
    assert np.array_equal(val.host.pt_xy, train.host.pt_xy) and np.array_equal(val.host.poly_off, train.host.poly_off)


def test_from_rasters_names_the_image_without_unambiguous_pairs(images):
    from deepmerge_amd.dataset import PairDataset
    blank = dict(images[1], truth=np.full_like(images[1]["truth"], -1))
    with pytest.raises(ValueError, match="image 1: no unambiguous pair"):
        PairDataset.from_rasters([images[0], blank], device=DEV)


def test_one_training_step_from_rasters(images):
    """tile + labels + truth -> PairDataset -> one step of the existing trainer: batch 4, v3 depth [1,1,1], 3 scales."""
    from deepmerge_amd.dataset import PairDataset
    from deepmerge_amd.feed import PairFeed
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    from deepmerge_amd.trainer import PairTrainer
    scales = [32, 64, 128]
    ds = PairDataset.from_rasters(images[:1], n_scales=3, seed=1, device=DEV)
    torch.manual_seed(3)
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=list(scales), depth=[1, 1, 1], in_c=3, numerics="bf16").to(DEV)
    before = [p.detach().clone() for p in net.parameters()]
    trainer = PairTrainer(net, margin=1.0, lr=1e-3, lamda=0.1, belta=0)
    feed = PairFeed(ds.tiles, scales, 4, ds.max_window(3), numerics="bf16")
    table = ds.epoch(0, 4)
    assert table.pairs_in_step(0) == 4
    loss = float(trainer.step(*feed.fill(table.step(0)), lr=1e-3))
    feed.check()
    assert math.isfinite(loss)
    assert any(not torch.equal(a, b) for a, b in zip(before, net.parameters()))
