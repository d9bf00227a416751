"""GPU: rag.clearance / rag.sample_points (csrc/dm_points.hip) against the numpy spec tests/points_ref.py, and
FeatureIO.merge_tile against the hand-written chain of the public calls -- every comparison is exact integer or bit equality."""
import numpy as np
import pytest
import torch

import points_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("xy", "label", "inner", "obj", "ptr", "idx", "bbox", "round")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assert_equals_spec(got, ref):
    for f in FIELDS:
        g, w = getattr(got, f).cpu().numpy(), ref[f]
        assert g.dtype == w.dtype == np.int32 and g.shape == w.shape, (f, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), f


def raster(H, W, cell, seed, holes=False, specks=False):
    lab, S = R.voronoi_labels(H, W, cell, seed)
    rng = np.random.default_rng(seed + 100)
    if holes:                                                     # ids outside [0, S): a band of -1, a blob of S + 7, scattered S
        lab[H // 3:H // 3 + 2, :] = -1
        lab[H // 2:H // 2 + 9, W // 4:W // 4 + 11] = S + 7
        lab[rng.random((H, W)) < 0.01] = S
    if specks:                                                    # single-pixel superpixels S, S + 1, ... inside the others
        ys, xs = rng.integers(0, H, 40), rng.integers(0, W, 40)
        keep = np.unique(ys.astype(np.int64) * W + xs)
        lab.reshape(-1)[keep] = S + np.arange(keep.size, dtype=np.int32)
        S += keep.size
    return lab, S


CASES = [  # H, W, cell, k, max_window, holes, specks
    (512, 512, 29, 3, 384, False, False),
    (512, 512, 13, 8, 384, True, False),
    (257, 301, 13, 3, 384, False, True),        # not multiples of the tile, odd width
    (257, 301, 13, 1, 31, True, True),
    (100, 77, 40, 8, 31, False, False),
    (64, 128, 5, 8, 384, True, True),           # k > area for most superpixels
    (33, 17, 40, 3, 384, False, False),
    (1, 1, 3, 3, 384, False, False),
    (5, 700, 9, 3, 384, True, False),
    (700, 6, 9, 8, 31, False, True),
    (400, 400, 1000, 3, 384, False, False),     # one label fills the raster: the cap
    (400, 404, 1000, 1, 31, False, False),
]


@pytest.mark.parametrize("H,W,cell,k,mw,holes,specks", CASES)
def test_clearance_and_points_match_the_spec(H, W, cell, k, mw, holes, specks):
    from deepmerge_amd import rag
    lab, S = raster(H, W, cell, H + W + k, holes, specks)
    tl = dev(lab)
    c = rag.clearance(tl, mw)
    assert c.dtype == torch.uint16 and tuple(c.shape) == (H, W)
    ref = R.sample_points(lab, S, k, mw)
    assert np.array_equal(c.cpu().numpy(), ref["clearance"])
    if H * W <= 6000:
        assert np.array_equal(ref["clearance"], R.clearance_brute(lab, mw))
    got = rag.sample_points(tl, S, k=k, max_window=mw)
    assert_equals_spec(got, ref)
    area = np.bincount(lab[(lab >= 0) & (lab < S)], minlength=S)
    assert np.array_equal(np.diff(ref["ptr"]), np.minimum(k, area))
    if specks:
        assert (area == 1).sum() >= 10
    if k == 8 and cell <= 5:
        assert (area < k).sum() > 10                               # k > area really occurs
    assert np.array_equal(tl.cpu().numpy(), lab)                   # the input is untouched
    d = torch.arange(S * 15, dtype=torch.float32, device=DEV).reshape(S, 15)
    assert torch.equal(got.region_features(d), d[got.label.long()])


def test_unaligned_raster_and_more_labels_than_table_slots():
    """A raster view that is not 16-byte aligned takes the scalar loads; a noise raster puts more than 64 labels into every 64x64
    tile, so labels overflow the tile's LDS table and go to global memory directly."""
    from deepmerge_amd import rag
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 3000, (128, 192)).astype(np.int32)
    lab[20:90, 30:150] = np.repeat(np.repeat(rng.integers(0, 3000, (10, 15)), 7, 0), 8, 1)
    for off in (0, 1, 3):
        buf = torch.zeros(lab.size + 8, dtype=torch.int32, device=DEV)
        view = buf[off:off + lab.size].view(*lab.shape)
        view.copy_(dev(lab))
        assert view.data_ptr() % 16 == (4 * off) % 16
        for k in (1, 3):
            assert_equals_spec(rag.sample_points(view, 3000, k=k), R.sample_points(lab, 3000, k))


def test_more_labels_than_one_scan_tile():
    """5000 labels: the emit's exclusive scan walks two tiles of 4096 counts, the second one partly filled, and carries the first
    tile's total into it."""
    from deepmerge_amd import rag
    lab = np.random.default_rng(5).integers(0, 5000, (96, 128)).astype(np.int32)
    ref = R.sample_points(lab, 5000, 3)
    assert ref["ptr"][4096] == 8457 and ref["ptr"][5000] == 10289
    assert_equals_spec(rag.sample_points(dev(lab), 5000, k=3), ref)


def test_two_runs_are_identical_and_a_side_stream_works():
    from deepmerge_amd import rag
    lab, S = raster(300, 420, 17, 5, holes=True)
    tl = dev(lab)
    a = rag.sample_points(tl, S, k=3)
    b = rag.sample_points(tl, S, k=3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = rag.sample_points(tl, S, k=3)
        cc = rag.clearance(tl)
    side.synchronize()
    ref = R.sample_points(lab, S, 3)
    for got in (a, b, c):
        assert_equals_spec(got, ref)
    assert np.array_equal(cc.cpu().numpy(), ref["clearance"]) and torch.equal(tl.cpu(), torch.from_numpy(lab))


def test_bad_arguments_raise_on_the_host():
    from deepmerge_amd import rag
    tl = torch.zeros((16, 16), dtype=torch.int32, device=DEV)
    for bad in (lambda: rag.sample_points(tl, 1, k=0), lambda: rag.sample_points(tl, 1, k=17), lambda: rag.sample_points(tl, 0),
                lambda: rag.sample_points(tl, 1, max_window=385), lambda: rag.clearance(tl, 0), lambda: rag.clearance(tl.long()),
                lambda: rag.sample_points(tl[0], 1), lambda: rag.clearance(tl[:0])):
        with pytest.raises(ValueError):
            bad()


def test_full_size_tile_by_properties():
    """4096 x 4096, cell 29 (the geometry of workload.config4r): the brute-force spec is too slow here, so check what defines the
    result -- every point lies in its superpixel, its `inner` square is uniformly labelled and the next larger one is not (unless
    capped or cut by the raster edge), the CSR is the one points_to_csr derives, bbox and counts agree with label_stats."""
    from deepmerge_amd import rag, dataset
    from deepmerge_amd.workload import voronoi_raster
    torch.manual_seed(0)
    H = W = 4096
    k = 3
    tl, _cy, _cx, S = voronoi_raster(H, W, 29)
    keep = tl.clone()
    tile = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, device=DEV)
    st = rag.label_stats(tl, tile, S)
    pts = rag.sample_points(tl, S, k=k)
    assert torch.equal(tl, keep)
    P = pts.xy.shape[0]
    x, y = pts.xy[:, 0].long(), pts.xy[:, 1].long()
    assert 3 * 19000 <= P <= 3 * S and bool(((x >= 0) & (x < W) & (y >= 0) & (y < H)).all())
    assert torch.equal(tl[y, x], pts.label)                        # every point lies in its superpixel
    ptr, idx = rag.points_to_csr(tl, pts.xy, S)
    assert torch.equal(ptr, pts.ptr) and torch.equal(idx, pts.idx)
    assert torch.equal(pts.bbox, st["bbox"])
    assert torch.equal((pts.ptr[1:] - pts.ptr[:-1]).long(), st["count"].clamp(max=k))
    assert torch.equal(pts.round.long(), torch.arange(P, device=DEV) - pts.ptr[pts.label.long()].long())
    lin = y * W + x
    assert torch.unique(lin).numel() == P                          # no duplicates
    w = dataset.window_sides(pts.inner.cpu().numpy(), pts.obj.cpu().numpy(), 4)
    assert w.min() >= 1 and w.max() <= 384
    side = torch.maximum(st["bbox"][:, 2] - st["bbox"][:, 0], st["bbox"][:, 3] - st["bbox"][:, 1])[pts.label.long()] + 1
    assert torch.equal(pts.obj, torch.minimum(side, (384 + 2 * pts.inner) // 3))
    lab = tl.cpu().numpy()
    xs, ys, inner, label = (t.cpu().numpy().astype(np.int64) for t in (x, y, pts.inner, pts.label))
    assert (inner % 2 == 1).all() and inner.max() < 383            # no superpixel of this raster reaches the cap
    h = inner // 2
    assert (xs - h >= 0).all() and (ys - h >= 0).all() and (xs + h < W).all() and (ys + h < H).all()
    uniform, larger_differs = np.ones(P, bool), np.zeros(P, bool)
    for r in range(int(h.max()) + 2):                              # ring r of every point at once
        ring = [(dx, dy) for dx in range(-r, r + 1) for dy in (-r, r)] + [(dx, dy) for dy in range(-r + 1, r) for dx in (-r, r)]
        for dx, dy in ring:
            xx, yy = xs + dx, ys + dy
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            same = np.zeros(P, bool)
            same[inside] = lab[yy[inside], xx[inside]] == label[inside]
            uniform &= same | (r > h)
            larger_differs |= ~same & (r == h + 1)                 # another label, or cut by the raster edge
    assert uniform.all() and larger_differs.all()
    # round 0 is the pixel farthest from the boundary: its clearance is the superpixel's maximum
    c = rag.clearance(tl).to(torch.int32).reshape(-1)
    top = torch.zeros(S, dtype=torch.int32, device=DEV).scatter_reduce(0, tl.reshape(-1).long(), c, "amax")
    first = pts.round == 0
    assert torch.equal(((pts.inner[first] + 1) // 2), top[pts.label[first].long()])
    again = rag.sample_points(tl, S, k=k)
    for f in FIELDS:
        assert torch.equal(getattr(again, f), getattr(pts, f)), f


def test_merge_tile_equals_the_hand_written_chain():
    from deepmerge_amd import rag
    from deepmerge_amd.ExtractFeatures import FeatureIO
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    torch.manual_seed(1)
    lab, S = R.voronoi_labels(256, 256, 23, 11)
    S += 2                                                         # two ids that never occur
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, (3, 4, 4)).astype(np.uint8)        # coarse colour blocks + noise: neighbours differ and resemble
    tile = np.clip(np.kron(base, np.ones((64, 64), np.uint8)).astype(np.int64) + rng.integers(-8, 9, (3, 256, 256)), 0, 255).astype(np.uint8)
    tl, tt = dev(lab), dev(tile)
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=[32, 64, 128], depth=[1, 1, 1], in_c=3, numerics="fp32")
    fio = FeatureIO(net, None, DEV)
    margin = 1.0
    # the chain, written out with the public calls
    st = rag.label_stats(tl, tt, S)
    designed = rag.designed_features(st)
    edges, w = rag.rag_edges(tl, S)
    pts = rag.sample_points(tl, S, k=3)
    assert_equals_spec(pts, R.sample_points(lab, S, 3))
    F = fio.extract_features_from_tile(tt, pts.xy, pts.inner, pts.obj, designed[pts.label.long()], batch_size=100).clone()
    # choose the margin inside the spread of the edge scores, so that rounds really merge and really stop
    from deepmerge_amd.ExtractFeatures import rag_similarity_sweep
    _, simi, _ = rag_similarity_sweep(F, pts.ptr, pts.idx, edges, 1.0)
    margin = float(simi.float().median())
    want = rag.merge_regions(F, pts.ptr, pts.idx, edges, margin=margin, weights=w, stats=st)
    got, gpts = fio.merge_tile(tt, tl, S, k=3, margin=margin, batch_size=100)
    assert want.rounds >= 1 and 1 <= want.ptr.numel() - 1 < S
    for f in FIELDS:
        assert torch.equal(getattr(gpts, f), getattr(pts, f)), f
    assert torch.equal(got.region_of, want.region_of) and torch.equal(got.history, want.history)
    assert torch.equal(got.history_simi.view(torch.int32), want.history_simi.view(torch.int32))
    assert got.rounds == want.rounds and got.regions_per_round == want.regions_per_round
    merged = got.labels(tl)
    assert torch.equal(merged, want.labels(tl)) and torch.equal(merged, got.region_of[tl.long()])
    C = got.ptr.numel() - 1
    st2 = rag.label_stats(merged, tt, C)
    for key in ("count", "sum", "sumsq", "bbox", "peri"):
        assert torch.equal(st2[key], got.stats[key]), key
    assert torch.equal(tl.cpu(), torch.from_numpy(lab)) and torch.equal(tt.cpu(), torch.from_numpy(tile))
