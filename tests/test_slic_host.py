"""CPU: the SLIC / connected-components rule itself (tests/slic_ref.py, the spec the kernels of csrc/dm_slic.hip must equal bit for
bit) holds the properties the issue states, and the library's new entry points validate their arguments without a GPU."""
import os

import numpy as np
import pytest

import slic_ref as R


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


def four_connected(labels, n):
    """Every id 0..n-1 is one 4-connected component: relabelling the components changes nothing."""
    again, m = R.connected_labels(labels)
    return m == n and np.array_equal(again, labels)


def first_pixel_order(labels, n):
    flat = labels.reshape(-1)
    ids, first = np.unique(flat, return_index=True)
    return np.array_equal(ids, np.arange(n)) and bool((np.diff(first) > 0).all())


def has_neighbour(labels, n):
    a, b, _ = R.region_edges(labels, n)
    out = np.zeros(n, bool)
    out[a] = True
    out[b] = True
    return out


IMAGES = {
    "blocks": lambda: R.block_image(3, 150, 170, 23, 1),
    "noise": lambda: R.noise_image(4, 97, 131, 2),
    "constant": lambda: np.full((1, 61, 83), 77, np.uint8),
}


@pytest.fixture(scope="module")
def results():
    """One run of the spec per image, shared by the property tests."""
    out = {}
    for name, make in IMAGES.items():
        tile = make()
        cell = 11
        labels, n, rounds = R.slic(tile, cell=cell, compactness=10, iters=3, return_rounds=True)
        out[name] = (tile, cell, labels, n, rounds)
    return out


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_regions_are_connected_dense_ordered_and_large_enough(results, name):
    tile, cell, labels, n, rounds = results[name]
    print(f"{name}: n = {n}, absorption rounds = {rounds}")
    assert labels.dtype == np.int32 and labels.shape == tile.shape[1:]
    assert four_connected(labels, n)
    assert first_pixel_order(labels, n)
    area = np.bincount(labels.reshape(-1), minlength=n)
    small = (area < R.default_min_size(cell)) & has_neighbour(labels, n)
    assert not small.any()
    assert rounds <= int(np.ceil(np.log2(labels.size)))


def test_no_iterations_full_compactness_constant_image_gives_the_clipped_grid():
    H, W, cell = 50, 67, 9
    labels, n = R.slic(np.full((2, H, W), 5, np.uint8), cell=cell, compactness=255, iters=0, min_size=1)
    gy, gx = -(-H // cell), -(-W // cell)
    yy, xx = np.mgrid[0:H, 0:W]
    # cells are numbered row by row, which is also their first-pixel order
    assert n == gy * gx and np.array_equal(labels, ((yy // cell) * gx + xx // cell).astype(np.int32))


def test_a_straight_colour_edge_is_never_crossed():
    H, W = 90, 110
    tile = np.zeros((3, H, W), np.uint8)
    tile[:, :, :47] = 40
    tile[:, :, 47:] = 200
    labels, n = R.slic(tile, cell=13, compactness=1, iters=4)
    left = np.unique(labels[:, :47])
    right = np.unique(labels[:, 47:])
    assert n >= 2 and np.intersect1d(left, right).size == 0


def test_min_size_one_absorbs_nothing_and_a_huge_one_leaves_a_single_region():
    tile = R.block_image(3, 64, 80, 16, 3)
    lab, _ = R.iterate(tile, 8, 10, 2)
    comp, m = R.connected_labels(lab)
    labels, n, rounds = R.slic(tile, cell=8, compactness=10, iters=2, min_size=1, return_rounds=True)
    assert rounds == 0 and n == m and np.array_equal(labels, comp)
    labels, n = R.slic(tile, cell=8, compactness=10, iters=2, min_size=64 * 80 + 1)
    assert n == 1 and not labels.any()


def test_wide_distance_does_not_wrap():
    """cell = 129: cell^2 * 4 * 255^2 > 2^32; the spec's int64 D must order like Python integers."""
    tile = R.noise_image(4, 40, 40, 5)
    centres, grid = R.initial_centres(tile, 129)
    lab = R.assign(tile, centres, 129, 255, grid)
    assert grid == (1, 1) and not lab.any()
    c = [int(v) for v in centres[0]]
    d = 129 * 129 * sum((int(tile[b, 0, 0]) - c[2 + b]) ** 2 for b in range(4)) + 255 * 255 * (c[0] ** 2 + c[1] ** 2)
    assert d < 2 ** 62


RASTERS = {
    "serpentine": lambda: R.serpentine(130, 130),
    "checkerboard": lambda: (np.indices((37, 41)).sum(0) % 2).astype(np.int32),
    "single": lambda: np.full((20, 33), -7, np.int32),
    "classes": lambda: np.random.default_rng(4).integers(0, 3, (90, 75)).astype(np.int32),
}


@pytest.mark.parametrize("name", sorted(RASTERS))
@pytest.mark.parametrize("background", [None, 0])
def test_component_labelling_equals_scipy_per_value(name, background):
    ndimage = pytest.importorskip("scipy.ndimage")
    r = RASTERS[name]()
    labels, n = R.connected_labels(r, background)
    assert labels.dtype == np.int32
    total = 0
    for v in np.unique(r):
        if background is not None and v == background:
            assert (labels[r == v] == -1).all()
            continue
        ref, m = ndimage.label(r == v)                            # default structure: 4-connectivity
        total += m
        mine = labels[r == v]
        pairs = np.unique(np.stack((mine, ref[r == v])), axis=1)
        assert pairs.shape[1] == m and np.unique(pairs[0]).size == m      # a bijection between the two numberings
    assert total == n
    live = labels >= 0
    assert first_pixel_order(labels[live], n) if n else not live.any()


def test_checkerboard_has_one_component_per_pixel():
    r = RASTERS["checkerboard"]()
    labels, n = R.connected_labels(r)
    assert n == r.size and np.array_equal(labels.reshape(-1), np.arange(r.size))


# ---- the library's side, without a GPU ------------------------------------------------------------------------------------------
NEW = ("dm_slic_iterate", "dm_connected_labels", "dm_label_area", "dm_slic_absorb_pick")


def test_header_signatures_and_exports_agree_and_abi_is_still_6(built):
    import ctypes
    lib = built.lib()
    assert lib.dm_abi_version() == 7
    declared = built.declared_symbols()
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW:
        assert name in declared and name in built.SIGNATURES and hasattr(raw, name), name
    assert sorted(built.SIGNATURES) == declared
    text = open(built.HEADER_PATH).read()
    for name, nargs in zip(NEW, (11, 10, 6, 10)):
        proto = text[text.index("int " + name + "("):]
        proto = proto[:proto.index(";")]
        assert proto.count(",") + 1 == nargs == len(built.SIGNATURES[name][1]), name


def test_slic_entry_points_validate_before_any_launch(built):
    lib = built.lib()
    p = 4096                                                       # any non-null address: validation never dereferences
    it = lambda *, tile=p, bands=3, H=8, W=8, cell=8, comp=10, iters=1, centres=p, sums=p, labels=p: \
        lib.dm_slic_iterate(tile, bands, H, W, cell, comp, iters, centres, sums, labels, None)
    cc = lambda *, raster=p, H=8, W=8, parent=p, chunks=p, labels=p, n=p: lib.dm_connected_labels(raster, H, W, 0, 0, parent, chunks, labels, n, None)
    ar = lambda *, labels=p, H=8, W=8, S=4, area=p: lib.dm_label_area(labels, H, W, S, area, None)
    pk = lambda *, edges=p, weights=p, E=4, area=p, S=4, min_size=2, best=p, merge=p, n=p: \
        lib.dm_slic_absorb_pick(edges, weights, E, area, S, min_size, best, merge, n, None)
    cases = [
        (lambda: it(tile=None), b"dm_slic_iterate: null pointer"),
        (lambda: it(centres=None), b"dm_slic_iterate: null pointer"),
        (lambda: it(sums=None), b"dm_slic_iterate: null pointer"),
        (lambda: it(labels=None), b"dm_slic_iterate: null pointer"),
        (lambda: it(H=0), b"dm_slic_iterate: bad sizes"),
        (lambda: it(bands=0), b"dm_slic_iterate: bad sizes"),
        (lambda: it(H=1 << 16, W=1 << 15), b"dm_slic_iterate: bad sizes"),
        (lambda: it(cell=3), b"dm_slic_iterate: cell = 3 outside 4..256"),
        (lambda: it(cell=257), b"dm_slic_iterate: cell = 257 outside 4..256"),
        (lambda: it(comp=-1), b"dm_slic_iterate: compactness = -1 outside 0..255"),
        (lambda: it(comp=256), b"dm_slic_iterate: compactness = 256 outside 0..255"),
        (lambda: it(iters=-1), b"dm_slic_iterate: iters = -1 is negative"),
        (lambda: cc(raster=None), b"dm_connected_labels: null pointer"),
        (lambda: cc(parent=None), b"dm_connected_labels: null pointer"),
        (lambda: cc(chunks=None), b"dm_connected_labels: null pointer"),
        (lambda: cc(labels=None), b"dm_connected_labels: null pointer"),
        (lambda: cc(n=None), b"dm_connected_labels: null pointer"),
        (lambda: cc(W=0), b"dm_connected_labels: bad sizes"),
        (lambda: cc(H=1 << 16, W=1 << 15), b"dm_connected_labels: bad sizes"),
        (lambda: ar(labels=None), b"dm_label_area: null pointer"),
        (lambda: ar(area=None), b"dm_label_area: null pointer"),
        (lambda: ar(S=0), b"dm_label_area: bad sizes"),
        (lambda: ar(H=1 << 16, W=1 << 15), b"dm_label_area: bad sizes"),
        (lambda: pk(edges=None), b"dm_slic_absorb_pick: null pointer"),
        (lambda: pk(best=None), b"dm_slic_absorb_pick: null pointer"),
        (lambda: pk(n=None), b"dm_slic_absorb_pick: null pointer"),
        (lambda: pk(E=0), b"dm_slic_absorb_pick: bad sizes"),
        (lambda: pk(S=0), b"dm_slic_absorb_pick: bad sizes"),
        (lambda: pk(min_size=0), b"dm_slic_absorb_pick: bad sizes"),
    ]
    for call, msg in cases:
        assert call() == -1, msg
        assert msg in lib.dm_last_error(), (msg, lib.dm_last_error())


def test_slic_has_no_cpu_fallback_and_checks_its_arguments_on_the_host(built):
    import torch
    from deepmerge_amd import rag
    tile = torch.zeros((3, 16, 16), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag.slic(tile)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag.connected_labels(torch.zeros((4, 4), dtype=torch.int32))
