"""CPU: the scene form of the SLIC rule (tests/scene_slic_ref.py: tile-local components joined across seams, numbered by scene-wide
first pixel, absorbed on the folded graph only) equals the rule on the whole raster (tests/slic_ref.py) whatever the tiling, and
the library's new entry points and the Python calls validate their arguments without a GPU."""
import os

import numpy as np
import pytest

import scene_slic_ref as S
import slic_ref as R

SIZES = {"a": (70, 90), "b": (61, 53)}
CELLS = (4, 5, 8, 16)
BANDS = (1, 3, 4)


def tilings(H, W):
    return [(H, W), (32, 32), (17, 23), (5, 7), (64, 64), (1, W)]


def image(kind, size, bands, seed):
    H, W = SIZES[size]
    return R.block_image(bands, H, W, 13, seed) if kind == "blocks" else R.noise_image(bands, H, W, seed)


# every image and size with every band count and every cell
CONFIGS = [(kind, size, bands, cell) for kind in ("blocks", "noise") for size in sorted(SIZES) for bands in BANDS for cell in CELLS]

_cache = {}


def whole(config):
    """Per configuration, once: the image's assigned raster (steps 1-3) and slic_ref.slic's result on it."""
    if config not in _cache:
        kind, size, bands, cell = config
        img = image(kind, size, bands, seed=7 + CELLS.index(cell) + 4 * BANDS.index(bands))
        assigned, _ = R.iterate(img, cell, 10, 3)
        comp, n = R.connected_labels(assigned)
        _cache[config] = (assigned, R.absorb(comp, n, R.default_min_size(cell)))
    return _cache[config]


@pytest.fixture(scope="module")
def infos():
    """What the cases saw, for the preconditions at the end of the module."""
    return []


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"{c[0]}-{c[1]}-b{c[2]}-cell{c[3]}")
def test_scene_form_equals_the_whole_raster_for_every_tiling(config, infos):
    assigned, (labels, n, rounds) = whole(config)
    H, W = assigned.shape
    for tiling in tilings(H, W):
        info = {}
        got, m, r = S.components_and_absorption(assigned, tiling, R.default_min_size(config[3]), info)
        print(f"{config} tiling {tiling}: n = {m}, rounds = {r}, provisional = {info['provisional']}, components = {info['components']}")
        assert got.dtype == np.int32 and (m, r) == (n, rounds), (config, tiling)
        assert np.array_equal(got, labels), (config, tiling)
        infos.append((tiling == (H, W), info))


def test_the_cases_meet_what_the_scene_form_is_about(infos):
    """Not vacuous: regions lie in two cores, picks join components of different cores, the scene-wide rank differs from the
    provisional order.  (Runs behind the cases above, in file order.)"""
    if not infos:
        for config in CONFIGS[:4]:
            assigned, _ = whole(config)
            for tiling in tilings(*assigned.shape):
                info = {}
                S.components_and_absorption(assigned, tiling, R.default_min_size(config[3]), info)
                infos.append((tiling == assigned.shape, info))
    tiled = [info for single, info in infos if not single]
    assert any(i["region_in_two_cores"] for i in tiled)
    assert any(i["cross_core_pick"] for i in tiled)
    assert any(i["rank_differs"] for i in tiled)
    assert any(i["seam_unions"] > 0 for i in tiled)
    for single, info in infos:
        if single:                                                # one core: nothing to join, nothing to reorder
            assert info["seam_unions"] == 0 and not info["rank_differs"] and info["provisional"] == info["components"]


def test_slic_in_cores_equals_slic_ref_end_to_end():
    """Through the front door, with explicit min_size and other iters / compactness."""
    img = R.block_image(3, 61, 53, 9, 21)
    for cell, comp, iters, min_size in ((5, 3, 0, 9), (8, 40, 2, None), (16, 10, 1, 1)):
        want = R.slic(img, cell, comp, iters, min_size, return_rounds=True)
        for tiling in ((17, 23), (5, 7), (1, 53)):
            got = S.slic(img, tiling, cell, comp, iters, min_size)
            assert got[1:] == want[1:] and np.array_equal(got[0], want[0]), (cell, tiling)


# ---- the library's side, without a GPU ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


NEW = ("dm_scene_slic_init", "dm_scene_slic_pass", "dm_scene_slic_update")


def test_new_entries_are_declared_exported_and_the_abi_is_still_7(built):
    import ctypes
    lib = built.lib()
    assert lib.dm_abi_version() == 7
    declared = built.declared_symbols()
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW:
        assert name in declared and name in built.SIGNATURES and hasattr(raw, name), name
    assert sorted(built.SIGNATURES) == declared
    text = open(built.HEADER_PATH).read()
    for name, nargs in zip(NEW, (12, 14, 4)):
        proto = text[text.index("int " + name + "("):]
        proto = proto[:proto.index(";")]
        assert proto.count(",") + 1 == nargs == len(built.SIGNATURES[name][1]), name


def test_scene_slic_entry_points_validate_before_any_launch(built):
    lib = built.lib()
    p = 4096                                                       # any non-null address: validation never dereferences
    big = (1 << 31) - 1
    init = lambda *, core=p, bands=3, h=8, w=8, y0=0, x0=0, H=16, W=16, cell=8, centres=p, sums=p: \
        lib.dm_scene_slic_init(core, bands, h, w, y0, x0, H, W, cell, centres, sums, None)
    ps = lambda *, core=p, bands=3, h=8, w=8, y0=0, x0=0, H=16, W=16, cell=8, comp=10, centres=p, sums=p, labels=p: \
        lib.dm_scene_slic_pass(core, bands, h, w, y0, x0, H, W, cell, comp, centres, sums, labels, None)
    up = lambda *, K=4, centres=p, sums=p: lib.dm_scene_slic_update(K, centres, sums, None)
    cases = []
    for name, call in (("dm_scene_slic_init", init), ("dm_scene_slic_pass", ps)):
        cases += [
            (lambda call=call: call(core=None), name + ": null pointer"),
            (lambda call=call: call(centres=None), name + ": null pointer"),
            (lambda call=call: call(bands=0), name + ": bad core"),
            (lambda call=call: call(h=0), name + ": bad core"),
            (lambda call=call: call(w=-1), name + ": bad core"),
            (lambda call=call: call(h=1 << 16, w=1 << 15, H=1 << 16, W=1 << 15), name + ": bad core"),
            (lambda call=call: call(y0=-1), name + ": the core does not lie in the scene"),
            (lambda call=call: call(x0=-1), name + ": the core does not lie in the scene"),
            (lambda call=call: call(y0=9), name + ": the core does not lie in the scene"),
            (lambda call=call: call(x0=9), name + ": the core does not lie in the scene"),
            (lambda call=call: call(y0=big, H=big), name + ": the core does not lie in the scene"),
            (lambda call=call: call(H=0), name + ": the core does not lie in the scene"),
            (lambda call=call: call(cell=3), name + ": cell outside 4..256"),
            (lambda call=call: call(cell=257), name + ": cell outside 4..256"),
            (lambda call=call: call(H=big, W=big, cell=4), name + ": the grid has 2^31 centres or more"),
        ]
    cases += [
        (lambda: init(sums=None), "dm_scene_slic_init: null pointer"),
        (lambda: ps(sums=None, labels=None), "dm_scene_slic_pass: null pointer"),
        (lambda: ps(comp=-1), "dm_scene_slic_pass: compactness = -1 outside 0..255"),
        (lambda: ps(comp=256), "dm_scene_slic_pass: compactness = 256 outside 0..255"),
        (lambda: up(centres=None), "dm_scene_slic_update: null pointer"),
        (lambda: up(sums=None), "dm_scene_slic_update: null pointer"),
        (lambda: up(K=0), "dm_scene_slic_update: K = 0 is not positive"),
        (lambda: up(K=-5), "dm_scene_slic_update: K = -5 is not positive"),
    ]
    for call, msg in cases:
        assert call() == -1, msg
        assert msg.encode() in lib.dm_last_error(), (msg, lib.dm_last_error())


def test_scene_slic_has_no_cpu_fallback(built):
    import torch
    from deepmerge_amd import scene
    img = torch.zeros((3, 16, 16), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.slic_labels(img, tile=8, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.slic_assign(img, tile=8, device="cpu")


def test_the_python_calls_check_their_arguments_before_any_device_work(built):
    from deepmerge_amd import scene
    img = np.zeros((3, 20, 30), np.uint8)
    for call in (scene.slic_labels, scene.slic_assign):
        for kw, msg in ((dict(cell=3), "cell must be in 4..256"), (dict(cell=257), "cell must be in 4..256"),
                        (dict(compactness=-1), "compactness must be in 0..255"), (dict(compactness=256), "compactness must be in 0..255"),
                        (dict(iters=-1), "iters must be >= 0"), (dict(resident_bytes=-1), "resident_bytes must be >= 0"),
                        (dict(tile=0), "tile must be >= 1"), (dict(tile=(4, 0)), "tile must be >= 1")):
            with pytest.raises(ValueError, match=msg):
                call(img, device="cpu", **kw)
        with pytest.raises(ValueError, match="source.shape must be"):
            call(np.zeros((20, 30), np.uint8), device="cpu")
    with pytest.raises(ValueError, match="min_size must be in"):
        scene.slic_labels(img, min_size=0, device="cpu")
    for bad in (np.zeros((20, 30), np.int64), np.zeros((20, 31), np.int32), [[0]]):
        with pytest.raises(ValueError, match="labels_out must be a writable int32"):
            scene.slic_labels(img, labels_out=bad, device="cpu")
        with pytest.raises(ValueError, match="assigned_out must be a writable int32"):
            scene.slic_assign(img, assigned_out=bad, device="cpu")
    frozen = np.zeros((20, 30), np.int32)
    frozen.flags.writeable = False
    with pytest.raises(ValueError, match="labels_out must be a writable int32"):
        scene.slic_labels(img, labels_out=frozen, device="cpu")


def test_segment_scene_refuses_what_does_not_go_with_cross_seams(built):
    from deepmerge_amd import scene
    img = np.zeros((3, 20, 30), np.uint8)
    with pytest.raises(ValueError, match="cross_seams=True makes the scene's superpixels itself"):
        scene.segment_scene(None, img, cross_seams=True, segmenter=lambda t: None)
    with pytest.raises(ValueError, match="cross_seams=True makes the scene's superpixels itself"):
        scene.segment_scene(None, img, cross_seams=True, labels=np.zeros((20, 30), np.int32), n_labels=1)
    with pytest.raises(ValueError, match="goes with cross_seams=True"):
        scene.segment_scene(None, img, slic=dict(cell=8))
