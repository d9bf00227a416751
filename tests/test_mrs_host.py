"""CPU: the multiresolution merge rule (tests/mrs_ref.py, the spec of rag.mrs) -- hand-worked costs, the planted quadrants, the
closed-form pixel start -- and the header, binding and argument validation of the two entry points, which need no GPU."""
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import merge_ref as M
import mrs_ref as R
from oracle import rag as OR


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


def two_pixels(p, q, bands=1):
    """Pixels (0,0) = p and (0,1) = q of a 1 x 2 raster as two regions with one edge."""
    tile = np.array([[[p, q]]] * bands, np.uint8)
    return R.pixel_regions_ref(tile)


# ---- hand-worked costs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q", [(10, 10), (3, 250), (200, 199)])
def test_two_single_pixels_by_hand(p, q):
    """V_m = 2 (p^2 + q^2) - (p + q)^2 = (p - q)^2, V_a = V_b = 0: hc = |p - q|.  l = 4, 4, 6 and n = 1, 1, 2: hcm = 6 sqrt(2) - 8.
    b = 4, 4, 6: hsm = 12 / 6 - 4 / 4 - 4 / 4 = 0."""
    st, e, w = two_pixels(p, q)
    assert e.tolist() == [[0, 1]] and w.tolist() == [1]
    hc, hcm = float(abs(p - q)), 6.0 * math.sqrt(2.0) - 8.0
    for shape, comp in ((0.0, 0.5), (0.1, 0.5), (0.9, 0.0), (0.9, 1.0), (0.5, 0.25)):
        hs = comp * hcm + (1.0 - comp) * 0.0
        want = np.float32((1.0 - shape) * hc + shape * hs)
        assert R.cost(st, e, w, shape, comp).view(np.uint32).tolist() == [int(want.view(np.uint32))], (shape, comp)
    assert R.cost(st, e, w, 0.0, 0.5, [2.5]).tolist() == [2.5 * abs(p - q)]


def test_negative_cost_is_clamped_to_plus_zero():
    """Two halves of a constant 2 x 2 block: hc = 0, n = 2, 2, 4, l = 6, 6, 8, b = 6, 6, 8: hcm = 16 - 12 sqrt(2) < 0 and
    hsm = 4 - 2 - 2 = 0, so f < 0 for any shape > 0 with compactness > 0: the result is +0.0, sign bit clear."""
    st = {"count": np.array([2, 2], np.int64), "sum": np.array([[14], [14]], np.int64), "sumsq": np.array([[98], [98]], np.int64),
          "bbox": np.array([[0, 0, 1, 0], [0, 1, 1, 1]], np.int32), "peri": np.array([[2, 4], [2, 4]], np.int64)}
    e, w = np.array([[0, 1]], np.int32), np.array([2], np.int32)
    assert 16.0 - 12.0 * math.sqrt(2.0) < 0
    c = R.cost(st, e, w, 0.5, 1.0)
    assert c.dtype == np.float32 and c.view(np.uint32).tolist() == [0]
    assert R.cost(st, e, w, 0.9, 0.5).view(np.uint32).tolist() == [0]
    assert R.cost(st, e, w, 0.0, 0.5).view(np.uint32).tolist() == [0]          # f = +0.0 exactly: not > 0, still +0.0


def test_large_counts_go_through_exact_integers():
    """count = 2^30: V exceeds 2^64, so neither int64 nor a double product holds it; compare with Python integers and
    correctly rounded conversions (math.sqrt of float(int))."""
    st, e, w = R.big_count_stats()
    n = int(st["count"][0])
    hc = 0.0
    for c in range(2):
        s1a, s1b, s2a, s2b = (int(st[k][r, c]) for k in ("sum", "sumsq") for r in (0, 1))
        va, vb, vm = n * s2a - s1a ** 2, n * s2b - s1b ** 2, 2 * n * (s2a + s2b) - (s1a + s1b) ** 2
        assert min(va, vb, vm) > 1 << 64
        hc = hc + 1.0 * ((math.sqrt(float(vm)) - math.sqrt(float(va))) - math.sqrt(float(vb)))
    la, lb = 40000 + 98304, 52001 + 98304
    lm = la + lb - 2 * 32768
    hcm = (float(lm) * math.sqrt(float(2 * n)) - float(la) * math.sqrt(float(n))) - float(lb) * math.sqrt(float(n))
    ba = bb = 2 * (32768 + 32768)
    bm = 2 * (65536 + 32768)
    hsm = ((float(2 * n) * float(lm)) / float(bm) - (float(n) * float(la)) / float(ba)) - (float(n) * float(lb)) / float(bb)
    hs = 0.5 * hcm + (1.0 - 0.5) * hsm
    f = (1.0 - 0.1) * hc + 0.1 * hs
    assert f > 0
    got = R.cost(st, e, w, 0.1, 0.5)
    assert got.view(np.uint32).tolist() == [int(np.float32(f).view(np.uint32))]


# ---- spec properties ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def quadrant_run(scale, shape):
    return R.mrs_ref(R.quadrant_tile(), scale, shape)


def quadrant_map(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy >= H // 2) * 2 + (xx >= W // 2)


def same_partition(a, b):
    pairs = np.unique(np.stack((a.reshape(-1), b.reshape(-1)), 1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))


def test_pixel_start_recovers_the_planted_quadrants():
    r = quadrant_run(10, 0.1)
    assert r["rounds"] == 23 and r["regions_per_round"][:4] == [960, 720, 572, 464] and r["regions_per_round"][-1] == 4
    assert r["clamped"] == 0
    assert same_partition(r["region_of"].reshape(24, 40), quadrant_map(24, 40))
    r = quadrant_run(5, 0.1)
    assert r["rounds"] == 17 and r["regions_per_round"][-1] == 62
    r = quadrant_run(10, 0.9)
    assert r["regions_per_round"][-1] == 4 and same_partition(r["region_of"].reshape(24, 40), quadrant_map(24, 40))
    assert r["clamped"] == 39                                      # the clamp and its tie-break by id are exercised


def test_label_start_on_jittered_superpixels():
    lab, gy, gx = M.superpixels(48, 64, 6, 1)
    assert gy * gx == 88 and len(np.unique(lab)) == 88
    tile = R.quadrant_tile(48, 64)
    r = R.mrs_ref(tile, 60, 0.1, labels=lab, n_labels=88)
    assert r["regions_per_round"][0] == 88 and r["regions_per_round"][-1] == 6 and r["rounds"] == 12
    r = R.mrs_ref(tile, 150, 0.5, labels=lab, n_labels=88)
    assert r["regions_per_round"][-1] == 3 and r["clamped"] > 0


def test_every_round_is_a_matching_and_the_history_is_consistent():
    for r in (quadrant_run(10, 0.1), quadrant_run(5, 0.1), quadrant_run(10, 0.9)):
        assert all(M.is_matching(m) for m in r["matchings"]) and len(r["matchings"]) == r["rounds"]
        assert sum(r["merges_per_round"]) == len(r["history"]) == 960 - r["regions_per_round"][-1]
        assert np.array_equal(M.region_of_at(r["history"], r["merges_per_round"], 960, r["rounds"]), r["region_of"])
        assert r["pooled"].shape == (r["regions_per_round"][-1], 0) and not r["ptr"].any() and r["idx"].size == 0
        assert (r["history_simi"] < np.float32(100)).all() and (r["simi"] >= 0).all()


def test_stops_at_max_rounds_and_before_min_regions():
    tile = R.quadrant_tile()
    full = quadrant_run(10, 0.1)
    r = R.mrs_ref(tile, 10, 0.1, max_rounds=3)
    assert r["rounds"] == 3 and r["regions_per_round"] == full["regions_per_round"][:4]
    r = R.mrs_ref(tile, 10, 0.1, min_regions=10)
    assert r["regions_per_round"] == [c for c in full["regions_per_round"] if c >= 10]


@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (5, 1), (3, 4), (7, 9)])
@pytest.mark.parametrize("bands", [1, 3, 4])
def test_pixel_regions_ref_equals_the_oracle_on_arange(H, W, bands):
    tile = np.random.default_rng(H * 100 + W + bands).integers(0, 256, (bands, H, W), dtype=np.uint8)
    st, e, w = R.pixel_regions_ref(tile)
    lab = np.arange(H * W, dtype=np.int32).reshape(H, W)
    oe, ow = OR.rag_edges(lab, H * W)
    ost = OR.label_stats(lab, tile, H * W)
    assert e.shape == (H * (W - 1) + (H - 1) * W, 2) and np.array_equal(e, oe.reshape(-1, 2)) and np.array_equal(w, ow)
    for k in M.STAT_KEYS:
        assert st[k].dtype == ost[k].dtype and np.array_equal(st[k], ost[k]), k


def test_cost_is_symmetric_in_the_two_regions():
    lab, gy, gx = M.superpixels(48, 64, 6, 1)
    tile = R.quadrant_tile(48, 64)
    st = OR.label_stats(lab, tile, 88)
    e, w = OR.rag_edges(lab, 88)
    perm = np.arange(88)[::-1].copy()                              # region r becomes 87 - r: every edge (a, b) becomes (87 - b, 87 - a)
    st2 = {k: st[k][perm] for k in M.STAT_KEYS}
    e2 = np.stack((87 - e[:, 1], 87 - e[:, 0]), 1).astype(np.int32)
    for shape, comp, bw in ((0.1, 0.5, None), (0.9, 0.0, [0.5, 2.0, 1.25])):
        c1, c2 = R.cost(st, e, w, shape, comp, bw), R.cost(st2, e2, w, shape, comp, bw)
        assert np.array_equal(c1.view(np.uint32), c2.view(np.uint32))


# ---- the library's side, without a GPU ----------------------------------------------------------------------------------------------
def test_header_binding_and_exports_carry_the_two_entries(built):
    text = re.sub(r"/\*.*?\*/", "", open(built.HEADER_PATH).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True).stdout
    for name, n_args in (("dm_region_merge_cost", 17), ("dm_pixel_regions", 12)):
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(built.SIGNATURES[name][1]), name
        assert re.search(r" T %s\b" % name, nm), name
    assert built.lib().dm_abi_version() == 7


def test_entry_points_refuse_bad_arguments_before_any_launch(built):
    lib = built.lib()
    p = 4096                                                       # any non-null address: validation never dereferences
    ok = dict(count=p, sum=p, sumsq=p, bbox=p, peri=p, edges=p, weights=p, E=4, C=4, bands=3, bw0=1.0, bw1=1.0, bw2=1.0, shape=0.1,
              compactness=0.5, cost=p)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(**{k: None}), b"null pointer") for k in ("count", "sum", "sumsq", "bbox", "peri", "edges", "weights", "cost")]
    cases += [(dict(E=0), b"bad sizes"), (dict(C=0), b"bad sizes"), (dict(C=(1 << 24) + 1), b"bad sizes"), (dict(bands=0), b"bands"),
              (dict(bands=4), b"bands"), (dict(shape=1.0), b"shape"), (dict(shape=-0.1), b"shape"), (dict(shape=nan), b"shape"),
              (dict(compactness=1.5), b"compactness"), (dict(compactness=nan), b"compactness"), (dict(bw0=-1.0), b"band weights"),
              (dict(bw1=inf), b"band weights"), (dict(bw2=nan), b"band weights")]
    for change, msg in cases:
        a = {**ok, **change}
        assert lib.dm_region_merge_cost(*a.values(), None) == -1, change
        assert b"dm_region_merge_cost" in lib.dm_last_error() and msg in lib.dm_last_error(), (change, lib.dm_last_error())
    ok = dict(tile=p, bands=3, H=8, W=8, count=p, sum=p, sumsq=p, bbox=p, peri=p, edges=p, weights=p)
    cases = [(dict(**{k: None}), b"null pointer") for k in ("tile", "count", "sum", "sumsq", "bbox", "peri")]
    cases += [(dict(edges=None), b"null edges"), (dict(weights=None), b"null edges"), (dict(H=0), b"bad sizes"), (dict(W=-3), b"bad sizes"),
              (dict(bands=0), b"bad sizes"), (dict(H=4100, W=4100), b"bad sizes"), (dict(H=1 << 24, W=2), b"bad sizes")]
    for change, msg in cases:
        a = {**ok, **change}
        assert lib.dm_pixel_regions(*a.values(), None) == -1, change
        assert b"dm_pixel_regions" in lib.dm_last_error() and msg in lib.dm_last_error(), (change, lib.dm_last_error())


def test_mrs_validates_in_python_and_has_no_cpu_fallback(built):
    import torch
    from deepmerge_amd import rag
    tile = torch.from_numpy(R.quadrant_tile())
    for call in (lambda: rag.mrs(tile, 10.0), lambda: rag.pixel_regions(tile), lambda: rag.mrs_segment(tile, 10.0)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="shape"):
        rag._mrs_params(3, 1.0, 0.5, None)
    with pytest.raises(ValueError, match="compactness"):
        rag._mrs_params(3, 0.1, 1.5, None)
    with pytest.raises(ValueError, match="band_weights"):
        rag._mrs_params(3, 0.1, 0.5, [1.0, 1.0])
    with pytest.raises(ValueError, match="band_weights"):
        rag._mrs_params(3, 0.1, 0.5, [1.0, -1.0, 1.0])
    assert rag._mrs_params(2, 0.0, 1.0, [0.0, 2.0]) == (0.0, 1.0, [0.0, 2.0, 1.0])
