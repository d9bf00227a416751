"""CPU: the numpy spec of the feed's dihedral augmentation (tests/augment_ref.py) has the properties DESIGN.md 3.8 / 3.9 state -- the
eight transforms form the group D4, orientation 0 is the plain pyramid, the orientation draw is a keyed function of (seed, epoch,
pair) -- and the two new entry points are declared, bound, exported and refuse bad arguments before any launch."""
import ctypes
import itertools

import numpy as np
import pytest

import augment_ref as A
import train_smt_ref as R
from oracle import patches as OP


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


# ---- the transform ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 5])
def test_the_eight_transforms_are_distinct_and_closed_under_composition(L):
    crop = np.arange(L * L, dtype=np.uint8).reshape(1, L, L)                      # asymmetric: every pixel its own value
    views = [A.orient_crop(crop, o) for o in range(8)]
    for a, b in itertools.combinations(range(8), 2):
        assert not np.array_equal(views[a], views[b]), (a, b)
    table = np.empty((8, 8), np.int64)
    for a, b in itertools.product(range(8), range(8)):
        hit = [c for c in range(8) if np.array_equal(A.orient_crop(views[a], b), views[c])]
        assert len(hit) == 1, (a, b)
        table[a, b] = hit[0]
    for a in range(8):                                                            # a group: identity, every row and column a permutation
        assert table[0, a] == a == table[a, 0]
        assert sorted(table[a]) == list(range(8)) == sorted(table[:, a])
    assert (table[4, 4], table[1, 1], table[2, 2], table[3, 3]) == (0, 0, 0, 0)   # the flips and the transposition are involutions
    assert table[5, 5] != 0 and table[table[5, 5], table[5, 5]] == 0              # a quarter turn has order 4
    assert {o for o in range(8) if np.array_equal(A.orient_crop(views[o], o), crop)} == {0, 1, 2, 3, 4, 7}
    with pytest.raises(ValueError):
        A.orient_crop(crop, 8)


@pytest.mark.parametrize("L", [1, 2, 6, 7])
def test_index_map_equals_slicing_form(L):
    rng = np.random.default_rng(L)
    crop = rng.integers(0, 256, (3, L, L), dtype=np.uint8)
    for o in range(8):
        assert np.array_equal(A.orient_crop_indexed(crop, o), A.orient_crop(crop, o)), o
    for o in range(8):                                                            # the map written out element by element
        fy = (lambda v: L - 1 - v) if o & 2 else (lambda v: v)
        fx = (lambda v: L - 1 - v) if o & 1 else (lambda v: v)
        want = np.empty_like(crop)
        for j in range(L):
            for i in range(L):
                a, b = (i, j) if o & 4 else (j, i)
                want[:, j, i] = crop[:, fy(a), fx(b)]
        assert np.array_equal(A.orient_crop(crop, o), want), o


@pytest.mark.parametrize("resize", ["opencv", "exact_area"])
def test_orientation_zero_is_the_plain_pyramid(resize):
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (3, 40, 50), dtype=np.uint8)
    for (x, y), L, t in (((0, 0), 9, 8), ((49, 39), 16, 8), ((20, 17), 24, 8), ((25, 20), 5, 8), ((-30, -30), 7, 8)):
        want = OP.patch_pyramid(img, x, y, [L], [t], resize=resize)[0]
        got = A.oriented_patch(img, x, y, L, t, 0, resize)
        assert got.dtype == want.dtype and np.array_equal(got, want)
    # and a transposed scene seen transposed is the scene itself: orientation 4 on img.T (sample point mirrored) == orientation 0
    L, t = 16, 8
    assert np.array_equal(A.oriented_patch(np.ascontiguousarray(img.transpose(0, 2, 1)), 17, 20, L, t, 4, resize),
                          A.oriented_patch(img, 20, 17, L, t, 0, resize))


def test_patch_rows_is_the_im2col_order():
    p = np.arange(2 * 8 * 8, dtype=np.float32).reshape(2, 8, 8)
    rows = A.patch_rows(p, 4)
    assert rows.shape == (16, 8)
    py, px, c, dy, dx = 2, 3, 1, 1, 0
    assert rows[py * 4 + px, (c * 2 + dy) * 2 + dx] == p[c, py * 2 + dy, px * 2 + dx]


# ---- the draw -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [3, 7])
@pytest.mark.parametrize("N,batch", [(1, 1), (5, 2), (37, 7), (37, 37), (1000, 32)])
def test_draw_is_equal_on_both_rows_of_a_pair_and_within_the_mask(N, batch, mask):
    o = A.epoch_orient(N, 5, 1, batch, mask)
    assert o.dtype == np.int32 and o.shape == (2 * N,)
    rl, rr = R.blocked_rows(N, batch)
    assert np.array_equal(o[rl], o[rr]) and o.min() >= 0 and o.max() <= mask
    assert np.array_equal(np.sort(np.concatenate((rl, rr))), np.arange(2 * N))
    # keyed by the pair, not by the position or the batch size: position j carries the value of pair perm(j)
    src = R.epoch_perm(N, 5, 1)
    per_pair = np.empty(N, np.int32)
    per_pair[src] = o[rl]
    other = A.epoch_orient(N, 5, 1, 1, mask)
    assert np.array_equal(per_pair[src], other[R.blocked_rows(N, 1)[0]])


def test_draw_covers_all_eight_and_depends_on_epoch_seed_and_mask():
    N = 8000
    base = A.epoch_orient(N, 0, 0, 32, 7)
    counts = np.bincount(base[R.blocked_rows(N, 32)[0]], minlength=8)
    assert counts.shape == (8,) and counts.min() > 0
    assert np.abs(counts - N / 8).max() < 5 * np.sqrt(N * (1 / 8) * (7 / 8))       # 1000 +- 5 sigma (sigma = 29.6)
    assert np.array_equal(base, A.epoch_orient(N, 0, 0, 32, 7))                    # a repeated call: the same table
    assert not np.array_equal(base, A.epoch_orient(N, 0, 1, 32, 7))
    assert not np.array_equal(base, A.epoch_orient(N, 1, 0, 32, 7))
    assert not np.array_equal(base, A.epoch_orient(N, 1 << 32, 0, 32, 7))          # the high key word counts
    flips = A.epoch_orient(N, 0, 0, 32, 3)
    assert not np.array_equal(base, flips) and np.array_equal(base & 3, flips) and set(np.unique(flips)) == {0, 1, 2, 3}
    # word 3 is a stream of its own: not the draw's (1), not the shuffle's (2)
    src = R.epoch_perm(N, 0, 0).astype(np.uint32)
    for word in (1, 2):
        assert not np.array_equal(R.philox4x32_10((src, 0, word, 0), R.seed_key(0))[0] & np.uint32(7), base[R.blocked_rows(N, 32)[0]])
    with pytest.raises(ValueError):
        A.epoch_orient(N, 0, 0, 32, 5)


# ---- the library's side, without a GPU ----------------------------------------------------------------------------------------------
NEW = ("dm_pair_batch_gather_oriented", "dm_pair_epoch_orient")


def test_new_symbols_are_declared_bound_and_exported_and_the_abi_is_still_7(built):
    lib = built.lib()
    assert lib.dm_abi_version() == 7
    declared = built.declared_symbols()
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW:
        assert name in declared and name in built.SIGNATURES and hasattr(raw, name), name
    assert sorted(built.SIGNATURES) == declared
    text = open(built.HEADER_PATH).read()
    for name, nargs in zip(NEW, (22, 7)):
        proto = text[text.index("int " + name + "("):]
        proto = proto[:proto.index(";")]
        assert proto.count(",") + 1 == nargs == len(built.SIGNATURES[name][1]), name
    assert len(built.SIGNATURES["dm_pair_batch_gather"][1]) == 21                  # the existing entry keeps its signature
    assert ctypes.sizeof(built.DmPairDraw) == 16 * 8 + 8 + 6 * 4                   # 16 pointers, the seed, 6 int32: unchanged
    from deepmerge_amd import ops
    assert ops.ORIENT_MASKS == A.MASKS


def test_entry_points_refuse_bad_arguments_before_any_launch(built):
    lib = built.lib()
    p = 4096                                                                       # any non-null address: validation never dereferences
    F32, BF16 = built.DM_F32, built.DM_BF16

    def gather(*, tiles=p, n_tiles=2, bands=3, H=64, W=64, xy=p, inner=p, obj=p, orient=p, scale_index=0, max_window=64, P=8, target=32,
               grid=0, rule=0, out=p, dtype=F32, region=None, designed=None):
        return lib.dm_pair_batch_gather_oriented(tiles, n_tiles, bands, H, W, p, xy, inner, obj, orient, scale_index, max_window, P, target,
                                                 grid, rule, out, dtype, region, designed, None, None)

    def orient(*, seed=1, epoch=0, n=10, batch=4, mask=7, out=p):
        return lib.dm_pair_epoch_orient(seed, epoch, n, batch, mask, out, None)

    name = b"dm_pair_batch_gather_oriented: "
    cases = [
        (lambda: gather(orient=None), -1, name + b"null orient"),
        (lambda: gather(rule=2), -6, name + b"unknown resize rule"),
        (lambda: gather(tiles=None), -1, name + b"bad arguments"),
        (lambda: gather(xy=None), -1, name + b"bad arguments"),
        (lambda: gather(inner=None), -1, name + b"bad arguments"),
        (lambda: gather(obj=None), -1, name + b"bad arguments"),
        (lambda: gather(out=None), -1, name + b"bad arguments"),
        (lambda: gather(n_tiles=0), -1, name + b"bad arguments"),
        (lambda: gather(bands=0), -1, name + b"bad arguments"),
        (lambda: gather(H=0), -1, name + b"bad arguments"),
        (lambda: gather(P=0), -1, name + b"bad arguments"),
        (lambda: gather(target=0), -1, name + b"bad arguments"),
        (lambda: gather(scale_index=4), -1, name + b"scale index"),
        (lambda: gather(scale_index=-1), -1, name + b"scale index"),
        (lambda: gather(grid=5), -1, name + b"target 32 is not a multiple"),
        (lambda: gather(grid=-1), -1, name + b"target 32 is not a multiple"),
        (lambda: gather(max_window=0), -6, name + b"window bound"),
        (lambda: gather(max_window=385), -6, name + b"window bound"),
        (lambda: gather(bands=65536), -1, name + b"too many bands"),
        (lambda: gather(region=p), -1, name + b"designed rows need"),
        (lambda: gather(designed=p), -1, name + b"designed rows need"),
        (lambda: gather(dtype=BF16), -2, name + b"planar patches are fp32"),
        (lambda: gather(grid=8, dtype=3), -2, name + b"bad dtype"),
        (lambda: orient(mask=0), -1, b"dm_pair_epoch_orient: mask 0"),
        (lambda: orient(mask=5), -1, b"dm_pair_epoch_orient: mask 5"),
        (lambda: orient(mask=15), -1, b"dm_pair_epoch_orient: mask 15"),
        (lambda: orient(n=0), -1, b"dm_pair_epoch_orient: 0 pairs"),
        (lambda: orient(n=(1 << 30) + 1), -1, b"dm_pair_epoch_orient: 1073741825 pairs"),
        (lambda: orient(batch=0), -1, b"dm_pair_epoch_orient: batch 0 < 1"),
        (lambda: orient(epoch=-1), -1, b"dm_pair_epoch_orient: epoch -1 < 0"),
        (lambda: orient(out=None), -1, b"dm_pair_epoch_orient: bad arguments (null output)"),
    ]
    for call, status, message in cases:
        assert call() == status, message
        assert message in lib.dm_last_error(), (message, lib.dm_last_error())
    # the existing entry reports under its own name, as before
    assert lib.dm_pair_batch_gather(p, 2, 3, 64, 64, p, p, p, p, 4, 64, 8, 32, 0, 0, p, F32, None, None, None, None) == -1
    assert b"dm_pair_batch_gather: scale index 4 outside 0..3" in lib.dm_last_error()


def _host_images():
    rng = np.random.default_rng(0)
    n = 8
    return [{"tile": rng.integers(0, 256, (3, 60, 70), dtype=np.uint8), "xy": np.stack((rng.integers(0, 70, n), rng.integers(0, 60, n)), 1),
             "inner": np.full(n, 10), "obj": np.full(n, 16), "region": rng.random((n, 15), dtype=np.float32),
             "polygon_points": [[k, k + 4] for k in range(4)], "positive": np.array([[0, 1], [2, 3]]), "negative": np.array([[0, 3]])}]


def test_python_layers_refuse_bad_arguments_without_a_gpu():
    import torch
    from deepmerge_amd import Train_SMT, ops
    from deepmerge_amd.dataset import PairDataset
    from deepmerge_amd.feed import PairTable
    ds = PairDataset.from_arrays(_host_images(), seed=1, device="cpu")            # host tensors: enough for the argument checks
    for bad in ("x", "D4", "", 7):
        with pytest.raises(ValueError, match="augment"):
            ds.epoch(0, 2, augment=bad)
        with pytest.raises(ValueError, match="augment"):
            Train_SMT.train(None, 1.0, 2, 1e-3, 0.0, 0.0, 0.1, 0, dataset=ds, augment=bad)
    with pytest.raises(ValueError, match="batch"):
        ds.epoch(0, 0, augment="d4")
    # PairTable: `orient` is the last field and optional; stack joins it only when both sides carry one
    B = 3
    i32 = lambda v: torch.full((B,), v, dtype=torch.int32)
    mk = lambda o: PairTable(i32(0), torch.zeros((B, 2), dtype=torch.int32), i32(10), i32(16), torch.zeros((B, 15)), torch.ones(B), o)
    assert [f for f in PairTable.__dataclass_fields__][-1] == "orient" and mk(None).orient is None
    both = PairTable.stack(mk(i32(5)), mk(i32(5)))
    assert both.orient.dtype == torch.int32 and both.orient.tolist() == [5] * (2 * B) and both.xy.shape == (2 * B, 2)
    assert PairTable.stack(mk(i32(5)), mk(None)).orient is None and PairTable.stack(mk(None), mk(None)).orient is None
    with pytest.raises((ValueError, RuntimeError)):                               # host tensors are refused, whatever orient says
        ops.pair_epoch_orient(0, 0, 3, 2, 7, torch.zeros(6, dtype=torch.int32))
