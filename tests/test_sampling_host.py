"""CPU: the weighted-sampling spec (tests/sampling_ref.py) against Python integers, dataset.balance_weights / hardness_weights, and
what the new entry points and Python layers refuse without a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import sampling_ref as S
import train_smt_ref as R

ZERO_PATTERNS = {"zeros first": [0, 0, 0, 5, 1, 2], "zeros last": [3, 1, 4, 0, 0], "a run in the middle": [2, 0, 0, 0, 0, 7, 1],
                 "a single non-zero": [0, 0, 0, 9, 0, 0], "alternating": [0, 1, 0, 1, 0, 1, 0]}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


# ---- the spec against itself --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [1, 2, 3, 255, (1 << 32) - 1, 1 << 32, (1 << 62) - 1])
def test_u_is_below_the_total(total):
    for seed, epoch in ((0, 0), (0x9E3779B97F4A7C15, 2 ** 31 - 1)):
        u = S.select_u(total, 2000, seed, epoch).tolist()
        assert all(0 <= x < total for x in u)
        r = R.philox4x32_10((np.arange(2000, dtype=np.uint32), epoch, 5, 0), R.seed_key(seed))
        assert u == [((int(a) << 32 | int(b)) * total) >> 64 for a, b in zip(r[0].tolist(), r[1].tolist())]       # Python integers
        if total > 1000:
            assert len(set(u)) > 1900                                # spread over the range, not stuck


@pytest.mark.parametrize("name", sorted(ZERO_PATTERNS))
def test_select_never_names_a_zero_weight_pair(name):
    w = np.asarray(ZERO_PATTERNS[name], np.int64)
    for seed in (0, 7, 1 << 40):
        for epoch in (0, 1, 2 ** 31 - 1):
            src = S.select(w, 3 * len(w) + 1, seed, epoch)
            assert src.dtype == np.int32 and src.min() >= 0 and src.max() < len(w)
            assert (w[src] > 0).all(), (name, seed, epoch)
    src = S.select(w, 4000, 3, 0)
    assert set(src.tolist()) == set(np.nonzero(w)[0].tolist())        # and every pair with weight is reachable


def test_select_is_the_count_of_prefix_sums_not_above_u():
    """The definition, in Python integers, against the vectorised search."""
    rng = np.random.default_rng(1)
    w = rng.integers(0, 50, 300)
    cum = S.cumsum(w)
    u = S.select_u(cum[-1], 500, 11, 4).tolist()
    assert S.select(w, 500, 11, 4).tolist() == [sum(c <= x for c in cum) for x in u]


@pytest.mark.parametrize("N", [1, 2, 7, 256, 1000])
def test_equal_weights_select_uniformly(N):
    """Equal weights k: src = floor(u / k) = floor(R N / 2^64), the plain uniform draw on [0, N)."""
    r = R.philox4x32_10((np.arange(5000, dtype=np.uint32), 3, 5, 0), R.seed_key(9))
    want = [((int(a) << 32 | int(b)) * N) >> 64 for a, b in zip(r[0].tolist(), r[1].tolist())]
    for k in (1, 1 << 20):                                            # N k a power of two times N: the floor commutes
        assert S.select(np.full(N, k, np.int64), 5000, 9, 3).tolist() == want
    if N >= 7:
        counts = np.bincount(want, minlength=N)
        assert counts.min() > 0 if N <= 256 else counts.max() < 25    # 5000 / N expected per cell


def test_total_just_below_2_62_uses_the_full_128_bit_product():
    w = [(1 << 61) - 1, (1 << 61) - 1]
    T = (1 << 62) - 2
    r = R.philox4x32_10((np.arange(4000, dtype=np.uint32), 0, 5, 0), R.seed_key(5))
    u = [((int(a) << 32 | int(b)) * T) >> 64 for a, b in zip(r[0].tolist(), r[1].tolist())]
    assert S.select_u(T, 4000, 5, 0).tolist() == u and max(u) < T and max(u) > 1 << 61
    src = S.select(w, 4000, 5, 0)
    assert src.tolist() == [int(x >= w[0]) for x in u] and 1800 < int(src.sum()) < 2200
    with pytest.raises(ValueError):
        S.cumsum([1 << 61, 1 << 61])                                  # 2^62 itself is refused
    with pytest.raises(ValueError):
        S.cumsum([0, 0])
    with pytest.raises(ValueError):
        S.cumsum([3, -1])


def test_streams_are_keyed_by_the_position_on_words_of_their_own():
    """Two positions that hold the same pair get different point draws, orientations and tables; no word of the sampled epoch is
    one the unsampled epoch uses."""
    assert len({1, 2, 3, 4, S.WORD_SELECT, S.WORD_DRAW, S.WORD_ORIENT, S.WORD_RADIO}) == 8
    assert (S.WORD_DRAW, S.WORD_ORIENT, S.WORD_RADIO) == (1 + 16, 3 + 16, 4 + 16)
    o = S.epoch_orient(64, 3, 0, 64, 7)[:64]
    assert len(set(o.tolist())) == 8
    t = S.position_radio(64, 3, 0, 3, 51, 13, 6528)
    assert len({tuple(row.reshape(-1).tolist()) for row in t}) == 64


# ---- balance_weights ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pos,n_neg,share", [(9, 1, 0.5), (3600, 400, 0.5), (7, 13, 0.25), (1, 1, 0.5), (5, 5, 1 / 65536), (11, 3, 65535 / 65536),
                                               (1000, 10, 0.3)])
def test_balance_weights_give_the_exact_share(n_pos, n_neg, share):
    from deepmerge_amd.dataset import balance_class_weights, balance_weights
    P = int(round(65536 * share))
    w_pos, w_neg = balance_class_weights(n_pos, n_neg, share)
    assert (w_pos, w_neg) == S.balance_class_weights(n_pos, n_neg, share) and math.gcd(w_pos, w_neg) == 1
    assert (n_pos * w_pos) * 65536 == P * (n_pos * w_pos + n_neg * w_neg)         # the share, exactly
    flag = np.concatenate((np.ones(n_pos, np.int32), np.zeros(n_neg, np.int32)))
    np.random.default_rng(0).shuffle(flag)
    for f in (flag, torch.from_numpy(flag)):
        w = balance_weights(f, share)
        assert w.dtype == torch.int64 and w.tolist() == [w_pos if v else w_neg for v in flag.tolist()]


def test_balance_weights_gcd_reduction():
    from deepmerge_amd.dataset import balance_class_weights
    assert balance_class_weights(3600, 400, 0.5) == (1, 9)            # 32768 * 400 : 32768 * 3600
    assert balance_class_weights(6, 4, 0.5) == (2, 3)
    assert balance_class_weights(10, 10, 0.25) == (1, 3)


def test_balance_weights_refusals():
    from deepmerge_amd.dataset import balance_class_weights, balance_weights
    for share in (0.0, 1.0, -0.1, 1.5, 1e-6, 1 - 1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="positive_share"):
            balance_class_weights(5, 5, share)
    for n_pos, n_neg in ((0, 5), (5, 0), (0, 0)):
        with pytest.raises(ValueError, match="both classes"):
            balance_class_weights(n_pos, n_neg, 0.5)
    with pytest.raises(ValueError, match="both classes"):
        balance_weights(np.ones(6, np.int32), 0.5)
    # 2 n_pos n_neg w / gcd: two coprime classes of ~2^29 pairs at an odd P overflow, the largest equal classes do not
    a, b = (1 << 29) + 1, (1 << 29) - 1
    with pytest.raises(ValueError, match="2\\^62"):
        balance_class_weights(a, b, 3 / 65536)
    assert balance_class_weights(1 << 29, 1 << 29, 0.5) == (1, 1)


def test_balanced_spec_draw_is_half_positive_within_five_sigma():
    """N = 4000 with 90 % positives, balance 0.5, M = N, one fixed seed: the positives drawn lie within 5 sqrt(M / 4) = 158 of M / 2."""
    from deepmerge_amd.dataset import balance_weights
    N = 4000
    flag = np.concatenate((np.ones(3600, np.int32), np.zeros(400, np.int32)))
    w = balance_weights(flag, 0.5).numpy()
    src = S.select(w, N, 2024, 0)
    n_pos = int(flag[src].sum())
    print("positives drawn:", n_pos)
    assert abs(n_pos - N // 2) <= 158
    assert abs(int(flag[S.select(np.ones(N, np.int64), N, 2024, 0)].sum()) - 3600) <= 5 * math.sqrt(N * 0.9 * 0.1)    # unweighted: the list's ratio


# ---- hardness_weights -------------------------------------------------------------------------------------------------------------------
def test_hardness_weights_ends_and_product():
    from deepmerge_amd.dataset import hardness_weights
    cap = 0.75
    term = torch.tensor([0.0, -0.0, cap, np.nextafter(np.float32(cap), np.float32(0)), 2 * cap, float("inf"), float("nan"), -1.0, float("-inf"),
                         cap / 255, cap / 2, 1e-30], dtype=torch.float32)
    h = hardness_weights(term, floor_share=1 / 256, cap=cap)
    assert h.dtype == torch.int64 and h.tolist() == S.hardness(term.numpy(), 1 / 256, cap).tolist()
    assert h.tolist()[:3] == [1, 1, 256] and h.tolist()[4:9] == [256, 256, 1, 1, 1] and h[10] == 128 and h[11] == 1
    assert hardness_weights(term, floor_share=1 / 16, cap=cap).tolist() == [max(16, v) for v in h.tolist()]
    assert hardness_weights(term, floor_share=1.0, cap=cap).tolist() == [256] * len(term)
    rng = np.random.default_rng(3)
    t = torch.from_numpy((rng.random(5000) * 1.5).astype(np.float32))
    for c in (1.0, 0.3, 7.0):
        assert hardness_weights(t, 1 / 256, c).tolist() == S.hardness(t.numpy(), 1 / 256, c).tolist()
    cw = torch.tensor([3, 5] * 6, dtype=torch.int64)
    assert hardness_weights(term, 1 / 256, cap, class_weights=cw).tolist() == (cw * h).tolist()
    with pytest.raises(ValueError, match="2\\^62"):                   # bounded at h = 256, whatever the terms say
        hardness_weights(torch.zeros(2), class_weights=torch.tensor([1 << 53, 1 << 53], dtype=torch.int64))
    hardness_weights(torch.zeros(2), class_weights=torch.tensor([(1 << 53) - 1, 1 << 53], dtype=torch.int64))
    for kw in ({"cap": 0.0}, {"cap": -1.0}, {"cap": float("nan")}, {"cap": float("inf")}, {"floor_share": 0.0}, {"floor_share": 1.5}):
        with pytest.raises(ValueError):
            hardness_weights(term, **kw)
    with pytest.raises(ValueError, match="float32"):
        hardness_weights(term.double())


# ---- the library and the Python layers, without a GPU -------------------------------------------------------------------------------------
NEW = {"dm_pair_epoch_select": 7, "dm_pair_epoch_draw_src": 4, "dm_pair_epoch_orient_src": 7, "dm_pair_epoch_radiometric_src": 10}


def test_new_symbols_are_declared_bound_and_exported_and_the_abi_is_still_7(built):
    lib = built.lib()
    assert lib.dm_abi_version() == 7
    declared = built.declared_symbols()
    raw = ctypes.CDLL(built.LIB_PATH)
    text = open(built.HEADER_PATH).read()
    for name, nargs in NEW.items():
        assert name in declared and name in built.SIGNATURES and hasattr(raw, name), name
        proto = text[text.index("int " + name + "("):]
        proto = proto[:proto.index(";")]
        assert proto.count(",") + 1 == nargs == len(built.SIGNATURES[name][1]), name
    assert sorted(built.SIGNATURES) == declared
    assert built.SIGNATURES["dm_pair_epoch_orient_src"] == built.SIGNATURES["dm_pair_epoch_orient"]
    assert built.SIGNATURES["dm_pair_epoch_radiometric_src"] == built.SIGNATURES["dm_pair_epoch_radiometric"]
    assert ctypes.sizeof(built.DmPairDraw) == 16 * 8 + 8 + 6 * 4                   # DmPairDraw is unchanged


def test_entry_points_refuse_bad_arguments_before_any_launch(built):
    lib = built.lib()
    p = 4096                                                                       # any non-null address: validation never dereferences

    def select(*, cum=p, n=10, m=10, seed=1, epoch=0, src=p):
        return lib.dm_pair_epoch_select(cum, n, m, seed, epoch, src, None)

    def draw(*, src=p, m=10, null=None, **over):
        a = built.DmPairDraw()
        for f, _ in built.DmPairDraw._fields_:
            if f not in ("seed", "n_pairs", "n_poly", "n_poly_pts", "n_pts", "epoch", "batch"):
                setattr(a, f, None if f == null else p)
        a.seed, a.n_pairs, a.n_poly, a.n_poly_pts, a.n_pts, a.epoch, a.batch = 1, 10, 4, 8, 8, 0, 4
        for k, v in over.items():
            setattr(a, k, v)
        return lib.dm_pair_epoch_draw_src(ctypes.byref(a), src, m, None)

    def orient(*, seed=1, epoch=0, n=10, batch=4, mask=7, out=p):
        return lib.dm_pair_epoch_orient_src(seed, epoch, n, batch, mask, out, None)

    def radio(*, seed=1, epoch=0, n=10, batch=4, bands=3, spans=(51, 13, 6528), out=p):
        return lib.dm_pair_epoch_radiometric_src(seed, epoch, n, batch, bands, *spans, out, None)

    big = (1 << 30) + 1
    cases = [
        (lambda: select(cum=None), b"dm_pair_epoch_select: bad arguments (null pointer)"),
        (lambda: select(src=None), b"dm_pair_epoch_select: bad arguments (null pointer)"),
        (lambda: select(n=0), b"dm_pair_epoch_select: 0 pairs"),
        (lambda: select(n=big), b"dm_pair_epoch_select: 1073741825 pairs"),
        (lambda: select(m=0), b"dm_pair_epoch_select: 0 draws"),
        (lambda: select(m=big), b"dm_pair_epoch_select: 1073741825 draws"),
        (lambda: select(epoch=-1), b"dm_pair_epoch_select: epoch -1 < 0"),
        (lambda: lib.dm_pair_epoch_draw_src(None, p, 10, None), b"dm_pair_epoch_draw_src: null arguments"),
        (lambda: draw(src=None), b"dm_pair_epoch_draw_src: bad arguments (null src)"),
        (lambda: draw(m=0), b"dm_pair_epoch_draw_src: 0 draws"),
        (lambda: draw(m=big), b"dm_pair_epoch_draw_src: 1073741825 draws"),
        (lambda: draw(n_pairs=0), b"dm_pair_epoch_draw_src: 0 pairs"),
        (lambda: draw(batch=0), b"dm_pair_epoch_draw_src: batch 0 < 1"),
        (lambda: draw(epoch=-1), b"dm_pair_epoch_draw_src: epoch -1 < 0"),
        (lambda: draw(n_pts=0), b"dm_pair_epoch_draw_src: empty polygon table"),
        (lambda: draw(null="pairs"), b"dm_pair_epoch_draw_src: bad arguments (null input)"),
        (lambda: draw(null="pt_region"), b"dm_pair_epoch_draw_src: bad arguments (null input)"),
        (lambda: draw(null="flag"), b"dm_pair_epoch_draw_src: bad arguments (null output)"),
        (lambda: orient(mask=5), b"dm_pair_epoch_orient_src: mask 5"),
        (lambda: orient(n=0), b"dm_pair_epoch_orient_src: 0 pairs"),
        (lambda: orient(n=big), b"dm_pair_epoch_orient_src: 1073741825 pairs"),
        (lambda: orient(batch=0), b"dm_pair_epoch_orient_src: batch 0 < 1"),
        (lambda: orient(epoch=-1), b"dm_pair_epoch_orient_src: epoch -1 < 0"),
        (lambda: orient(out=None), b"dm_pair_epoch_orient_src: bad arguments (null output)"),
        (lambda: radio(spans=(129, 0, 0)), b"dm_pair_epoch_radiometric_src: gain span 129"),
        (lambda: radio(spans=(0, 65, 0)), b"dm_pair_epoch_radiometric_src: band span 65"),
        (lambda: radio(spans=(0, 0, 16321)), b"dm_pair_epoch_radiometric_src: offset span 16321"),
        (lambda: radio(bands=17), b"dm_pair_epoch_radiometric_src: 17 bands"),
        (lambda: radio(n=0), b"dm_pair_epoch_radiometric_src: 0 pairs"),
        (lambda: radio(batch=0), b"dm_pair_epoch_radiometric_src: batch 0 < 1"),
        (lambda: radio(epoch=-1), b"dm_pair_epoch_radiometric_src: epoch -1 < 0"),
        (lambda: radio(out=None), b"dm_pair_epoch_radiometric_src: bad arguments (null output)"),
    ]
    for call, message in cases:
        assert call() == -1, message
        assert message in lib.dm_last_error(), (message, lib.dm_last_error())
    # the existing entry points report under their own names, as before
    assert lib.dm_pair_epoch_orient(1, 0, 0, 4, 7, p, None) == -1 and b"dm_pair_epoch_orient: 0 pairs (1 .. 2^30)" in lib.dm_last_error()
    assert lib.dm_pair_epoch_radiometric(1, 0, 10, 4, 3, 0, 0, 0, None, None) == -1
    assert b"dm_pair_epoch_radiometric: bad arguments (null output)" in lib.dm_last_error()
    assert lib.dm_pair_epoch_draw(None, None) == -1 and b"dm_pair_epoch_draw: null arguments" in lib.dm_last_error()


def _host_images():
    rng = np.random.default_rng(0)
    n = 8
    return [{"tile": rng.integers(0, 256, (3, 60, 70), dtype=np.uint8), "xy": np.stack((rng.integers(0, 70, n), rng.integers(0, 60, n)), 1),
             "inner": np.full(n, 10), "obj": np.full(n, 16), "region": rng.random((n, 15), dtype=np.float32),
             "polygon_points": [[k, k + 4] for k in range(4)], "positive": np.array([[0, 1], [2, 3]]), "negative": np.array([[0, 3]])}]


def test_python_layers_refuse_bad_arguments_without_a_gpu():
    from deepmerge_amd import Train_SMT, ops
    from deepmerge_amd.dataset import PairDataset
    ds = PairDataset.from_arrays(_host_images(), seed=1, device="cpu")            # host tensors: enough for the argument checks
    w = lambda *v: torch.tensor(v, dtype=torch.int64)
    with pytest.raises(ValueError, match="draws needs weights"):
        ds.epoch(0, 2, draws=5)
    with pytest.raises(ValueError, match=">= 0"):
        ds.epoch(0, 2, weights=w(1, -1, 1))
    with pytest.raises(ValueError, match="every weight is 0"):
        ds.epoch(0, 2, weights=w(0, 0, 0))
    with pytest.raises(ValueError, match="2\\^62"):
        ds.epoch(0, 2, weights=w(1 << 61, 1 << 61, 0))
    with pytest.raises(ValueError, match="overflow"):
        ds.epoch(0, 2, weights=w((1 << 63) - 1, (1 << 63) - 1, 5))
    with pytest.raises(ValueError, match="int64"):
        ds.epoch(0, 2, weights=torch.ones(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        ds.epoch(0, 2, weights=w(1, 1))
    for bad in (0, (1 << 30) + 1):
        with pytest.raises(ValueError, match="draws"):
            ds.epoch(0, 2, weights=w(1, 1, 1), draws=bad)
    with pytest.raises(ValueError, match="draws needs"):
        Train_SMT.train(None, 1.0, 2, 1e-3, 0.0, 0.0, 0.1, 0, dataset=ds, draws=4)
    with pytest.raises(ValueError, match="mining"):
        Train_SMT.train(None, 1.0, 2, 1e-3, 0.0, 0.0, 0.1, 0, dataset=ds, mining=5)
    for kw in ({"every": 0}, {"every": 2.0}, {"cap": 0.0}, {"cap": float("inf")}, {"floor_share": 0.0}):
        with pytest.raises(ValueError, match="Mining"):
            ops.Mining(**kw)
    assert ops.Mining() == ops.Mining(every=5, cap=1.0, floor_share=1 / 16)
    with pytest.raises((ValueError, RuntimeError)):                               # host tensors are refused
        ops.pair_epoch_select(torch.ones(3, dtype=torch.int64), 0, 0, torch.zeros(3, dtype=torch.int32))
