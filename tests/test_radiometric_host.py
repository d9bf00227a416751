"""CPU: the numpy spec of the feed's radiometric jitter (tests/radiometric_ref.py) has the properties DESIGN.md 3.8 / 3.9 state -- the
identity table is the oriented gather, the pixel rule is a monotone clamped affine map that floors, the padding stays 0, the draw is
a keyed function of (seed, epoch, pair) within range at the span limits -- and the two new entry points are declared, bound, exported
and refuse bad arguments before any launch."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

import augment_ref as A
import radiometric_ref as RR
import train_smt_ref as R
from oracle import patches as OP


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


# ---- the pixel rule -----------------------------------------------------------------------------------------------------------------
def test_identity_table_gives_the_oriented_gather_exactly():
    rng = np.random.default_rng(3)
    tiles = rng.integers(0, 256, (2, 3, 40, 50), dtype=np.uint8)
    P = 10
    tile_id = (np.arange(P) % 2).astype(np.int32)
    xy = np.array([(0, 0), (49, 39), (25, 20), (-30, -30), (49, 0), (0, 39), (10, 38), (48, 5), (20, 20), (30, 10)], np.int32)
    inner, obj = np.array([9, 16, 24, 7, 5, 8, 12, 13, 1, 2], np.int32), np.array([10, 17, 25, 8, 6, 9, 13, 14, 2, 3], np.int32)
    orient = (np.arange(P) % 8).astype(np.int32)
    ident = np.tile(np.array(RR.IDENTITY, np.int32), (P, 3, 1))
    for rule in ("opencv", "exact_area"):
        want, wf = A.gather(tiles, tile_id, xy, inner, obj, orient, 0, 8, 24, rule)
        got, gf = RR.gather(tiles, tile_id, xy, inner, obj, orient, ident, 0, 8, 24, rule)
        assert got.dtype == want.dtype and np.array_equal(got, want) and not wf and not gf
        none, _ = RR.gather(tiles, tile_id, xy, inner, obj, None, ident, 0, 8, 24, rule)
        zero, _ = A.gather(tiles, tile_id, xy, inner, obj, np.zeros(P, np.int32), 0, 8, 24, rule)
        assert np.array_equal(none, zero)
    v = np.arange(256)
    assert np.array_equal(RR.pixel(v, *RR.IDENTITY), v)


def test_pixel_rule_is_monotone_and_clamps_at_both_ends():
    v = np.arange(256)
    for gain, offset in ((0, 0), (0, 65535), (1, -65535), (64, -40896), (256, 0), (300, -5000), (448, 40896), (1023, 65535), (1023, -65535),
                         (512, -32768), (128, 16384)):
        out = RR.pixel(v, gain, offset)
        assert out.dtype == np.uint8 and (np.diff(out.astype(int)) >= 0).all(), (gain, offset)
    assert RR.pixel(v, 1023, 65535).max() == 255 and RR.pixel(255, 1023, 65535) == 255          # 326528 >> 8 = 1275 -> 255
    assert RR.pixel(v, 256, -65535).min() == 0 and RR.pixel(0, 256, -65535) == 0
    assert np.array_equal(RR.pixel(v, 0, 65535), np.full(256, 255)) and np.array_equal(RR.pixel(v, 0, 0), np.zeros(256))
    out = RR.pixel(v, 512, -32768)                                                                 # contrast 2 about mid-grey
    assert out[64] == 0 and out[63] == 0 and out[128] == 128 and out[191] == 254 and out[192] == 255 and out[255] == 255
    # rounding to nearest: + 128 before the shift
    assert RR.pixel(1, 128, 0) == 1 and RR.pixel(1, 127, 0) == 0 and RR.pixel(3, 128, 0) == 2


def test_pixel_rule_floors_negative_sums():
    gain, offset, v = 256, -1000, 3                        # 768 - 1000 + 128 = -104: not a multiple of 256
    s = gain * v + offset + 128
    assert s < 0 and s % 256 != 0
    assert s >> 8 == -1 and int(s / 256) == 0              # floor, where truncation toward zero would give 0
    assert RR.pixel(v, gain, offset) == 0                  # (the clamp then takes every negative quotient to 0)
    # an arithmetic shift on int32 is what the kernel does: numpy's >> on a signed array is the same
    assert (np.array([-104, -256, -257, -1], np.int32) >> 8).tolist() == [-1, -1, -2, -1]


def test_padding_stays_zero_under_a_positive_offset():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (3, 20, 30), dtype=np.uint8)
    radio = np.array([(256, 65535), (0, 30000), (1023, 1)], np.int32)
    for x0, y0, L in ((-4, -3, 10), (25, 15, 10), (-50, 0, 8), (10, -2, 6)):
        crop = RR.radio_crop(img, x0, y0, L, radio)
        inside = OP.cut_image(np.ones_like(img), x0, y0, L).astype(bool)
        assert not crop[~inside].any()
        if inside.any():
            assert (crop[0][inside[0]] == 255).all() and (crop[1][inside[1]] == 117).all()         # (30000 + 128) >> 8
    assert not RR.augmented_patch(img, -50, -50, 8, 4, 5, radio).any()


# ---- the designed row ---------------------------------------------------------------------------------------------------------------
def _region(rng, n):
    reg = rng.random((n, 15), dtype=np.float32) * np.float32(4)
    reg[:, 5:8] = rng.random((n, 3), dtype=np.float32) * np.float32(60)
    reg[:, 8:11] = rng.random((n, 3), dtype=np.float32) * np.float32(255)
    reg[:, 13] = reg[:, 8:11].mean(1)
    return reg


@pytest.mark.parametrize("bands", [1, 3, 4])
def test_designed_row_at_the_identity_is_the_untransformed_row_bit_for_bit_and_moves_only_its_seven_entries(bands):
    rng = np.random.default_rng(bands)
    reg = _region(rng, 6)
    nb = min(bands, 3)
    for r in reg:
        plain = A.designed_row(r, 20, 31)
        ident = RR.designed_row(r, 20, 31, np.tile(np.array(RR.IDENTITY), (bands, 1)), bands)
        assert ident.dtype == np.float32 and np.array_equal(ident.view(np.uint32), plain.view(np.uint32))
        radio = np.stack((rng.integers(64, 449, bands), rng.integers(-40896, 40897, bands)), 1)
        moved = RR.designed_row(r, 20, 31, radio, bands)
        touched = set(range(5, 5 + nb)) | set(range(8, 8 + nb)) | {13}
        same = [k for k in range(19) if moved.view(np.uint32)[k] == plain.view(np.uint32)[k]]
        assert set(range(19)) - touched <= set(same)
        for c in range(nb):
            g, b = radio[c, 0] / 256.0, radio[c, 1] / 256.0
            assert moved[8 + c] == pytest.approx(min(255.0, max(0.0, g * float(plain[8 + c]) + b)), rel=1e-6, abs=1e-4)
            assert moved[5 + c] == pytest.approx(g * float(plain[5 + c]), rel=1e-6)
        assert moved[13] == pytest.approx(float(plain[13]) + float(np.mean(moved[8:8 + nb].astype(np.float64) - plain[8:8 + nb])), abs=1e-3)
        bad = radio.copy()
        bad[bands - 1, 0] = 1024
        assert np.array_equal(RR.designed_row(r, 20, 31, bad, bands).view(np.uint32), plain.view(np.uint32))
    # the mean clamps at both ends
    r = reg[0].copy()
    r[8:11] = (250.0, 3.0, 100.0)
    moved = RR.designed_row(r, 20, 31, np.array([(448, 0), (256, -65535), (256, 256)]), 3)
    assert moved[8] == 255.0 and moved[9] == 0.0 and moved[10] == 101.0


# ---- the draw -----------------------------------------------------------------------------------------------------------------------
def test_sym_covers_exactly_minus_s_to_s_and_is_zero_at_zero():
    r = np.unique(np.concatenate((np.linspace(0, 2 ** 32 - 1, 1 << 20).astype(np.uint64), [0, 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]))).astype(np.uint32)
    for s in (1, 3, 64, 128, 16320):
        v = RR.sym(r, s)
        assert v.dtype == np.int32 and set(np.unique(v).tolist()) == set(range(-s, s + 1)), s
        assert RR.sym(0, s) == -s and RR.sym(2 ** 32 - 1, s) == s
        assert (np.diff(RR.sym(np.sort(r), s)) >= 0).all()
    assert not RR.sym(r, 0).any()
    counts = np.bincount(RR.sym(r, 3) + 3, minlength=7)
    assert np.abs(counts - len(r) / 7).max() <= 4        # evenly spaced words fill the bins evenly: +-1 at each bin edge, <= 2 added words a bin


@pytest.mark.parametrize("bands", [1, 3, 4, 5, 16])
def test_every_drawn_table_is_in_range_at_the_span_limits(bands):
    N = 4000
    t = RR.epoch_radio(N, 9, 2, 32, bands, *RR.MAX_SPANS)
    assert t.dtype == np.int32 and t.shape == (2 * N, bands, 2) and RR.in_range(t)
    assert t[..., 0].min() >= 64 and t[..., 0].max() <= 448 and np.abs(t[..., 1]).max() <= 40896
    assert t[..., 0].min() < 100 and t[..., 0].max() > 412                          # and the limits are approached
    assert (np.abs(t[..., 0].astype(np.int64) * 255 + t[..., 1] + 128) < 1 << 19).all()
    assert np.array_equal(t[..., 1] + 128 * (t[..., 0] - 256), np.broadcast_to(t[:, :1, 1] + 128 * (t[:, :1, 0] - 256), t.shape[:2]))   # one b0 per pair
    if bands > 1:
        assert (t[:, 0, 0] != t[:, 1, 0]).any()
    zero = RR.epoch_radio(N, 9, 2, 32, bands, 0, 0, 0)
    assert np.array_equal(zero, np.broadcast_to(np.array(RR.IDENTITY, np.int32), zero.shape))
    for bad in ((129, 0, 0), (0, 65, 0), (0, 0, 16321), (-1, 0, 0)):
        with pytest.raises(ValueError):
            RR.epoch_radio(N, 9, 2, 32, bands, *bad)
    for nb in (0, 17):
        with pytest.raises(ValueError):
            RR.epoch_radio(N, 9, 2, 32, nb, 1, 1, 1)


@pytest.mark.parametrize("N,batch", [(1, 1), (5, 2), (37, 7), (37, 37), (1000, 32)])
def test_both_rows_of_a_pair_are_equal_and_the_table_is_keyed_by_seed_epoch_and_pair(N, batch):
    sp = RR.spans()
    t = RR.epoch_radio(N, 5, 1, batch, 4, *sp)
    rl, rr = R.blocked_rows(N, batch)
    assert np.array_equal(t[rl], t[rr])
    src = R.epoch_perm(N, 5, 1)
    assert np.array_equal(t[rl], RR.pair_radio(src, 5, 1, 4, *sp))                  # keyed by the pair, not by position or batch size
    assert np.array_equal(t, RR.epoch_radio(N, 5, 1, batch, 4, *sp))
    if N >= 37:
        assert not np.array_equal(t, RR.epoch_radio(N, 5, 2, batch, 4, *sp))
        assert not np.array_equal(t, RR.epoch_radio(N, 6, 1, batch, 4, *sp))
        assert not np.array_equal(t, RR.epoch_radio(N, 5 + (1 << 32), 1, batch, 4, *sp))
        # word 4 is a stream of its own: not the orientation's (3)
        other = R.philox4x32_10((src.astype(np.uint32), 1, 3, 0), R.seed_key(5))
        assert not np.array_equal(256 + RR.sym(other[0], sp[0]), 256 + RR.sym(R.philox4x32_10((src.astype(np.uint32), 1, 4, 0), R.seed_key(5))[0], sp[0]))
    # band c of 5 reads word c % 4 of block 1 + c / 4: the first four bands of a 5-band table are the 4-band table
    assert np.array_equal(RR.epoch_radio(N, 5, 1, batch, 5, *sp)[:, :4], t)


# ---- the Python layers, without a GPU -----------------------------------------------------------------------------------------------
def test_radiometric_spans_and_refusals():
    from deepmerge_amd import ops
    r = ops.Radiometric()
    assert (r.contrast, r.brightness, r.colour) == (0.2, 0.1, 0.05)
    assert r.spans() == (51, 13, 6528) == RR.spans()
    assert ops.Radiometric(0.5, 0.25, 0.25).spans() == RR.MAX_SPANS
    assert ops.Radiometric(0, 0, 0).spans() == (0, 0, 0)
    assert ops.Radiometric(contrast=0.3, brightness=0.05, colour=0.1).spans() == RR.spans(0.3, 0.05, 0.1) == (77, 26, 3264)
    with pytest.raises(dataclasses.FrozenInstanceError):
        r.contrast = 0.3
    for kw in ({"contrast": 0.51}, {"contrast": -0.01}, {"brightness": 0.26}, {"brightness": -1}, {"colour": 0.251}, {"colour": -0.1},
               {"contrast": float("nan")}, {"colour": "0.1"}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            ops.Radiometric(**kw)
    assert ops.Radiometric.of(None) is None and ops.Radiometric.of(r) is r and ops.Radiometric.of((0.3, 0.05, 0.1)) == ops.Radiometric(0.3, 0.05, 0.1)
    for bad in ("d4", 0.2, (0.1, 0.1), (0.1, 0.1, 0.1, 0.1)):
        with pytest.raises(ValueError, match="radiometric"):
            ops.Radiometric.of(bad)


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
    for bad in ("d4", (0.6, 0.1, 0.1), (0.1, 0.3, 0.1), (0.1, 0.1), 1.0):
        with pytest.raises(ValueError, match="adiometric"):
            ds.epoch(0, 2, radiometric=bad)
        with pytest.raises(ValueError, match="adiometric"):
            Train_SMT.train(None, 1.0, 2, 1e-3, 0.0, 0.0, 0.1, 0, dataset=ds, radiometric=bad)
    # PairTable: `radio` is keyword-only and optional, the positional fields are unchanged; stack joins it only when both sides carry one
    B = 3
    i32 = lambda v: torch.full((B,), v, dtype=torch.int32)
    rad = lambda g: torch.tensor([[[g, 0]] * 3] * B, dtype=torch.int32)
    mk = lambda o, r: PairTable(i32(0), torch.zeros((B, 2), dtype=torch.int32), i32(10), i32(16), torch.zeros((B, 15)), torch.ones(B), o, radio=r)
    assert mk(None, None).radio is None and mk(i32(5), None).orient.tolist() == [5] * B
    with pytest.raises(TypeError):
        PairTable(i32(0), torch.zeros((B, 2), dtype=torch.int32), i32(10), i32(16), torch.zeros((B, 15)), torch.ones(B), None, rad(256))
    both = PairTable.stack(mk(i32(5), rad(300)), mk(i32(5), rad(200)))
    assert both.radio.dtype == torch.int32 and both.radio.shape == (2 * B, 3, 2) and both.radio[:, 0, 0].tolist() == [300] * B + [200] * B
    assert both.orient.tolist() == [5] * (2 * B)
    assert PairTable.stack(mk(None, rad(300)), mk(None, None)).radio is None and PairTable.stack(mk(None, rad(1)), mk(None, rad(2))).orient is None
    with pytest.raises((ValueError, RuntimeError)):                               # host tensors are refused
        ops.pair_epoch_radiometric(0, 0, 3, 2, 3, 1, 1, 1, torch.zeros((6, 3, 2), dtype=torch.int32))


# ---- the library's side, without a GPU ----------------------------------------------------------------------------------------------
NEW = ("dm_pair_batch_gather_augmented", "dm_pair_epoch_radiometric")


def test_new_symbols_are_declared_bound_and_exported_and_the_abi_is_still_7(built):
    lib = built.lib()
    assert lib.dm_abi_version() == 7
    declared = built.declared_symbols()
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW:
        assert name in declared and name in built.SIGNATURES and hasattr(raw, name), name
    text = open(built.HEADER_PATH).read()
    for name, nargs in zip(NEW, (23, 10)):
        proto = text[text.index("int " + name + "("):]
        proto = proto[:proto.index(";")]
        assert proto.count(",") + 1 == nargs == len(built.SIGNATURES[name][1]), name
    assert len(built.SIGNATURES["dm_pair_batch_gather"][1]) == 21 and len(built.SIGNATURES["dm_pair_batch_gather_oriented"][1]) == 22
    for macro, value in zip(("DM_RADIO_MAX_GAIN_SPAN", "DM_RADIO_MAX_BAND_SPAN", "DM_RADIO_MAX_OFFSET_SPAN"), RR.MAX_SPANS):
        assert f"#define {macro} {value}\n" in text


def test_entry_points_refuse_bad_arguments_before_any_launch(built):
    lib = built.lib()
    p = 4096                                                                       # any non-null address: validation never dereferences
    F32, BF16 = built.DM_F32, built.DM_BF16

    def gather(*, tiles=p, n_tiles=2, bands=3, H=64, W=64, xy=p, inner=p, obj=p, orient=p, radio=p, scale_index=0, max_window=64, P=8,
               target=32, grid=0, rule=0, out=p, dtype=F32, region=None, designed=None):
        return lib.dm_pair_batch_gather_augmented(tiles, n_tiles, bands, H, W, p, xy, inner, obj, orient, radio, scale_index, max_window, P,
                                                  target, grid, rule, out, dtype, region, designed, None, None)

    def draw(*, seed=1, epoch=0, n=10, batch=4, bands=3, gain=51, band=13, offset=6528, out=p):
        return lib.dm_pair_epoch_radiometric(seed, epoch, n, batch, bands, gain, band, offset, out, None)

    name, dname = b"dm_pair_batch_gather_augmented: ", b"dm_pair_epoch_radiometric: "
    cases = [
        (lambda: gather(radio=None), -1, name + b"null radio"),
        (lambda: gather(radio=None, orient=None), -1, name + b"null radio"),
        (lambda: gather(rule=2), -6, name + b"unknown resize rule"),
        (lambda: gather(tiles=None), -1, name + b"bad arguments"),
        (lambda: gather(xy=None), -1, name + b"bad arguments"),
        (lambda: gather(inner=None), -1, name + b"bad arguments"),
        (lambda: gather(obj=None), -1, name + b"bad arguments"),
        (lambda: gather(out=None), -1, name + b"bad arguments"),
        (lambda: gather(n_tiles=0), -1, name + b"bad arguments"),
        (lambda: gather(bands=0), -1, name + b"bad arguments"),
        (lambda: gather(P=0), -1, name + b"bad arguments"),
        (lambda: gather(target=0), -1, name + b"bad arguments"),
        (lambda: gather(scale_index=4), -1, name + b"scale index"),
        (lambda: gather(grid=5), -1, name + b"target 32 is not a multiple"),
        (lambda: gather(max_window=0), -6, name + b"window bound"),
        (lambda: gather(max_window=385), -6, name + b"window bound"),
        (lambda: gather(bands=65536), -1, name + b"too many bands"),
        (lambda: gather(region=p), -1, name + b"designed rows need"),
        (lambda: gather(designed=p), -1, name + b"designed rows need"),
        (lambda: gather(dtype=BF16), -2, name + b"planar patches are fp32"),
        (lambda: gather(orient=None, dtype=BF16), -2, name + b"planar patches are fp32"),          # a null orient alone is accepted
        (lambda: gather(grid=8, dtype=3), -2, name + b"bad dtype"),
        (lambda: draw(gain=129), -1, dname + b"gain span 129 outside 0..128"),
        (lambda: draw(gain=-1), -1, dname + b"gain span -1 outside 0..128"),
        (lambda: draw(band=65), -1, dname + b"band span 65 outside 0..64"),
        (lambda: draw(band=-1), -1, dname + b"band span -1 outside 0..64"),
        (lambda: draw(offset=16321), -1, dname + b"offset span 16321 outside 0..16320"),
        (lambda: draw(offset=-1), -1, dname + b"offset span -1 outside 0..16320"),
        (lambda: draw(bands=0), -1, dname + b"0 bands (1 .. 16)"),
        (lambda: draw(bands=17), -1, dname + b"17 bands (1 .. 16)"),
        (lambda: draw(n=0), -1, dname + b"0 pairs"),
        (lambda: draw(n=(1 << 30) + 1), -1, dname + b"1073741825 pairs"),
        (lambda: draw(batch=0), -1, dname + b"batch 0 < 1"),
        (lambda: draw(epoch=-1), -1, dname + b"epoch -1 < 0"),
        (lambda: draw(out=None), -1, dname + b"bad arguments (null output)"),
    ]
    for call, status, message in cases:
        assert call() == status, message
        assert message in lib.dm_last_error(), (message, lib.dm_last_error())
    # the oriented entry still needs its orient, and reports under its own name
    assert lib.dm_pair_batch_gather_oriented(p, 2, 3, 64, 64, p, p, p, p, None, 0, 64, 8, 32, 0, 0, p, F32, None, None, None, None) == -1
    assert b"dm_pair_batch_gather_oriented: null orient" in lib.dm_last_error()
