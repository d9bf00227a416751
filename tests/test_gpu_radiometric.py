"""GPU: the feed's radiometric jitter.  dm_pair_batch_gather_augmented and dm_pair_epoch_radiometric against the numpy spec
(tests/radiometric_ref.py) bit for bit -- every staging form, both resize rules, every output form, windows over the raster's corners,
edges and outside it, tables at the ends of their ranges -- and the training integration: PairDataset.epoch(radiometric=),
PairFeed.fill, the captured step and Train_SMT.train(radiometric=)."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import augment_ref as A
import radiometric_ref as RR
import train_smt_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 97, 113

# target -> (window sides, bound of the LDS staging)
#   32: 1, 2 (degenerate), 31 / 33 (either side of the identity 32: area tables / enlarging)
#   256: 100 (enlarging across the output-row bands), 384 (gridDim.z = 8, the full LDS, the transposed band staging)
CASES = {32: ((1, 2, 31, 32, 33), 40), 256: ((100, 384), 384)}
ORIENTS = (0, 3, 4, 7)                                    # plain rows, mirrored rows, the transposed walk, transposed and mirrored
# a raster corner, the opposite corner, an edge, inside, and a window wholly outside the raster at every side used here
POINTS = ((0, 0), (W - 1, H - 1), (W // 2, 0), (W // 2 + 3, H // 2 - 5), (-500, 40))
# per-band (gain, offset) tables: identity, gain 0, the top of both ranges, the bottom of the offset's, four different bands,
# a positive offset alone, gain 0 with the largest offset
RADIOS = (((256, 0),) * 4, ((0, 30000),) * 4, ((1023, 65535),) * 4, ((256, -65535),) * 4,
          ((300, -5000), (200, 7000), (448, -24576), (64, 24576)), ((256, 20000),) * 4, ((0, 65535), (1023, -65535), (0, 0), (1, 1)))


def up(a):
    return torch.from_numpy(np.array(a)).to(DEV)            # (a copy: the shared tables are read-only arrays)


@functools.lru_cache(maxsize=None)
def tiles4():
    rng = np.random.default_rng(7)
    t = rng.integers(0, 256, size=(2, 4, H, W), dtype=np.uint8)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def table(target):
    """Sample k: side sides[k // per_side], orientation and point and radiometric table rotating with periods 4, 5 and 7, so that every
    (point, table) combination occurs at target 32."""
    sides, _ = CASES[target]
    per = 8 if target == 32 else 4                        # (the 256 x 256 spec is the slow one on the host: one sample per orientation)
    rows, radio = [], []
    for k in range(len(sides) * per):
        x, y = POINTS[k % len(POINTS)]
        rows.append((k % 2, x, y, sides[k // per], ORIENTS[(k // (per // 4)) % 4]))
        radio.append(RADIOS[(k + (4 if target == 256 else 0)) % len(RADIOS)])
    t = np.asarray(rows, np.int32)
    cols = {"tile_id": t[:, 0].copy(), "xy": t[:, 1:3].copy(), "inner": t[:, 3].copy(), "obj": (t[:, 3] + 1).astype(np.int32), "orient": t[:, 4].copy(),
            "radio": np.asarray(radio, np.int32)}
    for v in cols.values():
        v.setflags(write=False)
    return cols


@functools.lru_cache(maxsize=None)
def spec(target, rule, oriented=True):
    """float32 [P, 4, target, target] for the 4-band tiles, computed once and shared (read only): bands are independent, so the first
    b planes are the spec of the first b bands under the first b rows of every table."""
    c = table(target)
    out, flagged = RR.gather(tiles4(), c["tile_id"], c["xy"], c["inner"], c["obj"], c["orient"] if oriented else None, c["radio"], 0, target,
                             CASES[target][1], rule)
    assert not flagged
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def region(P):
    """Attributes on the tile bytes' 0..255 scale, as rag.label_stats produces them."""
    rng = np.random.default_rng(P)
    reg = rng.random((P, 15), dtype=np.float32) * np.float32(4)
    reg[:, 5:8] = rng.random((P, 3), dtype=np.float32) * np.float32(60)
    reg[:, 8:11] = rng.random((P, 3), dtype=np.float32) * np.float32(255)
    reg[:, 13] = reg[:, 8:11].mean(1)
    reg.setflags(write=False)
    return reg


def run_gather(tiles, c, target, max_window, rule, form, orient="table", radio="table", designed=False, flag=None):
    """form: "planar" (fp32 [P, bands, t, t]), "rows_bf16" / "rows_fp32" (grid 8).  orient / radio: "table", None or an array."""
    from deepmerge_amd import ops
    P, bands = len(c["inner"]), tiles.shape[1]
    grid = 0 if form == "planar" else 8
    dtype = torch.bfloat16 if form == "rows_bf16" else torch.float32
    out = torch.full((P, bands, target, target) if grid == 0 else (P * 64, bands * (target // 8) ** 2), 7.0, dtype=dtype, device=DEV)
    o = c["orient"] if isinstance(orient, str) else orient
    r = c["radio"][:, :bands] if isinstance(radio, str) else radio
    reg = drow = None
    if designed:
        reg = up(region(P))
        drow = torch.full((P, 1, 19), 7.0, device=DEV)
    ops.pair_batch_gather(tiles, up(c["tile_id"]), up(c["xy"]), up(c["inner"]), up(c["obj"]), 0, target, max_window, out, grid=grid, resize=rule,
                          region_features=reg, designed=drow, error_flag=flag, orient=None if o is None else up(o),
                          radio=None if r is None else up(np.ascontiguousarray(r)))
    return (out, drow) if designed else out


def want_form(ref, form):
    """The spec [P, bands, t, t] in an output form, as a torch CPU tensor."""
    if form == "planar":
        return torch.from_numpy(np.array(ref))
    rows = torch.from_numpy(np.concatenate([A.patch_rows(p, 8) for p in ref]))
    return rows.to(torch.bfloat16) if form == "rows_bf16" else rows


def bits(t):
    return t.contiguous().view(torch.uint8)


def assert_samples_equal(got, want, c, what):
    assert got.dtype == want.dtype and got.shape == want.shape
    P = len(c["inner"])
    per = (bits(got).reshape(P, -1) != bits(want).reshape(P, -1)).any(1).numpy()
    bad = [(*c["xy"][p].tolist(), int(c["inner"][p]), int(c["orient"][p]), c["radio"][p].tolist()) for p in np.nonzero(per)[0][:4]]
    assert not per.any(), f"{what}: {int(per.sum())} of {P} samples differ, first (x, y, L, orient, radio): {bad}"


# ---- 1. the gather against the spec -------------------------------------------------------------------------------------------------
def test_the_tables_cover_what_they_claim():
    c = table(32)
    assert set(c["orient"]) == set(ORIENTS) == set(table(256)["orient"]) and set(c["inner"]) == {1, 2, 31, 32, 33}
    big = c["inner"] >= 31
    for x, y in POINTS[:3] + POINTS[4:]:                                           # corner, corner, edge, outside: each under a positive offset
        at = big & (c["xy"][:, 0] == x) & (c["xy"][:, 1] == y)
        assert (c["radio"][at][:, :, 1] > 0).any(), (x, y)
    seen = {tuple(map(tuple, r)) for r in c["radio"]}
    assert seen == set(RADIOS) and len({tuple(map(tuple, r)) for r in table(256)["radio"]}) >= 4
    ref = spec(32, "opencv")
    outside = c["xy"][:, 0] < -400
    assert outside.sum() >= 8 and (c["radio"][outside][:, :, 1] > 0).any() and not ref[outside].any()   # the pad stays 0
    plain, _ = A.gather(tiles4(), c["tile_id"], c["xy"], c["inner"], c["obj"], c["orient"], 0, 32, CASES[32][1])
    changed = (plain != ref).reshape(len(ref), -1).any(1)
    assert changed.sum() >= 20                                                     # the tables are not no-ops


@pytest.mark.parametrize("rule", ["opencv", "exact_area"])
@pytest.mark.parametrize("bands", [1, 3, 4])
@pytest.mark.parametrize("target", sorted(CASES))
def test_augmented_gather_equals_spec_bit_for_bit(target, bands, rule):
    tiles = up(tiles4()[:, :bands])
    c, ref = table(target), spec(target, rule)[:, :bands]
    for form in ("planar", "rows_bf16", "rows_fp32"):
        got = run_gather(tiles, c, target, CASES[target][1], rule, form).cpu()
        assert_samples_equal(got, want_form(ref, form), c, form)


@pytest.mark.parametrize("bands", [1, 4])
def test_a_null_orient_is_orientation_zero(bands):
    tiles = up(tiles4()[:, :bands])
    c = table(32)
    P = len(c["inner"])
    for rule in ("opencv", "exact_area"):
        ref = spec(32, rule, oriented=False)[:, :bands]
        for form in ("planar", "rows_bf16"):
            got = run_gather(tiles, c, 32, CASES[32][1], rule, form, orient=None).cpu()
            assert_samples_equal(got, want_form(ref, form), c, (rule, form))
    c = table(256)                                                                 # gridDim.z = 8: against the explicit zeros, on the device
    null = run_gather(tiles, c, 256, 384, "opencv", "rows_bf16", orient=None)
    zero = run_gather(tiles, c, 256, 384, "opencv", "rows_bf16", orient=np.zeros(len(c["inner"]), np.int32))
    other = run_gather(tiles, c, 256, 384, "opencv", "rows_bf16")
    assert torch.equal(bits(null), bits(zero)) and not torch.equal(bits(null), bits(other))


@pytest.mark.parametrize("target", [32, 256])
def test_the_identity_table_equals_the_oriented_gather_bit_for_bit(target):
    tiles = up(tiles4())
    c, mw = table(target), CASES[target][1]
    P = len(c["inner"])
    ident = np.tile(np.array(RR.IDENTITY, np.int32), (P, 4, 1))
    for rule in ("opencv", "exact_area"):
        for form in ("planar", "rows_bf16", "rows_fp32"):
            oriented, d_oriented = run_gather(tiles, c, target, mw, rule, form, radio=None, designed=True)
            got, d_got = run_gather(tiles, c, target, mw, rule, form, radio=ident, designed=True)
            assert oriented.dtype == got.dtype and torch.equal(bits(oriented), bits(got)), (rule, form)
            assert torch.equal(d_oriented.view(torch.int32), d_got.view(torch.int32))
    want = np.stack([A.designed_row(r, i, ob) for r, i, ob in zip(region(P), c["inner"], c["obj"])])
    assert np.array_equal(d_got.cpu().numpy().reshape(P, 19).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("bands", [1, 3, 4])
def test_designed_rows_equal_the_spec(bands):
    tiles = up(tiles4()[:, :bands])
    c = table(32)
    P = len(c["inner"])
    radio = c["radio"][:, :bands]
    want = np.stack([RR.designed_row(r, i, ob, t, bands) for r, i, ob, t in zip(region(P), c["inner"], c["obj"], radio)])
    plain = np.stack([A.designed_row(r, i, ob) for r, i, ob in zip(region(P), c["inner"], c["obj"])])
    nb = min(bands, 3)
    moved = want.view(np.uint32) != plain.view(np.uint32)
    touched = sorted(set(range(5, 5 + nb)) | set(range(8, 8 + nb)) | {13})
    assert moved[:, touched].any(0).all() and not np.delete(moved, touched, 1).any()          # the nb rule: these columns and no other
    assert (want[:, 8:8 + nb] == 0.0).any() and (want[:, 8:8 + nb] == 255.0).any()            # the mean clamps at both ends
    for form, orient in (("planar", "table"), ("rows_bf16", None)):
        _, drow = run_gather(tiles, c, 32, CASES[32][1], "opencv", form, orient=orient, designed=True)
        got = drow.cpu().numpy().reshape(P, 19)
        diff = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
        assert diff.size == 0, (form, diff[:4], got[diff[:1]], want[diff[:1]], radio[diff[:1]])


def test_a_value_out_of_range_feeds_zeros_for_that_sample_only_and_raises_the_flag():
    from deepmerge_amd.feed import PairFeed, PairTable
    bands = 3
    tiles = up(tiles4()[:, :bands])
    c = {k: v[:8].copy() for k, v in table(32).items()}
    c["inner"][:] = 31
    c["obj"][:] = 40
    c["xy"][:] = (50, 50)
    c["orient"][:] = np.arange(8)
    c["radio"] = np.ascontiguousarray(np.asarray([RADIOS[4]] * 8, np.int32)[:, :bands])
    ref, _ = RR.gather(tiles4()[:, :bands], c["tile_id"], c["xy"], c["inner"], c["obj"], c["orient"], c["radio"], 0, 32, 100)
    d_ref = np.stack([RR.designed_row(r, 31, 40, t, bands) for r, t in zip(region(8), c["radio"])])
    d_plain = np.stack([A.designed_row(r, 31, 40) for r in region(8)])
    assert ref.reshape(8, -1).any(1).all()
    flag = torch.zeros((1,), dtype=torch.int32, device=DEV)
    for bad_at, band, col, bad in ((2, 1, 0, 1024), (5, 2, 1, 65536), (0, 0, 0, -1), (7, 0, 1, -65536)):
        r = c["radio"].copy()
        r[bad_at, band, col] = bad
        spec_out, spec_flag = RR.gather(tiles4()[:, :bands], c["tile_id"], c["xy"], c["inner"], c["obj"], c["orient"], r, 0, 32, 100)
        want, want_d = ref.copy(), d_ref.copy()
        want[bad_at] = 0.0                                                           # every band of that sample, and no other sample
        want_d[bad_at] = d_plain[bad_at]                                             # its designed row: written, untransformed
        assert spec_flag and np.array_equal(spec_out, want)
        for form in ("planar", "rows_bf16"):
            flag.zero_()
            got, drow = run_gather(tiles, c, 32, 100, "opencv", form, radio=r, designed=True, flag=flag)
            assert torch.equal(bits(got.cpu()), bits(want_form(want, form))), (bad, form)
            assert np.array_equal(drow.cpu().numpy().reshape(8, 19).view(np.uint32), want_d.view(np.uint32)), (bad, form)
            assert int(flag.item()) == 1
    flag.zero_()
    run_gather(tiles, c, 32, 100, "opencv", "planar", flag=flag)
    assert int(flag.item()) == 0
    # through the feed: nothing is read back by fill(); check() raises once and the next batch is clean
    B = 4
    mk = lambda r: PairTable(up(c["tile_id"]), up(c["xy"]), up(c["inner"]), up(c["obj"]), up(region(8)), torch.ones(B, device=DEV), up(c["orient"]),
                             radio=up(r))
    feed = PairFeed(tiles, [32, 64], B, 100, rows=False)
    r = c["radio"].copy()
    r[6, 1, 0] = 1024
    left, _, right, _, _ = feed.fill(mk(r))
    assert float(right[0][2].abs().max()) == 0.0 and float(right[1][2].abs().max()) == 0.0 and float(right[0][1].abs().max()) > 0.0
    with pytest.raises(ValueError, match="radiometric"):
        feed.check()
    feed.fill(mk(c["radio"]))
    feed.check()


def test_inputs_are_unmodified_and_the_python_layer_refuses_a_misshapen_table():
    from deepmerge_amd import ops
    tiles = up(tiles4())
    c = table(32)
    ins = [up(c[k]) for k in ("tile_id", "xy", "inner", "obj", "orient", "radio")]
    before = [t.clone() for t in ins] + [tiles.clone()]
    P = len(c["inner"])
    out = torch.full((P * 64, 4 * 4 * 4), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.pair_batch_gather(tiles, *ins[:4], 0, 32, 40, out, grid=8, orient=ins[4], radio=ins[5])
    assert torch.equal(bits(out.cpu()), bits(want_form(spec(32, "opencv"), "rows_bf16")))
    assert all(torch.equal(a, b) for a, b in zip(ins + [tiles], before))
    for bad in (ins[5].to(torch.int64), ins[5][:-1], ins[5][:, :3], ins[5].reshape(P, 8)):
        with pytest.raises(ValueError, match="radio"):
            ops.pair_batch_gather(tiles, *ins[:4], 0, 32, 40, out, grid=8, orient=ins[4], radio=bad)


# ---- 2. the table draw --------------------------------------------------------------------------------------------------------------
def _kernel_radio(seed, epoch, N, batch, bands, spans):
    from deepmerge_amd import ops
    out = torch.full((2 * N, bands, 2), 99999, dtype=torch.int32, device=DEV)
    ops.pair_epoch_radiometric(seed, epoch, N, batch, bands, *spans, out)
    return out.cpu().numpy()


@pytest.mark.parametrize("N", [1, 5, 256, 257])
def test_epoch_radiometric_equals_spec_bit_for_bit(N):
    seed = 0x9E3779B97F4A7C15                                                        # above 2^32: both key words count
    for batch in (3, 7):                                                             # neither divides 5, 256 or 257
        for bands in (1, 3, 4, 5):
            for spans in ((0, 0, 0), RR.MAX_SPANS, RR.spans()):
                for epoch in (0, 2 ** 31 - 1):
                    got = _kernel_radio(seed, epoch, N, batch, bands, spans)
                    want = RR.epoch_radio(N, seed, epoch, batch, bands, *spans)
                    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (batch, bands, spans, epoch)
    if N >= 256:
        a = _kernel_radio(seed, 0, N, 7, 4, RR.MAX_SPANS)
        assert RR.in_range(a) and a[..., 0].min() >= 64 and a[..., 0].max() <= 448
        assert not np.array_equal(a, _kernel_radio(seed, 1, N, 7, 4, RR.MAX_SPANS))
        assert not np.array_equal(a, _kernel_radio(seed & 0xFFFFFFFF, 0, N, 7, 4, RR.MAX_SPANS))
        rl, rr = R.blocked_rows(N, 7)
        assert np.array_equal(a[rl], a[rr])
    from deepmerge_amd import ops
    for shape in ((2 * N, 4), (2 * N + 1, 4, 2)):
        with pytest.raises(ValueError, match="pair_epoch_radiometric"):
            ops.pair_epoch_radiometric(seed, 0, N, 3, 4, 1, 1, 1, torch.zeros(shape, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="gain span"):
        ops.pair_epoch_radiometric(seed, 0, N, 3, 4, 129, 1, 1, torch.zeros((2 * N, 4, 2), dtype=torch.int32, device=DEV))


# ---- 3. training integration --------------------------------------------------------------------------------------------------------
SCALES = [32, 64, 128]


def _images(seed=0):
    """Two images of different sizes, 24 points each in 8 polygons; 10 pairs in all; attributes on the 0..255 scale."""
    rng = np.random.default_rng(seed)
    ims = []
    for h, w in ((150, 180), (210, 170)):
        n = 24
        inner = rng.integers(8, 30, n)
        reg = rng.random((n, 15), dtype=np.float32)
        reg[:, 5:8] *= np.float32(60)
        reg[:, 8:11] *= np.float32(255)
        reg[:, 13] = reg[:, 8:11].mean(1)
        ims.append({"tile": rng.integers(0, 256, size=(3, h, w), dtype=np.uint8), "xy": np.stack((rng.integers(0, w, n), rng.integers(0, h, n)), 1),
                    "inner": inner, "obj": inner + rng.integers(4, 40, n), "region": reg,
                    "polygon_points": [list(range(k, n, 8)) for k in range(8)]})
    ims[0]["positive"], ims[1]["positive"] = np.array([[0, 1], [2, 3], [4, 5]]), np.array([[1, 2], [3, 4], [6, 7]])
    ims[0]["negative"], ims[1]["negative"] = np.array([[0, 7], [5, 6]]), np.array([[0, 5], [2, 7]])
    return ims


def _net(seed=3):
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    torch.manual_seed(seed)
    return ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=list(SCALES), depth=[1, 1, 1], in_c=3, numerics="bf16").to(DEV)


def _radiometric():
    from deepmerge_amd import ops
    return ops.Radiometric(contrast=0.4, brightness=0.2, colour=0.1)


def test_dataset_epoch_with_radiometric_and_d4_then_fill_equals_the_spec_driven_gather():
    from deepmerge_amd.dataset import PairDataset
    from deepmerge_amd.feed import PairFeed
    ds = PairDataset.from_arrays(_images(), seed=11)
    N, B, e, rad = len(ds), 4, 2, _radiometric()
    assert N == 10 and rad.spans() == RR.spans(0.4, 0.2, 0.1)
    plain = ds.epoch(e, B, augment="d4")
    assert "radio" not in plain.cols and plain.step(0).radio is None and plain.step(2).radio is None
    want_cols = {k: v.clone() for k, v in plain.cols.items()}
    only = ds.epoch(e, B, radiometric=rad)                                         # independent of augment=
    assert "orient" not in only.cols and only.step(1).orient is None and only.step(1).radio is not None
    tab = ds.epoch(e, B, augment="d4", radiometric=(0.4, 0.2, 0.1))                # a triple is an ops.Radiometric
    assert all(torch.equal(tab.cols[k], want_cols[k]) for k in want_cols)          # the draw and the orientations do not change
    assert tab.cols["radio"].data_ptr() == only.cols["radio"].data_ptr()           # allocated once
    radio = tab.cols["radio"].cpu().numpy()
    assert np.array_equal(radio, RR.epoch_radio(N, ds.seed, e, B, 3, *rad.spans()))
    assert len(np.unique(radio[..., 0])) > 5
    mw = ds.max_window(len(SCALES))
    for s in range(len(tab)):
        step = tab.step(s)
        b = tab.pairs_in_step(s)
        assert step.radio.shape == (2 * b, 3, 2) and torch.equal(step.radio[:b], step.radio[b:]) and step.radio.is_contiguous()
        cpu = {k: getattr(step, k).cpu().numpy() for k in ("tile_id", "xy", "inner", "obj", "orient", "radio", "region")}
        for rows in (False, True):
            feed = PairFeed(ds.tiles, SCALES, b, mw, rows=rows, numerics="bf16")
            left, ld, right, rd, _ = feed.fill(step)
            feed.check()
            for i, t in enumerate(SCALES):
                ref, flagged = RR.gather(ds.host.tiles, cpu["tile_id"], cpu["xy"], cpu["inner"], cpu["obj"], cpu["orient"], cpu["radio"], i, t, mw[i])
                assert not flagged
                got = torch.cat((left[i].cols, right[i].cols), 0) if rows else torch.cat((left[i], right[i]), 0)
                assert torch.equal(bits(got.cpu()), bits(want_form(ref, "rows_bf16" if rows else "planar"))), (s, rows, t)
            want_d = np.stack([RR.designed_row(r, a, o, t, 3) for r, a, o, t in zip(cpu["region"], cpu["inner"], cpu["obj"], cpu["radio"])])
            assert np.array_equal(torch.cat((ld, rd), 0).cpu().numpy().reshape(2 * b, 19).view(np.uint32), want_d.view(np.uint32))


def test_replayed_steps_with_different_tables_equal_eager_steps():
    """The radiometric table is read by the gather, outside the captured step: the feed writes into the graph's inputs, and two
    replays whose tables differ equal the same steps run eagerly, bit for bit."""
    from deepmerge_amd.dataset import PairDataset
    from deepmerge_amd.feed import PairFeed, PairTable
    from deepmerge_amd.trainer import PairTrainer
    ds = PairDataset.from_arrays(_images(1), seed=5)
    B = 4
    base = ds.epoch(0, B).step(0)
    tables = []
    for k in range(4):                                                              # eager warm-up, the capturing step, two replays
        half = RR.pair_radio(np.arange(B) + 10 * k, 3, k, 3, *RR.MAX_SPANS)
        tables.append(PairTable(*(getattr(base, f).clone() for f in ("tile_id", "xy", "inner", "obj", "region", "flag")),
                                radio=up(np.concatenate((half, half)))))
    assert not torch.equal(tables[2].radio, tables[3].radio)
    mw = ds.max_window(len(SCALES))
    losses, weights = {}, {}
    for kind in ("graph", "eager"):
        tr = PairTrainer(_net(4), margin=1.0, lr=1e-3)
        if kind == "graph":
            tr.enable_graph(warmup=1)
        feed = PairFeed(ds.tiles, SCALES, B, mw, numerics="bf16", trainer=tr if kind == "graph" else None)
        losses[kind] = [float(tr.step(*feed.fill(t))) for t in tables]
        feed.check()
        if kind == "graph":
            assert feed._bound and tr.graph_error is None
        weights[kind] = tr.fp.flat.clone()
    assert losses["graph"] == losses["eager"] and len(set(losses["graph"])) == 4
    assert torch.equal(weights["graph"], weights["eager"])


def _hand_loop(net, ds, batch, epochs, lr_init, milestones, augment, radiometric):
    from deepmerge_amd import Train_SMT
    from deepmerge_amd.feed import PairFeed
    from deepmerge_amd.trainer import PairTrainer
    tr = PairTrainer(net, margin=1.0, lr=lr_init, lamda=0.1, belta=0)
    mw = ds.max_window(len(SCALES))
    feeds, means = {}, []
    for e in range(epochs):
        lr = Train_SMT.epoch_lr(lr_init, e, milestones, 0.2)
        tab = ds.epoch(e, batch, augment=augment, radiometric=radiometric)
        total = torch.zeros((), dtype=torch.float32, device=DEV)
        for s in range(len(tab)):
            b = tab.pairs_in_step(s)
            if b not in feeds:
                feeds[b] = PairFeed(ds.tiles, SCALES, b, mw, numerics="bf16")
            total += tr.step(*feeds[b].fill(tab.step(s)), lr=lr)
        means.append(float(total) / len(tab))
        for f in feeds.values():
            f.check()
    return means, tr


def _train(ds, net, path, *resume, **kw):
    from deepmerge_amd import Train_SMT
    return Train_SMT.train(net, 1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0, *resume, dataset=ds, num_epochs=2, model_paras_path=str(path), **kw)


@pytest.fixture(scope="module")
def straight(tmp_path_factory):
    """train(radiometric=..., augment="d4"): 2 epochs of N = 10 pairs at train_bs = 4 (two replayed steps and an eager tail per epoch)
    on a tiny v3 net, a checkpoint after each epoch.  Run once; the tests below read it."""
    from deepmerge_amd import Train_SMT
    from deepmerge_amd.dataset import PairDataset
    path = tmp_path_factory.mktemp("straight")
    ds = PairDataset.from_arrays(_images(), seed=11)
    net = _net()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(Train_SMT, "checkpoint_due", lambda e: True)
        it, losses = _train(ds, net, path, augment="d4", radiometric=_radiometric())
    assert it == [0, 1] and all(np.isfinite(losses))
    return {"ds": ds, "losses": losses, "weights": [v.clone() for v in net.state_dict().values()], "path": str(path)}


def test_train_with_radiometric_equals_the_hand_written_loop(straight):
    net = _net()
    want, _ = _hand_loop(net, straight["ds"], 4, 2, 1e-3, (40, 80), "d4", _radiometric())
    assert straight["losses"] == want
    assert all(torch.equal(a, b) for a, b in zip(straight["weights"], net.state_dict().values()))


def test_train_with_radiometric_resumed_after_epoch_0_equals_the_uninterrupted_run(straight, tmp_path, monkeypatch):
    from deepmerge_amd import Train_SMT
    monkeypatch.setattr(Train_SMT, "checkpoint_due", lambda e: True)
    one = glob.glob(os.path.join(straight["path"], "*_1epochs.pth"))
    assert len(one) == 1
    it, resumed = _train(straight["ds"], _net(99), tmp_path, True, one[0], augment="d4", radiometric=(0.4, 0.2, 0.1))
    assert it == [1] and resumed == straight["losses"][1:]
    x = torch.load(glob.glob(os.path.join(straight["path"], "*_2epochs.pth"))[0], weights_only=False)
    y = torch.load(glob.glob(os.path.join(str(tmp_path), "*_2epochs.pth"))[0], weights_only=False)
    assert x["epoch"] == y["epoch"] == 1
    for k in x["net"]:
        assert torch.equal(x["net"][k], y["net"][k]), k
    ox, oy = x["optimizer"], y["optimizer"]
    assert ox["param_groups"] == oy["param_groups"] and sorted(ox["state"]) == sorted(oy["state"])
    for i in ox["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(ox["state"][i][k], oy["state"][i][k]), (i, k)


def test_train_with_radiometric_none_is_train_without_the_keyword(straight):
    ds = straight["ds"]
    net_c, net_d, net_e = _net(), _net(), _net()
    _, plain = _train(ds, net_c, "unused", augment="d4")
    _, none = _train(ds, net_d, "unused", augment="d4", radiometric=None)
    assert plain == none and all(torch.equal(a, b) for a, b in zip(net_c.state_dict().values(), net_d.state_dict().values()))
    assert plain != straight["losses"]                                             # and the jitter is not a no-op
    _, alone = _train(ds, net_e, "unused", radiometric=_radiometric())             # independent of augment=
    assert all(np.isfinite(alone)) and alone != plain and alone != straight["losses"]
