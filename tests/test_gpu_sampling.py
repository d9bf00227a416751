"""GPU: weighted pair sampling against tests/sampling_ref.py, bit for bit -- dm_pair_epoch_select, the three `_src` entry points,
PairDataset.epoch(weights=, draws=), PairDataset.pair_terms, and Train_SMT.train(balance=, mining=, draws=) against hand-written loops
and across a resume."""
import glob
import os

import numpy as np
import pytest
import torch

import augment_ref as A
import radiometric_ref as RR
import sampling_ref as S
import train_smt_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALES = [32, 64, 128]
SIZES = [1, 2, 255, 256, 257, 4099]
SEEDS = (3, 0x9E3779B97F4A7C15)
EPOCHS = (0, 1, 2 ** 31 - 1)

up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _draws(N):
    return sorted({1, N, 3 * N + 1})


def _weight_patterns(N, rng):
    """The patterns of tests/test_sampling_host.py at size N, and a total just below 2^62."""
    w = {"random": rng.integers(0, 50, N), "equal": np.full(N, 3), "huge": np.full(N, ((1 << 62) - 1) // N)}
    single = np.zeros(N, np.int64)
    single[N // 2] = 9
    w["a single non-zero"] = single
    if N >= 2:
        first, last, mid = (rng.integers(1, 50, N) for _ in range(3))
        first[:N // 2] = 0
        last[(N + 1) // 2:] = 0
        mid[N // 4:N // 4 + N // 2] = 0
        w.update({"zeros first": first, "zeros last": last, "a run in the middle": mid})
        w["huge"] = np.asarray([(1 << 61) - 1] * 2 + [0] * (N - 2)) if N <= 4 else w["huge"]
    w["random"][0] = max(1, w["random"][0])
    return {k: np.asarray(v, np.int64) for k, v in w.items()}


# ---- 1. the select ------------------------------------------------------------------------------------------------------------------
def _select(w, M, seed, epoch):
    from deepmerge_amd import ops
    out = torch.full((M,), -7, dtype=torch.int32, device=DEV)
    ops.pair_epoch_select(torch.cumsum(up(w), 0), seed, epoch, out)
    return out.cpu().numpy()


@pytest.mark.parametrize("N", SIZES)
def test_select_matches_the_spec_bit_for_bit(N):
    rng = np.random.default_rng(N)
    for name, w in _weight_patterns(N, rng).items():
        assert int(w.sum()) < 1 << 62
        for M in _draws(N):
            # every seed and epoch on two patterns, one pairing each on the rest
            keys = [(s, e) for s in SEEDS for e in EPOCHS] if name in ("random", "huge") else [(SEEDS[0], 1), (SEEDS[1], EPOCHS[2])]
            for seed, epoch in keys:
                got = _select(w, M, seed, epoch)
                assert got.dtype == np.int32 and np.array_equal(got, S.select(w, M, seed, epoch)), (name, M, seed, epoch)
                assert (w[got] > 0).all()


def test_select_depends_on_seed_epoch_and_weights_only():
    w = np.random.default_rng(0).integers(1, 9, 257)
    a = _select(w, 772, 3, 0)
    assert not np.array_equal(a, _select(w, 772, 3, 1)) and not np.array_equal(a, _select(w, 772, 4, 0))
    assert np.array_equal(a[:100], _select(w, 100, 3, 0))            # position j does not depend on how many are drawn


# ---- 2. the three _src entry points -------------------------------------------------------------------------------------------------
def _draw_inputs(rng, N):
    """Polygons of 1 or 9 points (every point in exactly one polygon, ids shuffled), N distinct pairs, random flags."""
    n_poly = max(4, int(np.sqrt(2 * N)) + 2)
    counts = np.where(rng.random(n_poly) < 0.5, 1, 9)
    n_pts = int(counts.sum())
    poly_off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    poly_pts = rng.permutation(n_pts).astype(np.int32)
    flat = rng.choice(n_poly * n_poly, size=N, replace=False)
    pairs = np.stack((flat // n_poly, flat % n_poly), 1).astype(np.int32)
    pts = {"tile": rng.integers(0, 5, n_pts).astype(np.int32), "xy": rng.integers(0, 4000, (n_pts, 2)).astype(np.int32),
           "inner": rng.integers(1, 50, n_pts).astype(np.int32), "obj": rng.integers(50, 100, n_pts).astype(np.int32),
           "region": rng.standard_normal((n_pts, 15)).astype(np.float32)}
    return pairs, rng.integers(0, 2, N).astype(np.int32), poly_off, poly_pts, pts


def _kernel_table(inputs, seed, epoch, batch, src=None):
    """dm_pair_epoch_draw (src None) or dm_pair_epoch_draw_src into poisoned outputs."""
    from deepmerge_amd import ops
    pairs, flag, poly_off, poly_pts, pts = inputs
    M = len(pairs) if src is None else len(src)
    i32 = lambda *s: torch.full(s, 7, dtype=torch.int32, device=DEV)
    out = {"tile_id": i32(2 * M), "xy": i32(2 * M, 2), "inner": i32(2 * M), "obj": i32(2 * M), "region": torch.full((2 * M, 15), 7.0, device=DEV),
           "flag": torch.full((M,), 7.0, device=DEV), "point_id": i32(2 * M)}
    ops.pair_epoch_draw(up(pairs), up(flag), up(poly_off), up(poly_pts), up(pts["tile"]), up(pts["xy"]), up(pts["inner"]), up(pts["obj"]),
                        up(pts["region"]), seed, epoch, batch, out["tile_id"], out["xy"], out["inner"], out["obj"], out["region"], out["flag"],
                        point_id=out["point_id"], src=None if src is None else up(np.asarray(src, np.int32)))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_tables_equal(got, want, where):
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, where)
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (k, where)


@pytest.mark.parametrize("N", SIZES)
def test_draw_src_matches_the_spec_bit_for_bit(N):
    rng = np.random.default_rng(100 + N)
    inputs = _draw_inputs(rng, N)
    pairs, flag, poly_off, poly_pts, pts = inputs
    w = rng.integers(0, 5, N)
    w[rng.integers(0, N)] = 3
    for M in _draws(N):
        for k, (seed, epoch) in enumerate(((SEEDS[0], 0), (SEEDS[1], 1), (SEEDS[1], EPOCHS[2]))):
            src = S.select(w, M, seed, epoch)
            for batch in sorted({1, 7, M}):
                got = _kernel_table(inputs, seed, epoch, batch, src)
                _assert_tables_equal(got, S.draw_table(pts, pairs, flag, poly_off, poly_pts, src, seed, epoch, batch), (M, seed, epoch, batch))
                # the blocked layout at a ragged last step, and flag[j] == pair_flag[src[j]]
                rl, rr = S.blocked_rows(M, batch)
                assert np.array_equal(np.sort(np.concatenate((rl, rr))), np.arange(2 * M))
                last = (M - 1) // batch
                assert rr[-1] == 2 * M - 1 and rl[-1] == 2 * last * batch + (M - last * batch) - 1
                assert np.array_equal(got["flag"], flag[src].astype(np.float32))
                owner = np.repeat(np.arange(len(poly_off) - 1), np.diff(poly_off))[np.argsort(poly_pts)]
                assert np.array_equal(owner[got["point_id"][rl]], pairs[src, 0]) and np.array_equal(owner[got["point_id"][rr]], pairs[src, 1])


@pytest.mark.parametrize("N", SIZES)
def test_orient_src_and_radiometric_src_match_the_spec_bit_for_bit(N):
    from deepmerge_amd import ops
    for M in _draws(N):
        for k, (seed, epoch) in enumerate(((SEEDS[0], 0), (SEEDS[1], 1), (SEEDS[1], EPOCHS[2]))):
            for batch in sorted({1, 7, M}):
                for mask in (3, 7):
                    out = torch.full((2 * M,), -1, dtype=torch.int32, device=DEV)
                    ops.pair_epoch_orient(seed, epoch, M, batch, mask, out, by_position=True)
                    assert np.array_equal(out.cpu().numpy(), S.epoch_orient(M, seed, epoch, batch, mask)), (M, seed, epoch, batch, mask)
                bands = (1, 3, 5)[k]
                spans = (RR.spans(), RR.MAX_SPANS, (0, 0, 0))[k]
                out = torch.full((2 * M, bands, 2), -1, dtype=torch.int32, device=DEV)
                ops.pair_epoch_radiometric(seed, epoch, M, batch, bands, *spans, out, by_position=True)
                assert np.array_equal(out.cpu().numpy(), S.epoch_radio(M, seed, epoch, batch, bands, *spans)), (M, seed, epoch, batch, bands)
    if N >= 255:                                                       # another stream than the unsampled epoch's, at every band count
        for bands in (1, 3, 5):
            a, b = (torch.empty((2 * N, bands, 2), dtype=torch.int32, device=DEV) for _ in range(2))
            ops.pair_epoch_radiometric(3, 0, N, 7, bands, *RR.spans(), a, by_position=True)
            ops.pair_epoch_radiometric(3, 0, N, 7, bands, *RR.spans(), b)
            assert np.array_equal(a.cpu().numpy(), S.epoch_radio(N, 3, 0, 7, bands, *RR.spans())) and not torch.equal(a, b)


def test_a_pair_drawn_twice_gets_different_streams_at_its_positions():
    """Two pairs of 9-point polygons, seven draws: a pair is drawn at least three times.  The seed is the first at which the spec
    gives its first two positions different point ids on both sides; the kernels agree, and orientation and table differ too."""
    from deepmerge_amd import ops
    poly_off, poly_pts = np.asarray([0, 9, 18, 27], np.int32), np.arange(27, dtype=np.int32)
    pairs, flag = np.asarray([[0, 1], [1, 2]], np.int32), np.asarray([1, 0], np.int32)
    rng = np.random.default_rng(0)
    pts = {"tile": np.zeros(27, np.int32), "xy": rng.integers(0, 99, (27, 2)).astype(np.int32), "inner": np.full(27, 8, np.int32),
           "obj": np.full(27, 16, np.int32), "region": rng.random((27, 15), dtype=np.float32)}
    M, batch, w = 7, 3, np.asarray([1, 1])
    rl, rr = S.blocked_rows(M, batch)
    for seed in range(256):
        src = S.select(w, M, seed, 0)
        same = np.nonzero(src == src[0])[0]
        if len(same) < 2:
            continue
        j1, j2 = same[:2]
        want = S.draw_table(pts, pairs, flag, poly_off, poly_pts, src, seed, 0, batch)
        want_o, want_r = S.epoch_orient(M, seed, 0, batch, 7), S.epoch_radio(M, seed, 0, batch, 3, *RR.spans())
        pid = want["point_id"]
        if (pid[rl[j1]] != pid[rl[j2]] and pid[rr[j1]] != pid[rr[j2]] and want_o[rl[j1]] != want_o[rl[j2]]
                and not np.array_equal(want_r[rl[j1]], want_r[rl[j2]])):
            break
    else:
        raise AssertionError("no seed below 256 separates the two positions in the spec")
    got = _kernel_table((pairs, flag, poly_off, poly_pts, pts), seed, 0, batch, src)
    _assert_tables_equal(got, want, seed)
    assert got["point_id"][rl[j1]] != got["point_id"][rl[j2]] and got["point_id"][rr[j1]] != got["point_id"][rr[j2]]
    # keyed by the pair these would be equal: the unsampled streams are a function of (seed, epoch, pair)
    radio = torch.empty((2 * M, 3, 2), dtype=torch.int32, device=DEV)
    ops.pair_epoch_radiometric(seed, 0, M, batch, 3, *RR.spans(), radio, by_position=True)
    radio = radio.cpu().numpy()
    assert np.array_equal(radio, want_r)
    assert not np.array_equal(radio[rl[j1]], radio[rl[j2]]) and np.array_equal(radio[rl[j1]], radio[rr[j1]])
    orient = torch.empty((2 * M,), dtype=torch.int32, device=DEV)
    ops.pair_epoch_orient(seed, 0, M, batch, 7, orient, by_position=True)
    orient = orient.cpu().numpy()
    assert np.array_equal(orient, want_o) and orient[rl[j1]] != orient[rl[j2]] and orient[rl[j1]] == orient[rr[j1]]


@pytest.mark.parametrize("N", [2, 257])
def test_src_out_of_range_yields_the_minus_one_rows(N):
    rng = np.random.default_rng(N)
    inputs = _draw_inputs(rng, N)
    pairs, flag, poly_off, poly_pts, pts = inputs
    src = rng.integers(0, N, 3 * N + 1).astype(np.int32)
    bad = np.asarray([0, 2, len(src) - 1, 4])
    src[bad] = [-1, N, N, -(2 ** 31)]
    src[1] = 2 ** 31 - 1
    for batch in (1, 4, len(src)):
        got = _kernel_table(inputs, 5, 2, batch, src)
        _assert_tables_equal(got, S.draw_table(pts, pairs, flag, poly_off, poly_pts, src, 5, 2, batch), batch)
        rl, rr = S.blocked_rows(len(src), batch)
        for j in list(bad) + [1]:
            for row in (rl[j], rr[j]):
                assert got["point_id"][row] == -1 and got["tile_id"][row] == -1 and not got["region"][row].any() and not got["xy"][row].any()
            assert got["flag"][j] == 0
        assert (got["point_id"] >= 0).sum() == 2 * (len(src) - 5)


# ---- 3. src = perm: the whole list once; the unsampled entry points as before ---------------------------------------------------------
@pytest.mark.parametrize("N", [1, 10, 257, 4099])
def test_src_perm_draws_every_pair_once_and_the_unsampled_entry_points_are_unchanged(N):
    from deepmerge_amd import ops
    rng = np.random.default_rng(200 + N)
    inputs = _draw_inputs(rng, N)
    pairs, flag, poly_off, poly_pts, pts = inputs
    owner = np.repeat(np.arange(len(poly_off) - 1), np.diff(poly_off))[np.argsort(poly_pts)]
    pair_index = {(int(a), int(b)): k for k, (a, b) in enumerate(pairs)}
    for seed, epoch, batch in ((SEEDS[0], 0, 7), (SEEDS[1], 3, 4)):
        perm = R.epoch_perm(N, seed, epoch)
        got = _kernel_table(inputs, seed, epoch, batch, perm)
        rl, rr = S.blocked_rows(N, batch)
        ks = np.asarray([pair_index[(int(a), int(b))] for a, b in zip(owner[got["point_id"][rl]], owner[got["point_id"][rr]])])
        assert np.array_equal(ks, perm) and np.array_equal(np.sort(ks), np.arange(N))
        old = _kernel_table(inputs, seed, epoch, batch)
        assert np.array_equal(got["flag"], old["flag"]) and np.array_equal(got["flag"], flag[perm].astype(np.float32))
        if N >= 257:
            assert not np.array_equal(got["point_id"], old["point_id"])          # the stream word differs, and the key
        # the existing entry points on these inputs: their restatements, as before
        _assert_tables_equal(old, R.epoch_table(pts, pairs, flag, poly_off, poly_pts, seed, epoch, batch), (seed, epoch, batch))
        for mask in (3, 7):
            o = torch.empty((2 * N,), dtype=torch.int32, device=DEV)
            ops.pair_epoch_orient(seed, epoch, N, batch, mask, o)
            assert np.array_equal(o.cpu().numpy(), A.epoch_orient(N, seed, epoch, batch, mask))
        for bands in (1, 3, 5):
            t = torch.empty((2 * N, bands, 2), dtype=torch.int32, device=DEV)
            ops.pair_epoch_radiometric(seed, epoch, N, batch, bands, *RR.spans(), t)
            assert np.array_equal(t.cpu().numpy(), RR.epoch_radio(N, seed, epoch, batch, bands, *RR.spans()))


# ---- a small synthetic dataset: the one tests/test_gpu_train_smt.py trains on ----------------------------------------------------------
def _images(seed=0, n_pos=6, n_neg=4):
    rng = np.random.default_rng(seed)
    ims = []
    for i, (h, w) in enumerate(((150, 180), (210, 170))):
        n = 24
        xy = np.stack((rng.integers(0, w, n), rng.integers(0, h, n)), 1)
        inner = rng.integers(8, 30, n)
        ims.append({"tile": rng.integers(0, 256, size=(3, h, w), dtype=np.uint8), "xy": xy, "inner": inner,
                    "obj": inner + rng.integers(4, 40, n), "region": rng.random((n, 15), dtype=np.float32),
                    "polygon_points": [" ".join(str(q) for q in range(k, n, 8)) for k in range(8)]})
    ims[0]["positive"], ims[1]["positive"] = np.array([[0, 1], [2, 3], [4, 5]]), np.array([[1, 2], [3, 4], [6, 7]])[: n_pos - 3]
    ims[0]["negative"], ims[1]["negative"] = np.array([[0, 7], [5, 6]]), np.array([[0, 5], [2, 7]])[: n_neg - 2]
    return ims


def _net(seed=3):
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    torch.manual_seed(seed)
    return ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=list(SCALES), depth=[1, 1, 1], in_c=3, numerics="bf16").to(DEV)


def _host_points(ds):
    h = ds.host
    return {"tile": h.pt_tile, "xy": h.pt_xy, "inner": h.pt_inner, "obj": h.pt_obj, "region": h.pt_region}


def _spec_step(tab, s, batch, M, with_aug=False):
    """Step s of a spec table (numpy columns in the blocked layout) as a feed.PairTable on the device."""
    from deepmerge_amd.feed import PairTable
    b, lo = min(batch, M - s * batch), 2 * s * batch
    col = lambda k: up(tab[k][lo:lo + 2 * b])
    return PairTable(tile_id=col("tile_id"), xy=col("xy"), inner=col("inner"), obj=col("obj"), region=col("region"),
                     flag=up(tab["flag"][s * batch:s * batch + b]), orient=col("orient") if with_aug else None,
                     radio=col("radio") if with_aug else None)


@pytest.fixture(scope="module")
def ds():
    from deepmerge_amd.dataset import PairDataset
    return PairDataset.from_arrays(_images(), seed=11)


# ---- 4. PairDataset.epoch(weights=, draws=) ----------------------------------------------------------------------------------------------
def test_dataset_epoch_weighted_equals_the_spec_and_leaves_the_unweighted_table_alone(ds):
    h, N = ds.host, len(ds)
    cols = lambda t: {k: v.cpu().numpy().copy() for k, v in t.cols.items()}
    plain = cols(ds.epoch(2, 4, augment="d4", radiometric=(0.2, 0.1, 0.05)))
    w = np.asarray([0, 5, 1, 0, 0, 2, 7, 0, 1, 3], np.int64)
    for M, batch in ((N, 4), (23, 7), (3, 5), (23, 23)):
        table = ds.epoch(2, batch, weights=up(w), draws=None if M == N else M)
        assert (table.n_pairs, table.batch, len(table)) == (M, batch, -(-M // batch)) and "orient" not in table.cols and "radio" not in table.cols
        want = S.epoch_table(_host_points(ds), h.pairs, h.flag, h.poly_off, h.poly_pts, w, M, ds.seed, 2, batch)
        got = cols(table)
        assert sorted(got) == sorted(want)
        _assert_tables_equal(got, want, (M, batch))
        assert (w[got["src"]] > 0).all()
        last = table.step(len(table) - 1)
        assert last.xy.shape[0] == 2 * table.pairs_in_step(len(table) - 1) and last.flag.shape[0] == table.pairs_in_step(len(table) - 1)
    table = ds.epoch(2, 7, augment="flips", radiometric=(0.2, 0.1, 0.05), weights=up(w), draws=23)
    got = cols(table)
    assert np.array_equal(got["orient"], S.epoch_orient(23, ds.seed, 2, 7, 3))
    assert np.array_equal(got["radio"], S.epoch_radio(23, ds.seed, 2, 7, 3, *RR.spans()))
    assert table.step(3).orient.shape[0] == 4 and tuple(table.step(3).radio.shape) == (4, 3, 2)
    # the unweighted table of the earlier call was not touched, and drawing it again gives it bit for bit
    again = ds.epoch(2, 4, augment="d4", radiometric=(0.2, 0.1, 0.05))
    for k, v in plain.items():
        assert np.array_equal(again.cols[k].cpu().numpy().view(np.uint32), v.view(np.uint32)), k
    assert "src" not in again.cols and again.n_pairs == N
    _assert_tables_equal({k: plain[k] for k in ("point_id", "flag")},
                         {k: R.epoch_table(_host_points(ds), h.pairs, h.flag, h.poly_off, h.poly_pts, ds.seed, 2, 4)[k] for k in ("point_id", "flag")}, "plain")


def test_dataset_epoch_refuses_bad_weights(ds):
    w = lambda *v: torch.tensor(v + (0,) * (len(ds) - len(v)), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match=">= 0"):
        ds.epoch(0, 4, weights=w(3, -1))
    with pytest.raises(ValueError, match="every weight is 0"):
        ds.epoch(0, 4, weights=w())
    with pytest.raises(ValueError, match="2\\^62"):
        ds.epoch(0, 4, weights=w(1 << 61, 1 << 61))
    with pytest.raises(ValueError, match="overflow"):
        ds.epoch(0, 4, weights=w((1 << 63) - 1, (1 << 63) - 1, 2))
    with pytest.raises(ValueError, match="draws needs weights"):
        ds.epoch(0, 4, draws=5)
    with pytest.raises(ValueError, match="int64"):
        ds.epoch(0, 4, weights=torch.ones(len(ds), dtype=torch.int64))          # a host tensor
    assert ds.epoch(0, 4, weights=w((1 << 61) - 1, (1 << 61) - 1)).n_pairs == len(ds)   # the largest total


# ---- 5. pair_terms ---------------------------------------------------------------------------------------------------------------------
def test_pair_terms_are_in_pair_order_and_leave_the_training_table_untouched(ds):
    """Against hand-fed forwards of the spec's rows: one pair at a time (batch 1) for three chosen pairs, and the step that holds
    each of them at batch 4.  Same feed sizes on both sides, so the comparison is bit for bit."""
    from deepmerge_amd import ops
    from deepmerge_amd.feed import PairFeed
    h, N = ds.host, len(ds)
    net = _net(4).train()
    table = ds.epoch(1, 4, weights=up(np.arange(1, N + 1)), draws=13)
    before = {k: v.clone() for k, v in table.cols.items()}
    plain = ds.epoch(1, 4)
    plain_before = {k: v.clone() for k, v in plain.cols.items()}
    key, margin = 6, 1.0
    terms = {b: ds.pair_terms(net, b, margin, key) for b in (1, 4)}
    assert net.training and all(t.dtype == torch.float32 and tuple(t.shape) == (N,) for t in terms.values())
    for cols, was in ((table.cols, before), (plain.cols, plain_before)):
        assert all(torch.equal(cols[k], was[k]) for k in was)
    assert torch.equal(ds.pair_terms(net, 4, margin, key), terms[4])               # a function of (model, seed, key): no RNG
    assert not torch.equal(ds.pair_terms(net, 4, margin, key + 1), terms[4])        # other sample points
    net.eval()
    mw = ds.max_window(len(SCALES))
    for batch in (1, 4):
        tab = S.draw_table(_host_points(ds), h.pairs, h.flag, h.poly_off, h.poly_pts, np.arange(N), ds.seed, key, batch)
        got = terms[batch].cpu().numpy()
        for pair in (0, 5, 9):
            s = pair // batch
            b = min(batch, N - s * batch)
            feed = PairFeed(ds.tiles, SCALES, b, mw, numerics="bf16")
            with torch.no_grad():
                _, _, _, _, flag = feed.fill(_spec_step(tab, s, batch, N))
                F = net(feed.both, feed.dboth).contiguous()
                _, term = ops.contrastive_terms(F[:b], F[b:], flag, margin)
            feed.check()
            want = term.cpu().numpy()
            assert flag.cpu().numpy()[pair - s * batch] == h.flag[pair]
            assert np.array_equal(got[s * batch:s * batch + b].view(np.uint32), want.view(np.uint32)), (batch, pair)
    assert len(set(terms[1].cpu().numpy()[[0, 5, 9]].tolist())) == 3                # the three pairs are told apart


# ---- 6. train(balance=, mining=, draws=) ------------------------------------------------------------------------------------------------
def _hand_loop(net, ds, batch, epochs, lr_init, milestones, tables, margin=1.0, lamda=0.1, belta=0):
    """The composition train() promises, written out: per epoch `tables(e, net)` -> (list of PairTable, one per step), PairFeed,
    eager PairTrainer steps."""
    from deepmerge_amd import Train_SMT
    from deepmerge_amd.feed import PairFeed
    from deepmerge_amd.trainer import PairTrainer
    tr = PairTrainer(net, margin=margin, lr=lr_init, lamda=lamda, belta=belta)
    mw = ds.max_window(len(SCALES))
    feeds, means = {}, []
    for e in range(epochs):
        lr = Train_SMT.epoch_lr(lr_init, e, milestones, 0.2)
        steps = tables(e, net)
        total = torch.zeros((), dtype=torch.float32, device=DEV)
        for table in steps:
            b = table.flag.shape[0]
            if b not in feeds:
                feeds[b] = PairFeed(ds.tiles, SCALES, b, mw, numerics="bf16")
            total += tr.step(*feeds[b].fill(table), lr=lr)
        means.append(float(total) / len(steps))
        for f in feeds.values():
            f.check()
    return means, tr


def _balance_tables(ds, batch, share, M, augment=None, radiometric=None):
    from deepmerge_amd.dataset import balance_weights
    h = ds.host
    w = balance_weights(h.flag, share).numpy()

    def tables(e, net):
        tab = S.epoch_table(_host_points(ds), h.pairs, h.flag, h.poly_off, h.poly_pts, w, M, ds.seed, e, batch)
        if augment is not None:
            tab["orient"] = S.epoch_orient(M, ds.seed, e, batch, A.MASKS[augment])
            tab["radio"] = S.epoch_radio(M, ds.seed, e, batch, 3, *RR.spans(*radiometric))
        return [_spec_step(tab, s, batch, M, with_aug=augment is not None) for s in range(-(-M // batch))]
    return tables


def test_train_balance_equals_hand_loop_bit_for_bit(ds, tmp_path):
    """N = 10 pairs (6 positive, 4 negative), balance 0.5, train_bs = 4: two graph-replayed steps and an eager tail per epoch against
    eager steps over the spec's tables; then draws = 13 (three replays and a tail of one) with both augmentations."""
    from deepmerge_amd import Train_SMT
    net_a, net_b = _net(), _net()
    it, losses = Train_SMT.train(net_a, 1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0, dataset=ds, num_epochs=3, milestones=(1, 2), model_paras_path=str(tmp_path),
                                 balance=0.5)
    want, _ = _hand_loop(net_b, ds, 4, 3, 1e-3, (1, 2), _balance_tables(ds, 4, 0.5, len(ds)))
    assert it == [0, 1, 2] and all(np.isfinite(losses)) and losses == want
    for (k, a), (k2, b) in zip(net_a.state_dict().items(), net_b.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    net_a, net_b = _net(6), _net(6)
    _, losses = Train_SMT.train(net_a, 1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0, dataset=ds, num_epochs=2, model_paras_path=str(tmp_path), balance=0.25,
                                draws=13, augment="d4", radiometric=(0.2, 0.1, 0.05))
    want, _ = _hand_loop(net_b, ds, 4, 2, 1e-3, (40, 80), _balance_tables(ds, 4, 0.25, 13, "d4", (0.2, 0.1, 0.05)))
    assert losses == want
    assert all(torch.equal(a, b) for a, b in zip(net_a.state_dict().values(), net_b.state_dict().values()))


def _assert_checkpoints_equal(a, b):
    x = torch.load(glob.glob(os.path.join(str(a), "*_6epochs.pth"))[0], weights_only=False)
    y = torch.load(glob.glob(os.path.join(str(b), "*_6epochs.pth"))[0], weights_only=False)
    assert x["epoch"] == y["epoch"] == 5 and list(x.keys()) == ["net", "optimizer", "epoch", "time", "scales", "depth", "name"]
    for k in x["net"]:
        assert torch.equal(x["net"][k], y["net"][k]), k
    ox, oy = x["optimizer"], y["optimizer"]
    assert ox["param_groups"] == oy["param_groups"] and sorted(ox["state"]) == sorted(oy["state"])
    for i in ox["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(ox["state"][i][k], oy["state"][i][k]), (i, k)


def test_train_balance_resume_equals_uninterrupted(ds, tmp_path, monkeypatch):
    from deepmerge_amd import Train_SMT
    monkeypatch.setattr(Train_SMT, "checkpoint_due", lambda e: e in (4, 5))
    a, b = tmp_path / "straight", tmp_path / "resumed"
    kw = dict(dataset=ds, num_epochs=6, milestones=(2, 4), balance=0.5, draws=9)
    _, straight = Train_SMT.train(_net(), 1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0, model_paras_path=str(a), **kw)
    five = glob.glob(os.path.join(str(a), "*_5epochs.pth"))
    assert len(five) == 1
    it, resumed = Train_SMT.train(_net(99), 1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0, True, five[0], model_paras_path=str(b), **kw)
    assert it == [5] and resumed == straight[5:]
    _assert_checkpoints_equal(a, b)


def test_train_mining_equals_hand_loop_and_resumes_bit_for_bit(ds, tmp_path, monkeypatch):
    """Mining(every=5) over 6 epochs: refreshes at epochs 0 and 5.  The hand loop is pair_terms -> hardness_weights (times the balance
    weights) -> epoch on a second dataset object of the same pairs and seed; the run resumed from the epoch-5 checkpoint refreshes
    at its first epoch, which is a refresh epoch of the straight run."""
    from deepmerge_amd import Train_SMT, ops
    from deepmerge_amd.dataset import PairDataset, balance_weights, hardness_weights
    monkeypatch.setattr(Train_SMT, "checkpoint_due", lambda e: e in (4, 5))
    mining = ops.Mining(every=5, cap=0.5, floor_share=1 / 8)
    a, b = tmp_path / "straight", tmp_path / "resumed"
    kw = dict(dataset=ds, num_epochs=6, milestones=(2, 4), mining=mining, balance=0.5, val_batch=7)
    net_a = _net()
    _, straight = Train_SMT.train(net_a, 1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0, model_paras_path=str(a), **kw)
    other = PairDataset.from_arrays(_images(), seed=11)
    class_w = balance_weights(other.host.flag, 0.5).to(DEV)
    state = {}

    def tables(e, net):
        if e % 5 == 0:
            term = other.pair_terms(net, 7, 1.0, key=e)
            state["w"] = hardness_weights(term, 1 / 8, 0.5, class_weights=class_w)
            state.setdefault("seen", []).append(state["w"].cpu().numpy())
        t = other.epoch(e, 4, weights=state["w"])
        return [t.step(s) for s in range(len(t))]
    net_b = _net()
    want, _ = _hand_loop(net_b, other, 4, 6, 1e-3, (2, 4), tables)
    assert straight == want
    assert all(torch.equal(x, y) for x, y in zip(net_a.state_dict().values(), net_b.state_dict().values()))
    assert len(state["seen"]) == 2                                     # refreshed at epochs 0 and 5 only
    assert all(set((w // class_w.cpu().numpy()).tolist()) <= set(range(32, 257)) for w in state["seen"])
    five = glob.glob(os.path.join(str(a), "*_5epochs.pth"))
    it, resumed = Train_SMT.train(_net(99), 1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0, True, five[0], model_paras_path=str(b), **kw)
    assert it == [5] and resumed == straight[5:]
    _assert_checkpoints_equal(a, b)


def test_train_all_three_none_is_the_unsampled_run(ds, tmp_path):
    """balance = mining = draws = None: the sampled buffers are never allocated and the losses are those of the keyword-free call."""
    from deepmerge_amd import Train_SMT
    from deepmerge_amd.dataset import PairDataset
    fresh = PairDataset.from_arrays(_images(), seed=11)
    _, a = Train_SMT.train(_net(), 1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0, dataset=fresh, num_epochs=1, model_paras_path=str(tmp_path))
    _, b = Train_SMT.train(_net(), 1.0, 4, 1e-3, 0.0, 0.0, 0.1, 0, dataset=fresh, num_epochs=1, model_paras_path=str(tmp_path), balance=None,
                           mining=None, draws=None)
    assert a == b and fresh._sampled is None and fresh._terms is None
