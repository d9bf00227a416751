"""GPU: the LayerNorm row kernels and the relpos chunk sum with their loads in flight ahead of the arithmetic (csrc/dm_rows.hip).

layernorm_fwd_kernel / layernorm_bwd_kernel request a wave's next row before the reductions of the current one, and chunk_sum_kernel
requests a batch of chunks before it adds them.  None of that may change a bit: a row's results must not depend on which rows the same
wave handled before or after it, nothing may be read or written past the last row, and the chunks must still be added in chunk order.

  * Row independence, bitwise: y / mean / rstd (forward) and dx with its bf16 copy or plane pair (backward) of a row computed inside
    R rows equal the same row submitted alone (rows = 1), for the first row, the last row and the rows on either side of every
    boundary between two iterations of a wave's row loop.  A wave's rows are r, r + W, r + 2 W, ... with W = 4 x the grid: 3072 in
    the backward (768 workgroups), 8192 in the forward (2048), so the row counts below give waves 0, 1, 2 and 3 rows (backward: 1, 5,
    3072, 3073, 6145, 9217; forward: 8192, 8193, 16385, 24577 -- 1, 2, 3 and 4 rows) and exercise the first and the last iteration
    of the pipeline with and without a row behind them.
  * At the same row counts everything, dgamma / dbeta included, stays inside the bounds of tests/rows_ref.py against float64.
  * Every output buffer is 8 rows longer than the kernel may write and filled with a sentinel: the tail is bit-unchanged afterwards.
  * Widths 4, 260, 768, 1024: a single partly filled chunk, a partly filled second chunk, the encoder's width (its own instance, no
    lane predicate) and the widest register-resident row.  Options: dres on / off, dy in bf16 / fp32, dx alone / with the bf16 copy /
    with the plane pair; y in fp32 / bf16 / as the plane pair.
  * Chunk sum: relpos_bias_scatter on a slab of 1, 2, 3, 6, 8, 9, 10, 17 chunks (every batch size of the kernel: 8, 4, 2, 1 and their
    sums) gives, bit for bit, the dtable of the same slab summed in fp32 in chunk order beforehand and passed as one chunk.

Tolerances and inputs are those of tests/rows_ref.py (no constants of its own).  Every check prints its worst err / tol (run with -s).
"""
import ctypes as C

import pytest
import torch

import bn_relpos_ref as RP
import rows_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
SENTINEL = -13.0                      # exact in fp32 and bf16
PAD_ROWS = 8
BWD_WAVES, FWD_WAVES = 4 * 768, 4 * 2048
BWD_ROWS = (1, 5, 3072, 3073, 6145, 9217)
FWD_ROWS = (8192, 8193, 16385, 24577)
COLS = (4, 260, 768, 1024)


def _L():
    from deepmerge_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _within(name, got, want, tol):
    err = (got.detach().double().cpu() - want.double()).abs()
    r = R.worst(err, tol)
    print(f"  [rows_inflight] {name:<60s} err/tol = {r:.3f}")
    assert r <= 1.0, f"{name}: {r:.3f} of the bound (worst error {float(err.max()) / R.U:.1f} U)"


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _padded(n_live, n_pad, dtype):
    return torch.full((n_live + n_pad,), SENTINEL, dtype=dtype, device=DEV)


def _tail_untouched(name, buf, n_live):
    live, tail = buf[:n_live], buf[n_live:]
    assert bool((tail == SENTINEL).all()), f"{name}: written past the end"
    assert bool(torch.isfinite(live.float()).all()), f"{name}: non-finite output"
    return live


def _boundary_rows(rows, waves):
    """First row, last row and both sides of every boundary between two iterations of a wave's row loop."""
    w = min(waves, 4 * ((rows + 3) // 4))
    pick = {0, rows - 1}
    for k in range(w, rows, w):
        pick.update((k - 1, k))
    return sorted(pick)


# =====================================================================================================================================
# forward
# =====================================================================================================================================
def _fwd(x, gamma, beta, mode):
    """mode: 'f32' | 'bf16' | 'pair' -> (y [rows, cols] or planes [2, rows, cols], mean, rstd); padded buffers, tails checked."""
    L = _L()
    rows, cols = x.shape
    pair = mode == "pair"
    dtype = F32 if mode == "f32" else BF16
    n_y = (2 if pair else 1) * rows * cols
    y, mean, rstd = _padded(n_y, PAD_ROWS * cols, dtype), _padded(rows, PAD_ROWS, F32), _padded(rows, PAD_ROWS, F32)
    code = L.DM_BF16_PAIR if pair else (L.DM_F32 if mode == "f32" else L.DM_BF16)
    L.check(L.lib().dm_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), code, mean.data_ptr(), rstd.data_ptr(),
                                     rows, cols, R.LN_EPS, _stream()), "dm_layernorm_fwd")
    y = _tail_untouched(f"y({mode})", y, n_y).view((2, rows, cols) if pair else (rows, cols))
    return y, _tail_untouched("mean", mean, rows), _tail_untouched("rstd", rstd, rows)


def _planes(x):
    hi = x.bfloat16()
    return torch.stack([hi, (x - hi.float()).bfloat16()])


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", FWD_ROWS)
def test_layernorm_fwd_rows_in_flight(rows, cols):
    d = R.ln_inputs(rows, cols)
    x, g, b = d["x"].to(DEV), d["gamma"].to(DEV), d["beta"].to(DEV)
    y64, mean64, rstd64, xhat64 = R.layernorm_ref(d["x"], d["gamma"], d["beta"])
    t = dict(y=y64, mean=mean64, rstd=rstd64, xhat=xhat64)
    name = f"ln fwd {rows}x{cols}"
    out = {mode: _fwd(x, g, b, mode) for mode in ("f32", "bf16", "pair")}
    y32, mean, rstd = out["f32"]
    _within(f"{name} y", y32, t["y"], R.ln_y_tol(d["x"], d["gamma"], t))
    _within(f"{name} y(bf16)", out["bf16"][0], t["y"], R.ln_y_tol(d["x"], d["gamma"], t, bf16=True))
    _within(f"{name} mean", mean, t["mean"], R.ln_mean_tol(d["x"]))
    _within(f"{name} rstd", rstd, t["rstd"], R.ln_rstd_tol(d["x"], t))
    assert _same_bits(out["pair"][0], _planes(y32)), f"{name}: plane pair != split of the fp32 rows"
    for mode in ("bf16", "pair"):
        assert _same_bits(out[mode][1], mean) and _same_bits(out[mode][2], rstd), f"{name}: statistics differ in mode {mode}"
    for r in _boundary_rows(rows, FWD_WAVES):
        for mode in ("f32", "bf16", "pair"):
            y1, m1, s1 = _fwd(x[r:r + 1], g, b, mode)
            yr = out[mode][0][:, r:r + 1] if mode == "pair" else out[mode][0][r:r + 1]
            assert _same_bits(y1, yr), f"{name}: row {r} ({mode}) differs from the same row alone"
            assert _same_bits(m1, mean[r:r + 1]) and _same_bits(s1, rstd[r:r + 1]), f"{name}: statistics of row {r} ({mode}) differ"


# =====================================================================================================================================
# backward
# =====================================================================================================================================
def _bwd(dy, x, gamma, mean, rstd, dres, lp):
    """lp: None | 'copy' | 'pair' -> (dx, dx_lp or None, dgamma, dbeta); padded buffers, tails checked.  The partial rows go through
    dm_partial_reduce_batch as in ops.layernorm_bwd."""
    L = _L()
    lib = L.lib()
    rows, cols = x.shape
    dx = _padded(rows * cols, PAD_ROWS * cols, F32)
    n_lp = 0 if lp is None else (2 if lp == "pair" else 1) * rows * cols
    dx_lp = _padded(n_lp, PAD_ROWS * cols, BF16) if lp else None
    n_part_max = lib.dm_layernorm_bwd_partial_floats(cols)
    part = _padded(n_part_max, PAD_ROWS * 2 * cols, F32)
    n_part = C.c_int32(0)
    fn = lib.dm_layernorm_bwd_partials_pair if lp == "pair" else lib.dm_layernorm_bwd_partials
    L.check(fn(dy.data_ptr(), L.DM_BF16 if dy.dtype == BF16 else L.DM_F32, x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
               None if dres is None else dres.data_ptr(), dx.data_ptr(), None if dx_lp is None else dx_lp.data_ptr(), part.data_ptr(),
               rows, cols, C.byref(n_part), _stream()), "dm_layernorm_bwd_partials")
    assert n_part.value == min(768, (rows + 3) // 4)
    _tail_untouched("partial rows", part, n_part.value * 2 * cols)
    dgamma, dbeta = torch.full((cols,), float("nan"), device=DEV), torch.full((cols,), float("nan"), device=DEV)
    item = (L.DmReduceItem * 1)()
    item[0].partial, item[0].out0, item[0].out1 = part.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr()
    item[0].nrows, item[0].width, item[0].split, item[0].accumulate = n_part.value, 2 * cols, cols, 0
    L.check(lib.dm_partial_reduce_batch(item, 1, _stream()), "dm_partial_reduce_batch")
    dx = _tail_untouched("dx", dx, rows * cols).view(rows, cols)
    if lp:
        dx_lp = _tail_untouched(f"dx {lp}", dx_lp, n_lp).view((2, rows, cols) if lp == "pair" else (rows, cols))
    return dx, dx_lp, dgamma, dbeta


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", BWD_ROWS)
def test_layernorm_bwd_rows_in_flight(rows, cols):
    d = R.ln_inputs(rows, cols)
    x, g, b = d["x"].to(DEV), d["gamma"].to(DEV), d["beta"].to(DEV)
    _, mean, rstd = _fwd(x, g, b, "f32")
    dres_dev = d["dres"].to(DEV)
    picks = _boundary_rows(rows, BWD_WAVES)
    for dy_bf16 in (False, True):
        t = R.ln_truth(rows, cols, dy_bf16)
        dy = t["dy"].to(DEV).to(BF16 if dy_bf16 else F32)
        tg, tb = R.ln_dgb_tol(t)
        for with_dres in (True, False):
            dres = dres_dev if with_dres else None
            name = f"ln bwd {rows}x{cols} dy={'bf16' if dy_bf16 else 'f32'} dres={int(with_dres)}"
            dx, _, dgam, dbet = _bwd(dy, x, g, mean, rstd, dres, None)
            _within(f"{name} dx", dx, t["dx"] + (d["dres"].double() if with_dres else 0),
                    R.ln_dx_tol(d["x"], d["gamma"], t, d["dres"] if with_dres else None))
            _within(f"{name} dgamma", dgam, t["dgamma"], tg)
            _within(f"{name} dbeta", dbet, t["dbeta"], tb)
            for lp in ("copy", "pair"):                  # the same dx and sums bit for bit, and the copy / pair is the rounding / split of dx
                dx2, low, dgam2, dbet2 = _bwd(dy, x, g, mean, rstd, dres, lp)
                assert _same_bits(dx2, dx) and _same_bits(dgam2, dgam) and _same_bits(dbet2, dbet), f"{name}: results change with lp={lp}"
                assert _same_bits(low, dx.bfloat16() if lp == "copy" else _planes(dx)), f"{name}: {lp} is not the rounding / split of dx"
            for r in picks:
                sl = slice(r, r + 1)
                for lp in (None, "copy", "pair"):
                    dx1, low1, _, _ = _bwd(dy[sl], x[sl], g, mean[sl], rstd[sl], None if dres is None else dres[sl], lp)
                    assert _same_bits(dx1, dx[sl]), f"{name}: dx of row {r} (lp={lp}) differs from the same row alone"
                    if lp == "copy":
                        assert _same_bits(low1, dx[sl].bfloat16()), f"{name}: bf16 copy of row {r} differs from the same row alone"
                    elif lp == "pair":
                        assert _same_bits(low1, _planes(dx[sl])), f"{name}: plane pair of row {r} differs from the same row alone"


# =====================================================================================================================================
# chunk sum
# =====================================================================================================================================
@pytest.mark.parametrize("chunks", (1, 2, 3, 6, 8, 9, 10, 17))
def test_chunk_sum_adds_in_chunk_order(chunks):
    """N = 72, H = 4: 5184 float4 positions, 21 workgroups, the last one partly filled."""
    _chunk_case(72, 4, chunks)


def test_chunk_sum_past_the_grid_cap():
    """N = 256, H = 36: 589824 float4 positions, more than the 2048 x 256 threads of the capped grid -- some threads take two."""
    _chunk_case(256, 36, 3)


def _chunk_case(N, H, chunks):
    from deepmerge_amd import ops
    assert RP.rp_chunk_sum_path(chunks, H, N) or chunks == 1
    nb = RP.rp_bins(N)
    csr = ops.relpos_index_csr(RP.rp_index(N, nb).to(DEV), nb)
    slab = RP.rp_slab(chunks, H, N, integer=False)
    pre = slab[0].clone()
    for c in range(1, chunks):
        pre = pre + slab[c]                                # fp32, chunk order: chunk_sum_kernel's arithmetic
    got, want = (torch.full((nb, H), float("nan"), device=DEV) for _ in range(2))
    ops.relpos_bias_scatter(slab.to(DEV).clone(), got, 1, H, (chunks, N, csr), nb)
    ops.relpos_bias_scatter(pre[None].to(DEV).clone(), want, 1, H, (1, N, csr), nb)
    assert bool(torch.isfinite(got).all())
    assert _same_bits(got, want), f"N={N} H={H} chunks={chunks}: dtable differs from that of the pre-summed slab"
