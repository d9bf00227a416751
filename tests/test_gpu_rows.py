"""GPU: the HBM-bound row / element kernels (csrc/dm_rows.hip, dm_rows_wide.hip, dm_gru.hip) at every output, width class and edge,
against the float64 restatements of tests/rows_ref.py.

Exact results (pooling on grid data, integer column sums, casts, plane pairs, the device-scalar Adam against the host-scalar one)
are compared bit for bit.  Everything else is compared inside a bound derived from the fp32 rounding model (U = 2^-24); the integer
constant in front of each bound is the smallest one for which a float32 restatement of the kernel's arithmetic stays at or below
half the bound on exactly these inputs (tests/test_rows_host.py asserts that on the CPU), so a correct kernel has a factor 2 to spare.

  constant    bound (derivation in rows_ref.py)                                                      worst err/tol  CPU     GPU (MI355X)
  C_LN_Y  7   U (max|x-mean| rstd |gamma| (1 + |mean| rstd) + |y|): the mean's error, rel. U per op   y             0.466   0.357
  C_BF16  2   bf16 output: + 2^-8 (|y| + tol), one rounding to 8 bits                                 y (bf16)      0.498   0.498
  C_LN_MEAN 4 U max|x|: tree sum around an offset                                                     mean          0.490   0.490
  C_LN_RSTD 6 rstd (U + (tol_mean rstd)^2 / 2): squares, sum, division, root; mean enters squared     rstd          0.433   0.378
  C_LN_DX 5   U (rstd G X (X + |mean| rstd) + |dres| + |dx|), G = max|dy gamma|, X = max(1, |xhat|)   dx            0.409   0.400
  C_LN_DG 3   U (1 + log2 rows) sum_r |dy| (|xhat| + |mean| rstd) [+ U |result| when accumulating]    dgamma/dbeta  0.466   0.466
  C_COLSUM 1  M U sum|x| per column (the issue's bound) [+ 2 U |result| when accumulating]            colsum        0.099   0.099 (0.477 accumulating, as on the CPU)
  C_ADAM_M 3  U k sum_j |b1^j (1-b1) g_j| after k steps                                               m             0.461   0.366
  C_ADAM_V 6  U k v                                                                                   v             0.418   0.424
  C_ADAM_P 6  U (max|p| + sum_t t |update_t|), |m| replaced by the sum of its terms' magnitudes       p             0.475   0.487
  C_CL_LOSS 1 U (1 + log2 D) mean(d + margin)                                                         loss          0.120   0.120
  C_CL_GRAD 3 U |grad| (a - b exact on the 2^-10 grid; coefficient and product rounded)               da, db        0.469   0.469
  C_CE_LOSS 1 U (1 + log2 K) mean_r sum_c q (|lse| + |x| + 1)                                         loss          0.110   0.127
  C_CE_GRAD 5 U upstream/B (softmax psum (1 + log2 K + |x| + |lse|) + q)                              dlogits       0.442   0.442
  C_GRU_FWD 4 U (1 + (1 - n^2)(|gi_n| + |r gh_n| + |gh_n|) + |h|); floor 4 U (fast exponential)       h'            0.381   0.381
  C_GRU_BWD 3 U |dh| (1 + |h|) (1 + |gh_n|) (1 + (1 - n^2)(|gi_n| + |r gh_n| + |gh_n|))               dgi, dgh, dh  0.359   0.359
  (one-pass variance, deliberately wrong, on the mu = 1e3 rows: y at 150 .. 264 times the bound, rstd at > 1e5 times)

Every check prints its worst err / tol ("[rows_gpu] ..."; run with -s).
"""
import numpy as np
import pytest
import torch

import rows_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16


def _ops():
    from deepmerge_amd import ops
    return ops


def _lib():
    from deepmerge_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _within(name, got, want, tol):
    """|got - want| <= tol everywhere; prints the worst ratio and, on failure, the worst error in units of U = 2^-24."""
    err = (got.detach().double().cpu() - want.double()).abs()
    r = R.worst(err, tol)
    print(f"  [rows_gpu] {name:<52s} err/tol = {r:.3f}")
    assert r <= 1.0, f"{name}: {r:.3f} of the bound (worst error {float(err.max()) / R.U:.1f} U)"


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _planes_on_device(x):
    hi = x.bfloat16()
    return torch.stack([hi, (x - hi.float()).bfloat16()])


# =====================================================================================================================================
# LayerNorm
# =====================================================================================================================================
def _ln_run(rows, cols, tag, out_dtype=F32, dres=True, accumulate=True, dy_bf16=False):
    ops = _ops()
    d, t = R.ln_inputs(rows, cols), R.ln_truth(rows, cols, dy_bf16)
    x, g, b = d["x"].to(DEV), d["gamma"].to(DEV), d["beta"].to(DEV)
    name = f"ln {tag} {rows}x{cols}"
    y, mean, rstd = ops.layernorm_fwd(x, g, b, R.LN_EPS, out_dtype)
    assert y.dtype == out_dtype
    _within(f"{name} y{'(bf16)' if out_dtype == BF16 else ''}", y, t["y"], R.ln_y_tol(d["x"], d["gamma"], t, bf16=out_dtype == BF16))
    _within(f"{name} mean", mean, t["mean"], R.ln_mean_tol(d["x"]))
    _within(f"{name} rstd", rstd, t["rstd"], R.ln_rstd_tol(d["x"], t))
    c = d["const_rows"]
    if bool(c.any()):                                       # variance 0: rstd = eps^-1/2 to 2 ulp (y == beta is inside the bound above)
        want = 1.0 / np.sqrt(np.float64(np.float32(R.LN_EPS)))
        assert float((rstd.cpu()[c].double() - want).abs().max()) <= 2 * float(np.spacing(np.float32(want)))
    dy = t["dy"].to(DEV).to(BF16 if dy_bf16 else F32)
    dr = d["dres"].to(DEV) if dres else None
    fill = d["g0"] if accumulate else torch.full((cols,), float("nan"))
    dgam, dbet = fill.clone().to(DEV), fill.clone().to(DEV)
    dx, dg_out, db_out = ops.layernorm_bwd(dy, x, g, mean, rstd, dres=dr, dgamma=dgam, dbeta=dbet, accumulate=accumulate)
    assert dg_out is dgam and db_out is dbet and bool(torch.isfinite(dx).all())
    g0 = d["g0"] if accumulate else None
    tg, tb = R.ln_dgb_tol(t, g0)
    _within(f"{name} dx", dx, t["dx"] + (d["dres"].double() if dres else 0), R.ln_dx_tol(d["x"], d["gamma"], t, d["dres"] if dres else None))
    _within(f"{name} dgamma", dgam, t["dgamma"] + (g0.double() if accumulate else 0), tg)
    _within(f"{name} dbeta", dbet, t["dbeta"] + (g0.double() if accumulate else 0), tb)


@pytest.mark.parametrize("cols", R.LN_WIDTHS)
def test_layernorm_widths(cols):
    """Each edge of a width class (CH = 3 up to 768, CH = 4 up to 1024, streamed beyond), with a partially filled last chunk group;
    every row family in one launch; y, mean, rstd, dx, dgamma, dbeta against float64."""
    for rows in R.LN_ROWS:
        _ln_run(rows, cols, "width")


@pytest.mark.parametrize("rows,cols", R.LN_CAP_CASES)
def test_layernorm_rows_past_the_grid_caps(rows, cols):
    """One row more than the backward grid (4 * 768), the forward grid (4 * 2048) and the streamed kernels' grid (4 * 4096) cover:
    the grid-stride loops take a second trip for some waves only."""
    _ln_run(rows, cols, "cap")


@pytest.mark.parametrize("cols", R.LN_OPTION_WIDTHS)
def test_layernorm_options(cols):
    """dres given / None x accumulate x dy dtype x output dtype."""
    for dy_bf16 in (False, True):
        for out_dtype in (F32, BF16):
            for dres in (True, False):
                for accumulate in (True, False):
                    _ln_run(67, cols, f"opt dres={int(dres)} acc={int(accumulate)} dy={'bf16' if dy_bf16 else 'f32'}", out_dtype, dres, accumulate, dy_bf16)


@pytest.mark.parametrize("cols", (100, 256, 768, 772, 1020, 1024))
def test_layernorm_pair_output_is_the_split_of_the_fp32_output(cols):
    """pair=True (DM_BF16_PAIR): hi / lo planes == the split of the fp32 result, bit for bit; same statistics."""
    ops = _ops()
    rows = 67
    d = R.ln_inputs(rows, cols)
    x, g, b = d["x"].to(DEV), d["gamma"].to(DEV), d["beta"].to(DEV)
    y32, mean, rstd = ops.layernorm_fwd(x, g, b, R.LN_EPS, F32)
    pl, mean_p, rstd_p = ops.layernorm_fwd(x, g, b, R.LN_EPS, BF16, pair=True)
    assert isinstance(pl, ops.Planes) and tuple(pl.t.shape) == (2, rows, cols)
    assert _same_bits(pl.t, _planes_on_device(y32))
    if cols % 8 == 0:
        assert _same_bits(pl.t, ops.split_planes(y32).t)
    assert _same_bits(mean, mean_p) and _same_bits(rstd, rstd_p)


@pytest.mark.parametrize("cols", (100, 768, 1024, 1028, 8188))
@pytest.mark.parametrize("dy_dtype", (F32, BF16))
def test_layernorm_bwd_lp_copy_is_the_rounded_dx(cols, dy_dtype):
    """want_lp: the bf16 copy == dx.bfloat16() bit for bit (register-resident kernels and the streamed dx kernel); dx, dgamma, dbeta
    are those of the plain call."""
    ops = _ops()
    rows = 67
    d = R.ln_inputs(rows, cols)
    x, g, b, dy, dr = d["x"].to(DEV), d["gamma"].to(DEV), d["beta"].to(DEV), d["dy"].to(DEV).to(dy_dtype), d["dres"].to(DEV)
    _, mean, rstd = ops.layernorm_fwd(x, g, b, R.LN_EPS, F32)
    dx0, dg0, db0 = ops.layernorm_bwd(dy, x, g, mean, rstd, dres=dr)
    dx, lp, dg, db = ops.layernorm_bwd(dy, x, g, mean, rstd, dres=dr, want_lp=True)
    assert lp.dtype == BF16 and _same_bits(lp, dx.bfloat16())
    assert _same_bits(dx, dx0) and _same_bits(dg, dg0) and _same_bits(db, db0)


@pytest.mark.parametrize("cols", (100, 256, 768, 772, 1024))
@pytest.mark.parametrize("dy_dtype", (F32, BF16))
def test_layernorm_bwd_pair_is_the_split_of_dx(cols, dy_dtype):
    """want_pair (dm_layernorm_bwd_partials_pair): planes == the split of dx bit for bit (the lo plane sits rows * cols behind the
    hi plane); dx, dgamma, dbeta equal the plain call's bit for bit."""
    ops = _ops()
    rows = 67
    d = R.ln_inputs(rows, cols)
    x, g, b, dy, dr = d["x"].to(DEV), d["gamma"].to(DEV), d["beta"].to(DEV), d["dy"].to(DEV).to(dy_dtype), d["dres"].to(DEV)
    _, mean, rstd = ops.layernorm_fwd(x, g, b, R.LN_EPS, F32)
    dx0, dg0, db0 = ops.layernorm_bwd(dy, x, g, mean, rstd, dres=dr)
    dx, pl, dg, db = ops.layernorm_bwd(dy, x, g, mean, rstd, dres=dr, want_pair=True)
    assert isinstance(pl, ops.Planes) and tuple(pl.t.shape) == (2, rows, cols)
    assert _same_bits(dx, dx0) and _same_bits(dg, dg0) and _same_bits(db, db0)
    assert _same_bits(pl.t, _planes_on_device(dx))
    if cols % 8 == 0:
        assert _same_bits(pl.t, ops.split_planes(dx).t)


def test_layernorm_pair_outputs_refuse_wide_rows():
    """Plane-pair results exist only for the register-resident widths: cols > 1024 is refused on the host, before any launch."""
    ops = _ops()
    d = R.ln_inputs(5, 1028)
    x, g, b = d["x"].to(DEV), d["gamma"].to(DEV), d["beta"].to(DEV)
    with pytest.raises(ValueError, match="plane-pair"):
        ops.layernorm_fwd(x, g, b, R.LN_EPS, BF16, pair=True)
    _, mean, rstd = ops.layernorm_fwd(x, g, b, R.LN_EPS, F32)
    with pytest.raises(ValueError, match="plane-pair"):
        ops.layernorm_bwd(d["dy"].to(DEV), x, g, mean, rstd, want_pair=True)


# =====================================================================================================================================
# token pool / group mean (grid data: every sum is exact in fp32)
# =====================================================================================================================================
@pytest.mark.parametrize("B,S,side,C", R.TOKEN_POOL_SHAPES + (R.TOKEN_POOL_BIG,))
def test_token_pool_exact(B, S, side, C):
    """Forward and backward (random upstream gradient) equal float64 exactly: four grid values sum exactly and x 0.25 is exact.
    The last shape has more than 4096 * 256 work items, so the grid-stride loop runs."""
    ops = _ops()
    x = R.grid_values((B, S * side * side, C), 61, B, S, side, C)
    go = R.grid_values((B, S * (side // 2) ** 2, C), 67, B, S, side, C)
    xd = x.to(DEV).requires_grad_(True)
    y = ops.TokenPoolFn.apply(xd, S, side)
    y.backward(go.to(DEV))
    xr = x.double().requires_grad_(True)
    want = R.token_pool_ref(xr, S, side)
    (want * go.double()).sum().backward()
    assert torch.equal(y.detach().cpu().double(), want.detach())
    assert torch.equal(xd.grad.cpu().double(), xr.grad)


@pytest.mark.parametrize("rows,g,C", R.GROUP_MEAN_CASES)
def test_group_mean_one_ulp(rows, g, C):
    """Forward and backward against float64 with a random upstream gradient (a wrong source row cannot hide): the group's sum is
    exact, the factor fl(1/g) and the product are one rounding each: |err| <= 2^-23 |want| (exact for g = 1, 4)."""
    ops = _ops()
    x = R.grid_values((rows * g, C), 71, rows, g, C)
    go = R.grid_values((rows, C), 73, rows, g, C)
    xd = x.to(DEV).requires_grad_(True)
    y = ops.GroupMeanFn.apply(xd, g)
    y.backward(go.to(DEV))
    xr = x.double().requires_grad_(True)
    want = R.group_mean_ref(xr, g)
    (want * go.double()).sum().backward()
    rel = 0.0 if g in (1, 4) else 2.0 ** -23
    assert tuple(y.shape) == (rows, C)
    assert bool(((y.detach().cpu().double() - want.detach()).abs() <= rel * want.detach().abs()).all())
    assert bool(((xd.grad.cpu().double() - xr.grad).abs() <= rel * xr.grad.abs()).all())


# =====================================================================================================================================
# colsum
# =====================================================================================================================================
def _colsum_raw(X, out, accumulate, ldx=None):
    L = _lib()
    M, N = X.shape
    part = torch.empty(L.lib().dm_colsum_partial_floats(N), dtype=F32, device=DEV)
    L.check(L.lib().dm_colsum(X.data_ptr(), 1 if X.dtype == BF16 else 0, X.stride(0) if ldx is None else ldx, out.data_ptr(), M, N,
                              int(accumulate), part.data_ptr(), _stream()), "dm_colsum")


@pytest.mark.parametrize("M", R.COLSUM_M)
def test_colsum_shapes(M):
    """Every slice-count edge (one slice: the direct path; 257 rows: two; > 16384 rows: 64 slices of > 256 rows) x vector and generic
    widths x fp32 / bf16, against float64; integer data bit for bit; accumulate both ways on the direct path and at 257 rows."""
    ops = _ops()
    base, basei = R.colsum_base(), R.colsum_base_int()
    for N in R.COLSUM_N_VEC + R.COLSUM_N_GEN:
        for dt in (F32, BF16):
            X = base[:M, :N].to(dt).contiguous()
            out = torch.full((N,), float("nan"), device=DEV)
            assert ops.colsum(X.to(DEV), out) is out
            _within(f"colsum {M}x{N} {str(dt)[6:]}", out, R.colsum_ref(X), R.colsum_tol(X))
            Xi = basei[:M, :N].to(dt).contiguous()
            outi = torch.full((N,), float("nan"), device=DEV)
            ops.colsum(Xi.to(DEV), outi)
            assert torch.equal(outi.cpu().double(), R.colsum_ref(Xi)), (M, N, dt)
        if M <= 257:
            X, o = base[:M, :N].contiguous(), R.colsum_out0(N)
            for acc in (True, False):
                out = o.clone().to(DEV)
                ops.colsum(X.to(DEV), out, accumulate=acc)
                _within(f"colsum {M}x{N} accumulate={int(acc)}", out, R.colsum_ref(X) + (o.double() if acc else 0), R.colsum_tol(X, o if acc else None))
                Xi, oi = basei[:M, :N].contiguous(), torch.arange(N, dtype=F32) - 3
                outi = oi.clone().to(DEV)
                ops.colsum(Xi.to(DEV), outi, accumulate=acc)
                assert torch.equal(outi.cpu().double(), R.colsum_ref(Xi) + (oi.double() if acc else 0)), (M, N, acc)


@pytest.mark.parametrize("M", (16, 256, 257, 16385))
def test_colsum_strides_and_alignment(M):
    """ldx > N (a column slice of a wider matrix), X one element off 16-byte alignment (the generic kernel takes it), out one element
    off (the direct path is refused: partial rows and the reduction).  Integer data: bit for bit."""
    ops = _ops()
    basei = R.colsum_base_int()
    wide = basei[:M, :96].contiguous().to(DEV)
    for N, c0 in ((68, 4), (64, 8), (10, 3), (60, 1)):                       # c0 = 1, 3: unaligned first column as well
        for dt in (F32, BF16):
            w = wide.to(dt)
            X = w[:, c0:c0 + N]
            assert X.stride(0) == 96 and not X.is_contiguous()
            want = R.colsum_ref(basei[:M, c0:c0 + N])
            for acc in (False, True):
                out = torch.full((N,), 2.0, device=DEV)
                ops.colsum(X, out, accumulate=acc)
                assert torch.equal(out.cpu().double(), want + (2.0 if acc else 0.0)), ("ldx", M, N, dt, acc)
    for N in (68, 768, 10):
        Xc = basei[:M, :N].contiguous()
        want = R.colsum_ref(Xc)
        for dt in (F32, BF16):
            flat = torch.zeros(M * N + 1, dtype=dt, device=DEV)
            Xu = flat[1:].view(M, N)
            Xu.copy_(Xc.to(dt))
            assert Xu.data_ptr() % 16 != 0
            out = torch.full((N,), float("nan"), device=DEV)
            ops.colsum(Xu, out)
            assert torch.equal(out.cpu().double(), want), ("unaligned X", M, N, dt)
        for acc in (False, True):
            buf = torch.full((N + 1,), 5.0, device=DEV)
            out = buf[1:]
            assert out.data_ptr() % 16 != 0
            _colsum_raw(Xc.to(DEV), out, acc)
            assert torch.equal(out.cpu().double(), want + (5.0 if acc else 0.0)), ("unaligned out", M, N, acc)
            assert float(buf[0]) == 5.0


# =====================================================================================================================================
# cast
# =====================================================================================================================================
@pytest.mark.parametrize("n", R.CAST_SIZES)
def test_cast_bf16_bitwise(n):
    """ops.cast to bf16 == torch.Tensor.bfloat16() bit for bit (NaN as NaN-ness): every tail length, ties both ways, +-0, +-inf,
    overflow to inf, denormals; the largest n runs the grid-stride loop (the grid is capped at 4096 workgroups)."""
    ops = _ops()
    x = R.cast_inputs(n)
    got = ops.cast(x.to(DEV), BF16)
    assert got.dtype == BF16 and tuple(got.shape) == (n,)
    gb = _bits(got).numpy()
    assert R.bf16_same(gb, _bits(x.bfloat16()).numpy())
    assert R.bf16_same(gb, R.cast_bf16_ref(x))


@pytest.mark.parametrize("n", R.COPY_SIZES)
def test_cast_f32_copy_bitwise(n):
    """dm_cast with DM_F32 (copy_f32_kernel, not reachable through ops.cast): a bit-exact copy, the element past the end untouched."""
    L = _lib()
    x = R.cast_inputs(n).to(DEV)
    dst = torch.full((n + 1,), 7.0, device=DEV)
    L.check(L.lib().dm_cast(x.data_ptr(), dst.data_ptr(), L.DM_F32, n, _stream()), "dm_cast")
    assert torch.equal(dst[:n].view(torch.int32), x.view(torch.int32)) and float(dst[n]) == 7.0


# =====================================================================================================================================
# Adam
# =====================================================================================================================================
def _adam_three_ways(n, grads, step0, gs):
    """Runs the host-scalar kernel call, the device-scalar one and the device-scalar plane-pair one; checks lp / lo after every step
    and that the three agree bit for bit; returns the host-scalar (p, m, v)."""
    ops = _ops()
    p0 = R.adam_p0(n) if n <= 200000 else torch.sin(torch.arange(n, dtype=F32))
    st = [[p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)] for _ in range(3)]
    lp = [torch.zeros(n, dtype=BF16, device=DEV) for _ in range(3)]
    lo = torch.zeros(n, dtype=BF16, device=DEV)
    for k, g in enumerate(grads):
        gd = g.to(DEV)
        step = step0 + k
        hyper = ops.adam_hyper(step, R.ADAM_LR).to(DEV)
        ops.adam_step(st[0][0], gd, st[0][1], st[0][2], step, lr=R.ADAM_LR, grad_scale=gs, param_lp=lp[0])
        ops.adam_step_dev(st[1][0], gd, st[1][1], st[1][2], hyper, grad_scale=gs, param_lp=lp[1])
        ops.adam_step_dev(st[2][0], gd, st[2][1], st[2][2], hyper, grad_scale=gs, param_lp=lp[2], param_lo=lo)
        for j in (1, 2):
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(st[0], st[j])), (n, step, j)
        p = st[2][0]
        for j in range(3):
            assert torch.equal(lp[j].view(torch.int16), p.bfloat16().view(torch.int16)), (n, step, j)
        assert torch.equal(lo.view(torch.int16), (p - lp[2].float()).bfloat16().view(torch.int16)), (n, step)
    return p0, st[0]


def _adam_check(n, grads, step0, gs, p0, got):
    fam = R.adam_family_index(n)
    p, m, v, tp, tm, tv = R.adam_run_ref(p0, grads, step0, gs)
    pg, mg, vg = (t.cpu() for t in got)
    fin = fam != 2
    name = f"adam n={n} step {step0} scale {gs}"
    _within(f"{name} p", pg, p, tp)
    _within(f"{name} m", mg, m, tm)
    _within(f"{name} v", vg[fin], v[fin], tv[fin])
    assert torch.equal(pg[~fin], p0[~fin]) and bool(torch.isinf(vg[~fin]).all())                  # g^2 overflows: update 0, as torch gives
    z = fam == 1
    assert torch.equal(pg[z], p0[z]) and not bool(mg[z].any()) and not bool(vg[z].any())          # zero gradient, v = 0: update exactly 0


@pytest.mark.parametrize("n", R.ADAM_SIZES)
def test_adam_three_paths(n):
    """adam_step, adam_step_dev and adam_step_dev with param_lp / param_lo: every tail length, three consecutive steps from early
    and late step numbers, grad_scale 1 and 0.3; float64 truth in torch.optim.Adam's order; the device-scalar paths equal the
    host-scalar one bit for bit; lp == bf16(p), lo == bf16(p - lp) bit for bit."""
    for step0 in R.ADAM_STEPS:
        for gs in (1.0, 0.3):
            grads = [R.adam_inputs(n, k) for k in range(3)]
            p0, got = _adam_three_ways(n, grads, step0, gs)
            _adam_check(n, grads, step0, gs, p0, got)


def test_adam_past_the_grid_cap():
    """n > 16384 * 256 * 4: the grid-stride loop of adam_kernel takes a second trip, and the scalar tail follows it."""
    n = R.ADAM_BIG
    g = R.adam_inputs(n, 0)
    grads = [g, g * -0.5, g * 0.25]                       # exact scalings: the families stay what they are
    p0, got = _adam_three_ways(n, grads, 1, 1.0)
    _adam_check(n, grads, 1, 1.0, p0, got)


def test_adam_dev_paths_refuse_misaligned_buffers():
    """A buffer off 16-byte alignment on a device-scalar path returns the alignment error on the host (no launch) and raises."""
    ops = _ops()
    n = 8
    mk = lambda dt=F32: torch.zeros(n + 4, dtype=dt, device=DEV)
    hyper = ops.adam_hyper(1, R.ADAM_LR).to(DEV)
    p, g, m, v, lp, lo = mk(), mk(), mk(), mk(), mk(BF16), mk(BF16)
    for bad in range(4):
        args = [t[1:1 + n] if i == bad else t[:n] for i, t in enumerate((p, g, m, v))]
        with pytest.raises(ValueError, match="aligned"):
            ops.adam_step_dev(*args, hyper)
        with pytest.raises(ValueError, match="aligned"):
            ops.adam_step_dev(*args, hyper, param_lp=lp[:n], param_lo=lo[:n])
    with pytest.raises(ValueError, match="aligned"):
        ops.adam_step_dev(p[:n], g[:n], m[:n], v[:n], hyper, param_lp=lp[1:1 + n])
    with pytest.raises(ValueError, match="aligned"):
        ops.adam_step_dev(p[:n], g[:n], m[:n], v[:n], hyper, param_lp=lp[:n], param_lo=lo[1:1 + n])
    assert not bool(p.any()) and not bool(m.any()) and not bool(v.any())


# =====================================================================================================================================
# contrastive loss / cross-entropy
# =====================================================================================================================================
def _contrastive_raw(a, b, flag, upstream):
    L = _lib()
    B, D = a.shape
    ad, bd, fd = a.to(DEV), b.to(DEV), flag.to(DEV).float()
    loss = torch.full((1,), float("nan"), device=DEV)
    da, db = torch.full_like(ad, float("nan")), torch.full_like(bd, float("nan"))
    L.check(L.lib().dm_contrastive_loss(ad.data_ptr(), bd.data_ptr(), fd.data_ptr(), R.CL_MARGIN, upstream, loss.data_ptr(), da.data_ptr(),
                                        db.data_ptr(), B, D, _stream()), "dm_contrastive_loss")
    return loss[0], da, db


@pytest.mark.parametrize("B", R.CL_B)
def test_contrastive_loss_shapes_and_hinge_boundary(B):
    """B x D (D below, at and above one wave; not a multiple of 64), int64 and float flags through ContrastiveLossFn, upstream 2.5
    through the kernel's own argument.  Rows with d == margin exactly and flag 0 have loss term 0 and gradient rows exactly 0
    (relu'(0) = 0 as in torch); rows with a == b have gradient exactly 0."""
    ops = _ops()
    for D in R.CL_D:
        a, b, flag, fam = R.cl_inputs(B, D)
        loss, da, db, d, tl, tg = R.contrastive_ref(a, b, flag)
        for fdt in (torch.int64, F32):
            ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
            got = ops.ContrastiveLossFn.apply(ad, bd, flag.to(fdt).to(DEV), R.CL_MARGIN)
            got.backward()
            name = f"contrastive B={B} D={D} flag {str(fdt)[6:]}"
            _within(f"{name} loss", got, loss, tl)
            _within(f"{name} da", ad.grad, da, tg)
            _within(f"{name} db", bd.grad, db, tg)
            zero = torch.tensor([f in ("boundary", "equal") for f in fam])
            assert not bool(ad.grad.cpu()[zero].any()) and not bool(bd.grad.cpu()[zero].any())
        loss, da, db, d, tl, tg = R.contrastive_ref(a, b, flag, upstream=2.5)
        gl, gda, gdb = _contrastive_raw(a, b, flag, 2.5)
        _within(f"contrastive B={B} D={D} up=2.5 loss", gl, loss, tl)
        _within(f"contrastive B={B} D={D} up=2.5 da", gda, da, tg)
        _within(f"contrastive B={B} D={D} up=2.5 db", gdb, db, tg)
        bnd = torch.tensor([f == "boundary" for f in fam])
        if bool(bnd.any()):                                  # the boundary rows alone: loss exactly 0, every gradient exactly 0
            gl, gda, gdb = _contrastive_raw(a[bnd], b[bnd], flag[bnd], 2.5)
            assert float(gl) == 0.0 and not bool(gda.any()) and not bool(gdb.any())


def _cross_entropy_raw(x, tgt, upstream):
    L = _lib()
    B, K = x.shape
    xd, td = x.to(DEV), tgt.to(DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    dl = torch.full_like(xd, float("nan"))
    ti, tp = (None, td.data_ptr()) if tgt.dtype.is_floating_point else (td.data_ptr(), None)
    L.check(L.lib().dm_cross_entropy(xd.data_ptr(), ti, tp, upstream, loss.data_ptr(), dl.data_ptr(), B, K, _stream()), "dm_cross_entropy")
    return loss[0], dl


@pytest.mark.parametrize("K", R.CE_K)
def test_cross_entropy_spread_logits(K):
    """K below, at and above one wave; logits N(0, 3), rows with one entry 1e4 above the rest and rows shifted by +-1e4; index and
    probability targets; loss and gradient against float64."""
    ops = _ops()
    for B in R.CE_B:
        x, ti, tp = R.ce_inputs(B, K)
        for tname, tgt in (("index", ti), ("prob", tp)):
            loss, grad, tl, tg = R.cross_entropy_ref(x, tgt, upstream=1.5)
            gl, gg = _cross_entropy_raw(x, tgt, 1.5)
            assert bool(torch.isfinite(gg).all())
            _within(f"cross-entropy B={B} K={K} {tname} loss", gl, loss, tl)
            _within(f"cross-entropy B={B} K={K} {tname} grad", gg, grad, tg)
            loss, grad, tl, tg = R.cross_entropy_ref(x, tgt)
            xg = x.to(DEV).requires_grad_(True)
            got = ops.CrossEntropyFn.apply(xg, tgt.to(DEV))
            got.backward()
            _within(f"cross-entropy B={B} K={K} {tname} Fn loss", got, loss, tl)
            _within(f"cross-entropy B={B} K={K} {tname} Fn grad", xg.grad, grad, tg)


# =====================================================================================================================================
# GRU cell
# =====================================================================================================================================
@pytest.mark.parametrize("strided", (False, True))
@pytest.mark.parametrize("B,H", R.GRU_SHAPES)
def test_gru_cell(B, H, strided):
    """GRUCellFn forward against float64 nn.GRUCell arithmetic and backward against float64 autograd with a random upstream
    gradient; gi contiguous and as the time slice gi_all[:, 1] of [B, T, 3H] (row stride T * 3H); rows with pre-activations at
    +-30 and +-100 stay finite."""
    ops = _ops()
    gi_all, gh, h, dh = R.gru_inputs(B, H)
    out, dgi, dgh, dhin, tf, tb = R.gru_truth(gi_all[:, 1], gh, h, dh)
    ghd, hd = gh.to(DEV).requires_grad_(True), h.to(DEV).requires_grad_(True)
    if strided:
        leaf = gi_all.to(DEV).requires_grad_(True)
        gi = leaf[:, 1]
        assert gi.stride(0) == R.GRU_T * 3 * H or B == 1
    else:
        leaf = gi_all[:, 1].contiguous().to(DEV).requires_grad_(True)
        gi = leaf
    got = ops.GRUCellFn.apply(gi, ghd, hd)
    got.backward(dh.to(DEV))
    g_gi = leaf.grad[:, 1] if strided else leaf.grad
    for t in (got, g_gi, ghd.grad, hd.grad):
        assert bool(torch.isfinite(t).all())
    if strided:
        assert not bool(leaf.grad[:, 0].any()) and not bool(leaf.grad[:, 2].any())
    name = f"gru B={B} H={H} {'strided' if strided else 'contiguous'}"
    _within(f"{name} h'", got, out, tf)
    _within(f"{name} dgi", g_gi, dgi, tb.repeat(1, 3))
    _within(f"{name} dgh", ghd.grad, dgh, tb.repeat(1, 3))
    _within(f"{name} dh", hd.grad, dhin, tb)
