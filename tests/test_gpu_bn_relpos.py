"""GPU: batch norm (csrc/dm_batchnorm.hip), the relative-position bias gather / reduce and patchify (csrc/dm_rows.hip,
dm_rows_wide.hip) at their edges, against the float64 restatements of tests/bn_relpos_ref.py.

Exact results (the gather, integer-slab reductions, the CSR, patchify in both dtypes) are compared bit for bit.  Everything else is
compared inside a bound derived from the fp32 rounding model (U = 2^-24); the integer constant in front of each bound is the smallest
one for which a float32 restatement of the kernel's arithmetic stays at or below half the bound on exactly these inputs
(tests/test_bn_relpos_host.py asserts that on the CPU), so a correct kernel has a factor 2 to spare.

  constant         bound (derivation in bn_relpos_ref.py)                                              worst err/tol   CPU     GPU (MI355X)
  C_BN_MEAN 2      U |mean| (+ the float64 sum's 2^-53 depth max|x|): one rounding of the float64 mean   save_mean      0.475   0.475
  C_BN_RSTD 2      U rstd (1 + float64 one-pass variance error x rstd^2 / 2): one rounding               save_rstd      0.492   0.492
  C_BN_RSTD_EVAL 4 U rstd: fp32 sum, root, division                                                      save_rstd      0.376   0.376
  C_BN_RUN 3       U ((1 - m) |r| + m |s|): fp32 momentum, one rounding of the float64 result            running stats  0.380   0.380
  C_BN_Y 7         U mask (|gamma| (|mean| rstd + |xhat|) + |z|): the fp32 mean, rel. U per operation    y              0.430   0.392
  C_BN_DX 4        U (|gamma| rstd (|g| + |mean g| + E0 + (A + |xhat|) |mean gx| + |xhat| (|mean gx| + E)) + |dx|),
                   A = |mean| rstd, E0 = mean_r |g| [mask != 1], E = mean_r |g| (A + |xhat|)             dx             0.487   0.487
  C_BN_DGB 3       U (|result| + sum_r |g| (A + |xhat|) resp. sum_r |g| [mask != 1]) [+ U |result| when accumulating]:
                   float64 sums rounded once, fp32 terms                                                 dgamma/dbeta   0.340   0.340
  C_RP_SUM 1       U (ceil(cnt / 64) chunks + 6) sum|terms| [+ 2 U |result| when accumulating]           dtable         0.457   0.457
  (deliberately wrong on the CPU: fp32 one-pass sums 8e5 .. 1.4e7 x the rstd bound and 1.5e2 .. 1.9e4 x the y bound on the mean-1e3
   columns; biased running variance 70 .. 2.8e6 x; a dropped last slice 2e6 .. 1e9 x the mean bound; a mask indexed by row writes
   non-zeros where y must be 0 and is 1.2e6 .. 2.4e6 x the bound elsewhere)

Every check prints its worst err / tol ("[bn_relpos_gpu] ..."; run with -s).
"""
import numpy as np
import pytest
import torch

import bn_relpos_ref as R
import rows_ref as RR

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
    print(f"  [bn_relpos_gpu] {name:<60s} err/tol = {r:.3f}")
    assert r <= 1.0, f"{name}: {r:.3f} of the bound (worst error {float(err.max()) / R.U:.1f} U)"


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# =====================================================================================================================================
# batch norm
# =====================================================================================================================================
def _bn_check_fwd(name, d, t, y, mean, rstd, rm, rv):
    """y, the saved statistics and (training, given) the running statistics of one forward against the truth `t`."""
    _within(f"{name} y", y, t["y"], R.bn_y_tol(d, t))
    assert float(y.detach().cpu()[t["mrow"] == 0].abs().sum()) == 0.0                 # dropped (sample, channel)s are exactly 0
    if t["training"]:
        _within(f"{name} save_mean", mean, t["mean"], R.bn_mean_tol(d, t))
        _within(f"{name} save_rstd", rstd, t["rstd"], R.bn_rstd_tol(t))
        c = d["const_cols"]                                 # zero variance (and the var < 0 clamp): rstd = eps^-1/2 to 2 ulp
        want, ulp2 = R.bn_const_rstd()
        assert float((rstd.cpu()[c].double() - want).abs().max()) <= ulp2
        if rm is not None:
            tm, tv = R.bn_run_tol(d, t)
            _within(f"{name} running_mean", rm, t["run_mean"], tm)
            _within(f"{name} running_var", rv, t["run_var"], tv)
    else:
        assert _same_bits(mean.cpu(), d["rm"]) and _same_bits(rm.cpu(), d["rm"]) and _same_bits(rv.cpu(), d["rv"])
        _within(f"{name} save_rstd (eval)", rstd, t["rstd"], R.bn_rstd_eval_tol(t))


def _bn_check_bwd(name, d, t, dx, dgamma, dbeta, g0=None):
    tg, tb = R.bn_dgb_tol(t, g0)
    if dx is not None:
        _within(f"{name} dx", dx, t["dx"], R.bn_dx_tol(d, t))
    _within(f"{name} dgamma", dgamma, t["dgamma"] + (g0[0].double() if g0 is not None else 0), tg)
    _within(f"{name} dbeta", dbeta, t["dbeta"] + (g0[1].double() if g0 is not None else 0), tb)


def _bn_abi_options(samples, rps, C, d, t):
    """What only the C entry points reach: training without running statistics (null pointers), accumulate = 0 into NaN-filled
    dgamma / dbeta (every column must be overwritten) and accumulate = 1 onto a known g0 (one more rounding in the bound)."""
    L = _lib()
    M = samples * rps
    name = f"bn {samples}x{rps}x{C} abi"
    x, g, b, mask, dy = (d[k].to(DEV) for k in ("x", "gamma", "beta", "mask", "dy"))
    y, dx = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    mean, rstd = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    ws = torch.empty(L.lib().dm_batchnorm_workspace_bytes(M, C), dtype=torch.uint8, device=DEV)
    L.check(L.lib().dm_batchnorm_fwd(x.data_ptr(), g.data_ptr(), b.data_ptr(), None, None, mask.data_ptr(), rps, y.data_ptr(), mean.data_ptr(),
                                     rstd.data_ptr(), M, C, R.BN_EPS, R.BN_MOMENTUM, 1, 1, ws.data_ptr(), _stream()), "dm_batchnorm_fwd")
    _bn_check_fwd(f"{name} no running stats", d, t, y, mean, rstd, None, None)
    for acc in (0, 1):
        g0 = d["g0"] if acc else None
        fill = d["g0"].to(DEV).clone() if acc else torch.full((2, C), float("nan"), device=DEV)
        L.check(L.lib().dm_batchnorm_bwd(dy.data_ptr(), x.data_ptr(), y.data_ptr(), g.data_ptr(), mask.data_ptr(), rps, mean.data_ptr(),
                                         rstd.data_ptr(), dx.data_ptr(), fill[0].data_ptr(), fill[1].data_ptr(), acc, M, C, 1, 1, ws.data_ptr(),
                                         _stream()), "dm_batchnorm_bwd")
        _bn_check_bwd(f"{name} accumulate={acc}", d, t, dx if acc == 0 else None, fill[0], fill[1], g0)


@pytest.mark.parametrize("samples,rps,C", R.BN_SHAPES)
def test_batchnorm_against_float64(samples, rps, C):
    """ops.BatchNormReluFn on every shape of bn_relpos_ref.BN_SHAPES (what each is for is noted there): training with ReLU and a
    mask, training plain, eval with ReLU; y, save_mean, save_rstd, both running statistics, dx, dgamma, dbeta against the float64
    restatement of BatchNorm2d -> ReLU -> per-(sample, channel) mask; y exactly 0 where the mask is 0; rstd of the constant
    columns at eps^-1/2 to 2 ulp.  Columns: N(0,1) | mean +-1e3, unit spread | constant | one outlier row.  Then, through the C
    entry points, the options BatchNormReluFn does not reach (_bn_abi_options)."""
    ops = _ops()
    d = R.bn_inputs(samples, rps, C)
    for tag, training, relu, masked in (("train relu mask", True, True, True), ("train plain", True, False, False),
                                        ("eval relu", False, True, False)):
        t = R.bn_truth(samples, rps, C, training, relu, masked)
        name = f"bn {samples}x{rps}x{C} {tag}"
        x, g, b = d["x"].to(DEV).requires_grad_(True), d["gamma"].to(DEV).requires_grad_(True), d["beta"].to(DEV).requires_grad_(True)
        rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
        y = ops.BatchNormReluFn.apply(x, g, b, rm, rv, d["mask"].to(DEV) if masked else None, rps, R.BN_EPS, R.BN_MOMENTUM, training, relu)
        mean, rstd = y.grad_fn.saved_tensors[4:6]
        _bn_check_fwd(name, d, t, y, mean, rstd, rm, rv)
        y.backward(d["dy"].to(DEV))
        _bn_check_bwd(name, d, t, x.grad, g.grad, b.grad)
        if masked:                                          # (the same truth serves the options only the C entry points reach)
            _bn_abi_options(samples, rps, C, d, t)


# =====================================================================================================================================
# relative-position bias: gather
# =====================================================================================================================================
def _gather_check(table, index, N, transposed):
    ops = _ops()
    out = ops.relpos_bias_gather(table.to(DEV), index.to(DEV), N, transposed=transposed)
    bias, bias_t = out if transposed else (out, None)
    want, want_t = R.rp_gather_ref(table, index)
    assert _same_bits(bias.cpu(), want)
    if transposed:
        assert _same_bits(bias_t.cpu(), want_t)
    else:
        assert isinstance(out, torch.Tensor)


@pytest.mark.parametrize("N", R.RP_GATHER_N)
@pytest.mark.parametrize("H", R.RP_GATHER_H)
@pytest.mark.parametrize("transposed", (False, True))
def test_relpos_gather_random_index_exact(N, H, transposed):
    """bias[h, i, j] == table[index[i, j], h] and bias_t[h, i, j] == table[index[j, i], h], bit for bit, on a seeded index that is
    NOT symmetric (a swapped or aliased bias_t fails) and a table with a distinct value per (bin, head)."""
    nb = R.rp_bins(N)
    _gather_check(R.rp_table(nb, H), R.rp_index(N, nb), N, transposed)


def test_relpos_gather_past_the_grid_cap():
    """N = 1025: N^2 > 4096 * 256, the grid-stride loop takes a second trip for some threads only (H = 3: 12.6 MB per output)."""
    N, H = R.RP_GATHER_BIG
    nb = R.rp_bins(N)
    _gather_check(R.rp_table(nb, H), R.rp_index(N, nb), N, True)


def test_relpos_gather_golden_cubes_exact():
    """Every cube of tests/golden/relpos_index.npz (the model's own, highly structured index tables), H = 3 and 12, both outputs."""
    from util import load_fx
    fx = load_fx("relpos_index.npz")
    cubes = [k[len("index/"):] for k in fx.files if k.startswith("index/")]
    assert len(cubes) == 8
    for cube in cubes:
        index, nb = torch.from_numpy(fx[f"index/{cube}"]), int(fx[f"table_rows/{cube}"])
        for H in (3, 12):
            _gather_check(R.rp_table(nb, H), index, index.shape[0], True)


def test_relpos_gather_clamps_out_of_range_indices():
    """Pins today's behaviour: the gather clamps entries outside [0, n_bins) to the nearest bin, while relpos_index_csr DROPS them
    (test_relpos_csr_drops_out_of_range_indices), so the two are not adjoint there.  The model never produces such entries."""
    N, H, nb = 4, 3, 7
    index = R.rp_index(N, nb).clone()
    index[0, 1], index[2, 0], index[3, 3] = -3, nb, nb + 100
    _gather_check(R.rp_table(nb, H), index, N, True)
    bias = _ops().relpos_bias_gather(R.rp_table(nb, H).to(DEV), index.to(DEV), N).cpu()
    assert torch.equal(bias[:, 0, 1], R.rp_table(nb, H)[0]) and torch.equal(bias[:, 2, 0], R.rp_table(nb, H)[nb - 1])


# =====================================================================================================================================
# relative-position bias: CSR and reduce
# =====================================================================================================================================
def _csr(index, nb):
    idx = index.to(DEV)
    return idx, _ops().relpos_index_csr(idx, nb)


@pytest.mark.parametrize("N", (1, 15, 16, 72, 256))
def test_relpos_index_csr_is_the_numpy_restatement(N):
    """positions / offsets equal the numpy restatement exactly: positions ascend within a bin, offsets are monotone from 0 to the
    number of entries, empty bins have equal offsets; also on a structured golden cube."""
    nb = R.rp_bins(N)
    index = R.rp_index(N, nb)
    _, (pos, off) = _csr(index, nb)
    wp, wo = R.rp_csr_ref(index, nb)
    assert pos.dtype == torch.int32 and off.dtype == torch.int32
    assert np.array_equal(pos.cpu().numpy(), wp) and np.array_equal(off.cpu().numpy(), wo)
    o = off.cpu().numpy()
    assert o[0] == 0 and o[-1] == N * N and bool((np.diff(o) >= 0).all())
    from util import load_fx
    fx = load_fx("relpos_index.npz")
    index, nb = torch.from_numpy(fx["index/3x4x4"]), int(fx["table_rows/3x4x4"])
    _, (pos, off) = _csr(index, nb)
    wp, wo = R.rp_csr_ref(index, nb)
    assert np.array_equal(pos.cpu().numpy(), wp) and np.array_equal(off.cpu().numpy(), wo)


def test_relpos_csr_drops_out_of_range_indices():
    """Pins today's behaviour: relpos_index_csr drops entries outside [0, n_bins) -- the reduce then never reads their slab
    positions -- while the gather CLAMPS them (test_relpos_gather_clamps_out_of_range_indices): not adjoint there.  The model
    never produces such entries."""
    ops = _ops()
    N, H, nb, chunks = 15, 3, 40, 2
    index = R.rp_index(N, nb).clone()
    index[0, 1], index[3, 2], index[14, 14] = -1, nb, nb + 5
    idx, (pos, off) = _csr(index, nb)
    wp, wo = R.rp_csr_ref(index, nb)
    assert np.array_equal(pos.cpu().numpy(), wp) and np.array_equal(off.cpu().numpy(), wo) and int(off[-1]) == N * N - 3
    slab = R.rp_slab(chunks, H, N, integer=True)
    dtable = torch.full((nb, H), float("nan"), device=DEV)
    ops.relpos_bias_scatter(slab.to(DEV).clone(), dtable, 1, H, (chunks, N, (pos, off)), nb)
    want, _ = R.rp_reduce_ref(slab, index, nb)
    assert torch.equal(dtable.cpu().double(), want)


def _reduce_run(N, H, chunks, aligned=True):
    ops = _ops()
    nb = R.rp_bins(N)
    index = R.rp_index(N, nb)
    _, csr = _csr(index, nb)
    info = (chunks, N, csr)
    path = "chunk_sum" if R.rp_chunk_sum_path(chunks, H, N, aligned) else "in-kernel loop"
    name = f"relpos reduce N={N} H={H} chunks={chunks} {path}"
    empty = torch.from_numpy(np.diff(R.rp_csr_ref(index, nb)[1]) == 0)
    assert bool(empty.any())

    def on_device(slab):                                    # a clone: chunk_sum_kernel overwrites chunk 0 of the slab it is given
        if aligned:
            return slab.to(DEV).clone()
        base = torch.empty(slab.numel() + 4, device=DEV)
        v = base[1:1 + slab.numel()].view(slab.shape)       # 4 bytes off a 16-byte boundary: the float4 chunk sum cannot run
        v.copy_(slab)
        assert v.data_ptr() % 16 != 0
        return v

    for integer in (True, False):
        slab = R.rp_slab(chunks, H, N, integer)
        want, mag = R.rp_reduce_ref(slab, index, nb)
        d0 = R.rp_dtable0(nb, H)
        for acc in (False, True):
            dtable = d0.to(DEV).clone() if acc else torch.full((nb, H), float("nan"), device=DEV)
            out = ops.relpos_bias_scatter(on_device(slab), dtable, 1, H, info, nb, accumulate=acc)
            assert out is dtable
            got = dtable.cpu()
            if acc:
                assert _same_bits(got[empty], d0[empty])                               # empty bins: unchanged bit for bit
            else:
                assert bool(torch.isfinite(got).all()) and not bool(got[empty].any())   # every bin overwritten, the empty ones with 0
            if integer and not acc:
                assert torch.equal(got.double(), want), name                            # every partial sum exact: any order gives the same bits
            else:
                res = want + d0.double() if acc else want
                _within(f"{name} {'int' if integer else 'real'} slab acc={int(acc)}", got, res,
                        R.rp_reduce_tol(index, nb, chunks, mag, res if acc else None))


@pytest.mark.parametrize("N,H,chunks", R.RP_REDUCE_CASES)
def test_relpos_reduce_against_add_at(N, H, chunks):
    """ops.relpos_index_csr -> ops.relpos_bias_scatter against np.add.at in float64, on an index whose bin counts include 0, 1, 63,
    64, 65 (and, at N >= 72, one bin of 4100 entries): H = 1, 3, 4, 5, 12 (a partly filled last group of four waves), chunks = 1,
    2, 5 through chunk_sum_kernel ((16, 4), (72, 4)) and through the in-kernel chunk loop ((15, 3), (73, 3): H N N % 4 != 0);
    accumulate = 0 into NaN (every bin, the empty ones included, is overwritten) and 1 (empty bins unchanged bit for bit); an
    integer slab bit for bit, a real-valued slab inside the derived bound."""
    _reduce_run(N, H, chunks)


def test_relpos_reduce_misaligned_slab_takes_the_in_kernel_loop():
    """H N N % 4 == 0 but the slab is not 16-byte aligned: the float4 chunk sum is skipped and the in-kernel chunk loop runs."""
    _reduce_run(16, 4, 2, aligned=False)


def test_relpos_gather_and_reduce_are_adjoint():
    """<gather(table), G> == <table, reduce(G)> in float64 on in-range indices: the gather is exact, so the difference is inside
    sum |table| x the reduce bound."""
    ops = _ops()
    for N, H, chunks in ((72, 5, 1), (16, 4, 2), (15, 3, 5)):
        nb = R.rp_bins(N)
        index = R.rp_index(N, nb)
        r = R._rng(101, N, H)
        table = R._t(r.standard_normal((nb, H)).astype(np.float32))
        G = R.rp_slab(chunks, H, N, integer=False)
        idx, csr = _csr(index, nb)
        bias = ops.relpos_bias_gather(table.to(DEV), idx, N).cpu()
        assert _same_bits(bias, R.rp_gather_ref(table, index)[0])
        dtable = torch.full((nb, H), float("nan"), device=DEV)
        ops.relpos_bias_scatter(G.to(DEV).clone(), dtable, 1, H, (chunks, N, csr), nb)
        lhs = float((bias.double()[None] * G.double()).sum())
        rhs = float((table.double() * dtable.cpu().double()).sum())
        _, mag = R.rp_reduce_ref(G, index, nb)
        tol = float((table.double().abs() * R.rp_reduce_tol(index, nb, chunks, mag)).sum())
        print(f"  [bn_relpos_gpu] relpos adjoint N={N} H={H} chunks={chunks}: |lhs - rhs| / tol = {abs(lhs - rhs) / tol:.3f}")
        assert abs(lhs - rhs) <= tol


# =====================================================================================================================================
# patchify
# =====================================================================================================================================
def _patchify_check(B, C, side, p, dtype):
    ops = _ops()
    x = R.patchify_input(B, C, side)
    want = torch.nn.functional.unfold(x, p, stride=p).transpose(1, 2).reshape(B * (side // p) ** 2, C * p * p).contiguous()
    got = ops.patchify(x.to(DEV), p, dtype)
    assert got.dtype == dtype and tuple(got.shape) == tuple(want.shape)
    if dtype == F32:
        assert _same_bits(got.cpu(), want)                  # a pure rearrangement: NaN payloads and signed zeros travel
        return
    assert _same_bits(got, ops.cast(want.to(DEV), BF16))    # the conversion of dm_cast, bit for bit
    gb = _bits(got).numpy().reshape(-1)
    assert RR.bf16_same(gb, _bits(want.bfloat16()).numpy().reshape(-1))               # torch's rounding (NaN as NaN-ness)
    assert RR.bf16_same(gb, RR.cast_bf16_ref(want.reshape(-1)))


@pytest.mark.parametrize("B,C,side,p", R.PATCHIFY_SHAPES)
@pytest.mark.parametrize("dtype", (F32, BF16))
def test_patchify_edges_bitwise(B, C, side, p, dtype):
    """== torch.nn.functional.unfold in (c, dy, dx) column order, bit for bit, at B = 1, C = 1, p = side, p = 4, p = 1, through
    patchify_kernel (p % 4 == 0) and patchify_any_kernel.  The input carries +-0, +-inf, NaNs, denormals and exact bf16 ties of
    both parities: the bf16 output equals dm_cast's bit for bit and torch.Tensor.bfloat16()'s."""
    _patchify_check(B, C, side, p, dtype)


@pytest.mark.parametrize("B,C,side,p", R.PATCHIFY_BIG)
@pytest.mark.parametrize("dtype", (F32, BF16))
def test_patchify_past_the_grid_cap_bitwise(B, C, side, p, dtype):
    """5 x 4 x 512 x 512 at p = 16: 1.3 M float4 items > 4096 * 256, so patchify_kernel's grid-stride loop runs.  5 x 4 x 504 x 504
    at p = 14: the same element count through patchify_any_kernel (whose grid is capped at 65536 workgroups, above this size)."""
    _patchify_check(B, C, side, p, dtype)
