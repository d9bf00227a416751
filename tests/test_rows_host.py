"""CPU: the references of tests/rows_ref.py against torch's own float64 operators, and the tolerance check of the GPU row tests.

For every tolerance tests/test_gpu_rows.py uses, the float32 restatement of the kernel's arithmetic runs here on exactly the GPU
test's inputs and must stay at or below HALF the bound (`_half`), so a correct kernel has a factor 2 of headroom.  The worst
err / tol per case is printed (run with -s); the table at the top of test_gpu_rows.py records it.  The deliberately wrong one-pass
variance must FAIL the LayerNorm bound on the large-offset rows: that failure is the evidence that the bound bites.
"""
import math

import numpy as np
import pytest
import torch

import rows_ref as R


def _half(name, err, tol):
    r = R.worst(err, tol)
    print(f"  [rows_host] {name:<44s} err/tol = {r:.3f}")
    assert r <= 0.5, f"{name}: fp32 restatement at {r:.3f} of the bound (must be <= 0.5)"
    return r


def _diff(a, b):
    return (a.double() - b.double()).abs()


# ---- the float64 restatements against torch's own operators ---------------------------------------------------------------------
def test_layernorm_ref_is_torch_layer_norm():
    d = R.ln_inputs(5, 100)
    t = R.ln_truth(5, 100)
    x, g, b = d["x"].double().requires_grad_(True), d["gamma"].double().requires_grad_(True), d["beta"].double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(x, (100,), g, b, float(np.float32(R.LN_EPS)))
    (y * d["dy"].double()).sum().backward()
    for got, want in ((t["y"], y.detach()), (t["dx"], x.grad), (t["dgamma"], g.grad), (t["dbeta"], b.grad)):
        torch.testing.assert_close(got, want, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(t["mean"], d["x"].double().mean(-1), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(t["rstd"], 1 / torch.sqrt(d["x"].double().var(-1, unbiased=False) + float(np.float32(R.LN_EPS))), rtol=1e-9, atol=0)


def test_pool_refs_are_avg_pool():
    B, S, side, C = 3, 4, 8, 12
    x = R.grid_values((B, S * side * side, C), 1).double()
    img = x.reshape(B * S, side, side, C).permute(0, 3, 1, 2)
    want = torch.nn.functional.avg_pool2d(img, 2, 2).permute(0, 2, 3, 1).reshape(B, S * 16, C)
    assert torch.equal(R.token_pool_ref(x, S, side), want)
    z = R.grid_values((B, S * 7, C), 2).double()
    want = torch.nn.functional.adaptive_avg_pool1d(z.reshape(B * S, 7, C).transpose(1, 2), 1).squeeze(-1)
    torch.testing.assert_close(R.group_mean_ref(z, 7), want, rtol=1e-14, atol=1e-14)


def test_cast_ref_is_torch_bfloat16():
    for n in (1, 5, 17, 1001, 4099):
        x = R.cast_inputs(n)
        assert R.bf16_same(R.cast_bf16_ref(x), x.bfloat16().view(torch.int16).numpy()), n
    x = R.cast_inputs(1001)
    assert set(R.CAST_SPECIALS.tolist()) <= set(x.numpy().view(np.uint32).tolist())


def test_adam_ref_is_oracle_adam_and_torch():
    from oracle import adam as OA
    n = 1023
    grads = [R.adam_inputs(n, k) for k in range(3)]
    keep = R.adam_family_index(n) != 2                         # (the overflow family has fp32 semantics: checked below)
    for step0 in R.ADAM_STEPS:
        p, m, v, *_ = R.adam_run_ref(R.adam_p0(n), grads, step0, grad_scale=0.3)
        po, mo, vo = R.adam_p0(n).double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        for k, g in enumerate(grads):
            OA.adam_step(po, g.double() * 0.3, mo, vo, step0 + k, lr=R.ADAM_LR)
        for a, b in ((p, po), (m, mo), (v, vo)):
            torch.testing.assert_close(a[keep], b[keep], rtol=1e-12, atol=1e-300)
    # torch.optim.Adam itself, fp32, from step 1: the overflow family leaves p untouched, v = inf
    w = torch.nn.Parameter(R.adam_p0(n).clone())
    opt = torch.optim.Adam([w], lr=R.ADAM_LR)
    for g in grads:
        w.grad = g.clone()
        opt.step()
    p, m, v, tp, _, _ = R.adam_run_ref(R.adam_p0(n), grads, 1)
    assert torch.equal(w.detach()[~keep], R.adam_p0(n)[~keep]) and torch.equal(p[~keep], R.adam_p0(n).double()[~keep])
    assert bool(torch.isinf(v[~keep]).all())
    assert R.worst(_diff(w.detach(), p), tp) <= 1.0


def test_loss_refs_are_torch():
    from oracle import losses as OL
    a, b, flag, _ = R.cl_inputs(33, 100)
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    (OL.contrastive_loss(ar, br, flag.double(), R.CL_MARGIN) * 2.5).backward()
    loss, da, db, *_ = R.contrastive_ref(a, b, flag, upstream=2.5)
    torch.testing.assert_close(loss, OL.contrastive_loss(a.double(), b.double(), flag.double(), R.CL_MARGIN), rtol=1e-13, atol=0)
    torch.testing.assert_close(da, ar.grad, rtol=1e-13, atol=1e-300)
    torch.testing.assert_close(db, br.grad, rtol=1e-13, atol=1e-300)
    x, ti, tp = R.ce_inputs(5, 65)
    for tgt in (ti, tp):
        xr = x.double().requires_grad_(True)
        want = torch.nn.functional.cross_entropy(xr, tgt.double() if tgt.dtype.is_floating_point else tgt)
        (want * 1.5).backward()
        loss, grad, _, _ = R.cross_entropy_ref(x, tgt, upstream=1.5)
        torch.testing.assert_close(loss, want.detach(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(grad, xr.grad, rtol=1e-11, atol=1e-15)


def test_gru_ref_is_gru_cell():
    B, I, H = 5, 7, 9
    g = torch.Generator().manual_seed(3)
    cell = torch.nn.GRUCell(I, H).double()
    x, h = torch.randn(B, I, generator=g).double(), torch.randn(B, H, generator=g).double()
    gi = x @ cell.weight_ih.T + cell.bias_ih
    gh = h @ cell.weight_hh.T + cell.bias_hh
    torch.testing.assert_close(R.gru_cell_ref(gi, gh, h), cell(x, h), rtol=1e-13, atol=1e-13)


# ---- the tolerance check: fp32 restatements on the GPU tests' inputs -------------------------------------------------------------
def _ln_check(rows, cols, tag):
    d, t = R.ln_inputs(rows, cols), R.ln_truth(rows, cols)
    y, mean, rstd = R.layernorm_fwd_f32(d["x"], d["gamma"], d["beta"])
    out = [_half(f"ln {tag} {rows}x{cols} y", _diff(y, t["y"]), R.ln_y_tol(d["x"], d["gamma"], t)),
           _half(f"ln {tag} {rows}x{cols} y(bf16)", _diff(y.bfloat16(), t["y"]), R.ln_y_tol(d["x"], d["gamma"], t, bf16=True)),
           _half(f"ln {tag} {rows}x{cols} mean", _diff(mean, t["mean"]), R.ln_mean_tol(d["x"])),
           _half(f"ln {tag} {rows}x{cols} rstd", _diff(rstd, t["rstd"]), R.ln_rstd_tol(d["x"], t))]
    dx, dg, db = R.layernorm_bwd_f32(d["dy"], d["x"], d["gamma"], mean, rstd, d["dres"], (d["g0"], d["g0"]))
    tg, tb = R.ln_dgb_tol(t, d["g0"])
    out += [_half(f"ln {tag} {rows}x{cols} dx", _diff(dx, t["dx"] + d["dres"].double()), R.ln_dx_tol(d["x"], d["gamma"], t, d["dres"])),
            _half(f"ln {tag} {rows}x{cols} dgamma", _diff(dg, t["dgamma"] + d["g0"].double()), tg),
            _half(f"ln {tag} {rows}x{cols} dbeta", _diff(db, t["dbeta"] + d["g0"].double()), tb)]
    return out


@pytest.mark.parametrize("cols", R.LN_WIDTHS)
def test_layernorm_bounds_widths(cols):
    for rows in R.LN_ROWS:
        _ln_check(rows, cols, "width")


@pytest.mark.parametrize("rows,cols", R.LN_CAP_CASES)
def test_layernorm_bounds_grid_caps(rows, cols):
    _ln_check(rows, cols, "cap")


@pytest.mark.parametrize("cols", R.LN_OPTION_WIDTHS)
def test_layernorm_bounds_options(cols):
    """dres None, accumulate False, bf16 dy: the other arms of the options cross."""
    rows = 67
    d, t = R.ln_inputs(rows, cols), R.ln_truth(rows, cols, bf16_dy=True)
    _, mean, rstd = R.layernorm_fwd_f32(d["x"], d["gamma"], d["beta"])
    dx, dg, db = R.layernorm_bwd_f32(t["dy"], d["x"], d["gamma"], mean, rstd)
    tg, tb = R.ln_dgb_tol(t)
    _half(f"ln opt 67x{cols} dx (bf16 dy, no dres)", _diff(dx, t["dx"]), R.ln_dx_tol(d["x"], d["gamma"], t))
    _half(f"ln opt 67x{cols} dgamma (bf16 dy)", _diff(dg, t["dgamma"]), tg)
    _half(f"ln opt 67x{cols} dbeta (bf16 dy)", _diff(db, t["dbeta"]), tb)


@pytest.mark.parametrize("cols", (100, 768, 1028, 8192))
def test_one_pass_variance_fails_the_bound(cols):
    """The deliberately wrong restatement (E[x^2] - mean^2) breaks the LayerNorm bounds on the large-offset rows, where the two-pass
    one passes with a factor 2 to spare: the offset mu = 1e3 is admitted, and the bound would catch a one-pass regression."""
    rows = 67
    d, t = R.ln_inputs(rows, cols), R.ln_truth(rows, cols)
    off = d["offset_rows"]
    y, _, rstd = R.layernorm_fwd_f32(d["x"], d["gamma"], d["beta"], one_pass=True)
    ry = R.worst(_diff(y, t["y"])[off], R.ln_y_tol(d["x"], d["gamma"], t)[off])
    rr = R.worst(_diff(rstd, t["rstd"])[off], R.ln_rstd_tol(d["x"], t)[off])
    print(f"  [rows_host] one-pass variance {rows}x{cols}: y err/tol = {ry:.1f}, rstd err/tol = {rr:.1f}")
    assert ry > 1.0 and rr > 1.0
    y2, _, rstd2 = R.layernorm_fwd_f32(d["x"], d["gamma"], d["beta"])
    assert R.worst(_diff(y2, t["y"])[off], R.ln_y_tol(d["x"], d["gamma"], t)[off]) <= 0.5
    assert R.worst(_diff(rstd2, t["rstd"])[off], R.ln_rstd_tol(d["x"], t)[off]) <= 0.5


def test_layernorm_constant_rows_are_exact_in_fp32():
    for cols in (100, 1028, 8192):
        d = R.ln_inputs(67, cols)
        y, mean, rstd = R.layernorm_fwd_f32(d["x"], d["gamma"], d["beta"])
        c = d["const_rows"]
        assert torch.equal(mean[c], d["x"][c][:, 0]) and torch.equal(y[c], d["beta"].expand(int(c.sum()), cols))


def test_pool_inputs_sum_exactly():
    """Sums of up to 7 grid values are exact in fp32, so the pooled results are exact (x 0.25) or one rounding of s * fl(1/g) away."""
    x = R.grid_values((2, 3 * 16, 100), 2, 3, 4, 100)
    assert torch.equal(R.token_pool_ref(x, 3, 4).double(), R.token_pool_ref(x.double(), 3, 4))
    for g in (1, 3, 4, 7):
        z = R.grid_values((5 * g, 100), g)
        got = z.reshape(5, g, 100).sum(1) * torch.tensor(1.0 / g, dtype=torch.float32)
        want = R.group_mean_ref(z.double(), g)
        assert bool((_diff(got, want) <= 2.0 ** -23 * want.abs()).all())


@pytest.mark.parametrize("M", R.COLSUM_M)
def test_colsum_bounds(M):
    base, basei = R.colsum_base(), R.colsum_base_int()
    for N in R.COLSUM_N_VEC + R.COLSUM_N_GEN:
        vec = N % 4 == 0
        for dt in (torch.float32, torch.bfloat16):
            X = base[:M, :N].to(dt)
            _half(f"colsum {M}x{N} {str(dt)[6:]}", _diff(R.colsum_f32(X, vec), R.colsum_ref(X)), R.colsum_tol(X))
        if M <= 257:
            X, o = base[:M, :N], R.colsum_out0(N)
            _half(f"colsum {M}x{N} accumulate", _diff(o + R.colsum_f32(X, vec), o.double() + R.colsum_ref(X)), R.colsum_tol(X, o))
        Xi = basei[:M, :N]
        assert torch.equal(R.colsum_f32(Xi, vec).double(), R.colsum_ref(Xi))


@pytest.mark.parametrize("n", R.ADAM_SIZES)
def test_adam_bounds(n):
    fam = R.adam_family_index(n)
    for step0 in R.ADAM_STEPS:
        for gs in (1.0, 0.3):
            grads = [R.adam_inputs(n, k) for k in range(3)]
            p, m, v, tp, tm, tv = R.adam_run_ref(R.adam_p0(n), grads, step0, gs)
            pf, mf, vf = R.adam_run_f32(R.adam_p0(n), grads, step0, gs)
            fin = fam != 2
            _half(f"adam n={n} step {step0} scale {gs} p", _diff(pf, p), tp)
            _half(f"adam n={n} step {step0} scale {gs} m", _diff(mf, m), tm)
            _half(f"adam n={n} step {step0} scale {gs} v", _diff(vf, v)[fin], tv[fin])
            assert torch.equal(pf[~fin], R.adam_p0(n)[~fin]) and bool(torch.isinf(vf[~fin]).all())
            assert torch.equal(pf[fam == 1], R.adam_p0(n)[fam == 1]) and not bool(mf[fam == 1].any()) and not bool(vf[fam == 1].any())


@pytest.mark.parametrize("B", R.CL_B)
def test_contrastive_bounds(B):
    for D in R.CL_D:
        a, b, flag, fam = R.cl_inputs(B, D)
        for up in (1.0, 2.5):
            loss, da, db, d, tl, tg = R.contrastive_ref(a, b, flag, upstream=up)
            lf, daf, dbf = R.contrastive_f32(a, b, flag, upstream=up)
            _half(f"contrastive B={B} D={D} up={up} loss", _diff(lf, loss), tl)
            _half(f"contrastive B={B} D={D} up={up} grad", torch.maximum(_diff(daf, da), _diff(dbf, db)), tg)
        for i, f in enumerate(fam):
            if f == "boundary":
                assert float(d[i]) == R.CL_MARGIN and not bool(daf[i].any())
            elif f == "push":                              # no random row sits where fp32 could take the other arm of the hinge
                assert abs(float(d[i]) - R.CL_MARGIN) > 1e-4


@pytest.mark.parametrize("K", R.CE_K)
def test_cross_entropy_bounds(K):
    for B in R.CE_B:
        x, ti, tp = R.ce_inputs(B, K)
        for name, tgt in (("index", ti), ("prob", tp)):
            loss, grad, tl, tg = R.cross_entropy_ref(x, tgt, upstream=1.5)
            lf, gf = R.cross_entropy_f32(x, tgt, upstream=1.5)
            _half(f"cross-entropy B={B} K={K} {name} loss", _diff(lf, loss), tl)
            _half(f"cross-entropy B={B} K={K} {name} grad", _diff(gf, grad), tg)


@pytest.mark.parametrize("B,H", R.GRU_SHAPES)
def test_gru_bounds(B, H):
    gi_all, gh, h, dh = R.gru_inputs(B, H)
    gi = gi_all[:, 1]
    out, dgi, dgh, dhin, tf, tb = R.gru_truth(gi, gh, h, dh)
    of, dgif, dghf, dhf = R.gru_cell_f32(gi, gh, h, dh)
    assert bool(torch.isfinite(of).all())
    _half(f"gru B={B} H={H} h'", _diff(of, out), tf)
    _half(f"gru B={B} H={H} dgi", _diff(dgif, dgi), tb.repeat(1, 3))
    _half(f"gru B={B} H={H} dgh", _diff(dghf, dgh), tb.repeat(1, 3))
    _half(f"gru B={B} H={H} dh", _diff(dhf, dhin), tb)
