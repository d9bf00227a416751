"""CPU: the references of tests/bn_relpos_ref.py against torch's own float64 operators, and the tolerance check of the GPU tests of
batch norm, the relative-position bias gather / reduce and patchify.

For every tolerance tests/test_gpu_bn_relpos.py uses, the float32 restatement of the kernel's arithmetic runs here on exactly the GPU
test's inputs and must stay at or below HALF the bound (`_half`); `test_constants_are_minimal` shows that no constant could be one
smaller.  The worst err / tol per case is printed (run with -s); the table at the top of test_gpu_bn_relpos.py records it.  The
deliberately wrong restatements (`mutate=`) must FAIL the bounds: that failure is the evidence that the inputs and bounds bite.
"""
import functools

import numpy as np
import pytest
import torch

import bn_relpos_ref as R
import rows_ref as RR

# (tag, training, relu, masked): the option runs of the GPU test
BN_RUNS = (("train relu mask", True, True, True), ("train plain", True, False, False), ("eval relu", False, True, False))


def _diff(a, b):
    return (a.double() - b.double()).abs()


def _half(name, ratio):
    print(f"  [bn_relpos_host] {name:<56s} err/tol = {ratio:.3f}")
    assert ratio <= 0.5, f"{name}: restatement at {ratio:.3f} of the bound (must be <= 0.5)"


# ---- the float64 restatements against torch's own operators ---------------------------------------------------------------------
@pytest.mark.parametrize("samples,rps,C", [(2, 1, 4), (3, 7, 12), (5, 4, 8)])
@pytest.mark.parametrize("training,relu,masked", [(True, True, True), (True, False, False), (False, True, False), (False, False, True)])
def test_bn_truth_is_torch_batchnorm2d(samples, rps, C, training, relu, masked):
    """nn.BatchNorm2d().double() -> ReLU -> channel mask on [samples, C, rows, 1] with autograd (a contiguous upstream gradient)."""
    d = R.bn_inputs(samples, rps, C)
    t = R.bn_truth(samples, rps, C, training, relu, masked)
    M = samples * rps
    bn = torch.nn.BatchNorm2d(C, eps=float(np.float32(R.BN_EPS)), momentum=R.BN_MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]); bn.bias.copy_(d["beta"]); bn.running_mean.copy_(d["rm"]); bn.running_var.copy_(d["rv"])
    bn.train(training)
    img = lambda a: a.double().view(samples, rps, C).permute(0, 2, 1).unsqueeze(-1).contiguous()
    back = lambda a: a.detach().squeeze(-1).permute(0, 2, 1).reshape(M, C)
    xr = img(d["x"]).requires_grad_(True)
    yr = bn(xr)
    if relu:
        yr = torch.relu(yr)
    if masked:
        yr = yr * d["mask"].double()[:, :, None, None]
    (yr * img(d["dy"])).sum().backward()
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-9)
    close(t["y"], back(yr)); close(t["dx"], back(xr.grad)); close(t["dgamma"], bn.weight.grad); close(t["dbeta"], bn.bias.grad)
    if training:
        close(t["run_mean"], bn.running_mean); close(t["run_var"], bn.running_var)
        close(t["mean"], d["x"].double().mean(0)); close(t["var"], d["x"].double().var(0, unbiased=False))
    else:
        assert torch.equal(bn.running_mean, d["rm"].double()) and torch.equal(bn.running_var, d["rv"].double())


def test_bn_shapes_reach_the_branches():
    """The slice arithmetic of dm_batchnorm.hip restated: what each shape of BN_SHAPES is there for."""
    M = {s * r: (s, r, c) for s, r, c in R.BN_SHAPES}
    assert sorted(M) == [2, 256, 257, 294, 771, 16384, 16385]
    assert R.bn_slicing(2) == (1, 2) and R.bn_slicing(256) == (1, 256) and R.bn_slicing(257) == (2, 129)
    assert R.bn_slicing(771) == (4, 193) and 257 % 193 != 0                       # the mask row changes inside a slice
    assert R.bn_slicing(16384) == (64, 256) and R.bn_slicing(16385) == (64, 257) and 16385 - 63 * 257 == 194
    assert 16385 * 260 // 4 == 1065025 > 4096 * 256 and 260 > 256                 # grid-stride loops; a second finalize block
    assert [c % 64 for _, _, c in R.BN_SHAPES] == [4, 0, 4, 60, 8, 4, 0]


@pytest.mark.parametrize("samples,rps,C", R.BN_SHAPES)
def test_bn_inputs_keep_the_relu_gate_unambiguous(samples, rps, C):
    """No x within BN_BAND / 2 of a sign change of its pre-activation (batch or running statistics): at most U * 1e3 = 6e-5 of fp32
    ambiguity cannot flip a gate.  Every family is present; the mask drops, keeps and fully drops a (sample, channel)."""
    d = R.bn_inputs(samples, rps, C)
    dist, zc = R.bn_gate_distance(d)
    print(f"  [bn_relpos_host] bn {samples}x{rps}x{C}: nearest sign change {dist:.4f}, constant columns' eval |z| >= {zc:.4f}")
    assert dist >= R.BN_BAND / 2 and zc >= 1e-5                 # (the fp32 z of a constant column is good to 1e-7 there)
    x = d["x"]
    c = d["const_cols"]
    assert bool((x[:, c] == x[0, c]).all()) and int(c.sum()) == C // 4 and int(d["offset_cols"].sum()) == C // 4
    assert float(x[:, d["offset_cols"]].abs().min()) > R.BN_MU - 10 and float(x[:, 3::4].abs().max()) >= R.BN_OUTLIER - 1
    m = d["mask"]
    assert set(m.unique().tolist()) == {0.0, float(np.float32(1.0) / np.float32(R.BN_KEEP))} and float(m[0, 0]) == 0 and float(m[0, 1]) > 0
    assert d["dy"].is_contiguous()


# ---- the tolerance check: restatements on the GPU tests' inputs ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bn_records(samples, rps, C):
    """[(constant, label, worst err / tol)] of the restatement on every option run of one shape."""
    d = R.bn_inputs(samples, rps, C)
    out = []
    name = f"bn {samples}x{rps}x{C}"
    for tag, training, relu, masked in BN_RUNS:
        t = R.bn_truth(samples, rps, C, training, relu, masked)
        y, mean, rstd, rm, rv = R.bn_fwd_f32(d, rps, training, relu, masked)
        rec = lambda c, what, err, tol: out.append((c, f"{name} {tag} {what}", R.worst(err, tol)))
        rec("C_BN_Y", "y", _diff(y, t["y"]), R.bn_y_tol(d, t))
        if training:
            rec("C_BN_MEAN", "save_mean", _diff(mean, t["mean"]), R.bn_mean_tol(d, t))
            rec("C_BN_RSTD", "save_rstd", _diff(rstd, t["rstd"]), R.bn_rstd_tol(t))
            tm, tv = R.bn_run_tol(d, t)
            rec("C_BN_RUN", "running_mean", _diff(rm, t["run_mean"]), tm)
            rec("C_BN_RUN", "running_var", _diff(rv, t["run_var"]), tv)
            c = d["const_cols"]                             # zero variance: mean exact, rstd = eps^-1/2 to 2 ulp, y = relu(beta) * mask
            want, ulp2 = R.bn_const_rstd()
            assert torch.equal(mean[c], d["x"][0, c]) and float((rstd[c].double() - want).abs().max()) <= ulp2
            assert torch.equal(y[:, c], (t["y"][:, c]).float())
        else:
            assert torch.equal(mean, d["rm"]) and torch.equal(rm, d["rm"]) and torch.equal(rv, d["rv"])
            rec("C_BN_RSTD_EVAL", "save_rstd", _diff(rstd, t["rstd"]), R.bn_rstd_eval_tol(t))
        assert bool((y[t["mrow"] == 0] == 0).all())
        for acc in ((False, True) if masked else (False,)):
            g0 = d["g0"] if acc else None
            dx, dg, db = R.bn_bwd_f32(d, rps, y, mean, rstd, training, relu, masked, g0)
            tg, tb = R.bn_dgb_tol(t, g0)
            a = " accumulate" if acc else ""
            if not acc:
                rec("C_BN_DX", "dx", _diff(dx, t["dx"]), R.bn_dx_tol(d, t))
            rec("C_BN_DGB", "dgamma" + a, _diff(dg, t["dgamma"] + (g0[0].double() if acc else 0)), tg)
            rec("C_BN_DGB", "dbeta" + a, _diff(db, t["dbeta"] + (g0[1].double() if acc else 0)), tb)
    return tuple(out)


@pytest.mark.parametrize("samples,rps,C", R.BN_SHAPES)
def test_bn_bounds(samples, rps, C):
    for _, label, ratio in _bn_records(samples, rps, C):
        _half(label, ratio)


@pytest.mark.parametrize("samples,rps,C", R.BN_SHAPES)
def test_bn_mutations_fail_the_bounds(samples, rps, C):
    """Each deliberately wrong variant lands above the bound that is there to catch it (the factor is printed), on every shape
    where it differs from the kernel at all: dropping the last slice needs two slices, the row-indexed mask more than one row per
    sample.  Measured over BN_SHAPES: fp32 one-pass sums 8e5 .. 1.4e7 x the rstd bound and 1.5e2 .. 1.9e4 x the y bound (mean-1e3
    columns); biased running variance 70 (M = 16384) .. 2.8e6 (M = 2) x; a dropped last slice 2e6 .. 1e9 x the mean bound; a
    row-indexed mask writes non-zeros where y must be exactly 0 (inf) and is 1.2e6 .. 2.4e6 x the bound on the kept part."""
    d = R.bn_inputs(samples, rps, C)
    t = R.bn_truth(samples, rps, C, True, True, True)
    M = samples * rps
    off, live = d["offset_cols"], ~d["const_cols"]
    say = lambda what, r: print(f"  [bn_relpos_host] bn {samples}x{rps}x{C} mutation {what:<34s} err/tol = {r:.3g}")
    y, mean, rstd, rm, rv = R.bn_fwd_f32(d, rps, True, True, True, mutate="fp32_one_pass")
    r1, r2 = R.worst(_diff(rstd, t["rstd"])[off], R.bn_rstd_tol(t)[off]), R.worst(_diff(y, t["y"])[:, off], R.bn_y_tol(d, t)[:, off])
    say("fp32 one-pass sums: rstd", r1); say("fp32 one-pass sums: y", r2)
    assert r1 > 1.0 and r2 > 1.0
    *_, rv = R.bn_fwd_f32(d, rps, True, True, True, mutate="biased_running_var")
    r = R.worst(_diff(rv, t["run_var"])[live], R.bn_run_tol(d, t)[1][live])
    say("biased running variance", r)
    assert r > 1.0
    if R.bn_slicing(M)[0] > 1:
        _, mean, *_ = R.bn_fwd_f32(d, rps, True, True, True, mutate="drop_last_slice")
        r = R.worst(_diff(mean, t["mean"])[live], R.bn_mean_tol(d, t)[live])
        say("last slice dropped: mean", r)
        assert r > 1.0
    if rps > 1:
        y, *_ = R.bn_fwd_f32(d, rps, True, True, True, mutate="mask_by_row")
        kept = t["mrow"] > 0
        r, rk = R.worst(_diff(y, t["y"]), R.bn_y_tol(d, t)), R.worst(_diff(y, t["y"])[kept], R.bn_y_tol(d, t)[kept])
        say("mask indexed by row: y", r); say("mask indexed by row: y (kept part)", rk)
        assert r > 1.0 and rk > 1.0


# ---- relative-position bias --------------------------------------------------------------------------------------------------------
def test_rp_gather_ref_is_torch_indexing():
    for N, H in ((1, 3), (15, 5), (16, 12)):
        nb = R.rp_bins(N)
        table, index = R.rp_table(nb, H), R.rp_index(N, nb)
        bias, bias_t = R.rp_gather_ref(table, index)
        want = table[index.long().reshape(-1)].reshape(N, N, H).permute(2, 0, 1)
        assert torch.equal(bias, want) and torch.equal(bias_t, want.transpose(1, 2))
        assert table.unique().numel() == nb * H                                    # distinct per (bin, head)
        if N > 2:
            assert not torch.equal(bias, bias_t)                                   # the index is not symmetric: a swapped bias_t shows
    table = R.rp_table(5, 2)
    index = torch.tensor([[-3, 0], [7, 4]], dtype=torch.int32)                     # out of range: clamped, as the kernel does
    assert torch.equal(R.rp_gather_ref(table, index)[0], table[torch.tensor([[0, 0], [4, 4]])].permute(2, 0, 1))


def test_rp_index_plants_the_bin_counts():
    for N in (15, 16, 72, 73, 256):
        nb = R.rp_bins(N)
        cnt = np.bincount(R.rp_index(N, nb).numpy().reshape(-1), minlength=nb)
        assert tuple(cnt[:5]) == R.RP_PLANTED and len(cnt) == nb
        if N >= 72:
            assert cnt[5] == R.RP_BIG_BIN > 4096
    assert all((72 * 72 * h) % 4 == 0 for h in (1, 3, 4, 5, 12)) and (15 * 15 * 3) % 4 != 0 and (73 * 73 * 3) % 4 != 0
    assert R.rp_chunk_sum_path(2, 4, 16) and not R.rp_chunk_sum_path(2, 3, 15) and not R.rp_chunk_sum_path(1, 4, 16)
    assert not R.rp_chunk_sum_path(2, 4, 16, aligned=False)


def test_rp_reduce_ref_is_the_adjoint_of_the_gather():
    """np.add.at over the slab == autograd of <table[index], G> in float64; the CSR restatement lists every in-range position once,
    ascending within its bin, and drops the rest."""
    N, H, chunks, nb = 15, 3, 2, 40
    index = R.rp_index(N, nb)
    slab = R.rp_slab(chunks, H, N, integer=False)
    table = R.rp_table(nb, H).double().requires_grad_(True)
    bias = table[index.long().reshape(-1)].reshape(N, N, H).permute(2, 0, 1)
    (bias[None] * slab.double()).sum().backward()
    got, mag = R.rp_reduce_ref(slab, index, nb)
    torch.testing.assert_close(got, table.grad, rtol=1e-13, atol=1e-13)
    assert bool((mag >= got.abs() - 1e-12).all())
    bad = index.clone()
    bad[0, 1], bad[3, 2], bad[14, 14] = -1, nb, nb + 5
    pos, off = R.rp_csr_ref(bad, nb)
    flat = bad.numpy().reshape(-1)
    assert len(pos) == N * N - 3 and off[0] == 0 and off[-1] == len(pos) and bool((np.diff(off) >= 0).all())
    for b in range(nb):
        seg = pos[off[b]:off[b + 1]]
        assert bool((flat[seg] == b).all()) and bool((np.diff(seg) > 0).all())
    got_bad, _ = R.rp_reduce_ref(slab, bad, nb)
    drop = torch.zeros(nb, H, dtype=torch.float64)
    for (i, j) in ((0, 1), (3, 2), (14, 14)):
        drop[int(index[i, j])] += slab.double()[:, :, i, j].sum(0)
    torch.testing.assert_close(got_bad, got - drop, rtol=1e-13, atol=1e-13)


@functools.lru_cache(maxsize=None)
def _rp_records(N, H, chunks):
    nb = R.rp_bins(N)
    index = R.rp_index(N, nb)
    out = []
    for aligned in ((True, False) if (N, H, chunks) == (16, 4, 2) else (True,)):
        path = R.rp_chunk_sum_path(chunks, H, N, aligned)
        si = R.rp_slab(chunks, H, N, integer=True)
        want, _ = R.rp_reduce_ref(si, index, nb)
        assert torch.equal(R.rp_reduce_f32(si, index, nb, path).double(), want)            # integer slab: exact in any order
        sr = R.rp_slab(chunks, H, N, integer=False)
        want, mag = R.rp_reduce_ref(sr, index, nb)
        d0 = R.rp_dtable0(nb, H)
        tag = f"relpos reduce N={N} H={H} chunks={chunks} {'chunk_sum' if path else 'in-kernel loop'}"
        out.append(("C_RP_SUM", tag, R.worst(_diff(R.rp_reduce_f32(sr, index, nb, path), want), R.rp_reduce_tol(index, nb, chunks, mag))))
        got = R.rp_reduce_f32(sr, index, nb, path, d0)
        out.append(("C_RP_SUM", tag + " accumulate", R.worst(_diff(got, want + d0.double()), R.rp_reduce_tol(index, nb, chunks, mag, want + d0.double()))))
        empty = torch.from_numpy(np.diff(R.rp_csr_ref(index, nb)[1]) == 0)
        assert bool(empty.any()) and torch.equal(got[empty], d0[empty])
    return tuple(out)


@pytest.mark.parametrize("N,H,chunks", R.RP_REDUCE_CASES)
def test_rp_reduce_bounds(N, H, chunks):
    for _, label, ratio in _rp_records(N, H, chunks):
        _half(label, ratio)


def test_constants_are_minimal():
    """Every bound is proportional to its constant, so with the constant one smaller the worst ratio grows by C / (C - 1): it must
    then exceed one half somewhere on the GPU tests' inputs.  (A constant of 1 has nothing below it.)"""
    worst = {}
    for rec in [r for s in R.BN_SHAPES for r in _bn_records(*s)] + [r for s in R.RP_REDUCE_CASES for r in _rp_records(*s)]:
        worst[rec[0]] = max(worst.get(rec[0], 0.0), rec[2])
    assert set(worst) == {k for k in vars(R) if k.startswith("C_")}
    for k, r in sorted(worst.items()):
        c = getattr(R, k)
        print(f"  [bn_relpos_host] {k:<16s} = {c}: worst err/tol = {r:.3f}" + (f", {r * c / (c - 1):.3f} with {c - 1}" if c > 1 else ""))
        assert isinstance(c, int) and c >= 1 and r <= 0.5
        assert c == 1 or r * c / (c - 1) > 0.5, f"{k} = {c} is not minimal"


# ---- patchify ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,side,p", R.PATCHIFY_SHAPES)
def test_patchify_ref_is_unfold(B, C, side, p):
    """The rearrangement == torch.nn.functional.unfold(x, p, stride=p) in (c, dy, dx) column order, bit for bit (special values
    included: NaN payloads travel); the bf16 reference is torch's own rounding, which rows_ref.cast_bf16_ref restates."""
    x = R.patchify_input(B, C, side)
    want = torch.nn.functional.unfold(x, p, stride=p).transpose(1, 2).reshape(B * (side // p) ** 2, C * p * p)
    got = R.patchify_ref(x, p)
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
    assert RR.bf16_same(RR.cast_bf16_ref(got.reshape(-1)), got.bfloat16().view(torch.int16).numpy().reshape(-1))


def test_patchify_shapes_reach_the_edges():
    s = R.PATCHIFY_SHAPES
    assert any(B == 1 for B, *_ in s) and any(C == 1 for _, C, *_ in s) and any(p == side and p % 4 == 0 for *_, side, p in s)
    assert any(p == side and p % 4 for *_, side, p in s) and any(p == 4 for *_, p in s) and any(p == 1 for *_, p in s)
    (B, C, S, p), (B2, C2, S2, p2) = R.PATCHIFY_BIG
    assert p % 4 == 0 and B * C * S * S // 4 > 4096 * 256 and p2 % 4 != 0 and S2 % p2 == 0 and B2 * C2 * S2 * S2 > 4096 * 256
    have = set(R.patchify_input(2, 4, 64).numpy().view(np.uint32).reshape(-1).tolist())
    assert set(RR.CAST_SPECIALS.tolist()) <= have
