"""GPU: the fused launches between the blocks (ops.PoolNormFn, the bf16 gradient copies of the final norm and of block 0's regrouped
rows) against the separate launches they replace.  Every comparison is bitwise: the fused row kernels run the arithmetic of
token_pool_*_kernel, layernorm_*_kernel<float> and cast_bf16_kernel in the same order."""
import ctypes as C

import pytest
import torch

from util import model_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5


def _ops():
    from deepmerge_amd import ops
    return ops


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(DEV)


def _affine(Cc, seed):
    return 1.0 + 0.1 * _rand((Cc,), seed), 0.1 * _rand((Cc,), seed + 1)


def _pool_then_norm(ops, x, gamma, beta, S, side):
    lib, st = ops._lib.lib(), ops._stream()
    B, N, Cc = x.shape
    pooled = torch.empty((B, S * (side // 2) ** 2, Cc), device=DEV)
    ops.check(lib.dm_token_pool_fwd(x.data_ptr(), pooled.data_ptr(), B, S, side, Cc, st), "dm_token_pool_fwd")
    y, mean, rstd = ops.layernorm_fwd(pooled, gamma, beta, EPS, torch.float32)
    return pooled, y, mean, rstd


POOL_SHAPES = [(2, 4, 8, 768), (3, 3, 4, 768), (1, 4, 2, 768)]


@pytest.mark.parametrize("B,S,side,Cc", POOL_SHAPES)
def test_pool_layernorm_fwd_is_pool_then_layernorm(B, S, side, Cc):
    ops = _ops()
    x = _rand((B, S * side * side, Cc), 1)
    gamma, beta = _affine(Cc, 2)
    want = _pool_then_norm(ops, x, gamma, beta, S, side)
    n = S * (side // 2) ** 2
    pooled, y = torch.empty((B, n, Cc), device=DEV), torch.empty((B, n, Cc), device=DEV)
    mean, rstd = torch.empty(B * n, device=DEV), torch.empty(B * n, device=DEV)
    ops.check(ops._lib.lib().dm_pool_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), pooled.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                                   rstd.data_ptr(), B, S, side, Cc, EPS, ops._stream()), "dm_pool_layernorm_fwd")
    for name, a, b in zip(("pooled", "y", "mean", "rstd"), (pooled, y, mean, rstd), want):
        assert torch.equal(a, b), name
    # and through the autograd Function the model calls
    assert ops.pool_norm_fused(x, "bf16") and ops.pool_norm_fused(x, "fp32") and not ops.pool_norm_fused(x, "bf16x3")
    assert torch.equal(ops.pool_norm(x, gamma, beta, EPS, S, side, "bf16"), want[1])


def test_uncovered_width_keeps_the_separate_launches():
    """C = 260 is not a width the fused kernels hold: the library refuses it, ops.pool_norm runs TokenPoolFn + LayerNormFn."""
    ops = _ops()
    B, S, side, Cc = 2, 3, 4, 260
    assert not ops._lib.lib().dm_pool_layernorm_ok(Cc) and ops._lib.lib().dm_pool_layernorm_ok(768)
    x = _rand((B, S * side * side, Cc), 3).requires_grad_(True)
    gamma, beta = _affine(Cc, 4)
    assert not ops.pool_norm_fused(x, "bf16")
    n = S * (side // 2) ** 2
    bufs = [torch.empty((B, n, Cc), device=DEV) for _ in range(2)] + [torch.empty(B * n, device=DEV) for _ in range(2)]
    with pytest.raises((ValueError, RuntimeError), match="768"):
        ops.check(ops._lib.lib().dm_pool_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), *[t.data_ptr() for t in bufs],
                                                       B, S, side, Cc, EPS, ops._stream()), "dm_pool_layernorm_fwd")
    want = _pool_then_norm(ops, x.detach(), gamma, beta, S, side)
    y = ops.pool_norm(x, gamma, beta, EPS, S, side, "bf16")
    assert torch.equal(y, want[1])
    go = _rand(y.shape, 5)
    y.backward(go)
    r = ops.layernorm_bwd(go, want[0], gamma, want[2], want[3])
    dx = torch.empty_like(x)
    ops.check(ops._lib.lib().dm_token_pool_bwd(r[0].data_ptr(), dx.data_ptr(), B, S, side, Cc, ops._stream()), "dm_token_pool_bwd")
    assert torch.equal(x.grad, dx)


def _separate_bwd(ops, dy, pooled, gamma, mean, rstd, dg, db, accumulate, B, S, side, Cc):
    """layernorm_bwd, token_pool_bwd, dm_cast: what the fused backward replaces."""
    r = ops.layernorm_bwd(dy, pooled, gamma, mean, rstd, dgamma=dg, dbeta=db, accumulate=accumulate)
    dx = torch.empty((B, S * side * side, Cc), device=DEV)
    ops.check(ops._lib.lib().dm_token_pool_bwd(r[0].data_ptr(), dx.data_ptr(), B, S, side, Cc, ops._stream()), "dm_token_pool_bwd")
    return dx, ops.cast(dx, torch.bfloat16)


@pytest.mark.parametrize("want_lp", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("B,S,side,Cc", POOL_SHAPES)
def test_pool_layernorm_bwd_is_layernorm_pool_cast(B, S, side, Cc, accumulate, want_lp):
    ops = _ops()
    lib = ops._lib.lib()
    x = _rand((B, S * side * side, Cc), 11)
    gamma, beta = _affine(Cc, 12)
    pooled, y, mean, rstd = _pool_then_norm(ops, x, gamma, beta, S, side)
    dy = _rand(y.shape, 13)
    seed_g, seed_b = _rand((Cc,), 14), _rand((Cc,), 15)
    dg0, db0 = seed_g.clone(), seed_b.clone()
    dx0, lp0 = _separate_bwd(ops, dy, pooled, gamma, mean, rstd, dg0, db0, accumulate, B, S, side, Cc)
    dg1, db1 = seed_g.clone(), seed_b.clone()
    dx1 = torch.full_like(dx0, float("nan"))
    lp1 = torch.full_like(lp0, float("nan")) if want_lp else None
    part = torch.empty(lib.dm_layernorm_bwd_partial_floats(Cc), device=DEV)
    ops.check(lib.dm_pool_layernorm_bwd(dy.data_ptr(), pooled.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx1.data_ptr(),
                                        ops._ptr(lp1), dg1.data_ptr(), db1.data_ptr(), int(accumulate), part.data_ptr(), None, B, S, side, Cc,
                                        ops._stream()), "dm_pool_layernorm_bwd")
    assert torch.equal(dx1, dx0)
    assert torch.equal(dg1, dg0) and torch.equal(db1, db0)
    if want_lp:
        assert torch.equal(lp1.view(torch.int16), lp0.view(torch.int16))
    # the partial rows alone (the deferred form): same rows as dm_layernorm_bwd_partials leaves
    n_a, n_b = C.c_int32(0), C.c_int32(0)
    part_b = torch.empty_like(part)
    scratch = torch.empty_like(pooled)
    rows = pooled.numel() // Cc
    ops.check(lib.dm_layernorm_bwd_partials(dy.data_ptr(), ops._dt(dy), pooled.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None,
                                            scratch.data_ptr(), None, part_b.data_ptr(), rows, Cc, C.byref(n_b), ops._stream()), "dm_layernorm_bwd_partials")
    ops.check(lib.dm_pool_layernorm_bwd(dy.data_ptr(), pooled.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx1.data_ptr(),
                                        None, None, None, 0, part.data_ptr(), C.byref(n_a), B, S, side, Cc, ops._stream()), "dm_pool_layernorm_bwd")
    assert n_a.value == n_b.value > 0
    assert torch.equal(part[:n_a.value * 2 * Cc], part_b[:n_b.value * 2 * Cc])


class _Probe(torch.autograd.Function):
    """Identity that keeps the gradient object its consumer hands back (what the next node's backward would receive)."""
    seen = None

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        _Probe.seen = g
        return g


def _sunk(t):
    """A parameter with a gradient sink, as trainer.FlatParams attaches them."""
    p = torch.nn.Parameter(t.clone())
    p._dm_grad_sink = torch.zeros_like(t)
    return p


@pytest.mark.parametrize("B,S,side,Cc", POOL_SHAPES[:2])
def test_pool_norm_backward_deferred_equals_immediate(B, S, side, Cc, monkeypatch):
    """PoolNormFn in a real backward(): two uses of one norm whose reductions are queued, against the immediate launches and against
    the separate Functions; the bf16 copy rides on the gradient."""
    ops = _ops()
    x0 = _rand((B, S * side * side, Cc), 21)
    gam, bet = _affine(Cc, 22)

    def run(defer, fused):
        monkeypatch.setattr(ops, "_DEFER_REDUCTIONS", defer)
        monkeypatch.setattr(ops, "_FUSED_GLUE", fused)
        g, b = _sunk(gam), _sunk(bet)
        x = x0.clone().requires_grad_(True)
        y = ops.pool_norm(_Probe.apply(x), g, b, EPS, S, side, "bf16") + ops.pool_norm(_Probe.apply(x * 0.5), g, b, EPS, S, side, "bf16")
        y.backward(_rand(y.shape, 23))
        ops.flush_reductions()
        return x.grad.clone(), g._dm_grad_sink.clone(), b._dm_grad_sink.clone(), _Probe.seen

    ref = run(False, False)
    assert getattr(ref[3], "_dm_lp_copy", None) is None
    for defer in (False, True):
        got = run(defer, True)
        for name, a, b in zip(("dx", "dgamma", "dbeta"), got, ref):
            assert torch.equal(a, b), (name, defer)
        lp, tag = got[3]._dm_lp_copy
        assert tag == ops._grad_tag(got[3]) and torch.equal(lp.view(torch.int16), ops.cast(got[3], torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize("dy_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S,T,Cc", [(3, 4, 64, 768), (2, 3, 4, 768), (3, 3, 5, 768), (2, 3, 5, 260)])
def test_regrouped_bf16_rows_are_a_permutation_of_the_copy(B, S, T, Cc, dy_dtype):
    """(3, 3, 5): 45 rows, not a multiple of the 4 rows a workgroup takes per round; 260 columns: the lane-predicated instance."""
    ops = _ops()
    rows = B * S * T
    x = _rand((rows, Cc), 31)
    gamma, beta = _affine(Cc, 32)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, beta, EPS, torch.float32)
    dy = _rand((rows, Cc), 33).to(dy_dtype)
    dres = _rand((rows, Cc), 34)
    dx0, lp0, dg0, db0 = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dres=dres, want_lp=True)
    dx1, lp1, dg1, db1 = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dres=dres, want_lp=True, regroup=(S, T))
    assert torch.equal(dx1, dx0) and torch.equal(dg1, dg0) and torch.equal(db1, db0)
    assert tuple(lp1.shape) == (S, B, T, Cc)
    want = lp0.view(B, S, T, Cc).transpose(0, 1).contiguous()
    assert torch.equal(lp1.view(torch.int16), want.view(torch.int16))
    with pytest.raises(ValueError):
        ops.layernorm_bwd(dy, x, gamma, mean, rstd, want_lp=True, regroup=(S, T + 1))


def test_final_norm_hands_its_consumer_the_bf16_copy(monkeypatch):
    ops = _ops()
    x = _rand((2, 16, 768), 41).requires_grad_(True)
    gamma, beta = _affine(768, 42)
    go = _rand((2, 16, 768), 43)
    ops.LayerNormFn.apply(_Probe.apply(x), gamma, beta, EPS, torch.float32, torch.bfloat16).backward(go)
    g = _Probe.seen
    lp, tag = g._dm_lp_copy
    assert tag == ops._grad_tag(g) and torch.equal(lp.view(torch.int16), ops.cast(g, torch.bfloat16).view(torch.int16))
    dx = x.grad.clone()
    for grad_lp in (None, torch.float32):           # not asked for, or an fp32 consumer: no copy, same dx
        x.grad = None
        ops.LayerNormFn.apply(_Probe.apply(x), gamma, beta, EPS, torch.float32, grad_lp).backward(go)
        assert getattr(_Probe.seen, "_dm_lp_copy", None) is None and torch.equal(x.grad, dx)


def test_training_step_is_bitwise_the_same_with_the_switch_off(monkeypatch):
    """Depth [1, 1, 1], 4 scales x 4 channels, 2 pairs, bf16: one PairTrainer.step with the fused launches and one without."""
    ops = _ops()
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    from deepmerge_amd.trainer import PairTrainer
    scales, in_c = (32, 64, 128, 256), 4
    left, ld, right, rd, flag = model_inputs("glue_fused", scales, in_c, 4)      # (the recipe builds four pairs: the first two)
    batch = ([t[:2].to(DEV) for t in left], ld[:2].to(DEV), [t[:2].to(DEV) for t in right], rd[:2].to(DEV), flag[:2].to(DEV))
    calls = {"regroup": 0, "pool": 0}
    real_bwd, real_fused = ops.layernorm_bwd, ops.pool_norm_fused

    def counting_bwd(*a, **kw):
        calls["regroup"] += kw.get("regroup") is not None
        return real_bwd(*a, **kw)

    def counting_fused(*a):
        calls["pool"] += real_fused(*a)
        return real_fused(*a)
    monkeypatch.setattr(ops, "layernorm_bwd", counting_bwd)
    monkeypatch.setattr(ops, "pool_norm_fused", counting_fused)

    def run(fused):
        monkeypatch.setattr(ops, "_FUSED_GLUE", fused)
        torch.manual_seed(7)
        net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=list(scales), depth=[1, 1, 1], in_c=in_c, numerics="bf16").to(DEV).train()
        tr = PairTrainer(net, lr=1e-4)
        loss = tr.step(*batch)
        return float(loss), tr.fp.grad.clone(), tr.fp.flat.clone()

    off = run(False)
    assert calls == {"regroup": 0, "pool": 0}
    on = run(True)
    assert calls == {"regroup": 1, "pool": 2}      # block 0 of stage 0, for the patch embeds; the two transitions
    assert on[0] == off[0]
    assert torch.equal(on[1], off[1]) and torch.equal(on[2], off[2])
    assert bool(off[1].abs().max() > 0)
