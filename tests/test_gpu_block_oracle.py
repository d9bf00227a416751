"""GPU: every gradient of the fused block (ops.BlockFn), per tensor, on every route, against the fp64 restatement of tests/block_ref.py.

Gate A, per tensor t of {y, dx, every parameter gradient, the table gradient}:  err[t] = ||kernel[t] - truth[t]|| / ||truth[t]||
  * "bf16":            err[t] <= 2 * yard[t], yard[t] = the restatement-with-rounding-points' own distance to truth for that tensor.
                       What remains between kernel and restatement is fp32 accumulation order plus sparse one-ulp rounding flips: an
                       independent error no larger than the yardstick itself, so sqrt(2) is expected and 2 leaves room.
  * "fp32", "bf16x3":  err[t] <= 1e-3, the project's parity gate (GATE in test_gpu_modules.py), here per tensor.
A wholly wrong tensor (a bias that lost a contribution, swapped gamma / beta gradients, a table gradient scaled by 2) is an error of
order 1: two to three orders of magnitude over either bound.  Measured ratios: profiles/block_grad_errors.txt.

Cases (tests/block_ref.py CASES) are the smallest shapes that reach each route; every case asserts its route with the project's own
predicates (ROUTES below).  No DM_* environment switch is set anywhere in this file: routes B are reached through the Python routing
constants ops._WGRAD_GROUP_TOKENS / ops._WGRAD_PAIR.
"""
import pytest
import torch

import block_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 1e-3
MODES = ("fp32", "bf16", "bf16x3")

# case -> (relpos_inkernel for bf16 tensors, attention_split_ok, plane pairs under "bf16x3").  What each row means:
#   s256   B * heads = 24 is below the batch rule of the table-reading kernels: bf16 gathers dense bias rows (register kernels);
#          "bf16x3": split attention reading the table + plane pairs
#   s192   the three-scale table, M = 576 a multiple of 64
#   s48    gathered dense bias, register attention in every mode; M = 96: no plane pairs
#   n256   M * C^2 = 2^24 exactly: ON the _SPLIT_MIN_WORK boundary, so plane pairs; 256-wide LayerNorm rows
#   v197   no table, ragged key tail and GEMM rows; "bf16x3": split attention WITHOUT plane pairs (M = 591)
#   v50    everything ragged, 192-wide rows, nothing split
#   s256b8 B * heads = 96: the table read inside the bf16 attention kernels (forward, dQ, dK / dV)
#   v197b8 B * heads = 96: the persistent bias-free bf16 attention kernels at a ragged N
ROUTES = {
    "s256": (False, True, True), "s192": (False, True, True), "s48": (False, False, False), "n256": (False, True, True),
    "v197": (False, True, False), "v50": (False, False, False), "s256b8": (True, True, True), "v197b8": (False, True, False),
}
BF16_ONLY = ("s256b8", "v197b8")      # the batch rule they are here for exists in the bf16 kernels' plan only

_ref = {}


def ops():
    from deepmerge_amd import ops as o
    return o


def shape_of(name):
    kind, C, heads, tok, B = R.CASES[name]
    return kind, C, heads, (tok if kind == "cross" else None), B, R.case_tokens(name)


def plane_pairs(name):
    """The `planes` condition of BlockFn.forward for fp32 tensors inside a "bf16x3" scope."""
    o = ops()
    _, C, _, _, B, N = shape_of(name)
    M, Hd = B * N, 4 * C
    return bool(o.planes_ok(M, C) and o.planes_ok(M, Hd) and o.planes_ok(Hd, C) and C <= o._PAIR_LN_MAX_COLS and M * C * C >= o._SPLIT_MIN_WORK)


def assert_route(name):
    o = ops()
    _, C, heads, cube, B, N = shape_of(name)
    got = (bool(o.relpos_inkernel(B, N, heads, C // heads, cube, torch.bfloat16)), bool(o.attention_split_ok(B, N, heads, C // heads, cube)),
           plane_pairs(name))
    assert got == ROUTES[name], f"{name}: (table in kernel, split attention, plane pairs) = {got}, the case was chosen for {ROUTES[name]}"
    assert not o.relpos_inkernel(B, N, heads, C // heads, cube, torch.float32)      # fp32 tensors never read the table in the plain kernels


def reference(key, params, x, go, forward):
    """(truth, yardstick per tensor) of a graph, computed once per key and shared by every mode and route."""
    if key not in _ref:
        truth = R.evaluate(lambda P, X: forward(P, X, False), params, x, go)
        pts = R.evaluate(lambda P, X: forward(P, X, True), params, x, go)
        _ref[key] = (truth, {k: R.rel_l2(pts[k], truth[k]) for k in truth})
    return _ref[key]


def block_reference(name):
    heads = R.CASES[name][2]
    p, x, go = R.case_data(name)
    return (p, x, go) + reference(("block", name), p, x, go, lambda P, X, pts: R.block(P, X, heads, pts))


def build(name, mode, params, drop_path_ratio=0.):
    kind, C, heads, cube, _, _ = shape_of(name)
    if kind == "cross":
        from deepmerge_amd.nets.ShfitScaleFormer import CrossScaleBlock
        m = CrossScaleBlock(dim=C, num_heads=heads, cube_size=list(cube), drop_path_ratio=drop_path_ratio, numerics=mode)
    else:
        from deepmerge_amd.vit_model import Block
        m = Block(dim=C, num_heads=heads, qkv_bias=True, drop_path_ratio=drop_path_ratio, numerics=mode)
    m.load_state_dict(params, strict=True)
    return m.to(DEV)


def collect(y, X, named_params):
    res = {"y": y.detach(), "dx": X.grad}
    for n, p in named_params:
        assert p.grad is not None, f"no gradient for {n}"
        res["d_" + n] = p.grad
    return res


def run(module, x, go):
    """y and every gradient through plain .backward() on parameters without a .grad."""
    for p in module.parameters():
        p.grad = None
    X = x.to(DEV).requires_grad_(True)
    y = module(X)
    (y * go.to(DEV)).sum().backward()
    return collect(y, X, module.named_parameters())


def gate(tag, case, mode, got, truth, yard):
    assert set(got) == set(truth), (sorted(got), sorted(truth))
    bad = []
    for k in truth:
        err = R.rel_l2(got[k], truth[k])
        print(f"{tag} {case} {mode} {k}: err {err:.3e} yard {yard[k]:.3e} err/yard {err / yard[k]:.2f}")
        limit = 2.0 * yard[k] if mode == "bf16" else GATE
        if not err <= limit:        # (a NaN fails too)
            bad.append((k, err, limit))
    assert not bad, f"{case} {mode}: over the gate: {bad}"


def same_bits(a, b, keys=None):
    return [k for k in (keys or a) if not torch.equal(a[k], b[k])]


# ---- A: per-tensor gate, default routing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [(n, m) for n in R.CASES for m in MODES if n not in BF16_ONLY or m == "bf16"])
def test_every_tensor_of_the_block(name, mode):
    assert_route(name)
    p, x, go, truth, yard = block_reference(name)
    gate("BLOCK", name, mode, run(build(name, mode, p), x, go), truth, yard)


# ---- B: the three issue routes of the weight gradients -------------------------------------------------------------------------------------
WGRAD_ROUTES = (("grouped", {}, 4), ("late", {"_WGRAD_GROUP_TOKENS": 0}, 2), ("immediate", {"_WGRAD_GROUP_TOKENS": 0, "_WGRAD_PAIR": False}, 0))


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("name", ["s256", "v197"])
def test_weight_gradient_routes(name, mode, monkeypatch):
    """Grouped launch (default), the proj + qkv pair in one sliced launch, every weight gradient issued at once: each passes gate A (the
    bias column sums ride on whichever launch carries them; the LayerNorm reductions are the same on all three), and the dgrad chain
    -- dx, the table gradient, y -- does not depend on when the weight gradients are issued: bit-identical."""
    o = ops()
    assert_route(name)
    p, x, go, truth, yard = block_reference(name)
    M = x.shape[0] * x.shape[1]
    assert 0 < M <= o._WGRAD_GROUP_TOKENS and o._WGRAD_PAIR      # the defaults this test starts from
    fused = mode == "bf16" or plane_pairs(name)      # (fp32 tensors without plane pairs: BlockFn issues every weight gradient at once)
    module = build(name, mode, p)
    real = o.gemm_grouped
    results = {}
    for route, settings, n_grouped in WGRAD_ROUTES:
        calls = []
        with monkeypatch.context() as mp:
            for k, v in settings.items():
                mp.setattr(o, k, v)
            mp.setattr(o, "gemm_grouped", lambda c: (calls.append(len(c)), real(c))[1])
            results[route] = run(module, x, go)
        assert calls == ([n_grouped] if (fused and n_grouped) else []), (route, calls)
        gate("ROUTE-" + route, name, mode, results[route], truth, yard)
    chain = [k for k in ("y", "dx", "d_attn.relative_position_bias_table") if k in truth]
    for route in ("late", "immediate"):
        assert same_bits(results["grouped"], results[route], chain) == [], route


# ---- C: the hand-over between blocks -------------------------------------------------------------------------------------------------------
def two_block_reference(side, shared):
    name = "s256"
    heads = R.CASES[name][2]
    p, x, go = R.case_data(name, blocks=("b1.", "b2."))
    c = torch.randn(x.shape, generator=torch.Generator().manual_seed(77), dtype=torch.float32)
    fwd = lambda P, X, pts: R.two_blocks(P, X, heads, pts, side=c.double() if side else None, shared=shared)
    return (p, x, go, c) + reference(("two", side, shared), p, x, go, fwd)


def run_two(b1, b2, x, go, c=None, side_first=False, hook=False, transpose=False, counters=None):
    """b2(b1(x)); c: the middle activation also feeds (x_mid * c).sum(), created before or after b2; hook: the middle gradient is replaced
    by a clone (no attribute reaches b1); transpose: the loss reads b2's result through a transpose (non-contiguous gradient into b2)."""
    mods = [b1] if b2 is b1 else [b1, b2]
    for m in mods:
        for q in m.parameters():
            q.grad = None
    X = x.to(DEV).requires_grad_(True)
    mid = b1(X)
    if hook:
        mid.register_hook(lambda g: g.clone())
    extra = (mid * c.to(DEV)).sum() if (c is not None and side_first) else None
    y = b2(mid)
    if c is not None and not side_first:
        extra = (mid * c.to(DEV)).sum()
    g = go.to(DEV)
    loss = (y.transpose(1, 2) * g.transpose(1, 2).contiguous()).sum() if transpose else (y * g).sum()
    if extra is not None:
        loss = loss + extra
    if counters is not None:
        counters.clear()
    loss.backward()
    named = [("b1." + n, q) for n, q in b1.named_parameters()]
    if b2 is not b1:
        named += [("b2." + n, q) for n, q in b2.named_parameters()]
    return collect(y, X, named)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_handover_between_blocks(mode, monkeypatch):
    """The bf16 copy (`_dm_lp_copy`) / plane pair (`_dm_planes`) of dx that one block's backward attaches for the previous block's:
    the previous block must compute exactly what it computes from a gradient without attributes (a hook hands it a clone), with one
    consumer, with a second consumer created before or after the block, and with a non-contiguous gradient at the top.  With one
    consumer the attached copy IS used (no cast / split of its own in b1's backward)."""
    o = ops()
    assert_route("s256")
    assert plane_pairs("s256")
    refs = {side: two_block_reference(side, False) for side in (False, True)}
    p, x, go, c = refs[False][:4]
    b1, b2 = build("s256", mode, R.strip(p, "b1.")), build("s256", mode, R.strip(p, "b2."))
    # what a backward pass does itself to get its operand: bf16 casts its incoming gradient, "bf16x3" splits it into planes
    made = []
    probe = "_as_operand" if mode == "bf16" else "split_planes"
    real = getattr(o, probe)
    monkeypatch.setattr(o, probe, lambda *a, **k: (made.append(1), real(*a, **k))[1])
    for transpose in (False, True):
        # 1. one consumer
        plain = run_two(b1, b2, x, go, hook=True, transpose=transpose, counters=made)
        n_plain = len(made)
        attr = run_two(b1, b2, x, go, transpose=transpose, counters=made)
        n_attr = len(made)
        print(f"HANDOVER {mode} transpose={transpose}: operand copies made in backward: {n_plain} with a clone, {n_attr} with the attribute")
        assert same_bits(plain, attr) == []
        assert (n_plain, n_attr) == (2, 1)            # b2 always makes its own (the loss hands it a plain tensor); b1 only without the attribute
        truth, yard = refs[False][4:]
        gate("HANDOVER-1", "s256x2", mode, attr, truth, yard)
        # 2. two consumers, the side one created before / after b2
        truth, yard = refs[True][4:]
        for side_first in (True, False):
            plain = run_two(b1, b2, x, go, c=c, side_first=side_first, hook=True, transpose=transpose, counters=made)
            attr = run_two(b1, b2, x, go, c=c, side_first=side_first, transpose=transpose, counters=made)
            print(f"HANDOVER {mode} transpose={transpose} side_first={side_first}: operand copies made in backward: {len(made)}")
            assert same_bits(plain, attr) == [], (transpose, side_first)
            gate(f"HANDOVER-2{'a' if side_first else 'b'}", "s256x2", mode, attr, truth, yard)


def test_stale_copy_is_refused():
    """The rule itself, without relying on what the engine happens to do: a gradient that was added to in place after the copy was
    attached must not be read through the copy."""
    o = ops()
    p, x, go = R.case_data("s48")
    results = {}
    for how in ("none", "stale", "current"):
        b = build("s48", "bf16", p)
        X = x.to(DEV).requires_grad_(True)
        y = b(X)
        g = go.to(DEV).clone()
        wrong = torch.zeros_like(g, dtype=torch.bfloat16)            # a copy that is NOT the rounding of g
        if how != "none":
            g._dm_lp_copy = (wrong, o._grad_tag(g))
        if how == "stale":
            g.add_(0.0)                                              # same bytes, same values, _version bumped: the tag no longer matches
        y.backward(g)
        results[how] = collect(y, X, b.named_parameters())
    assert same_bits(results["none"], results["stale"]) == []
    # (and the attribute on this very tensor object IS what the block reads while the tag matches: the wrong copy shows)
    assert "d_mlp.fc2.weight" in same_bits(results["none"], results["current"])


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_block_applied_twice_with_and_without_sinks(mode):
    """b(b(x)) with shared weights: autograd sums the two contributions of every parameter (gate A against the shared-weight truth); with
    the trainer's gradient sinks and first-write state the first contribution stores over a NaN-filled buffer and the second adds."""
    from deepmerge_amd.trainer import FlatParams
    p, x, go, _, truth, yard = two_block_reference(False, True)
    p1 = R.strip(p, "b1.")
    b = build("s256", mode, p1)
    free = run_two(b, b, x, go)
    gate("TWICE", "s256x2", mode, free, truth, yard)

    class Twice(torch.nn.Module):
        _dm_first_write_blocks = True

        def __init__(self, blk):
            super().__init__()
            self.b = blk

        def forward(self, t):
            return self.b(self.b(t))

    tw = Twice(build("s256", mode, p1))
    fp = FlatParams(tw, lp_mirror=(mode == "bf16"), first_write=True, pair_mirror=(mode == "bf16x3"))
    assert len(fp.tracked) == 13 and fp._zero_ranges == []
    fp.zero_grad()
    fp.grad.fill_(float("nan"))
    X = x.to(DEV).requires_grad_(True)
    y = tw(X)
    (y * go.to(DEV)).sum().backward()
    assert fp.finish_grads() == 0
    torch.testing.assert_close(y.detach(), free["y"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(X.grad, free["dx"], rtol=1e-5, atol=1e-6)
    for n, q in tw.b.named_parameters():
        assert q.grad.data_ptr() == q._dm_grad_sink.data_ptr()
        torch.testing.assert_close(q.grad, free["d_b1." + n], rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")


# ---- D: forward without gradients --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["s256", "s48", "v197", "v50"])
def test_forward_without_gradients(name, mode):
    """torch.no_grad(): fc1 runs the DM_EPI_GELU epilogue, not DM_EPI_GELU_GRAD.  Both form GELU as x * cdf from the same function
    (csrc/dm_gemm_common.h: dm_gelu_fast(v) == v * cdf of dm_gelu_parts_fast; dm_gelu in the fp32 instances), so y is the training y."""
    p, x, go, truth, yard = block_reference(name)
    m = build(name, mode, p)
    X = x.to(DEV)
    with torch.no_grad():
        y_inf = m(X)
    y_train = m(X.clone().requires_grad_(True)).detach()
    assert not y_inf.requires_grad
    gate("NOGRAD", name, mode, {"y": y_inf}, {"y": truth["y"]}, yard)
    same = torch.equal(y_inf, y_train)
    print(f"NOGRAD {name} {mode}: y equals the training-mode y bit for bit: {same}")
    assert same


# ---- E: the separate-node forms in bf16 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["attention", "mlp"])
@pytest.mark.parametrize("name", ["s48", "s256"])
def test_separate_nodes_in_bf16(name, which):
    """CrossScaleAttention / Mlp with numerics="bf16": LinearFn + AttentionFn + LinearFn and MlpFn behind a cast node, the forms the
    stochastic-depth path trains through, against the matching sub-graphs of the restatement."""
    from deepmerge_amd.nets.ShfitScaleFormer import CrossScaleAttention, Mlp
    _, C, heads, cube, _, _ = shape_of(name)
    p, x, go = R.case_data(name)
    if which == "attention":
        sub = R.strip(p, "attn.")
        m = CrossScaleAttention(dim=C, num_heads=heads, cube_size=list(cube), qkv_bias=True, numerics="bf16")
        fwd = lambda P, X, pts: R.attention_module(P, X, heads, pts)
    else:
        sub = R.strip(p, "mlp.")
        m = Mlp(in_features=C, hidden_features=4 * C, numerics="bf16")
        fwd = lambda P, X, pts: R.mlp_module(P, X, pts)
    m.load_state_dict(sub, strict=True)
    truth, yard = reference((which, name), sub, x, go, fwd)
    for k, v in yard.items():
        assert 2e-4 <= v <= 5e-2, (k, v)
    gate("NODES-" + which, name, "bf16", run(m.to(DEV), x, go), truth, yard)


@pytest.mark.parametrize("name", ["s48", "s256", "v50"])
def test_block_as_separate_nodes_in_bf16(name):
    """The stochastic-depth form of the block (training mode, drop_path_ratio > 0): LayerNormFn -> attention module -> torch add ->
    LayerNormFn -> Mlp -> torch add, seven autograd nodes instead of one.  It rounds where the fused node rounds (the LayerNorm
    outputs, the operand copies LinearFn / MlpFn make of the gradient at each branch's result, the bf16 dx each branch hands back to
    its LayerNorm; the residual adds are torch's, in fp32), so it is held to the fused block's reference and yardstick.  The ratio is
    too small to drop anything: keep = 1 - 1e-12 is 1.0 in fp32, the mask is floor(1 + U[0, 1)) = 1."""
    p, x, go, truth, yard = block_reference(name)
    m = build(name, "bf16", p, drop_path_ratio=1e-12).train()
    assert not m._dm_fused_block
    torch.manual_seed(0)
    probe = m(x.to(DEV).requires_grad_(True))
    assert type(probe.grad_fn).__name__ == "AddBackward0"          # the second residual add is torch's: not the fused node
    assert type(build(name, "bf16", p)(x.to(DEV).requires_grad_(True)).grad_fn).__name__ == "BlockFnBackward"
    gate("NODES-block", name, "bf16", run(m, x, go), truth, yard)
