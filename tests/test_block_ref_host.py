"""CPU: the fp64 restatement of the fused block (tests/block_ref.py) is pinned before the GPU test divides by it.

  * truth mode IS the oracle's block (same op sequence): equal to the last bit for y, dx and every gradient;
  * with the bf16 points on, every tensor of every GPU case sits in the bf16 range [2e-4, 5e-2] from truth -- never near zero, so
    "err <= 2 * yardstick" in tests/test_gpu_block_oracle.py is never vacuous, and never so large that it would admit a wrong tensor
    (a dropped contribution, a swapped pair, a factor 2 are all errors of order 1);
  * the two-block graph with a side consumer equals its hand-expanded form (b2 alone, its dx plus the side gradient fed to b1 alone).
"""
import pytest
import torch

import block_ref as R
from oracle import s2former as O

_cache = {}


def truth_and_points(name):
    if name not in _cache:
        heads = R.CASES[name][2]
        p, x, go = R.case_data(name)
        _cache[name] = (R.evaluate(lambda P, X: R.block(P, X, heads, False), p, x, go),
                        R.evaluate(lambda P, X: R.block(P, X, heads, True), p, x, go))
    return _cache[name]


@pytest.mark.parametrize("name", ["s48", "n256"])
def test_truth_mode_is_the_oracle_block(name):
    heads = R.CASES[name][2]
    p, x, go = R.case_data(name)
    mine = truth_and_points(name)[0]
    theirs = R.evaluate(lambda P, X: O.cross_scale_block(P, "", X, heads, R.EPS), p, x, go)
    assert set(mine) == set(theirs) == {"y", "dx"} | {"d_" + k for k in R.GRAD_NAMES}
    for k in mine:
        assert mine[k].dtype == torch.float64
        assert R.rel_l2(mine[k], theirs[k]) <= 1e-14, k


def test_vit_form_is_the_block_without_a_table():
    """No table keys: the same graph without the bias add; a zero table gives the same y / dx and the same parameter gradients."""
    name = "n256"
    heads = R.CASES[name][2]
    p, x, go = R.case_data(name)
    zero = dict(p)
    zero["attn.relative_position_bias_table"] = torch.zeros_like(p["attn.relative_position_bias_table"])
    bare = {k: v for k, v in p.items() if "relative_position" not in k}
    for points in (False, True):
        a = R.evaluate(lambda P, X: R.block(P, X, heads, points), zero, x, go)
        b = R.evaluate(lambda P, X: R.block(P, X, heads, points), bare, x, go)
        assert set(a) - set(b) == {"d_attn.relative_position_bias_table"}
        for k in b:
            assert R.rel_l2(b[k], a[k]) <= 1e-14, (points, k)


@pytest.mark.parametrize("name", list(R.CASES))
def test_points_put_every_tensor_in_the_bf16_range(name):
    truth, pts = truth_and_points(name)
    want = {"y", "dx"} | {"d_" + k for k in R.GRAD_NAMES if R.CASES[name][0] == "cross" or "relative_position" not in k}
    assert set(truth) == set(pts) == want
    for k in truth:
        yard = R.rel_l2(pts[k], truth[k])
        print(f"YARD {name} {k}: {yard:.3e}")
        assert 2e-4 <= yard <= 5e-2, (k, yard)


def test_rounding_nodes():
    x = torch.tensor([1.0 + 2.0 ** -9, 3.0, -(1.0 + 3 * 2.0 ** -9)], dtype=torch.float64, requires_grad=True)
    g = torch.tensor([1.0 + 2.0 ** -10, 1.0, 1.0 + 2.0 ** -7], dtype=torch.float64)
    y = R.rf(x, True)
    assert y.tolist() == [1.0, 3.0, -(1.0 + 2.0 ** -7)]          # round to nearest even on 8 significant bits
    y.backward(g)
    assert torch.equal(x.grad, g)                                 # forward node: gradient passes through
    x.grad = None
    y = R.rb(x, True)
    assert torch.equal(y, x)
    y.backward(g)
    assert x.grad.tolist() == [1.0, 1.0, 1.0 + 2.0 ** -7]
    assert R.rf(x, False) is x and R.rb(x, False) is x


@pytest.mark.parametrize("points", [False, True])
@pytest.mark.parametrize("shared", [False, True])
def test_two_blocks_with_a_side_consumer_match_the_hand_expansion(points, shared):
    name = "n256"
    heads = R.CASES[name][2]
    p, x, go = R.case_data(name, blocks=("b1.", "b2."))
    c = torch.randn(x.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    whole = R.evaluate(lambda P, X: R.two_blocks(P, X, heads, points, side=c, shared=shared), p, x, go)
    # by hand: b1 forward, b2 alone on the middle activation, then b1 alone with (b2's dx + c) as its output gradient
    second = "b1." if shared else "b2."
    p1, p2 = R.strip(p, "b1."), R.strip(p, second)
    mid = R.evaluate(lambda P, X: R.block(P, X, heads, points), p1, x, go)["y"]
    r2 = R.evaluate(lambda P, X: R.block(P, X, heads, points), p2, mid, go)
    r1 = R.evaluate(lambda P, X: R.block(P, X, heads, points), p1, x, r2["dx"] + c)
    tol = 1e-13
    assert R.rel_l2(whole["y"], r2["y"]) <= tol and R.rel_l2(whole["dx"], r1["dx"]) <= tol
    for k in R.GRAD_NAMES:
        if shared:
            assert R.rel_l2(whole["d_b1." + k], r1["d_" + k] + r2["d_" + k]) <= tol, k
        else:
            assert R.rel_l2(whole["d_b1." + k], r1["d_" + k]) <= tol and R.rel_l2(whole["d_b2." + k], r2["d_" + k]) <= tol, k
    if not shared:
        assert "d_b2.norm1.weight" in whole and len(whole) == 2 + 2 * len(R.GRAD_NAMES)
