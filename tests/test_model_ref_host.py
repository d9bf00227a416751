"""CPU: the fp64 restatement of the v3 training step (tests/model_ref.py) is pinned before the GPU test divides by it.

  * the truth run IS oracle.s2former.forward_pair + oracle.losses.contrastive_loss on the same fp64 parameters (1e-12);
  * the truth run of m3b4 meets the fixture the reference itself produced (tests/golden/model_v3.npz) at the project's 1e-3;
  * the yardstick (points run against truth) is finite for every tensor of every case, and the tensors it leaves below 1e-3 are
    the ones listed here by name -- a rounding point removed by accident shows up as a longer list;
  * the gate max(2 * yard, 1e-3) of tests/test_gpu_model_oracle.py sees the errors it is for: mutants of the truth dict (a writer of
    the shared norm dropped or counted twice, a doubled table gradient, swapped tensors) all sit beyond twice their gate.

Two things follow from the loss and not from the inputs, so no input can change them (model_ref's header): the output gradients of
the two sides of a pair are equal and opposite, hence the bias of the final Linear has an exactly zero gradient and the final norm
and the designed-feature norm contribute exactly nothing to d_norm.bias.  Dropping or doubling a share that is zero leaves a correct
gradient: there is no wrong tensor for the gate to see, and the test asserts that these shares ARE zero (1e-12 of the tensor) instead.
"""
import pytest
import torch

import model_ref as M
import recipe
from oracle import losses as OL
from oracle import s2former as O
from util import load_fx

GATE = 1e-3
# every tensor the bf16 mode leaves within 1e-3 of truth: the loss (a mean of squared distances: the embeddings' 4e-3 averages out) and
# the bias gradient that is zero by symmetry.  Everything else, the designed-feature branch included (its kernels are fp32, its
# output gradient 2 (fa - fb) is not), carries the blocks' roundings.
BELOW_GATE = {"loss", "d_final_features_with_design.bias"}


def test_truth_run_is_the_oracle_forward_pair_and_loss():
    for name in ("m3b4", "m3b2"):
        r = M.reference(name)
        cfg, (left, ld, right, rd, flag) = r["cfg"], r["inputs"]
        P = {k: (v.detach().double().requires_grad_(True) if v.is_floating_point() else v) for k, v in r["params"].items()}
        dd = lambda t: t.double()
        fa, fb = O.forward_pair(P, [dd(t) for t in left], dd(ld), [dd(t) for t in right], dd(rd), cfg)
        loss = OL.contrastive_loss(fa, fb, flag, M.MARGIN)
        loss.backward()
        theirs = {"out_a": fa.detach(), "out_b": fb.detach(), "loss": loss.detach()}
        theirs.update({"d_" + k: v.grad for k, v in P.items() if v.is_floating_point() and v.grad is not None})
        assert sorted(k for k, v in P.items() if v.is_floating_point() and v.grad is None) == sorted(M.NO_GRAD)
        truth = r["truth"]
        assert set(truth) == set(theirs)
        for k in truth:
            assert truth[k].dtype == torch.float64
            if k in M.ZERO_BY_SYMMETRY:      # both are rounding residue of terms that cancel: compared with what cancels
                assert M.rel_err(truth[k], theirs[k], r["scale"][k]) <= 1e-12, k
            else:
                assert M.rel_err(truth[k], theirs[k]) <= 1e-12, (name, k)


def test_truth_run_meets_the_reference_fixture():
    tag = "v3_3s3c_111"
    fx = load_fx("model_v3.npz")
    truth = M.reference("m3b4")["truth"]
    recipe.check_summary(tag + "/out_a", truth["out_a"].numpy(), fx, GATE)
    recipe.check_summary(tag + "/out_b", truth["out_b"].numpy(), fx, GATE)
    want = float(fx[tag + "/loss"])
    assert abs(float(truth["loss"]) - want) <= GATE * abs(want)
    assert sorted(str(s) for s in fx[tag + "/grad_none"]) == sorted(M.NO_GRAD)
    names = [k[2:] for k in truth if k.startswith("d_")]
    assert len(names) == 3 * 13 + 2 * 3 + 6 + 2 + 2
    for n in names:
        # (the fixture pins exact zeros for the bias gradient that cancels; the fp64 run leaves ~1e-16 of the 12.6 that cancel)
        atol = 1e-12 if "d_" + n in M.ZERO_BY_SYMMETRY else 0.0
        recipe.check_summary(tag + "/grad/" + n, truth["d_" + n].numpy(), fx, GATE, k=1024, atol=atol)


@pytest.mark.parametrize("name", list(M.CASES))
def test_yardstick_exists_for_every_tensor(name):
    r = M.reference(name)
    print(f"HOST {name}: truth + points run took {r['seconds']:.1f} s")
    below = set()
    for k, y in r["yard"].items():
        print(f"YARD {name} {k}: {y:.3e}   gate {M.gate(y):.3e}")
        assert y == y and y != float("inf"), k
        assert y <= 0.25, (k, y)      # (twice the yardstick must stay far below the order-1 error of a wrong tensor)
        if y < GATE:
            below.add(k)
    assert below == BELOW_GATE


@pytest.mark.parametrize("name", list(M.CASES))
def test_the_gate_sees_what_it_is_for(name):
    r = M.reference(name)
    truth, yard, parts = r["truth"], r["yard"], r["parts"]
    seen = []

    def must_see(what, key, mutant):
        g = M.gate(yard[key])
        d = M.rel_err(mutant, truth[key])
        print(f"MUTANT {name} {what}: {key} moves {d:.3e}, gate {g:.3e}, ratio to the gate {d / g:.1f}")
        assert d > 2 * g, (what, key, d, g)
        seen.append(what)

    for k in ("norm.weight", "norm.bias"):
        total = truth["d_" + k]
        shares = {w: float(parts[k][w].norm() / total.norm()) for w in M.WRITERS}
        print(f"SHARE {name} d_{k}: " + ", ".join(f"{w} {s:.3e}" for w, s in shares.items()) + f"   gate {M.gate(yard['d_' + k]):.3e}")
        for w in M.WRITERS:
            if (k, w) in M.ZERO_SHARES:
                assert shares[w] <= 1e-12, (k, w, shares[w])      # zero by the pair symmetry: dropping it changes nothing
                continue
            must_see(f"{k} without {w}", "d_" + k, total - parts[k][w])
            must_see(f"{k} with {w} twice", "d_" + k, total + parts[k][w])
    t = "d_blocks1.0.attn.relative_position_bias_table"
    must_see("stage 1 table gradient times 2", t, 2 * truth[t])
    for a, b in (("d_patch_embed_blocks.0.proj.bias", "d_patch_embed_blocks.1.proj.bias"), ("d_blocks0.0.norm1.weight", "d_blocks0.0.norm1.bias")):
        must_see(f"{a[2:]} <- {b[2:]}", a, truth[b])
        must_see(f"{b[2:]} <- {a[2:]}", b, truth[a])
    assert len(seen) == 2 * (4 + 2) + 1 + 4
