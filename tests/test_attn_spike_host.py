"""CPU: the spiked rows of tests/attn_spike.py do reach what tests/test_gpu_attention_spikes.py is about, and its tolerances hold for a
float32 computation that is right and not for one that is subtly wrong.  Conditions on the data, not measurements of the library:

  margin     in fp64 every (row, tile, lane half) gap over the running reference is at least 0.25 log2 units from the threshold of
             16, so fp32 and fp64 take the same branches (seen: 0.91; a_r is a bf16 value);
  events     the (row, tile) rescales that follow from the kernels' rule are the ones the construction promises;
  headroom   plain_restatement (whole-row softmax, the kernels' operand roundings) and deferred_restatement (the kernels' rule) stay
             at or below HALF of every tolerance of the GPU module, backward included (plain_backward);
  tightness  deferred_restatement with l not rescaled, with O not rescaled, or with the new maximum taken per lane half exceeds them.

Worst err / tol over the cases (G_top = 300, C = 256):    forward   lse     dqkv    dtable
  plain_restatement      bf16 (q32, relpos, pipe16)       0.39      0.007   0.30    0.054
                         split-bf16                       0.046     0.005   0.23    0.12
                         fp32 (register)                  0.056     0.001   0.11
  deferred_restatement   bf16                             0.39      0.015   0.30    0.043
                         split-bf16                       0.069     0.011   0.22    0.085
                         fp32                             0.066     0.001   0.11
  faulty variants        bf16: >= 170 (l), >= 830 (O), >= 180 (half-local maximum); split-bf16: >= 6e4, 3e5, 6e4.
G_top stayed at 300: no bound asked for less.
"""
import pytest
import torch

import attn_spike as A

MARGIN = 0.25


@pytest.fixture(scope="module", params=A.CASES, ids=A.case_id)
def case(request):
    c = A.make(request.param)
    gap, grow, resc = A.deferred_events(c)
    return request.param, c, gap, grow, resc


def test_values_are_bf16_numbers(case):
    _, c, _, _, _ = case
    assert torch.equal(A.bf16(c.qkv), c.qkv) and torch.equal(A.bf16(c.dout), c.dout)
    assert c.qkv[:, :, 0, :, 55].abs().max().item() == c.C / A.K_SHIFT and (c.qkv[:, :, 1, :, 55] == A.K_SHIFT).all()
    assert torch.isfinite(c.o_ref).all() and torch.isfinite(c.lse_ref).all()
    assert c.lse_ref.abs().max().item() > 200.0                     # G_top = 300 log2 units are 208 natural units


def test_relpos_index_is_the_oracle_s():
    from oracle import s2former as O
    for cube in ((3, 8, 8), (4, 8, 8)):
        assert (A._relpos_index(cube) == O.relpos_index(cube)).all()


def test_threshold_margin(case):
    _, c, gap, _, _ = case
    g = gap[~torch.isnan(gap)]
    margin = (g - A.RESCALE_LOG2).abs().min().item()
    print(f"SPIKES host {A.case_id(case[0])}: least distance of a gap from the threshold {margin:.3f}")
    assert margin >= MARGIN


def test_expected_rescale_events(case):
    _, c, gap, grow, resc = case
    N, nkt = c.N, c.nkt
    key_half = (torch.from_numpy(c.keys) & 4) >> 2                  # [B, H, NKT]
    grows_at = grow.any(-1)                                         # [B, H, N, NKT]
    # every later tile has growing rows with the spike in each lane half (the last tile: in each half that has a valid key)
    for t in range(1, nkt):
        halves = {int((j & 4) >> 2) for j in range(32 * t, min(N, 32 * t + 32))}
        for hh in halves:
            units = key_half[:, :, t] == hh
            assert grow[..., t, hh][units].any(), f"tile {t}: no row grows with the spike in half {hh}"
            assert not grow[..., t, 1 - hh][units].any(), f"tile {t}: growth seen by the half without the spike"
    # key N - 1 is a spike that makes rows grow
    last = torch.from_numpy(c.keys[:, :, nkt - 1] == N - 1)
    assert last.any() and grows_at[..., nkt - 1][last].any()
    full = 32 * (N // 32)                                           # rows of whole waves
    kind = torch.from_numpy(c.kind)
    tile0 = torch.from_numpy(c.spike_tile[..., 0])
    tile1 = torch.from_numpy(c.spike_tile[..., 1])
    gap0 = torch.from_numpy(c.spike_gap[..., 0])
    # dense: every whole wave rescales at every later tile, and rows that do not grow themselves are carried along
    d = kind == 0
    assert resc[d][:, :full, 1:].all()
    assert (resc[d] & ~grows_at[d]).any()
    # plain: never
    assert not resc[kind == 1].any()
    # single: exactly one growing row per 32-row block; its 15 row causes no event
    s = kind == 2
    per_block = torch.nn.functional.pad(grows_at[s].any(-1), (0, (-N) % 32)).reshape(int(s.sum()), -1, 32).sum(-1)
    assert (per_block == 1).all()
    assert (grows_at[s].sum(-1).sum(-1) == (N + 31) // 32).all()    # ... and it grows once
    fifteen = s[..., None] & (gap0 == 15.0)
    assert fifteen.any()
    at = torch.nn.functional.one_hot(tile0.clamp(min=0), nkt).bool()
    assert not (resc & at)[fifteen].any() and not grows_at[fifteen].any()
    # double: two rescales of the row itself, two tiles apart
    dbl = (kind == 3)[..., None] & (tile1 >= 0)
    assert dbl.any() and (grows_at[dbl].sum(-1) == 2).all() and (tile1[dbl] == tile0[dbl] + 2).all()
    # rows that move by less than the threshold inside a rescaling wave: the alpha = 2^(m - mn) rows
    moved = resc[..., None] & (gap > 0) & (gap < A.RESCALE_LOG2)
    assert moved.any()


def _ratios(c, out, lse, backward):
    dqkv = dtable = None
    if backward:
        dqkv, dtable = A.plain_backward(c, out, lse)
    return {k: e / t for k, (e, t) in A.errors(c, out, lse, dqkv, dtable).items()}


def test_tolerance_headroom(case):
    """A factor of 2 between the right float32 computation and each bound of the GPU module."""
    _, c, _, _, _ = case
    for name, fn in (("plain", A.plain_restatement), ("deferred", A.deferred_restatement)):
        r = _ratios(c, *fn(c), backward=True)
        print(f"SPIKES host {A.case_id(case[0])} {name}: err / tol " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
        assert max(r.values()) <= 0.5, (name, r)


def test_tightness(case):
    """Each faulty variant of the kernels' rule is past a bound on the same inputs: the net is tight where it matters."""
    cs, c, _, _, _ = case
    for fault in A.FAULTS:
        r = _ratios(c, *A.deferred_restatement(c, fault=fault), backward=False)
        print(f"SPIKES host {A.case_id(cs)} {fault}: err / tol " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
        assert max(r.values()) > 1.0, (fault, r)
        if fault == "o_not_rescaled":
            assert r["fwd"] > 1.0 and r["lse"] <= 0.5               # lse does not see O
        else:
            assert r["lse"] > 1.0 and r["lse_shift"] > 1.0

