"""GPU: the deferred-maximum rescale of dm_attention_q32.hip and dm_attention_x3.hip (`tile_max`, `rescale_o`) on spiked rows, and the
backward kernels fed the lse that comes out of it (default routing, one process; no DM_ATTN_* switch is set).

On random operands no 32-key tile exceeds the first tile's row maximum by 2^16, so the branch never runs in the rest of the suite
(test_attention_q32_deferred_maximum takes it on every row at almost every tile, forward only before this module, and never in
dm_attention_x3.hip).  tests/attn_spike.py builds rows whose maximum arrives late by a chosen gap -- 15 (no rescale, still exact), 17,
40, 300 log2 units (alpha and every earlier probability flush to zero), twice in a row, in one row of a wave, in either lane half, on
key N - 1 next to the masked columns, on rows shifted by +-32 natural units -- and tests/test_attn_spike_host.py shows on the CPU that
these rows do what is claimed, that a right float32 computation stays under half of each bound below and that three subtly wrong ones do
not.  The bounds are the existing ones (attn_spike.errors): test_attention_forward_backward for bf16 and fp32,
test_split_tile_count_matrix for the split-bf16 kernels, its lse bound scaled by max(1, |lse_ref|) since lse reaches 240 here.

Cases (attn_spike.CASES; routes as in test_q32_tile_count_matrix):
  q32      bf16, B = 8, H = 12, N in 129, 160, 193, 224, 255, 256, without a bias (8 waves up to 7 tiles, 4 waves at 8) and with dense
           rows (4 waves); backward through ops.attention_bwd, the table gradient through the slab;
  relpos   the table-in-kernel instances at cubes (3, 8, 8) and (4, 8, 8), also against ops.attention_fwd on the gathered rows (the
           bounds of test_attention_relpos_table_in_kernel), backward through the table-reading passes;
  split    fp32 tensors, B = 3, H = 4, N in 129, 192, 255, 256, the table at 192 and 256;
  pipe16, register   controls on whole-row families with the same data: the 16-row pipeline at N = 128, the fp32 register kernels at 197.
Every case: outputs finite; forward, lse, dqkv, dtable within tolerance of fp64; on shifted rows lse = the unshifted row's lse +
c_r * scale within the lse tolerance; inputs unchanged.

Worst err / tol over the cases (G_top = 300, C = 256):   forward   lse     lse (shift)   dqkv    dtable
  CPU   plain_restatement     bf16                       0.39      0.007   0.002         0.30    0.054
                              split-bf16                 0.046     0.005   0.004         0.23    0.12
                              fp32                       0.056     0.001   0.001         0.11
        deferred_restatement  bf16                       0.39      0.015   0.010         0.30    0.043
                              split-bf16                 0.069     0.011   0.006         0.22    0.085
  GPU   (MI355X)              bf16                       0.39      0.015   0.010         0.30    0.043
                              split-bf16                 0.074     0.10    0.10          0.29    0.16
                              fp32 register control      0.15      0.007   0.007         0.052
  (the table in the kernel and the dense rows agree bit for bit on these rows: out and lse differences are 0)

Tightness on the real kernels (one-line numeric faults on a scratch copy of the library, one build and one run of this module each):
  dm_attention_q32.hip, rescale_o without `la[i] *= alpha`:  all 12 q32 cases and both relpos cases fail (forward error 3.5 - 4.5
      against 2e-2); split, pipe16 and register pass.  test_attention_q32_deferred_maximum fails at all four points (lse off by up
      to 11.7); tests/test_gpu_attention_edges.py passes (56 of 56).
  dm_attention_x3.hip, `mn = fmaxf(m, th)` for `fmaxf(m, half_max(th))`:  all 6 split cases fail; every bf16 case passes.
      test_attention_q32_deferred_maximum passes (it does not run this file) and tests/test_gpu_attention_edges.py passes (56 of 56):
      before this module nothing saw it.
"""
import numpy as np
import pytest
import torch

import attn_spike as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = A.D


def _ops():
    from deepmerge_amd import ops
    return ops


def _snapshot(ts):
    return [None if t is None else t.clone() for t in ts]


def _unchanged(ts, before, what):
    for i, (t, b) in enumerate(zip(ts, before)):
        if t is not None:
            assert torch.equal(t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32), b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), \
                f"{what}: the call changed its input {i}"


def _report(cs, res):
    print(f"SPIKES {A.case_id(cs)}: " + "  ".join(f"{k} {e:.3e} (tol {t:.3e}, {e / t:.3f})" for k, (e, t) in res.items()))
    for k, (e, t) in res.items():
        assert e < t, f"{A.case_id(cs)}: {k} {e:.3e} against {t:.3e}"


@pytest.mark.parametrize("cs", A.CASES, ids=A.case_id)
def test_spiked_rows(cs):
    ops = _ops()
    family, N, B, H, bias_mode, mode = cs
    c = A.make(cs)
    scale = c.scale
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    qd = c.qkv.to(DEV).to(dt)
    dout = c.dout.to(DEV).to(dt)
    table = None if c.table is None else c.table.to(DEV)
    idx32 = None if c.index is None else c.index.to(torch.int32).to(DEV)
    bias = bias_t = None
    if bias_mode == "dense" or family == "relpos":
        bias, bias_t = ops.relpos_bias_gather(table, idx32, N, transposed=True)
        assert torch.equal(bias.cpu(), c.bias)
    inputs = [qd, dout, table, idx32, bias, bias_t]
    before = _snapshot(inputs)

    slab = info = None
    if family == "split":
        assert ops.attention_split_ok(B, N, H, D, c.cube)
        out, lse, hi, lo = ops.attention_fwd_split(qd, table, c.cube, B, N, H, D, scale)
        assert torch.equal(hi.float(), qd) and not lo.float().any()         # bf16 numbers: the lo plane is zero
        fwd = _snapshot([out, lse, hi, lo])
        dqkv, slab, info = ops.attention_bwd_split(hi, lo, table, c.cube, out, dout, lse, B, N, H, D, scale, idx32, c.n_bins)
        _unchanged([out, lse, hi, lo], fwd, "backward")
    elif family == "relpos":
        assert ops.relpos_inkernel(B, N, H, D, c.cube, torch.bfloat16)
        out, lse = ops.attention_fwd_relpos(qd, table, c.cube, B, N, H, D, scale)
        o_dense, lse_dense = ops.attention_fwd(qd, bias, B, N, H, D, scale)
        assert torch.isfinite(o_dense.float()).all() and torch.isfinite(lse_dense).all()
        agree_o = (out.float() - o_dense.float()).abs().max().item()
        agree_l = (lse - lse_dense).abs().max().item()
        print(f"SPIKES {A.case_id(cs)}: table in kernel against dense rows: out {agree_o:.3e} (2^-6) lse {agree_l:.3e} (1e-4)")
        assert agree_o <= 2 ** -6
        np.testing.assert_allclose(lse.cpu().numpy(), lse_dense.cpu().numpy(), rtol=0, atol=1e-4)
        fwd = _snapshot([out, lse])
        dqkv, slab, info = ops.attention_bwd(qd, None, out, dout, lse, B, N, H, D, scale, idx32, c.n_bins, table=table, cube=c.cube)
        _unchanged([out, lse], fwd, "backward")
    else:
        out, lse = ops.attention_fwd(qd, bias, B, N, H, D, scale)
        fwd = _snapshot([out, lse])
        dqkv, slab, info = ops.attention_bwd(qd, bias, out, dout, lse, B, N, H, D, scale, idx32, c.n_bins, bias_t=bias_t)
        _unchanged([out, lse], fwd, "backward")
    dtable = None
    if slab is not None:
        dtable = torch.empty((c.n_bins, H), device=DEV)
        ops.relpos_bias_scatter(slab, dtable, B, H, info, c.n_bins)
    torch.cuda.synchronize()
    _unchanged(inputs, before, "forward / backward")
    for name, t in (("out", out), ("lse", lse), ("dqkv", dqkv), ("dtable", dtable)):
        assert t is None or torch.isfinite(t.float()).all(), f"{A.case_id(cs)}: non-finite {name}"
    _report(cs, A.errors(c, out.float().cpu(), lse.cpu(), dqkv.float().cpu(), None if dtable is None else dtable.cpu()))
