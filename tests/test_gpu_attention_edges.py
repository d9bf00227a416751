"""GPU: the attention families at every key-tile count, ragged tail and NaN neighbour (default routing; no DM_ATTN_* switch is set).

Two gaps of tests/test_gpu_kernels.py are closed here.

1. The tile-count matrix.  dm_attention_q32.hip, dm_attention_q32_bwd.hip and dm_attention_x3.hip instantiate one kernel per
   (32-key tiles NKT in 5..8, ragged or exact, bias mode, 4 or 8 waves).  N in MATRIX_N gives every NKT one valid key in the last
   tile (32 (NKT - 1) + 1), one missing key (32 NKT - 1) and the exact tiling, with and without a bias, at the tolerances of
   test_attention_forward_backward / test_attention_split_forward_backward: nothing new is measured, instances are reached.

2. Isolation.  The persistent kernels read keys >= N through a per-sample buffer descriptor that returns zero past the sample, and
   mask them; the register and generic kernels guard rows in code.  The masked probability is exactly 0, so a wrong descriptor
   length, a stale LDS tail or a missing guard computes 0 x (what lies behind the sample) -- invisible while that is finite.  Here
   every tensor a call reads or writes sits between NaN guards (tests/attn_frame.py) at an address that is 16-byte but not 256-byte
   aligned, outputs are NaN before the call, and every second sample is NaN, once the odd and once the even ones: each real sample
   has NaN on both sides.  The real samples must be finite, within the family's fp64 tolerance, BIT-identical to the same call on
   plain tensors without NaN, the guards untouched and the inputs unchanged.  Calls that fill the bias-gradient slab sum over the
   samples and run with guards only.
"""
import math

import numpy as np
import pytest
import torch

import attn_frame as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")
MATRIX_N = [129, 159, 160, 161, 191, 192, 193, 223, 224, 225, 255, 256]


def _ops():
    from deepmerge_amd import ops
    return ops


def _lib():
    from deepmerge_amd import _lib as L
    return L.lib(), L.check


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- B. the tile-count matrix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("N", MATRIX_N)
def test_q32_tile_count_matrix(N, with_bias):
    """bf16, B = 8, H = 12 (B * H = 96: the smallest batch the plan sends to the 32-row kernels), D = 64; the body and tolerances of
    test_attention_forward_backward (fp64 reference; forward, backward, table gradient through the slab).  Routes (attn_plan_fwd /
    attn_plan_bwd in dm_attention.hip), NKT = ceil(N / 32), ragged = N % 32 != 0:
      forward   no bias: 32-row NONE on 8 waves for NKT <= 7, on 4 waves at NKT = 8; bias: 32-row DENSE on 4 waves;
      backward  no bias: 32-row dQ and dK / dV (8 waves for NKT <= 7, 4 waves at 8);
                bias + slab at N = 192, 256: 32-row DENSE dQ plus the 16-row pipelined dK / dV, which fills the slab;
                bias + slab at any other N (ragged for the 16-row pipeline): the register kernels."""
    ops = _ops()
    B, H, D, mode = 8, 12, 64, "bf16"
    rng = np.random.default_rng(N)
    dt = DT[mode]
    qkv = torch.from_numpy(rng.normal(size=(B, N, 3, H, D)).astype(np.float32))
    qkv = qkv.to(dt).float()                     # operands exactly representable in the mode's dtype
    n_bins = 157
    table = torch.from_numpy(rng.normal(size=(n_bins, H)).astype(np.float32))
    index = torch.from_numpy(rng.integers(0, n_bins, size=(N, N)).astype(np.int32))
    dout = torch.from_numpy(rng.normal(size=(B, N, H * D)).astype(np.float32)).to(dt).float()
    scale = 0.125

    q64 = qkv.double().requires_grad_(True)
    t64 = table.double().requires_grad_(True)
    bias64 = t64[index.long().reshape(-1)].reshape(N, N, H).permute(2, 0, 1) if with_bias else None
    o_ref, lse_ref = F.attn_ref(q64, bias64, scale)
    (o_ref * dout.double()).sum().backward()

    qd = qkv.to(DEV).to(dt)
    bias = bias_t = None
    if with_bias:
        bias, bias_t = ops.relpos_bias_gather(table.to(DEV), index.to(DEV), N, transposed=True)
        np.testing.assert_array_equal(bias.cpu().numpy(), bias64.detach().float().numpy())
        np.testing.assert_array_equal(bias_t.cpu().numpy(), bias64.detach().float().transpose(1, 2).numpy())
        if N in (48, 192):
            bias_t = None           # exercise the strided fallback of the key-major kernel too
    out, lse = ops.attention_fwd(qd, bias, B, N, H, D, scale)
    tol = 2e-5 if mode == "fp32" else 2e-2
    err_l = (lse.cpu().double() - lse_ref.detach()).abs().max().item()
    err = (out.float().cpu().double() - o_ref.detach()).abs().max().item()
    print(f"EDGES matrix q32 N={N} bias={int(with_bias)}: fwd {err:.3e} (tol {tol:.0e}) lse {err_l:.3e} (rtol = atol = 2e-2)")
    np.testing.assert_allclose(lse.cpu().numpy(), lse_ref.detach().numpy(), rtol=1e-4 if mode == "fp32" else 2e-2, atol=1e-4 if mode == "fp32" else 2e-2)
    assert err < tol, f"forward max err {err}"

    dqkv, slab, rows = ops.attention_bwd(qd, bias, out, dout.to(DEV).to(dt), lse, B, N, H, D, scale,
                                         index.to(DEV) if with_bias else None, n_bins if with_bias else 0, bias_t=bias_t)
    gq = q64.grad
    scale_ref = gq.abs().max().item()
    err = (dqkv.float().cpu().double() - gq).abs().max().item()
    print(f"EDGES matrix q32 N={N} bias={int(with_bias)}: dqkv {err:.3e} (tol {(5e-5 if mode == 'fp32' else 4e-2) * max(1.0, scale_ref):.3e})")
    assert err < (5e-5 if mode == "fp32" else 4e-2) * max(1.0, scale_ref), f"dqkv max err {err} (scale {scale_ref})"
    if with_bias:
        dtable = torch.empty((n_bins, H), device=DEV)
        ops.relpos_bias_scatter(slab, dtable, B, H, rows, n_bins)
        gt = t64.grad
        err = (dtable.cpu().double() - gt).abs().max().item()
        print(f"EDGES matrix q32 N={N} bias={int(with_bias)}: dtable {err:.3e} (tol {(1e-4 if mode == 'fp32' else 6e-2) * max(1.0, gt.abs().max().item()):.3e})")
        assert err < (1e-4 if mode == "fp32" else 6e-2) * max(1.0, gt.abs().max().item()), f"dtable max err {err}"


@pytest.mark.parametrize("N,scales", [(n, 0) for n in MATRIX_N] + [(192, 3), (256, 4)])
def test_split_tile_count_matrix(N, scales):
    """The split-bf16 entry points (dm_attention_x3.hip: fp32 tensors, every product a split-bf16 triple) at B = 3, H = 4, D = 64 --
    they have no B * H rule -- without a table at every N of the matrix, and with the (N / 64, 8, 8) table at 192 and 256.  Forward
    and dQ on 8 waves, dK / dV on 4, NKT = ceil(N / 32), ragged = N % 32 != 0.  Body and tolerances of
    test_attention_split_forward_backward (5e-5, 5e-5, 2e-5 against fp64) without its plane-pair part."""
    from oracle import s2former as O
    ops = _ops()
    B, H, D = 3, 4, 64
    rng = np.random.default_rng(7 * N + scales)
    qkv = torch.from_numpy(rng.normal(size=(B, N, 3, H, D)).astype(np.float32))
    cube = (scales, 8, 8) if scales else None
    table = bias64 = None
    if scales:
        n_bins = (2 * scales - 1) * 225
        table = torch.from_numpy(rng.normal(size=(n_bins, H)).astype(np.float32))
        index = torch.from_numpy(O.relpos_index(cube).astype(np.int64))
        bias64 = table.double()[index.reshape(-1)].reshape(N, N, H).permute(2, 0, 1)
    assert ops.attention_split_ok(B, N, H, D, cube)
    o_ref, lse_ref = F.attn_ref(qkv.double(), bias64, 0.125)
    out, lse, hi, lo = ops.attention_fwd_split(qkv.to(DEV), None if table is None else table.to(DEV), cube, B, N, H, D, 0.125)
    # the images: hi is the bf16 rounding, hi + lo recovers x to 2^-17 relative
    assert torch.equal(hi.cpu(), qkv.to(torch.bfloat16))
    assert ((hi.float() + lo.float()).cpu() - qkv).abs().max().item() <= 2.0 ** -16 * qkv.abs().max().item()
    err_o = (out.cpu().double() - o_ref).abs().max().item()
    err_l = (lse.cpu().double() - lse_ref).abs().max().item()
    print(f"EDGES matrix split N={N} table={scales}: fwd {err_o:.3e} (tol 5e-5) lse {err_l:.3e} (tol 5e-5)")
    assert err_o < 5e-5 and err_l < 5e-5
    o32, lse32 = ops.attention_fwd(qkv.to(DEV), None if bias64 is None else bias64.float().contiguous().to(DEV), B, N, H, D, 0.125)
    assert (out - o32).abs().max().item() < 5e-5
    # backward: dqkv (and the table gradient through the slab) against fp64 autograd
    dout = torch.from_numpy(rng.normal(size=(B, N, H * D)).astype(np.float32))
    q64 = qkv.double().requires_grad_(True)
    t64 = None if table is None else table.double().requires_grad_(True)
    b64 = None if table is None else t64[index.reshape(-1)].reshape(N, N, H).permute(2, 0, 1)
    o64, _ = F.attn_ref(q64, b64, 0.125)
    o64.backward(dout.double())
    idx32 = None if table is None else index.to(torch.int32).to(DEV)
    dqkv, slab, info = ops.attention_bwd_split(hi, lo, None if table is None else table.to(DEV), cube, out, dout.to(DEV), lse, B, N, H, D, 0.125,
                                               idx32, 0 if table is None else n_bins)
    g = q64.grad
    err_g = (dqkv.cpu().double() - g).abs().max().item() / g.abs().max().item()
    print(f"EDGES matrix split N={N} table={scales}: dqkv {err_g:.3e} (tol 2e-5, relative to max)")
    assert err_g < 2e-5
    if table is not None:
        dt = torch.empty((n_bins, H), device=DEV)
        ops.relpos_bias_scatter(slab, dt, B, H, info, n_bins)
        err_t = (dt.cpu().double() - t64.grad).abs().max().item() / t64.grad.abs().max().item()
        print(f"EDGES matrix split N={N} table={scales}: dtable {err_t:.3e} (tol 2e-5, relative to max)")
        assert err_t < 2e-5


# ---- C. isolation -------------------------------------------------------------------------------------------------------------------
class _Tensors:
    """The device tensors of one C call, by argument name: framed between NaN guards, or plain.  Inputs are remembered bit for bit."""

    def __init__(self, frame):
        self.frame, self.t, self.handles, self.before = frame, {}, {}, {}

    def _place(self, name, t, guard):
        if self.frame:
            self.t[name], self.handles[name] = F.framed(t, guard)
        else:
            self.t[name] = t.clone()
        return self.t[name]

    def input(self, name, t, guard, poison=None):
        v = self._place(name, t.to(DEV), guard)
        if poison is not None:
            F.poison_samples(v, poison)
        self.before[name] = F.bits(v).clone()

    def output(self, name, shape, dtype, guard):
        self._place(name, torch.full(shape, NAN, dtype=dtype, device=DEV), guard)        # NaN before the call: an unwritten row shows

    def __getitem__(self, name):
        return self.t.get(name)

    def check(self, what):
        for name, h in self.handles.items():
            assert F.guards_intact(h), f"{what}: the call wrote outside `{name}`"
        for name, b in self.before.items():
            assert torch.equal(F.bits(self.t[name]), b), f"{what}: the call changed its input `{name}`"


def _same_bits(a, b, real):
    return torch.equal(F.bits(a[real].contiguous()), F.bits(b[real].contiguous()))


def _case_inputs(mode, B, H, D, N, bias):
    """CPU inputs and the fp64 reference of one isolation case.  D = 64, N <= 256: the inputs of test_attention_forward_backward
    (table cases: of test_attention_relpos_table_in_kernel); otherwise the inputs of test_attention_generic_shapes."""
    dt = DT[mode]
    c = {"mode": mode, "dt": dt, "B": B, "H": H, "D": D, "N": N, "bias_kind": bias, "generic": D != 64 or N > 256}
    table = index = None
    if c["generic"]:
        g = torch.Generator().manual_seed(N + D)
        qkv = (torch.randn(B, N, 3, H, D, generator=g) * 0.7).to(dt).float()
        dense = torch.randn(H, N, N, generator=g) * 0.5 if bias else None
        dout = torch.randn(B, N, H * D, generator=g).to(dt).float()
        c["scale"] = D ** -0.5
    else:
        rng = np.random.default_rng(N)
        qkv = torch.from_numpy(rng.normal(size=(B, N, 3, H, D)).astype(np.float32)).to(dt).float()
        if bias == "table":
            from oracle import s2former as O
            c["cube"] = (N // 64, 8, 8)
            c["n_bins"] = (2 * c["cube"][0] - 1) * 225
            table = torch.from_numpy(rng.normal(size=(c["n_bins"], H)).astype(np.float32))
            index = torch.from_numpy(O.relpos_index(c["cube"]).astype(np.int32))
        else:
            c["n_bins"] = 157
            table = torch.from_numpy(rng.normal(size=(c["n_bins"], H)).astype(np.float32))
            index = torch.from_numpy(rng.integers(0, c["n_bins"], size=(N, N)).astype(np.int32))
        dout = torch.from_numpy(rng.normal(size=(B, N, H * D)).astype(np.float32)).to(dt).float()
        dense = None
        c["scale"] = 0.125
    q64 = qkv.double().requires_grad_(True)
    t64 = b64 = None
    if c["generic"]:
        b64 = None if dense is None else dense.double()
    elif bias:
        t64 = table.double().requires_grad_(True)
        b64 = t64[index.long().reshape(-1)].reshape(N, N, H).permute(2, 0, 1)
        dense = b64.detach().float().contiguous()
    o_ref, lse_ref = F.attn_ref(q64, b64, c["scale"])
    (o_ref * dout.double()).sum().backward()
    c.update(qkv=qkv.to(dt), dout=dout.to(dt), dense=dense, dense_t=None if dense is None else dense.transpose(1, 2).contiguous(),
             table=table, index=index, o_ref=o_ref.detach(), lse_ref=lse_ref.detach(), gq=q64.grad, gt=None if t64 is None else t64.grad)
    return c


def _forward(c, split, frame, parity):
    """One forward call through the C entry point; returns its _Tensors."""
    L, check = _lib()
    B, H, D, N, dt = c["B"], c["H"], c["D"], c["N"], c["dt"]
    code = _ops()._dt(c["qkv"])
    tok = 64 * H * D
    s = _Tensors(frame)
    s.input("qkv", c["qkv"], 3 * tok, parity)
    s.output("out", (B, N, H * D), dt, tok)
    s.output("lse", (B, H, N), torch.float32, 64 * H)
    if split:
        s.output("hi", c["qkv"].shape, torch.bfloat16, 3 * tok)
        s.output("lo", c["qkv"].shape, torch.bfloat16, 3 * tok)
        check(L.dm_attention_split_fwd(s["qkv"].data_ptr(), s["hi"].data_ptr(), s["lo"].data_ptr(), None, 0, 0, 0, s["out"].data_ptr(),
                                       s["lse"].data_ptr(), B, N, H, D, c["scale"], _stream()), "dm_attention_split_fwd")
    elif c["bias_kind"] == "table":
        s.input("table", c["table"], 64 * H)
        cs, ch, cw = c["cube"]
        check(L.dm_attention_fwd_relpos(s["qkv"].data_ptr(), s["table"].data_ptr(), cs, ch, cw, s["out"].data_ptr(), s["lse"].data_ptr(),
                                        B, N, H, D, c["scale"], code, _stream()), "dm_attention_fwd_relpos")
    else:
        if c["dense"] is not None:
            s.input("bias", c["dense"], 64 * N)
        check(L.dm_attention_fwd(s["qkv"].data_ptr(), _ptr(s["bias"]), s["out"].data_ptr(), s["lse"].data_ptr(), B, N, H, D, c["scale"],
                                 code, _stream()), "dm_attention_fwd")
    torch.cuda.synchronize()
    return s


def _backward(c, split, frame, parity, fwd):
    """One backward call through the C entry point on the outputs of the plain forward `fwd`; returns its _Tensors."""
    L, check = _lib()
    B, H, D, N, dt = c["B"], c["H"], c["D"], c["N"], c["dt"]
    code = _ops()._dt(c["qkv"])
    tok = 64 * H * D
    slab = c["bias_kind"] in ("index", "table")
    s = _Tensors(frame)
    s.input("out", fwd["out"], tok, parity)
    s.input("dout", c["dout"], tok, parity)
    s.input("lse", fwd["lse"], 64 * H, parity)
    s.output("dqkv", c["qkv"].shape, dt, 3 * tok)
    s.output("delta", (B, H, N), torch.float32, 64 * H)
    if split:
        s.input("hi", fwd["hi"], 3 * tok, parity)
        s.input("lo", fwd["lo"], 3 * tok, parity)
        s.output("dhi", c["dout"].shape, torch.bfloat16, tok)
        s.output("dlo", c["dout"].shape, torch.bfloat16, tok)
        check(L.dm_attention_split_bwd(s["hi"].data_ptr(), s["lo"].data_ptr(), None, 0, 0, 0, s["out"].data_ptr(), s["dout"].data_ptr(),
                                       s["dhi"].data_ptr(), s["dlo"].data_ptr(), s["lse"].data_ptr(), s["dqkv"].data_ptr(),
                                       s["delta"].data_ptr(), None, B, N, H, D, c["scale"], _stream()), "dm_attention_split_bwd")
        torch.cuda.synchronize()
        return s
    s.input("qkv", c["qkv"], 3 * tok, parity)
    if slab:
        assert parity is None                                   # the slab sums over the samples
        chunks = L.dm_attention_bwd_batch_chunks(B, N, H, code)
        s.output("slab", (chunks, H, N, N), torch.float32, 64 * N)
    if c["bias_kind"] == "table":
        s.input("table", c["table"], 64 * H)
        cs, ch, cw = c["cube"]
        check(L.dm_attention_bwd_relpos(s["qkv"].data_ptr(), s["table"].data_ptr(), cs, ch, cw, None, None, s["out"].data_ptr(),
                                        s["dout"].data_ptr(), s["lse"].data_ptr(), s["dqkv"].data_ptr(), s["delta"].data_ptr(),
                                        s["slab"].data_ptr(), B, N, H, D, c["scale"], code, _stream()), "dm_attention_bwd_relpos")
    else:
        if c["dense"] is not None:
            s.input("bias", c["dense"], 64 * N)
            if not c["generic"]:
                s.input("bias_t", c["dense_t"], 64 * N)
        check(L.dm_attention_bwd(s["qkv"].data_ptr(), _ptr(s["bias"]), _ptr(s["bias_t"]), s["out"].data_ptr(), s["dout"].data_ptr(),
                                 s["lse"].data_ptr(), s["dqkv"].data_ptr(), s["delta"].data_ptr(), _ptr(s["slab"]), B, N, H, D, c["scale"],
                                 code, _stream()), "dm_attention_bwd")
    torch.cuda.synchronize()
    return s


def _check_forward(c, split, s, real, what):
    """The real samples of out / lse (and of the two images) are finite and within the family's existing fp64 tolerance."""
    mode = c["mode"]
    out, lse = s["out"][real].float().cpu().double(), s["lse"][real].cpu().double()
    assert torch.isfinite(out).all() and torch.isfinite(lse).all(), f"{what}: non-finite forward output in a real sample"
    o_ref, lse_ref = c["o_ref"][real], c["lse_ref"][real]
    err_o, err_l = (out - o_ref).abs().max().item(), (lse - lse_ref).abs().max().item()
    print(f"EDGES isolation {what}: fwd {err_o:.3e} lse {err_l:.3e}")
    if split:                                                   # test_attention_split_forward_backward
        assert err_o < 5e-5 and err_l < 5e-5, what
        assert torch.equal(s["hi"][real].cpu(), c["qkv"][real].to(torch.bfloat16)), what
        assert ((s["hi"][real].float() + s["lo"][real].float()).cpu() - c["qkv"][real]).abs().max().item() <= 2.0 ** -16 * c["qkv"][real].abs().max().item(), what
    elif c["generic"]:                                          # test_attention_generic_shapes
        tol = 2e-5 if mode == "fp32" else 2e-2
        np.testing.assert_allclose(out.numpy(), o_ref.numpy(), rtol=tol, atol=tol, err_msg=what)
        np.testing.assert_allclose(lse.numpy(), lse_ref.numpy(), rtol=1e-5, atol=1e-5, err_msg=what)
    elif c["bias_kind"] == "table":                             # test_attention_relpos_table_in_kernel
        np.testing.assert_allclose(lse.numpy(), lse_ref.numpy(), rtol=2e-2, atol=2e-2, err_msg=what)
        assert err_o < 3e-2, what
    else:                                                       # test_attention_forward_backward
        lt = 1e-4 if mode == "fp32" else 2e-2
        np.testing.assert_allclose(lse.numpy(), lse_ref.numpy(), rtol=lt, atol=lt, err_msg=what)
        assert err_o < (2e-5 if mode == "fp32" else 2e-2), f"{what}: forward max err {err_o}"


def _check_backward(c, split, s, real, what):
    """The real samples of dqkv and delta (and of dout's two images) are finite; dqkv within the family's existing fp64 tolerance.
    delta = rowsum(dout * out) has no tolerance in the existing tests.  Every family sums the D products in fp32 from the tensors it
    is given (bf16 products are exact in fp32), so against the fp64 sum of the same tensors the error is at most D roundings of the
    running sum, each 2^-24 of a partial sum that sum |dout * out| bounds; a factor 4 covers any summation order and an accumulator
    that truncates: |delta - delta64| <= 4 D 2^-24 sum_d |dout * out|."""
    mode, B, H, D, N = c["mode"], c["B"], c["H"], c["D"], c["N"]
    dqkv, delta = s["dqkv"][real].float().cpu().double(), s["delta"][real].cpu().double()
    assert torch.isfinite(dqkv).all() and torch.isfinite(delta).all(), f"{what}: non-finite backward output in a real sample"
    gq = c["gq"][real]
    prod = (s["dout"][real].float().cpu().double() * s["out"][real].float().cpu().double()).reshape(len(real), N, H, D)
    d_err = ((delta - prod.sum(-1).permute(0, 2, 1)).abs() - 4 * D * 2.0 ** -24 * prod.abs().sum(-1).permute(0, 2, 1)).max().item()
    assert d_err <= 0, f"{what}: delta is {d_err:.3e} past its bound"
    if split:
        err = (dqkv - gq).abs().max().item() / gq.abs().max().item()
        assert err < 2e-5, f"{what}: dqkv {err}"
        dhi, dlo, dout = s["dhi"][real], s["dlo"][real], s["dout"][real]
        assert torch.equal(dhi, dout.to(torch.bfloat16)) and (dhi.float() + dlo.float() - dout).abs().max().item() <= 2.0 ** -16 * dout.abs().max().item(), what
    elif c["generic"]:
        err = float((dqkv - gq).norm() / gq.norm())
        assert err < (1e-4 if mode == "fp32" else 2e-2), f"{what}: dqkv {err}"
    elif c["bias_kind"] == "table":
        err = (dqkv - gq).abs().max().item() / gq.abs().max().item()
        assert err < 2e-2, f"{what}: dqkv {err}"
    else:
        err = (dqkv - gq).abs().max().item()
        assert err < (5e-5 if mode == "fp32" else 4e-2) * max(1.0, gq.abs().max().item()), f"{what}: dqkv max err {err}"
    print(f"EDGES isolation {what}: dqkv {err:.3e} delta within its bound by {-d_err:.3e}")


def _check_table_gradient(c, s, what):
    """Slab -> table gradient as the existing tests do (the scatter consumes the slab), against fp64."""
    ops = _ops()
    B, H, N, n_bins = c["B"], c["H"], c["N"], c["n_bins"]
    slab = s["slab"]
    assert torch.isfinite(slab).all(), f"{what}: the slab has unwritten or non-finite entries"
    info = (slab.shape[0], N, ops.relpos_index_csr(c["index"].to(DEV), n_bins))
    dtable = torch.empty((n_bins, H), device=DEV)
    ops.relpos_bias_scatter(slab, dtable, B, H, info, n_bins)
    torch.cuda.synchronize()
    gt = c["gt"]
    err = (dtable.cpu().double() - gt).abs().max().item()
    print(f"EDGES isolation {what}: dtable {err:.3e} (max |gt| {gt.abs().max().item():.3e})")
    if c["bias_kind"] == "table":
        assert err / gt.abs().max().item() < 1e-2, f"{what}: dtable {err}"
    else:
        assert err < (1e-4 if c["mode"] == "fp32" else 6e-2) * max(1.0, gt.abs().max().item()), f"{what}: dtable max err {err}"
    assert F.guards_intact(s.handles["slab"]), f"{what}: the slab reduction wrote outside the slab"


def _isolation(mode, B, H, D, N, bias, split=False, poisoned=True):
    c = _case_inputs(mode, B, H, D, N, bias)
    every = list(range(B))
    fwd_names = ["out", "lse"] + (["hi", "lo"] if split else [])
    bwd_names = ["dqkv", "delta"] + (["dhi", "dlo"] if split else []) + ([] if poisoned or not bias else ["slab"])
    # the plain call, twice: bit-reproducible, or the comparison below means nothing
    plain_f, again_f = _forward(c, split, False, None), _forward(c, split, False, None)
    for name in fwd_names:
        assert _same_bits(plain_f[name], again_f[name], every), f"two plain forward calls differ in `{name}`"
    plain_b, again_b = _backward(c, split, False, None, plain_f), _backward(c, split, False, None, plain_f)
    for name in bwd_names:
        assert _same_bits(plain_b[name], again_b[name], list(range(plain_b[name].shape[0]))), f"two plain backward calls differ in `{name}`"
    _check_forward(c, split, plain_f, every, "plain")
    _check_backward(c, split, plain_b, every, "plain")
    for parity in ((1, 0) if poisoned else (None,)):
        real = [b for b in every if b % 2 != parity]
        what = f"framed, samples b % 2 == {parity} NaN" if poisoned else "framed"
        sf = _forward(c, split, True, parity)
        sf.check(what + ", forward")
        _check_forward(c, split, sf, real, what)
        for name in fwd_names:
            assert _same_bits(sf[name], plain_f[name], real), f"{what}: `{name}` differs from the plain call's"
        sb = _backward(c, split, True, parity, plain_f)
        sb.check(what + ", backward")
        _check_backward(c, split, sb, real, what)
        for name in bwd_names:
            assert _same_bits(sb[name], plain_b[name], real if name != "slab" else list(range(sb[name].shape[0]))), f"{what}: `{name}` differs from the plain call's"
        if "slab" in bwd_names:
            _check_table_gradient(c, sb, what)


@pytest.mark.parametrize("N", [129, 197, 255])
def test_isolation_q32_no_bias(N):
    """32-row forward, dQ and dK / dV without a bias (bf16, B * H = 96): 8 waves at 5 and 7 tiles, 4 waves at 8; all ragged."""
    _isolation("bf16", 8, 12, 64, N, None)


@pytest.mark.parametrize("N", [193, 255])
def test_isolation_q32_dense_forward_register_backward(N):
    """32-row DENSE forward; a ragged N with dense rows sends the backward to the register kernels (no index, so no slab)."""
    _isolation("bf16", 8, 12, 64, N, "dense")


def test_isolation_pipelined_forward():
    """N = 128 is below the 32-row kernels' range: the 16-row pipelined forward and backward (dm_attention_pipe.hip)."""
    _isolation("bf16", 8, 12, 64, 128, None)


@pytest.mark.parametrize("bias", [None, "dense"], ids=["nobias", "dense"])
@pytest.mark.parametrize("mode,N", [("fp32", 37), ("bf16", 100)])
def test_isolation_register_kernels(mode, N, bias):
    """B * H = 8 keeps bf16 on the register kernels (dm_attention.hip); fp32 is always theirs.  N = 37: a ragged 16-key tile in a
    single 64-row block; N = 100: two blocks, the second ragged."""
    _isolation(mode, 4, 2, 64, N, bias)


@pytest.mark.parametrize("N", [129, 197, 255])
def test_isolation_split(N):
    """The split-bf16 entry points without a table (dm_attention_x3.hip): qkv, its two images, dout and its two images framed."""
    _isolation("fp32", 4, 3, 64, N, None, split=True)


@pytest.mark.parametrize("mode,B,H,D,N,bias", [("bf16", 4, 3, 80, 257, None), ("fp32", 4, 2, 32, 300, "dense")])
def test_isolation_generic(mode, B, H, D, N, bias):
    """dm_attention_generic.hip: a head dim other than 64, more than 256 tokens."""
    _isolation(mode, B, H, D, N, bias)


@pytest.mark.parametrize("N,bias", [(193, "index"), (256, "index"), (192, "table")], ids=["register-193", "q32-dq-pipe-dkv-256", "table-192"])
def test_isolation_slab(N, bias):
    """The calls that fill the bias-gradient slab (guards only: the slab sums over the samples), bf16, B = 8, H = 12.
    193 + dense rows: the register kernels, whose dQ pass sums the slab; 256 + dense rows: 32-row dQ and the pipelined dK / dV,
    which sums it; 192 + the (3, 8, 8) table: table forward, table dQ and the table-reading dK / dV.  The slab's guards, and the
    table gradient against fp64 as in test_attention_forward_backward / test_attention_relpos_table_in_kernel."""
    _isolation("bf16", 8, 12, 64, N, bias, poisoned=False)
