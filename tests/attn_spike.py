"""Spiked softmax rows for the attention kernels' deferred-maximum rescale, and float32 restatements of what the kernels compute.
Plain numpy and torch on the CPU: tests/test_attn_spike_host.py checks the data and the tolerances here, tests/test_gpu_attention_spikes.py
runs the kernels on it.

dm_attention_q32.hip and dm_attention_x3.hip take the softmax reference maximum m from the first 32-key tile.  A later tile moves it only
when one of its scores, seen by one lane half, is more than 2^16 above (`tile_max`); the whole wave then follows the ballot, the new m is
the ROW maximum (`half_max`), and O and the row sums are multiplied by 2^(m - mn) in their accumulator registers (`rescale_o`).  On random
operands no tile ever grows.  Here q and k carry, behind 55 random dimensions, one dimension that shifts a whole row and one dimension
per key tile that lifts ONE key of the tile for chosen rows by a chosen gap:

  d = 55        k[:, 55] = K_SHIFT, q[r, 55] = c_r / K_SHIFT with c_r in {0, +C, -C}: every score of row r moves by c_r * scale;
  d = 56 + t    k[j_t, 56 + t] = K_SPIKE for the spike key j_t of tile t = 1 .. NKT - 1, q[r, 56 + t] = a_r / K_SPIKE for the rows
                assigned to tile t: the bf16 value nearest to what puts score(r, j_t) the target gap (log2 units: score * log2 e,
                scale and bias included) above the row's running reference -- the first-tile maximum, moved to the row maximum of
                every earlier tile at which the row's WAVE rescaled (second spike of a "double" row: above its first spike).

Each reserved product is split between q and k (powers of two, so nothing is rounded) because the backward pass multiplies dS by
these operands: on a row that one key dominates, dS = P (dP - delta) is pure rounding noise (about 1e-2 with a bf16 `out` in delta),
and with k = 1 and a_r up to 1700 on the q side it lands in dk[j_t, 56 + t] at about 1 -- past the bf16 dqkv bound for every G_top
down to 40 (measured on plain_backward); likewise +-256 on the q side of the shift puts the bf16 rounding of dS into dk[:, 55] at
0.7 of the bound.  With a_r / 32 against 32 and c_r / 16 against 16 neither gradient sees an operand above 53.  All values are bf16
numbers, so the split-bf16 kernels' lo planes are zero.

Targets cycle through TARGETS = none, 15, 17, 40, G_top.  A unit (b, h) has rot = b * H + h and is of kind (b + h) % 4:

  dense    row r spikes in tile (r + rot) % NKT (tile 0: no spike), target TARGETS[(r // NKT + rot) % 5]: every wave rescales at every tile;
  plain    no spikes (the common path, beside rescaling units of the same persistent workgroup);
  single   per 32-row block one row that grows (17, 40 or G_top) and one row of gap 15 in another tile, which must cause no event;
  double   rows with (r + rot) % 4 == 0 spike by 17 in tile t and by 40 above that in tile t + 2.

The spike key of tile t sits in lane half (t + 1 + rot) & 1 (a half hh holds the keys with (key & 4) == 4 hh), i.e. half 0 for odd t
and half 1 for even t in even units, the other way round in odd ones.  In the last tile the spike key of even units is N - 1, next to
the masked columns; odd units take the last key of the other half where the tile has one.
"""
import functools
import types

import numpy as np
import torch

from attn_frame import attn_ref

D = 64
SCALE = 0.125
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
RESCALE_LOG2 = 16.0
G_TOP = 300.0               # log2 units: 2^-300 and every earlier probability flush to zero in fp32
SHIFT_C = 256.0             # raw units: c_r * scale = +-32 natural units
K_SHIFT = 16.0              # k[:, 55]; q[r, 55] = c_r / K_SHIFT
K_SPIKE = 32.0              # k[j_t, 56 + t]; q[r, 56 + t] = a_r / K_SPIKE
KINDS = ("dense", "plain", "single", "double")
NEG_BIG = -1e30


def bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def targets(g_top):
    return (None, 15.0, 17.0, 40.0, float(g_top))


def spike_key(N, t, rot):
    """The spike key of tile t in unit `rot`."""
    nkt = (N + 31) // 32
    half = (t + 1 + rot) & 1
    if t < nkt - 1:
        return 32 * t + 8 * ((t + rot) % 4) + 4 * half + (rot // 2) % 4
    if rot % 2 == 0:
        return N - 1
    other = [j for j in range(32 * t, N) if (j & 4) != ((N - 1) & 4)]
    return other[-1] if other else N - 1


def _relpos_index(cube):
    s, h, w = cube
    z, y, x = np.meshgrid(np.arange(s), np.arange(h), np.arange(w), indexing="ij")
    z, y, x = z.reshape(-1), y.reshape(-1), x.reshape(-1)
    return ((z[:, None] - z[None] + s - 1) * (2 * h - 1) * (2 * w - 1) + (y[:, None] - y[None] + h - 1) * (2 * w - 1) + x[:, None] - x[None] + w - 1).astype(np.int64)


@functools.lru_cache(maxsize=2)
def spike_case(N, B, H, bias_mode=None, dtype="bf16", seed=0, C=SHIFT_C, g_top=G_TOP):
    """bias_mode: None, "dense" (a random [157, H] table gathered through a random [N, N] index, as test_attention_forward_backward
    has it, so that the table gradient is defined) or "table" (the (N / 64, 8, 8) token cube's table and index).  dtype names the
    kernels' numerics: "bf16", "x3" (fp32 tensors, split-bf16 products) or "fp32"; the operands are bf16 numbers in all three.
    Returns a namespace: qkv [B, N, 3, H, 64] fp32, dout, table / index / bias (fp32 [H, N, N]) or None, o_ref / lse_ref (fp64),
    lse_ref0 (fp64, the same rows without their shift), and the per-row record kind [B, H], shift [B, H, N] (c_r),
    spike_tile / spike_gap [B, H, N, 2] (-1 / nan: none), keys [B, H, NKT] (-1 for tile 0)."""
    nkt = (N + 31) // 32
    assert 5 <= nkt <= 8 or bias_mode is None, "the reserved dimensions 57 .. 63 serve tiles 1 .. 7"
    rng = np.random.default_rng(seed)
    qkv = bf16(torch.from_numpy(rng.normal(size=(B, N, 3, H, D)).astype(np.float32)))
    dout = bf16(torch.from_numpy(rng.normal(size=(B, N, H * D)).astype(np.float32)))
    qkv[:, :, 0:2, :, 55:] = 0.0
    qkv[:, :, 1, :, 55] = K_SHIFT
    table = index = bias = cube = None
    n_bins = 0
    if bias_mode == "dense":
        n_bins = 157
        table = torch.from_numpy(rng.normal(size=(n_bins, H)).astype(np.float32))
        index = torch.from_numpy(rng.integers(0, n_bins, size=(N, N)).astype(np.int64))
    elif bias_mode == "table":
        assert N % 64 == 0
        cube = (N // 64, 8, 8)
        n_bins = (2 * cube[0] - 1) * 225
        table = torch.from_numpy(rng.normal(size=(n_bins, H)).astype(np.float32))
        index = torch.from_numpy(_relpos_index(cube))
    if table is not None:
        bias = table[index.reshape(-1)].reshape(N, N, H).permute(2, 0, 1).contiguous()
    tg = targets(g_top)
    kind = np.zeros((B, H), np.int64)
    shift = np.zeros((B, H, N), np.float32)
    spike_tile = np.full((B, H, N, 2), -1, np.int64)
    spike_gap = np.full((B, H, N, 2), np.nan)
    keys = np.full((B, H, nkt), -1, np.int64)
    rows = np.arange(N)
    for b in range(B):
        for h in range(H):
            rot = b * H + h
            kd = KINDS[(b + h) % 4]
            kind[b, h] = (b + h) % 4
            base = qkv[b, :, 0, h, :55].double() @ qkv[b, :, 1, h, :55].double().T              # raw q . k of the random dimensions
            bh = torch.zeros((N, N), dtype=torch.float64) if bias is None else bias[h].double()
            nat = SCALE * base + bh                                                              # natural units, unshifted
            c = np.array([0.0, C, -C], np.float32)[(rows + rot) % 3]
            shift[b, h] = c
            qkv[b, :, 0, h, 55] = torch.from_numpy(c / np.float32(K_SHIFT))
            for t in range(1, nkt):
                keys[b, h, t] = spike_key(N, t, rot)
                qkv[b, keys[b, h, t], 1, h, 56 + t] = K_SPIKE

            # the plan: per tile, (rows, target gap, slot) -- placed tile by tile below, against the running reference
            plan = {t: [] for t in range(1, nkt)}
            if kd == "dense":
                tt = (rows + rot) % nkt
                gi = (rows // nkt + rot) % 5
                for g in range(1, 5):
                    for t in range(1, nkt):
                        rr = rows[(tt == t) & (gi == g)]
                        if len(rr):
                            plan[t].append((rr, tg[g], 0))
            elif kd == "single":
                for blk in range((N + 31) // 32):
                    nrow = min(32, N - 32 * blk)
                    r0 = 32 * blk + (7 * rot + 5 * blk) % nrow
                    plan[1 + (rot + blk) % (nkt - 1)].append((np.array([r0]), tg[2 + (rot // 4 + blk) % 3], 0))
                    if nrow > 1:
                        r1 = 32 * blk + (7 * rot + 5 * blk + 11) % nrow
                        r1 = r1 if r1 != r0 else 32 * blk + (r0 - 32 * blk + 1) % nrow
                        plan[1 + (rot + blk + 1) % (nkt - 1)].append((np.array([r1]), 15.0, 0))
            elif kd == "double":
                rr = rows[(rows + rot) % 4 == 0]
                tt = 1 + (rr // 4 + rot) % (nkt - 3)
                for t in range(1, nkt - 2):
                    if (tt == t).any():
                        plan[t].append((rr[tt == t], 17.0, 0))
                        plan[t + 2].append((rr[tt == t], 40.0, 1))
            # The gap is set over the row's RUNNING reference: the first-tile maximum, moved to the row maximum of every earlier tile at
            # which the row's wave rescaled (the kernels' rule, followed here in fp64) -- what `grow` compares with.
            m_run = nat[:, :32].amax(1)
            for t in range(1, nkt):
                lo, hi, j = 32 * t, min(N, 32 * t + 32), keys[b, h, t]
                for rr, gap, slot in plan[t]:
                    a = bf16(((((gap / LOG2E + m_run[rr] - bh[rr, j]) / SCALE) - base[rr, j]) / K_SPIKE).float())      # a_r / K_SPIKE: a bf16 value
                    qkv[b, rr, 0, h, 56 + t] = a
                    nat[rr, j] = SCALE * (base[rr, j] + a.double() * K_SPIKE) + bh[rr, j]
                    spike_tile[b, h, rr, slot] = t
                    spike_gap[b, h, rr, slot] = gap
                th = _tile_half_max(nat[:, lo:hi], lo, hi)
                ballot = _wave_any((((th - m_run[:, None]) * LOG2E) > RESCALE_LOG2).any(-1))
                m_run = torch.where(ballot, torch.maximum(m_run, th.amax(-1)), m_run)
    q64 = qkv.double()
    b64 = None if bias is None else bias.double()
    o_ref, lse_ref = attn_ref(q64, b64, SCALE)
    lse_ref0 = lse_ref - torch.from_numpy(shift).double() * SCALE       # fp64: the shift is exact in the scores
    return types.SimpleNamespace(N=N, B=B, H=H, nkt=nkt, seed=seed, dtype=dtype, bias_mode=bias_mode, C=C, g_top=g_top, scale=SCALE, qkv=qkv, dout=dout,
                                 table=table, index=index, bias=bias, cube=cube, n_bins=n_bins, o_ref=o_ref, lse_ref=lse_ref, lse_ref0=lse_ref0,
                                 kind=kind, shift=torch.from_numpy(shift), spike_tile=spike_tile, spike_gap=spike_gap, keys=keys)


@functools.lru_cache(maxsize=2)
def _reference_backward(N, B, H, bias_mode, dtype, seed, C, g_top):
    c = spike_case(N, B, H, bias_mode, dtype, seed, C, g_top)
    q64 = c.qkv.double().requires_grad_(True)
    t64 = b64 = None
    if c.table is not None:
        t64 = c.table.double().requires_grad_(True)
        b64 = t64[c.index.reshape(-1)].reshape(N, N, H).permute(2, 0, 1)
    o, _ = attn_ref(q64, b64, SCALE)
    o.backward(c.dout.double())
    return q64.grad, None if t64 is None else t64.grad


def reference_backward(c):
    """(dqkv, dtable or None) in fp64 by autograd on attn_ref, for the case's dout."""
    return _reference_backward(c.N, c.B, c.H, c.bias_mode, c.dtype, c.seed, c.C, c.g_top)


# ---- the deferred rule in fp64: which (row, tile) rescale ----------------------------------------------------------------------------
def _wave_any(x):
    """any() over the 32 rows of a wave (rows 32 w .. 32 w + 31), broadcast back to the rows: x [..., N] bool."""
    n = x.shape[-1]
    pad = (-n) % 32
    y = torch.nn.functional.pad(x, (0, pad)).reshape(*x.shape[:-1], -1, 32).any(-1, keepdim=True)
    return y.expand(*x.shape[:-1], (n + pad) // 32, 32).reshape(*x.shape[:-1], n + pad)[..., :n]


def _half_of_keys(lo, hi):
    return (torch.arange(lo, hi) & 4) >> 2


def _tile_half_max(st, lo, hi):
    """[..., N, 2]: the maximum of tile scores st [..., N, hi - lo] over the keys of each lane half (NEG_BIG where a half has none)."""
    kh = _half_of_keys(lo, hi)
    out = []
    for hh in (0, 1):
        sel = st[..., kh == hh]
        out.append(sel.amax(-1) if sel.shape[-1] else torch.full(st.shape[:-1], NEG_BIG, dtype=st.dtype))
    return torch.stack(out, -1)


def deferred_events(c):
    """The kernels' rule in fp64 (log2 units).  Returns gap [B, H, N, NKT, 2] (the half's tile maximum over the running reference; nan
    for tile 0 and for a half without valid keys), grow (gap > 16) and resc [B, H, N, NKT] (the row's wave rescales at this tile)."""
    q, k = c.qkv[:, :, 0].permute(0, 2, 1, 3).double(), c.qkv[:, :, 1].permute(0, 2, 1, 3).double()
    s = (q @ k.transpose(-1, -2)) * SCALE
    if c.bias is not None:
        s = s + c.bias.double()[None]
    s = s * LOG2E
    gap = torch.full((c.B, c.H, c.N, c.nkt, 2), float("nan"), dtype=torch.float64)
    resc = torch.zeros((c.B, c.H, c.N, c.nkt), dtype=torch.bool)
    m = s[..., :32].amax(-1)
    for t in range(1, c.nkt):
        lo, hi = 32 * t, min(c.N, 32 * t + 32)
        th = _tile_half_max(s[..., lo:hi], lo, hi)
        g = th - m[..., None]
        gap[..., t, :] = torch.where(th > NEG_BIG / 2, g, torch.full_like(g, float("nan")))
        ballot = _wave_any((g > RESCALE_LOG2).any(-1))
        resc[..., t] = ballot
        m = torch.where(ballot, torch.maximum(m, th.amax(-1)), m)
    return gap, gap > RESCALE_LOG2, resc


# ---- float32 restatements ------------------------------------------------------------------------------------------------------------
def _operands(c):
    q, k, v = (c.qkv[:, :, i].permute(0, 2, 1, 3).contiguous() for i in range(3))
    return q, k, v


def scores32(c):
    """Raw q . k (+ bias / scale) as the matrix pipe accumulates it: the bias over the scale is the C operand, each 16-wide k-step
    is summed exactly and added with one fp32 rounding."""
    q, k, _ = _operands(c)
    acc = torch.zeros((c.B, c.H, c.N, c.N), dtype=torch.float32)
    if c.bias is not None:
        acc = acc + (c.bias * torch.tensor(1.0 / SCALE, dtype=torch.float32))[None]
    for ks in range(4):
        sl = slice(16 * ks, 16 * ks + 16)
        acc = (acc.double() + q[..., sl].double() @ k[..., sl].double().transpose(-1, -2)).float()
    return acc


def round_p(p, mode):
    """The probabilities as the second product reads them: bf16; a bf16 pair hi + lo (16 bits); fp32 as they are."""
    if mode == "bf16":
        return bf16(p)
    if mode == "x3":
        hi = bf16(p)
        return hi + bf16(p - hi)
    return p


def _finish(c, mode, o, l, m):
    """o [B, H, N, 64], l broadcastable to it, m [B, H, N] -> out [B, N, H * 64] (rounded to the mode's output type), lse [B, H, N]."""
    scale2 = torch.tensor(SCALE * LOG2E, dtype=torch.float32)
    out = o * (1.0 / l)
    if mode == "bf16":
        out = bf16(out)
    lse = (m * scale2 + torch.log2(l[..., 0])) * torch.tensor(LN2, dtype=torch.float32)
    return out.permute(0, 2, 1, 3).reshape(c.B, c.N, c.H * D), lse


def plain_restatement(c, mode=None):
    """Whole-row softmax with the kernels' operand roundings: the model the tolerances are measured against."""
    mode = mode or c.dtype
    s = scores32(c)
    v = _operands(c)[2]
    scale2 = torch.tensor(SCALE * LOG2E, dtype=torch.float32)
    m = s.amax(-1)
    msc = -(m * scale2)
    p = torch.exp2((s.double() * scale2.double() + msc[..., None].double()).float())
    pb = round_p(p, mode)
    l = pb.sum(-1, keepdim=True)
    o = (pb.double() @ v.double()).float()
    return _finish(c, mode, o, l, m)


FAULTS = ("l_not_rescaled", "o_not_rescaled", "half_local_maximum")


def deferred_restatement(c, mode=None, fault=None):
    """The kernels' rule in float32: the reference maximum is tile 0's; a later tile moves it when a lane half sees a score more than
    2^16 above; the whole wave follows the ballot; the new maximum is the row's; O and l are multiplied by 2^(m - mn).  State is kept
    per lane half (a lane holds the output columns with (d & 4) == 4 hh and its own copy of m and l), so that the three faulty
    variants can be stated: `fault` in FAULTS."""
    mode = mode or c.dtype
    assert fault is None or fault in FAULTS
    s = scores32(c)
    v = _operands(c)[2]
    scale2 = torch.tensor(SCALE * LOG2E, dtype=torch.float32)
    dhalf = (torch.arange(D) & 4) >> 2
    m1 = s[..., :32].amax(-1)
    m = torch.stack([m1, m1], -1)                                   # [B, H, N, 2]
    l = torch.zeros_like(m)
    o = torch.zeros((c.B, c.H, c.N, D), dtype=torch.float32)
    for t in range(c.nkt):
        lo, hi = 32 * t, min(c.N, 32 * t + 32)
        st = s[..., lo:hi]
        kh = _half_of_keys(lo, hi)
        if t > 0:
            th = _tile_half_max(st, lo, hi)
            grow = (th - m) * scale2 > RESCALE_LOG2
            ballot = _wave_any(grow.any(-1))[..., None]
            new = torch.maximum(m, th if fault == "half_local_maximum" else th.amax(-1, keepdim=True))
            mn = torch.where(ballot, new, m)
            alpha = torch.exp2((m - mn) * scale2)
            if fault != "l_not_rescaled":
                l = l * alpha
            if fault != "o_not_rescaled":
                o = o * alpha[..., dhalf]
            m = mn
        msc = -(m * scale2)
        p = torch.exp2((st.double() * scale2.double() + msc[..., kh].double()).float())
        pb = round_p(p, mode)
        l = l + pb.sum(-1, keepdim=True)
        o = (o.double() + pb.double() @ v[..., lo:hi, :].double()).float()
    return _finish(c, mode, o, l[..., dhalf], m[..., 0])      # (column 0 is half 0's: the lane that stores lse)


def plain_backward(c, out, lse, mode=None):
    """The backward pass with the kernels' operand roundings, from a forward's out [B, N, H * 64] and lse [B, H, N]: -lse / scale is
    folded into the scores' accumulator, P = exp2(scale2 (S - lse / scale)), dS = P (dP - delta); P and dS are rounded like the
    forward's P before their products.  Returns (dqkv, dtable or None) as float32 / float64 tensors."""
    mode = mode or c.dtype
    q, k, v = _operands(c)
    scale2 = torch.tensor(SCALE * LOG2E, dtype=torch.float32)
    s = scores32(c)
    sp = (s.double() - (lse.float() * torch.tensor(1.0 / SCALE, dtype=torch.float32))[..., None].double()).float()
    p = torch.exp2(sp * scale2)
    do = c.dout.reshape(c.B, c.N, c.H, D).permute(0, 2, 1, 3)
    oo = out.float().reshape(c.B, c.N, c.H, D).permute(0, 2, 1, 3)
    delta = (do.double() * oo.double()).sum(-1).float()
    dp = (do.double() @ v.double().transpose(-1, -2)).float()
    ds = p * (dp - delta[..., None])
    pb, dsb = round_p(p, mode), round_p(ds, mode)
    dq = (dsb.double() @ k.double()).float() * SCALE
    dk = (dsb.double().transpose(-1, -2) @ q.double()).float() * SCALE
    dv = (pb.double().transpose(-1, -2) @ do.double()).float()
    dqkv = torch.stack([dq, dk, dv], 2).permute(0, 3, 2, 1, 4).contiguous()      # [B, H, 3, N, D] -> [B, N, 3, H, D]
    if mode == "bf16":
        dqkv = bf16(dqkv)
    dtable = None
    if c.table is not None:
        dtable = torch.zeros((c.n_bins, c.H), dtype=torch.float64)
        dtable.index_add_(0, c.index.reshape(-1), ds.double().sum(0).permute(1, 2, 0).reshape(-1, c.H))
    return dqkv, dtable


# ---- the tolerances (no new constant: the bounds of the existing tests) --------------------------------------------------------------
def errors(c, out, lse, dqkv=None, dtable=None):
    """err / tol of each check for the case's numerics, as {name: (err, tol)}.  bf16: test_attention_forward_backward (forward 2e-2;
    lse rtol = atol = 2e-2; dqkv 4e-2 max(1, max |g|); dtable 6e-2 max(1, max |g|)).  x3: test_split_tile_count_matrix (forward 5e-5;
    lse 5e-5, scaled by max(1, |lse_ref|) since lse reaches ~200 here; dqkv and dtable 2e-5 of the gradient's maximum).  fp32: the
    fp32 bounds of test_attention_forward_backward (2e-5; 1e-4; 5e-5; 1e-4).  The lse figures are the worst ratio err / tol."""
    mode = c.dtype
    res = {}
    lse, lref = lse.double(), c.lse_ref
    res["fwd"] = ((out.double() - c.o_ref).abs().max().item(), {"bf16": 2e-2, "x3": 5e-5, "fp32": 2e-5}[mode])
    if mode == "x3":
        ltol = 5e-5 * lref.abs().clamp(min=1.0)
    else:
        lt = 2e-2 if mode == "bf16" else 1e-4
        ltol = lt + lt * lref.abs()
    res["lse"] = (((lse - lref).abs() / ltol).max().item(), 1.0)
    sh = c.shift != 0
    res["lse_shift"] = (((lse - (c.lse_ref0 + c.shift.double() * SCALE)).abs() / ltol)[sh].max().item(), 1.0)
    if dqkv is not None:
        g, gt = reference_backward(c)
        gm = g.abs().max().item()
        res["dqkv"] = ((dqkv.double() - g).abs().max().item(), {"bf16": 4e-2 * max(1.0, gm), "x3": 2e-5 * gm, "fp32": 5e-5 * max(1.0, gm)}[mode])
        if dtable is not None:
            tm = gt.abs().max().item()
            res["dtable"] = ((dtable.double() - gt).abs().max().item(), {"bf16": 6e-2 * max(1.0, tm), "x3": 2e-5 * tm, "fp32": 1e-4 * max(1.0, tm)}[mode])
    return res


# ---- the cases: (family, N, B, H, bias_mode, dtype) -----------------------------------------------------------------------------------
Q32_N = (129, 160, 193, 224, 255, 256)
CASES = ([("q32", n, 8, 12, bm, "bf16") for n in Q32_N for bm in (None, "dense")]
         + [("relpos", n, 8, 12, "table", "bf16") for n in (192, 256)]
         + [("split", n, 3, 4, None, "x3") for n in (129, 192, 255, 256)] + [("split", n, 3, 4, "table", "x3") for n in (192, 256)]
         + [("pipe16", 128, 8, 12, None, "bf16"), ("register", 197, 3, 4, None, "fp32")])
RESCALING = [c for c in CASES if c[0] in ("q32", "relpos", "split")]


def case_id(c):
    return f"{c[0]}-N{c[1]}-{c[4] or 'nobias'}"


def make(c):
    return spike_case(c[1], c[2], c[3], c[4], c[5], seed=c[1])
