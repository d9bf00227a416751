"""CPU references, input generators and error bounds for the HBM-bound row / element kernels (csrc/dm_rows.hip, dm_rows_wide.hip,
dm_gru.hip).  No GPU here: tests/test_rows_host.py checks this file against torch's own float64 operators and fixes the tolerance
constants; tests/test_gpu_rows.py compares the kernels with it.  Both see the same inputs through the generators below.

Every operation has
  * a float64 restatement written from its definition (`*_ref`), the truth of the GPU tests;
  * where a tolerance is needed, a float32 restatement of the kernel's arithmetic order (`*_f32`: two-pass mean and variance, fp32
    accumulators, strided partial sums folded in a tree -- not lane-exact), whose only use is to show on the CPU that honest fp32
    arithmetic stays inside the tolerance on the chosen inputs;
  * a bound `*_tol` derived from the fp32 rounding model (U = 2^-24, the unit roundoff), with an integer constant C_* in front.
    The constants are the smallest integers for which the float32 restatement stays at or below HALF the bound on the GPU tests'
    inputs (test_rows_host.py asserts it), so a correct kernel has a factor 2 of headroom.

What each restatement mirrors:
  LayerNorm       nn.LayerNorm of the reference's blocks (nets/ShfitScaleFormer.py, vit_model.py: eps 1e-6 / 1e-5), Ba et al. 2016:
                  y = (x - E[x]) / sqrt(Var[x] + eps) * gamma + beta, biased variance over the last axis.
  token pool      AvgPool2d(2, 2) over each scale's token grid (nets/ShfitScaleFormer.py:892-901, :905-914).
  group mean      AdaptiveAvgPool1d(1) per scale (nets/ShfitScaleFormer.py:930-938).
  colsum          the bias gradient of nn.Linear: db = sum over rows of dy.
  cast            torch.Tensor.bfloat16(): IEEE round-to-nearest-even to 8 significant bits, NaN stays NaN.
  Adam            torch.optim.Adam's single-tensor order (Train_SMT.py:192-193; oracle/adam.py is pinned to it).
  contrastive     Losses.py:34-38 (oracle/losses.py): mean(flag * d + (1 - flag) * relu(margin - d)), d = squared distance.
  cross-entropy   nn.CrossEntropyLoss, mean reduction (Losses.py:52-53, :83-84), index and probability targets.
  GRU cell        nn.GRU's step (Nets.py:60-66), gate order r, z, n, from the two projections gi and gh.
"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24                 # fp32 unit roundoff
UB = 2.0 ** -8                 # bf16 unit roundoff (8 significant bits)

# ---- tolerance constants (fixed by tests/test_rows_host.py; the table is at the top of tests/test_gpu_rows.py) ----------------------
C_LN_Y = 7
C_LN_MEAN = 4
C_LN_RSTD = 6
C_LN_DX = 5
C_LN_DG = 3
C_BF16 = 2                     # a single rounding to bf16 reaches 2^-8 relative by itself: 2 * 2^-8 keeps the factor 2
C_COLSUM = 1
C_ADAM_M = 3
C_ADAM_V = 6
C_ADAM_P = 6
C_CL_LOSS = 1
C_CL_GRAD = 3
C_CE_LOSS = 1
C_CE_GRAD = 5
C_GRU_FWD = 4                  # the issue's floor: never below 4 * 2^-24
C_GRU_BWD = 3


def _rng(*key):
    return np.random.default_rng([int(k) & 0xFFFFFFFF for k in key])


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def worst(err, tol):
    """max err / tol over all elements (0 / 0 counts as 0, anything / 0 as inf)."""
    err, tol = torch.as_tensor(err, dtype=torch.float64).reshape(-1), torch.as_tensor(tol, dtype=torch.float64).reshape(-1)
    if tol.numel() == 1 and err.numel() > 1:
        tol = tol.expand_as(err)
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    return float(r.max()) if r.numel() else 0.0


# =====================================================================================================================================
# LayerNorm
# =====================================================================================================================================
LN_EPS = 1e-5
LN_MU = 1.0e3                  # common offset of the "large offset" rows
LN_FAMILIES = ("normal", "offset", "small", "large", "const")
LN_WIDTHS = (4, 100, 252, 256, 260, 764, 768, 772, 1020, 1024, 1028, 1284, 8188, 8192)
LN_ROWS = (1, 3, 5, 67)
LN_OPTION_WIDTHS = (100, 768, 772, 1024, 1028)
LN_CAP_CASES = ((4 * 768 + 1, 256), (4 * 2048 + 1, 256), (4 * 4096 + 1, 1028))      # backward cap, forward cap, wide-path cap


def ln_family(row, rows):
    """Family of a row.  A one-row tensor is a large-offset row (the hardest one); otherwise the families cycle."""
    return "offset" if rows == 1 else LN_FAMILIES[row % len(LN_FAMILIES)]


@functools.lru_cache(maxsize=2)
def ln_inputs(rows, cols, mu=LN_MU):
    """fp32 x [rows, cols] with one family per row, gamma ~ N(1, 0.2), beta ~ N(0, 1), dy, dres ~ N(0, 1), g0 (what the
    accumulating backward adds to).  Constant rows hold small integers, for which the fp32 mean is exact (every partial sum of
    <= 8192 copies is representable), so y == beta and xhat == 0 exactly in any fp32 evaluation order."""
    r = _rng(11, rows, cols)
    x = r.standard_normal((rows, cols), dtype=np.float32)
    for i in range(rows):
        f = ln_family(i, rows)
        if f == "offset":
            x[i] += np.float32(mu if (i // 5) % 2 == 0 else -mu)
        elif f == "small":
            x[i] *= np.float32(1e-3)
        elif f == "large":
            x[i] *= np.float32(1e3)
        elif f == "const":
            x[i] = np.float32((i % 7) - 3)
    out = dict(x=_t(x), gamma=_t(1 + 0.2 * r.standard_normal(cols, dtype=np.float32)), beta=_t(r.standard_normal(cols, dtype=np.float32)),
               dy=_t(r.standard_normal((rows, cols), dtype=np.float32)), dres=_t(r.standard_normal((rows, cols), dtype=np.float32)),
               g0=_t(r.standard_normal(cols, dtype=np.float32)))
    out["const_rows"] = torch.tensor([ln_family(i, rows) == "const" for i in range(rows)])
    out["offset_rows"] = torch.tensor([ln_family(i, rows) == "offset" for i in range(rows)])
    return out


def layernorm_ref(x, gamma, beta, eps=LN_EPS):
    """float64 (y, mean, rstd, xhat) from the definition."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + float(np.float32(eps)))
    xhat = (x - mean) * rstd
    return xhat * gamma.double() + beta.double(), mean.squeeze(-1), rstd.squeeze(-1), xhat


@functools.lru_cache(maxsize=2)
def ln_truth(rows, cols, bf16_dy=False):
    """float64 truth of one generated case, forward and (autograd) backward; dx without the residual gradient."""
    d = ln_inputs(rows, cols)
    dy = d["dy"].bfloat16().float() if bf16_dy else d["dy"]
    x, g, b = d["x"].double().requires_grad_(True), d["gamma"].double().requires_grad_(True), d["beta"].double().requires_grad_(True)
    y, mean, rstd, xhat = layernorm_ref(x, g, b)
    (y * dy.double()).sum().backward()
    return dict(y=y.detach(), mean=mean.detach(), rstd=rstd.detach(), xhat=xhat.detach(), dx=x.grad, dgamma=g.grad, dbeta=b.grad, dy=dy)


def _wave_sum(v):
    """The 64-lane xor butterfly = folding halves."""
    n = v.shape[-1]
    while n > 1:
        n //= 2
        v = v[..., :n] + v[..., n:2 * n]
    return v[..., 0]


def _chunks(x):
    """[rows, cols] -> ([rows, I, 64, 4] zero padded, valid [I, 64]): lane l holds the float4 chunks l, l + 64, ..."""
    rows, cols = x.shape
    nch = cols // 4
    I = (nch + 63) // 64
    xp = torch.nn.functional.pad(x, (0, I * 256 - cols)).view(rows, I, 64, 4)
    return xp, (torch.arange(I * 64) < nch).view(I, 64)


def layernorm_fwd_f32(x, gamma, beta, eps=LN_EPS, one_pass=False):
    """fp32 restatement of layernorm_fwd_kernel / layernorm_wide_fwd_kernel: per-lane sums over the lane's chunks, butterfly, a second
    pass over x - mean for the variance.  one_pass=True is DELIBERATELY WRONG (E[x^2] - mean^2): the bound must reject it."""
    x = x.float()
    rows, cols = x.shape
    xp, valid = _chunks(x)
    s = torch.zeros(rows, 64)
    for i in range(xp.shape[1]):
        v = xp[:, i]
        s = s + ((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3]))
    fc = torch.tensor(float(cols), dtype=torch.float32)
    mean = _wave_sum(s) / fc
    q = torch.zeros(rows, 64)
    for i in range(xp.shape[1]):
        for e in range(4):
            d = xp[:, i, :, e] if one_pass else xp[:, i, :, e] - mean[:, None]
            q = q + torch.where(valid[i], d * d, torch.zeros(()))
    var = _wave_sum(q) / fc
    if one_pass:
        var = var - mean * mean
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    y = (x - mean[:, None]) * rstd[:, None] * gamma.float() + beta.float()
    return y, mean, rstd


def _strided_tree_sum(terms, lanes):
    """sum over rows of terms [rows, cols] as `lanes` grid-strided fp32 accumulators folded in a tree."""
    rows, cols = terms.shape
    lanes = max(1, min(lanes, rows))
    p2 = 1 << (lanes - 1).bit_length()
    acc = torch.zeros(p2, cols)
    for k in range(0, rows, lanes):
        blk = terms[k:k + lanes]
        acc[:blk.shape[0]] += blk
    while p2 > 1:
        p2 //= 2
        acc = acc[:p2] + acc[p2:2 * p2]
    return acc[0]


def layernorm_bwd_f32(dy, x, gamma, mean, rstd, dres=None, g0=None):
    """fp32 restatement of layernorm_bwd_kernel / layernorm_wide_{dx,param}_kernel + partial_reduce_kernel.
    Returns (dx, dgamma, dbeta); g0 = (dgamma0, dbeta0) is added (accumulate)."""
    dy, x, gamma = dy.float(), x.float(), gamma.float()
    rows, cols = x.shape
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    gp, valid = _chunks(g)
    hp, _ = _chunks(g * xh)
    s1, s2 = torch.zeros(rows, 64), torch.zeros(rows, 64)
    for i in range(gp.shape[1]):
        for e in range(4):
            s1 = s1 + gp[:, i, :, e]
            s2 = s2 + hp[:, i, :, e]
    fc = torch.tensor(float(cols), dtype=torch.float32)
    c1, c2 = _wave_sum(s1) / fc, _wave_sum(s2) / fc
    dx = rstd[:, None] * (g - c1[:, None] - xh * c2[:, None])
    if dres is not None:
        dx = dx + dres.float()
    lanes = 4 * min((rows + 3) // 4, 768) if cols <= 1024 else 16 * max(1, min(64, rows // 64))
    dg, db = _strided_tree_sum(dy * xh, lanes), _strided_tree_sum(dy, lanes)
    if g0 is not None:
        dg, db = g0[0].float() + dg, g0[1].float() + db
    return dx, dg, db


def ln_mean_tol(x):
    """|mean - truth| <= C * U * max|x|: a sum of n fp32 terms in a tree of depth ~log n around an offset is off by a few U * max|x|."""
    return C_LN_MEAN * U * x.double().abs().amax(-1)


def ln_rstd_tol(x, t):
    """Relative error of rstd: C * U from the squares, their sum, the division and the root; the error dm of the mean adds dm^2 to the
    variance (the first-order term sum(x - mean) vanishes), i.e. (dm * rstd)^2 / 2 relative."""
    return t["rstd"] * (C_LN_RSTD * U + 0.5 * (ln_mean_tol(x) * t["rstd"]) ** 2)


def ln_y_tol(x, gamma, t, bf16=False):
    """C * U * (max|x - mean| * rstd * |gamma| * (1 + |mean| / std) + |y|), std = 1 / rstd = sqrt(var + eps).
    The error of the fp32 mean is a few U * |mean|; it moves every x - mean by that much, which relative to the row's spread
    max|x - mean| is |mean| / std after scaling by rstd; the remaining operations are each relative U of their result (|xhat * gamma|
    and |y|).  bf16 output: one more rounding of relative 2^-8 (times C_BF16)."""
    xd = x.double()
    spread = (xd - t["mean"][:, None]).abs().amax(-1) * t["rstd"]
    tol = C_LN_Y * U * ((spread * (1 + t["mean"].abs() * t["rstd"]))[:, None] * gamma.double().abs() + t["y"].abs())
    return tol + C_BF16 * UB * (t["y"].abs() + tol) if bf16 else tol


def ln_dx_tol(x, gamma, t, dres=None):
    """dx = dres + rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma.  With G = max|g| and X = max(1, max|xhat|) of the row
    each of the three terms is at most G * X^2 and carries a few U of relative error; the error U * |mean| of the forward's mean moves
    xhat by U * |mean| * rstd, which enters through xhat and through mean(g * xhat): G * X * |mean| * rstd.  Plus U * (|dres| + |dx|) of
    the last additions."""
    G = (t["dy"].double() * gamma.double()).abs().amax(-1)
    X = t["xhat"].abs().amax(-1).clamp(min=1.0)
    row = t["rstd"] * G * X * (X + t["mean"].abs() * t["rstd"])
    dx = t["dx"] + (dres.double() if dres is not None else 0)
    return C_LN_DX * U * (row[:, None] + dx.abs() + (dres.double().abs() if dres is not None else 0))


def ln_dgb_tol(t, g0=None):
    """dgamma_j = sum_r dy * xhat, dbeta_j = sum_r dy: C * U * sum_r |dy| * (|xhat| + |mean| * rstd) resp. C * U * sum_r |dy| per term
    rounding and the mean's error, times a summation depth of (1 + log2 rows) for the strided accumulators and the reduction tree;
    an accumulating call adds U * |result| once more."""
    dy = t["dy"].double().abs()
    rows = dy.shape[0]
    depth = 1 + math.log2(rows) if rows > 1 else 1
    tg = C_LN_DG * U * depth * (dy * (t["xhat"].abs() + (t["mean"].abs() * t["rstd"])[:, None])).sum(0)
    tb = C_LN_DG * U * depth * dy.sum(0)
    if g0 is not None:
        tg = tg + C_LN_DG * U * (t["dgamma"] + g0.double()).abs()
        tb = tb + C_LN_DG * U * (t["dbeta"] + g0.double()).abs()
    return tg, tb


# =====================================================================================================================================
# token pool / group mean: inputs on the grid 2^-10 * [-4096, 4096], so sums of <= 7 terms are exact in fp32
# =====================================================================================================================================
TOKEN_POOL_SHAPES = ((1, 1, 2, 4), (2, 3, 4, 100), (3, 4, 8, 192), (2, 1, 16, 768))
TOKEN_POOL_BIG = (24, 4, 16, 768)                 # > 4096 * 256 float4 work items in both directions
GROUP_MEAN_CASES = ((1, 1, 4), (5, 3, 100), (13, 4, 192), (9, 7, 100), (31, 7, 768), (5463, 3, 768))      # (rows, g, C); the last: > 4096 * 256 float4 items both ways


def grid_values(shape, *key):
    g = torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) & 0x7FFFFFFF)
    return torch.randint(-4096, 4097, tuple(shape), generator=g).float() / 1024.0


def token_pool_ref(x, S, side):
    """[B, S * side^2, C] -> [B, S * (side/2)^2, C]: the mean of each 2 x 2 block of every scale's side x side token grid."""
    B, _, C = x.shape
    h = side // 2
    v = x.reshape(B, S, h, 2, h, 2, C)
    return ((v[:, :, :, 0, :, 0] + v[:, :, :, 0, :, 1]) + (v[:, :, :, 1, :, 0] + v[:, :, :, 1, :, 1])).mul(0.25).reshape(B, S * h * h, C)


def group_mean_ref(x, g):
    C = x.shape[-1]
    return x.reshape(-1, g, C).sum(1) / g


# =====================================================================================================================================
# colsum
# =====================================================================================================================================
COLSUM_M = (1, 16, 255, 256, 257, 1234, 16385, 70000)
COLSUM_N_VEC = (4, 60, 64, 68, 768)
COLSUM_N_GEN = (1, 10, 250)


@functools.lru_cache(maxsize=1)
def colsum_base():
    """One [70000, 776] fp32 matrix; every case is a corner of it (N(0,1) * 10^U(-2,1) per element)."""
    r = _rng(23)
    a = r.standard_normal((70000, 776), dtype=np.float32)
    a *= np.float32(10.0) ** r.uniform(-2, 1, size=(1, 776)).astype(np.float32)
    return _t(a)


@functools.lru_cache(maxsize=1)
def colsum_base_int():
    g = torch.Generator().manual_seed(29)
    return torch.randint(-3, 4, (70000, 776), generator=g).float()


def colsum_ref(X):
    return X.double().sum(0)


def colsum_tol(X, out0=None):
    """C * M * U * sum|x| per column: the classical bound of a length-M fp32 sum in any order.  An accumulating call rounds
    out0 + sum once more: U * |result|, doubled for the factor 2 (a one-row sum has no other error)."""
    tol = C_COLSUM * X.shape[0] * U * X.double().abs().sum(0)
    return tol if out0 is None else tol + 2 * U * (out0.double() + X.double().sum(0)).abs()


def colsum_out0(N):
    return _t(_rng(59, N).standard_normal(N).astype(np.float32))


def colsum_f32(X, vec=True):
    """fp32 restatement of colsum_kernel (+ partial_reduce_kernel): row slices, 16 strided accumulators per slice (1 in the generic
    kernel), folded in order; slices folded in order."""
    X = X.float()
    M, N = X.shape
    slices = min((M + 255) // 256, 64)
    rps = (M + slices - 1) // slices
    slices = (M + rps - 1) // rps
    total = torch.zeros(N)
    for sl in range(slices):
        sub = X[sl * rps:min(M, (sl + 1) * rps)]
        lanes = 16 if vec else 1
        acc = torch.zeros(lanes, N)
        for k in range(0, sub.shape[0], lanes):
            blk = sub[k:k + lanes]
            acc[:blk.shape[0]] += blk
        s = acc[0].clone()
        for k in range(1, lanes):
            s = s + acc[k]
        total = total + s
    return total


# =====================================================================================================================================
# cast
# =====================================================================================================================================
CAST_SPECIALS = np.array([
    0x00000000, 0x80000000,                              # +0, -0
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # exact ties: to even downwards, to even upwards, both signs
    0x3F808001, 0x3F807FFF,                              # just over / under a tie
    0x7F800000, 0xFF800000,                              # +inf, -inf
    0x7FC00000, 0xFFC00001, 0x7F800001,                  # NaNs (quiet, negative with payload, signalling pattern)
    0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF,      # bf16 max, just under the overflow tie, the tie (-> inf), fp32 max (-> inf)
    0xFF7F7FFF, 0xFF7F8000,                              # the same, negative
    0x007FFFFF, 0x807FFFFF, 0x00000001, 0x00008000,      # largest denormal (-> smallest normal), negative, smallest, a denormal tie
], dtype=np.uint32)
CAST_SIZES = tuple(range(1, 18)) + (1001, 4096 * 256 * 8 + 13)
COPY_SIZES = tuple(range(1, 10)) + (4096 * 256 * 4 + 3,)


def cast_inputs(n):
    """fp32 [n]: the special values (rotated by n, so every tail length meets different ones) followed by N(0,1) * 10^U(-20,20)."""
    r = _rng(31, n)
    rest = max(0, n - len(CAST_SPECIALS))
    body = (r.standard_normal(rest) * 10.0 ** r.uniform(-20, 20, size=rest)).astype(np.float32)
    bits = np.concatenate([np.roll(CAST_SPECIALS, -3 * n), body.view(np.uint32)])[:n]
    return torch.from_numpy(bits.view(np.float32).copy())


def cast_bf16_ref(x):
    """Round-to-nearest-even to bf16 on the bit pattern -> uint16 bits (NaN: any NaN pattern; compare with `bf16_same`)."""
    b = x.numpy().view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x.numpy())
    r[nan] = 0x7FC0
    return r


def bf16_same(a_bits, b_bits):
    """Equal bit for bit, except that any NaN equals any NaN.  uint16 / int16 bit arrays."""
    a, b = np.asarray(a_bits).view(np.uint16), np.asarray(b_bits).view(np.uint16)
    na, nb = (a & 0x7FFF) > 0x7F80, (b & 0x7FFF) > 0x7F80
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]))


# =====================================================================================================================================
# Adam
# =====================================================================================================================================
ADAM_SIZES = (1, 2, 3, 4, 5, 1023, 100003)
ADAM_BIG = 16384 * 256 * 4 + 1027                 # past the grid cap: the grid-stride loop and the scalar tail both run
ADAM_STEPS = (1, 2, 1000, 100000)
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8
ADAM_FAMILIES = ("loguniform", "zero", "overflow", "normal")


def adam_family_index(n):
    """Family of element i: i % 4 (a one-element tensor is log-uniform)."""
    return torch.arange(n) % 4


def adam_inputs(n, k):
    """p0 [n] ~ N(0,1) and the k-th gradient: 10^U(-6,0) * N(0,1) | exact 0 | +-1e25 (g^2 overflows fp32) | N(0,1), by i % 4."""
    r = _rng(37, n, k)
    g = r.standard_normal(n) * 10.0 ** r.uniform(-6, 0, size=n)
    fam = np.arange(n) % 4
    g = np.where(fam == 1, 0.0, g)
    g = np.where(fam == 2, np.where((np.arange(n) // 4) % 2 == 0, 1e25, -1e25), g)
    g = np.where(fam == 3, r.standard_normal(n), g)
    return _t(g.astype(np.float32))


def adam_p0(n):
    return _t(_rng(41, n).standard_normal(n).astype(np.float32))


def adam_run_ref(p0, grads, step0, grad_scale=1.0, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
    """float64 torch.optim.Adam, single-tensor order, from m = v = 0, for steps step0, step0 + 1, ...; with the fp32 semantics of an
    overflowing g^2 (v = inf, update 0) where g^2 exceeds the fp32 range, as torch's fp32 Adam gives.
    Returns (p, m, v, tol_p, tol_m, tol_v)."""
    p, m, v = p0.double().clone(), torch.zeros(p0.numel(), dtype=torch.float64), torch.zeros(p0.numel(), dtype=torch.float64)
    mabs = torch.zeros_like(m)
    usum = torch.zeros_like(m)
    pmax = p.abs()
    fmax = float(np.finfo(np.float32).max)
    for k, g32 in enumerate(grads):
        step = step0 + k
        g = g32.double() * grad_scale
        m = m * b1 + g * (1 - b1)
        mabs = mabs * b1 + g.abs() * (1 - b1)
        g2 = g * g
        g2 = torch.where(g2 > fmax, torch.full_like(g2, float("inf")), g2)
        v = v * b2 + g2 * (1 - b2)
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        denom = v.sqrt() / math.sqrt(bc2) + eps
        p = p - (lr / bc1) * (m / denom)
        usum = usum + (k + 1) * (lr / bc1) * (mabs / denom)
        pmax = torch.maximum(pmax, p.abs())
    # m = sum of k terms b1^j (1-b1) g_j, each with a few roundings (the fp32 coefficients, the scale, the products, the sums):
    # C * U * k * sum|terms|.  v the same (positive terms).  p: U * max|p| for the subtractions, and step t's update inherits t
    # steps of m's and v's relative error plus its own root, two divisions, sum and product: C * U * sum_t t * |update_t| (with |m|
    # replaced by sum|terms|).
    k = len(grads)
    vf = torch.where(torch.isfinite(v), v, torch.zeros_like(v))
    return p, m, v, C_ADAM_P * U * (pmax + usum), C_ADAM_M * U * k * mabs, C_ADAM_V * U * k * vf


def adam_run_f32(p0, grads, step0, grad_scale=1.0, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
    """fp32 restatement of adam_kernel (scalars rounded to fp32 as dm_adam_step does)."""
    f = lambda a: torch.tensor(a, dtype=torch.float32)
    p, m, v = p0.float().clone(), torch.zeros(p0.numel()), torch.zeros(p0.numel())
    for k, g32 in enumerate(grads):
        step = step0 + k
        g = g32.float() * f(grad_scale)
        m = m * f(b1) + g * f(1.0 - b1)
        v = v * f(b2) + (g * g) * f(1.0 - b2)
        denom = v.sqrt() / f(math.sqrt(1.0 - b2 ** step)) + f(eps)
        p = p - f(lr / (1.0 - b1 ** step)) * (m / denom)
    return p, m, v


def planes_ref(x):
    """(hi, lo) bf16 planes of fp32 x: hi = bf16(x), lo = bf16(x - hi) (dm_split_bf16_planes)."""
    hi = x.bfloat16()
    return hi, (x - hi.float()).bfloat16()


# =====================================================================================================================================
# contrastive loss
# =====================================================================================================================================
CL_B = (1, 3, 4, 5, 33)
CL_D = (1, 63, 64, 65, 100, 3840)
CL_MARGIN = 1.0
CL_FAMILIES = ("pull", "push", "boundary", "equal")


def cl_inputs(B, D):
    """a, b [B, D] on the grid 2^-10 (so a - b is exact) and flag [B] (int64).  Row r is of family (r + B) % 4: random with flag 1;
    random with flag 0 (d around the margin); b + e_k with flag 0, so d == margin exactly; a == b with alternating flag."""
    r = _rng(43, B, D)
    s = 0.7 / math.sqrt(D)
    a = np.round(r.standard_normal((B, D)) * s * 1024) / 1024
    b = np.round(r.standard_normal((B, D)) * s * 1024) / 1024
    flag = np.zeros(B, np.int64)
    fam = []
    for i in range(B):
        f = CL_FAMILIES[(i + B) % 4]
        fam.append(f)
        if f == "pull":
            flag[i] = 1
        elif f == "boundary":
            a[i] = b[i]
            a[i, (7 * i) % D] += 1.0
        elif f == "equal":
            a[i] = b[i]
            flag[i] = (i // 4) % 2
    return _t(a.astype(np.float32)), _t(b.astype(np.float32)), torch.from_numpy(flag), fam


def contrastive_ref(a, b, flag, margin=CL_MARGIN, upstream=1.0):
    """float64 (loss, da, db, d, tol_loss, tol_da): Losses.py:34-38 and its gradient with relu'(0) = 0."""
    a, b, f = a.double(), b.double(), flag.double()
    B = a.shape[0]
    t = a - b
    d = (t * t).sum(1)
    hinge = margin - d
    loss = (f * d + (1 - f) * hinge.clamp(min=0)).mean()
    coef = (f - (1 - f) * (hinge > 0).double()) * 2.0 * upstream / B
    da = coef[:, None] * t
    # d is a sum of D non-negative fp32 squares (64 strided accumulators, a butterfly): relative C * U * (1 + log2 D); the hinge
    # subtracts it from the margin: absolute U * (d + margin); the row terms are summed and divided by B.
    depth = 1 + math.log2(max(2, a.shape[1]))
    tol_loss = C_CL_LOSS * U * depth * (d + margin).mean()
    tol_da = C_CL_GRAD * U * da.abs()                     # t is exact on the grid; coef = +-2 * upstream / B: two roundings; one product
    return loss, da, -da, d, tol_loss, tol_da


def contrastive_f32(a, b, flag, margin=CL_MARGIN, upstream=1.0):
    a, b, f = a.float(), b.float(), flag.float()
    B, D = a.shape
    t = a - b
    pad = (-D) % 64
    sq = torch.nn.functional.pad(t * t, (0, pad)).view(B, -1, 64)
    acc = torch.zeros(B, 64)
    for i in range(sq.shape[1]):
        acc = acc + sq[:, i]
    d = _wave_sum(acc)
    hinge = torch.tensor(margin, dtype=torch.float32) - d
    term = f * d + (1 - f) * hinge.clamp(min=0)
    acc = torch.zeros(4)
    for r in range(B):
        acc[r % 4] = acc[r % 4] + term[r]
    loss = ((acc[0] + acc[1]) + (acc[2] + acc[3])) / torch.tensor(float(B), dtype=torch.float32)
    gscale = torch.tensor(upstream, dtype=torch.float32) / torch.tensor(float(B), dtype=torch.float32)
    coef = (f - (1 - f) * (hinge > 0).float()) * 2.0 * gscale
    return loss, coef[:, None] * t, -coef[:, None] * t


# =====================================================================================================================================
# cross-entropy
# =====================================================================================================================================
CE_K = (1, 2, 63, 64, 65, 1000)
CE_B = (1, 3, 4, 5)
CE_FAMILIES = ("normal", "peak", "shift_up", "shift_down")


def ce_inputs(B, K):
    """logits [B, K] ~ N(0, 3); row r of family (r + K) % 4: as is | one entry 1e4 above the rest | all + 1e4 | all - 1e4.
    Index targets (on a peaked row: the peak for even r // 4, another class otherwise) and probability targets (softmax of N(0,1))."""
    r = _rng(47, B, K)
    x = (3.0 * r.standard_normal((B, K))).astype(np.float32)
    ti = r.integers(0, K, size=B)
    for i in range(B):
        f = CE_FAMILIES[(i + K) % 4]
        if f == "peak":
            j = int(r.integers(0, K))
            x[i, j] += np.float32(1e4)
            ti[i] = j if (i // 4) % 2 == 0 else (j + 1) % K
        elif f == "shift_up":
            x[i] += np.float32(1e4)
        elif f == "shift_down":
            x[i] -= np.float32(1e4)
    tp = torch.softmax(_t(r.standard_normal((B, K)).astype(np.float32)), 1)
    return _t(x), torch.from_numpy(ti.astype(np.int64)), tp


def cross_entropy_ref(x, target, upstream=1.0):
    """float64 (loss, dlogits, tol_loss, tol_grad), mean over rows; target int64 [B] or probabilities [B, K]."""
    x = x.double()
    B, K = x.shape
    mx = x.amax(1, keepdim=True)
    lse = mx + torch.log(torch.exp(x - mx).sum(1, keepdim=True))
    if target.dtype.is_floating_point:
        q = target.double()
    else:
        q = torch.zeros_like(x)
        q[torch.arange(B), target] = 1.0
    psum = q.sum(1, keepdim=True)
    loss = (q * (lse - x)).sum(1).mean()
    sm = torch.exp(x - lse)
    grad = (sm * psum - q) * (upstream / B)
    # lse - x: both rounded at their own magnitude -> absolute U * (|lse| + |x|) per term, a few of them, plus the sum's own
    # relative error (1 + log2 K terms deep); softmax = exp(x - lse): the argument's absolute error U * (|x| + |lse|) is the
    # relative error of the exponential, plus the exponential's own few ulp.
    depth = 1 + math.log2(max(2, K))
    tol_loss = C_CE_LOSS * U * depth * (q * (lse.abs() + x.abs() + 1)).sum(1).mean()
    tol_grad = C_CE_GRAD * U * (upstream / B) * (sm * psum * (depth + x.abs() + lse.abs()) + q)
    return loss, grad, tol_loss, tol_grad


def cross_entropy_f32(x, target, upstream=1.0):
    x = x.float()
    B, K = x.shape
    mx = x.amax(1, keepdim=True)
    pad = (-K) % 64
    e = torch.nn.functional.pad(torch.exp(x - mx), (0, pad)).view(B, -1, 64)
    acc = torch.zeros(B, 64)
    for i in range(e.shape[1]):
        acc = acc + e[:, i]
    lse = mx + torch.log(_wave_sum(acc))[:, None]
    if target.dtype.is_floating_point:
        q = target.float()
    else:
        q = torch.zeros_like(x)
        q[torch.arange(B), target] = 1.0
    psum = q.sum(1, keepdim=True)
    rows = (q * (lse - x)).sum(1)
    acc = torch.zeros(4)
    for r in range(B):
        acc[r % 4] = acc[r % 4] + rows[r]
    fb = torch.tensor(float(B), dtype=torch.float32)
    loss = ((acc[0] + acc[1]) + (acc[2] + acc[3])) / fb
    grad = (torch.exp(x - lse) * psum - q) * (torch.tensor(upstream, dtype=torch.float32) / fb)
    return loss, grad


# =====================================================================================================================================
# GRU cell
# =====================================================================================================================================
GRU_SHAPES = ((1, 1), (3, 80), (37, 80), (5, 257))
GRU_T = 3                      # time steps of the strided variant: gi = gi_all[:, 1] of [B, T, 3H]


def gru_inputs(B, H):
    """gi_all [B, T, 3H], gh [B, 3H], h [B, H], upstream dh [B, H].  Row b of family b % 4 (a one-row case: family 0):
    N(0,1) | pre-activations +-30 | +-100 | N(0,1) with gh_n = +-100 (signs vary per element)."""
    r = _rng(53, B, H)
    gi_all = r.standard_normal((B, GRU_T, 3 * H)).astype(np.float32)
    gh = r.standard_normal((B, 3 * H)).astype(np.float32)
    for b in range(B):
        f = b % 4
        if f in (1, 2):
            mag = np.float32(30.0 if f == 1 else 100.0)
            gi_all[b] = mag * np.sign(gi_all[b])
            gh[b] = mag * np.sign(gh[b])
        elif f == 3:
            gh[b, 2 * H:] = np.float32(100.0) * np.sign(gh[b, 2 * H:])
    h = r.standard_normal((B, H)).astype(np.float32)
    dh = r.standard_normal((B, H)).astype(np.float32)
    return _t(gi_all), _t(gh), _t(h), _t(dh)


def gru_cell_ref(gi, gh, h):
    """float64 h' from the projections; differentiable (autograd gives the backward truth)."""
    H = h.shape[1]
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1 - z) * n + z * h


def gru_truth(gi, gh, h, dh):
    """(h', dgi, dgh, dh_in, tol_fwd, tol_bwd [B, H]) in float64."""
    gi, gh, h = gi.double().requires_grad_(True), gh.double().requires_grad_(True), h.double().requires_grad_(True)
    out = gru_cell_ref(gi, gh, h)
    (out * dh.double()).sum().backward()
    H = h.shape[1]
    with torch.no_grad():
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        ghn, gin = gh[:, 2 * H:], gi[:, 2 * H:]
        n = torch.tanh(gin + r * ghn)
        # sigmoid through a fast exponential: exp's relative error |x| * U gives an absolute error of at most a few U in the gate;
        # n = tanh(gi_n + r * gh_n): the argument is off by U * (|gi_n| + |r gh_n|) + |gh_n| * (error of r), damped by tanh' = 1 - n^2.
        amp = 1 + (1 - n * n) * (gin.abs() + (r * ghn).abs() + ghn.abs())
        tol_fwd = max(C_GRU_FWD, 4) * U * (amp + h.abs())
        # every backward product has the factors g = dh, (h - n) or 1, gates in [0, 1] with absolute error of the forward's size,
        # and for the r gate and dgh_n one factor gh_n resp. r.
        tol_bwd = C_GRU_BWD * U * dh.double().abs() * (1 + h.abs()) * (1 + ghn.abs()) * amp
    return out.detach(), gi.grad, gh.grad, h.grad, tol_fwd, tol_bwd


def _fast_exp(x):
    """exp as a base-2 hardware exponential of the fp32-rounded x * log2(e), the shape of a fast-math expf."""
    return torch.exp2(x * torch.tensor(1.4426950408889634, dtype=torch.float32))


def gru_cell_f32(gi, gh, h, dh):
    """fp32 restatement of gru_cell_{fwd,bwd}_kernel -> (h', dgi, dgh, dh_in)."""
    gi, gh, h, g = gi.float(), gh.float(), h.float(), dh.float()
    H = h.shape[1]
    sig = lambda x: 1.0 / (1.0 + _fast_exp(-x))
    r = sig(gi[:, :H] + gh[:, :H])
    z = sig(gi[:, H:2 * H] + gh[:, H:2 * H])
    ghn = gh[:, 2 * H:]
    n = torch.tanh(gi[:, 2 * H:] + r * ghn)
    out = (1 - z) * n + z * h
    dn = g * (1 - z) * (1 - n * n)
    dz = g * (h - n) * z * (1 - z)
    dr = dn * ghn * r * (1 - r)
    return out, torch.cat([dr, dz, dn], 1), torch.cat([dr, dz, dn * r], 1), g * z
