"""CPU references, input generators and error bounds for batch norm (csrc/dm_batchnorm.hip), the relative-position bias gather /
reduce (csrc/dm_rows.hip: relpos_gather_kernel, chunk_sum_kernel, relpos_reduce_kernel) and patchify (patchify_kernel,
patchify_any_kernel).  No GPU here: tests/test_bn_relpos_host.py checks this file against torch's own float64 operators and fixes the
tolerance constants; tests/test_gpu_bn_relpos.py compares the kernels with it.  Both see the same inputs through the generators below.
The layout follows tests/rows_ref.py (whose rounding unit, `worst` and bf16 helpers are reused):

  * a float64 restatement written from the definition (`*_ref` / `*_truth`), the truth of the GPU tests;
  * where a tolerance is needed, a float32 restatement of the kernel's arithmetic order (`*_f32`; not lane-exact), whose only use
    is to show on the CPU that honest arithmetic of the kernel's kind stays inside the tolerance on the chosen inputs -- and that
    arithmetic of the wrong kind (`mutate=`) does not;
  * a bound `*_tol` = C_* x U x (a sum of magnitudes), U = 2^-24, derived from the fp32 rounding model.  Every bound is
    proportional to its constant, and each constant is the smallest integer for which the float32 restatement stays at or below
    HALF the bound on the GPU tests' inputs (test_bn_relpos_host.py asserts both halves of that), so a correct kernel has a factor
    2 of headroom.

What each restatement mirrors:
  batch norm   nn.BatchNorm2d -> ReLU -> Dropout2d of the auxiliary heads (nets/ShfitScaleFormer.py:340-346 in the reference) on the
               channels-last matrix x [M = samples * rows_per_sample, C]: per column c, y = relu((x - E[x]) / sqrt(Var[x] + eps) *
               gamma + beta) * mask[row / rows_per_sample, c], biased variance; running statistics updated with the unbiased one
               (Ioffe & Szegedy 2015); the analytic backward.
  gather       relative_position_bias_table[relative_position_index] of the window attention (Liu et al. 2021, Swin):
               bias[h, i, j] = table[index[i, j], h], bias_t[h, i, j] = table[index[j, i], h].
  reduce       its adjoint: dtable[b, h] = sum over chunks and over the (i, j) with index[i, j] == b of slab[chunk, h, i, j].
  patchify     im2col of non-overlapping p x p patches = torch.nn.functional.unfold(x, p, stride=p), columns in (c, dy, dx) order.
"""
import functools

import numpy as np
import torch

import rows_ref as RR

U = RR.U                       # fp32 unit roundoff, 2^-24
D53 = 2.0 ** -29               # the float64 unit roundoff 2^-53 in units of U
worst = RR.worst

# ---- tolerance constants (fixed by tests/test_bn_relpos_host.py; the table is at the top of tests/test_gpu_bn_relpos.py) -------------
C_BN_MEAN = 2                  # a single rounding reaches U by itself: 2 keeps the factor 2
C_BN_RSTD = 2                  # the same
C_BN_RSTD_EVAL = 4
C_BN_RUN = 3
C_BN_Y = 7
C_BN_DX = 4
C_BN_DGB = 3
C_RP_SUM = 1


def _rng(*key):
    return np.random.default_rng([int(k) & 0xFFFFFFFF for k in key])


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# =====================================================================================================================================
# batch norm
# =====================================================================================================================================
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
BN_MU = 1.0e3                  # mean of the "offset" columns (unit spread)
BN_OUTLIER = 1.0e2             # the one outlier row of the "outlier" columns
BN_KEEP = 0.7                  # Dropout2d(p = 0.3): the mask holds 0 or 1 / 0.7
BN_BAND = 2.0 ** -6            # no pre-activation changes sign within this distance (in units of x) of any x: see bn_inputs
BN_CONST = (-3.0, 0.1, 2.0, -0.7)
BN_FAMILIES = ("normal", "offset", "const", "outlier")      # of column c: c % 4
# (samples, rows_per_sample, C); M = samples * rows_per_sample.  The smallest shapes that reach each branch of dm_batchnorm.hip:
BN_SHAPES = (
    (2, 1, 4),                 # minimum training size: row groups 2, 3 empty, one float4 per row, M / (M - 1) = 2
    (4, 64, 64),               # M = 256: one slice
    (257, 1, 68),              # M = 257: two slices (129 + 128 rows); the second column block has 4 live columns
    (3, 257, 60),              # M = 771: four slices, a partly live column block, the mask row changes inside a slice
    (64, 256, 8),              # M = 16384: exactly 64 slices
    (145, 113, 260),           # M = 16385: the slice cap (257 rows per slice, the last 194); finalize kernels run a second block;
                               # M * C / 4 = 1,065,025 float4s > 4096 * 256: the grid-stride loops of both apply kernels run
    (6, 49, 768),              # the workload's own shape
)


def bn_slicing(M):
    """(slices, rows_per_slice) of bn_partial_kernel's grid: ceil(M / 256) slices, at most 64."""
    slices = min(max((M + 255) // 256, 1), 64)
    return slices, (M + slices - 1) // slices


def bn_depth(M):
    """Longest chain of float64 additions behind one column statistic: a thread's rows, the 4 row groups, the slices."""
    slices, rps = bn_slicing(M)
    return (rps + 3) // 4 + 4 + slices


def _bn_crossings(x, gamma, beta, rm, rv):
    """The two x at which a column's pre-activation changes sign: with batch statistics and with the running ones."""
    eps = float(np.float32(BN_EPS))
    mu = x.mean(0)
    var = ((x - mu) ** 2).mean(0)
    return mu - beta * np.sqrt(var + eps) / gamma, rm - beta * np.sqrt(rv + eps) / gamma


@functools.lru_cache(maxsize=2)
def bn_inputs(samples, rps, C):
    """fp32 x [M, C] with one family per column (c % 4): N(0,1) | +-1e3 + N(0,1) | a constant of BN_CONST | N(0,1) with one row at
    +-1e2.  gamma ~ +-(1 + 0.2 N(0,1)), |gamma| >= 0.5, every third group of four negative; beta ~ 0.2 N(0,1); running mean within
    0.1 of the column's centre, running variance U(0.5, 1.5); mask [samples, C] of 0 and fp32(1 / 0.7) with (0, 0) and the last
    (sample, channel) dropped and (0, 1) kept; a contiguous upstream gradient dy ~ N(0,1); g0 [2, C] for the accumulating call.

    The ReLU gate of the backward is decided by the sign of the pre-activation z.  An element whose z is within rounding of 0
    could be gated either way, and no bound on dx / dgamma / dbeta can cover a flipped gate, so the generator moves every x that
    lies within BN_BAND of a sign change -- with the batch statistics or with the running ones -- to 2 * BN_BAND from it (the
    ambiguity of an fp32 evaluation is U * 1e3 = 6e-5 at most here).  Constant columns are left alone: there x - mean is exactly 0
    in the kernel's arithmetic, so z = beta in both.  test_bn_relpos_host.py asserts the band on the result."""
    M = samples * rps
    r = _rng(71, samples, rps, C)
    cols = np.arange(C)
    fam = cols % 4
    x = r.standard_normal((M, C), dtype=np.float32)
    x[:, fam == 1] += np.where((cols // 4) % 2 == 0, BN_MU, -BN_MU).astype(np.float32)[fam == 1]
    centre = np.where(fam == 1, np.where((cols // 4) % 2 == 0, BN_MU, -BN_MU), 0.0)
    for c in cols[fam == 2]:
        x[:, c] = np.float32(BN_CONST[(c // 4) % len(BN_CONST)])
        centre[c] = float(x[0, c])
    for c in cols[fam == 3]:
        x[(7 * c) % M, c] = np.float32(BN_OUTLIER if (c // 4) % 2 == 0 else -BN_OUTLIER)
    gamma = 1 + 0.2 * r.standard_normal(C)
    gamma = np.sign(gamma) * np.maximum(np.abs(gamma), 0.5) * np.where((cols // 4) % 3 == 2, -1.0, 1.0)
    gamma = gamma.astype(np.float32)
    beta = (0.2 * r.standard_normal(C)).astype(np.float32)
    rm = (centre + 0.1 * r.standard_normal(C)).astype(np.float32)
    rv = r.uniform(0.5, 1.5, C).astype(np.float32)
    mask = np.where(r.uniform(size=(samples, C)) > 1 - BN_KEEP, np.float32(1.0) / np.float32(BN_KEEP), np.float32(0)).astype(np.float32)
    mask[0, 0] = mask[samples - 1, C - 1] = 0
    mask[0, 1] = np.float32(1.0) / np.float32(BN_KEEP)
    dy = r.standard_normal((M, C), dtype=np.float32)
    g0 = r.standard_normal((2, C), dtype=np.float32)
    live = fam != 2
    ga, be = gamma.astype(np.float64), beta.astype(np.float64)
    for _ in range(8):
        xd = x.astype(np.float64)
        ct, ce = _bn_crossings(xd, ga, be, rm.astype(np.float64), rv.astype(np.float64))
        lo, hi = np.minimum(ct, ce), np.maximum(ct, ce)
        one = hi - lo < 4 * BN_BAND                      # the two sign changes of a column too close to stand between them: one zone
        zlo, zhi = np.where(one, lo, ct), np.where(one, hi, ct)
        moved = False
        for a, b, cols_ in ((zlo, zhi, live), (ce, ce, live & ~one)):
            near = (xd > a - BN_BAND) & (xd < b + BN_BAND) & cols_
            if near.any():
                x = np.where(near, np.where(xd >= (a + b) / 2, b + 2 * BN_BAND, a - 2 * BN_BAND).astype(np.float32), x)
                xd = x.astype(np.float64)
                moved = True
        if not moved:
            break
    return dict(x=_t(x), gamma=_t(gamma), beta=_t(beta), rm=_t(rm), rv=_t(rv), mask=_t(mask), dy=_t(dy), g0=_t(g0),
                const_cols=torch.from_numpy(fam == 2), offset_cols=torch.from_numpy(fam == 1))


def bn_gate_distance(d):
    """Smallest |x - sign change| over the non-constant columns, and smallest |z| of the constant columns in eval mode (in training
    their z is beta exactly, whatever the arithmetic)."""
    x = d["x"].double().numpy()
    ga, be, rm, rv = (d[k].double().numpy() for k in ("gamma", "beta", "rm", "rv"))
    live = ~d["const_cols"].numpy()
    ct, ce = _bn_crossings(x, ga, be, rm, rv)
    dist = min(float(np.abs(x - ct)[:, live].min()), float(np.abs(x - ce)[:, live].min()))
    zc = ((x - rm) / np.sqrt(rv + float(np.float32(BN_EPS))) * ga + be)[:, ~live]
    return dist, float(np.abs(zc).min()) if zc.size else float("inf")


def _mask_rows(mask, rps):
    return mask.repeat_interleave(rps, 0)


@functools.lru_cache(maxsize=1)
def bn_truth(samples, rps, C, training=True, relu=True, masked=True):
    """float64 truth of one generated case from the definitions, forward and analytic backward.  `mrow` is the mask per row (ones
    without a mask), `g` the gradient behind the mask and the ReLU, A = |mean| * rstd where the mean is computed (training), else 0."""
    d = bn_inputs(samples, rps, C)
    x, gamma, beta, dy = d["x"].double(), d["gamma"].double(), d["beta"].double(), d["dy"].double()
    M = x.shape[0]
    eps = float(np.float32(BN_EPS))
    bmean = x.mean(0)
    bvar = ((x - bmean) ** 2).mean(0)
    mean, var = (bmean, bvar) if training else (d["rm"].double(), d["rv"].double())
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    z = xhat * gamma + beta
    mrow = _mask_rows(d["mask"].double(), rps) if masked else torch.ones_like(x)
    y = (z.clamp(min=0) if relu else z) * mrow
    g = dy * mrow * ((z > 0).double() if relu else 1.0)
    mg, mgx = g.mean(0), (g * xhat).mean(0)
    dx = gamma * rstd * (g - mg - xhat * mgx) if training else gamma * rstd * g
    unbiased = bvar * M / (M - 1) if M > 1 else bvar
    return dict(mean=mean, var=var, rstd=rstd, xhat=xhat, z=z, mrow=mrow, y=y, g=g, mg=mg, mgx=mgx, dx=dx,
                dgamma=(g * xhat).sum(0), dbeta=g.sum(0), unbiased=unbiased,
                run_mean=(1 - BN_MOMENTUM) * d["rm"].double() + BN_MOMENTUM * bmean,
                run_var=(1 - BN_MOMENTUM) * d["rv"].double() + BN_MOMENTUM * unbiased,
                A=mean.abs() * rstd if training else torch.zeros_like(mean), M=M, training=training)


BN_MUTATIONS = ("fp32_one_pass", "biased_running_var", "drop_last_slice", "mask_by_row")


def _bn_column_sums(a, b, M, fp32=False, drop_last=False):
    """(sum a, sum a * b) over the rows as bn_partial_kernel forms them: per slice, four strided row groups, folded in order;
    slices folded in order; in float64 (fp32=True: DELIBERATELY WRONG, every accumulator in fp32)."""
    slices, rpsl = bn_slicing(M)
    acc = torch.float32 if fp32 else torch.float64
    s, q = torch.zeros(a.shape[1], dtype=acc), torch.zeros(a.shape[1], dtype=acc)
    for k in range(slices):
        if drop_last and slices > 1 and k == slices - 1:
            continue
        sa, sb = torch.zeros_like(s), torch.zeros_like(q)
        for grp in range(4):
            u, v = a[k * rpsl + grp:min(M, (k + 1) * rpsl):4].to(acc), b[k * rpsl + grp:min(M, (k + 1) * rpsl):4].to(acc)
            sa, sb = sa + u.sum(0), sb + (u * v).sum(0)
        s, q = s + sa, q + sb
    return s, q


def bn_fwd_f32(d, rps, training=True, relu=True, masked=True, mutate=None):
    """Restatement of dm_batchnorm_fwd's arithmetic: one-pass column sums of x and x^2 in float64, mean and 1 / sqrt(var + eps)
    rounded to fp32 once, the running statistics formed in float64 with the fp32 momentum and rounded once; eval: the running
    mean, 1 / sqrtf(rv + eps) in fp32; the apply pass in fp32.  -> (y, save_mean, save_rstd, running_mean, running_var)."""
    x, gamma, beta = d["x"], d["gamma"], d["beta"]
    M = x.shape[0]
    eps32 = torch.tensor(BN_EPS, dtype=torch.float32)
    rm, rv = d["rm"].clone(), d["rv"].clone()
    if training:
        s, q = _bn_column_sums(x, x, M, fp32=mutate == "fp32_one_pass", drop_last=mutate == "drop_last_slice")
        mu = s / M
        var = (q / M - mu * mu).clamp(min=0)
        mean32, rstd32 = mu.float(), (1.0 / torch.sqrt(var.double() + eps32.double())).float()
        mom = float(np.float32(BN_MOMENTUM))
        unbiased = var.double() if (mutate == "biased_running_var" or M == 1) else var.double() * (M / (M - 1))
        rm = ((1.0 - mom) * rm.double() + mom * mu.double()).float()
        rv = ((1.0 - mom) * rv.double() + mom * unbiased).float()
    else:
        mean32, rstd32 = rm.clone(), 1.0 / torch.sqrt(rv + eps32)
    o = (x - mean32) * rstd32 * gamma + beta
    if relu:
        o = o.clamp(min=0)
    if masked:
        o = o * (d["mask"][torch.arange(M) % d["mask"].shape[0]] if mutate == "mask_by_row" else _mask_rows(d["mask"], rps))
    return o, mean32, rstd32, rm, rv


def bn_bwd_f32(d, rps, y, mean32, rstd32, training=True, relu=True, masked=True, g0=None):
    """Restatement of dm_batchnorm_bwd: g = dy gated by y > 0, times the mask, in fp32; column sums of g and g * xhat (xhat in fp32)
    in float64, rounded once (and added to g0 = (dgamma0, dbeta0) in fp32 when accumulating); the two column means rounded to fp32;
    dx in fp32.  -> (dx, dgamma, dbeta)."""
    x, gamma, dy = d["x"], d["gamma"], d["dy"]
    M = x.shape[0]
    g = torch.where(y > 0, dy, torch.zeros(())) if relu else dy
    if masked:
        g = g * _mask_rows(d["mask"], rps)
    xh = (x - mean32) * rstd32
    s, q = _bn_column_sums(g, xh, M)
    dbeta, dgamma = s.float(), q.float()
    if g0 is not None:
        dgamma, dbeta = g0[0] + dgamma, g0[1] + dbeta
    o = g - (s / M).float() - xh * (q / M).float() if training else g
    return o * gamma * rstd32, dgamma, dbeta


def bn_mean_tol(d, t):
    """save_mean = fp32(float64 mean): one rounding, U * |mean|, plus the float64 sum's own error: 2^-53 * depth * max|x|."""
    return C_BN_MEAN * U * (t["mean"].abs() + bn_depth(t["M"]) * D53 * d["x"].double().abs().amax(0))


def _bn_var_err(t):
    """Error of the float64 one-pass variance E[x^2] - mean^2 in units of U: 2^-53 * depth * (mean^2 + var)."""
    return bn_depth(t["M"]) * D53 * (t["mean"] ** 2 + t["var"])


def bn_rstd_tol(t):
    """save_rstd = fp32(1 / sqrt(var + eps)) from the float64 one-pass variance: one rounding, plus half the variance's relative
    error against var + eps (= rstd^2 / 2 times its absolute error)."""
    return C_BN_RSTD * U * t["rstd"] * (1 + 0.5 * _bn_var_err(t) * t["rstd"] ** 2)


def bn_rstd_eval_tol(t):
    """Eval: 1 / sqrtf(rv + eps) in fp32: the sum (half of its U under the root), the root, the division."""
    return C_BN_RSTD_EVAL * U * t["rstd"]


def bn_run_tol(d, t):
    """(1 - m) * r + m * s in float64, rounded once: U * |result|; m is passed as fp32, which moves both coefficients by U * m:
    together at most U * ((1 - m) |r| + m |s|) times a small constant.  The variance adds its float64 one-pass error."""
    m = BN_MOMENTUM
    tm = C_BN_RUN * U * ((1 - m) * d["rm"].double().abs() + m * t["mean"].abs())
    tv = C_BN_RUN * U * ((1 - m) * d["rv"].double().abs() + m * (t["unbiased"] + 2 * _bn_var_err(t)))
    return tm, tv


def bn_y_tol(d, t):
    """y = relu((x - mean) * rstd * gamma + beta) * mask in fp32.  The stored mean is off by U * |mean| (it is kept in fp32: inherent
    in the design), which moves every xhat by U * |mean| * rstd = U * A; the subtraction, the fp32 rstd and the two products are
    each relative U of |xhat * gamma|; the addition and the mask product relative U of the result:
    C * U * mask * (|gamma| * (A + |xhat|) + |z|).  Where the mask is 0 the bound is 0: y must be exactly 0."""
    return C_BN_Y * U * t["mrow"] * (d["gamma"].double().abs() * (t["A"] + t["xhat"].abs()) + t["z"].abs())


def _bn_xhat_err(t):
    return t["A"] + t["xhat"].abs()


def bn_dx_tol(d, t):
    """dx = gamma * rstd * (g - mean(g) - xhat * mean(g * xhat)).  g = dy * mask carries U * |g| where the mask is not 1; the fp32
    xhat is off by U * (A + |xhat|) (the mean's error and its own roundings); mean(g) is rounded once and inherits
    E0 = mean_r |g| [mask != 1] from its terms (it is small against them where they cancel); mean(g * xhat) is rounded once and
    inherits E = mean_r |g| (A + |xhat|); the difference and the two products are relative U of their operands and results:
    C * U * (|gamma| rstd (|g| + |mean g| + E0 + (A + |xhat|) |mean gx| + |xhat| (|mean gx| + E)) + |dx|).
    Eval: dx = gamma * rstd * g."""
    scale = d["gamma"].double().abs() * t["rstd"]
    if not t["training"]:
        return C_BN_DX * U * (scale * t["g"].abs() + t["dx"].abs())
    E = (t["g"].abs() * _bn_xhat_err(t)).mean(0)
    E0 = (t["g"].abs() * (t["mrow"] != 1)).mean(0)
    inner = t["g"].abs() + t["mg"].abs() + E0 + _bn_xhat_err(t) * t["mgx"].abs() + t["xhat"].abs() * (t["mgx"].abs() + E)
    return C_BN_DX * U * (scale * inner + t["dx"].abs())


def bn_dgb_tol(t, g0=None):
    """dgamma = fp32(sum_r g * xhat), dbeta = fp32(sum_r g), summed in float64: one rounding of the result plus the fp32 error of
    each term: U * |g| where the mask is not 1 (the mask product) resp. U * |g| (A + |xhat|).  An accumulating call rounds
    g0 + result once more."""
    tg = C_BN_DGB * U * (t["dgamma"].abs() + (t["g"].abs() * _bn_xhat_err(t)).sum(0))
    tb = C_BN_DGB * U * (t["dbeta"].abs() + (t["g"].abs() * (t["mrow"] != 1)).sum(0))
    if g0 is not None:
        tg = tg + C_BN_DGB * U * (t["dgamma"] + g0[0].double()).abs()
        tb = tb + C_BN_DGB * U * (t["dbeta"] + g0[1].double()).abs()
    return tg, tb


def bn_const_rstd():
    """rstd of a zero-variance column and its 2 ulp."""
    want = 1.0 / np.sqrt(np.float64(np.float32(BN_EPS)))
    return want, 2 * float(np.spacing(np.float32(want)))


# =====================================================================================================================================
# relative-position bias: gather (exact) and reduce
# =====================================================================================================================================
RP_GATHER_N = (1, 15, 16, 64, 256)
RP_GATHER_H = (1, 3, 12)
RP_GATHER_BIG = (1025, 3)      # N^2 = 1,050,625 > 4096 * 256: the grid-stride loop runs
RP_PLANTED = (0, 1, 63, 64, 65)
RP_BIG_BIN = 4100              # one bin with more than 4096 entries where N^2 allows it
# (N, H, chunks).  H * N * N % 4 == 0 and chunks > 1: chunk_sum_kernel folds the chunks first; otherwise the in-kernel chunk loop.
RP_REDUCE_CASES = (tuple((72, h, 1) for h in (1, 3, 4, 5, 12))
                   + tuple((16, 4, c) for c in (1, 2, 5)) + tuple((15, 3, c) for c in (1, 2, 5))
                   + ((72, 4, 2), (73, 3, 2)))


def rp_bins(N):
    return 1 if N == 1 else (40 if N * N < 1024 else min(4099, N * N // 8))


def rp_table(n_bins, H):
    """fp32 [n_bins, H] with a distinct value per (bin, head): bin * H + head + 0.5 (exact in fp32)."""
    return (torch.arange(n_bins * H, dtype=torch.float32) + 0.5).reshape(n_bins, H)


@functools.lru_cache(maxsize=4)
def rp_index(N, n_bins):
    """A seeded random int32 index [N, N] that is NOT symmetric, whose bin counts include RP_PLANTED (bins 0 .. 4) and, where
    N^2 >= 2 * RP_BIG_BIN, one bin (5) of RP_BIG_BIN entries; the rest is spread at random over the remaining bins."""
    r = _rng(83, N, n_bins)
    NN = N * N
    counts = [c for c in RP_PLANTED] + ([RP_BIG_BIN] if NN >= RP_BIG_BIN + sum(RP_PLANTED) + 1 else [])
    if n_bins <= len(counts) or NN < sum(counts):
        flat = r.integers(0, n_bins, NN)
    else:
        rest = r.integers(len(counts), n_bins, NN - sum(counts))
        flat = np.concatenate([np.repeat(np.arange(len(counts)), counts), rest])
        r.shuffle(flat)
    idx = flat.reshape(N, N).astype(np.int32)
    if N > 2:
        assert not np.array_equal(idx, idx.T)
    return torch.from_numpy(idx)


def rp_gather_ref(table, index):
    """(bias, bias_t) [H, N, N] from the definition; out-of-range entries clamped into [0, n_bins) as the kernel does."""
    t, i = table.numpy(), np.clip(index.numpy(), 0, table.shape[0] - 1)
    bias = np.ascontiguousarray(np.transpose(t[i], (2, 0, 1)))
    return torch.from_numpy(bias), torch.from_numpy(np.ascontiguousarray(np.transpose(t[i.T], (2, 0, 1))))


def rp_csr_ref(index, n_bins):
    """(positions, offsets) of ops.relpos_index_csr restated in numpy: the flat positions of each bin ascending, bins in order,
    entries outside [0, n_bins) dropped."""
    flat = index.numpy().reshape(-1)
    pos = [np.nonzero(flat == b)[0] for b in range(n_bins)]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pos])])
    return np.concatenate(pos).astype(np.int32) if pos else np.zeros(0, np.int32), off.astype(np.int32)


def rp_reduce_ref(slab, index, n_bins):
    """float64 dtable [n_bins, H] = np.add.at over the slab [chunks, H, N, N]; entries outside [0, n_bins) dropped.
    Also the sum of magnitudes behind each entry (for the bound)."""
    s = slab.double().numpy()
    chunks, H = s.shape[:2]
    flat = index.numpy().reshape(-1).astype(np.int64)
    ok = (flat >= 0) & (flat < n_bins)
    out, mag = np.zeros((n_bins, H)), np.zeros((n_bins, H))
    v = s.reshape(chunks, H, -1)[:, :, ok]
    for c in range(chunks):
        np.add.at(out, flat[ok], v[c].T)
        np.add.at(mag, flat[ok], np.abs(v[c]).T)
    return torch.from_numpy(out), torch.from_numpy(mag)


def rp_slab(chunks, H, N, integer):
    """Slab [chunks, H, N, N]: small integers (every sum of them is exact in fp32, whatever the order) or N(0,1) * 10^U(-2,1)."""
    r = _rng(89, chunks, H, N, int(integer))
    if integer:
        return _t(r.integers(-3, 4, (chunks, H, N, N)).astype(np.float32))
    return _t((r.standard_normal((chunks, H, N, N)) * 10.0 ** r.uniform(-2, 1, (chunks, H, N, N))).astype(np.float32))


def rp_dtable0(n_bins, H):
    return _t(_rng(97, n_bins, H).standard_normal((n_bins, H)).astype(np.float32))


def rp_chunk_sum_path(chunks, H, N, aligned=True):
    """Does dm_relpos_bias_reduce fold the chunks with chunk_sum_kernel first?"""
    return chunks > 1 and (H * N * N) % 4 == 0 and aligned


def rp_reduce_f32(slab, index, n_bins, chunk_sum, d0=None):
    """fp32 restatement of dm_relpos_bias_reduce: (chunk_sum: the chunks of each position summed in order first;) lane l of a wave
    takes the bin's items l, l + 64, ... serially (chunk by chunk in the in-kernel loop), then the 64-lane butterfly."""
    chunks, H = slab.shape[:2]
    pos, off = rp_csr_ref(index, n_bins)
    s = slab.float().reshape(chunks, H, -1)
    if chunk_sum:
        f = s[0].clone()
        for c in range(1, chunks):
            f = f + s[c]
        s = f[None]
    out = torch.zeros(n_bins, H) if d0 is None else d0.clone()
    for b in range(n_bins):
        p = torch.from_numpy(pos[off[b]:off[b + 1]].astype(np.int64))
        items = s[:, :, p]                                             # [chunks', H, cnt]
        I = (len(p) + 63) // 64
        items = torch.nn.functional.pad(items, (0, I * 64 - len(p))).reshape(s.shape[0], H, I, 64)
        acc = torch.zeros(H, 64)
        for c in range(s.shape[0]):
            for i in range(I):
                acc = acc + items[c, :, i]
        tot = RR._wave_sum(acc)
        out[b] = tot if d0 is None else d0[b] + tot
    return out


def rp_reduce_tol(index, n_bins, chunks, mag, result=None):
    """A lane adds ceil(cnt / 64) * chunks items serially (either path: chunk_sum_kernel only reorders them), the butterfly adds 6
    more steps: (ceil(cnt / 64) * chunks + 6) * U * sum|terms|; an accumulating call rounds dtable + sum once more: U * |result|,
    doubled for the factor 2 (a one-entry bin has no other error), as rows_ref.colsum_tol does."""
    _, off = rp_csr_ref(index, n_bins)
    cnt = torch.from_numpy(np.diff(off).astype(np.float64))
    depth = torch.ceil(cnt / 64) * chunks + 6
    tol = C_RP_SUM * U * depth[:, None] * mag
    return tol if result is None else tol + 2 * U * result.abs()


# =====================================================================================================================================
# patchify
# =====================================================================================================================================
# (B, C, side, p): B = 1, C = 1, p = side (one patch per image), p = 4 (one float4 per patch row), p = 1; both kernels
PATCHIFY_SHAPES = ((1, 1, 4, 4), (1, 1, 8, 4), (2, 3, 8, 8), (3, 2, 12, 4), (2, 4, 64, 16),        # p % 4 == 0: patchify_kernel
                   (1, 1, 3, 1), (2, 3, 5, 1), (1, 1, 6, 6), (2, 3, 6, 2), (3, 3, 56, 14), (1, 2, 9, 3))   # patchify_any_kernel
PATCHIFY_BIG = ((5, 4, 512, 16), (5, 4, 504, 14))      # 5.2 M / 5.1 M elements: 1.3 M float4 items > 4096 * 256 in patchify_kernel


def patchify_input(B, C, side):
    """fp32 [B, C, side, side]: rows_ref.cast_inputs -- the special values (+-0, +-inf, NaNs, denormals, exact bf16 ties of both
    parities, the overflow tie; rotated by the size, cut off in images of fewer than 23 elements) followed by
    N(0,1) * 10^U(-20,20), so a misplaced element shows."""
    return RR.cast_inputs(B * C * side * side).reshape(B, C, side, side).clone()


def patchify_ref(x, p):
    """[B, C, S, S] -> [B * (S/p)^2, C * p * p] from the definition: row (b, py, px), column (c, dy, dx).  A pure rearrangement."""
    B, C, S, _ = x.shape
    g = S // p
    return x.reshape(B, C, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, C * p * p).contiguous()
