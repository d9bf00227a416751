// Dense pairwise Euclidean distance (gfx950): D[i,j] = sqrt(max(0, (x2[i] + y2[j]) - 2 xy[i,j])) for row-major X [n,p],
// Y [m,p] -> D [n,m], the reference's Euclidean_distance / MC_Lyu_2020 (ExtractFeatures.py:119-147, :228-237; Train_SMT.py:115-131)
// in one launch per call.
//
// Arithmetic contract (one per dtype, independent of the shape and of the tile an entry falls in):
//   xy[i,j] = fma chain over k = 0, 1, ..., p-1 from +0 of x[i,k] * y[j,k]
//   x2[i]   = the same chain of x[i,k] * x[i,k];  y2[j] likewise
// so a row of X that equals a row of Y bit for bit gives x2 == y2 == xy and an EXACT zero distance (the reference shows up to
// 5e-3 of cancellation noise there).  fp32: xy on v_mfma_f32_16x16x4_f32, whose result is bit for bit the k-ordered fmaf chain;
// each lane group of the MFMA feeds one k of a 4-k step in natural order (A[r][k] / B[k][c] from lane r + 16k), and K is zero
// padded to the next multiple of 4 (fma(0, 0, acc) == acc, and acc is never -0).  The norms are the same chain in fmaf on the
// VALU, from the staged LDS panels.  fp64: everything on VALU fma(double) chains in the same order.
// Epilogue: (x2 + y2) - 2 xy in the reference's order (no contraction: the file is built with -ffp-contract=off), d < 0 -> 0
// (NaN stays NaN), correctly rounded sqrt.  Stores: plain C++, restaged through LDS into whole row segments (16-byte vectors
// when m % 4 == 0 and D is 16-byte aligned).
#include "dm_common.h"

#pragma clang fp contract(off)

namespace {

// ---- fp32: 128x128 tile of D per 256-thread workgroup, 4 waves as 2x2, 64x64 per wave = 4x4 MFMA tiles of 16x16 ----------------
constexpr int F_TILE = 128;
constexpr int F_KS = 16;          // k per LDS stage
constexpr int F_PITCH = 20;       // floats per staged row: rows 0..15 at 20 r mod 64 are distinct multiples of 4 -> the
                                  // fragment reads (16 rows x 4 consecutive k per MFMA step) hit 64 distinct banks
constexpr int EP_PITCH = 68;      // floats per row of a wave's 16 x 64 epilogue block (4 waves x 16 x 68 <= one panel buffer)
static_assert(4 * 16 * EP_PITCH <= 2 * 2 * F_TILE * F_PITCH, "epilogue blocks must fit in the panel buffers");

// Stage rows [row0, row0 + 128) x k [k0, k0 + 16) of A [rows, p] into registers (zeros past the matrix).  Element e = t + 256 q:
// row e / 16, k e % 16 (16 consecutive threads read 64 contiguous bytes of one row).
__device__ __forceinline__ void f32_load(float (&r)[8], const float *__restrict__ A, int rows, int p, int row0, int k0) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = threadIdx.x + 256 * q;
    const int row = row0 + (e >> 4), k = k0 + (e & 15);
    r[q] = (row < rows && k < p) ? A[(long long)row * p + k] : 0.f;
  }
}
__device__ __forceinline__ void f32_store_lds(float *s, const float (&r)[8]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = threadIdx.x + 256 * q;
    s[(e >> 4) * F_PITCH + (e & 15)] = r[q];
  }
}

// One 4-k step of the wave's 64x64 block: lane group g feeds k = 4 q + g.  A = the Y fragment, B = the X fragment, so the
// lane ends with D[x row r16][4 consecutive y rows 4g..4g+3] of each 16x16 tile.
__device__ __forceinline__ void f32_kstep(f32x4 (&acc)[4][4], const float *xb, const float *yb, int wm, int wn, int r16, int k) {
  float fx[4], fy[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) fx[a] = xb[(wm * 64 + a * 16 + r16) * F_PITCH + k];
#pragma unroll
  for (int b = 0; b < 4; ++b) fy[b] = yb[(wn * 64 + b * 16 + r16) * F_PITCH + k];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fy[b], fx[a], acc[a][b], 0, 0, 0);
}

__global__ __launch_bounds__(256) void distance_f32_kernel(const float *__restrict__ X, const float *__restrict__ Y, float *__restrict__ D,
                                                           int n, int m, int p, int tiles_n, bool vec) {
  // [buffer][X panel | Y panel][128 rows x F_PITCH]; after the K loop the epilogue restages the results here
  __shared__ __attribute__((aligned(16))) float panels[2][2][F_TILE * F_PITCH];
  __shared__ __attribute__((aligned(16))) float nrm[2 * F_TILE];   // x2 of the tile's 128 X rows, then y2 of its 128 Y rows

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int row0 = (int)(blockIdx.x / (unsigned)tiles_n) * F_TILE;   // X rows (rows of D)
  const int col0 = (int)(blockIdx.x % (unsigned)tiles_n) * F_TILE;   // Y rows (columns of D)
  const int stages = (p + F_KS - 1) / F_KS;

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  float sq = 0.f;                 // thread t: the norm of staged row t (t < 128: X row row0 + t, else Y row col0 + t - 128)

  float rx[8], ry[8];
  f32_load(rx, X, n, p, row0, 0);
  f32_load(ry, Y, m, p, col0, 0);
  f32_store_lds(panels[0][0], rx);
  f32_store_lds(panels[0][1], ry);
  __syncthreads();

  const int r16 = lane & 15, g = lane >> 4;
  for (int s = 0; s < stages; ++s) {
    const int buf = s & 1, k0 = s * F_KS;
    if (s + 1 < stages) {
      f32_load(rx, X, n, p, row0, k0 + F_KS);
      f32_load(ry, Y, m, p, col0, k0 + F_KS);
    }
    const float *xb = panels[buf][0], *yb = panels[buf][1];
    {
      const float *mine = (t < F_TILE ? xb + t * F_PITCH : yb + (t - F_TILE) * F_PITCH);
#pragma unroll
      for (int c = 0; c < F_KS / 4; ++c) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(mine + 4 * c);
#pragma unroll
        for (int j = 0; j < 4; ++j) sq = __builtin_fmaf(v[j], v[j], sq);
      }
    }
    // k-steps of 4 that hold any k < p (the rest of the stage is zero padding)
    const int steps = min(F_KS / 4, (p - k0 + 3) >> 2);
    for (int q = 0; q < steps; ++q) f32_kstep(acc, xb, yb, wm, wn, r16, 4 * q + g);
    if (s + 1 < stages) {
      f32_store_lds(panels[buf ^ 1][0], rx);
      f32_store_lds(panels[buf ^ 1][1], ry);
    }
    __syncthreads();
  }
  nrm[t] = sq;
  __syncthreads();

  // Epilogue in four passes of 16 rows per wave: the results go through LDS (the panels are free now) so that every store
  // instruction writes whole row segments of D -- 64 consecutive floats (dword stores: any m) or 4 rows x 64 floats (16-byte
  // stores when m % 4 == 0 and D is 16-byte aligned) -- instead of 16 rows x 4 floats.
  float *ep = &panels[0][0][0] + wave * (16 * EP_PITCH);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float x2 = nrm[wm * 64 + a * 16 + r16];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int lj = wn * 64 + b * 16 + 4 * g;
      const f32x4 y2 = *reinterpret_cast<const f32x4 *>(nrm + F_TILE + lj);
      f32x4 out;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        float d = (x2 + y2[v]) - 2.0f * acc[a][b][v];
        if (d < 0.f) d = 0.f;                 // D[D < 0] = 0 (NaN stays NaN)
        // correctly rounded float sqrt: a double sqrt rounded to float (53 >= 2*24 + 2), as edge_similarity_kernel
        out[v] = (float)sqrt((double)d);
      }
      *reinterpret_cast<f32x4 *>(ep + r16 * EP_PITCH + b * 16 + 4 * g) = out;
    }
    __syncthreads();
    const int i0 = row0 + wm * 64 + a * 16;              // first D row of this pass
    const int j0 = col0 + wn * 64;                       // first D column of the wave
    if (vec) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rr = 4 * q + (lane >> 4), c = 4 * (lane & 15);
        const f32x4 val = *reinterpret_cast<const f32x4 *>(ep + rr * EP_PITCH + c);
        if (i0 + rr < n && j0 + c < m) *reinterpret_cast<f32x4 *>(D + (long long)(i0 + rr) * m + j0 + c) = val;
      }
    } else {
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        const float val = ep[rr * EP_PITCH + lane];
        if (i0 + rr < n && j0 + lane < m) D[(long long)(i0 + rr) * m + j0 + lane] = val;
      }
    }
    __syncthreads();
  }
}

// ---- fp64: 64x64 tile per 256-thread workgroup on VALU fma(double); thread (ty, tx) owns rows ty + 16 a, columns tx + 16 b -------
constexpr int D_TILE = 64;
constexpr int D_KS = 16;
constexpr int D_PITCH = D_TILE + 1;   // k-major panels [k][row]

__global__ __launch_bounds__(256) void distance_f64_kernel(const double *__restrict__ X, const double *__restrict__ Y, double *__restrict__ D,
                                                           int n, int m, int p, int tiles_n) {
  __shared__ double xs[D_KS * D_PITCH];
  __shared__ double ys[D_KS * D_PITCH];
  __shared__ double nrm[2 * D_TILE];

  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int row0 = (int)(blockIdx.x / (unsigned)tiles_n) * D_TILE;
  const int col0 = (int)(blockIdx.x % (unsigned)tiles_n) * D_TILE;

  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  double sq = 0.0;                // t < 128: norm of panel row t (X rows, then Y rows)

  for (int k0 = 0; k0 < p; k0 += D_KS) {
    // element e = t + 256 q of each 64 x 16 panel: row e / 16, k e % 16
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = t + 256 * q, r = e >> 4, k = k0 + (e & 15);
      xs[(e & 15) * D_PITCH + r] = (row0 + r < n && k < p) ? X[(long long)(row0 + r) * p + k] : 0.0;
      ys[(e & 15) * D_PITCH + r] = (col0 + r < m && k < p) ? Y[(long long)(col0 + r) * p + k] : 0.0;
    }
    __syncthreads();
    if (t < 2 * D_TILE) {
      const double *mine = (t < D_TILE ? xs + t : ys + (t - D_TILE));
#pragma unroll
      for (int kk = 0; kk < D_KS; ++kk) sq = fma(mine[kk * D_PITCH], mine[kk * D_PITCH], sq);
    }
#pragma unroll 4
    for (int kk = 0; kk < D_KS; ++kk) {
      double fx[4], fy[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) fx[a] = xs[kk * D_PITCH + ty + 16 * a];
#pragma unroll
      for (int b = 0; b < 4; ++b) fy[b] = ys[kk * D_PITCH + tx + 16 * b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = fma(fx[a], fy[b], acc[a][b]);
    }
    __syncthreads();
  }
  if (t < 2 * D_TILE) nrm[t] = sq;
  __syncthreads();

#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = row0 + ty + 16 * a;
    if (i >= n) continue;
    const double x2 = nrm[ty + 16 * a];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = col0 + tx + 16 * b;
      if (j >= m) continue;
      double d = (x2 + nrm[D_TILE + tx + 16 * b]) - 2.0 * acc[a][b];
      if (d < 0.0) d = 0.0;
      D[(long long)i * m + j] = sqrt(d);
    }
  }
}

}  // namespace

extern "C" int dm_pairwise_distance(const void *X, const void *Y, void *D, int32_t n, int32_t m, int32_t p, int32_t dtype, void *stream) {
  DM_REQUIRE(X && Y && D && n >= 1 && m >= 1 && p >= 1, DM_ERR_BAD_SHAPE,
             "dm_pairwise_distance: bad arguments (n = %d, m = %d, p = %d must be >= 1, pointers non-null)", n, m, p);
  DM_REQUIRE(dtype == DM_F32 || dtype == DM_F64, DM_ERR_BAD_DTYPE, "dm_pairwise_distance: dtype %d is not DM_F32 or DM_F64", dtype);
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int tile = dtype == DM_F32 ? F_TILE : D_TILE;
  const long long tiles_m = (n + tile - 1) / tile, tiles_n = (m + tile - 1) / tile;
  DM_REQUIRE(tiles_m * tiles_n <= 0x7fffffffLL / 256, DM_ERR_UNSUPPORTED, "dm_pairwise_distance: %d x %d result exceeds one launch", n, m);
  const dim3 grid((unsigned)(tiles_m * tiles_n));
  if (dtype == DM_F32) {
    const bool vec = (m % 4) == 0 && dm_aligned16(D);
    hipLaunchKernelGGL(distance_f32_kernel, grid, dim3(256), 0, st, static_cast<const float *>(X), static_cast<const float *>(Y),
                       static_cast<float *>(D), n, m, p, (int)tiles_n, vec);
  } else {
    hipLaunchKernelGGL(distance_f64_kernel, grid, dim3(256), 0, st, static_cast<const double *>(X), static_cast<const double *>(Y),
                       static_cast<double *>(D), n, m, p, (int)tiles_n);
  }
  DM_LAUNCH_CHECK("dm_pairwise_distance");
  return DM_OK;
}
