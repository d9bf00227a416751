// The SLIC assignment pass and the centre update, once, for a tile (dm_slic.hip: the raster is the whole image, origin zero) and
// for a core of a scene (dm_scene_slic.hip: the raster is the core at (y0, x0) of an H x W scene, the centre table is the scene's).
// The rule is stated in include/deepmerge_hip.h; everything is an integer and every reduction an integer add, so neither form
// depends on the order in which threads arrive, and a scene's sums are the sums of its cores.
//
// What the scene form changes (SCENE = true; at SCENE = false the origin is the constant 0 and the code is the tile form's):
//   - a pixel's position, its grid cell and the staged window of centres come from scene coordinates (y0 + y, x0 + x);
//   - the workgroup's 64x64 tiles are aligned to the core, not to the grid: 64 rows from any start meet at most 63 / cell + 2
//     grid rows, with one more on either side 63 / cell + 4 <= 64 / cell + 3 for cell >= 4: SLIC_SIDE stays 19;
//   - the tile-relative sums are flushed as acc + n * (y0 + Y0) in 64 bits;
//   - loads and label stores use core-local indices.
#pragma once
#include <type_traits>

#include "dm_raster.h"

namespace {

// A centre of grid cell J only ever owns pixels of the cells J-1 .. J+1, so its rounded mean stays inside them: a pixel and a
// candidate centre are less than 3 cell apart on either axis, and a 64-row tile sees the centres of at most 64 / cell + 3 grid
// rows (cell >= 4: 19).
constexpr int SLIC_SIDE = 19, SLIC_SLOTS = SLIC_SIDE * SLIC_SIDE;
constexpr int CENTRE_INTS = 6;                                  // y, x, band 0..3
constexpr int SUM_INTS = 7;                                     // n, sum y, sum x, sum band 0..3

// Rounded mean (2 sum + n) / (2 n) of every centre that owns a pixel; the sums are cleared for the next pass.
__global__ void slic_update_kernel(int K, int *__restrict__ centres, long long *__restrict__ sums) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= K) return;
  long long *s = sums + (long long)c * SUM_INTS;
  const long long n = s[0];
  if (n > 0)
    for (int k = 0; k < CENTRE_INTS; ++k) centres[(long long)c * CENTRE_INTS + k] = (int)((2 * s[1 + k] + n) / (2 * n));
  for (int k = 0; k < SUM_INTS; ++k) s[k] = 0;
}

// The strip's pixels, band b in byte b of pix[i] (bands >= NB stay 0).
template <int NB, bool VEC>
__device__ __forceinline__ void load_pixels(const uint8_t *__restrict__ tile, long long plane, long long base, int n, unsigned *pix) {
#pragma unroll
  for (int i = 0; i < STRIP; ++i) pix[i] = 0;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const uint8_t *p = tile + b * plane + base;
    if (VEC && n == STRIP) {
      const u32x4 v = *reinterpret_cast<const u32x4 *>(p);
#pragma unroll
      for (int i = 0; i < STRIP; ++i) pix[i] |= ((v[i >> 2] >> (8 * (i & 3))) & 0xffu) << (8 * b);
    } else {
#pragma unroll
      for (int i = 0; i < STRIP; ++i)
        if (i < n) pix[i] |= (unsigned)p[i] << (8 * b);
    }
  }
}

// tile uint8 [NB.., h, w]: the raster the workgroups walk, whose first pixel is (y0, x0) of the H x W raster the gy x gx grid of
// centres belongs to (SCENE = false: y0 = x0 = 0, h = H, w = W).  labels int32 [h, w].
// D: unsigned 32-bit where the host proved cell^2 (NB 255^2 + 18 compactness^2) < 2^32, else 64-bit.
template <int NB, bool WIDE, bool VEC, bool SCENE>
__global__ __launch_bounds__(256) void slic_pass_kernel(const uint8_t *__restrict__ tile, long long plane, int h, int w, int y0_, int x0_,
                                                        int H, int W, int cell, int gy, int gx, unsigned cell2, unsigned comp2,
                                                        const int *__restrict__ centres, long long *__restrict__ sums,
                                                        int *__restrict__ labels) {
  typedef typename std::conditional<WIDE, u64, unsigned>::type dist_t;
  __shared__ int c_y[SLIC_SLOTS], c_x[SLIC_SLOTS];
  __shared__ unsigned c_col[SLIC_SLOTS];
  __shared__ int acc[SLIC_SLOTS * SUM_INTS];
  const int oy = SCENE ? y0_ : 0, ox = SCENE ? x0_ : 0;          // the raster's origin
  const int tiles_x = (w + 63) / 64;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int Y0 = ty * 64, X0 = tx * 64;                           // in the raster
  const int j0 = max(0, (oy + Y0) / cell - 1), j1 = min(gy - 1, (oy + min(h - 1, Y0 + 63)) / cell + 1);
  const int i0 = max(0, (ox + X0) / cell - 1), i1 = min(gx - 1, (ox + min(w - 1, X0 + 63)) / cell + 1);
  const int nj = j1 - j0 + 1, ni = i1 - i0 + 1;                  // <= SLIC_SIDE each
  for (int s = threadIdx.x; s < nj * ni; s += blockDim.x) {
    const int jj = s / ni, ii = s - jj * ni;
    const int *c = centres + ((long long)(j0 + jj) * gx + i0 + ii) * CENTRE_INTS;
    c_y[s] = c[0];
    c_x[s] = c[1];
    c_col[s] = (unsigned)c[2] | (unsigned)c[3] << 8 | (unsigned)c[4] << 16 | (unsigned)c[5] << 24;
    for (int k = 0; k < SUM_INTS; ++k) acc[s * SUM_INTS + k] = 0;
  }
  __syncthreads();

  const Strip g = strip_of(h, w);
  if (g.live) {
    unsigned pix[STRIP];
    load_pixels<NB, VEC>(tile, plane, g.base, g.n, pix);
    const int py = oy + g.y;                                      // the strip's row and first column in the grid's raster
    const int j = py / cell;
    int i = (ox + g.x0) / cell, rem = (ox + g.x0) - i * cell;
    // the 9 candidates of grid cell (j, i), in ascending centre id; slot < 0: outside the grid
    int k_slot[9], k_y[9], k_x[9];
    unsigned k_col[9];
    dist_t k_dy[9];
    auto reload = [&]() {
#pragma unroll
      for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
        for (int di = -1; di <= 1; ++di) {
          const int k = (dj + 1) * 3 + di + 1, cj = j + dj, ci = i + di;
          const bool in = cj >= 0 && cj < gy && ci >= 0 && ci < gx;
          const int s = in ? (cj - j0) * ni + (ci - i0) : -1;
          k_slot[k] = s;
          k_y[k] = in ? c_y[s] : 0;
          k_x[k] = in ? c_x[s] : 0;
          k_col[k] = in ? c_col[s] : 0;
          const int dy = py - k_y[k];
          k_dy[k] = (dist_t)comp2 * (dist_t)(unsigned)(dy * dy);
        }
    };
    reload();
    int out[STRIP];
    int run_slot = -1, run_n = 0, run_x = 0, run_b[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) run_b[b] = 0;
    auto flush = [&]() {
      if (run_n == 0) return;
      int *a = acc + run_slot * SUM_INTS;
      atomicAdd(a + 0, run_n);
      atomicAdd(a + 1, run_n * (g.y - Y0));
      atomicAdd(a + 2, run_x);
#pragma unroll
      for (int b = 0; b < NB; ++b) atomicAdd(a + 3 + b, run_b[b]);
    };
#pragma unroll
    for (int p = 0; p < STRIP; ++p) {
      if (p < g.n) {
        const int x = g.x0 + p;
        dist_t best = 0;
        int best_k = -1;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          unsigned dc = 0;
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            const int d = (int)((pix[p] >> (8 * b)) & 0xffu) - (int)((k_col[k] >> (8 * b)) & 0xffu);
            dc += (unsigned)(d * d);
          }
          const int dx = ox + x - k_x[k];
          const dist_t D = (dist_t)cell2 * (dist_t)dc + k_dy[k] + (dist_t)comp2 * (dist_t)(unsigned)(dx * dx);
          const bool better = (k_slot[k] >= 0) & ((best_k < 0) | (D < best));      // selects, no branches: the grid's edge is rare
          best = better ? D : best;
          best_k = better ? k : best_k;
        }
        int slot = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k)
          if (k == best_k) slot = k_slot[k];
        const int sj = slot / ni;
        out[p] = (j0 + sj) * gx + i0 + (slot - sj * ni);
        if (sums) {
          if (slot != run_slot) {
            flush();
            run_slot = slot; run_n = 0; run_x = 0;
#pragma unroll
            for (int b = 0; b < NB; ++b) run_b[b] = 0;
          }
          ++run_n;
          run_x += x - X0;
#pragma unroll
          for (int b = 0; b < NB; ++b) run_b[b] += (int)((pix[p] >> (8 * b)) & 0xffu);
        }
        if (++rem == cell) {
          rem = 0; ++i;
          if (p + 1 < g.n) reload();                               // the next pixel is in the tile: its candidates are staged
        }
      } else {
        out[p] = 0;
      }
    }
    if (sums) flush();
    if (labels) {
      if (VEC && g.n == STRIP) {
#pragma unroll
        for (int v = 0; v < STRIP / 4; ++v)
          *reinterpret_cast<i32x4 *>(labels + g.base + 4 * v) = (i32x4){out[4 * v], out[4 * v + 1], out[4 * v + 2], out[4 * v + 3]};
      } else {
#pragma unroll
        for (int p = 0; p < STRIP; ++p)
          if (p < g.n) labels[g.base + p] = out[p];
      }
    }
  }
  if (!sums) return;
  __syncthreads();
  for (int s = threadIdx.x; s < nj * ni; s += blockDim.x) {
    const int n = acc[s * SUM_INTS];
    if (n == 0) continue;
    const int jj = s / ni, ii = s - jj * ni;
    long long *dst = sums + ((long long)(j0 + jj) * gx + i0 + ii) * SUM_INTS;
    atomic_add64(dst + 0, n);
    atomic_add64(dst + 1, (long long)acc[s * SUM_INTS + 1] + (long long)n * (oy + Y0));     // tile-relative sums fit 32 bits: 4096 * 63
    atomic_add64(dst + 2, (long long)acc[s * SUM_INTS + 2] + (long long)n * (ox + X0));
#pragma unroll
    for (int b = 0; b < NB; ++b) atomic_add64(dst + 3 + b, acc[s * SUM_INTS + 3 + b]);
  }
}

// One raster's assignment pass.  origin: where the raster lies in the grid's H x W raster.
struct SlicPass {
  int nb;                 // bands used, 1..4
  bool wide, vec;         // 64-bit distances; 16-byte strip loads / stores
  int h, w, y0, x0;       // the raster and its origin
  int H, W, cell, gy, gx; // the grid's raster and the grid
  unsigned comp2;
};

template <int NB, bool WIDE, bool SCENE>
void launch_pass(const SlicPass &a, hipStream_t s, const uint8_t *tile, const int *centres, long long *sums, int *labels) {
  const long long plane = (long long)a.h * a.w;
  const unsigned cell2 = (unsigned)(a.cell * a.cell);
  if (a.vec)
    hipLaunchKernelGGL((slic_pass_kernel<NB, WIDE, true, SCENE>), tile_grid(a.h, a.w), dim3(256), 0, s, tile, plane, a.h, a.w, a.y0, a.x0, a.H, a.W,
                       a.cell, a.gy, a.gx, cell2, a.comp2, centres, sums, labels);
  else
    hipLaunchKernelGGL((slic_pass_kernel<NB, WIDE, false, SCENE>), tile_grid(a.h, a.w), dim3(256), 0, s, tile, plane, a.h, a.w, a.y0, a.x0, a.H, a.W,
                       a.cell, a.gy, a.gx, cell2, a.comp2, centres, sums, labels);
}

template <bool SCENE>
void slic_pass(const SlicPass &a, hipStream_t s, const uint8_t *tile, const int *centres, long long *sums, int *labels) {
#define DM_PASS(NB_)                                                                 \
  do {                                                                               \
    if (a.wide) launch_pass<NB_, true, SCENE>(a, s, tile, centres, sums, labels);    \
    else launch_pass<NB_, false, SCENE>(a, s, tile, centres, sums, labels);          \
  } while (0)
  switch (a.nb) {
    case 1: DM_PASS(1); break;
    case 2: DM_PASS(2); break;
    case 3: DM_PASS(3); break;
    default: DM_PASS(4); break;
  }
#undef DM_PASS
}

// D <= cell^2 (nb 255^2 + 2 * 3^2 compactness^2): a pixel and a candidate centre are less than 3 cell apart on either axis
inline bool slic_wide(int cell, int nb, unsigned comp2) { return (u64)cell * cell * ((u64)nb * 65025 + 18ULL * comp2) >= (1ULL << 32); }

}  // namespace
