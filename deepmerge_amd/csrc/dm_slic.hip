// SLIC superpixels from an image tile to a label raster, and 4-connected component labelling (gfx950).  The segmentation the
// reference reads from shapefiles written by external GIS software; the rule is the build's own: stated in
// include/deepmerge_hip.h, restated in numpy in tests/slic_ref.py.
//
// Every quantity is an integer and every reduction an integer add / min / max, so the result does not depend on the order in
// which threads arrive: the GPU and the numpy spec agree bit for bit.  No floating point anywhere in this file.
//
// The passes run on dm_raster.h's tile walk (a workgroup per 64x64 tile, a thread per 16-pixel strip: one 16-byte load per band):
//   slic_pass_kernel   (dm_slic_pass.h, shared with the scene form in dm_scene_slic.hip; here at origin zero)
//                      assignment: the centres a tile can see are staged in LDS, every pixel takes the nearest of the 9 centres
//                      around its grid cell, the next centres' sums are collected per tile with integer LDS atomics (one group
//                      per run of equal assignments in a strip) and flushed once per tile with 64-bit global adds; only the
//                      last pass writes labels.  slic_update_kernel turns sums into centres.  No readback inside the loop.
//   ccl_*              tile-local union-find in LDS, joins across tile borders in global memory (min-index hooking with
//                      atomicMin: the representative of a component is its smallest linear pixel index whatever the schedule),
//                      flatten, renumber by first pixel (a scan over "is root" on block_exclusive), apply.
//   label_area_kernel / absorb_*   what a round of the absorption needs beside rag_edges, merge_components and relabel_raster.
#include "dm_slic_pass.h"

namespace {

// ---- SLIC assignment pass: dm_slic_pass.h, here at origin zero --------------------------------------------------------------
__global__ void slic_init_kernel(const uint8_t *__restrict__ tile, long long plane, int H, int W, int nb, int cell, int gx, int K,
                                 int *__restrict__ centres, long long *__restrict__ sums) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= K) return;
  const int j = c / gx, i = c - j * gx;
  const int y = min(H - 1, j * cell + cell / 2), x = min(W - 1, i * cell + cell / 2);
  centres[c * CENTRE_INTS + 0] = y;
  centres[c * CENTRE_INTS + 1] = x;
  for (int b = 0; b < 4; ++b) centres[c * CENTRE_INTS + 2 + b] = b < nb ? (int)tile[b * plane + (long long)y * W + x] : 0;
  for (int k = 0; k < SUM_INTS; ++k) sums[(long long)c * SUM_INTS + k] = 0;
}

// ---- 4-connected components ---------------------------------------------------------------------------------------------
// Union-find with min-index hooking.  Parents only ever decrease and always name a pixel of the same component, so a find that
// races with a hook still ends at a root candidate, and the loop in `unite` retries until the two roots are one.
__device__ __forceinline__ int uf_load(const int *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

__device__ __forceinline__ int uf_root(const int *parent, int x) {
  int p = uf_load(parent + x);
  while (p != x) { x = p; p = uf_load(parent + x); }
  return x;
}

__device__ __forceinline__ void uf_unite(int *parent, int a, int b) {
  while (true) {
    a = uf_root(parent, a);
    b = uf_root(parent, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }               // a < b: hook b under a
    const int old = atomicMin(parent + b, a);
    if (old == b) return;
    b = old;                                                     // somebody hooked b first: unite a with where it went
  }
}

// Components inside a 64x64 tile, in LDS; parent[pixel] = linear index of the tile-local root (its first pixel), -1 for background.
template <bool VEC>
__global__ __launch_bounds__(256) void ccl_tile_kernel(const int *__restrict__ raster, int H, int W, int use_bg, int bg, int *__restrict__ parent) {
  __shared__ int val[64 * 64], par[64 * 64];
  const Strip g = strip_of(H, W);
  const int ly = threadIdx.x >> 2, lx0 = (threadIdx.x & 3) * STRIP, l0 = ly * 64 + lx0;
  int v[STRIP];
  load_strip<VEC>(raster, g.base, g.n, 0, v);
  int start = l0;
#pragma unroll
  for (int i = 0; i < STRIP; ++i) {                              // a run of equal values in the strip hangs under its first pixel
    if (i > 0 && v[i] != v[i - 1]) start = l0 + i;
    val[l0 + i] = v[i];
    par[l0 + i] = start;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < STRIP; ++i) {
    if (i >= g.n || (use_bg && v[i] == bg)) continue;
    if (ly > 0) {
      const int up = val[l0 + i - 64];
      // a run that continues under an equal run above is already joined through its previous pixel
      const bool joined = i > 0 && v[i - 1] == v[i] && val[l0 + i - 65] == v[i];
      if (up == v[i] && !joined) uf_unite(par, l0 + i, l0 + i - 64);
    }
    if (i == 0 && lx0 > 0 && val[l0 - 1] == v[0]) uf_unite(par, l0, l0 - 1);
  }
  __syncthreads();
  const int tiles_x = (W + 63) / 64;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
#pragma unroll
  for (int i = 0; i < STRIP; ++i) {
    if (i >= g.n) continue;
    const int r = uf_root(par, l0 + i);
    parent[g.base + i] = (use_bg && v[i] == bg) ? -1 : (ty * 64 + (r >> 6)) * W + tx * 64 + (r & 63);
  }
}

// Joins across tile borders: the tile's top row with the row above, its left column with the column to the left.
__global__ __launch_bounds__(128) void ccl_border_kernel(const int *__restrict__ raster, int H, int W, int use_bg, int bg, int *parent) {
  const int tiles_x = (W + 63) / 64;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const bool top = threadIdx.x < 64;
  const int t = threadIdx.x & 63;
  const int y = ty * 64 + (top ? 0 : t), x = tx * 64 + (top ? t : 0);
  if (y >= H || x >= W || (top ? y == 0 : x == 0)) return;
  const int a = y * W + x, b = top ? a - W : a - 1;
  const int v = raster[a];
  if (v != raster[b] || (use_bg && v == bg)) return;
  uf_unite(parent, a, b);
}

// parent[i] = root of i; counts[chunk] = roots in the chunk of SCAN_TILE pixels.
__global__ __launch_bounds__(SCAN_THREADS) void ccl_flatten_kernel(int *parent, int N, int *__restrict__ counts) {
  __shared__ int roots;
  if (threadIdx.x == 0) roots = 0;
  __syncthreads();
  int mine = 0;
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    const long long i = (long long)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS + j;
    if (i >= N) break;
    if (uf_load(parent + i) < 0) continue;
    const int r = uf_root(parent, (int)i);
    __atomic_store_n(parent + i, r, __ATOMIC_RELAXED);
    mine += r == (int)i;
  }
  if (mine) atomicAdd(&roots, mine);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = roots;
}

// Exclusive scan of the chunk counts in place, by one looping workgroup; counts[n_chunks] = n_out[0] = the total.
__global__ __launch_bounds__(SCAN_THREADS) void ccl_scan_kernel(int *__restrict__ counts, int n_chunks, int *__restrict__ n_out) {
  __shared__ int lds[SCAN_THREADS / 64];
  int carry = 0;
  for (int base = 0; base < n_chunks; base += SCAN_TILE) {
    int item[SCAN_ITEMS], sum = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      const int i = base + threadIdx.x * SCAN_ITEMS + j;
      item[j] = i < n_chunks ? counts[i] : 0;
      sum += item[j];
    }
    int total;
    int run = carry + block_exclusive(sum, lds, total);
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      const int i = base + threadIdx.x * SCAN_ITEMS + j;
      if (i < n_chunks) counts[i] = run;
      run += item[j];
    }
    carry += total;
  }
  if (threadIdx.x == 0) { counts[n_chunks] = carry; *n_out = carry; }
}

// labels[root] = rank of the root among the roots in raster-scan order.
__global__ __launch_bounds__(SCAN_THREADS) void ccl_rank_kernel(const int *__restrict__ parent, int N, const int *__restrict__ offsets,
                                                                int *__restrict__ labels) {
  __shared__ int lds[SCAN_THREADS / 64];
  int flag[SCAN_ITEMS], sum = 0;
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    const long long i = (long long)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS + j;
    flag[j] = (i < N && parent[i] == (int)i) ? 1 : 0;
    sum += flag[j];
  }
  int total;
  int run = offsets[blockIdx.x] + block_exclusive(sum, lds, total);
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    const long long i = (long long)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS + j;
    if (flag[j]) labels[i] = run;
    run += flag[j];
  }
}

// Every other pixel takes its root's rank (a root's entry is read, never written here); background pixels get -1.
__global__ __launch_bounds__(256) void ccl_apply_kernel(const int *__restrict__ parent, int N, int *labels) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
    const int p = parent[i];
    if (p == (int)i) continue;
    labels[i] = p < 0 ? -1 : labels[p];
  }
}

// ---- absorption ------------------------------------------------------------------------------------------------------------
__global__ void area_clear_kernel(int *__restrict__ area, int S) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < S) area[i] = 0;
}

template <bool VEC>
__global__ __launch_bounds__(256) void label_area_kernel(const int *__restrict__ labels, int H, int W, int S, int *__restrict__ area) {
  const Strip g = strip_of(H, W);
  int lab[STRIP];
  load_strip<VEC>(labels, g.base, g.n, -1, lab);
  int run = -1, cnt = 0;
#pragma unroll
  for (int i = 0; i < STRIP; ++i) {
    const int l = (i < g.n && (unsigned)lab[i] < (unsigned)S) ? lab[i] : -1;
    if (l == run) { ++cnt; continue; }
    if (run >= 0) atomicAdd(area + run, cnt);
    run = l; cnt = 1;
  }
  if (run >= 0) atomicAdd(area + run, cnt);
}

__global__ void absorb_clear_kernel(u64 *__restrict__ best, int S, int *__restrict__ n_picked) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < S) best[i] = 0;
  if (i == 0) *n_picked = 0;
}

// best[r] = max of (weight << 32) | (0xFFFFFFFF - neighbour) over the edges at a region smaller than min_size (weights >= 1, so 0 = none).
__global__ __launch_bounds__(256) void absorb_best_kernel(const int *__restrict__ edges, const int *__restrict__ weights, int E,
                                                          const int *__restrict__ area, int S, int min_size, u64 *__restrict__ best) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (long long)gridDim.x * blockDim.x) {
    const int a = edges[2 * e], b = edges[2 * e + 1], w = weights[e];
    if ((unsigned)a >= (unsigned)S || (unsigned)b >= (unsigned)S || a == b || w <= 0) continue;
    if (area[a] < min_size) atomicMax(best + a, ((u64)(unsigned)w << 32) | (u64)(0xFFFFFFFFu - (unsigned)b));
    if (area[b] < min_size) atomicMax(best + b, ((u64)(unsigned)w << 32) | (u64)(0xFFFFFFFFu - (unsigned)a));
  }
}

// merge[e] = 1 iff one end of the edge picked the other.
__global__ __launch_bounds__(256) void absorb_flag_kernel(const int *__restrict__ edges, int E, int S, const u64 *__restrict__ best,
                                                          unsigned char *__restrict__ merge, int *__restrict__ n_picked) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (long long)gridDim.x * blockDim.x) {
    const int a = edges[2 * e], b = edges[2 * e + 1];
    bool p = false;
    if ((unsigned)a < (unsigned)S && (unsigned)b < (unsigned)S && a != b) {
      const u64 ba = best[a], bb = best[b];
      p = (ba != 0 && (unsigned)ba == 0xFFFFFFFFu - (unsigned)b) || (bb != 0 && (unsigned)bb == 0xFFFFFFFFu - (unsigned)a);
    }
    merge[e] = p ? 1 : 0;
    if (p) atomicAdd(n_picked, 1);
  }
}

}  // namespace

extern "C" int dm_slic_iterate(const uint8_t *tile, int32_t bands, int32_t H, int32_t W, int32_t cell, int32_t compactness, int32_t iters,
                               int32_t *centres, int64_t *sums, int32_t *labels, void *stream) {
  DM_REQUIRE(tile && centres && sums && labels, DM_ERR_BAD_SHAPE, "dm_slic_iterate: null pointer");
  DM_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1LL << 31) && bands >= 1, DM_ERR_BAD_SHAPE,
             "dm_slic_iterate: bad sizes (bands=%d H=%d W=%d; need bands >= 1, H*W < 2^31)", bands, H, W);
  DM_REQUIRE(cell >= 4 && cell <= 256, DM_ERR_BAD_SHAPE, "dm_slic_iterate: cell = %d outside 4..256", cell);
  DM_REQUIRE(compactness >= 0 && compactness <= 255, DM_ERR_BAD_SHAPE, "dm_slic_iterate: compactness = %d outside 0..255", compactness);
  DM_REQUIRE(iters >= 0, DM_ERR_BAD_SHAPE, "dm_slic_iterate: iters = %d is negative", iters);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nb = bands < 4 ? bands : 4;
  const int gy = (H + cell - 1) / cell, gx = (W + cell - 1) / cell, K = gy * gx;
  const unsigned comp2 = (unsigned)(compactness * compactness);
  // 16-byte strip loads / stores need W % 16 == 0 (then every band plane keeps the alignment) and 16-byte aligned rasters
  const bool vec = W % STRIP == 0 && dm_aligned16(tile) && dm_aligned16(labels);
  const SlicPass pass = {nb, slic_wide(cell, nb, comp2), vec, H, W, 0, 0, H, W, cell, gy, gx, comp2};
  const long long plane = (long long)H * W;
  hipLaunchKernelGGL(slic_init_kernel, dim3((K + 255) / 256), dim3(256), 0, s, tile, plane, H, W, nb, cell, gx, K, centres, (long long *)sums);
  for (int it = 0; it < iters; ++it) {
    slic_pass<false>(pass, s, tile, centres, (long long *)sums, nullptr);
    hipLaunchKernelGGL(slic_update_kernel, dim3((K + 255) / 256), dim3(256), 0, s, K, centres, (long long *)sums);
  }
  slic_pass<false>(pass, s, tile, centres, nullptr, labels);
  DM_LAUNCH_CHECK("dm_slic_iterate");
  return DM_OK;
}

extern "C" int dm_connected_labels(const int32_t *raster, int32_t H, int32_t W, int32_t use_background, int32_t background, int32_t *parent,
                                   int32_t *chunk_counts, int32_t *labels, int32_t *n_labels, void *stream) {
  DM_REQUIRE(raster && parent && chunk_counts && labels && n_labels, DM_ERR_BAD_SHAPE, "dm_connected_labels: null pointer");
  DM_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1LL << 31), DM_ERR_BAD_SHAPE, "dm_connected_labels: bad sizes (H=%d W=%d; need H*W < 2^31)", H, W);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int N = H * W, n_chunks = (N + SCAN_TILE - 1) / SCAN_TILE;
  const int bg = use_background ? 1 : 0;
  if (W % STRIP == 0 && dm_aligned16(raster))
    hipLaunchKernelGGL(ccl_tile_kernel<true>, tile_grid(H, W), dim3(256), 0, s, raster, H, W, bg, background, parent);
  else
    hipLaunchKernelGGL(ccl_tile_kernel<false>, tile_grid(H, W), dim3(256), 0, s, raster, H, W, bg, background, parent);
  hipLaunchKernelGGL(ccl_border_kernel, tile_grid(H, W), dim3(128), 0, s, raster, H, W, bg, background, parent);
  hipLaunchKernelGGL(ccl_flatten_kernel, dim3(n_chunks), dim3(SCAN_THREADS), 0, s, parent, N, chunk_counts);
  hipLaunchKernelGGL(ccl_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, chunk_counts, n_chunks, n_labels);
  hipLaunchKernelGGL(ccl_rank_kernel, dim3(n_chunks), dim3(SCAN_THREADS), 0, s, (const int *)parent, N, (const int *)chunk_counts, labels);
  hipLaunchKernelGGL(ccl_apply_kernel, dim3(grid_for(N, 4096)), dim3(256), 0, s, (const int *)parent, N, labels);
  DM_LAUNCH_CHECK("dm_connected_labels");
  return DM_OK;
}

extern "C" int dm_label_area(const int32_t *labels, int32_t H, int32_t W, int32_t S, int32_t *area, void *stream) {
  DM_REQUIRE(labels && area, DM_ERR_BAD_SHAPE, "dm_label_area: null pointer");
  DM_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1LL << 31) && S > 0, DM_ERR_BAD_SHAPE,
             "dm_label_area: bad sizes (H=%d W=%d S=%d; need H*W < 2^31)", H, W, S);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(area_clear_kernel, dim3((S + 255) / 256), dim3(256), 0, s, area, S);
  if (W % STRIP == 0 && dm_aligned16(labels))
    hipLaunchKernelGGL(label_area_kernel<true>, tile_grid(H, W), dim3(256), 0, s, labels, H, W, S, area);
  else
    hipLaunchKernelGGL(label_area_kernel<false>, tile_grid(H, W), dim3(256), 0, s, labels, H, W, S, area);
  DM_LAUNCH_CHECK("dm_label_area");
  return DM_OK;
}

extern "C" int dm_slic_absorb_pick(const int32_t *edges, const int32_t *weights, int32_t E, const int32_t *area, int32_t S, int32_t min_size,
                                   uint64_t *best, uint8_t *merge, int32_t *n_picked, void *stream) {
  DM_REQUIRE(edges && weights && area && best && merge && n_picked, DM_ERR_BAD_SHAPE, "dm_slic_absorb_pick: null pointer");
  DM_REQUIRE(E > 0 && S > 0 && min_size >= 1, DM_ERR_BAD_SHAPE, "dm_slic_absorb_pick: bad sizes (E=%d S=%d min_size=%d; need E, S, min_size >= 1)", E,
             S, min_size);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(absorb_clear_kernel, dim3((S + 255) / 256), dim3(256), 0, s, (u64 *)best, S, n_picked);
  hipLaunchKernelGGL(absorb_best_kernel, dim3(grid_for(E)), dim3(256), 0, s, edges, weights, E, area, S, min_size, (u64 *)best);
  hipLaunchKernelGGL(absorb_flag_kernel, dim3(grid_for(E)), dim3(256), 0, s, edges, E, S, (const u64 *)best, merge, n_picked);
  DM_LAUNCH_CHECK("dm_slic_absorb_pick");
  return DM_OK;
}
