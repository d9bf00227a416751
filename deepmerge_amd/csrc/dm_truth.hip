// Overlap (contingency) table of a label raster against a ground-truth raster, the facts derived from it and the pair flags
// (gfx950).  The reference trains from `positive` / `negative` polygon-pair lists that somebody produced outside the program by
// comparing the over-segmentation with a ground-truth map (GenerateTrainPairData.py only counts their lines), and has nothing
// that scores a partition against a reference map.  Both need the sparse table n[s,g] = #{pixels: labels == s, truth == g}.
// The rule is the build's own: stated in include/deepmerge_hip.h, restated in numpy in tests/truth_ref.py.
//
// Every quantity is an integer and every reduction an integer add / max, so the result does not depend on the order in which
// threads arrive: the GPU and the numpy spec agree bit for bit.  No floating point anywhere in this file.
//
// dm_label_overlap is a pass on dm_raster.h's tile walk over BOTH rasters (64 B of labels + 64 B of truth per strip), run-length
// merged; the tile's cells are counted in its TileTable and from there in the global table.
#include "dm_raster.h"

namespace {

constexpr int CSLOTS_LOG2 = 7;                                 // 128 cells per 64x64 tile kept in LDS (more: global table directly)

template <bool VEC>
__global__ __launch_bounds__(256) void label_overlap_kernel(const int *__restrict__ labels, const int *__restrict__ truth, int H, int W, long long S,
                                                            long long G, long long *__restrict__ keys, int *__restrict__ cnt, unsigned mask,
                                                            int *__restrict__ overflow) {
  __shared__ TileTable<CSLOTS_LOG2> cells;
  cells.clear();
  {
    const Strip g = strip_of(H, W);
    const int n = g.n;
    int lab[STRIP], tru[STRIP];
    load_strip<VEC>(labels, g.base, n, -1, lab);
    load_strip<VEC>(truth, g.base, n, -1, tru);
    const long long cols = G + 1;
    long long run_key = EMPTY_KEY;
    int run_cnt = 0;
#pragma unroll
    for (int i = 0; i < STRIP; ++i) {
      if (i >= n) break;
      const int l = lab[i], t = tru[i];
      // ids outside [0,S) are ignored; any truth value outside [0,G) is the "unlabelled" column G
      const long long key = (l >= 0 && l < S) ? (long long)l * cols + ((t >= 0 && t < G) ? (long long)t : G) : EMPTY_KEY;
      if (key == run_key) { ++run_cnt; continue; }
      if (run_key != EMPTY_KEY) cells.add(run_key, run_cnt, keys, cnt, mask, overflow);
      run_key = key; run_cnt = 1;
    }
    if (run_key != EMPTY_KEY) cells.add(run_key, run_cnt, keys, cnt, mask, overflow);
  }
  cells.flush(keys, cnt, mask, overflow);
}

// ---- row / column facts and the summary from the compacted cells -----------------------------------------------------------
__global__ void reduce_init_kernel(u64 *__restrict__ row_best, long long *__restrict__ row_labelled, long long *__restrict__ area,
                                   long long *__restrict__ size, int *__restrict__ cover, long long *__restrict__ summary, long long S, long long G) {
  const long long rows = max(max(S, G), 8LL);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (long long)gridDim.x * blockDim.x) {
    if (i < S) { row_best[i] = 0; row_labelled[i] = 0; area[i] = 0; }
    if (i < G) { size[i] = 0; cover[i] = 0; }
    if (i < 8) summary[i] = 0;
  }
}

// Sum over the wave, then one atomic per wave (lane 0).
__device__ __forceinline__ void wave_add64(long long *p, long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0 && v) atomic_add64(p, v);
}

__global__ __launch_bounds__(256) void overlap_cells_kernel(const long long *__restrict__ keys, const int *__restrict__ counts, int K, long long S, long long G,
                                                            u64 *__restrict__ row_best, long long *__restrict__ row_labelled,
                                                            long long *__restrict__ area, long long *__restrict__ size, int *__restrict__ cover,
                                                            long long *__restrict__ summary) {
  const long long cols = G + 1;
  long long n = 0, sq = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < K; i += (long long)gridDim.x * blockDim.x) {
    const long long key = keys[i];
    const long long c = counts[i];
    if (key < 0 || c <= 0) continue;
    const long long s = key / cols;
    const long long g = key - s * cols;
    if (s >= S) continue;
    atomic_add64(area + s, c);
    if (g < G) {
      atomic_add64(row_labelled + s, c);
      atomicMax(row_best + s, ((u64)c << 32) | (u64)(0xFFFFFFFFu - (unsigned)g));
      atomic_add64(size + g, c);
      atomicMax(cover + g, (int)c);
      n += c; sq += c * c;
    }
  }
  wave_add64(summary + 0, n);
  wave_add64(summary + 1, sq);
}

__global__ __launch_bounds__(256) void overlap_finish_kernel(const u64 *__restrict__ row_best, const long long *__restrict__ row_labelled,
                                                             const long long *__restrict__ size, const int *__restrict__ cover, long long S,
                                                             long long G, int *__restrict__ owner, int *__restrict__ owner_count,
                                                             long long *__restrict__ summary) {
  long long r2 = 0, z2 = 0, oc = 0, cv = 0, rows = 0, colsn = 0;
  const long long items = max(S, G);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (long long)gridDim.x * blockDim.x) {
    if (i < S) {
      const u64 b = row_best[i];
      const int c = (int)(b >> 32);
      owner[i] = b ? (int)(0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFULL)) : -1;
      owner_count[i] = c;
      const long long r = row_labelled[i];
      r2 += r * r; oc += c; rows += r > 0;
    }
    if (i < G) {
      const long long z = size[i];
      z2 += z * z; cv += cover[i]; colsn += z > 0;
    }
  }
  wave_add64(summary + 2, r2);
  wave_add64(summary + 3, z2);
  wave_add64(summary + 4, oc);
  wave_add64(summary + 5, cv);
  wave_add64(summary + 6, rows);
  wave_add64(summary + 7, colsn);
}

__global__ void pair_flags_kernel(const int *__restrict__ edges, int E, const long long *__restrict__ area, const int *__restrict__ owner,
                                  const int *__restrict__ owner_count, int S, int purity_pm, signed char *__restrict__ flags) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (long long)gridDim.x * blockDim.x) {
    const int a = edges[2 * e], b = edges[2 * e + 1];
    signed char f = -1;
    if ((unsigned)a < (unsigned)S && (unsigned)b < (unsigned)S) {
      const int oa = owner[a], ob = owner[b];
      const bool pa = oa >= 0 && 1000LL * owner_count[a] >= (long long)purity_pm * area[a];
      const bool pb = ob >= 0 && 1000LL * owner_count[b] >= (long long)purity_pm * area[b];
      if (pa && pb) f = oa == ob ? 1 : 0;
    }
    flags[e] = f;
  }
}

inline bool key_bound_ok(long long S, long long G) { return S <= ((1LL << 62) - 1) / (G + 1); }     // S (G + 1) < 2^62, no overflow

}  // namespace

extern "C" int dm_label_overlap(const int32_t *labels, const int32_t *truth, int32_t H, int32_t W, int64_t S, int64_t G, int64_t *table_keys,
                                int32_t *table_counts, int32_t capacity_log2, int64_t *cell_keys, int32_t *cell_counts, int32_t max_cells,
                                int32_t *n_cells, int32_t *overflow, void *stream) {
  DM_REQUIRE(labels && truth && table_keys && table_counts && cell_keys && cell_counts && n_cells && overflow, DM_ERR_BAD_SHAPE,
             "dm_label_overlap: null pointer");
  DM_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1LL << 31) && S > 0 && G > 0 && G < (1LL << 31) && capacity_log2 >= 8 && capacity_log2 <= 30 &&
                 max_cells > 0,
             DM_ERR_BAD_SHAPE, "dm_label_overlap: bad sizes (H=%d W=%d S=%lld G=%lld capacity_log2=%d max_cells=%d; need H*W < 2^31, G < 2^31)", H, W,
             (long long)S, (long long)G, capacity_log2, max_cells);
  DM_REQUIRE(key_bound_ok(S, G), DM_ERR_BAD_SHAPE, "dm_label_overlap: key bound exceeded (S=%lld G=%lld; need S*(G+1) < 2^62)", (long long)S,
             (long long)G);
  // 16-byte strip loads need W % 16 == 0 and 16-byte aligned rasters
  const bool vec = W % STRIP == 0 && dm_aligned16(labels) && dm_aligned16(truth);
  run_tile_table(label_overlap_kernel<true>, label_overlap_kernel<false>, vec, reinterpret_cast<hipStream_t>(stream), H, W, table_keys, table_counts,
                 capacity_log2, cell_keys, cell_counts, max_cells, n_cells, overflow, labels, truth, H, W, (long long)S, (long long)G);
  DM_LAUNCH_CHECK("dm_label_overlap");
  return DM_OK;
}

extern "C" int dm_overlap_reduce(const int64_t *cell_keys, const int32_t *cell_counts, int32_t K, int64_t S, int64_t G, uint64_t *row_best,
                                 int64_t *row_labelled, int64_t *area, int32_t *owner, int32_t *owner_count, int64_t *size, int32_t *cover,
                                 int64_t *summary, void *stream) {
  DM_REQUIRE(row_best && row_labelled && area && owner && owner_count && size && cover && summary && (K == 0 || (cell_keys && cell_counts)),
             DM_ERR_BAD_SHAPE, "dm_overlap_reduce: null pointer");
  DM_REQUIRE(K >= 0 && S > 0 && G > 0 && G < (1LL << 31), DM_ERR_BAD_SHAPE, "dm_overlap_reduce: bad sizes (K=%d S=%lld G=%lld; need G < 2^31)", K,
             (long long)S, (long long)G);
  DM_REQUIRE(key_bound_ok(S, G), DM_ERR_BAD_SHAPE, "dm_overlap_reduce: key bound exceeded (S=%lld G=%lld; need S*(G+1) < 2^62)", (long long)S,
             (long long)G);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 rgrid(grid_for(S > G ? S : G));
  hipLaunchKernelGGL(reduce_init_kernel, rgrid, dim3(256), 0, s, (u64 *)row_best, (long long *)row_labelled, (long long *)area, (long long *)size,
                     cover, (long long *)summary, (long long)S, (long long)G);
  if (K > 0)
    hipLaunchKernelGGL(overlap_cells_kernel, dim3(grid_for(K)), dim3(256), 0, s, (const long long *)cell_keys, cell_counts, K, (long long)S, (long long)G,
                       (u64 *)row_best, (long long *)row_labelled, (long long *)area, (long long *)size, cover, (long long *)summary);
  hipLaunchKernelGGL(overlap_finish_kernel, rgrid, dim3(256), 0, s, (const u64 *)row_best, (const long long *)row_labelled, (const long long *)size,
                     cover, (long long)S, (long long)G, owner, owner_count, (long long *)summary);
  DM_LAUNCH_CHECK("dm_overlap_reduce");
  return DM_OK;
}

extern "C" int dm_pair_flags(const int32_t *edges, int32_t E, const int64_t *area, const int32_t *owner, const int32_t *owner_count, int32_t S,
                             int32_t purity_pm, int8_t *flags, void *stream) {
  DM_REQUIRE(area && owner && owner_count && (E == 0 || (edges && flags)), DM_ERR_BAD_SHAPE, "dm_pair_flags: null pointer");
  DM_REQUIRE(E >= 0 && S > 0, DM_ERR_BAD_SHAPE, "dm_pair_flags: bad sizes (E=%d S=%d)", E, S);
  DM_REQUIRE(purity_pm >= 0 && purity_pm <= 1000, DM_ERR_BAD_SHAPE, "dm_pair_flags: purity_pm = %d outside 0..1000", purity_pm);
  if (E == 0) return DM_OK;
  hipLaunchKernelGGL(pair_flags_kernel, dim3(grid_for(E)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), edges, E,
                     (const long long *)area, owner, owner_count, S, purity_pm, (signed char *)flags);
  DM_LAUNCH_CHECK("dm_pair_flags");
  return DM_OK;
}
