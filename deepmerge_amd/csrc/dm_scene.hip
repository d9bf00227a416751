// Seam stitch: what lies between the tiles of a scene that is segmented tile by tile (gfx950).  DESIGN.md 3.5.9.
// The per-tile passes (dm_rag.hip) see one tile's raster: they miss the RAG edges whose two pixels lie in different tiles, and
// they count a tile's outer pixel edges as "on the raster border" although, inside the scene, another label faces them.  This
// pass walks the seam positions of the whole scene once -- a[i] / b[i] = the scene-wide ids of the two pixels that face each
// other across position i -- and (1) counts the label pairs through dm_raster.h's table, key and overflow report, exactly as
// rag_edges_kernel does for the pairs inside a raster, (2) moves every seam pixel edge in `peri` from the border column to the
// column dm_label_stats would have put it in had it seen the facing pixel.
// Integer adds only: no result depends on the order in which threads arrive.
#include "dm_raster.h"

namespace {

// A thread takes SEAM_STRIP consecutive positions (one 16-byte load per side), a workgroup 1024 per step; its LDS table has a slot
// per position of a step, so a step cannot fill it (a position adds at most one distinct pair), whatever the size of the
// superpixels.  (A full table costs every later add a walk over all its slots before it goes to the global table.)
constexpr int SEAM_STRIP = 4;
constexpr int SEAM_BLOCK = 256 * SEAM_STRIP;                     // positions per workgroup and step
constexpr int SEAM_SLOTS_LOG2 = 10;                              // = log2(SEAM_BLOCK)

__device__ __forceinline__ void load_seam(const int *__restrict__ p, long long base, int m, bool vec, int *out) {
  if (vec && m == SEAM_STRIP) {
    const i32x4 q = *reinterpret_cast<const i32x4 *>(p + base);
#pragma unroll
    for (int e = 0; e < SEAM_STRIP; ++e) out[e] = q[e];
  } else {
#pragma unroll
    for (int e = 0; e < SEAM_STRIP; ++e) out[e] = e < m ? p[base + e] : -2;
  }
}

// One side's perimeter moves, run-length merged: a seam run repeats the same id for about a cell's length.
struct PeriRun {
  int id = -1;
  long long inner = 0, border = 0;
  __device__ __forceinline__ void flush(long long *peri) {
    if (id >= 0) {
      if (inner) atomic_add64(peri + 2 * (long long)id, inner);
      if (border) atomic_add64(peri + 2 * (long long)id + 1, -border);
    }
  }
  // the pixel edge of `l` that faces `f`: dm_label_stats' rule for a neighbour inside the raster (-2 is its "outside" marker)
  __device__ __forceinline__ void face(int l, int f, int S, long long *peri) {
    if (l < 0 || l >= S || f == -2) return;
    if (l != id) { flush(peri); id = l; inner = 0; border = 0; }
    ++border;                                                    // the tile counted it as raster border
    if (f != l) ++inner;                                         // in the scene it faces another label
  }
};

__global__ __launch_bounds__(256) void seam_stitch_kernel(const int *__restrict__ a, const int *__restrict__ b, long long n, int S, bool vec,
                                                          long long *__restrict__ peri, long long *__restrict__ keys, int *__restrict__ cnt,
                                                          unsigned mask, int *__restrict__ overflow) {
  __shared__ TileTable<SEAM_SLOTS_LOG2> pairs;                   // the workgroup's pairs, each added to the global table once
  pairs.clear();
  long long run_key = EMPTY_KEY;
  int run_cnt = 0;
  PeriRun pa, pb;
  for (long long base = (long long)blockIdx.x * SEAM_BLOCK + (long long)threadIdx.x * SEAM_STRIP; base < n;
       base += (long long)gridDim.x * SEAM_BLOCK) {
    const int m = (int)min((long long)SEAM_STRIP, n - base);
    int la[SEAM_STRIP], lb[SEAM_STRIP];
    load_seam(a, base, m, vec, la);
    load_seam(b, base, m, vec, lb);
#pragma unroll
    for (int i = 0; i < SEAM_STRIP; ++i) {
      if (i >= m) break;
      const int x = la[i], y = lb[i];
      pa.face(x, y, S, peri);
      pb.face(y, x, S, peri);
      if (x == y || x < 0 || y < 0 || x >= S || y >= S) continue;
      const long long key = (long long)min(x, y) * S + max(x, y);
      if (key == run_key) { ++run_cnt; continue; }
      if (run_cnt) pairs.add(run_key, run_cnt, keys, cnt, mask, overflow);
      run_key = key; run_cnt = 1;
    }
  }
  if (run_cnt) pairs.add(run_key, run_cnt, keys, cnt, mask, overflow);
  pa.flush(peri);
  pb.flush(peri);
  pairs.flush(keys, cnt, mask, overflow);
}

}  // namespace

extern "C" int dm_seam_stitch(const int32_t *a, const int32_t *b, int64_t n, int64_t S, int64_t *peri, int64_t *table_keys,
                              int32_t *table_counts, int32_t capacity_log2, int64_t *edge_keys, int32_t *edge_counts, int32_t max_edges,
                              int32_t *n_edges, int32_t *overflow, void *stream) {
  DM_REQUIRE(a && b && peri && table_keys && table_counts && edge_keys && edge_counts && n_edges && overflow, DM_ERR_BAD_SHAPE,
             "dm_seam_stitch: null pointer");
  DM_REQUIRE(n >= 1 && S >= 1 && S <= (1LL << 24) && capacity_log2 >= 8 && capacity_log2 <= 30 && max_edges > 0, DM_ERR_BAD_SHAPE,
             "dm_seam_stitch: bad sizes (n=%lld S=%lld capacity_log2=%d max_edges=%d)", (long long)n, (long long)S, capacity_log2, max_edges);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long cap = 1LL << capacity_log2;
  const long long blocks = (n + SEAM_BLOCK - 1) / SEAM_BLOCK;
  hipLaunchKernelGGL(table_clear_kernel, dim3(grid_for(cap)), dim3(256), 0, s, (long long *)table_keys, table_counts, cap, overflow, n_edges);
  hipLaunchKernelGGL(seam_stitch_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, s, a, b, (long long)n, (int)S,
                     dm_aligned16(a) && dm_aligned16(b), (long long *)peri, (long long *)table_keys, table_counts, (unsigned)(cap - 1), overflow);
  hipLaunchKernelGGL(table_compact_kernel, dim3(grid_for(cap)), dim3(256), 0, s, (const long long *)table_keys, table_counts, cap,
                     (long long *)edge_keys, edge_counts, n_edges, max_edges);
  DM_LAUNCH_CHECK("dm_seam_stitch");
  return DM_OK;
}
