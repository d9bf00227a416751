// What the passes over a label raster share (dm_rag.hip, dm_truth.hip, dm_points.hip, dm_merge.hip, dm_vector.hip), each piece once:
//   - the tile walk: a workgroup of 256 threads owns a 64x64-pixel tile, a thread a 16-pixel strip of one row (Strip, load_strip);
//   - the tile's LDS tables: 64-bit keys with counts in front of the global table (TileTable), label -> slot (claim_label_slot),
//     bounding boxes (box_init / box_fold, on LDS and on global boxes alike);
//   - the global open-addressing table of 64-bit keys with int32 counts and its clear / tile kernel / compact sequence (run_tile_table);
//   - the exclusive scan over one looping workgroup (block_exclusive).
// A new raster pass writes what is particular to it: the work per strip and what is flushed per tile.
// All of it is integer work on integer atomics: no result depends on the order in which threads arrive.
#pragma once
#include <climits>

#include "dm_common.h"

namespace {

typedef unsigned long long u64;

inline int grid_for(long long items, int cap = 2048) {
  long long g = (items + 255) / 256;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

__device__ __forceinline__ void atomic_add64(long long *p, long long v) { atomicAdd(reinterpret_cast<u64 *>(p), (u64)v); }

// ---- tile walk -------------------------------------------------------------------------------------------------------------
constexpr int STRIP = 16;

// This thread's strip: pixels x0 .. x0 + n - 1 of row y, the first at linear index `base`.  A strip outside the raster is not
// `live`: n == 0, and base stays inside the raster.
struct Strip {
  int y, x0, n;
  bool live;
  long long base;
};

__device__ __forceinline__ Strip strip_of(int H, int W) {
  const int tiles_x = (W + 63) / 64;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  Strip g;
  g.y = ty * 64 + (threadIdx.x >> 2);
  g.x0 = tx * 64 + (threadIdx.x & 3) * STRIP;
  g.live = g.y < H && g.x0 < W;
  g.n = g.live ? min(STRIP, W - g.x0) : 0;
  g.base = (long long)(g.live ? g.y : 0) * W + (g.live ? g.x0 : 0);
  return g;
}

inline dim3 tile_grid(int H, int W) { return dim3((unsigned)(((W + 63) / 64) * ((H + 63) / 64))); }     // one workgroup per tile

// out[0 .. STRIP) = p[base .. base + n), `fill` behind the strip's end; all `fill` when the row does not exist (the rows above
// the first and below the last).  VEC: four 16-byte loads for a whole strip, which needs W % STRIP == 0 and p 16-byte aligned.
template <bool VEC>
__device__ __forceinline__ void load_strip(const int *__restrict__ p, long long base, int n, int fill, int *out, bool row_exists = true) {
  if (VEC && n == STRIP) {
#pragma unroll
    for (int v = 0; v < STRIP / 4; ++v) {
      const i32x4 a = row_exists ? *reinterpret_cast<const i32x4 *>(p + base + 4 * v) : (i32x4){fill, fill, fill, fill};
#pragma unroll
      for (int e = 0; e < 4; ++e) out[4 * v + e] = a[e];
    }
  } else {
#pragma unroll
    for (int i = 0; i < STRIP; ++i) out[i] = (row_exists && i < n) ? p[base + i] : fill;
  }
}

// ---- global table of 64-bit keys with int32 counts -------------------------------------------------------------------------------
// Open addressing in global memory, filled with integer atomics (dm_rag.hip: label pairs, dm_truth.hip: (label, truth) cells).
// Keys are >= 0; a slot is claimed with one 64-bit CAS and counted with one 32-bit add.
constexpr long long EMPTY_KEY = -1;

__device__ __forceinline__ u64 mix64(u64 k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
  return k;
}
__device__ __forceinline__ void table_add(long long *keys, int *cnt, unsigned mask, long long key, int c, int *overflow) {
  unsigned slot = (unsigned)mix64((u64)key) & mask;
  for (unsigned probe = 0; probe <= mask; ++probe) {
    const long long seen = (long long)atomicCAS(reinterpret_cast<u64 *>(keys + slot), (u64)EMPTY_KEY, (u64)key);
    if (seen == EMPTY_KEY || seen == key) {
      atomicAdd(cnt + slot, c);
      return;
    }
    slot = (slot + 1) & mask;
    if (probe > 4096) break;
  }
  atomicExch(overflow, 1);
}

__global__ void table_clear_kernel(long long *keys, int *cnt, long long n, int *overflow, int *n_out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    keys[i] = EMPTY_KEY;
    cnt[i] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { *overflow = 0; *n_out = 0; }
}

__global__ void table_compact_kernel(const long long *__restrict__ keys, const int *__restrict__ cnt, long long n,
                                     long long *__restrict__ out_keys, int *__restrict__ out_cnt, int *__restrict__ n_out, int max_out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long k = keys[i];
    if (k == EMPTY_KEY) continue;
    const int pos = atomicAdd(n_out, 1);
    if (pos < max_out) { out_keys[pos] = k; out_cnt[pos] = cnt[i]; }
  }
}

// The tile's LDS-private table in front of the global one (a __shared__ object): keys are first counted here with integer LDS
// atomics, and every distinct key of the tile then costs ONE add into the global table.  A key that finds the tile's table
// full goes straight to the global table.
template <int SLOTS_LOG2>
struct TileTable {
  static constexpr int SLOTS = 1 << SLOTS_LOG2;
  long long key[SLOTS];
  int cnt[SLOTS];

  __device__ __forceinline__ void clear() {                    // by the whole workgroup, which is synchronised on return
    for (int i = threadIdx.x; i < SLOTS; i += blockDim.x) { key[i] = EMPTY_KEY; cnt[i] = 0; }
    __syncthreads();
  }
  __device__ __forceinline__ void add(long long k, int c, long long *keys, int *counts, unsigned mask, int *overflow) {
    unsigned slot = (unsigned)mix64((u64)k) & (SLOTS - 1);
    for (int probe = 0; probe < SLOTS; ++probe) {
      const long long seen = (long long)atomicCAS(reinterpret_cast<u64 *>(&key[slot]), (u64)EMPTY_KEY, (u64)k);
      if (seen == EMPTY_KEY || seen == k) { atomicAdd(&cnt[slot], c); return; }
      slot = (slot + 1) & (SLOTS - 1);
    }
    table_add(keys, counts, mask, k, c, overflow);
  }
  __device__ __forceinline__ void flush(long long *keys, int *counts, unsigned mask, int *overflow) {      // after every add of the workgroup
    __syncthreads();
    for (int i = threadIdx.x; i < SLOTS; i += blockDim.x)
      if (key[i] != EMPTY_KEY) table_add(keys, counts, mask, key[i], cnt[i], overflow);
  }
};

// Host: clear the global table, run the tile kernel (its 16-byte-load or its scalar instantiation; the kernel's own arguments
// come first, the table's keys, counts, mask and overflow flag last), compact the table's entries to the front of out_*.
template <typename Kernel, typename... Args>
inline void run_tile_table(Kernel vec_kernel, Kernel scalar_kernel, bool vec, hipStream_t s, int H, int W, int64_t *table_keys,
                           int32_t *table_counts, int capacity_log2, int64_t *out_keys, int32_t *out_counts, int max_out, int32_t *n_out,
                           int32_t *overflow, Args... args) {
  const long long cap = 1LL << capacity_log2;
  hipLaunchKernelGGL(table_clear_kernel, dim3(grid_for(cap)), dim3(256), 0, s, (long long *)table_keys, table_counts, cap, overflow, n_out);
  hipLaunchKernelGGL(vec ? vec_kernel : scalar_kernel, tile_grid(H, W), dim3(256), 0, s, args..., (long long *)table_keys, table_counts,
                     (unsigned)(cap - 1), overflow);
  hipLaunchKernelGGL(table_compact_kernel, dim3(grid_for(cap)), dim3(256), 0, s, (const long long *)table_keys, table_counts, cap,
                     (long long *)out_keys, out_counts, n_out, max_out);
}

// ---- per-label LDS tables ----------------------------------------------------------------------------------------------------
// Slot of label l in the tile's table t_key[1 << SLOTS_LOG2] (open addressing, -1 = free); -1 when the table is full: that
// label goes to global memory.
template <int SLOTS_LOG2>
__device__ __forceinline__ int claim_label_slot(int *t_key, int l) {
  constexpr int SLOTS = 1 << SLOTS_LOG2;
  unsigned slot = ((unsigned)l * 2654435761u) >> (32 - SLOTS_LOG2);
  for (int probe = 0; probe < SLOTS; ++probe) {
    const int seen = atomicCAS(&t_key[slot], -1, l);
    if (seen == -1 || seen == l) return (int)slot;
    slot = (slot + 1) & (SLOTS - 1);
  }
  return -1;
}

// Bounding box xmin, ymin, xmax, ymax; the empty box folds to whatever it meets first.
__device__ __forceinline__ void box_init(int *box) { box[0] = INT_MAX; box[1] = INT_MAX; box[2] = -1; box[3] = -1; }
__device__ __forceinline__ void box_fold(int *box, int xmin, int ymin, int xmax, int ymax) {
  atomicMin(box + 0, xmin); atomicMin(box + 1, ymin);
  atomicMax(box + 2, xmax); atomicMax(box + 3, ymax);
}

// ---- exclusive scan by one looping workgroup ---------------------------------------------------------------------------------------
// The workgroup walks its items in tiles of SCAN_TILE: SCAN_ITEMS consecutive items per thread, summed, then block_exclusive.
constexpr int SCAN_THREADS = 1024, SCAN_ITEMS = 4, SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

__device__ __forceinline__ int shfl_up(int v, int o) { return __shfl_up(v, o, 64); }

// Exclusive prefix of `v` over the workgroup's THREADS threads (thread order) and the workgroup total.  T: int, or a struct
// of ints with +, - and shfl_up.  lds: THREADS / 64 entries; the first barrier lets the previous tile's readers finish.
// THREADS = 256 scans the strips of a tile inside a tile kernel (dm_vector.hip).
template <typename T, int THREADS = SCAN_THREADS>
__device__ __forceinline__ T block_exclusive(T v, T *lds, T &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T up = shfl_up(inc, o);
    if (lane >= o) inc = inc + up;
  }
  __syncthreads();
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  T before{}, all{};
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    const T t = lds[w];
    if (w < wave) before = before + t;
    all = all + t;
  }
  total = all;
  return before + inc - v;
}

}  // namespace
