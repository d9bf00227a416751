// A label raster traced into closed polygon rings and boundary arcs (gfx950).  SURVEY 8f ranks 2 and 4: the geometry the reference
// reads from shapefiles written by external GIS software (polygon layer MyUtils1.py:79-114, lines.shp MyUtils2.py:155-193).  The
// definitions are the build's own (include/deepmerge_hip.h states them, tests/vector_ref.py restates them in numpy); everything is
// an integer, so the device and the spec agree bit for bit.
//
// A dart is a unit pixel side with another label (or the outside) across it; the successor rule makes the darts a permutation
// whose cycles are the rings.  Ordering the darts along their rings is list ranking: pointer jumping, double-buffered, ceil(log2
// of the longest ring) rounds, first a 64-bit min (the ring's head) and then suffix sums (vertex rank and arc ordinal).
//   count      tile walk (dm_raster.h): 4-bit side mask per pixel, darts per tile; one looping workgroup scans the tiles
//   emit       tile walk again with a block scan over the strips: first slot per pixel, dart id per slot
//   link       per dart: label, other label, successor slot; vertex / break flag written at the successor
//   head       rounds of key[i] = min(key[i], key[jump[i]]), jump[i] = jump[jump[i]] until no key changes
//   rank       the cycle is cut in front of its head; rounds of sum[i] += sum[nxt[i]], nxt[i] = nxt[nxt[i]] until all nxt are -1
//   ring_emit  vertices at ring_ptr[ring] + vertex rank, area2 (integer atomic add per dart), the arcs' first darts and counts
//   arc_emit   vertices of the kept arcs at arc_ptr[arc] + rank inside the arc; the last dart writes the arc's end corner
// The sorts and the scans over rings and arcs between the stages are the caller's (rag._trace: torch.sort, as rag_edges).
// Every slot is written by exactly one thread; all atomics are integer adds: no result depends on the order of arrival.
// count, the scan, the successor rule and the two emit kernels live in dm_vector.h, shared with dm_scene_vector.hip.
#include "dm_vector.h"

namespace {

// ---- emit: first slot per pixel, dart id per slot ----------------------------------------------------------------------------
// Slots run in tile order, inside a tile in strip order, inside a strip by pixel and side: slot(dart) = first_slot[pixel] +
// popcount(mask & ((1 << side) - 1)).
template <bool VEC>
__global__ __launch_bounds__(256) void vec_emit_kernel(const unsigned char *__restrict__ mask, const int *__restrict__ tile_off, int H, int W,
                                                       int *__restrict__ first_slot, int *__restrict__ dart) {
  __shared__ int lds[256 / 64];
  const Strip g = strip_of(H, W);
  const int n = g.n;
  unsigned packed[STRIP / 4] = {0, 0, 0, 0};
  if (VEC && n == STRIP) {
    const u32x4 q = *reinterpret_cast<const u32x4 *>(mask + g.base);
#pragma unroll
    for (int v = 0; v < 4; ++v) packed[v] = q[v];
  } else {
#pragma unroll
    for (int i = 0; i < STRIP; ++i)
      if (i < n) packed[i >> 2] |= (unsigned)mask[g.base + i] << (8 * (i & 3));
  }
  int c = 0;
#pragma unroll
  for (int v = 0; v < 4; ++v) c += __popc(packed[v]);
  int total;
  int slot = tile_off[blockIdx.x] + block_exclusive<int, 256>(c, lds, total);
  int first[STRIP];
#pragma unroll
  for (int i = 0; i < STRIP; ++i) {
    const int m = (packed[i >> 2] >> (8 * (i & 3))) & 15;
    first[i] = slot;
    if (i < n) {
      const int id = 4 * (int)(g.base + i);
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (m >> s & 1) dart[slot++] = id + s;
    }
  }
  if (VEC && n == STRIP) {
#pragma unroll
    for (int v = 0; v < 4; ++v)
      *reinterpret_cast<i32x4 *>(first_slot + g.base + 4 * v) = (i32x4){first[4 * v], first[4 * v + 1], first[4 * v + 2], first[4 * v + 3]};
  } else {
#pragma unroll
    for (int i = 0; i < STRIP; ++i)
      if (i < n) first_slot[g.base + i] = first[i];
  }
}

// ---- link: successor, labels, flags -----------------------------------------------------------------------------------------------
__global__ void vec_link_kernel(const int *__restrict__ labels, const unsigned char *__restrict__ mask, const int *__restrict__ first_slot,
                                const int *__restrict__ dart, int H, int W, int D, int *__restrict__ next, int *__restrict__ lab,
                                int *__restrict__ other, unsigned char *__restrict__ flags, long long *__restrict__ key) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < D; i += gridDim.x * blockDim.x) {
    const int id = dart[i], pix = id >> 2, s = id & 3;
    const int y = pix / W, x = pix - y * W;
    int qx = x, qy = y;
    const int t = successor_of(mask, W, qx, qy, s);
    const int q = qy * W + qx;
    const int succ = first_slot[q] + popc4(mask[q] & ((1 << t) - 1));
    const int o = label_across(labels, H, W, x, y, s);
    next[i] = succ;
    lab[i] = labels[pix];
    other[i] = o;
    key[i] = ((long long)id << 32) | (long long)i;
    flags[succ] = (unsigned char)((t != s ? VTX : 0) | (label_across(labels, H, W, qx, qy, t) != o ? BRK : 0));
  }
}

// ---- head: the smallest dart id of every cycle ------------------------------------------------------------------------------------
__global__ void vec_head_kernel(const long long *__restrict__ key_in, const int *__restrict__ jump_in, long long *__restrict__ key_out,
                                int *__restrict__ jump_out, int D, int *__restrict__ changed) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < D; i += gridDim.x * blockDim.x) {
    const int j = jump_in[i];
    const long long a = key_in[i], b = key_in[j];
    key_out[i] = b < a ? b : a;
    jump_out[i] = jump_in[j];
    if (b < a) *changed = 1;
  }
}

// ---- rank: suffix sums of (vertex flag << 32 | break flag) along the cycle cut in front of its head -------------------------------
__global__ void vec_rank_init_kernel(const long long *__restrict__ key, const int *__restrict__ next, const unsigned char *__restrict__ flags,
                                     const int *__restrict__ lab, int D, long long *__restrict__ sum, int *__restrict__ nxt,
                                     long long *__restrict__ ring_key, int *__restrict__ ring_slot, int *__restrict__ n_rings, int max_rings) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < D; i += gridDim.x * blockDim.x) {
    const long long k = key[i];
    const int head = (int)(k & 0xffffffffLL);
    const int f = flags[i], j = next[i];
    sum[i] = ((long long)(f & VTX) << 32) | (long long)((f & BRK) >> 1);
    nxt[i] = j == head ? -1 : j;
    if (head == i) {                                             // arrival order only places the ring in a list that is sorted next
      const int pos = atomicAdd(n_rings, 1);
      if (pos < max_rings) { ring_key[pos] = ((long long)lab[i] << 32) | (k >> 32); ring_slot[pos] = i; }
    }
  }
}

__global__ void vec_rank_kernel(const long long *__restrict__ sum_in, const int *__restrict__ nxt_in, long long *__restrict__ sum_out,
                                int *__restrict__ nxt_out, int D, int *__restrict__ changed) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < D; i += gridDim.x * blockDim.x) {
    const int j = nxt_in[i];
    long long s = sum_in[i];
    int jj = -1;
    if (j >= 0) {
      s += sum_in[j];
      jj = nxt_in[j];
      if (jj >= 0) *changed = 1;
    }
    sum_out[i] = s;
    nxt_out[i] = jj;
  }
}

}  // namespace

extern "C" int dm_vector_count(const int32_t *labels, int32_t H, int32_t W, uint8_t *mask, int32_t *tile_off, int32_t *n_darts, void *stream) {
  DM_REQUIRE(labels && mask && tile_off && n_darts, DM_ERR_BAD_SHAPE, "dm_vector_count: null pointer");
  DM_REQUIRE(H > 0 && W > 0 && (long long)H * W <= (1LL << 28), DM_ERR_BAD_SHAPE, "dm_vector_count: need 1 <= H*W <= 2^28 (H=%d W=%d)", H, W);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid = tile_grid(H, W);
  const bool vec = W % STRIP == 0 && dm_aligned16(labels) && dm_aligned16(mask);
  unsigned char *none = nullptr;
  if (vec) hipLaunchKernelGGL((vec_count_kernel<true, false>), grid, dim3(256), 0, s, labels, H, W, mask, tile_off, none, 0, 0, 0, 0);
  else hipLaunchKernelGGL((vec_count_kernel<false, false>), grid, dim3(256), 0, s, labels, H, W, mask, tile_off, none, 0, 0, 0, 0);
  hipLaunchKernelGGL(vec_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, tile_off, (int)grid.x, n_darts);
  DM_LAUNCH_CHECK("dm_vector_count");
  return DM_OK;
}

extern "C" int dm_vector_emit(const uint8_t *mask, const int32_t *tile_off, int32_t H, int32_t W, int32_t *first_slot, int32_t *dart,
                              void *stream) {
  DM_REQUIRE(mask && tile_off && first_slot && dart, DM_ERR_BAD_SHAPE, "dm_vector_emit: null pointer");
  DM_REQUIRE(H > 0 && W > 0 && (long long)H * W <= (1LL << 28), DM_ERR_BAD_SHAPE, "dm_vector_emit: need 1 <= H*W <= 2^28 (H=%d W=%d)", H, W);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool vec = W % STRIP == 0 && dm_aligned16(mask) && dm_aligned16(first_slot);
  if (vec) hipLaunchKernelGGL(vec_emit_kernel<true>, tile_grid(H, W), dim3(256), 0, s, mask, tile_off, H, W, first_slot, dart);
  else hipLaunchKernelGGL(vec_emit_kernel<false>, tile_grid(H, W), dim3(256), 0, s, mask, tile_off, H, W, first_slot, dart);
  DM_LAUNCH_CHECK("dm_vector_emit");
  return DM_OK;
}

extern "C" int dm_vector_link(const int32_t *labels, const uint8_t *mask, const int32_t *first_slot, const int32_t *dart, int32_t H, int32_t W,
                              int32_t D, int32_t *next, int32_t *lab, int32_t *other, uint8_t *flags, int64_t *key, void *stream) {
  DM_REQUIRE(labels && mask && first_slot && dart && next && lab && other && flags && key, DM_ERR_BAD_SHAPE, "dm_vector_link: null pointer");
  DM_REQUIRE(H > 0 && W > 0 && (long long)H * W <= (1LL << 28) && D >= 4 && (long long)D <= 4LL * H * W, DM_ERR_BAD_SHAPE,
             "dm_vector_link: bad sizes (H=%d W=%d D=%d)", H, W, D);
  hipLaunchKernelGGL(vec_link_kernel, dim3(grid_for(D)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), labels, mask, first_slot, dart, H,
                     W, D, next, lab, other, flags, (long long *)key);
  DM_LAUNCH_CHECK("dm_vector_link");
  return DM_OK;
}

extern "C" int dm_vector_head_round(const int64_t *key_in, const int32_t *jump_in, int64_t *key_out, int32_t *jump_out, int32_t D,
                                    int32_t *changed, void *stream) {
  DM_REQUIRE(key_in && jump_in && key_out && jump_out && changed && D > 0 && key_in != key_out && jump_in != jump_out, DM_ERR_BAD_SHAPE,
             "dm_vector_head_round: bad arguments (a round reads one buffer and writes the other)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipMemsetAsync(changed, 0, sizeof(int32_t), s);
  hipLaunchKernelGGL(vec_head_kernel, dim3(grid_for(D)), dim3(256), 0, s, (const long long *)key_in, jump_in, (long long *)key_out, jump_out, D,
                     changed);
  DM_LAUNCH_CHECK("dm_vector_head_round");
  return DM_OK;
}

extern "C" int dm_vector_rank_init(const int64_t *key, const int32_t *next, const uint8_t *flags, const int32_t *lab, int32_t D, int64_t *sum,
                                   int32_t *nxt, int64_t *ring_key, int32_t *ring_slot, int32_t *n_rings, int32_t max_rings, void *stream) {
  DM_REQUIRE(key && next && flags && lab && sum && nxt && ring_key && ring_slot && n_rings && D > 0 && max_rings > 0, DM_ERR_BAD_SHAPE,
             "dm_vector_rank_init: bad arguments");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipMemsetAsync(n_rings, 0, sizeof(int32_t), s);
  hipLaunchKernelGGL(vec_rank_init_kernel, dim3(grid_for(D)), dim3(256), 0, s, (const long long *)key, next, flags, lab, D, (long long *)sum, nxt,
                     (long long *)ring_key, ring_slot, n_rings, max_rings);
  DM_LAUNCH_CHECK("dm_vector_rank_init");
  return DM_OK;
}

extern "C" int dm_vector_rank_round(const int64_t *sum_in, const int32_t *nxt_in, int64_t *sum_out, int32_t *nxt_out, int32_t D,
                                    int32_t *changed, void *stream) {
  DM_REQUIRE(sum_in && nxt_in && sum_out && nxt_out && changed && D > 0 && sum_in != sum_out && nxt_in != nxt_out, DM_ERR_BAD_SHAPE,
             "dm_vector_rank_round: bad arguments (a round reads one buffer and writes the other)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipMemsetAsync(changed, 0, sizeof(int32_t), s);
  hipLaunchKernelGGL(vec_rank_kernel, dim3(grid_for(D)), dim3(256), 0, s, (const long long *)sum_in, nxt_in, (long long *)sum_out, nxt_out, D,
                     changed);
  DM_LAUNCH_CHECK("dm_vector_rank_round");
  return DM_OK;
}

extern "C" int dm_vector_ring_emit(const DmVectorTrace *t, void *stream) {
  if (int rc = vector_trace_ok(t, "dm_vector_ring_emit", false)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vec_ring_init_kernel, dim3(grid_for(t->n_arcs)), dim3(256), 0, s, (long long *)t->area2, t->R, t->arc_count, t->n_arcs);
  hipLaunchKernelGGL((vec_ring_emit_kernel<DmVectorTrace, int, false>), dim3(grid_for(t->D)), dim3(256), 0, s, *t);
  DM_LAUNCH_CHECK("dm_vector_ring_emit");
  return DM_OK;
}

extern "C" int dm_vector_arc_emit(const DmVectorTrace *t, void *stream) {
  if (int rc = vector_trace_ok(t, "dm_vector_arc_emit", true)) return rc;
  hipLaunchKernelGGL((vec_arc_emit_kernel<DmVectorTrace, int>), dim3(grid_for(t->D)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *t);
  DM_LAUNCH_CHECK("dm_vector_arc_emit");
  return DM_OK;
}
