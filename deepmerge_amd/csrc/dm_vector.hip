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
#include "dm_raster.h"

namespace {

constexpr int BRK = 2, VTX = 1;                                // flags[slot]

__device__ __forceinline__ int popc4(int m) { return __popc((unsigned)m); }

// ---- count: side masks and darts per tile ----------------------------------------------------------------------------------
// mask bit s: the neighbour across side s (0 top, 1 right, 2 bottom, 3 left) has another label or lies outside.
template <bool VEC>
__global__ __launch_bounds__(256) void vec_count_kernel(const int *__restrict__ labels, int H, int W, unsigned char *__restrict__ mask,
                                                        int *__restrict__ tile_count) {
  __shared__ int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  const Strip g = strip_of(H, W);
  const int n = g.n;
  int lab[STRIP + 2], up[STRIP], dn[STRIP];
  load_strip<VEC>(labels, g.base, n, -2, lab + 1);              // -2 = outside the raster
  load_strip<VEC>(labels, g.base - W, n, -2, up, g.y > 0);
  load_strip<VEC>(labels, g.base + W, n, -2, dn, g.y + 1 < H);
  lab[0] = (g.live && g.x0 > 0) ? labels[g.base - 1] : -2;
  lab[STRIP + 1] = (g.live && g.x0 + STRIP < W) ? labels[g.base + STRIP] : -2;
  unsigned packed[STRIP / 4] = {0, 0, 0, 0};
  int c = 0;
#pragma unroll
  for (int i = 0; i < STRIP; ++i) {
    const int l = lab[1 + i];
    const int m = (i < n) ? ((up[i] != l) | ((lab[2 + i] != l) << 1) | ((dn[i] != l) << 2) | ((lab[i] != l) << 3)) : 0;
    c += popc4(m);
    packed[i >> 2] |= (unsigned)m << (8 * (i & 3));
  }
  if (VEC && n == STRIP) {
    *reinterpret_cast<u32x4 *>(mask + g.base) = (u32x4){packed[0], packed[1], packed[2], packed[3]};
  } else {
#pragma unroll
    for (int i = 0; i < STRIP; ++i)
      if (i < n) mask[g.base + i] = (unsigned char)(packed[i >> 2] >> (8 * (i & 3)));
  }
  if (c) atomicAdd(&total, c);
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// Exclusive scan of the tile counts in place, by one looping workgroup; counts[n_tiles] = n_out[0] = the number of darts.
__global__ __launch_bounds__(SCAN_THREADS) void vec_scan_kernel(int *__restrict__ counts, int n_tiles, int *__restrict__ n_out) {
  __shared__ int lds[SCAN_THREADS / 64];
  int carry = 0;
  for (int base = 0; base < n_tiles; base += SCAN_TILE) {
    int item[SCAN_ITEMS], sum = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      const int i = base + threadIdx.x * SCAN_ITEMS + j;
      item[j] = i < n_tiles ? counts[i] : 0;
      sum += item[j];
    }
    int total;
    int run = carry + block_exclusive(sum, lds, total);
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      const int i = base + threadIdx.x * SCAN_ITEMS + j;
      if (i < n_tiles) counts[i] = run;
      run += item[j];
    }
    carry += total;
  }
  if (threadIdx.x == 0) { counts[n_tiles] = carry; *n_out = carry; }
}

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
__device__ __forceinline__ int dir_x(int s) { return s == 0 ? 1 : (s == 2 ? -1 : 0); }
__device__ __forceinline__ int dir_y(int s) { return s == 1 ? 1 : (s == 3 ? -1 : 0); }

// Label across side s of pixel (x, y): to the dart's left; -1 outside the raster.
__device__ __forceinline__ int label_across(const int *__restrict__ labels, int H, int W, int x, int y, int s) {
  const int ax = x + dir_y(s), ay = y - dir_x(s);
  return (ax >= 0 && ax < W && ay >= 0 && ay < H) ? labels[(long long)ay * W + ax] : -1;
}

__global__ void vec_link_kernel(const int *__restrict__ labels, const unsigned char *__restrict__ mask, const int *__restrict__ first_slot,
                                const int *__restrict__ dart, int H, int W, int D, int *__restrict__ next, int *__restrict__ lab,
                                int *__restrict__ other, unsigned char *__restrict__ flags, long long *__restrict__ key) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < D; i += gridDim.x * blockDim.x) {
    const int id = dart[i], pix = id >> 2, s = id & 3;
    const int y = pix / W, x = pix - y * W;
    const int m = mask[pix];
    // the successor from the masks alone: ahead-right differs <=> this pixel has a dart on side s + 1; ahead-left differs (given
    // that ahead-right is the same label) <=> the ahead-right pixel has a dart on side s
    int qx = x, qy = y, t = (s + 1) & 3;                          // turn right
    if (!(m >> t & 1)) {
      qx = x + dir_x(s); qy = y + dir_y(s); t = s;                // straight: the ahead-right pixel is inside (it has this label)
      if (!(mask[qy * W + qx] >> s & 1)) {
        qx += dir_y(s); qy -= dir_x(s); t = (s + 3) & 3;          // turn left: the ahead-left pixel has this label as well
      }
    }
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

// ---- rings and arcs -------------------------------------------------------------------------------------------------------------
struct DartPlace {                                               // where a dart sits in its ring and its arc
  int head, ring, vertices, breaks;                              // head slot, ring index, the ring's vertex and break darts
  int vrank;                                                     // vertex darts in [head, dart)
  int binc;                                                      // break darts in [head, dart]
  int arc;                                                       // index of its arc before the arcs are sorted
  bool first;                                                    // the arc's first dart
};

__device__ __forceinline__ DartPlace place_of(const DmVectorTrace &t, int i, int f) {
  DartPlace p;
  p.head = (int)(t.key[i] & 0xffffffffLL);
  p.ring = t.ring_of_slot[p.head];
  const long long all = t.sum[p.head], mine = t.sum[i];
  p.vertices = (int)(all >> 32);
  p.breaks = (int)(all & 0xffffffffLL);
  p.vrank = p.vertices - (int)(mine >> 32);
  p.binc = p.breaks - (int)(mine & 0xffffffffLL) + ((f & BRK) >> 1);
  const int ordinal = p.breaks == 0 ? 0 : (p.binc == 0 ? p.breaks : p.binc) - 1;     // the darts in front of the first break dart
  p.arc = t.arc_base[p.ring] + ordinal;                                               // belong to the ring's last arc
  p.first = p.breaks == 0 ? i == p.head : (f & BRK) != 0;
  return p;
}

__device__ __forceinline__ void store_corner(int *__restrict__ xy, long long at, int W, int id, bool end) {
  const int pix = id >> 2, s = id & 3;
  const int y = pix / W, x = pix - y * W;
  int cx = x + (s == 1 || s == 2), cy = y + (s >= 2);             // the dart's start corner
  if (end) { cx += dir_x(s); cy += dir_y(s); }
  xy[2 * at] = cx;
  xy[2 * at + 1] = cy;
}

__global__ void vec_ring_init_kernel(long long *__restrict__ area2, int R, int *__restrict__ arc_count, int n_arcs) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < max(R, n_arcs); i += gridDim.x * blockDim.x) {
    if (i < R) area2[i] = 0;
    if (i < n_arcs) arc_count[i] = 2;                            // the first dart's start corner and the last dart's end corner
  }
}

__global__ void vec_ring_emit_kernel(DmVectorTrace t) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < t.D; i += gridDim.x * blockDim.x) {
    const int f = t.flags[i], id = t.dart[i];
    const DartPlace p = place_of(t, i, f);
    if (f & VTX) store_corner(t.xy, t.ring_ptr[p.ring] + p.vrank, t.W, id, false);
    // the shoelace term of a unit dart: -y east, +x south, +y west, -x north, at the dart's own line
    const int pix = id >> 2, s = id & 3, y = pix / t.W, x = pix - y * t.W;
    const long long term = s == 0 ? -(long long)y : s == 1 ? (long long)(x + 1) : s == 2 ? (long long)(y + 1) : -(long long)x;
    if (term) atomic_add64((long long *)t.area2 + p.ring, term);
    if (p.first) {
      t.arc_first[p.arc] = id;
      t.arc_right[p.arc] = t.lab[i];
      t.arc_left[p.arc] = t.other[i];
      t.arc_vstart[p.arc] = p.vrank + (f & VTX);                 // vertex darts in [head, first dart]
    } else if (f & VTX) {
      atomicAdd(t.arc_count + p.arc, 1);
    }
  }
}

__global__ void vec_arc_emit_kernel(DmVectorTrace t) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < t.D; i += gridDim.x * blockDim.x) {
    const int f = t.flags[i], id = t.dart[i];
    const DartPlace p = place_of(t, i, f);
    const int pos = t.arc_pos[p.arc];
    if (pos < 0) continue;                                       // the arc is kept from its other side
    const long long base = t.arc_ptr[pos];
    if (p.first) {
      store_corner(t.arc_xy, base, t.W, id, false);
    } else if (f & VTX) {
      const int start = t.arc_vstart[p.arc];
      const bool wrapped = p.breaks != 0 && p.binc == 0;         // in front of the ring's first break dart: the arc began behind
      store_corner(t.arc_xy, base + 1 + (wrapped ? p.vertices - start + p.vrank : p.vrank - start), t.W, id, false);
    }
    const int j = t.next[i];
    if (p.breaks == 0 ? j == p.head : (t.flags[j] & BRK) != 0) store_corner(t.arc_xy, t.arc_ptr[pos + 1] - 1, t.W, id, true);
  }
}

}  // namespace

extern "C" int dm_vector_count(const int32_t *labels, int32_t H, int32_t W, uint8_t *mask, int32_t *tile_off, int32_t *n_darts, void *stream) {
  DM_REQUIRE(labels && mask && tile_off && n_darts, DM_ERR_BAD_SHAPE, "dm_vector_count: null pointer");
  DM_REQUIRE(H > 0 && W > 0 && (long long)H * W <= (1LL << 28), DM_ERR_BAD_SHAPE, "dm_vector_count: need 1 <= H*W <= 2^28 (H=%d W=%d)", H, W);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid = tile_grid(H, W);
  const bool vec = W % STRIP == 0 && dm_aligned16(labels) && dm_aligned16(mask);
  if (vec) hipLaunchKernelGGL(vec_count_kernel<true>, grid, dim3(256), 0, s, labels, H, W, mask, tile_off);
  else hipLaunchKernelGGL(vec_count_kernel<false>, grid, dim3(256), 0, s, labels, H, W, mask, tile_off);
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

static int vector_trace_ok(const DmVectorTrace *t, const char *what, bool arcs) {
  DM_REQUIRE(t && t->dart && t->next && t->lab && t->other && t->flags && t->key && t->sum && t->ring_of_slot && t->arc_base && t->arc_vstart,
             DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  DM_REQUIRE(t->W > 0 && t->D >= 4 && t->R >= 1 && t->n_arcs >= t->R, DM_ERR_BAD_SHAPE, "%s: bad sizes (W=%d D=%d R=%d n_arcs=%d)", what, t->W,
             t->D, t->R, t->n_arcs);
  if (arcs) DM_REQUIRE(t->arc_pos && t->arc_ptr && t->arc_xy, DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  else DM_REQUIRE(t->ring_ptr && t->xy && t->area2 && t->arc_first && t->arc_left && t->arc_right && t->arc_count, DM_ERR_BAD_SHAPE,
                  "%s: null pointer", what);
  return DM_OK;
}

extern "C" int dm_vector_ring_emit(const DmVectorTrace *t, void *stream) {
  if (int rc = vector_trace_ok(t, "dm_vector_ring_emit", false)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vec_ring_init_kernel, dim3(grid_for(t->n_arcs)), dim3(256), 0, s, (long long *)t->area2, t->R, t->arc_count, t->n_arcs);
  hipLaunchKernelGGL(vec_ring_emit_kernel, dim3(grid_for(t->D)), dim3(256), 0, s, *t);
  DM_LAUNCH_CHECK("dm_vector_ring_emit");
  return DM_OK;
}

extern "C" int dm_vector_arc_emit(const DmVectorTrace *t, void *stream) {
  if (int rc = vector_trace_ok(t, "dm_vector_arc_emit", true)) return rc;
  hipLaunchKernelGGL(vec_arc_emit_kernel, dim3(grid_for(t->D)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *t);
  DM_LAUNCH_CHECK("dm_vector_arc_emit");
  return DM_OK;
}
