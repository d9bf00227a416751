// What the two tracers share (dm_vector.hip: one raster; dm_scene_vector.hip: a scene's raster tile by tile), each
// piece once: the side masks and darts per tile, the scan of the tiles, the successor's geometry, a dart's place in its ring and
// arc, and the two emit kernels.  The emit kernels are templates over the argument struct: DmVectorTrace keeps 32-bit dart ids and
// a 32-bit W, DmSceneVectorTrace 64-bit ones; the arithmetic on a 32-bit id is the one dm_vector.hip always had.
#pragma once
#include "dm_raster.h"

namespace {

constexpr int BRK = 2, VTX = 1;                                // flags[slot]

__device__ __forceinline__ int popc4(int m) { return __popc((unsigned)m); }

// ---- count: side masks and darts per tile ----------------------------------------------------------------------------------
// mask bit s: the neighbour across side s (0 top, 1 right, 2 bottom, 3 left) has another label or lies outside.
// CORE: the raster is a scene tile's window; core_mask is the mask inside the box [cy0, cy1) x [cx0, cx1) and 0 outside it, and
// only the box's darts are counted (the apron's pixels own no dart of this tile).
template <bool VEC, bool CORE>
__global__ __launch_bounds__(256) void vec_count_kernel(const int *__restrict__ labels, int H, int W, unsigned char *__restrict__ mask,
                                                        int *__restrict__ tile_count, unsigned char *__restrict__ core_mask, int cy0, int cy1,
                                                        int cx0, int cx1) {
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
  unsigned packed[STRIP / 4] = {0, 0, 0, 0}, inner[STRIP / 4] = {0, 0, 0, 0};
  const bool row_in = CORE && g.y >= cy0 && g.y < cy1;
  int c = 0;
#pragma unroll
  for (int i = 0; i < STRIP; ++i) {
    const int l = lab[1 + i];
    const int m = (i < n) ? ((up[i] != l) | ((lab[2 + i] != l) << 1) | ((dn[i] != l) << 2) | ((lab[i] != l) << 3)) : 0;
    packed[i >> 2] |= (unsigned)m << (8 * (i & 3));
    if (CORE) {
      const int mc = (row_in && g.x0 + i >= cx0 && g.x0 + i < cx1) ? m : 0;
      c += popc4(mc);
      inner[i >> 2] |= (unsigned)mc << (8 * (i & 3));
    } else {
      c += popc4(m);
    }
  }
  if (VEC && n == STRIP) {
    *reinterpret_cast<u32x4 *>(mask + g.base) = (u32x4){packed[0], packed[1], packed[2], packed[3]};
    if (CORE) *reinterpret_cast<u32x4 *>(core_mask + g.base) = (u32x4){inner[0], inner[1], inner[2], inner[3]};
  } else {
#pragma unroll
    for (int i = 0; i < STRIP; ++i)
      if (i < n) {
        mask[g.base + i] = (unsigned char)(packed[i >> 2] >> (8 * (i & 3)));
        if (CORE) core_mask[g.base + i] = (unsigned char)(inner[i >> 2] >> (8 * (i & 3)));
      }
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

// ---- the successor's geometry ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int dir_x(int s) { return s == 0 ? 1 : (s == 2 ? -1 : 0); }
__device__ __forceinline__ int dir_y(int s) { return s == 1 ? 1 : (s == 3 ? -1 : 0); }

// Label across side s of pixel (x, y): to the dart's left; -1 outside the raster.
__device__ __forceinline__ int label_across(const int *__restrict__ labels, int H, int W, int x, int y, int s) {
  const int ax = x + dir_y(s), ay = y - dir_x(s);
  return (ax >= 0 && ax < W && ay >= 0 && ay < H) ? labels[(long long)ay * W + ax] : -1;
}

// The successor of the dart on side s of pixel (x, y) from the masks alone: ahead-right differs <=> this pixel has a dart on side
// s + 1; ahead-left differs (given that ahead-right is the same label) <=> the ahead-right pixel has a dart on side s.
// On return (x, y) is the successor's pixel and the result its side.
__device__ __forceinline__ int successor_of(const unsigned char *__restrict__ mask, int W, int &x, int &y, int s) {
  int t = (s + 1) & 3;                                          // turn right
  if (!(mask[(long long)y * W + x] >> t & 1)) {
    x += dir_x(s); y += dir_y(s); t = s;                        // straight: the ahead-right pixel is inside (it has this label)
    if (!(mask[(long long)y * W + x] >> s & 1)) {
      x += dir_y(s); y -= dir_x(s); t = (s + 3) & 3;            // turn left: the ahead-left pixel has this label as well
    }
  }
  return t;
}

// ---- rings and arcs -------------------------------------------------------------------------------------------------------------
struct DartPlace {                                               // where a dart sits in its ring and its arc
  int head, ring, vertices, breaks;                              // head slot, ring index, the ring's vertex and break darts
  int vrank;                                                     // vertex darts in [head, dart)
  int binc;                                                      // break darts in [head, dart]
  int arc;                                                       // index of its arc before the arcs are sorted
  bool first;                                                    // the arc's first dart
};

template <typename Trace>
__device__ __forceinline__ DartPlace place_of(const Trace &t, int i, int f) {
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

// Id: int (one raster, ids below 2^30) or long long (a scene); pixel coordinates fit an int either way.
template <typename Id>
__device__ __forceinline__ void pixel_of(Id W, Id id, int &x, int &y, int &s) {
  const Id pix = id >> 2, row = pix / W;
  s = (int)(id & 3);
  y = (int)row;
  x = (int)(pix - row * W);
}

template <typename Id>
__device__ __forceinline__ void store_corner(int *__restrict__ xy, long long at, Id W, Id id, bool end) {
  int x, y, s;
  pixel_of(W, id, x, y, s);
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

// FIRST_SLOT: arc_first holds the first dart's slot (a scene: slot order is dart-id order) instead of its id.
template <typename Trace, typename Id, bool FIRST_SLOT>
__global__ void vec_ring_emit_kernel(Trace t) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < t.D; i += gridDim.x * blockDim.x) {
    const int f = t.flags[i];
    const Id id = t.dart[i];
    const DartPlace p = place_of(t, i, f);
    if (f & VTX) store_corner<Id>(t.xy, t.ring_ptr[p.ring] + p.vrank, t.W, id, false);
    // the shoelace term of a unit dart: -y east, +x south, +y west, -x north, at the dart's own line
    int x, y, s;
    pixel_of<Id>(t.W, id, x, y, s);
    const long long term = s == 0 ? -(long long)y : s == 1 ? (long long)x + 1 : s == 2 ? (long long)y + 1 : -(long long)x;
    if (term) atomic_add64((long long *)t.area2 + p.ring, term);
    if (p.first) {
      t.arc_first[p.arc] = FIRST_SLOT ? i : (int)id;
      t.arc_right[p.arc] = t.lab[i];
      t.arc_left[p.arc] = t.other[i];
      t.arc_vstart[p.arc] = p.vrank + (f & VTX);                 // vertex darts in [head, first dart]
    } else if (f & VTX) {
      atomicAdd(t.arc_count + p.arc, 1);
    }
  }
}

template <typename Trace, typename Id>
__global__ void vec_arc_emit_kernel(Trace t) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < t.D; i += gridDim.x * blockDim.x) {
    const int f = t.flags[i];
    const Id id = t.dart[i];
    const DartPlace p = place_of(t, i, f);
    const int pos = t.arc_pos[p.arc];
    if (pos < 0) continue;                                       // the arc is kept from its other side
    const long long base = t.arc_ptr[pos];
    if (p.first) {
      store_corner<Id>(t.arc_xy, base, t.W, id, false);
    } else if (f & VTX) {
      const int start = t.arc_vstart[p.arc];
      const bool wrapped = p.breaks != 0 && p.binc == 0;         // in front of the ring's first break dart: the arc began behind
      store_corner<Id>(t.arc_xy, base + 1 + (wrapped ? p.vertices - start + p.vrank : p.vrank - start), t.W, id, false);
    }
    const int j = t.next[i];
    if (p.breaks == 0 ? j == p.head : (t.flags[j] & BRK) != 0) store_corner<Id>(t.arc_xy, t.arc_ptr[pos + 1] - 1, t.W, id, true);
  }
}

template <typename Trace>
inline int vector_trace_ok(const Trace *t, const char *what, bool arcs) {
  DM_REQUIRE(t && t->dart && t->next && t->lab && t->other && t->flags && t->key && t->sum && t->ring_of_slot && t->arc_base && t->arc_vstart,
             DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  DM_REQUIRE(t->W > 0 && t->D >= 4 && t->R >= 1 && t->n_arcs >= t->R, DM_ERR_BAD_SHAPE, "%s: bad sizes (W=%lld D=%d R=%d n_arcs=%d)", what,
             (long long)t->W, t->D, t->R, t->n_arcs);
  if (arcs) DM_REQUIRE(t->arc_pos && t->arc_ptr && t->arc_xy, DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  else DM_REQUIRE(t->ring_ptr && t->xy && t->area2 && t->arc_first && t->arc_left && t->arc_right && t->arc_count, DM_ERR_BAD_SHAPE,
                  "%s: null pointer", what);
  return DM_OK;
}

}  // namespace
