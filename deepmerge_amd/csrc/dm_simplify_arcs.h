// What the two simplifiers share (dm_simplify.hip: one raster, keep flags per pixel corner; dm_scene_simplify.hip: a scene, keep
// flags per stored arc vertex), each piece once: an arc as its wavefront sees it, the Douglas-Peucker walk of a
// chain, the chains kernel, the arc count / emit kernel and the area of the new rings.  The kernels are templates over how a
// vertex's keep flag is addressed: CornerKeep is the dense raster keep[y (W+1) + x] and performs the arithmetic dm_simplify.hip
// always had; VertexKeep is arc_keep[first + skip + p mod len], one byte per stored vertex, for corner ids that do not fit 32 bits.
#pragma once
#include "dm_raster.h"
#include "dm_simplify.h"

namespace {

constexpr int MAX_SIDE = DM_SIMPLIFY_MAX_SIDE;
constexpr int WAVES = 4;                                         // wavefronts per workgroup of 256

template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

// ---- an arc as its wavefront sees it ---------------------------------------------------------------------------------------------
// Stored vertices xy[first .. first + n).  A closed arc (first vertex == last) is the cyclic sequence of its first n - 1 vertices,
// without the stored start when `skip`: logical position p in [0, 2 len) is stored vertex skip + (p mod len).
struct Arc {
  const int *xy;
  long long first;
  int n, len, skip;
  bool closed;
};

__device__ __forceinline__ void vertex(const Arc &c, int p, int &x, int &y) {
  const long long at = c.first + c.skip + (p >= c.len ? p - c.len : p);
  x = c.xy[2 * at];
  y = c.xy[2 * at + 1];
}

// Index of corner (x, y) in keep; -1 outside the raster.
__device__ __forceinline__ int corner_index(int x, int y, int H, int W) {
  return (x >= 0 && x <= W && y >= 0 && y <= H) ? y * (W + 1) + x : -1;      // (H+1)(W+1) <= 32769^2 < 2^31
}

// False for an arc the tables do not hold.  Wave-uniform.
__device__ __forceinline__ bool arc_of(const int *__restrict__ xy, const long long *__restrict__ arc_ptr, int a, long long Va, Arc &c) {
  const long long first = arc_ptr[a], end = arc_ptr[a + 1];
  if (first < 0 || end > Va || end - first < 2 || end - first > INT_MAX) return false;
  c.xy = xy;
  c.first = first;
  c.n = (int)(end - first);
  c.closed = c.n >= 3 && xy[2 * first] == xy[2 * (end - 1)] && xy[2 * first + 1] == xy[2 * (end - 1) + 1];
  c.len = c.closed ? c.n - 1 : c.n;
  c.skip = 0;
  return true;
}

// ---- where a vertex's keep flag lives --------------------------------------------------------------------------------------------
// at(c, p, x, y): the index in `keep` of the vertex at logical position p of arc c, whose corner is (x, y); -1 outside the raster.
// Anchor: the vertex smallest in (y, x) of a closed arc without a node, folded per lane by see() and over the wave by reduce(),
// which returns its position and its index in keep.  EXTENT: the arc's bounding box has to be checked (see the chains kernel).
template <typename Byte>
struct CornerKeep {
  static constexpr bool EXTENT = false;                          // H, W <= 32768 bound every arc
  Byte *keep;
  int H, W;
  __device__ __forceinline__ long long at(const Arc &, int, int x, int y) const { return corner_index(x, y, H, W); }
  struct Anchor {
    u64 smallest = ~0ULL;                                        // corner index << 32 | position: the corner index orders by (y, x)
    __device__ __forceinline__ void see(const CornerKeep &, long long at, int, int, int p) {
      const u64 key = ((u64)at << 32) | (u64)p;
      smallest = key < smallest ? key : smallest;
    }
    __device__ __forceinline__ int reduce(const CornerKeep &, const Arc &, long long &at) {
      smallest = wave_min(smallest);
      at = (int)(smallest >> 32);
      return (int)(smallest & 0xffffffffULL);
    }
  };
};

template <typename Byte>
struct VertexKeep {
  static constexpr bool EXTENT = true;
  Byte *keep;                                                    // arc_keep [Va]
  int H, W;                                                      // the scene's: below 2^31 - 1
  __device__ __forceinline__ long long at(const Arc &c, int p, int x, int y) const {
    return (x >= 0 && x <= W && y >= 0 && y <= H) ? c.first + c.skip + (p >= c.len ? p - c.len : p) : -1;
  }
  struct Anchor {
    long long corner = LLONG_MAX;                                // y (W+1) + x does not fit beside a position in 64 bits:
    int pos = INT_MAX;                                           // the wave's smallest corner first, then the smallest position that holds it
    __device__ __forceinline__ void see(const VertexKeep &k, long long, int x, int y, int p) {
      const long long id = (long long)y * ((long long)k.W + 1) + x;
      if (id < corner || (id == corner && p < pos)) { corner = id; pos = p; }
    }
    __device__ __forceinline__ int reduce(const VertexKeep &, const Arc &c, long long &at) {
      const long long least = wave_min(corner);
      const int p = wave_min(corner == least ? pos : INT_MAX);
      at = c.first + c.skip + p;                                 // p < len
      return p;
    }
  };
};

// ---- chains -------------------------------------------------------------------------------------------------------------------------
// Douglas-Peucker on the chain of logical positions [s, e] of arc c, by the whole wavefront.  The walk is depth first: the left
// half of a split is taken at once, the right half is pushed.  Every entry on the stack is a segment with at least one interior
// vertex, and the interiors of the entries and of the segment in hand are disjoint parts of the chain's interior, so the stack never
// holds more entries than the chain has interior vertices: fewer than the arc has vertices, which is what `cap` is (the arc's
// share of the workspace, one int64 per stored vertex).  Lane 0 alone reads and writes the stack; the others get it by a shuffle.
template <typename Keep>
__device__ __forceinline__ void split_chain(const Arc &c, int s, int e, const Keep &K, u64 q2, long long *__restrict__ stack, int cap, int lane) {
  int i = s, j = e, sp = 0;
  bool have = e - s > 1;
  while (have) {
    int xi, yi, xj, yj;
    vertex(c, i, xi, yi);
    vertex(c, j, xj, yj);
    const long long dx = xj - xi, dy = yj - yi;
    const u64 len2 = (u64)(dx * dx + dy * dy);
    u64 best = 0;                                                // d << 32 | ~(k - i): the greatest d, then the smallest k
    for (int k = i + 1 + lane; k < j; k += 64) {
      int x, y;
      vertex(c, k, x, y);
      const long long rx = x - xi, ry = y - yi;
      const long long cr = dx * ry - dy * rx;
      const u64 d = len2 == 0 ? (u64)(rx * rx + ry * ry) : (u64)(cr < 0 ? -cr : cr);
      const u64 key = (d << 32) | (u64)(0xffffffffu - (unsigned)(k - i));
      best = key > best ? key : best;
    }
    best = wave_max(best);
    const int k = i + (int)(0xffffffffu - (unsigned)(best & 0xffffffffu));
    bool left = false, right = false;
    if (dm_simplify_exceeds(best >> 32, len2, q2)) {                          // wave-uniform; d = 0 never exceeds
      if (lane == 0) {
        int x, y;
        vertex(c, k, x, y);
        const long long at = K.at(c, k, x, y);
        if (at >= 0) K.keep[at] = 1;
      }
      left = k - i > 1;
      right = j - k > 1;
    }
    if (left && right) {
      if (sp < cap) {
        if (lane == 0) stack[sp] = ((long long)k << 32) | (long long)j;
        ++sp;
      }
      j = k;
    } else if (left) {
      j = k;
    } else if (right) {
      i = k;
    } else if (sp > 0) {
      --sp;
      long long top = lane == 0 ? stack[sp] : 0;
      top = __shfl(top, 0, 64);
      i = (int)(top >> 32);
      j = (int)(top & 0xffffffffLL);
    } else {
      have = false;
    }
  }
}

template <typename Keep>
__global__ __launch_bounds__(256) void simplify_chains_kernel(const int *__restrict__ xy, const long long *__restrict__ arc_ptr, int A, long long Va,
                                                              Keep K, u64 q2, long long *__restrict__ stack) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int a = blockIdx.x * WAVES + wave; a < A; a += gridDim.x * WAVES) {
    Arc c;
    if (!arc_of(xy, arc_ptr, a, Va, c)) continue;
    if (c.closed) {                                              // a stored start inside a straight run is no vertex of the cyclic sequence
      int x0, y0, x1, y1, x2, y2;
      vertex(c, c.len - 1, x0, y0);
      vertex(c, 0, x1, y1);
      vertex(c, 1, x2, y2);
      const long long at = K.at(c, 0, x1, y1);
      const bool node = at >= 0 && K.keep[at] == 2;
      if (!node && (long long)(x1 - x0) * (y2 - y1) == (long long)(y1 - y0) * (x2 - x1)) { c.skip = 1; c.len -= 1; }
    }
    if (c.len < 2) continue;
    // the node scan: the first cut, or the anchor (the vertex smallest in (y, x)); a vertex outside the raster refuses the arc.
    // The scan ends before the first write; the writes store 1 where keep was 0 and a cut is keep == 2, so the later searches for
    // the next cut see the same nodes.
    u64 first_node = ~0ULL;
    typename Keep::Anchor anchor;
    bool bad = false;
    int xmin = INT_MAX, xmax = INT_MIN, ymin = INT_MAX, ymax = INT_MIN;
    for (int p = lane; p < c.len; p += 64) {
      int x, y;
      vertex(c, p, x, y);
      const long long at = K.at(c, p, x, y);
      if (at < 0) { bad = true; continue; }
      if (K.keep[at] == 2 && first_node == ~0ULL) first_node = (u64)p;
      anchor.see(K, at, x, y, p);
      if (Keep::EXTENT) { xmin = min(xmin, x); xmax = max(xmax, x); ymin = min(ymin, y); ymax = max(ymax, y); }
    }
    if (__any(bad)) continue;
    if (Keep::EXTENT) {                                          // |cross| < 2^31 needs the arc's box within 32768 x 32768: else left alone
      const long long w = (long long)wave_max(xmax) - wave_min(xmin), h = (long long)wave_max(ymax) - wave_min(ymin);
      if (w > MAX_SIDE || h > MAX_SIDE) continue;
    }
    first_node = wave_min(first_node);
    int s = 0, end = c.len - 1;                                  // an open arc is cut at its two ends, which are nodes
    if (c.closed) {
      if (first_node != ~0ULL) {
        s = (int)first_node;
      } else {
        long long at;
        s = anchor.reduce(K, c, at);
        if (lane == 0) K.keep[at] = 1;                           // no node: the anchor is kept
      }
      end = s + c.len;
    }
    long long *const stk = stack + c.first;
    while (s < end) {
      int e = end;                                               // the next cut behind s
      for (int base = s + 1; base < end; base += 64) {
        const int p = base + lane;
        bool node = false;
        if (p < end) {
          int x, y;
          vertex(c, p, x, y);
          node = K.keep[K.at(c, p, x, y)] == 2;                  // inside the raster: the scan above saw every vertex
        }
        const u64 m = __ballot(node);
        if (m) { e = base + __ffsll((unsigned long long)m) - 1; break; }
      }
      split_chain(c, s, e, K, q2, stk, c.n, lane);
      s = e;
    }
  }
}

// ---- arcs out -----------------------------------------------------------------------------------------------------------------------
// Kept vertices of an arc in stored order; a closed arc is walked without its repeated end and gets its first kept vertex again
// at its end, which rotates away a stored start that is not kept.  OUT: write them at out[new_ptr[a] ..); else count[a].
template <bool OUT, typename Keep>
__global__ __launch_bounds__(256) void simplify_arc_kernel(const int *__restrict__ xy, const long long *__restrict__ arc_ptr, int A, long long Va,
                                                           Keep K, int *__restrict__ count, const long long *__restrict__ new_ptr, long long Vn,
                                                           int *__restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int a = blockIdx.x * WAVES + wave; a < A; a += gridDim.x * WAVES) {
    Arc c;
    if (!arc_of(xy, arc_ptr, a, Va, c)) {
      if (!OUT && lane == 0) count[a] = 0;
      continue;
    }
    long long to = 0, room = 0;
    if (OUT) {
      to = new_ptr[a];
      room = new_ptr[a + 1] - to;
      if (to < 0 || room < 0 || to + room > Vn) continue;
    }
    int total = 0, fx = 0, fy = 0;
    for (int base = 0; base < c.len; base += 64) {
      const int p = base + lane;
      int x = 0, y = 0;
      bool kept = false;
      if (p < c.len) {
        vertex(c, p, x, y);
        const long long at = K.at(c, p, x, y);
        kept = at >= 0 && K.keep[at] != 0;
      }
      const u64 m = __ballot(kept);
      if (OUT) {
        const int rank = total + __popcll(m & ((1ULL << lane) - 1));
        if (kept && rank < room) { out[2 * (to + rank)] = x; out[2 * (to + rank) + 1] = y; }
        if (total == 0 && m) {                                    // the first kept vertex, for the closing repeat
          const int src = __ffsll((unsigned long long)m) - 1;
          fx = __shfl(x, src, 64);
          fy = __shfl(y, src, 64);
        }
      }
      total += __popcll(m);
    }
    const bool repeat = c.closed && total > 0;
    if (OUT) {
      if (repeat && lane == 0 && total < room) { out[2 * (to + total)] = fx; out[2 * (to + total) + 1] = fy; }
    } else if (lane == 0) {
      count[a] = total + repeat;
    }
  }
}

// ---- the area of the new rings ------------------------------------------------------------------------------------------------------
__global__ void simplify_area_init_kernel(long long *__restrict__ area2, int R) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < R; r += gridDim.x * blockDim.x) area2[r] = 0;
}

// The shoelace term of every new vertex and its successor within its ring (found by an upper-bound search in new_ring_ptr), added
// with integer atomics: the sum does not depend on the order of arrival.  Corners are below 2^31: a term is below 2^63 in 64 bits.
__global__ void simplify_area_kernel(const int *__restrict__ out, const long long *__restrict__ new_ring_ptr, int R, long long Vn,
                                     long long *__restrict__ area2) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < Vn; i += (long long)gridDim.x * blockDim.x) {
    int lo = 0, hi = R;                                          // the last r with new_ring_ptr[r] <= i
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      if (new_ring_ptr[mid] <= i) lo = mid; else hi = mid;
    }
    const long long first = new_ring_ptr[lo], end = new_ring_ptr[lo + 1];
    if (i < first || i >= end || end > Vn) continue;
    const long long n = i + 1 == end ? first : i + 1;
    const long long term = (long long)out[2 * i] * out[2 * n + 1] - (long long)out[2 * n] * out[2 * i + 1];
    if (term) atomic_add64(area2 + lo, term);
  }
}

inline int wave_grid(int items) { return grid_for((long long)items * 64); }

}  // namespace
