// Shared-boundary Douglas-Peucker on the rings and arcs of dm_vector.hip (gfx950).  What leaves the tracing is a pixel staircase;
// simplified per polygon, two neighbours would treat their common boundary differently and leave slivers and overlaps.  Here every
// stretch of boundary is simplified once, as the arc that stores it, and both neighbours see the result through one keep flag per
// pixel corner.  The rule is the build's own: stated in include/deepmerge_hip.h, restated in numpy / Python ints in
// tests/simplify_ref.py.  Everything is an integer, so the device and the spec agree bit for bit.
//   nodes       per corner (the tile walk of dm_raster.h over the (H+1) x (W+1) corners): keep = 2 where at least three of the four
//               grid edges are boundary edges or the corner is a raster corner, else 0
//   chains      one wavefront per arc: lanes stride over the vertices for the cuts (keep == 2) or, on a closed arc without one, the
//               anchor; the wave then splits every chain with an explicit stack, each split a lane-strided arg-max and a wave
//               reduction.  It writes keep = 1, only at corners with two boundary edges, which lie on this arc alone: no races
//   arc_count   one wavefront per arc: its kept vertices          arc_emit   the same walk, writing them
//   ring_count  per ring vertex: the kept corners on the unit steps from it to its successor (this inserts the nodes on a
//               straight run)                                      ring_emit  the same walk, writing them; then area2 per new vertex
// The scans between count and emit are the caller's (rag.simplify: torch.cumsum, as rag._trace and rag.rasterize do it).
#include "dm_raster.h"
#include "dm_simplify.h"

namespace {

constexpr int MAX_SIDE = DM_SIMPLIFY_MAX_SIDE;
constexpr int WAVES = 4;                                         // wavefronts per workgroup of 256

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ u64 wave_min(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

// ---- nodes ------------------------------------------------------------------------------------------------------------------
// The strip of the tile walk is 16 corners of one corner row y: they look at pixels x0 - 1 .. x0 + n - 1 of pixel rows y - 1 and y.
__global__ __launch_bounds__(256) void simplify_nodes_kernel(const int *__restrict__ labels, int H, int W, unsigned char *__restrict__ keep) {
  const Strip g = strip_of(H + 1, W + 1);
  if (!g.live) return;
  int up[STRIP + 1], dn[STRIP + 1];
#pragma unroll
  for (int i = 0; i <= STRIP; ++i) {
    const int px = g.x0 - 1 + i;
    const bool col = i <= g.n && px >= 0 && px < W;
    up[i] = (col && g.y > 0) ? labels[(long long)(g.y - 1) * W + px] : -1;
    dn[i] = (col && g.y < H) ? labels[(long long)g.y * W + px] : -1;
  }
#pragma unroll
  for (int i = 0; i < STRIP; ++i) {
    if (i < g.n) {
      const int degree = (up[i] != up[i + 1]) + (dn[i] != dn[i + 1]) + (up[i] != dn[i]) + (up[i + 1] != dn[i + 1]);
      const int x = g.x0 + i;
      const bool corner = (x == 0 || x == W) && (g.y == 0 || g.y == H);
      keep[g.base + i] = (degree >= 3 || corner) ? 2 : 0;
    }
  }
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

// ---- chains -------------------------------------------------------------------------------------------------------------------------
// Douglas-Peucker on the chain of logical positions [s, e] of arc c, by the whole wavefront.  The walk is depth first: the left
// half of a split is taken at once, the right half is pushed.  Every entry on the stack is a segment with at least one interior
// vertex, and the interiors of the entries and of the segment in hand are disjoint parts of the chain's interior, so the stack never
// holds more entries than the chain has interior vertices: fewer than the arc has vertices, which is what `cap` is (the arc's
// share of the workspace, one int64 per stored vertex).  Lane 0 alone reads and writes the stack; the others get it by a shuffle.
__device__ __forceinline__ void split_chain(const Arc &c, int s, int e, int H, int W, u64 q2, unsigned char *__restrict__ keep,
                                            long long *__restrict__ stack, int cap, int lane) {
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
        const int at = corner_index(x, y, H, W);
        if (at >= 0) keep[at] = 1;
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

__global__ __launch_bounds__(256) void simplify_chains_kernel(const int *__restrict__ xy, const long long *__restrict__ arc_ptr, int A, long long Va,
                                                              int H, int W, u64 q2, unsigned char *__restrict__ keep, long long *__restrict__ stack) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int a = blockIdx.x * WAVES + wave; a < A; a += gridDim.x * WAVES) {
    Arc c;
    if (!arc_of(xy, arc_ptr, a, Va, c)) continue;
    if (c.closed) {                                              // a stored start inside a straight run is no vertex of the cyclic sequence
      int x0, y0, x1, y1, x2, y2;
      vertex(c, c.len - 1, x0, y0);
      vertex(c, 0, x1, y1);
      vertex(c, 1, x2, y2);
      const int at = corner_index(x1, y1, H, W);
      const bool node = at >= 0 && keep[at] == 2;
      if (!node && (long long)(x1 - x0) * (y2 - y1) == (long long)(y1 - y0) * (x2 - x1)) { c.skip = 1; c.len -= 1; }
    }
    if (c.len < 2) continue;
    // the node scan: the first cut, or the anchor (the vertex smallest in (y, x), which is its corner index); a vertex outside the
    // raster refuses the arc.  The scan ends before the first write; the writes store 1 where keep was 0 and a cut is keep == 2,
    // so the later searches for the next cut see the same nodes.
    u64 first_node = ~0ULL, smallest = ~0ULL;
    bool bad = false;
    for (int p = lane; p < c.len; p += 64) {
      int x, y;
      vertex(c, p, x, y);
      const int at = corner_index(x, y, H, W);
      if (at < 0) { bad = true; continue; }
      if (keep[at] == 2 && first_node == ~0ULL) first_node = (u64)p;
      const u64 key = ((u64)at << 32) | (u64)p;
      smallest = key < smallest ? key : smallest;
    }
    if (__any(bad)) continue;
    first_node = wave_min(first_node);
    int s = 0, end = c.len - 1;                                  // an open arc is cut at its two ends, which are nodes
    if (c.closed) {
      if (first_node != ~0ULL) {
        s = (int)first_node;
      } else {
        smallest = wave_min(smallest);
        s = (int)(smallest & 0xffffffffULL);
        if (lane == 0) keep[(int)(smallest >> 32)] = 1;          // no node: the anchor is kept
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
          node = keep[corner_index(x, y, H, W)] == 2;            // inside the raster: the scan above saw every vertex
        }
        const u64 m = __ballot(node);
        if (m) { e = base + __ffsll((unsigned long long)m) - 1; break; }
      }
      split_chain(c, s, e, H, W, q2, keep, stk, c.n, lane);
      s = e;
    }
  }
}

// ---- arcs out -----------------------------------------------------------------------------------------------------------------------
// Kept vertices of an arc in stored order; a closed arc is walked without its repeated end and gets its first kept vertex again
// at its end, which rotates away a stored start that is not kept.  OUT: write them at out[new_ptr[a] ..); else count[a].
template <bool OUT>
__global__ __launch_bounds__(256) void simplify_arc_kernel(const int *__restrict__ xy, const long long *__restrict__ arc_ptr, int A, long long Va, int H,
                                                           int W, const unsigned char *__restrict__ keep, int *__restrict__ count,
                                                           const long long *__restrict__ new_ptr, long long Vn, int *__restrict__ out) {
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
        const int at = corner_index(x, y, H, W);
        kept = at >= 0 && keep[at] != 0;
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

// ---- rings out ----------------------------------------------------------------------------------------------------------------------
// The unit steps from ring vertex v to its successor within its ring: start corner, direction, number of steps.  0 steps for a
// vertex the tables do not hold, outside the raster, or with a successor that is not on its row or column.
struct Walk {
  int x, y, sx, sy, steps;
};

__device__ __forceinline__ Walk walk_of(const int *__restrict__ xy, const long long *__restrict__ ring_ptr, const int *__restrict__ vert_ring, int v,
                                        int V, int R, int H, int W) {
  Walk w = {0, 0, 0, 0, 0};
  const int r = vert_ring[v];
  if (r < 0 || r >= R) return w;
  const long long first = ring_ptr[r], end = ring_ptr[r + 1];
  if (first < 0 || end > V || v < first || v >= end) return w;
  const long long n = v + 1 == end ? first : v + 1;
  const int x0 = xy[2 * (long long)v], y0 = xy[2 * (long long)v + 1], x1 = xy[2 * n], y1 = xy[2 * n + 1];
  if (corner_index(x0, y0, H, W) < 0 || corner_index(x1, y1, H, W) < 0 || (x0 != x1 && y0 != y1)) return w;
  w.x = x0;
  w.y = y0;
  w.sx = (x1 > x0) - (x1 < x0);
  w.sy = (y1 > y0) - (y1 < y0);
  w.steps = abs(x1 - x0) + abs(y1 - y0);                         // every corner of the walk lies between two corners inside the raster
  return w;
}

template <bool OUT>
__global__ void simplify_ring_kernel(const int *__restrict__ xy, const long long *__restrict__ ring_ptr, const int *__restrict__ vert_ring, int V, int R,
                                     int H, int W, const unsigned char *__restrict__ keep, int *__restrict__ count,
                                     const long long *__restrict__ scan, long long Vn, int *__restrict__ out) {
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
    const Walk w = walk_of(xy, ring_ptr, vert_ring, v, V, R, H, W);
    const int stride = w.sy * (W + 1) + w.sx;
    int at = w.y * (W + 1) + w.x, x = w.x, y = w.y, c = 0;
    long long to = 0, room = 0;
    if (OUT) {
      to = scan[v];
      room = scan[v + 1] - to;
      if (to < 0 || room < 0 || to + room > Vn) continue;
    }
    for (int s = 0; s < w.steps; ++s, at += stride, x += w.sx, y += w.sy) {
      if (keep[at]) {
        if (OUT && c < room) { out[2 * (to + c)] = x; out[2 * (to + c) + 1] = y; }
        ++c;
      }
    }
    if (!OUT) count[v] = c;
  }
}

__global__ void simplify_area_init_kernel(long long *__restrict__ area2, int R) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < R; r += gridDim.x * blockDim.x) area2[r] = 0;
}

// The shoelace term of every new vertex and its successor within its ring (found by an upper-bound search in new_ring_ptr), added
// with integer atomics: the sum does not depend on the order of arrival.
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

inline bool side_ok(int H, int W) { return H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE; }
inline int wave_grid(int items) { return grid_for((long long)items * 64); }

}  // namespace

#define SIDES "need 1 <= H, W <= 32768"

extern "C" int dm_simplify_nodes(const int32_t *labels, int32_t H, int32_t W, uint8_t *keep, void *stream) {
  DM_REQUIRE(labels && keep, DM_ERR_BAD_SHAPE, "dm_simplify_nodes: null pointer");
  DM_REQUIRE(side_ok(H, W), DM_ERR_BAD_SHAPE, "dm_simplify_nodes: bad sizes (H=%d W=%d; " SIDES ")", H, W);
  hipLaunchKernelGGL(simplify_nodes_kernel, tile_grid(H + 1, W + 1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), labels, H, W, keep);
  DM_LAUNCH_CHECK("dm_simplify_nodes");
  return DM_OK;
}

extern "C" int dm_simplify_chains(const int32_t *arc_xy, const int64_t *arc_ptr, int32_t A, int64_t Va, int32_t H, int32_t W, int32_t q, uint8_t *keep,
                                  int64_t *stack, void *stream) {
  DM_REQUIRE(arc_xy && arc_ptr && keep && stack, DM_ERR_BAD_SHAPE, "dm_simplify_chains: null pointer");
  DM_REQUIRE(side_ok(H, W) && A > 0 && Va >= 2 && Va <= (1LL << 30), DM_ERR_BAD_SHAPE,
             "dm_simplify_chains: bad sizes (H=%d W=%d A=%d Va=%lld; " SIDES ", A >= 1, 2 <= Va <= 2^30)", H, W, A, (long long)Va);
  DM_REQUIRE(q >= 0 && q <= DM_SIMPLIFY_MAX_Q, DM_ERR_BAD_SHAPE, "dm_simplify_chains: bad tolerance (q=%d; need 0 <= q <= 2^20)", q);
  hipLaunchKernelGGL(simplify_chains_kernel, dim3(wave_grid(A)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), arc_xy,
                     (const long long *)arc_ptr, A, (long long)Va, H, W, (u64)q * (u64)q, keep, (long long *)stack);
  DM_LAUNCH_CHECK("dm_simplify_chains");
  return DM_OK;
}

static int simplify_arcs_ok(const char *what, const void *a, const void *b, const void *c, const void *d, int32_t A, int64_t Va, int32_t H, int32_t W) {
  DM_REQUIRE(a && b && c && d, DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  DM_REQUIRE(side_ok(H, W) && A > 0 && Va >= 2 && Va <= (1LL << 30), DM_ERR_BAD_SHAPE,
             "%s: bad sizes (H=%d W=%d A=%d Va=%lld; " SIDES ", A >= 1, 2 <= Va <= 2^30)", what, H, W, A, (long long)Va);
  return DM_OK;
}

extern "C" int dm_simplify_arc_count(const int32_t *arc_xy, const int64_t *arc_ptr, int32_t A, int64_t Va, int32_t H, int32_t W, const uint8_t *keep,
                                     int32_t *count, void *stream) {
  if (int rc = simplify_arcs_ok("dm_simplify_arc_count", arc_xy, arc_ptr, keep, count, A, Va, H, W)) return rc;
  hipLaunchKernelGGL(simplify_arc_kernel<false>, dim3(wave_grid(A)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), arc_xy,
                     (const long long *)arc_ptr, A, (long long)Va, H, W, keep, count, (const long long *)nullptr, 0LL, (int *)nullptr);
  DM_LAUNCH_CHECK("dm_simplify_arc_count");
  return DM_OK;
}

extern "C" int dm_simplify_arc_emit(const int32_t *arc_xy, const int64_t *arc_ptr, const int64_t *new_ptr, int32_t A, int64_t Va, int64_t Vn, int32_t H,
                                    int32_t W, const uint8_t *keep, int32_t *out_xy, void *stream) {
  if (int rc = simplify_arcs_ok("dm_simplify_arc_emit", arc_xy, arc_ptr, keep, out_xy, A, Va, H, W)) return rc;
  DM_REQUIRE(new_ptr, DM_ERR_BAD_SHAPE, "dm_simplify_arc_emit: null pointer");
  DM_REQUIRE(Vn >= 1 && Vn <= Va, DM_ERR_BAD_SHAPE, "dm_simplify_arc_emit: bad sizes (Vn=%lld Va=%lld; need 1 <= Vn <= Va)", (long long)Vn,
             (long long)Va);
  hipLaunchKernelGGL(simplify_arc_kernel<true>, dim3(wave_grid(A)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), arc_xy,
                     (const long long *)arc_ptr, A, (long long)Va, H, W, keep, (int *)nullptr, (const long long *)new_ptr, (long long)Vn, out_xy);
  DM_LAUNCH_CHECK("dm_simplify_arc_emit");
  return DM_OK;
}

static int simplify_rings_ok(const char *what, const void *a, const void *b, const void *c, const void *d, const void *e, int32_t V, int32_t R, int32_t H,
                             int32_t W) {
  DM_REQUIRE(a && b && c && d && e, DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  DM_REQUIRE(side_ok(H, W) && V > 0 && V <= (1 << 30) && R > 0 && R <= V, DM_ERR_BAD_SHAPE,
             "%s: bad sizes (H=%d W=%d V=%d R=%d; " SIDES ", 1 <= R <= V <= 2^30)", what, H, W, V, R);
  return DM_OK;
}

extern "C" int dm_simplify_ring_count(const int32_t *xy, const int64_t *ring_ptr, const int32_t *vert_ring, int32_t V, int32_t R, int32_t H, int32_t W,
                                      const uint8_t *keep, int32_t *count, void *stream) {
  if (int rc = simplify_rings_ok("dm_simplify_ring_count", xy, ring_ptr, vert_ring, keep, count, V, R, H, W)) return rc;
  hipLaunchKernelGGL(simplify_ring_kernel<false>, dim3(grid_for(V)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), xy,
                     (const long long *)ring_ptr, vert_ring, V, R, H, W, keep, count, (const long long *)nullptr, 0LL, (int *)nullptr);
  DM_LAUNCH_CHECK("dm_simplify_ring_count");
  return DM_OK;
}

extern "C" int dm_simplify_ring_emit(const int32_t *xy, const int64_t *ring_ptr, const int32_t *vert_ring, const int64_t *scan,
                                     const int64_t *new_ring_ptr, int32_t V, int32_t R, int64_t Vn, int32_t H, int32_t W, const uint8_t *keep,
                                     int32_t *out_xy, int64_t *area2, void *stream) {
  if (int rc = simplify_rings_ok("dm_simplify_ring_emit", xy, ring_ptr, vert_ring, keep, out_xy, V, R, H, W)) return rc;
  DM_REQUIRE(scan && new_ring_ptr && area2, DM_ERR_BAD_SHAPE, "dm_simplify_ring_emit: null pointer");
  DM_REQUIRE(Vn >= 1 && Vn <= (1LL << 30), DM_ERR_BAD_SHAPE, "dm_simplify_ring_emit: bad sizes (Vn=%lld; need 1 <= Vn <= 2^30)", (long long)Vn);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(simplify_ring_kernel<true>, dim3(grid_for(V)), dim3(256), 0, s, xy, (const long long *)ring_ptr, vert_ring, V, R, H, W, keep,
                     (int *)nullptr, (const long long *)scan, (long long)Vn, out_xy);
  hipLaunchKernelGGL(simplify_area_init_kernel, dim3(grid_for(R)), dim3(256), 0, s, (long long *)area2, R);
  hipLaunchKernelGGL(simplify_area_kernel, dim3(grid_for(Vn)), dim3(256), 0, s, (const int *)out_xy, (const long long *)new_ring_ptr, R, (long long)Vn,
                     (long long *)area2);
  DM_LAUNCH_CHECK("dm_simplify_ring_emit");
  return DM_OK;
}
