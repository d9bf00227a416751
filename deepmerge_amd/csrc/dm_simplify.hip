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
#include "dm_simplify_arcs.h"                                     // an arc, the chains and arc kernels, the area: shared with dm_scene_simplify.hip

namespace {

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

typedef CornerKeep<const unsigned char> DenseRead;

inline bool side_ok(int H, int W) { return H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE; }

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
  hipLaunchKernelGGL(simplify_chains_kernel<CornerKeep<unsigned char>>, dim3(wave_grid(A)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), arc_xy,
                     (const long long *)arc_ptr, A, (long long)Va, CornerKeep<unsigned char>{keep, H, W}, (u64)q * (u64)q, (long long *)stack);
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
  hipLaunchKernelGGL((simplify_arc_kernel<false, DenseRead>), dim3(wave_grid(A)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), arc_xy,
                     (const long long *)arc_ptr, A, (long long)Va, DenseRead{keep, H, W}, count, (const long long *)nullptr, 0LL, (int *)nullptr);
  DM_LAUNCH_CHECK("dm_simplify_arc_count");
  return DM_OK;
}

extern "C" int dm_simplify_arc_emit(const int32_t *arc_xy, const int64_t *arc_ptr, const int64_t *new_ptr, int32_t A, int64_t Va, int64_t Vn, int32_t H,
                                    int32_t W, const uint8_t *keep, int32_t *out_xy, void *stream) {
  if (int rc = simplify_arcs_ok("dm_simplify_arc_emit", arc_xy, arc_ptr, keep, out_xy, A, Va, H, W)) return rc;
  DM_REQUIRE(new_ptr, DM_ERR_BAD_SHAPE, "dm_simplify_arc_emit: null pointer");
  DM_REQUIRE(Vn >= 1 && Vn <= Va, DM_ERR_BAD_SHAPE, "dm_simplify_arc_emit: bad sizes (Vn=%lld Va=%lld; need 1 <= Vn <= Va)", (long long)Vn,
             (long long)Va);
  hipLaunchKernelGGL((simplify_arc_kernel<true, DenseRead>), dim3(wave_grid(A)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), arc_xy,
                     (const long long *)arc_ptr, A, (long long)Va, DenseRead{keep, H, W}, (int *)nullptr, (const long long *)new_ptr, (long long)Vn, out_xy);
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
