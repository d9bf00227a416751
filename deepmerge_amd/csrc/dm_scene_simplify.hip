// Shared-boundary Douglas-Peucker on a scene's rings and arcs across tile seams (gfx950).  DESIGN.md 3.5.11.
// The rule is dm_simplify.hip's, unchanged; what is new is how `keep` is held.  A scene has no (H+1) x (W+1) corner raster on the
// device, and its corner ids y (W+1) + x need 64 bits.  Three facts about the rule let three sparse things stand for the raster:
//   1. a corner with keep == 1 is a stored vertex of exactly one arc, once among its positions below len;
//   2. a node that lies on an arc is a stored vertex of it: the chain pass needs keep only at arc vertices;
//   3. on the straight run from a ring vertex v to its successor the kept corners are v itself, if kept, and the NODES strictly
//      inside the run (the T-junctions).
// So: the scene's nodes as two sorted int64 lists (node_row by y (W+1) + x, node_col by x (H+1) + y), one keep byte per stored arc
// vertex (arc_keep, 2 where the vertex is a node), and the sorted kept set kept_row (nodes and arc vertices with arc_keep == 1).
//   nodes       per tile: the node rule of simplify_nodes_kernel over the corners a tile's core owns, read through the window that
//               scene.trace_labels reads (core + one pixel, clipped to the scene); count per 64x64 block, scan, emit int64 scene ids
//   chains      dm_simplify_arcs.h's kernel on VertexKeep: the flag of a vertex is found by its position, not by its corner
//   arc_count / arc_emit   dm_simplify_arcs.h's kernel on VertexKeep
//   ring_count  per ring vertex: one binary search in kept_row, two in node_row (a horizontal run) or node_col (a vertical one);
//               O(log nodes) where the dense walk is O(run length)        ring_emit  the same searches, writing; then area2
// The sorts, the scans and arc_keep's 2s are the caller's (scene.simplify_labels: table arithmetic in torch).
#include "dm_simplify_arcs.h"
#include "dm_vector.h"                                           // vec_scan_kernel

namespace {

constexpr long long MAX_SCENE_SIDE = DM_SCENE_VECTOR_MAX_SIDE;

// ---- nodes per tile ---------------------------------------------------------------------------------------------------------------
// The tile walk runs over the (H+1) x (W+1) corners of the window; corner (x, y) of the window is scene corner (x + ox, y + oy).  It
// belongs to the core that holds scene pixel (min(Y, scene_h - 1), min(X, scene_w - 1)): the bottom and right cores also own corner
// row scene_h and corner column scene_w.  The four pixels of an owned corner lie in core + apron, so outside the window is only
// ever asked where it is outside the scene: -1, as in the one-raster rule.
struct NodeTile {
  const int *labels;
  int H, W, cy0, cy1, cx0, cx1;
  long long oy, ox, scene_h, scene_w;
};

template <bool OUT>
__global__ __launch_bounds__(256) void scene_nodes_kernel(NodeTile t, int *__restrict__ tile_count, const int *__restrict__ tile_off, int N,
                                                          long long *__restrict__ out) {
  __shared__ int lds[4];
  const Strip g = strip_of(t.H + 1, t.W + 1);
  unsigned nodes = 0;                                            // bit i: corner x0 + i of the strip is an owned node
  if (g.live) {
    const int py = (int)min((long long)g.y, t.scene_h - 1 - t.oy);                 // the window row of the pixel that decides the owner
    const bool row_in = py >= t.cy0 && py < t.cy1;
    int up[STRIP + 1], dn[STRIP + 1];
#pragma unroll
    for (int i = 0; i <= STRIP; ++i) {
      const int px = g.x0 - 1 + i;
      const bool col = row_in && i <= g.n && px >= 0 && px < t.W;
      up[i] = (col && g.y > 0) ? t.labels[(long long)(g.y - 1) * t.W + px] : -1;
      dn[i] = (col && g.y < t.H) ? t.labels[(long long)g.y * t.W + px] : -1;
    }
#pragma unroll
    for (int i = 0; i < STRIP; ++i) {
      if (i < g.n) {
        const int x = g.x0 + i;
        const int px = (int)min((long long)x, t.scene_w - 1 - t.ox);
        const long long X = x + t.ox, Y = g.y + t.oy;
        const int degree = (up[i] != up[i + 1]) + (dn[i] != dn[i + 1]) + (up[i] != dn[i]) + (up[i + 1] != dn[i + 1]);
        const bool corner = (X == 0 || X == t.scene_w) && (Y == 0 || Y == t.scene_h);
        if (row_in && px >= t.cx0 && px < t.cx1 && (degree >= 3 || corner)) nodes |= 1u << i;
      }
    }
  }
  int total;
  const int before = block_exclusive<int, 256>(__popc(nodes), lds, total);
  if (!OUT) {
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
    return;
  }
  long long to = (long long)tile_off[blockIdx.x] + before;
  const long long row = (g.y + t.oy) * (t.scene_w + 1) + t.ox;
  for (int i = 0; i < STRIP; ++i)
    if (nodes >> i & 1) {
      if (to >= 0 && to < N) out[to] = row + g.x0 + i;
      ++to;
    }
}

inline int node_tile_ok(const char *what, const int32_t *labels, int32_t H, int32_t W, int32_t cy0, int32_t cy1, int32_t cx0, int32_t cx1, int64_t oy,
                        int64_t ox, int64_t scene_h, int64_t scene_w) {
  DM_REQUIRE(labels, DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  DM_REQUIRE(H > 0 && W > 0 && (long long)H * W <= (1LL << 28), DM_ERR_BAD_SHAPE, "%s: need 1 <= H*W <= 2^28 (H=%d W=%d)", what, H, W);
  DM_REQUIRE(0 <= cy0 && cy0 < cy1 && cy1 <= H && 0 <= cx0 && cx0 < cx1 && cx1 <= W && cy0 <= 1 && cx0 <= 1 && H - cy1 <= 1 && W - cx1 <= 1,
             DM_ERR_BAD_SHAPE, "%s: the core [%d,%d) x [%d,%d) must lie in the window %d x %d with an apron of 0 or 1", what, cy0, cy1, cx0, cx1, H,
             W);
  DM_REQUIRE(scene_h >= 1 && scene_w >= 1 && scene_h < MAX_SCENE_SIDE && scene_w < MAX_SCENE_SIDE && scene_h <= DM_SCENE_VECTOR_MAX_PIXELS / scene_w &&
                 oy >= 0 && ox >= 0 && H <= scene_h && W <= scene_w && oy <= scene_h - H && ox <= scene_w - W,
             DM_ERR_BAD_SHAPE, "%s: the window %d x %d at (y=%lld, x=%lld) must lie in a scene of %lld x %lld, sides < 2^31-1, at most 2^60 pixels",
             what, H, W, (long long)oy, (long long)ox, (long long)scene_h, (long long)scene_w);
  // an apron of 0 only where the window's edge is the scene's: else an owned corner would ask a pixel the window does not hold
  DM_REQUIRE((cy0 == 1 || oy == 0) && (cx0 == 1 || ox == 0) && (H - cy1 == 1 || oy + H == scene_h) && (W - cx1 == 1 || ox + W == scene_w),
             DM_ERR_BAD_SHAPE, "%s: the core [%d,%d) x [%d,%d) may touch an edge of the window %d x %d only where that is the scene's edge", what,
             cy0, cy1, cx0, cx1, H, W);
  return DM_OK;
}

// ---- rings out from the sorted lists ----------------------------------------------------------------------------------------------
struct SceneRings {
  const int *xy;
  const long long *ring_ptr;
  const int *vert_ring;
  const long long *node_row, *node_col, *kept_row;
  long long Nn, Nk, scene_h, scene_w;
  int V, R;
};

// The first index i in [0, n) with list[i] >= key, n if there is none.
__device__ __forceinline__ long long lower_bound(const long long *__restrict__ list, long long n, long long key) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (list[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The run from ring vertex v to its successor within its ring.  steps == 0 for a vertex the tables do not hold, outside the scene,
// or with a successor that is not on its row or column (or on itself).  Otherwise: `kept` (v is in kept_row), and the nodes strictly
// inside the run are list[a .. b) of node_row (horizontal) or node_col (vertical), whose ids are base + the moving coordinate.
struct Run {
  int x0, y0, x1, y1;
  long long steps, a, b, base, lo, hi;
  const long long *list;
  bool kept, horizontal;
};

__device__ __forceinline__ Run run_of(const SceneRings &t, long long v) {
  Run w = {};
  const int r = t.vert_ring[v];
  if (r < 0 || r >= t.R) return w;
  const long long first = t.ring_ptr[r], end = t.ring_ptr[r + 1];
  if (first < 0 || end > t.V || v < first || v >= end) return w;
  const long long n = v + 1 == end ? first : v + 1;
  const int x0 = t.xy[2 * v], y0 = t.xy[2 * v + 1], x1 = t.xy[2 * n], y1 = t.xy[2 * n + 1];
  if (x0 < 0 || x0 > t.scene_w || y0 < 0 || y0 > t.scene_h || x1 < 0 || x1 > t.scene_w || y1 < 0 || y1 > t.scene_h || (x0 != x1 && y0 != y1)) return w;
  w.x0 = x0; w.y0 = y0; w.x1 = x1; w.y1 = y1;
  w.steps = llabs((long long)x1 - x0) + llabs((long long)y1 - y0);
  if (w.steps == 0) return w;
  const long long id = (long long)y0 * (t.scene_w + 1) + x0;
  const long long k = lower_bound(t.kept_row, t.Nk, id);
  w.kept = k < t.Nk && t.kept_row[k] == id;
  w.horizontal = y0 == y1;
  w.list = w.horizontal ? t.node_row : t.node_col;
  w.base = w.horizontal ? (long long)y0 * (t.scene_w + 1) : (long long)x0 * (t.scene_h + 1);
  const long long from = w.horizontal ? x0 : y0, to = w.horizontal ? x1 : y1;
  w.lo = w.base + min(from, to) + 1;                             // ids in [lo, hi): strictly inside the run
  w.hi = w.base + max(from, to);
  if (w.steps > 1) {                                             // a unit step, most of a staircase, has no corner inside
    w.a = lower_bound(w.list, t.Nn, w.lo);
    w.b = lower_bound(w.list, t.Nn, w.hi);
  }
  return w;
}

// status[0] = 1 where a list shows itself unsorted: a range that ends before it begins or holds more nodes than the run has inner
// corners, or (emit) an entry of the range outside [lo, hi).  ring_count clears it first; ring_emit only ever sets it.
template <bool OUT>
__global__ void scene_ring_kernel(SceneRings t, int *__restrict__ count, const long long *__restrict__ scan, long long Vn, int *__restrict__ out,
                                  int *__restrict__ status) {
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < t.V; v += (long long)gridDim.x * blockDim.x) {
    const Run w = run_of(t, v);
    bool bad = w.steps > 0 && (w.b < w.a || w.b - w.a >= w.steps);
    const long long inside = (w.steps == 0 || bad) ? 0 : w.b - w.a;
    if (!OUT) {
      count[v] = (int)(w.kept + inside);                          // inside < steps < 2^31
    } else {
      long long to = scan[v];
      const long long room = scan[v + 1] - to;
      if (to >= 0 && room >= 0 && to + room <= Vn) {
        const long long stop = to + room;
        if (w.kept && to < stop) { out[2 * to] = w.x0; out[2 * to + 1] = w.y0; ++to; }
        const bool up = w.horizontal ? w.x1 > w.x0 : w.y1 > w.y0;                    // emitted in the walk's direction
        for (long long i = 0; i < inside && to < stop; ++i, ++to) {
          const long long id = w.list[up ? w.a + i : w.b - 1 - i];
          if (id < w.lo || id >= w.hi) { bad = true; break; }
          const int c = (int)(id - w.base);
          out[2 * to] = w.horizontal ? c : w.x0;
          out[2 * to + 1] = w.horizontal ? w.y0 : c;
        }
      }
    }
    if (bad) atomicExch(status, 1);
  }
}

__global__ void scene_status_clear_kernel(int *__restrict__ status) { *status = 0; }

inline int scene_sides_ok(const char *what, int64_t scene_h, int64_t scene_w) {
  DM_REQUIRE(scene_h >= 1 && scene_w >= 1 && scene_h < MAX_SCENE_SIDE && scene_w < MAX_SCENE_SIDE && scene_h <= DM_SCENE_VECTOR_MAX_PIXELS / scene_w,
             DM_ERR_BAD_SHAPE, "%s: bad scene (%lld x %lld; need sides in 1..2^31-2 and at most 2^60 pixels)", what, (long long)scene_h,
             (long long)scene_w);
  return DM_OK;
}

inline int scene_arcs_ok(const char *what, const void *a, const void *b, const void *c, const void *d, int32_t A, int64_t Va, int64_t scene_h,
                         int64_t scene_w) {
  DM_REQUIRE(a && b && c && d, DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  if (int rc = scene_sides_ok(what, scene_h, scene_w)) return rc;
  DM_REQUIRE(A > 0 && Va >= 2 && Va < (1LL << 31), DM_ERR_BAD_SHAPE, "%s: bad sizes (A=%d Va=%lld; need A >= 1, 2 <= Va < 2^31)", what, A,
             (long long)Va);
  return DM_OK;
}

inline int scene_rings_ok(const char *what, const DmSceneSimplifyRings *t) {
  DM_REQUIRE(t, DM_ERR_BAD_SHAPE, "%s: null argument struct", what);
  DM_REQUIRE(t->xy && t->ring_ptr && t->vert_ring && t->node_row && t->node_col && t->kept_row && t->status, DM_ERR_BAD_SHAPE, "%s: null pointer",
             what);
  if (int rc = scene_sides_ok(what, t->scene_h, t->scene_w)) return rc;
  DM_REQUIRE(t->V > 0 && t->R > 0 && t->R <= t->V, DM_ERR_BAD_SHAPE, "%s: bad sizes (V=%d R=%d; need 1 <= R <= V)", what, t->V, t->R);
  // every scene has its four corners; a kept vertex is a node or a vertex of an arc, and arcs have fewer than 2^31 vertices
  DM_REQUIRE(t->n_nodes >= 4 && t->n_nodes < (1LL << 31) && t->n_kept >= t->n_nodes && t->n_kept < (1LL << 32), DM_ERR_BAD_SHAPE,
             "%s: oversized or undersized list (n_nodes=%lld n_kept=%lld; need 4 <= n_nodes < 2^31, n_nodes <= n_kept < 2^32)", what,
             (long long)t->n_nodes, (long long)t->n_kept);
  return DM_OK;
}

inline SceneRings rings_of(const DmSceneSimplifyRings *t) {
  return SceneRings{t->xy, (const long long *)t->ring_ptr, t->vert_ring, (const long long *)t->node_row, (const long long *)t->node_col,
                    (const long long *)t->kept_row, t->n_nodes, t->n_kept, t->scene_h, t->scene_w, t->V, t->R};
}

typedef VertexKeep<unsigned char> SparseKeep;
typedef VertexKeep<const unsigned char> SparseRead;

}  // namespace

extern "C" int dm_scene_simplify_node_count(const int32_t *labels, int32_t H, int32_t W, int32_t cy0, int32_t cy1, int32_t cx0, int32_t cx1, int64_t oy,
                                            int64_t ox, int64_t scene_h, int64_t scene_w, int32_t *tile_off, int32_t *n_nodes, void *stream) {
  if (int rc = node_tile_ok("dm_scene_simplify_node_count", labels, H, W, cy0, cy1, cx0, cx1, oy, ox, scene_h, scene_w)) return rc;
  DM_REQUIRE(tile_off && n_nodes, DM_ERR_BAD_SHAPE, "dm_scene_simplify_node_count: null pointer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid = tile_grid(H + 1, W + 1);
  const NodeTile t{labels, H, W, cy0, cy1, cx0, cx1, (long long)oy, (long long)ox, (long long)scene_h, (long long)scene_w};
  hipLaunchKernelGGL(scene_nodes_kernel<false>, grid, dim3(256), 0, s, t, tile_off, (const int *)nullptr, 0, (long long *)nullptr);
  hipLaunchKernelGGL(vec_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, tile_off, (int)grid.x, n_nodes);
  DM_LAUNCH_CHECK("dm_scene_simplify_node_count");
  return DM_OK;
}

extern "C" int dm_scene_simplify_node_emit(const int32_t *labels, int32_t H, int32_t W, int32_t cy0, int32_t cy1, int32_t cx0, int32_t cx1, int64_t oy,
                                           int64_t ox, int64_t scene_h, int64_t scene_w, const int32_t *tile_off, int32_t N, int64_t *node,
                                           void *stream) {
  if (int rc = node_tile_ok("dm_scene_simplify_node_emit", labels, H, W, cy0, cy1, cx0, cx1, oy, ox, scene_h, scene_w)) return rc;
  DM_REQUIRE(tile_off && node, DM_ERR_BAD_SHAPE, "dm_scene_simplify_node_emit: null pointer");
  DM_REQUIRE(N >= 1 && (long long)N <= ((long long)H + 1) * ((long long)W + 1), DM_ERR_BAD_SHAPE,
             "dm_scene_simplify_node_emit: bad sizes (N=%d; need 1 <= N <= (H+1)(W+1))", N);
  const NodeTile t{labels, H, W, cy0, cy1, cx0, cx1, (long long)oy, (long long)ox, (long long)scene_h, (long long)scene_w};
  hipLaunchKernelGGL(scene_nodes_kernel<true>, tile_grid(H + 1, W + 1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), t, (int *)nullptr, tile_off,
                     N, (long long *)node);
  DM_LAUNCH_CHECK("dm_scene_simplify_node_emit");
  return DM_OK;
}

extern "C" int dm_scene_simplify_chains(const int32_t *arc_xy, const int64_t *arc_ptr, int32_t A, int64_t Va, int64_t scene_h, int64_t scene_w,
                                        int32_t q, uint8_t *arc_keep, int64_t *stack, void *stream) {
  if (int rc = scene_arcs_ok("dm_scene_simplify_chains", arc_xy, arc_ptr, arc_keep, stack, A, Va, scene_h, scene_w)) return rc;
  DM_REQUIRE(q >= 0 && q <= DM_SIMPLIFY_MAX_Q, DM_ERR_BAD_SHAPE, "dm_scene_simplify_chains: bad tolerance (q=%d; need 0 <= q <= 2^20)", q);
  hipLaunchKernelGGL(simplify_chains_kernel<SparseKeep>, dim3(wave_grid(A)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), arc_xy,
                     (const long long *)arc_ptr, A, (long long)Va, SparseKeep{arc_keep, (int)scene_h, (int)scene_w}, (u64)q * (u64)q,
                     (long long *)stack);
  DM_LAUNCH_CHECK("dm_scene_simplify_chains");
  return DM_OK;
}

extern "C" int dm_scene_simplify_arc_count(const int32_t *arc_xy, const int64_t *arc_ptr, int32_t A, int64_t Va, int64_t scene_h, int64_t scene_w,
                                           const uint8_t *arc_keep, int32_t *count, void *stream) {
  if (int rc = scene_arcs_ok("dm_scene_simplify_arc_count", arc_xy, arc_ptr, arc_keep, count, A, Va, scene_h, scene_w)) return rc;
  hipLaunchKernelGGL((simplify_arc_kernel<false, SparseRead>), dim3(wave_grid(A)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), arc_xy,
                     (const long long *)arc_ptr, A, (long long)Va, SparseRead{arc_keep, (int)scene_h, (int)scene_w}, count,
                     (const long long *)nullptr, 0LL, (int *)nullptr);
  DM_LAUNCH_CHECK("dm_scene_simplify_arc_count");
  return DM_OK;
}

extern "C" int dm_scene_simplify_arc_emit(const int32_t *arc_xy, const int64_t *arc_ptr, const int64_t *new_ptr, int32_t A, int64_t Va, int64_t Vn,
                                          int64_t scene_h, int64_t scene_w, const uint8_t *arc_keep, int32_t *out_xy, void *stream) {
  if (int rc = scene_arcs_ok("dm_scene_simplify_arc_emit", arc_xy, arc_ptr, arc_keep, out_xy, A, Va, scene_h, scene_w)) return rc;
  DM_REQUIRE(new_ptr, DM_ERR_BAD_SHAPE, "dm_scene_simplify_arc_emit: null pointer");
  DM_REQUIRE(Vn >= 1 && Vn <= Va, DM_ERR_BAD_SHAPE, "dm_scene_simplify_arc_emit: bad sizes (Vn=%lld Va=%lld; need 1 <= Vn <= Va)", (long long)Vn,
             (long long)Va);
  hipLaunchKernelGGL((simplify_arc_kernel<true, SparseRead>), dim3(wave_grid(A)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), arc_xy,
                     (const long long *)arc_ptr, A, (long long)Va, SparseRead{arc_keep, (int)scene_h, (int)scene_w}, (int *)nullptr,
                     (const long long *)new_ptr, (long long)Vn, out_xy);
  DM_LAUNCH_CHECK("dm_scene_simplify_arc_emit");
  return DM_OK;
}

extern "C" int dm_scene_simplify_ring_count(const DmSceneSimplifyRings *t, int32_t *count, void *stream) {
  if (int rc = scene_rings_ok("dm_scene_simplify_ring_count", t)) return rc;
  DM_REQUIRE(count, DM_ERR_BAD_SHAPE, "dm_scene_simplify_ring_count: null pointer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(scene_status_clear_kernel, dim3(1), dim3(1), 0, s, t->status);
  hipLaunchKernelGGL(scene_ring_kernel<false>, dim3(grid_for(t->V)), dim3(256), 0, s, rings_of(t), count, (const long long *)nullptr, 0LL,
                     (int *)nullptr, t->status);
  DM_LAUNCH_CHECK("dm_scene_simplify_ring_count");
  return DM_OK;
}

extern "C" int dm_scene_simplify_ring_emit(const DmSceneSimplifyRings *t, const int64_t *scan, const int64_t *new_ring_ptr, int64_t Vn,
                                           int32_t *out_xy, int64_t *area2, void *stream) {
  if (int rc = scene_rings_ok("dm_scene_simplify_ring_emit", t)) return rc;
  DM_REQUIRE(scan && new_ring_ptr && out_xy && area2, DM_ERR_BAD_SHAPE, "dm_scene_simplify_ring_emit: null pointer");
  DM_REQUIRE(Vn >= 1 && Vn < (1LL << 32), DM_ERR_BAD_SHAPE, "dm_scene_simplify_ring_emit: bad sizes (Vn=%lld; need 1 <= Vn < 2^32)", (long long)Vn);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(scene_ring_kernel<true>, dim3(grid_for(t->V)), dim3(256), 0, s, rings_of(t), (int *)nullptr, (const long long *)scan,
                     (long long)Vn, out_xy, t->status);
  hipLaunchKernelGGL(simplify_area_init_kernel, dim3(grid_for(t->R)), dim3(256), 0, s, (long long *)area2, t->R);
  hipLaunchKernelGGL(simplify_area_kernel, dim3(grid_for(Vn)), dim3(256), 0, s, (const int *)out_xy, (const long long *)new_ring_ptr, t->R,
                     (long long)Vn, (long long *)area2);
  DM_LAUNCH_CHECK("dm_scene_simplify_ring_emit");
  return DM_OK;
}
