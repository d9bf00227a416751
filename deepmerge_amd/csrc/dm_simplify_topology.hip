// Topology-safe simplification (gfx950): find the segments of a simplified scene that meet another segment or jumped over a fixed
// point, and repair them by keeping more vertices.  The rule is the build's own: stated in include/deepmerge_hip.h, restated in
// numpy / Python ints in tests/simplify_topology_ref.py.  Integers only: the device and the spec agree bit for bit.
//   points     once per call, one wavefront per arc: its nodes (keep == 2) or, on a closed arc without one, its anchor, binned by
//              grid cell (count, the caller's scan, fill).  A node is an end of several arcs and is binned once per arc: the jump
//              test is an OR over the points, so copies change nothing
//   segments   per round, one wavefront per arc: slot e of the table is vertex e of the simplified arcs dm_simplify_arc_emit would
//              write (arc, skip, logical position in the arc as dm_simplify_chains sees it, corner); segment e joins slots e and
//              e + 1 of one arc, so the last slot of every arc starts no segment
//   bin_count  per slot: kind = 1 for a degenerate segment, else 0; every other segment adds 1 to the cells it passes through
//   bin_fill   the same walk, writing the slot into its cells (the order within a cell is the order of arrival; nothing reads it)
//   pairs      one wavefront per cell: a lane per registered segment against every other one of the cell; atomicOr of kind bit 1
//   jumps      one wavefront per segment with interior vertices: the fixed points of the cells under the sub-chain's bounding box,
//              a lane per point, the polygon's edges in step over the wave; atomicOr of kind bit 2
//   refine     one wavefront per slot: tallies the flagged segments and, for one with interior vertices, keeps the arg-max and
//              runs split_chain (dm_simplify_arcs.h) on both halves.  It stores keep = 1 only at interior vertices of its own
//              segment, which no other segment holds, and reads no keep: no races
// Work follows the segments and points per cell; only the per-cell counters are as many as the raster has cells.
#include "dm_simplify_arcs.h"
#include "dm_simplify_topology.h"

namespace {

constexpr int LOG2 = DM_SIMPLIFY_TOPOLOGY_CELL_LOG2;
typedef DmSimplifyTopology Topo;
typedef CornerKeep<const unsigned char> KeepRead;

__device__ __forceinline__ int grid_w(const Topo &t) { return (t.W >> LOG2) + 1; }
__device__ __forceinline__ int grid_h(const Topo &t) { return (t.H >> LOG2) + 1; }
__device__ __forceinline__ int cell_of(const Topo &t, int cx, int cy) {
  return (cx >= 0 && cx < grid_w(t) && cy >= 0 && cy < grid_h(t)) ? cy * grid_w(t) + cx : -1;     // at most 1025^2 cells
}

// The slots in use: the total of the caller's scan, never more than the table holds.
__device__ __forceinline__ long long slots_of(const Topo &t) {
  const long long n = t.new_ptr[t.A];
  return n < 0 ? 0 : (n > t.Va ? t.Va : n);
}

// The arc as dm_simplify_chains sees it: a closed arc drops a stored start that is no node and lies inside a straight run.
__device__ __forceinline__ bool drops_start(const Arc &c, const KeepRead &K) {
  if (!c.closed) return false;
  int x0, y0, x1, y1, x2, y2;
  vertex(c, c.len - 1, x0, y0);
  vertex(c, 0, x1, y1);
  vertex(c, 1, x2, y2);
  const long long at = K.at(c, 0, x1, y1);
  const bool node = at >= 0 && K.keep[at] == 2;
  return !node && (long long)(x1 - x0) * (y2 - y1) == (long long)(y1 - y0) * (x2 - x1);
}

// ---- fixed points ------------------------------------------------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(256) void topo_points_kernel(Topo t) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const KeepRead K{t.keep, t.H, t.W};
  auto put = [&](int x, int y) {
    const int cell = cell_of(t, x >> LOG2, y >> LOG2);
    if (cell < 0) return;
    if (!FILL) {
      atomicAdd(t.point_count + cell, 1);
    } else {
      const long long first = t.point_ptr[cell], end = t.point_ptr[cell + 1];
      const long long slot = first + atomicAdd(t.point_fill + cell, 1);
      if (first >= 0 && slot < end && end <= t.Va) { t.point_xy[2 * slot] = x; t.point_xy[2 * slot + 1] = y; }
    }
  };
  for (int a = blockIdx.x * WAVES + wave; a < t.A; a += gridDim.x * WAVES) {
    Arc c;
    if (!arc_of(t.arc_xy, (const long long *)t.arc_ptr, a, t.Va, c)) continue;
    if (drops_start(c, K)) { c.skip = 1; c.len -= 1; }
    if (c.len < 2) continue;
    bool bad = false, any = false;
    KeepRead::Anchor anchor;
    for (int p = lane; p < c.len; p += 64) {                       // the first pass only looks: an arc dm_simplify_chains refuses has no points
      int x, y;
      vertex(c, p, x, y);
      const long long at = K.at(c, p, x, y);
      if (at < 0) { bad = true; continue; }
      any |= K.keep[at] == 2;
      anchor.see(K, at, x, y, p);
    }
    if (__any(bad)) continue;
    if (__any(any)) {
      for (int p = lane; p < c.len; p += 64) {
        int x, y;
        vertex(c, p, x, y);
        if (K.keep[K.at(c, p, x, y)] == 2) put(x, y);
      }
    } else if (c.closed) {
      long long at;
      const int p = anchor.reduce(K, c, at);
      if (lane == 0) {
        int x, y;
        vertex(c, p, x, y);
        put(x, y);
      }
    }
  }
}

// ---- the segment table -------------------------------------------------------------------------------------------------------------
// Slot e is an int4: (tag = 2 arc + skip, position, x, y); tag -1 for a slot nothing wrote.
__global__ __launch_bounds__(256) void topo_segments_kernel(Topo t) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const KeepRead K{t.keep, t.H, t.W};
  const long long Vn = slots_of(t);
  int4 *const table = reinterpret_cast<int4 *>(t.seg);
  for (int a = blockIdx.x * WAVES + wave; a < t.A; a += gridDim.x * WAVES) {
    Arc c;
    if (!arc_of(t.arc_xy, (const long long *)t.arc_ptr, a, t.Va, c)) continue;
    const long long to = t.new_ptr[a], room = t.new_ptr[a + 1] - to;
    if (to < 0 || room < 0 || to + room > Vn) continue;
    const int skip = (drops_start(c, K) && c.len - 1 >= 2) ? 1 : 0;
    const int tag = 2 * a + skip;
    int total = 0, fx = 0, fy = 0, fp = 0;
    for (int base = 0; base < c.len; base += 64) {               // the walk of simplify_arc_kernel: stored order, the stored start included
      const int p = base + lane;
      int x = 0, y = 0;
      bool kept = false;
      if (p < c.len) {
        vertex(c, p, x, y);
        const long long at = K.at(c, p, x, y);
        kept = at >= 0 && K.keep[at] != 0;
      }
      const u64 m = __ballot(kept);
      const int rank = total + __popcll(m & ((1ULL << lane) - 1));
      if (kept && rank < room) table[to + rank] = make_int4(tag, p - skip, x, y);
      if (total == 0 && m) {
        const int src = __ffsll((unsigned long long)m) - 1;
        fx = __shfl(x, src, 64);
        fy = __shfl(y, src, 64);
        fp = __shfl(p, src, 64);
      }
      total += __popcll(m);
    }
    if (c.closed && total > 0 && total < room && lane == 0) table[to + total] = make_int4(tag, fp - skip + (c.len - skip), fx, fy);
  }
}

// Segment e: slots e and e + 1 of one arc.  False for a slot that starts none or holds what the tables cannot.
struct Segment {
  int arc, skip, i, j, ax, ay, bx, by;
};

__device__ __forceinline__ bool segment_of(const Topo &t, long long e, long long Vn, Segment &s) {
  if (e < 0 || e + 1 >= Vn) return false;
  const int4 *const table = reinterpret_cast<const int4 *>(t.seg);
  const int4 u = table[e], w = table[e + 1];
  if (u.x < 0 || u.x != w.x || (u.x >> 1) >= t.A) return false;
  if (u.z < 0 || u.z > t.W || u.w < 0 || u.w > t.H || w.z < 0 || w.z > t.W || w.w < 0 || w.w > t.H) return false;
  if (u.y < 0 || w.y <= u.y) return false;
  s.arc = u.x >> 1; s.skip = u.x & 1; s.i = u.y; s.j = w.y;
  s.ax = u.z; s.ay = u.w; s.bx = w.z; s.by = w.w;
  return true;
}

// The arc of a segment with its positions checked against it: i < len, j <= i + len.
__device__ __forceinline__ bool arc_of_segment(const Topo &t, const Segment &s, Arc &c) {
  if (!arc_of(t.arc_xy, (const long long *)t.arc_ptr, s.arc, t.Va, c)) return false;
  if (s.skip) { if (!c.closed) return false; c.skip = 1; c.len -= 1; }
  if (c.len < 2 || s.i >= c.len || s.j > (c.closed ? s.i + c.len : c.len - 1)) return false;
  return true;
}

template <bool FILL>
__global__ void topo_bin_kernel(Topo t) {
  const long long Vn = slots_of(t);
  const int cells = grid_w(t) * grid_h(t);
  if (FILL && blockIdx.x == 0 && threadIdx.x == 0) {
    const long long need = t.cell_ptr[cells];
    t.status[2] = need < 0 ? INT_MAX : (need > INT_MAX ? INT_MAX : (int)need);
  }
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < Vn; e += (long long)gridDim.x * blockDim.x) {
    Segment s;
    const bool ok = segment_of(t, e, Vn, s);
    const bool flat = ok && s.ax == s.bx && s.ay == s.by;
    if (!FILL) t.kind[e] = flat ? 1 : 0;
    if (!ok || flat) continue;
    dm_topo_walk_cells(s.ax, s.ay, s.bx, s.by, LOG2, [&](int cx, int cy) {
      const int cell = cell_of(t, cx, cy);
      if (cell < 0) return;
      if (!FILL) {
        atomicAdd(t.cell_count + cell, 1);
      } else {
        const long long first = t.cell_ptr[cell], end = t.cell_ptr[cell + 1];
        const long long slot = first + atomicAdd(t.cell_fill + cell, 1);
        if (first >= 0 && slot < end && end <= t.cap) t.cell_seg[slot] = (int)e;
      }
    });
  }
}

// ---- flags -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topo_pairs_kernel(Topo t) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long Vn = slots_of(t);
  const int cells = grid_w(t) * grid_h(t);
  for (int cell = blockIdx.x * WAVES + wave; cell < cells; cell += gridDim.x * WAVES) {
    const long long first = t.cell_ptr[cell], end = t.cell_ptr[cell + 1];
    if (first < 0 || end < first || end > t.cap || end - first < 2) continue;
    const int n = (int)(end - first);
    for (int base = 0; base < n; base += 64) {                   // a lane per segment of the cell, 64 at a time
      const int m = base + lane;
      Segment s;
      int e = -1;
      bool live = false;
      if (m < n) {
        e = t.cell_seg[first + m];
        live = segment_of(t, e, Vn, s);
      }
      bool hit = false;
      for (int k = 0; k < n; ++k) {                              // every other one, in step over the wave
        const int f = t.cell_seg[first + k];
        Segment o;
        if (!segment_of(t, f, Vn, o) || (o.ax == o.bx && o.ay == o.by)) continue;
        if (live && !hit && f != e) hit = dm_topo_meets(s.ax, s.ay, s.bx, s.by, o.ax, o.ay, o.bx, o.by);
      }
      if (hit) atomicOr(t.kind + e, 1);
    }
  }
}

__global__ __launch_bounds__(256) void topo_jumps_kernel(Topo t) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long Vn = slots_of(t);
  for (long long e = (long long)blockIdx.x * WAVES + wave; e < Vn; e += (long long)gridDim.x * WAVES) {
    Segment s;
    Arc c;
    if (!segment_of(t, e, Vn, s) || s.j - s.i < 2 || !arc_of_segment(t, s, c)) continue;
    int xmin = min(s.ax, s.bx), xmax = max(s.ax, s.bx), ymin = min(s.ay, s.by), ymax = max(s.ay, s.by);
    for (int k = s.i + 1 + lane; k < s.j; k += 64) {
      int x, y;
      vertex(c, k, x, y);
      xmin = min(xmin, x); xmax = max(xmax, x); ymin = min(ymin, y); ymax = max(ymax, y);
    }
    xmin = max(wave_min(xmin), 0); ymin = max(wave_min(ymin), 0);
    xmax = min(wave_max(xmax), t.W); ymax = min(wave_max(ymax), t.H);
    bool jumped = false;
    for (int cy = ymin >> LOG2; cy <= (ymax >> LOG2) && !jumped; ++cy) {
      for (int cx = xmin >> LOG2; cx <= (xmax >> LOG2) && !jumped; ++cx) {
        const int cell = cell_of(t, cx, cy);
        if (cell < 0) continue;
        const long long first = t.point_ptr[cell], end = t.point_ptr[cell + 1];
        if (first < 0 || end < first || end > t.Va) continue;
        for (long long base = first; base < end && !jumped; base += 64) {
          const long long m = base + lane;
          int px = 0, py = 0;
          bool cand = false;
          if (m < end) {
            px = t.point_xy[2 * m];
            py = t.point_xy[2 * m + 1];
            cand = px >= xmin && px <= xmax && py >= ymin && py <= ymax && !(px == s.ax && py == s.ay) && !(px == s.bx && py == s.by);
          }
          if (!__any(cand)) continue;
          int crossings = 0, ux = s.ax, uy = s.ay;
          for (int k = s.i + 1; k <= s.j + 1; ++k) {               // the edges v[i] v[i+1] .. v[j-1] v[j], then v[j] v[i]
            int wx = s.ax, wy = s.ay;
            if (k <= s.j) vertex(c, k, wx, wy);
            crossings += cand && dm_topo_edge_counts(ux, uy, wx, wy, px, py);
            ux = wx;
            uy = wy;
          }
          jumped = __any(crossings & 1);
        }
      }
    }
    if (jumped && lane == 0) atomicOr(t.kind + e, 2);
  }
}

// ---- tally and refine --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topo_refine_kernel(Topo t, int apply) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long Vn = slots_of(t);
  const CornerKeep<unsigned char> K{t.keep, t.H, t.W};
  const bool whole = t.status[2] <= t.cap;                       // a cell list that did not fit: the flags are not all there, keep nothing
  const u64 q2 = (u64)t.q * (u64)t.q;
  for (long long e = (long long)blockIdx.x * WAVES + wave; e < Vn; e += (long long)gridDim.x * WAVES) {
    if (t.kind[e] == 0) continue;
    Segment s;
    Arc c;
    const bool inner = segment_of(t, e, Vn, s) && s.j - s.i > 1 && arc_of_segment(t, s, c);
    if (lane == 0) {
      atomicAdd(t.status, 1);
      if (inner) atomicAdd(t.status + 1, 1);
    }
    if (!inner || !apply || !whole) continue;
    int xi, yi, xj, yj;
    vertex(c, s.i, xi, yi);
    vertex(c, s.j, xj, yj);
    const long long dx = xj - xi, dy = yj - yi;
    const u64 len2 = (u64)(dx * dx + dy * dy);
    u64 best = 0;                                                // the arg-max of split_chain: d << 32 | ~(k - i)
    for (int k = s.i + 1 + lane; k < s.j; k += 64) {
      int x, y;
      vertex(c, k, x, y);
      const long long rx = x - xi, ry = y - yi;
      const long long cr = dx * ry - dy * rx;
      const u64 d = len2 == 0 ? (u64)(rx * rx + ry * ry) : (u64)(cr < 0 ? -cr : cr);
      const u64 key = (d << 32) | (u64)(0xffffffffu - (unsigned)(k - s.i));
      best = key > best ? key : best;
    }
    best = wave_max(best);
    const int k = s.i + (int)(0xffffffffu - (unsigned)(best & 0xffffffffu));
    if (k <= s.i || k >= s.j) continue;
    if (lane == 0) {
      int x, y;
      vertex(c, k, x, y);
      const long long at = K.at(c, k, x, y);
      if (at >= 0) K.keep[at] = 1;
    }
    // the segment's share of the workspace: two entries per stored vertex of its arc, from its logical start; j - i entries hold
    // the walk of either half (dm_simplify_arcs.h), and the segments of one arc are disjoint in [0, 2 len)
    long long *const stk = (long long *)t.stack + 2 * c.first + s.i;
    split_chain(c, s.i, k, K, q2, stk, s.j - s.i, lane);
    split_chain(c, k, s.j, K, q2, stk, s.j - s.i, lane);
  }
}

__global__ void topo_clear_kernel(int *__restrict__ a, int *__restrict__ b, int n, int *__restrict__ status) {
  if (status && blockIdx.x == 0 && threadIdx.x < 4) status[threadIdx.x] = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { a[i] = 0; b[i] = 0; }
}

inline int cells_of(int H, int W) { return ((H >> LOG2) + 1) * ((W >> LOG2) + 1); }

}  // namespace

// What every entry asks of the struct; `tables`: the round's arrays beyond the fixed points'.
static int topology_ok(const char *what, const DmSimplifyTopology *t, bool tables) {
  DM_REQUIRE(t, DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  DM_REQUIRE(t->arc_xy && t->arc_ptr && t->keep && t->point_count && t->point_fill, DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  DM_REQUIRE(!tables || (t->new_ptr && t->seg && t->kind && t->cell_count && t->cell_fill && t->status), DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  DM_REQUIRE(t->H > 0 && t->W > 0 && t->H <= DM_SIMPLIFY_MAX_SIDE && t->W <= DM_SIMPLIFY_MAX_SIDE && t->A > 0 && t->Va >= 2 && t->Va <= (1LL << 30),
             DM_ERR_BAD_SHAPE, "%s: bad sizes (H=%d W=%d A=%d Va=%lld; need 1 <= H, W <= 32768, A >= 1, 2 <= Va <= 2^30)", what, t->H, t->W, t->A,
             (long long)t->Va);
  DM_REQUIRE(t->q >= 0 && t->q <= DM_SIMPLIFY_MAX_Q, DM_ERR_BAD_SHAPE, "%s: bad tolerance (q=%d; need 0 <= q <= 2^20)", what, t->q);
  DM_REQUIRE(!tables || (t->cap >= 1 && t->cap <= INT32_MAX), DM_ERR_BAD_SHAPE, "%s: bad sizes (cap=%lld; need 1 <= cap < 2^31)", what,
             (long long)t->cap);
  return DM_OK;
}

#define TOPO_STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" int dm_simplify_topology_point_count(const DmSimplifyTopology *t, void *stream) {
  if (int rc = topology_ok("dm_simplify_topology_point_count", t, false)) return rc;
  const int cells = cells_of(t->H, t->W);
  hipLaunchKernelGGL(topo_clear_kernel, dim3(grid_for(cells)), dim3(256), 0, TOPO_STREAM, t->point_count, t->point_fill, cells, (int *)nullptr);
  hipLaunchKernelGGL(topo_points_kernel<false>, dim3(wave_grid(t->A)), dim3(256), 0, TOPO_STREAM, *t);
  DM_LAUNCH_CHECK("dm_simplify_topology_point_count");
  return DM_OK;
}

extern "C" int dm_simplify_topology_point_fill(const DmSimplifyTopology *t, void *stream) {
  if (int rc = topology_ok("dm_simplify_topology_point_fill", t, false)) return rc;
  DM_REQUIRE(t->point_ptr && t->point_xy, DM_ERR_BAD_SHAPE, "dm_simplify_topology_point_fill: null pointer");
  hipLaunchKernelGGL(topo_points_kernel<true>, dim3(wave_grid(t->A)), dim3(256), 0, TOPO_STREAM, *t);
  DM_LAUNCH_CHECK("dm_simplify_topology_point_fill");
  return DM_OK;
}

extern "C" int dm_simplify_topology_segments(const DmSimplifyTopology *t, void *stream) {
  if (int rc = topology_ok("dm_simplify_topology_segments", t, true)) return rc;
  const int cells = cells_of(t->H, t->W);
  hipLaunchKernelGGL(topo_clear_kernel, dim3(grid_for(cells)), dim3(256), 0, TOPO_STREAM, t->cell_count, t->cell_fill, cells, t->status);
  hipLaunchKernelGGL(topo_segments_kernel, dim3(wave_grid(t->A)), dim3(256), 0, TOPO_STREAM, *t);
  DM_LAUNCH_CHECK("dm_simplify_topology_segments");
  return DM_OK;
}

extern "C" int dm_simplify_topology_bin_count(const DmSimplifyTopology *t, void *stream) {
  if (int rc = topology_ok("dm_simplify_topology_bin_count", t, true)) return rc;
  hipLaunchKernelGGL(topo_bin_kernel<false>, dim3(grid_for(t->Va)), dim3(256), 0, TOPO_STREAM, *t);
  DM_LAUNCH_CHECK("dm_simplify_topology_bin_count");
  return DM_OK;
}

extern "C" int dm_simplify_topology_bin_fill(const DmSimplifyTopology *t, void *stream) {
  if (int rc = topology_ok("dm_simplify_topology_bin_fill", t, true)) return rc;
  DM_REQUIRE(t->cell_ptr && t->cell_seg, DM_ERR_BAD_SHAPE, "dm_simplify_topology_bin_fill: null pointer");
  hipLaunchKernelGGL(topo_bin_kernel<true>, dim3(grid_for(t->Va)), dim3(256), 0, TOPO_STREAM, *t);
  DM_LAUNCH_CHECK("dm_simplify_topology_bin_fill");
  return DM_OK;
}

extern "C" int dm_simplify_topology_pairs(const DmSimplifyTopology *t, void *stream) {
  if (int rc = topology_ok("dm_simplify_topology_pairs", t, true)) return rc;
  DM_REQUIRE(t->cell_ptr && t->cell_seg, DM_ERR_BAD_SHAPE, "dm_simplify_topology_pairs: null pointer");
  hipLaunchKernelGGL(topo_pairs_kernel, dim3(wave_grid(cells_of(t->H, t->W))), dim3(256), 0, TOPO_STREAM, *t);
  DM_LAUNCH_CHECK("dm_simplify_topology_pairs");
  return DM_OK;
}

extern "C" int dm_simplify_topology_jumps(const DmSimplifyTopology *t, void *stream) {
  if (int rc = topology_ok("dm_simplify_topology_jumps", t, true)) return rc;
  DM_REQUIRE(t->point_ptr && t->point_xy, DM_ERR_BAD_SHAPE, "dm_simplify_topology_jumps: null pointer");
  hipLaunchKernelGGL(topo_jumps_kernel, dim3(grid_for(t->Va * 64, 8192)), dim3(256), 0, TOPO_STREAM, *t);
  DM_LAUNCH_CHECK("dm_simplify_topology_jumps");
  return DM_OK;
}

extern "C" int dm_simplify_topology_refine(const DmSimplifyTopology *t, int32_t apply, void *stream) {
  if (int rc = topology_ok("dm_simplify_topology_refine", t, true)) return rc;
  DM_REQUIRE(apply == 0 || t->stack, DM_ERR_BAD_SHAPE, "dm_simplify_topology_refine: null pointer");
  hipLaunchKernelGGL(topo_refine_kernel, dim3(grid_for(t->Va * 64, 8192)), dim3(256), 0, TOPO_STREAM, *t, (int)apply);
  DM_LAUNCH_CHECK("dm_simplify_topology_refine");
  return DM_OK;
}
