// The kernels of topology-safe simplification, once for its two forms: dm_simplify_topology.hip, one
// raster, keep flags per pixel corner (CornerKeep) on a grid of 32-corner cells; dm_scene_simplify_topology.hip, a scene, keep flags
// per stored arc vertex (VertexKeep) on a grid whose cell side is a field of the struct.  A form F names the struct its entries
// take, the keep accessor of dm_simplify_arcs.h and the cell side:
//   F::Struct                      DmSimplifyTopology / DmSceneSimplifyTopology: the same fields but for the keep array and cell_log2
//   F::Keep, F::KeepRead           the accessor on unsigned char / const unsigned char;  F::keep(t), F::keep_read(t) build one
//   F::log2(t)                     log2 of the cell side: a compile-time constant or t.cell_log2
// The accessor decides four things: where a vertex's flag lives (K.at, by corner or by position), the anchor of a closed arc without
// a node (K's Anchor), and, where KeepRead::EXTENT, that an arc or sub-chain wider than DM_SIMPLIFY_MAX_SIDE is refused as
// dm_simplify_chains refuses it.  With CornerKeep every EXTENT branch is compiled out and the arithmetic is what
// dm_simplify_topology.hip always performed.
//
// Arithmetic (the scene form; the one-raster form is the special case H, W <= 32768).  Coordinates are int32 in [0, 2^31 - 2]:
// every difference of two fits an int, every product of two differences is below 2^62 and every orient (a difference of two such
// products) below 2^63, so nothing here overflows whatever the tables hold.  What the RULE needs is narrower and is kept by the
// extent limit: within a sub-chain of extent <= 32768 every |cross| is below 2^31, so refine's key d << 32 | ~(k - i) holds d whole.
//   points     once per call, one wavefront per arc: its nodes (keep == 2) or, on a closed arc without one, its anchor, binned by
//              grid cell (count, the caller's scan, fill).  A node is an end of several arcs and is binned once per arc: the jump
//              test is an OR over the points, so copies change nothing
//   segments   per round, one wavefront per arc: slot e of the table is vertex e of the simplified arcs the arc emit kernel would
//              write (arc, skip, logical position in the arc as the chains kernel sees it, corner); segment e joins slots e and
//              e + 1 of one arc, so the last slot of every arc starts no segment
//   bin_count  per slot: kind = 1 for a degenerate segment, else 0; every other segment adds 1 to the cells it passes through
//   bin_fill   the same walk, writing the slot into its cells (the order within a cell is the order of arrival; nothing reads it)
//   pairs      one wavefront per cell: a lane per registered segment against every other one of the cell; atomicOr of kind bit 1
//   jumps      one wavefront per segment with interior vertices: the fixed points of the cells under the sub-chain's bounding box,
//              a lane per point, the polygon's edges in step over the wave; atomicOr of kind bit 2
//   refine     one wavefront per slot: tallies the flagged segments and, for one with interior vertices, keeps the arg-max and
//              runs split_chain (dm_simplify_arcs.h) on both halves.  It stores keep = 1 only at interior vertices of its own
//              segment, which no other segment holds, and reads no keep: no races
// Work follows the segments and points per cell; only the per-cell counters are as many as the grid has cells.  The flags are ORs
// over all pairs that share a cell and dm_topo_walk_cells covers the cell of every point of a segment, so two segments that share
// a point share a cell whatever the cell side: the result does not depend on it.
#pragma once
#include "dm_simplify_arcs.h"
#include "dm_simplify_topology.h"

namespace {

// Cells per row and column, and the id of cell (cx, cy): -1 outside the grid.  The entries refuse a grid of more than 2^22 cells
// (the dense form has at most 1025^2), so grid_w grid_h and every id fit an int.
template <typename F>
__host__ __device__ __forceinline__ int grid_w(const typename F::Struct &t) { return (t.W >> F::log2(t)) + 1; }
template <typename F>
__host__ __device__ __forceinline__ int grid_h(const typename F::Struct &t) { return (t.H >> F::log2(t)) + 1; }
template <typename F>
__device__ __forceinline__ int cell_of(const typename F::Struct &t, int cx, int cy) {
  return (cx >= 0 && cx < grid_w<F>(t) && cy >= 0 && cy < grid_h<F>(t)) ? cy * grid_w<F>(t) + cx : -1;
}

// The slots in use: the total of the caller's scan, never more than the table holds.
template <typename T>
__device__ __forceinline__ long long slots_of(const T &t) {
  const long long n = t.new_ptr[t.A];
  return n < 0 ? 0 : (n > t.Va ? t.Va : n);
}

// The arc as the chains kernel sees it: a closed arc drops a stored start that is no node and lies inside a straight run.
template <typename KeepRead>
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
template <typename F, bool FILL>
__global__ __launch_bounds__(256) void topo_points_kernel(typename F::Struct t) {
  typedef typename F::KeepRead KeepRead;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int log2 = F::log2(t);
  const KeepRead K = F::keep_read(t);
  auto put = [&](int x, int y) {
    const int cell = cell_of<F>(t, x >> log2, y >> log2);
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
    typename KeepRead::Anchor anchor;
    int xmin = INT_MAX, xmax = INT_MIN, ymin = INT_MAX, ymax = INT_MIN;
    for (int p = lane; p < c.len; p += 64) {                       // the first pass only looks: an arc the chains kernel refuses has no points
      int x, y;
      vertex(c, p, x, y);
      const long long at = K.at(c, p, x, y);
      if (at < 0) { bad = true; continue; }
      any |= K.keep[at] == 2;
      anchor.see(K, at, x, y, p);
      if (KeepRead::EXTENT) { xmin = min(xmin, x); xmax = max(xmax, x); ymin = min(ymin, y); ymax = max(ymax, y); }
    }
    if (__any(bad)) continue;
    if (KeepRead::EXTENT) {                                        // the chains kernel's limit, in its words
      const long long w = (long long)wave_max(xmax) - wave_min(xmin), h = (long long)wave_max(ymax) - wave_min(ymin);
      if (w > MAX_SIDE || h > MAX_SIDE) continue;
    }
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
// Slot e is an int4: (tag = 2 arc + skip, position, x, y); tag -1 for a slot nothing wrote.  The entries refuse A >= 2^30 (the
// dense form's arcs are fewer than its 2^30 vertices), so the tag fits an int.
template <typename F>
__global__ __launch_bounds__(256) void topo_segments_kernel(typename F::Struct t) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const typename F::KeepRead K = F::keep_read(t);
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

template <typename T>
__device__ __forceinline__ bool segment_of(const T &t, long long e, long long Vn, Segment &s) {
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
template <typename T>
__device__ __forceinline__ bool arc_of_segment(const T &t, const Segment &s, Arc &c) {
  if (!arc_of(t.arc_xy, (const long long *)t.arc_ptr, s.arc, t.Va, c)) return false;
  if (s.skip) { if (!c.closed) return false; c.skip = 1; c.len -= 1; }
  if (c.len < 2 || s.i >= c.len || s.j > (c.closed ? s.i + c.len : c.len - 1)) return false;
  return true;
}

template <typename F, bool FILL>
__global__ void topo_bin_kernel(typename F::Struct t) {
  const long long Vn = slots_of(t);
  const int cells = grid_w<F>(t) * grid_h<F>(t);                  // at most 2^22: the entries checked the product in 64 bits
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
    dm_topo_walk_cells(s.ax, s.ay, s.bx, s.by, F::log2(t), [&](int cx, int cy) {
      const int cell = cell_of<F>(t, cx, cy);
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
template <typename F>
__global__ __launch_bounds__(256) void topo_pairs_kernel(typename F::Struct t) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long Vn = slots_of(t);
  const int cells = grid_w<F>(t) * grid_h<F>(t);
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

template <typename F>
__global__ __launch_bounds__(256) void topo_jumps_kernel(typename F::Struct t) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int log2 = F::log2(t);
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
    xmin = wave_min(xmin); ymin = wave_min(ymin); xmax = wave_max(xmax); ymax = wave_max(ymax);
    // a sub-chain the chains kernel would refuse (a vertex outside the scene, wider than the limit) jumps over nothing: one factor of
    // every orient term below is then an extent of at most 32768
    if (F::KeepRead::EXTENT && (xmin < 0 || ymin < 0 || xmax > t.W || ymax > t.H || (long long)xmax - xmin > MAX_SIDE || (long long)ymax - ymin > MAX_SIDE))
      continue;
    xmin = max(xmin, 0); ymin = max(ymin, 0);
    xmax = min(xmax, t.W); ymax = min(ymax, t.H);
    bool jumped = false;
    for (int cy = ymin >> log2; cy <= (ymax >> log2) && !jumped; ++cy) {
      for (int cx = xmin >> log2; cx <= (xmax >> log2) && !jumped; ++cx) {
        const int cell = cell_of<F>(t, cx, cy);
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
template <typename F>
__global__ __launch_bounds__(256) void topo_refine_kernel(typename F::Struct t, int apply) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long Vn = slots_of(t);
  const typename F::Keep K = F::keep(t);
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
    if (F::Keep::EXTENT) {                                       // |cross| < 2^31 needs the sub-chain's box within 32768 x 32768: else left alone
      int xmin = min(xi, xj), xmax = max(xi, xj), ymin = min(yi, yj), ymax = max(yi, yj);
      for (int k = s.i + 1 + lane; k < s.j; k += 64) {
        int x, y;
        vertex(c, k, x, y);
        xmin = min(xmin, x); xmax = max(xmax, x); ymin = min(ymin, y); ymax = max(ymax, y);
      }
      const long long w = (long long)wave_max(xmax) - wave_min(xmin), h = (long long)wave_max(ymax) - wave_min(ymin);
      if (w > MAX_SIDE || h > MAX_SIDE) continue;
    }
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

// ---- the eight entries of a form -----------------------------------------------------------------------------------------------------
// F::ok(what, t, tables) is what every entry asks of the struct; `tables`: the round's arrays beyond the fixed points'.  It bounds
// the grid, so cells_of fits an int.
template <typename F>
inline int cells_of(const typename F::Struct *t) { return grid_w<F>(*t) * grid_h<F>(*t); }

#define TOPO_STREAM reinterpret_cast<hipStream_t>(stream)

template <typename F>
inline int topo_point_count(const char *what, const typename F::Struct *t, void *stream) {
  if (int rc = F::ok(what, t, false)) return rc;
  const int cells = cells_of<F>(t);
  hipLaunchKernelGGL(topo_clear_kernel, dim3(grid_for(cells)), dim3(256), 0, TOPO_STREAM, t->point_count, t->point_fill, cells, (int *)nullptr);
  hipLaunchKernelGGL((topo_points_kernel<F, false>), dim3(wave_grid(t->A)), dim3(256), 0, TOPO_STREAM, *t);
  DM_LAUNCH_CHECK(what);
  return DM_OK;
}

template <typename F>
inline int topo_point_fill(const char *what, const typename F::Struct *t, void *stream) {
  if (int rc = F::ok(what, t, false)) return rc;
  DM_REQUIRE(t->point_ptr && t->point_xy, DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  hipLaunchKernelGGL((topo_points_kernel<F, true>), dim3(wave_grid(t->A)), dim3(256), 0, TOPO_STREAM, *t);
  DM_LAUNCH_CHECK(what);
  return DM_OK;
}

template <typename F>
inline int topo_segments(const char *what, const typename F::Struct *t, void *stream) {
  if (int rc = F::ok(what, t, true)) return rc;
  const int cells = cells_of<F>(t);
  hipLaunchKernelGGL(topo_clear_kernel, dim3(grid_for(cells)), dim3(256), 0, TOPO_STREAM, t->cell_count, t->cell_fill, cells, t->status);
  hipLaunchKernelGGL(topo_segments_kernel<F>, dim3(wave_grid(t->A)), dim3(256), 0, TOPO_STREAM, *t);
  DM_LAUNCH_CHECK(what);
  return DM_OK;
}

template <typename F, bool FILL>
inline int topo_bin(const char *what, const typename F::Struct *t, void *stream) {
  if (int rc = F::ok(what, t, true)) return rc;
  DM_REQUIRE(!FILL || (t->cell_ptr && t->cell_seg), DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  hipLaunchKernelGGL((topo_bin_kernel<F, FILL>), dim3(grid_for(t->Va)), dim3(256), 0, TOPO_STREAM, *t);
  DM_LAUNCH_CHECK(what);
  return DM_OK;
}

template <typename F>
inline int topo_pairs(const char *what, const typename F::Struct *t, void *stream) {
  if (int rc = F::ok(what, t, true)) return rc;
  DM_REQUIRE(t->cell_ptr && t->cell_seg, DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  hipLaunchKernelGGL(topo_pairs_kernel<F>, dim3(wave_grid(cells_of<F>(t))), dim3(256), 0, TOPO_STREAM, *t);
  DM_LAUNCH_CHECK(what);
  return DM_OK;
}

template <typename F>
inline int topo_jumps(const char *what, const typename F::Struct *t, void *stream) {
  if (int rc = F::ok(what, t, true)) return rc;
  DM_REQUIRE(t->point_ptr && t->point_xy, DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  hipLaunchKernelGGL(topo_jumps_kernel<F>, dim3(grid_for(t->Va * 64, 8192)), dim3(256), 0, TOPO_STREAM, *t);
  DM_LAUNCH_CHECK(what);
  return DM_OK;
}

template <typename F>
inline int topo_refine(const char *what, const typename F::Struct *t, int32_t apply, void *stream) {
  if (int rc = F::ok(what, t, true)) return rc;
  DM_REQUIRE(apply == 0 || t->stack, DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  hipLaunchKernelGGL(topo_refine_kernel<F>, dim3(grid_for(t->Va * 64, 8192)), dim3(256), 0, TOPO_STREAM, *t, (int)apply);
  DM_LAUNCH_CHECK(what);
  return DM_OK;
}

}  // namespace
