// The integer predicates and the cell walk of dm_simplify_topology_kernels.h, shared with the host checks
// tools/simplify_topology_host_check.cpp and tools/scene_simplify_topology_host_check.cpp.  The rule: include/deepmerge_hip.h,
// DESIGN.md 3.5.12; tests/simplify_topology_ref.py restates it.
// Arithmetic.  Coordinates are int32 in [0, 2^31 - 2] (one raster: 0 .. 32768), so every difference of two fits an int, every
// product of two differences is below 2^62 and every difference of two such products below 2^63: nothing below overflows 64 bits.
// What is actually met is far smaller: two segments that share a cell, or a fixed point inside a sub-chain's box, have a segment or
// chain extent of at most 32768 (DM_SIMPLIFY_MAX_SIDE, the arc-extent limit) as one factor of each product and a difference below
// 2^32 as the other, so every orient term is below 2^48.
#pragma once
#include "dm_simplify.h"

// (b - a) x (c - a)
DM_HD static inline long long dm_topo_orient(int ax, int ay, int bx, int by, int cx, int cy) {
  return (long long)(bx - ax) * (cy - ay) - (long long)(by - ay) * (cx - ax);
}

// (px, py) lies on the closed segment (a, b) and is neither a nor b.
DM_HD static inline bool dm_topo_inner(int ax, int ay, int bx, int by, int px, int py) {
  if (dm_topo_orient(ax, ay, bx, by, px, py) != 0) return false;
  if (px < (ax < bx ? ax : bx) || px > (ax < bx ? bx : ax) || py < (ay < by ? ay : by) || py > (ay < by ? by : ay)) return false;
  return !(px == ax && py == ay) && !(px == bx && py == by);
}

// Two non-degenerate segments (a, b), (c, d) share a point that is not an end of both: the same two ends, a proper crossing, or
// an end of one on the other that is no end of that other.
DM_HD static inline bool dm_topo_meets(int ax, int ay, int bx, int by, int cx, int cy, int dx, int dy) {
  if ((ax == cx && ay == cy && bx == dx && by == dy) || (ax == dx && ay == dy && bx == cx && by == cy)) return true;
  const long long o1 = dm_topo_orient(ax, ay, bx, by, cx, cy), o2 = dm_topo_orient(ax, ay, bx, by, dx, dy);
  const long long o3 = dm_topo_orient(cx, cy, dx, dy, ax, ay), o4 = dm_topo_orient(cx, cy, dx, dy, bx, by);
  if (((o1 > 0 && o2 < 0) || (o1 < 0 && o2 > 0)) && ((o3 > 0 && o4 < 0) || (o3 < 0 && o4 > 0))) return true;
  return dm_topo_inner(ax, ay, bx, by, cx, cy) || dm_topo_inner(ax, ay, bx, by, dx, dy) || dm_topo_inner(cx, cy, dx, dy, ax, ay) ||
         dm_topo_inner(cx, cy, dx, dy, bx, by);
}

// The even-odd count's term of polygon edge (u, w) for the point p, half-open in y.
DM_HD static inline bool dm_topo_edge_counts(int ux, int uy, int wx, int wy, int px, int py) {
  if ((uy <= py) == (wy <= py)) return false;
  const long long o = dm_topo_orient(ux, uy, wx, wy, px, py);
  return wy > uy ? o > 0 : o < 0;
}

// floor(a / b), b > 0
DM_HD static inline long long dm_topo_floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// Calls f(cx, cy) for a set of grid cells (side 2^log2, cell of a point = its coordinates >> log2) that holds the cell of every
// point of the closed segment (x0, y0) - (x1, y1): per cell column the segment crosses, the rows between its heights at the
// column's two sides.  At most |dx| / side + |dy| / side + 3 columns and rows in all: the walk follows the segment, not its box.
template <typename F>
DM_HD static inline void dm_topo_walk_cells(int x0, int y0, int x1, int y1, int log2, F f) {
  if (x0 > x1) { int t = x0; x0 = x1; x1 = t; t = y0; y0 = y1; y1 = t; }
  const long long dx = x1 - x0, dy = y1 - y0;
  for (int cx = x0 >> log2; cx <= (x1 >> log2); ++cx) {
    int lo, hi;
    if (dx == 0) {
      lo = y0 < y1 ? y0 : y1;
      hi = y0 < y1 ? y1 : y0;
    } else {
      // cx <= x1 >> log2, so cx << log2 <= x1 < 2^31 fits the int it is formed in, at any log2; dy xa and dy xb are below 2^62
      const long long left = cx << log2, right = left + (1LL << log2);
      const long long xa = (left > x0 ? left : x0) - x0, xb = (right < x1 ? right : x1) - x0;
      const int ya = y0 + (int)dm_topo_floor_div(dy * xa, dx), yb = y0 + (int)dm_topo_floor_div(dy * xb, dx);
      lo = ya < yb ? ya : yb;
      hi = ya < yb ? yb : ya;
    }
    for (int cy = lo >> log2; cy <= (hi >> log2); ++cy) f(cx, cy);
  }
}
