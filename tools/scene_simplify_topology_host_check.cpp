// Host check of csrc/dm_scene_simplify_topology.hip for a sanitizer build: a stand-alone program, nothing of it is loaded into Python
// and it needs no GPU (every call below returns from its argument validation, before any launch).
//
//   cd deepmerge_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I../../include -I. -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined ../../tools/scene_simplify_topology_host_check.cpp dm_scene_simplify_topology.hip \
//       dm_api.cpp -o /tmp/scene_simplify_topology_host_check
//   /tmp/scene_simplify_topology_host_check
//
// 1. the argument validation of the eight dm_scene_simplify_topology_* entries: every refusal returns DM_ERR_BAD_SHAPE with its
//    message, among them a cell product that only 64 bits hold and an absurd H, W and cell_log2;
// 2. the integer predicates of csrc/dm_simplify_topology.h (the code the kernels run) against a plain restatement in __int128 with
//    points near (2^31 - 2, 2^31 - 2): collinear, shared ends, identical segments, extents of exactly 32768, and differences of
//    almost 2^31, which the rule never meets but the code must survive without overflow;
// 3. the cell walk against a brute-force cover of the cell of every point of the segment, for cell sides 2^5, 2^6, 2^12, 2^20 and
//    2^24 and segments that end at x = 2^31 - 2;
// 4. the grid arithmetic: the cell product the entries accept never exceeds 2^22 and every cell id fits an int.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "deepmerge_hip.h"
#include "dm_simplify_topology.h"

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static const int FAR = 2147483646;                                 // 2^31 - 2: the last corner of the widest scene

static bool refused(int rc, const char *what) { return rc == DM_ERR_BAD_SHAPE && std::strstr(dm_last_error(), what) != nullptr; }

typedef int (*Entry)(const DmSceneSimplifyTopology *, void *);
static int refine_apply(const DmSceneSimplifyTopology *t, void *s) { return dm_scene_simplify_topology_refine(t, 1, s); }
static int refine_count(const DmSceneSimplifyTopology *t, void *s) { return dm_scene_simplify_topology_refine(t, 0, s); }

static void check_validation() {
  static int32_t i32[8];
  static int64_t i64[8];
  static uint8_t u8[8];
  DmSceneSimplifyTopology ok = {};
  ok.arc_xy = i32; ok.arc_ptr = i64; ok.new_ptr = i64; ok.arc_keep = u8; ok.point_count = i32; ok.point_fill = i32; ok.point_ptr = i64;
  ok.point_xy = i32; ok.seg = i32; ok.kind = i32; ok.cell_count = i32; ok.cell_fill = i32; ok.cell_ptr = i64; ok.cell_seg = i32;
  ok.stack = i64; ok.status = i32; ok.Va = 9; ok.cap = 64; ok.A = 3; ok.H = 8; ok.W = 8; ok.q = 256; ok.cell_log2 = 5;
  const struct { Entry fn; const char *name; bool tables; } entries[] = {
      {dm_scene_simplify_topology_point_count, "dm_scene_simplify_topology_point_count", false},
      {dm_scene_simplify_topology_point_fill, "dm_scene_simplify_topology_point_fill", false},
      {dm_scene_simplify_topology_segments, "dm_scene_simplify_topology_segments", true},
      {dm_scene_simplify_topology_bin_count, "dm_scene_simplify_topology_bin_count", true},
      {dm_scene_simplify_topology_bin_fill, "dm_scene_simplify_topology_bin_fill", true},
      {dm_scene_simplify_topology_pairs, "dm_scene_simplify_topology_pairs", true},
      {dm_scene_simplify_topology_jumps, "dm_scene_simplify_topology_jumps", true},
      {refine_apply, "dm_scene_simplify_topology_refine", true},
      {refine_count, "dm_scene_simplify_topology_refine", true}};
  for (const auto &e : entries) {
    DmSceneSimplifyTopology t;
    CHECK(refused(e.fn(nullptr, nullptr), e.name) && refused(e.fn(nullptr, nullptr), "null pointer"));
    t = ok; t.arc_xy = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
    t = ok; t.arc_ptr = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
    t = ok; t.arc_keep = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
    t = ok; t.point_count = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
    t = ok; t.point_fill = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
    t = ok; t.H = 0; CHECK(refused(e.fn(&t, nullptr), "H=0"));
    t = ok; t.W = -1; CHECK(refused(e.fn(&t, nullptr), "W=-1"));
    t = ok; t.H = INT32_MAX; t.cell_log2 = 24; CHECK(refused(e.fn(&t, nullptr), "H=2147483647"));      // 2^31 - 1 is no side
    t = ok; t.W = INT32_MAX; t.cell_log2 = 24; CHECK(refused(e.fn(&t, nullptr), "W=2147483647"));
    t = ok; t.H = INT32_MIN; CHECK(refused(e.fn(&t, nullptr), "bad scene"));
    t = ok; t.cell_log2 = 4; CHECK(refused(e.fn(&t, nullptr), "cell_log2=4"));
    t = ok; t.cell_log2 = 25; CHECK(refused(e.fn(&t, nullptr), "cell_log2=25"));
    t = ok; t.cell_log2 = -3; CHECK(refused(e.fn(&t, nullptr), "cell_log2=-3"));
    t = ok; t.cell_log2 = INT32_MAX; CHECK(refused(e.fn(&t, nullptr), "bad cell side"));               // no shift by it is ever formed
    t = ok; t.H = 65536; t.W = 65536; CHECK(refused(e.fn(&t, nullptr), "cells=4198401"));                // 2049^2 = 2^22 + 4097
    t = ok; t.H = FAR; t.W = FAR; CHECK(refused(e.fn(&t, nullptr), "cells=4503599627370496"));           // (2^26)^2: 0 in 32 bits
    t = ok; t.H = FAR; t.W = FAR; t.cell_log2 = 19; CHECK(refused(e.fn(&t, nullptr), "cells=16777216"));
    t = ok; t.H = 1 << 29; t.W = FAR; t.cell_log2 = 19; CHECK(refused(e.fn(&t, nullptr), "cells=4198400"));
    t = ok; t.A = 0; CHECK(refused(e.fn(&t, nullptr), "A=0"));
    t = ok; t.A = 1 << 30; CHECK(refused(e.fn(&t, nullptr), "A=1073741824"));
    t = ok; t.A = INT32_MIN; CHECK(refused(e.fn(&t, nullptr), "bad sizes"));
    t = ok; t.Va = 1; CHECK(refused(e.fn(&t, nullptr), "Va=1"));
    t = ok; t.Va = (1LL << 30) + 1; CHECK(refused(e.fn(&t, nullptr), "2^30"));
    t = ok; t.q = -1; CHECK(refused(e.fn(&t, nullptr), "q=-1"));
    t = ok; t.q = DM_SIMPLIFY_MAX_Q + 1; CHECK(refused(e.fn(&t, nullptr), "2^20"));
    if (!e.tables) continue;
    t = ok; t.cap = 0; CHECK(refused(e.fn(&t, nullptr), "cap=0"));
    t = ok; t.cap = 1LL << 31; CHECK(refused(e.fn(&t, nullptr), "cap=2147483648"));
    t = ok; t.new_ptr = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
    t = ok; t.seg = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
    t = ok; t.kind = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
    t = ok; t.cell_count = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
    t = ok; t.cell_fill = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
    t = ok; t.status = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
  }
  DmSceneSimplifyTopology t;
  t = ok; t.point_ptr = nullptr; CHECK(refused(dm_scene_simplify_topology_point_fill(&t, nullptr), "dm_scene_simplify_topology_point_fill: null pointer"));
  t = ok; t.point_xy = nullptr; CHECK(refused(dm_scene_simplify_topology_point_fill(&t, nullptr), "null pointer"));
  t = ok; t.cell_ptr = nullptr; CHECK(refused(dm_scene_simplify_topology_bin_fill(&t, nullptr), "dm_scene_simplify_topology_bin_fill: null pointer"));
  t = ok; t.cell_seg = nullptr; CHECK(refused(dm_scene_simplify_topology_bin_fill(&t, nullptr), "null pointer"));
  t = ok; t.cell_ptr = nullptr; CHECK(refused(dm_scene_simplify_topology_pairs(&t, nullptr), "dm_scene_simplify_topology_pairs: null pointer"));
  t = ok; t.cell_seg = nullptr; CHECK(refused(dm_scene_simplify_topology_pairs(&t, nullptr), "null pointer"));
  t = ok; t.point_ptr = nullptr; CHECK(refused(dm_scene_simplify_topology_jumps(&t, nullptr), "dm_scene_simplify_topology_jumps: null pointer"));
  t = ok; t.point_xy = nullptr; CHECK(refused(dm_scene_simplify_topology_jumps(&t, nullptr), "null pointer"));
  t = ok; t.stack = nullptr; CHECK(refused(dm_scene_simplify_topology_refine(&t, 1, nullptr), "dm_scene_simplify_topology_refine: null pointer"));
}

// ---- the grid ---------------------------------------------------------------------------------------------------------------------------
static long long cells_at(long long H, long long W, int log2) { return ((H >> log2) + 1) * ((W >> log2) + 1); }

static void check_grid() {
  // the smallest side the driver picks, and that an accepted grid's last cell id fits an int with room to spare
  const long long sides[] = {1, 31, 32, 32768, 65535, 65536, 131071, 131072, 1LL << 29, FAR};
  for (long long H : sides)
    for (long long W : sides) {
      if (H * W > DM_SCENE_VECTOR_MAX_PIXELS) continue;
      int log2 = DM_SCENE_SIMPLIFY_TOPOLOGY_MIN_CELL_LOG2;
      while (cells_at(H, W, log2) > DM_SCENE_SIMPLIFY_TOPOLOGY_MAX_CELLS) ++log2;
      CHECK(log2 <= DM_SCENE_SIMPLIFY_TOPOLOGY_MAX_CELL_LOG2);
      const long long last = (H >> log2) * ((W >> log2) + 1) + (W >> log2);      // cy grid_w + cx of corner (W, H)
      CHECK(last + 1 == cells_at(H, W, log2) && last < (1LL << 22));
    }
  CHECK(cells_at(65535, 65535, 5) == 1LL << 22 && cells_at(65536, 65536, 5) == (1LL << 22) + 4097 && cells_at(65536, 65536, 6) == 1025 * 1025);
  CHECK(cells_at(131071, 131071, 6) == 1LL << 22 && cells_at(1LL << 29, FAR, 20) == 513 * 2048 && cells_at(1LL << 29, FAR, 19) == 1025 * 4096);
  CHECK(2 * ((1LL << 30) - 1) + 1 <= INT32_MAX);                  // the table's tag, 2 arc + skip, at the last arc the entries accept
}

// ---- the predicates, restated plainly ------------------------------------------------------------------------------------------------
typedef __int128 wide;
struct P { int x, y; };
static bool same(P a, P b) { return a.x == b.x && a.y == b.y; }
static wide orient_wide(P a, P b, P c) { return (wide)(b.x - (wide)a.x) * (c.y - (wide)a.y) - (wide)(b.y - (wide)a.y) * (c.x - (wide)a.x); }
static bool on_wide(P a, P b, P p) {
  return orient_wide(a, b, p) == 0 && p.x >= (a.x < b.x ? a.x : b.x) && p.x <= (a.x < b.x ? b.x : a.x) && p.y >= (a.y < b.y ? a.y : b.y) &&
         p.y <= (a.y < b.y ? b.y : a.y);
}
static bool meets_wide(P a, P b, P c, P d) {
  if ((same(a, c) && same(b, d)) || (same(a, d) && same(b, c))) return true;
  const wide o1 = orient_wide(a, b, c), o2 = orient_wide(a, b, d), o3 = orient_wide(c, d, a), o4 = orient_wide(c, d, b);
  if (((o1 > 0 && o2 < 0) || (o1 < 0 && o2 > 0)) && ((o3 > 0 && o4 < 0) || (o3 < 0 && o4 > 0))) return true;
  return (on_wide(a, b, c) && !same(c, a) && !same(c, b)) || (on_wide(a, b, d) && !same(d, a) && !same(d, b)) ||
         (on_wide(c, d, a) && !same(a, c) && !same(a, d)) || (on_wide(c, d, b) && !same(b, c) && !same(b, d));
}
static bool counts_wide(P u, P w, P p) {
  if ((u.y <= p.y) == (w.y <= p.y)) return false;
  const wide o = orient_wide(u, w, p);
  return (w.y > u.y && o > 0) || (w.y < u.y && o < 0);
}
static bool meets_hd(P a, P b, P c, P d) { return dm_topo_meets(a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y); }

static void check_predicates() {
  const int M = DM_SIMPLIFY_MAX_SIDE;
  // a lattice at both ends of the coordinate range: differences of 0 .. 3, of exactly 32768 and of almost 2^31
  const int v[] = {0, 1, 3, M, FAR - M, FAR - 3, FAR - 1, FAR};
  std::vector<P> pts;
  for (int x : v)
    for (int y : v) pts.push_back({x, y});
  for (P a : pts)
    for (P b : pts)
      for (P c : pts) {
        const wide w = orient_wide(a, b, c);
        CHECK(w < ((wide)1 << 63) && w >= -((wide)1 << 63));      // two products below 2^62 each
        CHECK((wide)dm_topo_orient(a.x, a.y, b.x, b.y, c.x, c.y) == w);
      }
  CHECK(dm_topo_orient(FAR - M, FAR - M, FAR, FAR - M, FAR - M, FAR) == (1LL << 30));                   // extents of exactly 32768, far out
  CHECK(dm_topo_orient(FAR, FAR, FAR - M, FAR - M, FAR, FAR - M) == (1LL << 30) && dm_topo_orient(FAR - M, FAR - M, FAR, FAR, FAR - M / 2, FAR - M / 2) == 0);
  // the named configurations at the far corner, small and with extents of exactly 32768
  for (int s : {1, M / 4}) {
    const int B = FAR - 4 * s;
    const P o = {B, B}, d = {B + 4 * s, B + 4 * s}, m = {B + 2 * s, B + 2 * s}, e = {B + 4 * s, B}, n = {B, B + 4 * s};
    CHECK(meets_hd(o, d, o, d) && meets_hd(o, d, d, o));                                        // identical, either order
    CHECK(meets_hd(o, d, n, e));                                                                // a proper crossing
    CHECK(!meets_hd(o, d, n, {B + s, B + 3 * s}));                                              // the lines cross, the segments do not
    CHECK(meets_hd(o, d, m, e) && meets_hd(m, e, o, d));                                        // an end inside the other
    CHECK(!meets_hd(o, m, m, d) && !meets_hd(o, m, d, m) && !meets_hd(o, m, e, o));             // shared ends, collinear or not
    CHECK(meets_hd(o, {B + 3 * s, B + 3 * s}, m, d) && meets_hd(o, d, {B + s, B + s}, {B + 3 * s, B + 3 * s}));       // collinear overlap, containment
    CHECK(meets_hd(o, d, o, m) && meets_hd(o, m, d, o));                                        // a shared end, the other end on it
    CHECK(!meets_hd(o, m, {B + 3 * s, B + 3 * s}, d) && !meets_hd(o, e, {B, B + s}, {B + 4 * s, B + s}));             // collinear apart, parallel
    CHECK(!meets_hd(o, m, {B + 3 * s, B + 3 * s}, {B + 3 * s, B}));                             // on the line, outside the box
  }
  uint64_t s = 88172645463325252ULL;                              // xorshift: the same values on every run
  auto next = [&](int n) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (int)(s % (uint64_t)n); };
  for (int n = 0; n < 400000; ++n) {
    P q[4];
    const int span = n % 3 == 0 ? 4 : (n % 3 == 1 ? 9 : M + 1);   // small grids give the collinear cases; all of them at the far corner
    const int bx = FAR + 1 - span, by = n % 2 ? FAR + 1 - span : (1 << 29) - span;
    for (P &p : q) p = {bx + next(span), by + next(span)};
    if (!same(q[0], q[1]) && !same(q[2], q[3])) CHECK(meets_hd(q[0], q[1], q[2], q[3]) == meets_wide(q[0], q[1], q[2], q[3]));
    if (!same(q[0], q[1]) && !same(q[2], q[3])) CHECK(meets_hd(q[0], q[1], q[2], q[3]) == meets_hd(q[2], q[3], q[1], q[0]));
    CHECK(dm_topo_edge_counts(q[0].x, q[0].y, q[1].x, q[1].y, q[2].x, q[2].y) == counts_wide(q[0], q[1], q[2]));
  }
  for (int n = 0; n < 100000; ++n) {                              // anywhere in the range: what a table may hold, not what the rule meets
    P q[4];
    for (P &p : q) p = {next(FAR) + next(2), next(FAR) + next(2)};
    if (!same(q[0], q[1]) && !same(q[2], q[3])) CHECK(meets_hd(q[0], q[1], q[2], q[3]) == meets_wide(q[0], q[1], q[2], q[3]));
    CHECK(dm_topo_edge_counts(q[0].x, q[0].y, q[1].x, q[1].y, q[2].x, q[2].y) == counts_wide(q[0], q[1], q[2]));
  }
}

// ---- the cell walk -----------------------------------------------------------------------------------------------------------------------
static void check_walk_of(int x0, int y0, int x1, int y1, int log2) {
  std::set<std::pair<int, int>> cells;
  int visits = 0;
  dm_topo_walk_cells(x0, y0, x1, y1, log2, [&](int cx, int cy) { cells.insert({cx, cy}); ++visits; });
  const int cx0 = (x0 < x1 ? x0 : x1) >> log2, cx1 = (x0 < x1 ? x1 : x0) >> log2, cy0 = (y0 < y1 ? y0 : y1) >> log2, cy1 = (y0 < y1 ? y1 : y0) >> log2;
  for (const auto &c : cells) CHECK(c.first >= cx0 && c.first <= cx1 && c.second >= cy0 && c.second <= cy1);
  CHECK(visits == (int)cells.size() && visits <= 2 * (cx1 - cx0 + 1) + (cy1 - cy0 + 1));
  const long long dx = (long long)x1 - x0, dy = (long long)y1 - y0, n = 2 * ((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy)) + 1;
  for (long long k = 0; k <= n; ++k) {                            // points of the segment, floored: exact in integers (below 2^50)
    const long long x = dm_topo_floor_div(x0 * n + dx * k, n), y = dm_topo_floor_div(y0 * n + dy * k, n);
    CHECK(cells.count({(int)(x >> log2), (int)(y >> log2)}) == 1);
  }
}

static void check_walk() {
  const int M = DM_SIMPLIFY_MAX_SIDE;
  const int sides[] = {5, 6, 12, 20, 24};
  for (int L : sides) {
    check_walk_of(FAR - M, FAR, FAR, FAR, L); check_walk_of(FAR, FAR - M, FAR, FAR, L); check_walk_of(FAR - M, FAR - M, FAR, FAR, L);
    check_walk_of(FAR, FAR - M, FAR - M, FAR, L); check_walk_of(FAR - M, 0, FAR, 1, L); check_walk_of(FAR, 7, FAR - 1, M, L);
    check_walk_of(FAR, FAR, FAR, FAR, L); check_walk_of(0, 0, M, M, L);
    const int edge = (FAR >> L) << L;                             // the last cell edge before the scene's end
    check_walk_of(edge - 1, edge - 1, edge, edge, L); check_walk_of(edge, FAR - 64, edge, FAR, L); check_walk_of(edge - 40, edge, FAR, edge, L);
  }
  {                                                               // a 4096-long frame side at the far end costs its cells, not their square
    int visits = 0;
    dm_topo_walk_cells(FAR - 4096, FAR, FAR, FAR, 5, [&](int, int) { ++visits; });
    CHECK(visits == 129);
    visits = 0;
    dm_topo_walk_cells(FAR - 4096, FAR, FAR, FAR, 24, [&](int, int) { ++visits; });
    CHECK(visits == 1);
  }
  uint64_t s = 2463534242ULL;
  auto next = [&](int n) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (int)(s % (uint64_t)n); };
  for (int n = 0; n < 20000; ++n) {
    const int span = n % 4 == 0 ? 40 : (n % 4 == 1 ? 200 : (n % 4 == 2 ? 2000 : 70));
    const int bx = FAR - span, by = n % 3 == 0 ? FAR - span : (n % 3 == 1 ? (1 << 29) - span : 0);
    const int x1 = n % 5 == 0 ? FAR : bx + next(span + 1);        // every fifth segment ends at x = 2^31 - 2
    check_walk_of(bx + next(span + 1), by + next(span + 1), x1, by + next(span + 1), sides[n % 5]);
  }
}

int main() {
  check_validation();
  check_grid();
  check_predicates();
  check_walk();
  std::printf(failures ? "scene_simplify_topology_host_check: %d FAILED\n" : "scene_simplify_topology_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
