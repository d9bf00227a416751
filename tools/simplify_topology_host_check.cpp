// Host check of csrc/dm_simplify_topology.hip for a sanitizer build: a stand-alone program, nothing of it is loaded into Python and
// it needs no GPU (every call below returns from its argument validation, before any launch).
//
//   cd deepmerge_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I../../include -I. -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined ../../tools/simplify_topology_host_check.cpp dm_simplify_topology.hip dm_api.cpp \
//       -o /tmp/simplify_topology_host_check
//   /tmp/simplify_topology_host_check
//
// 1. the argument validation of the eight dm_simplify_topology_* entries: every refusal returns DM_ERR_BAD_SHAPE with its message;
// 2. the integer predicates of csrc/dm_simplify_topology.h (the code the kernels run) against a plain restatement in __int128, on
//    every configuration the rule names and at the coordinate extremes 0 and 32768;
// 3. the cell walk: the cells it visits hold the cell of every point of the segment, lie inside the segment's box of cells, and
//    are as few as a walk along the segment allows;
// 4. a segment's share of the refine stack stays inside the workspace.
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

static bool refused(int rc, const char *what) { return rc == DM_ERR_BAD_SHAPE && std::strstr(dm_last_error(), what) != nullptr; }

typedef int (*Entry)(const DmSimplifyTopology *, void *);
static int refine_apply(const DmSimplifyTopology *t, void *s) { return dm_simplify_topology_refine(t, 1, s); }
static int refine_count(const DmSimplifyTopology *t, void *s) { return dm_simplify_topology_refine(t, 0, s); }

static void check_validation() {
  static int32_t i32[8];
  static int64_t i64[8];
  static uint8_t u8[8];
  DmSimplifyTopology ok = {};
  ok.arc_xy = i32; ok.arc_ptr = i64; ok.new_ptr = i64; ok.keep = u8; ok.point_count = i32; ok.point_fill = i32; ok.point_ptr = i64;
  ok.point_xy = i32; ok.seg = i32; ok.kind = i32; ok.cell_count = i32; ok.cell_fill = i32; ok.cell_ptr = i64; ok.cell_seg = i32;
  ok.stack = i64; ok.status = i32; ok.Va = 9; ok.cap = 64; ok.A = 3; ok.H = 8; ok.W = 8; ok.q = 256;
  const struct { Entry fn; const char *name; bool tables; } entries[] = {
      {dm_simplify_topology_point_count, "dm_simplify_topology_point_count", false}, {dm_simplify_topology_point_fill, "dm_simplify_topology_point_fill", false},
      {dm_simplify_topology_segments, "dm_simplify_topology_segments", true},        {dm_simplify_topology_bin_count, "dm_simplify_topology_bin_count", true},
      {dm_simplify_topology_bin_fill, "dm_simplify_topology_bin_fill", true},        {dm_simplify_topology_pairs, "dm_simplify_topology_pairs", true},
      {dm_simplify_topology_jumps, "dm_simplify_topology_jumps", true},              {refine_apply, "dm_simplify_topology_refine", true},
      {refine_count, "dm_simplify_topology_refine", true}};
  for (const auto &e : entries) {
    DmSimplifyTopology t;
    CHECK(refused(e.fn(nullptr, nullptr), e.name) && refused(e.fn(nullptr, nullptr), "null pointer"));
    t = ok; t.arc_xy = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
    t = ok; t.arc_ptr = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
    t = ok; t.keep = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
    t = ok; t.point_count = nullptr; CHECK(refused(e.fn(&t, nullptr), "null pointer"));
    t = ok; t.H = 0; CHECK(refused(e.fn(&t, nullptr), "H=0"));
    t = ok; t.W = -1; CHECK(refused(e.fn(&t, nullptr), "W=-1"));
    t = ok; t.H = 32769; CHECK(refused(e.fn(&t, nullptr), "H=32769"));
    t = ok; t.A = 0; CHECK(refused(e.fn(&t, nullptr), "A=0"));
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
  DmSimplifyTopology t;
  t = ok; t.point_ptr = nullptr; CHECK(refused(dm_simplify_topology_point_fill(&t, nullptr), "dm_simplify_topology_point_fill: null pointer"));
  t = ok; t.point_xy = nullptr; CHECK(refused(dm_simplify_topology_point_fill(&t, nullptr), "null pointer"));
  t = ok; t.cell_ptr = nullptr; CHECK(refused(dm_simplify_topology_bin_fill(&t, nullptr), "dm_simplify_topology_bin_fill: null pointer"));
  t = ok; t.cell_seg = nullptr; CHECK(refused(dm_simplify_topology_bin_fill(&t, nullptr), "null pointer"));
  t = ok; t.cell_ptr = nullptr; CHECK(refused(dm_simplify_topology_pairs(&t, nullptr), "dm_simplify_topology_pairs: null pointer"));
  t = ok; t.cell_seg = nullptr; CHECK(refused(dm_simplify_topology_pairs(&t, nullptr), "null pointer"));
  t = ok; t.point_ptr = nullptr; CHECK(refused(dm_simplify_topology_jumps(&t, nullptr), "dm_simplify_topology_jumps: null pointer"));
  t = ok; t.point_xy = nullptr; CHECK(refused(dm_simplify_topology_jumps(&t, nullptr), "null pointer"));
  t = ok; t.stack = nullptr; CHECK(refused(dm_simplify_topology_refine(&t, 1, nullptr), "dm_simplify_topology_refine: null pointer"));
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
  const int v[] = {0, 1, 2, 3, M / 2, M - 1, M};
  std::vector<P> pts;
  for (int x : v)
    for (int y : v) pts.push_back({x, y});
  for (P a : pts)
    for (P b : pts)
      for (P c : pts) CHECK((wide)dm_topo_orient(a.x, a.y, b.x, b.y, c.x, c.y) == orient_wide(a, b, c));
  CHECK(dm_topo_orient(0, 0, M, 0, 0, M) == (1LL << 30) && dm_topo_orient(0, 0, 0, M, M, 0) == -(1LL << 30));
  CHECK(dm_topo_orient(M, M, 0, 0, M, 0) == (1LL << 30) && dm_topo_orient(0, 0, M, M, M / 2, M / 2) == 0);
  // the named configurations, small and at the extremes
  for (int s : {1, M / 4}) {
    const P o = {0, 0}, d = {4 * s, 4 * s}, m = {2 * s, 2 * s};
    CHECK(meets_hd(o, d, o, d) && meets_hd(o, d, d, o));                                        // identical, either order
    CHECK(meets_hd(o, d, {0, 4 * s}, {4 * s, 0}));                                             // a proper crossing
    CHECK(!meets_hd(o, d, {0, 4 * s}, {s, 3 * s}));                                            // the lines cross, the segments do not
    CHECK(meets_hd(o, d, m, {4 * s, 0}) && meets_hd(m, {4 * s, 0}, o, d));                     // an end inside the other
    CHECK(!meets_hd(o, m, m, d) && !meets_hd(o, m, d, m) && !meets_hd(o, m, {4 * s, 0}, o));   // shared ends, collinear or not
    CHECK(meets_hd(o, {3 * s, 3 * s}, m, d) && meets_hd(o, d, {s, s}, {3 * s, 3 * s}));          // collinear overlap, containment
    CHECK(meets_hd(o, d, o, m) && meets_hd(o, m, d, o));                                       // a shared end, the other end on it
    CHECK(!meets_hd(o, m, {3 * s, 3 * s}, d) && !meets_hd(o, {4 * s, 0}, {0, s}, {4 * s, s})); // collinear apart, parallel
    CHECK(!meets_hd(o, m, {3 * s, 3 * s}, {3 * s, 0}));                                        // on the line, outside the box
  }
  uint64_t s = 88172645463325252ULL;                              // xorshift: the same values on every run
  auto next = [&](int n) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (int)(s % (uint64_t)n); };
  for (int n = 0; n < 400000; ++n) {
    P q[4];
    const int span = n % 3 == 0 ? 4 : (n % 3 == 1 ? 9 : M + 1), base = n % 2 ? 0 : M + 1 - span;      // small grids give the collinear cases
    for (P &p : q) p = {base + next(span), base + next(span)};
    if (!same(q[0], q[1]) && !same(q[2], q[3])) CHECK(meets_hd(q[0], q[1], q[2], q[3]) == meets_wide(q[0], q[1], q[2], q[3]));
    if (!same(q[0], q[1]) && !same(q[2], q[3])) CHECK(meets_hd(q[0], q[1], q[2], q[3]) == meets_hd(q[2], q[3], q[1], q[0]));
    CHECK(dm_topo_edge_counts(q[0].x, q[0].y, q[1].x, q[1].y, q[2].x, q[2].y) == counts_wide(q[0], q[1], q[2]));
  }
  for (long long a = -70; a <= 70; ++a)
    for (long long b = 1; b <= 9; ++b) {
      const long long f = dm_topo_floor_div(a, b);
      CHECK(f * b <= a && a < (f + 1) * b);
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
  const long long dx = x1 - x0, dy = y1 - y0, n = 2 * ((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy)) + 1;
  for (long long k = 0; k <= n; ++k) {                            // points of the segment, floored: exact in integers
    const long long x = dm_topo_floor_div(x0 * n + dx * k, n), y = dm_topo_floor_div(y0 * n + dy * k, n);
    CHECK(cells.count({(int)(x >> log2), (int)(y >> log2)}) == 1);
  }
}

static void check_walk() {
  const int M = DM_SIMPLIFY_MAX_SIDE, L = DM_SIMPLIFY_TOPOLOGY_CELL_LOG2;
  check_walk_of(0, 0, M, 0, L); check_walk_of(M, M, 0, M, L); check_walk_of(0, 0, 0, M, L); check_walk_of(M, 0, M, M, L);
  check_walk_of(0, 0, M, M, L); check_walk_of(M, 0, 0, M, L); check_walk_of(0, 0, M, 1, L); check_walk_of(0, M, 1, 0, L);
  check_walk_of(5, 5, 5, 5, L); check_walk_of(31, 31, 32, 32, L); check_walk_of(32, 0, 32, 64, L); check_walk_of(0, 32, 64, 32, L);
  {                                                               // a 4096-long frame side costs its 129 cells, not 129^2
    int visits = 0;
    dm_topo_walk_cells(0, 0, 4096, 0, L, [&](int, int) { ++visits; });
    CHECK(visits == 129);
  }
  uint64_t s = 2463534242ULL;
  auto next = [&](int n) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (int)(s % (uint64_t)n); };
  for (int n = 0; n < 20000; ++n) {
    const int span = n % 4 == 0 ? 40 : (n % 4 == 1 ? 200 : (n % 4 == 2 ? 2000 : 70)), base = n % 2 ? 0 : M - span;
    check_walk_of(base + next(span + 1), base + next(span + 1), base + next(span + 1), base + next(span + 1), n % 5 == 0 ? 3 : L);
  }
}

static void check_stack_share() {
  // arc a owns stack[2 arc_ptr[a] .. 2 arc_ptr[a + 1]); segment (i, j), i < len, j <= i + len, len <= n, owns j - i entries from
  // 2 first + i: the last is 2 first + j - 1 < 2 first + 2 len <= 2 (first + n).  Either half of the segment has fewer interior
  // vertices than j - i, which is what the walk of dm_simplify_arcs.h needs (tools/simplify_host_check.cpp holds it to that).
  for (long long first : {0LL, 7LL, (1LL << 30) - 5})
    for (long long n : {2LL, 3LL, 5LL})
      for (long long len : {n - 1, n})
        for (long long i = 0; i < len; ++i)
          for (long long j = i + 1; j <= i + len; ++j) CHECK(2 * first + i + (j - i) <= 2 * (first + n) && j - i >= 1);
  CHECK(2 * (1LL << 30) * (long long)sizeof(int64_t) == 1LL << 34);
}

int main() {
  check_validation();
  check_predicates();
  check_walk();
  check_stack_share();
  std::printf(failures ? "simplify_topology_host_check: %d FAILED\n" : "simplify_topology_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
