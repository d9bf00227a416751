// Host check of csrc/dm_simplify.hip for a sanitizer build: a stand-alone program, nothing of it is loaded into Python and it
// needs no GPU (every call below returns from its argument validation, before any launch).
//
//   cd deepmerge_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I../../include -I. -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined ../../tools/simplify_host_check.cpp dm_simplify.hip dm_api.cpp -o /tmp/simplify_host_check
//   /tmp/simplify_host_check
//
// 1. the argument validation of the six dm_simplify_* entries: every refusal returns DM_ERR_BAD_SHAPE with its message;
// 2. dm_simplify_exceeds (csrc/dm_simplify.h, the code the kernel runs) against unsigned __int128 at the edges of its range;
// 3. the stack bound of the chains kernel: the same depth-first walk (left half at once, right half pushed) on chains that split at
//    every vertex, on a stack of exactly one entry per interior vertex that the sanitizer guards, against the plain recursion.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "deepmerge_hip.h"
#include "dm_simplify.h"

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static bool refused(int rc, const char *what) { return rc == DM_ERR_BAD_SHAPE && std::strstr(dm_last_error(), what) != nullptr; }

static void check_validation() {
  int32_t i32[8] = {0};
  int64_t i64[8] = {0};
  uint8_t u8[8] = {0};
  CHECK(refused(dm_simplify_nodes(nullptr, 8, 8, u8, nullptr), "null pointer"));
  CHECK(refused(dm_simplify_nodes(i32, 8, 8, nullptr, nullptr), "null pointer"));
  CHECK(refused(dm_simplify_nodes(i32, 0, 8, u8, nullptr), "H=0"));
  CHECK(refused(dm_simplify_nodes(i32, 8, -1, u8, nullptr), "W=-1"));
  CHECK(refused(dm_simplify_nodes(i32, 32769, 8, u8, nullptr), "H=32769"));
  CHECK(refused(dm_simplify_chains(i32, i64, 3, 9, 8, 8, 256, u8, nullptr, nullptr), "null pointer"));
  CHECK(refused(dm_simplify_chains(i32, i64, 0, 9, 8, 8, 256, u8, i64, nullptr), "A=0"));
  CHECK(refused(dm_simplify_chains(i32, i64, 3, 1, 8, 8, 256, u8, i64, nullptr), "Va=1"));
  CHECK(refused(dm_simplify_chains(i32, i64, 3, (1LL << 30) + 1, 8, 8, 256, u8, i64, nullptr), "2^30"));
  CHECK(refused(dm_simplify_chains(i32, i64, 3, 9, 8, 32769, 256, u8, i64, nullptr), "W=32769"));
  CHECK(refused(dm_simplify_chains(i32, i64, 3, 9, 8, 8, -1, u8, i64, nullptr), "q=-1"));
  CHECK(refused(dm_simplify_chains(i32, i64, 3, 9, 8, 8, DM_SIMPLIFY_MAX_Q + 1, u8, i64, nullptr), "2^20"));
  CHECK(refused(dm_simplify_arc_count(i32, i64, 3, 9, 8, 8, nullptr, i32, nullptr), "null pointer"));
  CHECK(refused(dm_simplify_arc_count(i32, i64, 3, 9, 0, 8, u8, i32, nullptr), "H=0"));
  CHECK(refused(dm_simplify_arc_emit(i32, i64, nullptr, 3, 9, 6, 8, 8, u8, i32, nullptr), "null pointer"));
  CHECK(refused(dm_simplify_arc_emit(i32, i64, i64, 3, 9, 0, 8, 8, u8, i32, nullptr), "Vn=0"));
  CHECK(refused(dm_simplify_arc_emit(i32, i64, i64, 3, 9, 10, 8, 8, u8, i32, nullptr), "Vn=10"));
  CHECK(refused(dm_simplify_ring_count(i32, i64, nullptr, 12, 3, 8, 8, u8, i32, nullptr), "null pointer"));
  CHECK(refused(dm_simplify_ring_count(i32, i64, i32, 0, 3, 8, 8, u8, i32, nullptr), "V=0"));
  CHECK(refused(dm_simplify_ring_count(i32, i64, i32, 2, 3, 8, 8, u8, i32, nullptr), "R=3"));
  CHECK(refused(dm_simplify_ring_emit(i32, i64, i32, i64, i64, 12, 3, 12, 8, 8, u8, i32, nullptr, nullptr), "null pointer"));
  CHECK(refused(dm_simplify_ring_emit(i32, i64, i32, nullptr, i64, 12, 3, 12, 8, 8, u8, i32, i64, nullptr), "null pointer"));
  CHECK(refused(dm_simplify_ring_emit(i32, i64, i32, i64, i64, 12, 3, 0, 8, 8, u8, i32, i64, nullptr), "Vn=0"));
  CHECK(refused(dm_simplify_ring_emit(i32, i64, i32, i64, i64, 12, 3, 12, 40000, 8, u8, i32, i64, nullptr), "H=40000"));
}

static bool exceeds_wide(uint64_t d, uint64_t len2, uint64_t q2) {
  typedef unsigned __int128 u128;
  return len2 == 0 ? (u128)65536 * d > (u128)q2 : (u128)65536 * d * d > (u128)q2 * len2;
}

static void check_exceeds() {
  const uint64_t ds[] = {0, 1, 2, 255, 256, 4095, 4096, 4097, (1ULL << 24) - 1, 1ULL << 24, (1ULL << 24) + 1, (1ULL << 30) - 1, 1ULL << 30, (1ULL << 31) - 1, 1ULL << 31};
  const uint64_t lens[] = {0, 1, 2, 5, 65536, (1ULL << 30) + 1, (1ULL << 31) - 1, 1ULL << 31};
  const uint64_t qs[] = {0, 1, 179, 192, 256, 384, 1024, (1ULL << 20) - 1, 1ULL << 20};
  for (uint64_t d : ds)
    for (uint64_t l : lens)
      for (uint64_t q : qs) CHECK(dm_simplify_exceeds(d, l, q * q) == exceeds_wide(d, l, q * q));
  uint64_t s = 88172645463325252ULL;                              // xorshift: the same values on every run
  for (int n = 0; n < 200000; ++n) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    const uint64_t d = s % ((1ULL << 31) + 1), l = (s >> 20) % ((1ULL << 31) + 1), q = (s >> 40) % ((1ULL << 20) + 1);
    CHECK(dm_simplify_exceeds(d, l, q * q) == exceeds_wide(d, l, q * q));
  }
}

struct P { long long x, y; };

static void farthest(const std::vector<P> &v, int i, int j, int &k, uint64_t &d, uint64_t &len2) {
  const long long dx = v[j].x - v[i].x, dy = v[j].y - v[i].y;
  len2 = (uint64_t)(dx * dx + dy * dy);
  d = 0; k = i + 1;
  for (int m = i + 1; m < j; ++m) {
    const long long rx = v[m].x - v[i].x, ry = v[m].y - v[i].y, cr = dx * ry - dy * rx;
    const uint64_t e = len2 == 0 ? (uint64_t)(rx * rx + ry * ry) : (uint64_t)(cr < 0 ? -cr : cr);
    if (e > d) { d = e; k = m; }                                  // ties to the smallest k
  }
}

static void recurse(const std::vector<P> &v, int i, int j, uint64_t q2, std::vector<char> &keep) {
  if (j - i < 2) return;
  int k; uint64_t d, len2;
  farthest(v, i, j, k, d, len2);
  if (!dm_simplify_exceeds(d, len2, q2)) return;
  keep[k] = 1;
  recurse(v, i, k, q2, keep);
  recurse(v, k, j, q2, keep);
}

// The kernel's walk on a stack of exactly `interior` entries (heap memory: the sanitizer sees an entry too many); returns the
// deepest the stack got.
static size_t walk(const std::vector<P> &v, uint64_t q2, std::vector<char> &keep) {
  const int n = (int)v.size();
  const size_t cap = n > 2 ? (size_t)(n - 2) : 0;
  int64_t *stack = (int64_t *)std::malloc(cap ? cap * sizeof(int64_t) : 1);
  size_t sp = 0, deepest = 0;
  int i = 0, j = n - 1;
  bool have = j - i > 1;
  while (have) {
    int k; uint64_t d, len2;
    farthest(v, i, j, k, d, len2);
    bool left = false, right = false;
    if (dm_simplify_exceeds(d, len2, q2)) { keep[k] = 1; left = k - i > 1; right = j - k > 1; }
    if (left && right) { stack[sp++] = ((int64_t)k << 32) | (int64_t)j; j = k; }
    else if (left) j = k;
    else if (right) i = k;
    else if (sp > 0) { const int64_t top = stack[--sp]; i = (int)(top >> 32); j = (int)(top & 0xffffffffLL); }
    else have = false;
    if (sp > deepest) deepest = sp;
  }
  std::free(stack);
  return deepest;
}

static void check_stack_bound() {
  std::vector<std::vector<P>> chains;
  for (int n : {2, 3, 4, 5, 64, 65, 1000, 8193}) {
    std::vector<P> stair, comb, spiral, closed;
    for (int m = 0; m < n; ++m) stair.push_back({(m + 1) / 2, m / 2});                                  // a staircase
    for (int m = 0; m < n; ++m) comb.push_back({m / 2, ((m + 1) / 2) % 2 ? (m % 4 < 2 ? 0 : 7 + m % 5) : 0});
    long long x = 0, y = 0, side = 1;
    for (int m = 0; m < n; ++m) {                                                                      // a square spiral: ever longer legs
      spiral.push_back({x, y});
      const int dir = m % 4;
      x += dir == 0 ? side : dir == 2 ? -side : 0;
      y += dir == 1 ? side : dir == 3 ? -side : 0;
      if (dir % 2) ++side;
    }
    closed = stair;
    if (n > 2) closed.back() = closed.front();                                                         // coinciding ends: the first split is by distance
    chains.push_back(stair); chains.push_back(comb); chains.push_back(spiral); chains.push_back(closed);
  }
  for (const auto &v : chains)
    for (uint64_t q : {0ULL, 128ULL, 192ULL, 1024ULL, 1ULL << 20}) {
      std::vector<char> a(v.size(), 0), b(v.size(), 0);
      const size_t deepest = walk(v, q * q, a);
      recurse(v, 0, (int)v.size() - 1, q * q, b);
      CHECK(a == b);
      CHECK(deepest <= (v.size() > 2 ? v.size() - 2 : 0));
    }
  // the workspace layout: arc a owns stack[arc_ptr[a] .. arc_ptr[a + 1]), one entry per stored vertex, so its interior fits and the
  // last entry of the last arc is Va - 1 < 2^30 entries of 8 bytes
  const int64_t Va = 1LL << 30;
  CHECK(Va * (int64_t)sizeof(int64_t) == 1LL << 33 && (Va - 1) * (int64_t)sizeof(int64_t) + 8 <= Va * 8);
}

int main() {
  check_validation();
  check_exceeds();
  check_stack_bound();
  std::printf(failures ? "simplify_host_check: %d FAILED\n" : "simplify_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
