// Host check of csrc/dm_scene_simplify.hip for a sanitizer build, after the pattern of tools/simplify_host_check.cpp: a stand-alone
// program, nothing of it is loaded into Python and it needs no GPU (every call below returns from its argument validation,
// before any launch).
//
//   cd deepmerge_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I../../include -I. -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined ../../tools/scene_simplify_host_check.cpp dm_scene_simplify.hip dm_api.cpp \
//       -o /tmp/scene_simplify_host_check
//   /tmp/scene_simplify_host_check
//
// The argument validation of the seven dm_scene_simplify_* entries: every refusal returns DM_ERR_BAD_SHAPE with its message, and
// the products and sums the validation forms (H * W, oy + H, (H + 1)(W + 1), scene_h * scene_w) do not overflow at the limits.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "deepmerge_hip.h"

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static bool refused(int rc, const char *what) { return rc == DM_ERR_BAD_SHAPE && std::strstr(dm_last_error(), what) != nullptr; }

int main() {
  int32_t i32[8] = {0};
  int64_t i64[8] = {0};
  uint8_t u8[8] = {0};
  const int64_t big = DM_SCENE_VECTOR_MAX_SIDE - 1;               // the widest scene
  // nodes per tile: the window 10 x 12 at (7, 9), core [1, 9) x [1, 11)
  CHECK(refused(dm_scene_simplify_node_count(nullptr, 10, 12, 1, 9, 1, 11, 7, 9, 100, big, i32, i32, nullptr), "null pointer"));
  CHECK(refused(dm_scene_simplify_node_count(i32, 10, 12, 1, 9, 1, 11, 7, 9, 100, big, nullptr, i32, nullptr), "null pointer"));
  CHECK(refused(dm_scene_simplify_node_count(i32, 10, 12, 1, 9, 1, 11, 7, 9, 100, big, i32, nullptr, nullptr), "null pointer"));
  CHECK(refused(dm_scene_simplify_node_count(i32, 0, 12, 1, 9, 1, 11, 7, 9, 100, big, i32, i32, nullptr), "H*W"));
  CHECK(refused(dm_scene_simplify_node_count(i32, INT32_MAX, INT32_MAX, 1, 9, 1, 11, 7, 9, 100, big, i32, i32, nullptr), "H*W"));
  CHECK(refused(dm_scene_simplify_node_count(i32, 10, 12, 2, 9, 1, 11, 7, 9, 100, big, i32, i32, nullptr), "must lie in the window"));
  CHECK(refused(dm_scene_simplify_node_count(i32, 10, 12, 1, 9, 1, 13, 7, 9, 100, big, i32, i32, nullptr), "must lie in the window"));
  CHECK(refused(dm_scene_simplify_node_count(i32, 10, 12, 1, 9, 1, 11, 7, big - 11, 100, big, i32, i32, nullptr), "must lie in a scene"));
  CHECK(refused(dm_scene_simplify_node_count(i32, 10, 12, 1, 9, 1, 11, INT64_MAX - 5, 9, 100, big, i32, i32, nullptr), "must lie in a scene"));
  CHECK(refused(dm_scene_simplify_node_count(i32, 10, 12, 1, 9, 1, 11, 7, 9, big, big, i32, i32, nullptr), "must lie in a scene"));
  CHECK(refused(dm_scene_simplify_node_count(i32, 10, 12, 1, 9, 1, 11, 7, 9, 100, big + 1, i32, i32, nullptr), "must lie in a scene"));
  CHECK(refused(dm_scene_simplify_node_count(i32, 10, 12, 0, 9, 1, 11, 7, 9, 100, big, i32, i32, nullptr), "only where that is the scene's edge"));
  CHECK(refused(dm_scene_simplify_node_count(i32, 10, 12, 1, 9, 1, 12, 7, 9, 100, big, i32, i32, nullptr), "only where that is the scene's edge"));
  CHECK(refused(dm_scene_simplify_node_emit(i32, 10, 12, 1, 9, 1, 11, 7, 9, 100, big, i32, 5, nullptr, nullptr), "null pointer"));
  CHECK(refused(dm_scene_simplify_node_emit(i32, 10, 12, 1, 9, 1, 11, 7, 9, 100, big, i32, 0, i64, nullptr), "N=0"));
  CHECK(refused(dm_scene_simplify_node_emit(i32, 10, 12, 1, 9, 1, 11, 7, 9, 100, big, i32, 11 * 13 + 1, i64, nullptr), "N=144"));
  CHECK(refused(dm_scene_simplify_node_emit(i32, 10, 12, 1, 9, 1, 11, 7, 9, 0, big, i32, 5, i64, nullptr), "must lie in a scene"));
  // chains and arcs
  CHECK(refused(dm_scene_simplify_chains(i32, i64, 3, 9, big, 100, 384, u8, nullptr, nullptr), "null pointer"));
  CHECK(refused(dm_scene_simplify_chains(i32, i64, 0, 9, big, 100, 384, u8, i64, nullptr), "A=0"));
  CHECK(refused(dm_scene_simplify_chains(i32, i64, 3, 1, big, 100, 384, u8, i64, nullptr), "Va=1"));
  CHECK(refused(dm_scene_simplify_chains(i32, i64, 3, 1LL << 31, big, 100, 384, u8, i64, nullptr), "2^31"));
  CHECK(refused(dm_scene_simplify_chains(i32, i64, 3, 9, big + 1, 100, 384, u8, i64, nullptr), "bad scene"));
  CHECK(refused(dm_scene_simplify_chains(i32, i64, 3, 9, big, big, 384, u8, i64, nullptr), "bad scene"));
  CHECK(refused(dm_scene_simplify_chains(i32, i64, 3, 9, INT64_MAX, INT64_MAX, 384, u8, i64, nullptr), "bad scene"));
  CHECK(refused(dm_scene_simplify_chains(i32, i64, 3, 9, big, 100, -1, u8, i64, nullptr), "q=-1"));
  CHECK(refused(dm_scene_simplify_chains(i32, i64, 3, 9, big, 100, DM_SIMPLIFY_MAX_Q + 1, u8, i64, nullptr), "2^20"));
  CHECK(refused(dm_scene_simplify_arc_count(i32, i64, 3, 9, big, 100, nullptr, i32, nullptr), "null pointer"));
  CHECK(refused(dm_scene_simplify_arc_count(i32, i64, 3, 9, 0, 100, u8, i32, nullptr), "bad scene"));
  CHECK(refused(dm_scene_simplify_arc_emit(i32, i64, nullptr, 3, 9, 6, big, 100, u8, i32, nullptr), "null pointer"));
  CHECK(refused(dm_scene_simplify_arc_emit(i32, i64, i64, 3, 9, 0, big, 100, u8, i32, nullptr), "Vn=0"));
  CHECK(refused(dm_scene_simplify_arc_emit(i32, i64, i64, 3, 9, 10, big, 100, u8, i32, nullptr), "Vn=10"));
  // rings
  DmSceneSimplifyRings t = {i32, i64, i32, i64, i64, i64, i32, 40, 90, 1 << 20, big, 64, 3};
  CHECK(refused(dm_scene_simplify_ring_count(nullptr, i32, nullptr), "null argument struct"));
  CHECK(refused(dm_scene_simplify_ring_count(&t, nullptr, nullptr), "null pointer"));
  DmSceneSimplifyRings bad = t;
  bad.kept_row = nullptr;
  CHECK(refused(dm_scene_simplify_ring_count(&bad, i32, nullptr), "null pointer"));
  bad = t; bad.status = nullptr;
  CHECK(refused(dm_scene_simplify_ring_emit(&bad, i64, i64, 70, i32, i64, nullptr), "null pointer"));
  bad = t; bad.R = 65;
  CHECK(refused(dm_scene_simplify_ring_count(&bad, i32, nullptr), "R=65"));
  bad = t; bad.n_nodes = 3;
  CHECK(refused(dm_scene_simplify_ring_count(&bad, i32, nullptr), "oversized or undersized list"));
  bad = t; bad.n_nodes = 1LL << 31; bad.n_kept = 1LL << 31;
  CHECK(refused(dm_scene_simplify_ring_count(&bad, i32, nullptr), "oversized or undersized list"));
  bad = t; bad.n_kept = 39;
  CHECK(refused(dm_scene_simplify_ring_emit(&bad, i64, i64, 70, i32, i64, nullptr), "oversized or undersized list"));
  bad = t; bad.n_kept = INT64_MAX;
  CHECK(refused(dm_scene_simplify_ring_emit(&bad, i64, i64, 70, i32, i64, nullptr), "oversized or undersized list"));
  bad = t; bad.scene_h = big;
  CHECK(refused(dm_scene_simplify_ring_count(&bad, i32, nullptr), "bad scene"));
  CHECK(refused(dm_scene_simplify_ring_emit(&t, nullptr, i64, 70, i32, i64, nullptr), "null pointer"));
  CHECK(refused(dm_scene_simplify_ring_emit(&t, i64, i64, 70, i32, nullptr, nullptr), "null pointer"));
  CHECK(refused(dm_scene_simplify_ring_emit(&t, i64, i64, 0, i32, i64, nullptr), "Vn=0"));
  CHECK(refused(dm_scene_simplify_ring_emit(&t, i64, i64, 1LL << 32, i32, i64, nullptr), "2^32"));
  std::printf(failures ? "%d check(s) FAILED\n" : "scene_simplify_host_check: all checks passed\n", failures);
  return failures != 0;
}
