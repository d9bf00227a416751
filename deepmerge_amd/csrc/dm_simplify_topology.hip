// Topology-safe simplification (gfx950): find the segments of a simplified scene that meet another segment or jumped over a fixed
// point, and repair them by keeping more vertices.  The rule is the build's own: stated in include/deepmerge_hip.h, restated in
// numpy / Python ints in tests/simplify_topology_ref.py.  Integers only: the device and the spec agree bit for bit.
// The kernels and the passes they make are dm_simplify_topology_kernels.h's, shared with the scene form
// (dm_scene_simplify_topology.hip); this file is their one-raster form: keep is a byte per pixel corner (CornerKeep, H, W <= 32768)
// and the grid has cells of 2^DM_SIMPLIFY_TOPOLOGY_CELL_LOG2 corners, at most 1025^2 of them.
#include "dm_simplify_topology_kernels.h"

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

namespace {

struct DenseTopology {
  typedef DmSimplifyTopology Struct;
  typedef CornerKeep<unsigned char> Keep;
  typedef CornerKeep<const unsigned char> KeepRead;
  static __host__ __device__ __forceinline__ int log2(const Struct &) { return DM_SIMPLIFY_TOPOLOGY_CELL_LOG2; }
  static __device__ __forceinline__ Keep keep(const Struct &t) { return Keep{t.keep, t.H, t.W}; }
  static __device__ __forceinline__ KeepRead keep_read(const Struct &t) { return KeepRead{t.keep, t.H, t.W}; }
  static int ok(const char *what, const Struct *t, bool tables) { return topology_ok(what, t, tables); }
};

}  // namespace

extern "C" int dm_simplify_topology_point_count(const DmSimplifyTopology *t, void *stream) {
  return topo_point_count<DenseTopology>("dm_simplify_topology_point_count", t, stream);
}
extern "C" int dm_simplify_topology_point_fill(const DmSimplifyTopology *t, void *stream) {
  return topo_point_fill<DenseTopology>("dm_simplify_topology_point_fill", t, stream);
}
extern "C" int dm_simplify_topology_segments(const DmSimplifyTopology *t, void *stream) {
  return topo_segments<DenseTopology>("dm_simplify_topology_segments", t, stream);
}
extern "C" int dm_simplify_topology_bin_count(const DmSimplifyTopology *t, void *stream) {
  return topo_bin<DenseTopology, false>("dm_simplify_topology_bin_count", t, stream);
}
extern "C" int dm_simplify_topology_bin_fill(const DmSimplifyTopology *t, void *stream) {
  return topo_bin<DenseTopology, true>("dm_simplify_topology_bin_fill", t, stream);
}
extern "C" int dm_simplify_topology_pairs(const DmSimplifyTopology *t, void *stream) {
  return topo_pairs<DenseTopology>("dm_simplify_topology_pairs", t, stream);
}
extern "C" int dm_simplify_topology_jumps(const DmSimplifyTopology *t, void *stream) {
  return topo_jumps<DenseTopology>("dm_simplify_topology_jumps", t, stream);
}
extern "C" int dm_simplify_topology_refine(const DmSimplifyTopology *t, int32_t apply, void *stream) {
  return topo_refine<DenseTopology>("dm_simplify_topology_refine", t, apply, stream);
}
