// Topology-safe simplification of a scene (gfx950): the detection and repair rounds of dm_simplify_topology.hip on a scene's arcs,
// for scene.simplify_labels_topology.  DESIGN.md 3.5.13.  No new geometry rule and no new kernel: the kernels are
// dm_simplify_topology_kernels.h's, here in their scene form.  Two things differ from the one-raster form:
//   keep       one byte per stored arc vertex (arc_keep, VertexKeep of dm_simplify_arcs.h): a scene has no raster of corners on the
//              device and its corner ids need 64 bits.  A vertex's flag is found by its position in its arc, a closed arc's anchor by
//              the wave minimum of the 64-bit corner id.  Refine stores arc_keep = 1 at positions of its own segment only.
//   the grid   dense as before, but of cells of 2^cell_log2 corners, a field of the struct chosen by the caller so that the grid has
//              at most 2^22 cells whatever the scene's sides.  The result does not depend on it (dm_simplify_topology_kernels.h
//              says why); a coarser grid only tests more pairs per cell.
// The arithmetic argument is in dm_simplify_topology_kernels.h and dm_simplify_topology.h; what this file adds is the validation
// that makes it hold: sides below 2^31 - 1, 5 <= cell_log2 <= 24, the cell product formed in 64 bits, A < 2^30 for the table's tag.
#include "dm_simplify_topology_kernels.h"

namespace {

constexpr long long MAX_TOPOLOGY_SIDE = DM_SCENE_VECTOR_MAX_SIDE;

// What every entry asks of the struct; `tables`: the round's arrays beyond the fixed points'.
int scene_topology_ok(const char *what, const DmSceneSimplifyTopology *t, bool tables) {
  DM_REQUIRE(t, DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  DM_REQUIRE(t->arc_xy && t->arc_ptr && t->arc_keep && t->point_count && t->point_fill, DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  DM_REQUIRE(!tables || (t->new_ptr && t->seg && t->kind && t->cell_count && t->cell_fill && t->status), DM_ERR_BAD_SHAPE, "%s: null pointer", what);
  DM_REQUIRE(t->H > 0 && t->W > 0 && t->H < MAX_TOPOLOGY_SIDE && t->W < MAX_TOPOLOGY_SIDE, DM_ERR_BAD_SHAPE,
             "%s: bad scene (H=%d W=%d; need sides in 1..2^31-2)", what, t->H, t->W);
  DM_REQUIRE(t->cell_log2 >= DM_SCENE_SIMPLIFY_TOPOLOGY_MIN_CELL_LOG2 && t->cell_log2 <= DM_SCENE_SIMPLIFY_TOPOLOGY_MAX_CELL_LOG2, DM_ERR_BAD_SHAPE,
             "%s: bad cell side (cell_log2=%d; need 5 <= cell_log2 <= 24)", what, t->cell_log2);
  const long long cells = ((long long)(t->H >> t->cell_log2) + 1) * ((long long)(t->W >> t->cell_log2) + 1);       // each factor at most 2^26 + 1
  DM_REQUIRE(cells <= DM_SCENE_SIMPLIFY_TOPOLOGY_MAX_CELLS, DM_ERR_BAD_SHAPE,
             "%s: bad grid (cells=%lld for H=%d W=%d cell_log2=%d; need ((H >> cell_log2) + 1) ((W >> cell_log2) + 1) <= 2^22)", what, cells, t->H, t->W,
             t->cell_log2);
  DM_REQUIRE(t->A > 0 && t->A < (1 << 30) && t->Va >= 2 && t->Va <= (1LL << 30), DM_ERR_BAD_SHAPE,
             "%s: bad sizes (A=%d Va=%lld; need 1 <= A < 2^30, 2 <= Va <= 2^30)", what, t->A, (long long)t->Va);
  DM_REQUIRE(t->q >= 0 && t->q <= DM_SIMPLIFY_MAX_Q, DM_ERR_BAD_SHAPE, "%s: bad tolerance (q=%d; need 0 <= q <= 2^20)", what, t->q);
  DM_REQUIRE(!tables || (t->cap >= 1 && t->cap <= INT32_MAX), DM_ERR_BAD_SHAPE, "%s: bad sizes (cap=%lld; need 1 <= cap < 2^31)", what,
             (long long)t->cap);
  return DM_OK;
}

struct SceneTopology {
  typedef DmSceneSimplifyTopology Struct;
  typedef VertexKeep<unsigned char> Keep;
  typedef VertexKeep<const unsigned char> KeepRead;
  static __host__ __device__ __forceinline__ int log2(const Struct &t) { return t.cell_log2; }
  static __device__ __forceinline__ Keep keep(const Struct &t) { return Keep{t.arc_keep, t.H, t.W}; }
  static __device__ __forceinline__ KeepRead keep_read(const Struct &t) { return KeepRead{t.arc_keep, t.H, t.W}; }
  static int ok(const char *what, const Struct *t, bool tables) { return scene_topology_ok(what, t, tables); }
};

}  // namespace

extern "C" int dm_scene_simplify_topology_point_count(const DmSceneSimplifyTopology *t, void *stream) {
  return topo_point_count<SceneTopology>("dm_scene_simplify_topology_point_count", t, stream);
}
extern "C" int dm_scene_simplify_topology_point_fill(const DmSceneSimplifyTopology *t, void *stream) {
  return topo_point_fill<SceneTopology>("dm_scene_simplify_topology_point_fill", t, stream);
}
extern "C" int dm_scene_simplify_topology_segments(const DmSceneSimplifyTopology *t, void *stream) {
  return topo_segments<SceneTopology>("dm_scene_simplify_topology_segments", t, stream);
}
extern "C" int dm_scene_simplify_topology_bin_count(const DmSceneSimplifyTopology *t, void *stream) {
  return topo_bin<SceneTopology, false>("dm_scene_simplify_topology_bin_count", t, stream);
}
extern "C" int dm_scene_simplify_topology_bin_fill(const DmSceneSimplifyTopology *t, void *stream) {
  return topo_bin<SceneTopology, true>("dm_scene_simplify_topology_bin_fill", t, stream);
}
extern "C" int dm_scene_simplify_topology_pairs(const DmSceneSimplifyTopology *t, void *stream) {
  return topo_pairs<SceneTopology>("dm_scene_simplify_topology_pairs", t, stream);
}
extern "C" int dm_scene_simplify_topology_jumps(const DmSceneSimplifyTopology *t, void *stream) {
  return topo_jumps<SceneTopology>("dm_scene_simplify_topology_jumps", t, stream);
}
extern "C" int dm_scene_simplify_topology_refine(const DmSceneSimplifyTopology *t, int32_t apply, void *stream) {
  return topo_refine<SceneTopology>("dm_scene_simplify_topology_refine", t, apply, stream);
}
