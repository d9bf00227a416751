// A scene's label raster traced into rings and arcs across tile seams (gfx950).  DESIGN.md 3.5.10.
// The rule is dm_vector.hip's, unchanged; what is new is where the darts come from and how wide their ids are.  The scene is read
// tile by tile: the core [cy0, cy1) x [cx0, cx1) of a tile inside its window, the core grown by one pixel of the neighbours'
// labels and clipped to the scene.  Only the core's pixels own darts, with scene-wide ids 4 ((y + oy) W + (x + ox)) + side, int64.
//   count      dm_vector.h's tile walk over the window: the side mask of every window pixel, the same mask zeroed outside the core,
//              darts per tile from the core mask, the scan.  dm_vector_emit then runs unchanged on the core mask.
//   link       per core dart: its scene id, its successor's scene id, label, other label, and the vertex / break flag that belongs
//              to the successor -- returned, not scattered: the successor's slot may lie in another tile's table.
//   emit64     dm_vector.h's ring and arc emit over the joined table, dart ids and W in 64 bits, arc_first = slot.
// Why one pixel of apron is enough: a core dart consults its own pixel, the ahead-right and the ahead-left pixel, and the pixel
// across the successor's side; all are 8-neighbours of the core pixel.  A window edge that is not a scene edge is therefore never
// consulted for a core dart, and a window edge that is a scene edge is the raster's outside, as in the one-raster rule.
// The join of the tiles' tables (one sort by id, one searchsorted) is the caller's (scene.trace_labels).
#include "dm_vector.h"

namespace {

__global__ void scene_vec_link_kernel(const int *__restrict__ labels, const unsigned char *__restrict__ mask, const int *__restrict__ dart,
                                      int H, int W, int D, long long oy, long long ox, long long scene_w, long long *__restrict__ id_out,
                                      long long *__restrict__ succ_out, int *__restrict__ lab, int *__restrict__ other,
                                      unsigned char *__restrict__ succ_flags) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < D; i += gridDim.x * blockDim.x) {
    const int id = dart[i], pix = id >> 2, s = id & 3;          // window-local: the window has at most 2^28 pixels
    const int y = pix / W, x = pix - y * W;
    int qx = x, qy = y;
    const int t = successor_of(mask, W, qx, qy, s);
    const int o = label_across(labels, H, W, x, y, s);
    id_out[i] = 4 * ((y + oy) * scene_w + (x + ox)) + s;
    succ_out[i] = 4 * ((qy + oy) * scene_w + (qx + ox)) + t;
    lab[i] = labels[pix];
    other[i] = o;
    succ_flags[i] = (unsigned char)((t != s ? VTX : 0) | (label_across(labels, H, W, qx, qy, t) != o ? BRK : 0));
  }
}

inline bool window_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W <= (1LL << 28); }

}  // namespace

extern "C" int dm_scene_vector_count(const int32_t *labels, int32_t H, int32_t W, int32_t cy0, int32_t cy1, int32_t cx0, int32_t cx1,
                                     uint8_t *mask, uint8_t *core_mask, int32_t *tile_off, int32_t *n_darts, void *stream) {
  DM_REQUIRE(labels && mask && core_mask && tile_off && n_darts && mask != core_mask, DM_ERR_BAD_SHAPE,
             "dm_scene_vector_count: null pointer (or mask == core_mask)");
  DM_REQUIRE(window_ok(H, W), DM_ERR_BAD_SHAPE, "dm_scene_vector_count: need 1 <= H*W <= 2^28 (H=%d W=%d)", H, W);
  DM_REQUIRE(0 <= cy0 && cy0 < cy1 && cy1 <= H && 0 <= cx0 && cx0 < cx1 && cx1 <= W && cy0 <= 1 && cx0 <= 1 && H - cy1 <= 1 && W - cx1 <= 1,
             DM_ERR_BAD_SHAPE, "dm_scene_vector_count: the core [%d,%d) x [%d,%d) must lie in the window %d x %d with an apron of 0 or 1", cy0,
             cy1, cx0, cx1, H, W);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid = tile_grid(H, W);
  const bool vec = W % STRIP == 0 && dm_aligned16(labels) && dm_aligned16(mask) && dm_aligned16(core_mask);
  if (vec) hipLaunchKernelGGL((vec_count_kernel<true, true>), grid, dim3(256), 0, s, labels, H, W, mask, tile_off, core_mask, cy0, cy1, cx0, cx1);
  else hipLaunchKernelGGL((vec_count_kernel<false, true>), grid, dim3(256), 0, s, labels, H, W, mask, tile_off, core_mask, cy0, cy1, cx0, cx1);
  hipLaunchKernelGGL(vec_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, tile_off, (int)grid.x, n_darts);
  DM_LAUNCH_CHECK("dm_scene_vector_count");
  return DM_OK;
}

extern "C" int dm_scene_vector_link(const int32_t *labels, const uint8_t *mask, const int32_t *dart, int32_t H, int32_t W, int32_t D,
                                    int64_t oy, int64_t ox, int64_t scene_h, int64_t scene_w, int64_t *id, int64_t *succ, int32_t *lab,
                                    int32_t *other, uint8_t *succ_flags, void *stream) {
  DM_REQUIRE(labels && mask && dart && id && succ && lab && other && succ_flags, DM_ERR_BAD_SHAPE, "dm_scene_vector_link: null pointer");
  DM_REQUIRE(window_ok(H, W) && D >= 1 && (long long)D <= 4LL * H * W, DM_ERR_BAD_SHAPE, "dm_scene_vector_link: bad sizes (H=%d W=%d D=%d)", H,
             W, D);
  DM_REQUIRE(scene_h >= 1 && scene_w >= 1 && scene_h < DM_SCENE_VECTOR_MAX_SIDE && scene_w < DM_SCENE_VECTOR_MAX_SIDE &&
                 scene_h <= DM_SCENE_VECTOR_MAX_PIXELS / scene_w && oy >= 0 && ox >= 0 && oy + H <= scene_h && ox + W <= scene_w,
             DM_ERR_BAD_SHAPE, "dm_scene_vector_link: the window %d x %d at (y=%lld, x=%lld) must lie in a scene of %lld x %lld, sides < 2^31-1, "
             "at most 2^60 pixels", H, W, (long long)oy, (long long)ox, (long long)scene_h, (long long)scene_w);
  hipLaunchKernelGGL(scene_vec_link_kernel, dim3(grid_for(D)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), labels, mask, dart, H, W, D,
                     (long long)oy, (long long)ox, (long long)scene_w, (long long *)id, (long long *)succ, lab, other, succ_flags);
  DM_LAUNCH_CHECK("dm_scene_vector_link");
  return DM_OK;
}

extern "C" int dm_scene_vector_ring_emit(const DmSceneVectorTrace *t, void *stream) {
  if (int rc = vector_trace_ok(t, "dm_scene_vector_ring_emit", false)) return rc;
  DM_REQUIRE(t->W < DM_SCENE_VECTOR_MAX_SIDE, DM_ERR_BAD_SHAPE, "dm_scene_vector_ring_emit: W must be below 2^31-1, got %lld", (long long)t->W);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vec_ring_init_kernel, dim3(grid_for(t->n_arcs)), dim3(256), 0, s, (long long *)t->area2, t->R, t->arc_count, t->n_arcs);
  hipLaunchKernelGGL((vec_ring_emit_kernel<DmSceneVectorTrace, long long, true>), dim3(grid_for(t->D)), dim3(256), 0, s, *t);
  DM_LAUNCH_CHECK("dm_scene_vector_ring_emit");
  return DM_OK;
}

extern "C" int dm_scene_vector_arc_emit(const DmSceneVectorTrace *t, void *stream) {
  if (int rc = vector_trace_ok(t, "dm_scene_vector_arc_emit", true)) return rc;
  DM_REQUIRE(t->W < DM_SCENE_VECTOR_MAX_SIDE, DM_ERR_BAD_SHAPE, "dm_scene_vector_arc_emit: W must be below 2^31-1, got %lld", (long long)t->W);
  hipLaunchKernelGGL((vec_arc_emit_kernel<DmSceneVectorTrace, long long>), dim3(grid_for(t->D)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), *t);
  DM_LAUNCH_CHECK("dm_scene_vector_arc_emit");
  return DM_OK;
}
