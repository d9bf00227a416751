// Polygon rings rasterised into a label raster (gfx950): the inverse of dm_vector.hip.  The reference reads its superpixels, and
// its users digitise their ground truth, as polygons written by external GIS software; every raster pass of this build starts from
// a label raster.  The rule is the build's own: stated in include/deepmerge_hip.h, restated in numpy in tests/rasterize_ref.py
// (DESIGN.md 3.5.6).  Coordinates are fixed point with 8 sub-pixel bits and every product is an integer below 2^60, so the device
// and the spec agree bit for bit; the raster is written with integer max alone, so no result depends on the order of arrival.
//
// The kernels (count per edge, emit per event, fill per pair of the sorted keys) are dm_rasterize_kernels.h's, here on the band
// [0, H) and the window [0, W): the whole raster.
// The scan of the counts and the sort of the keys between the stages are the caller's (rag.rasterize: torch.cumsum, torch.sort).
#include "dm_rasterize_kernels.h"

namespace {

inline bool raster_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W < (1LL << 31); }

}  // namespace

extern "C" int dm_rasterize_count(const int32_t *xy, const int64_t *ring_ptr, const int32_t *vert_ring, int32_t V, int32_t R, int32_t H, int32_t W,
                                  int32_t *count, void *stream) {
  DM_REQUIRE(xy && ring_ptr && vert_ring && count, DM_ERR_BAD_SHAPE, "dm_rasterize_count: null pointer");
  DM_REQUIRE(raster_ok(H, W) && V > 0 && V <= (1 << 30) && R > 0, DM_ERR_BAD_SHAPE,
             "dm_rasterize_count: bad sizes (H=%d W=%d V=%d R=%d; need H, W, R >= 1, 1 <= V <= 2^30, H*W < 2^31)",
             H, W, V, R);
  hipLaunchKernelGGL(rasterize_count_kernel, dim3(grid_for(V)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), xy,
                     (const long long *)ring_ptr, vert_ring, V, R, 0, H, count);
  DM_LAUNCH_CHECK("dm_rasterize_count");
  return DM_OK;
}

extern "C" int dm_rasterize_emit(const int32_t *xy, const int64_t *ring_ptr, const int32_t *vert_ring, const int32_t *ring_label,
                                 const int64_t *scan, int32_t V, int32_t R, int64_t N, int32_t H, int32_t W, int64_t n_labels, int64_t *keys,
                                 void *stream) {
  DM_REQUIRE(xy && ring_ptr && vert_ring && ring_label && scan && keys, DM_ERR_BAD_SHAPE, "dm_rasterize_emit: null pointer");
  DM_REQUIRE(raster_ok(H, W) && V > 0 && V <= (1 << 30) && R > 0 && N > 0 && N <= (1LL << 30) && n_labels > 0 && n_labels < (1LL << 31), DM_ERR_BAD_SHAPE,
             "dm_rasterize_emit: bad sizes (H=%d W=%d V=%d R=%d N=%lld n_labels=%lld; need 1 <= V, N <= 2^30, 1 <= n_labels < 2^31, H*W < 2^31)", H, W,
             V, R, (long long)N, (long long)n_labels);
  DM_REQUIRE(n_labels <= LLONG_MAX / ((long long)H * (W + 1LL)), DM_ERR_BAD_SHAPE,
             "dm_rasterize_emit: key bound exceeded (n_labels=%lld H=%d W=%d; need n_labels*H*(W+1) < 2^63)", (long long)n_labels, H, W);
  hipLaunchKernelGGL(rasterize_emit_kernel, dim3(grid_for(N)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), xy,
                     (const long long *)ring_ptr, vert_ring, ring_label, (const long long *)scan, V, R, (long long)N, 0, H, W, (long long *)keys);
  DM_LAUNCH_CHECK("dm_rasterize_emit");
  return DM_OK;
}

extern "C" int dm_rasterize_fill(const int64_t *keys, int64_t N, int32_t H, int32_t W, int32_t fill, int32_t *out, int32_t *error, void *stream) {
  DM_REQUIRE(out && error && (N == 0 || keys), DM_ERR_BAD_SHAPE, "dm_rasterize_fill: null pointer");
  DM_REQUIRE(raster_ok(H, W) && N >= 0 && N <= (1LL << 30) && N % 2 == 0 && fill < 0, DM_ERR_BAD_SHAPE,
             "dm_rasterize_fill: bad arguments (H=%d W=%d N=%lld fill=%d; need H, W >= 1, H*W < 2^31, N even in 0..2^30, fill < 0)", H, W,
             (long long)N, fill);
  launch_fill(keys, N, H, W, 0, W, fill, out, error, reinterpret_cast<hipStream_t>(stream));
  DM_LAUNCH_CHECK("dm_rasterize_fill");
  return DM_OK;
}
