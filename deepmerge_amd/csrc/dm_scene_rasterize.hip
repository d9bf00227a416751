// Polygon rings rasterised on a scene (gfx950): dm_rasterize.hip's event passes restricted to a band of pixel rows, and its fill
// restricted to a window of columns (scene.RingSource).  The scene H x W may have 2^31 pixels or more: no raster
// of it exists, on the device or anywhere.  A band [r0, r1) is counted, emitted and sorted once; every window [x0, x1) of it is
// one fill into a dense int32 [r1 - r0, x1 - x0].  The rule is unchanged (include/deepmerge_hip.h; in its band and window form in
// tests/scene_rasterize_ref.py): cx is clamped to [0, W] scene-wide, so a crossing left of a window still toggles the parity
// inside it, and a window's pixels are those of the whole raster.  The kernels are dm_rasterize_kernels.h's.
#include "dm_rasterize_kernels.h"

namespace {

inline bool band_ok(int H, int W, int r0, int r1) { return H > 0 && W > 0 && r0 >= 0 && r0 < r1 && r1 <= H; }

}  // namespace

extern "C" int dm_rasterize_count_rows(const int32_t *xy, const int64_t *ring_ptr, const int32_t *vert_ring, int32_t V, int32_t R, int32_t H,
                                       int32_t W, int32_t r0, int32_t r1, int32_t *count, void *stream) {
  DM_REQUIRE(xy && ring_ptr && vert_ring && count, DM_ERR_BAD_SHAPE, "dm_rasterize_count_rows: null pointer");
  DM_REQUIRE(band_ok(H, W, r0, r1), DM_ERR_BAD_SHAPE, "dm_rasterize_count_rows: bad band (H=%d W=%d r0=%d r1=%d; need H, W >= 1, 0 <= r0 < r1 <= H)",
             H, W, r0, r1);
  DM_REQUIRE(V > 0 && V <= (1 << 30) && R > 0, DM_ERR_BAD_SHAPE, "dm_rasterize_count_rows: bad sizes (V=%d R=%d; need R >= 1, 1 <= V <= 2^30)", V, R);
  hipLaunchKernelGGL(rasterize_count_kernel, dim3(grid_for(V)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), xy,
                     (const long long *)ring_ptr, vert_ring, V, R, r0, r1, count);
  DM_LAUNCH_CHECK("dm_rasterize_count_rows");
  return DM_OK;
}

extern "C" int dm_rasterize_emit_rows(const int32_t *xy, const int64_t *ring_ptr, const int32_t *vert_ring, const int32_t *ring_label,
                                      const int64_t *scan, int32_t V, int32_t R, int64_t N, int32_t H, int32_t W, int32_t r0, int32_t r1,
                                      int64_t n_labels, int64_t *keys, void *stream) {
  DM_REQUIRE(xy && ring_ptr && vert_ring && ring_label && scan && keys, DM_ERR_BAD_SHAPE, "dm_rasterize_emit_rows: null pointer");
  DM_REQUIRE(band_ok(H, W, r0, r1), DM_ERR_BAD_SHAPE, "dm_rasterize_emit_rows: bad band (H=%d W=%d r0=%d r1=%d; need H, W >= 1, 0 <= r0 < r1 <= H)",
             H, W, r0, r1);
  DM_REQUIRE(V > 0 && V <= (1 << 30) && R > 0 && N > 0 && N <= (1LL << 30) && n_labels > 0 && n_labels < (1LL << 31), DM_ERR_BAD_SHAPE,
             "dm_rasterize_emit_rows: bad sizes (V=%d R=%d N=%lld n_labels=%lld; need R >= 1, 1 <= V, N <= 2^30 events per band, 1 <= n_labels < 2^31)",
             V, R, (long long)N, (long long)n_labels);
  DM_REQUIRE(n_labels <= LLONG_MAX / ((long long)(r1 - r0) * (W + 1LL)), DM_ERR_BAD_SHAPE,
             "dm_rasterize_emit_rows: key bound exceeded (n_labels=%lld rows=%d W=%d; need n_labels*(r1-r0)*(W+1) < 2^63)", (long long)n_labels,
             r1 - r0, W);
  hipLaunchKernelGGL(rasterize_emit_kernel, dim3(grid_for(N)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), xy,
                     (const long long *)ring_ptr, vert_ring, ring_label, (const long long *)scan, V, R, (long long)N, r0, r1, W, (long long *)keys);
  DM_LAUNCH_CHECK("dm_rasterize_emit_rows");
  return DM_OK;
}

extern "C" int dm_rasterize_fill_window(const int64_t *keys, int64_t N, int32_t H, int32_t W, int32_t r0, int32_t r1, int32_t x0, int32_t x1,
                                        int32_t fill, int32_t *out, int32_t *error, void *stream) {
  DM_REQUIRE(out && error && (N == 0 || keys), DM_ERR_BAD_SHAPE, "dm_rasterize_fill_window: null pointer");
  DM_REQUIRE(band_ok(H, W, r0, r1), DM_ERR_BAD_SHAPE, "dm_rasterize_fill_window: bad band (H=%d W=%d r0=%d r1=%d; need H, W >= 1, 0 <= r0 < r1 <= H)",
             H, W, r0, r1);
  DM_REQUIRE(x0 >= 0 && x0 < x1 && x1 <= W && (long long)(r1 - r0) * (x1 - x0) < (1LL << 31), DM_ERR_BAD_SHAPE,
             "dm_rasterize_fill_window: bad window (x0=%d x1=%d rows=%d W=%d; need 0 <= x0 < x1 <= W and fewer than 2^31 pixels)", x0, x1, r1 - r0, W);
  DM_REQUIRE(N >= 0 && N <= (1LL << 30) && N % 2 == 0 && fill < 0, DM_ERR_BAD_SHAPE,
             "dm_rasterize_fill_window: bad arguments (N=%lld fill=%d; need N even in 0..2^30, fill < 0)", (long long)N, fill);
  launch_fill(keys, N, r1 - r0, W, x0, x1, fill, out, error, reinterpret_cast<hipStream_t>(stream));
  DM_LAUNCH_CHECK("dm_rasterize_fill_window");
  return DM_OK;
}
