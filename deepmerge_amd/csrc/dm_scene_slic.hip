// SLIC steps 1-3 on a scene larger than one tile (gfx950): one scene-wide table of centres, the pixels streamed core by core
// (scene.slic_assign / scene.slic_labels; the rule and its scene form: include/deepmerge_hip.h).
//
// A pixel's assignment depends on its own colour, its position and the nine centres around its grid cell, and the next centres
// are integer sums: given the scene's table a core needs no halo and no neighbour's labels, and the sums over the cores are the
// sums over the scene.  So the kernels are dm_slic.hip's, told where the core lies:
//   scene_slic_init_kernel   the centres whose start pixel lies in the core take their position and colour; their sums are cleared.
//                            Every core runs it before any core is assigned.
//   slic_pass_kernel         dm_slic_pass.h in its scene form: positions, grid cells and the staged window of centres in scene
//                            coordinates, sums flushed as acc + n * (y0 + Y0) in 64 bits, labels written core-locally.
//   slic_update_kernel       dm_slic_pass.h, unchanged: once per round over the whole table.
// Integers only; no result depends on the order in which threads or cores arrive.
#include "dm_slic_pass.h"

namespace {

// A thread per grid cell that meets the core.  The start pixel of cell (j, i) lies in that cell (the clamp to H-1 / W-1 only
// applies in the last row / column, which holds H-1 / W-1), so the cells that meet the core are all that can start in it.
__global__ void scene_slic_init_kernel(const uint8_t *__restrict__ core, long long plane, int h, int w, int y0, int x0, int H, int W, int nb,
                                       int cell, int gx, int ja, int ia, int ni, long long n, int *__restrict__ centres,
                                       long long *__restrict__ sums) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int j = ja + (int)(t / ni), i = ia + (int)(t % ni);
  const long long y = min((long long)H - 1, (long long)j * cell + cell / 2), x = min((long long)W - 1, (long long)i * cell + cell / 2);
  if (y < y0 || y >= (long long)y0 + h || x < x0 || x >= (long long)x0 + w) return;
  const long long c = (long long)j * gx + i;
  centres[c * CENTRE_INTS + 0] = (int)y;
  centres[c * CENTRE_INTS + 1] = (int)x;
  for (int b = 0; b < 4; ++b) centres[c * CENTRE_INTS + 2 + b] = b < nb ? (int)core[b * plane + (y - y0) * w + (x - x0)] : 0;
  for (int k = 0; k < SUM_INTS; ++k) sums[c * SUM_INTS + k] = 0;
}

// The checks the two per-core entries share; 0 when the core and the grid are in range.
const char *bad_core(const void *core, int bands, int h, int w, int y0, int x0, int H, int W, int cell) {
  if (!core) return "null pointer";
  if (!(bands >= 1 && h > 0 && w > 0 && (long long)h * w < (1LL << 31))) return "bad core (need bands >= 1, h, w >= 1, h*w < 2^31)";
  if (!(H > 0 && W > 0 && y0 >= 0 && x0 >= 0 && (long long)y0 + h <= H && (long long)x0 + w <= W)) return "the core does not lie in the scene";
  if (!(cell >= 4 && cell <= 256)) return "cell outside 4..256";
  const long long gy = ((long long)H + cell - 1) / cell, gx = ((long long)W + cell - 1) / cell;
  if (gy * gx >= (1LL << 31)) return "the grid has 2^31 centres or more";
  return nullptr;
}

}  // namespace

extern "C" int dm_scene_slic_init(const uint8_t *core, int32_t bands, int32_t h, int32_t w, int32_t y0, int32_t x0, int32_t H, int32_t W,
                                  int32_t cell, int32_t *centres, int64_t *sums, void *stream) {
  DM_REQUIRE(centres && sums, DM_ERR_BAD_SHAPE, "dm_scene_slic_init: null pointer");
  const char *bad = bad_core(core, bands, h, w, y0, x0, H, W, cell);
  DM_REQUIRE(!bad, DM_ERR_BAD_SHAPE, "dm_scene_slic_init: %s (bands=%d core %d x %d at (%d, %d) of %d x %d, cell=%d)", bad, bands, h, w, y0, x0, H,
             W, cell);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nb = bands < 4 ? bands : 4;
  const int gx = (int)(((long long)W + cell - 1) / cell);
  const int ja = y0 / cell, jb = (int)(((long long)y0 + h - 1) / cell), ia = x0 / cell, ib = (int)(((long long)x0 + w - 1) / cell);
  const int ni = ib - ia + 1;
  const long long n = (long long)(jb - ja + 1) * ni;            // <= (h / 4 + 2) (w / 4 + 2): below 2^31
  hipLaunchKernelGGL(scene_slic_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, core, (long long)h * w, h, w, y0, x0, H, W, nb,
                     cell, gx, ja, ia, ni, n, centres, (long long *)sums);
  DM_LAUNCH_CHECK("dm_scene_slic_init");
  return DM_OK;
}

extern "C" int dm_scene_slic_pass(const uint8_t *core, int32_t bands, int32_t h, int32_t w, int32_t y0, int32_t x0, int32_t H, int32_t W,
                                  int32_t cell, int32_t compactness, const int32_t *centres, int64_t *sums, int32_t *labels, void *stream) {
  DM_REQUIRE(centres, DM_ERR_BAD_SHAPE, "dm_scene_slic_pass: null pointer");
  DM_REQUIRE(sums || labels, DM_ERR_BAD_SHAPE, "dm_scene_slic_pass: null pointer (sums and labels: at least one is needed)");
  const char *bad = bad_core(core, bands, h, w, y0, x0, H, W, cell);
  DM_REQUIRE(!bad, DM_ERR_BAD_SHAPE, "dm_scene_slic_pass: %s (bands=%d core %d x %d at (%d, %d) of %d x %d, cell=%d)", bad, bands, h, w, y0, x0, H,
             W, cell);
  DM_REQUIRE(compactness >= 0 && compactness <= 255, DM_ERR_BAD_SHAPE, "dm_scene_slic_pass: compactness = %d outside 0..255", compactness);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nb = bands < 4 ? bands : 4;
  const int gy = (int)(((long long)H + cell - 1) / cell), gx = (int)(((long long)W + cell - 1) / cell);
  const unsigned comp2 = (unsigned)(compactness * compactness);
  // 16-byte strip loads / stores need w % 16 == 0 (then every band plane keeps the alignment) and 16-byte aligned rasters
  const bool vec = w % STRIP == 0 && dm_aligned16(core) && (!labels || dm_aligned16(labels));
  const SlicPass pass = {nb, slic_wide(cell, nb, comp2), vec, h, w, y0, x0, H, W, cell, gy, gx, comp2};
  slic_pass<true>(pass, s, core, centres, (long long *)sums, labels);
  DM_LAUNCH_CHECK("dm_scene_slic_pass");
  return DM_OK;
}

extern "C" int dm_scene_slic_update(int32_t K, int32_t *centres, int64_t *sums, void *stream) {
  DM_REQUIRE(centres && sums, DM_ERR_BAD_SHAPE, "dm_scene_slic_update: null pointer");
  DM_REQUIRE(K >= 1, DM_ERR_BAD_SHAPE, "dm_scene_slic_update: K = %d is not positive", K);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(slic_update_kernel, dim3((unsigned)(((long long)K + 255) / 256)), dim3(256), 0, s, K, centres, (long long *)sums);
  DM_LAUNCH_CHECK("dm_scene_slic_update");
  return DM_OK;
}
