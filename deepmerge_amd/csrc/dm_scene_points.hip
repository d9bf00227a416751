// Sample points of a scene's label raster whose regions cross tile seams (gfx950; DESIGN.md 3.5.14, scene.sample_points).
// The rule is dm_points.hip's, word for word, with "linear index" read as the SCENE's y * W + x: a region's pixels lie in several
// tiles, so a round's per-region maximum is taken over all of them.  The state (best, points, point_clearance, counts, bbox) is
// scene-wide and stays on the device; per round every tile's halo window is visited once (select), then the round's winners
// become points (commit).  Only the window's core pixels are candidates: the halo is there so that the window's clearance
// (dm_label_clearance on the window) equals the scene's at every core pixel.
//
// The key.  score (<= cap <= 192) in bits 56..63, 2^48 - 1 - lin in bits 8..55, the pixel's clearance (<= 192) in bits 0..7.
// Positions are unique, so the clearance never decides an order: it rides behind the position, and the commit kernel needs
// neither a raster nor a tile.  Largest score first, then smallest scene linear index: one unsigned 64-bit max per region.
//
// Integer work on integer atomics only: nothing depends on the order in which threads, tiles or windows arrive.
#include "dm_raster.h"

namespace {

constexpr int TSLOTS_LOG2 = 6, TSLOTS = 1 << TSLOTS_LOG2;      // labels per 64x64 tile kept in LDS (more: global atomics)
constexpr int KMAX = 16;                                       // points per superpixel
constexpr u64 LIN_MASK = (1ULL << 48) - 1;

__device__ __forceinline__ u64 scene_key(int score, long long lin, int c) {
  return ((u64)(unsigned)score << 56) | ((LIN_MASK - (u64)lin) << 8) | (u64)(unsigned)c;
}

__global__ void scene_point_init_kernel(u64 *__restrict__ best, int *__restrict__ cnt, int *__restrict__ bbox, int S) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  best[s] = 0;
  cnt[s] = 0;
  box_init(bbox + 4 * s);
}

// Round j over the core rectangle (cy0, cx0, ch x cw) of a window of ww columns whose first pixel is (oy, ox) of a scene of
// SW columns.  The tile walk runs over the core; x, y below are SCENE coordinates.  FIRST (j == 0): no earlier points, and the
// bounding box rides along.  VEC: every whole strip starts on a 16-byte boundary of both rasters (the host checks it).
template <bool FIRST, bool VEC>
__global__ __launch_bounds__(256) void scene_point_select_kernel(const int *__restrict__ labels, const unsigned short *__restrict__ clr, int ww,
                                                                 int cy0, int cx0, int ch, int cw, int oy, int ox, long long SW, int S,
                                                                 int k, int j, const int *__restrict__ pts, const int *__restrict__ cnt,
                                                                 u64 *__restrict__ best, int *__restrict__ bbox) {
  __shared__ int t_key[TSLOTS];
  __shared__ u64 t_best[TSLOTS];
  __shared__ int t_box[TSLOTS][4];
  __shared__ int t_np[TSLOTS];
  __shared__ int t_pt[TSLOTS][KMAX][2];
  for (int i = threadIdx.x; i < TSLOTS; i += blockDim.x) {
    t_key[i] = -1; t_best[i] = 0; t_np[i] = 0;
    box_init(t_box[i]);
  }
  __syncthreads();
  const Strip g = strip_of(ch, cw);                             // in core coordinates
  const int n = g.n;
  const long long base = (long long)(cy0 + g.y) * ww + cx0 + g.x0;      // in the window; read only when n > 0
  const int y = oy + cy0 + g.y, x0 = ox + cx0 + g.x0;           // in the scene
  const long long lin0 = (long long)y * SW + x0;
  int lab[STRIP], c[STRIP];
  load_strip<VEC>(labels, base, n, -1, lab);
  if (VEC && n == STRIP) {
#pragma unroll
    for (int v = 0; v < STRIP / 8; ++v) {
      const u32x4 q = *reinterpret_cast<const u32x4 *>(clr + base + 8 * v);
#pragma unroll
      for (int e = 0; e < 8; ++e) c[8 * v + e] = (int)((q[e >> 1] >> (16 * (e & 1))) & 0xFFFFu);
    }
  } else {
#pragma unroll
    for (int i = 0; i < STRIP; ++i) c[i] = (i < n) ? (int)clr[base + i] : 0;
  }
  if (!FIRST) {
    // claim the strip's labels, then load every claimed label's earlier points once for the whole tile
    int cur = -1;
#pragma unroll
    for (int i = 0; i < STRIP; ++i) {
      if (i >= n) break;
      const int l = lab[i];
      if (l != cur) {
        cur = l;
        if ((unsigned)l < (unsigned)S) claim_label_slot<TSLOTS_LOG2>(t_key, l);
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TSLOTS * KMAX; i += blockDim.x) {
      const int slot = i / KMAX, q = i - slot * KMAX;
      const int l = t_key[slot];
      if (l < 0) continue;
      const int np = min(min(j, k), cnt[l]);
      if (q == 0) t_np[slot] = np;
      if (q < np) {
        t_pt[slot][q][0] = pts[((long long)l * k + q) * 2];
        t_pt[slot][q][1] = pts[((long long)l * k + q) * 2 + 1];
      }
    }
    __syncthreads();
  }
  {
    int cur = -1, slot = -1, np = 0, run_x0 = 0;
    bool valid = false;
    u64 run_best = 0;
    auto flush = [&](int xend) {
      if (!valid) return;
      if (slot >= 0) {
        if (run_best) atomicMax(&t_best[slot], run_best);
        if (FIRST) box_fold(t_box[slot], run_x0, y, xend, y);
        return;
      }
      if (run_best) atomicMax(best + cur, run_best);
      if (FIRST) box_fold(bbox + 4 * cur, run_x0, y, xend, y);
    };
#pragma unroll
    for (int i = 0; i < STRIP; ++i) {
      if (i >= n) break;
      const int x = x0 + i;
      const int l = lab[i];
      if (l != cur) {
        flush(x - 1);
        cur = l; run_x0 = x; run_best = 0;
        valid = (unsigned)l < (unsigned)S;
        slot = valid ? claim_label_slot<TSLOTS_LOG2>(t_key, l) : -1;    // -1: table full, the label goes to global memory
        np = 0;
        if (!FIRST && valid) np = slot >= 0 ? t_np[slot] : min(min(j, k), cnt[l]);
      }
      if (!valid) continue;
      int score = c[i];
      if (!FIRST) {
        for (int q = 0; q < np; ++q) {
          const int px = slot >= 0 ? t_pt[slot][q][0] : pts[((long long)l * k + q) * 2];
          const int py = slot >= 0 ? t_pt[slot][q][1] : pts[((long long)l * k + q) * 2 + 1];
          score = min(score, max(abs(x - px), abs(y - py)));
        }
      }
      if (score >= 1) {
        const u64 key = scene_key(score, lin0 + i, c[i]);
        run_best = key > run_best ? key : run_best;
      }
    }
    if (g.live) flush(x0 + n - 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TSLOTS; i += blockDim.x) {      // one global max (and one box) per label of the tile
    const int l = t_key[i];
    if (l < 0) continue;
    if (t_best[i]) atomicMax(best + l, t_best[i]);
    if (FIRST && t_box[i][2] >= 0) box_fold(bbox + 4 * l, t_box[i][0], t_box[i][1], t_box[i][2], t_box[i][3]);
  }
}

// The round's scene-wide winners become points: position and clearance both come out of the key; best is cleared for the next round.
__global__ void scene_point_commit_kernel(u64 *__restrict__ best, long long SW, long long npix, int S, int k, int *__restrict__ pts,
                                          int *__restrict__ pclr, int *__restrict__ cnt) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const u64 b = best[s];
  if (!b) return;
  best[s] = 0;
  const long long lin = (long long)(LIN_MASK - ((b >> 8) & LIN_MASK));
  const int m = cnt[s];
  if (lin >= npix || m >= k) return;
  pts[((long long)s * k + m) * 2] = (int)(lin % SW);
  pts[((long long)s * k + m) * 2 + 1] = (int)(lin / SW);
  pclr[(long long)s * k + m] = (int)(b & 0xFFULL);
  cnt[s] = m + 1;
}

inline bool scene_ok(long long SH, long long SW) {
  return SH > 0 && SW > 0 && SH <= INT_MAX && SW <= INT_MAX && SH <= DM_SCENE_POINTS_MAX_PIXELS / SW;
}

}  // namespace

extern "C" int dm_scene_point_init(uint64_t *best, int32_t *counts, int32_t *bbox, int32_t S, void *stream) {
  DM_REQUIRE(best && counts && bbox, DM_ERR_BAD_SHAPE, "dm_scene_point_init: null pointer");
  DM_REQUIRE(S > 0, DM_ERR_BAD_SHAPE, "dm_scene_point_init: S = %d must be >= 1", S);
  hipLaunchKernelGGL(scene_point_init_kernel, dim3((S + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), (u64 *)best, counts,
                     bbox, S);
  DM_LAUNCH_CHECK("dm_scene_point_init");
  return DM_OK;
}

extern "C" int dm_scene_point_select(const int32_t *labels, const uint16_t *clearance, int32_t wh, int32_t ww, int32_t cy0, int32_t cy1,
                                     int32_t cx0, int32_t cx1, int64_t oy, int64_t ox, int64_t scene_h, int64_t scene_w, int32_t S,
                                     int32_t k, int32_t round, const int32_t *points, const int32_t *counts, uint64_t *best, int32_t *bbox,
                                     void *stream) {
  DM_REQUIRE(labels && clearance && best && points && counts && bbox, DM_ERR_BAD_SHAPE, "dm_scene_point_select: null pointer");
  DM_REQUIRE(wh > 0 && ww > 0 && (long long)wh * ww < (1LL << 31) && S > 0, DM_ERR_BAD_SHAPE,
             "dm_scene_point_select: bad sizes (wh=%d ww=%d S=%d; need wh*ww < 2^31)", wh, ww, S);
  DM_REQUIRE(0 <= cy0 && cy0 < cy1 && cy1 <= wh && 0 <= cx0 && cx0 < cx1 && cx1 <= ww, DM_ERR_BAD_SHAPE,
             "dm_scene_point_select: core rows %d..%d, columns %d..%d outside the %d x %d window", cy0, cy1, cx0, cx1, wh, ww);
  DM_REQUIRE(scene_ok(scene_h, scene_w), DM_ERR_BAD_SHAPE,
             "dm_scene_point_select: bad scene (H=%lld W=%lld; need H, W < 2^31 and H*W <= 2^48)", (long long)scene_h, (long long)scene_w);
  DM_REQUIRE(oy >= 0 && ox >= 0 && oy + wh <= scene_h && ox + ww <= scene_w, DM_ERR_BAD_SHAPE,
             "dm_scene_point_select: the window at (%lld, %lld) leaves the scene", (long long)oy, (long long)ox);
  DM_REQUIRE(k >= 1 && k <= KMAX, DM_ERR_BAD_SHAPE, "dm_scene_point_select: k = %d outside 1..16", k);
  DM_REQUIRE(round >= 0 && round < k, DM_ERR_BAD_SHAPE, "dm_scene_point_select: round = %d outside 0..k-1 (k = %d)", round, k);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ch = cy1 - cy0, cw = cx1 - cx0;
  const dim3 grid = tile_grid(ch, cw);
  // a whole strip starts at window index (cy0 + y) ww + cx0 + 16 m: 16-byte loads of int32 need it a multiple of 4, of uint16 of 8
  const bool vec = (ww % 8 == 0) && (cx0 % 8 == 0) && dm_aligned16(labels) && dm_aligned16(clearance);
#define DM_SCENE_SELECT(FIRST, VEC)                                                                                                        \
  hipLaunchKernelGGL((scene_point_select_kernel<FIRST, VEC>), grid, dim3(256), 0, s, labels, clearance, ww, cy0, cx0, ch, cw, (int)oy,      \
                     (int)ox, (long long)scene_w, S, k, round, points, counts, (u64 *)best, bbox)
  if (round == 0) {
    if (vec) DM_SCENE_SELECT(true, true); else DM_SCENE_SELECT(true, false);
  } else {
    if (vec) DM_SCENE_SELECT(false, true); else DM_SCENE_SELECT(false, false);
  }
#undef DM_SCENE_SELECT
  DM_LAUNCH_CHECK("dm_scene_point_select");
  return DM_OK;
}

extern "C" int dm_scene_point_commit(uint64_t *best, int64_t scene_h, int64_t scene_w, int32_t S, int32_t k, int32_t *points,
                                     int32_t *point_clearance, int32_t *counts, void *stream) {
  DM_REQUIRE(best && points && point_clearance && counts, DM_ERR_BAD_SHAPE, "dm_scene_point_commit: null pointer");
  DM_REQUIRE(scene_ok(scene_h, scene_w) && S > 0, DM_ERR_BAD_SHAPE,
             "dm_scene_point_commit: bad sizes (H=%lld W=%lld S=%d; need H, W < 2^31 and H*W <= 2^48)", (long long)scene_h, (long long)scene_w, S);
  DM_REQUIRE(k >= 1 && k <= KMAX, DM_ERR_BAD_SHAPE, "dm_scene_point_commit: k = %d outside 1..16", k);
  hipLaunchKernelGGL(scene_point_commit_kernel, dim3((S + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), (u64 *)best,
                     (long long)scene_w, (long long)scene_h * scene_w, S, k, points, point_clearance, counts);
  DM_LAUNCH_CHECK("dm_scene_point_commit");
  return DM_OK;
}
