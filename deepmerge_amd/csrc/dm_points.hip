// Sample points and window sides from a label raster (gfx950): the first stage of the ExtractFeatures pipeline.  The
// reference reads a point shapefile that external GIS software wrote (pixel position and the `inner` / `object` window
// fields, MyUtils1.py:64-66, MyUtils2.py:234-236, and the polygons' `PointID` lists) and never defines how it was made; this
// build derives the points on the device from the segmentation's label raster.  The rule is the build's own: it is stated in
// include/deepmerge_hip.h and restated in numpy in tests/points_ref.py.
//
// Every quantity is an integer and every reduction an integer min / max, so the result does not depend on the order in
// which threads arrive: the GPU and the numpy spec agree bit for bit.  No floating point anywhere in this file.
//
// Clearance c(p) = Chebyshev distance from p to the nearest pixel of another label or outside the raster, capped at
// cap = (max_window + 1) / 2.  c - 1 is the chessboard distance to the nearest BOUNDARY pixel (a pixel with an 8-neighbour of
// another label, or on the raster edge), which no longer looks at labels and is separable:
//   1. boundary_bits_kernel   one bit per pixel (a wave's ballot is one 64-bit word of the row)
//   2. row_distance_kernel    g(y, x) = distance to the nearest set bit of row y: count-leading / trailing-zeros on at most
//                             four words per side (cap - 1 <= 191), O(1) per pixel
//   3. column_clearance_kernel  c - 1 = min over y' of max(|y - y'|, g(y', x)): rows are visited outwards until |y - y'|
//                             reaches the best value so far, i.e. c rows up and c rows down per pixel (4 pixels per thread)
// Selection round j: one pass over the raster, key = (score << 32) | (0xFFFFFFFF - linear index), one 64-bit max per
// superpixel, on dm_raster.h's tile walk: the tile's labels get a slot in an LDS table, the strip's runs are folded there
// with 64-bit LDS max, and each label of the tile then costs ONE global 64-bit atomicMax.  Round 0 carries the bounding box in
// the same table.
#include "dm_raster.h"

namespace {

constexpr int TSLOTS_LOG2 = 6, TSLOTS = 1 << TSLOTS_LOG2;      // labels per 64x64 tile kept in LDS (more: global atomics)
constexpr int KMAX = 16;                                       // points per superpixel
constexpr int ROW_THREADS = 256;

// ---- clearance -----------------------------------------------------------------------------------------------------------
// A workgroup covers 256 consecutive pixels of one row: four waves, one 64-bit word each.
__global__ __launch_bounds__(ROW_THREADS) void boundary_bits_kernel(const int *__restrict__ labels, int H, int W, int WW, int groups,
                                                                    u64 *__restrict__ bits) {
  const int y = blockIdx.x / groups, g = blockIdx.x - y * groups;
  const int w = g * (ROW_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (y >= H || w >= WW) return;                               // wave-uniform
  const int x = w * 64 + lane;
  bool b = false;
  if (x < W) {
    b = x == 0 || y == 0 || x == W - 1 || y == H - 1;
    if (!b) {
      const int *row = labels + (long long)y * W + x;
      const int l = row[0];
      b = row[-1] != l || row[1] != l || row[-W - 1] != l || row[-W] != l || row[-W + 1] != l || row[W - 1] != l || row[W] != l ||
          row[W + 1] != l;
    }
  }
  const u64 mask = __ballot(b);
  if (lane == 0) bits[(long long)y * WW + w] = mask;
}

__global__ __launch_bounds__(ROW_THREADS) void row_distance_kernel(const u64 *__restrict__ bits, int H, int W, int WW, int groups, int capm1,
                                                                   unsigned char *__restrict__ g) {
  const int y = blockIdx.x / groups;
  const int x = (blockIdx.x - y * groups) * ROW_THREADS + threadIdx.x;
  if (y >= H || x >= W) return;
  const u64 *rb = bits + (long long)y * WW;
  const int w = x >> 6, bit = x & 63;
  int dl = capm1, dr = capm1;
  u64 m = rb[w] & (~0ULL >> (63 - bit));                       // this pixel and the ones left of it in its word
  if (m) {
    dl = bit - (63 - __builtin_clzll(m));
  } else {
    for (int k = 1; w - k >= 0; ++k) {
      const int base = bit + 1 + 64 * (k - 1);                 // distance to bit 63 of word w - k
      if (base > capm1) break;
      const u64 v = rb[w - k];
      if (v) { dl = base + __builtin_clzll(v); break; }
    }
  }
  m = rb[w] & (~0ULL << bit);
  if (m) {
    dr = __builtin_ctzll(m) - bit;
  } else {
    for (int k = 1; w + k < WW; ++k) {
      const int base = 64 - bit + 64 * (k - 1);                // distance to bit 0 of word w + k
      if (base > capm1) break;
      const u64 v = rb[w + k];
      if (v) { dr = base + __builtin_ctzll(v); break; }
    }
  }
  g[(long long)y * W + x] = (unsigned char)min(min(dl, dr), capm1);
}

// Thread = 4 consecutive pixels of one row (one 4-byte load per visited row); workgroup = 1024 pixels of the row.
template <bool VEC>
__global__ __launch_bounds__(ROW_THREADS) void column_clearance_kernel(const unsigned char *__restrict__ g, int H, int W, int groups,
                                                                       unsigned short *__restrict__ clr) {
  const int y = blockIdx.x / groups;
  const int x0 = ((blockIdx.x - y * groups) * ROW_THREADS + threadIdx.x) * 4;
  if (y >= H || x0 >= W) return;
  const int n = min(4, W - x0);
  auto load4 = [&](int yy) -> unsigned {                      // four row distances, 255 beyond the raster's right edge
    const unsigned char *p = g + (long long)yy * W + x0;
    if (VEC) return *reinterpret_cast<const unsigned *>(p);
    unsigned v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) v |= (unsigned)(i < n ? p[i] : 255) << (8 * i);
    return v;
  };
  int best[4];
  const unsigned own = load4(y);
  int reach = 0;                                              // rows further than every pixel's best cannot improve any of them
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    best[i] = i < n ? (int)((own >> (8 * i)) & 255) : 0;
    reach = max(reach, best[i]);
  }
  for (int dy = 1; dy < reach; ++dy) {
    const unsigned u = (y - dy >= 0) ? load4(y - dy) : 0xFFFFFFFFu;
    const unsigned d = (y + dy < H) ? load4(y + dy) : 0xFFFFFFFFu;
    reach = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = max(dy, (int)min((u >> (8 * i)) & 255, (d >> (8 * i)) & 255));
      best[i] = min(best[i], v);
      reach = max(reach, best[i]);
    }
  }
  unsigned short *out = clr + (long long)y * W + x0;
  if (VEC) {
    u32x2 o = {(unsigned)(best[0] + 1) | ((unsigned)(best[1] + 1) << 16), (unsigned)(best[2] + 1) | ((unsigned)(best[3] + 1) << 16)};
    *reinterpret_cast<u32x2 *>(out) = o;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < n) out[i] = (unsigned short)(best[i] + 1);
  }
}

// ---- selection -----------------------------------------------------------------------------------------------------------
__global__ void select_init_kernel(u64 *__restrict__ best, int *__restrict__ cnt, int *__restrict__ bbox, int S) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  best[s] = 0;
  cnt[s] = 0;
  box_init(bbox + 4 * s);
}

// Round j over the raster.  FIRST (j == 0): no earlier points, and the bounding box rides along.
template <bool FIRST, bool VEC>
__global__ __launch_bounds__(256) void point_select_kernel(const int *__restrict__ labels, const unsigned short *__restrict__ clr, int H, int W,
                                                           int S, int k, int j, const int *__restrict__ pts, const int *__restrict__ cnt,
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
  const Strip g = strip_of(H, W);
  const int y = g.y, x0 = g.x0, n = g.n;
  const long long base = g.base;
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
        const u64 key = ((u64)(unsigned)score << 32) | (u64)(0xFFFFFFFFu - (unsigned)(base + i));
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

// The round's winners become points: position, clearance at the point; best is cleared for the next round.
__global__ void point_commit_kernel(u64 *__restrict__ best, const unsigned short *__restrict__ clr, int W, long long npix, int S, int k,
                                    int *__restrict__ pts, int *__restrict__ pclr, int *__restrict__ cnt) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const u64 b = best[s];
  if (!b) return;
  best[s] = 0;
  const long long lin = (long long)(0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFULL));
  const int m = cnt[s];
  if (lin >= npix || m >= k) return;
  pts[((long long)s * k + m) * 2] = (int)(lin % W);
  pts[((long long)s * k + m) * 2 + 1] = (int)(lin / W);
  pclr[(long long)s * k + m] = (int)clr[lin];
  cnt[s] = m + 1;
}

// ---- emit ------------------------------------------------------------------------------------------------------------------
// Exclusive scan of the counts by one looping workgroup (S is tens of thousands: a few tiles of 4096).
__global__ __launch_bounds__(SCAN_THREADS) void count_scan_kernel(const int *__restrict__ cnt, int S, int k, int *__restrict__ ptr) {
  __shared__ int lds[SCAN_THREADS / 64];
  int carry = 0;
  for (long long base = 0; base < S; base += SCAN_TILE) {
    int item[SCAN_ITEMS], sum = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
      const long long s = base + (long long)threadIdx.x * SCAN_ITEMS + i;
      item[i] = s < S ? min(max(cnt[s], 0), k) : 0;
      sum += item[i];
    }
    int total;
    int run = carry + block_exclusive(sum, lds, total);
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
      const long long s = base + (long long)threadIdx.x * SCAN_ITEMS + i;
      if (s < S) ptr[s] = run;
      run += item[i];
    }
    carry += total;
  }
  if (threadIdx.x == 0) ptr[S] = carry;
}

__global__ __launch_bounds__(256) void point_emit_kernel(const int *__restrict__ cnt, const int *__restrict__ pts, const int *__restrict__ pclr,
                                                         const int *__restrict__ bbox, const int *__restrict__ ptr, int S, int k,
                                                         int max_window, int capacity, int *__restrict__ xy, int *__restrict__ label,
                                                         int *__restrict__ inner, int *__restrict__ obj, int *__restrict__ round) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)S * k) return;
  const int s = (int)(t / k), q = (int)(t - (long long)s * k);
  if (q >= min(max(cnt[s], 0), k)) return;
  const long long row = (long long)ptr[s] + q;
  if (row < 0 || row >= capacity) return;
  const int in = 2 * pclr[(long long)s * k + q] - 1;
  const int side = max(bbox[4 * s + 2] - bbox[4 * s + 0], bbox[4 * s + 3] - bbox[4 * s + 1]) + 1;
  xy[2 * row] = pts[((long long)s * k + q) * 2];
  xy[2 * row + 1] = pts[((long long)s * k + q) * 2 + 1];
  label[row] = s;
  inner[row] = in;
  obj[row] = min(side, (max_window + 2 * in) / 3);
  round[row] = q;
}

}  // namespace

extern "C" int dm_label_clearance(const int32_t *labels, int32_t H, int32_t W, int32_t max_window, uint64_t *bits, uint8_t *row_dist,
                                  uint16_t *clearance, void *stream) {
  DM_REQUIRE(labels && bits && row_dist && clearance, DM_ERR_BAD_SHAPE, "dm_label_clearance: null pointer");
  DM_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1LL << 31), DM_ERR_BAD_SHAPE, "dm_label_clearance: bad sizes (H=%d W=%d; need H*W < 2^31)", H, W);
  DM_REQUIRE(max_window >= 1 && max_window <= 384, DM_ERR_BAD_SHAPE, "dm_label_clearance: max_window = %d outside 1..384", max_window);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int capm1 = (max_window + 1) / 2 - 1;
  const int WW = (W + 63) / 64;
  const int gb = (WW + ROW_THREADS / 64 - 1) / (ROW_THREADS / 64);       // == groups of 256 pixels per row
  hipLaunchKernelGGL(boundary_bits_kernel, dim3((unsigned)((long long)H * gb)), dim3(ROW_THREADS), 0, s, labels, H, W, WW, gb, (u64 *)bits);
  hipLaunchKernelGGL(row_distance_kernel, dim3((unsigned)((long long)H * gb)), dim3(ROW_THREADS), 0, s, (const u64 *)bits, H, W, WW, gb, capm1,
                     row_dist);
  const int gc = (W + 4 * ROW_THREADS - 1) / (4 * ROW_THREADS);
  if (W % 4 == 0 && dm_aligned(row_dist, 4) && dm_aligned(clearance, 8))
    hipLaunchKernelGGL(column_clearance_kernel<true>, dim3((unsigned)((long long)H * gc)), dim3(ROW_THREADS), 0, s, row_dist, H, W, gc, clearance);
  else
    hipLaunchKernelGGL(column_clearance_kernel<false>, dim3((unsigned)((long long)H * gc)), dim3(ROW_THREADS), 0, s, row_dist, H, W, gc, clearance);
  DM_LAUNCH_CHECK("dm_label_clearance");
  return DM_OK;
}

extern "C" int dm_point_select_round(const int32_t *labels, const uint16_t *clearance, int32_t H, int32_t W, int32_t S, int32_t k,
                                     int32_t round, uint64_t *best, int32_t *points, int32_t *point_clearance, int32_t *counts,
                                     int32_t *bbox, void *stream) {
  DM_REQUIRE(labels && clearance && best && points && point_clearance && counts && bbox, DM_ERR_BAD_SHAPE, "dm_point_select_round: null pointer");
  DM_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1LL << 31) && S > 0, DM_ERR_BAD_SHAPE,
             "dm_point_select_round: bad sizes (H=%d W=%d S=%d; need H*W < 2^31)", H, W, S);
  DM_REQUIRE(k >= 1 && k <= KMAX, DM_ERR_BAD_SHAPE, "dm_point_select_round: k = %d outside 1..16", k);
  DM_REQUIRE(round >= 0 && round < k, DM_ERR_BAD_SHAPE, "dm_point_select_round: round = %d outside 0..k-1 (k = %d)", round, k);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid = tile_grid(H, W);
  const bool vec = (W % STRIP == 0) && dm_aligned16(labels) && dm_aligned16(clearance);
  if (round == 0) {
    hipLaunchKernelGGL(select_init_kernel, dim3((S + 255) / 256), dim3(256), 0, s, (u64 *)best, counts, bbox, S);
    if (vec) hipLaunchKernelGGL((point_select_kernel<true, true>), grid, dim3(256), 0, s, labels, clearance, H, W, S, k, 0, points, counts, (u64 *)best, bbox);
    else hipLaunchKernelGGL((point_select_kernel<true, false>), grid, dim3(256), 0, s, labels, clearance, H, W, S, k, 0, points, counts, (u64 *)best, bbox);
  } else {
    if (vec) hipLaunchKernelGGL((point_select_kernel<false, true>), grid, dim3(256), 0, s, labels, clearance, H, W, S, k, round, points, counts, (u64 *)best, bbox);
    else hipLaunchKernelGGL((point_select_kernel<false, false>), grid, dim3(256), 0, s, labels, clearance, H, W, S, k, round, points, counts, (u64 *)best, bbox);
  }
  hipLaunchKernelGGL(point_commit_kernel, dim3((S + 255) / 256), dim3(256), 0, s, (u64 *)best, clearance, W, (long long)H * W, S, k, points,
                     point_clearance, counts);
  DM_LAUNCH_CHECK("dm_point_select_round");
  return DM_OK;
}

extern "C" int dm_point_emit(const int32_t *counts, const int32_t *points, const int32_t *point_clearance, const int32_t *bbox, int32_t S,
                             int32_t k, int32_t max_window, int32_t capacity, int32_t *ptr, int32_t *xy, int32_t *label, int32_t *inner,
                             int32_t *obj, int32_t *round, void *stream) {
  DM_REQUIRE(counts && points && point_clearance && bbox && ptr && xy && label && inner && obj && round, DM_ERR_BAD_SHAPE,
             "dm_point_emit: null pointer");
  DM_REQUIRE(S > 0 && capacity > 0 && (long long)S * k < (1LL << 31), DM_ERR_BAD_SHAPE, "dm_point_emit: bad sizes (S=%d capacity=%d)", S, capacity);
  DM_REQUIRE(k >= 1 && k <= KMAX, DM_ERR_BAD_SHAPE, "dm_point_emit: k = %d outside 1..16", k);
  DM_REQUIRE(max_window >= 1 && max_window <= 384, DM_ERR_BAD_SHAPE, "dm_point_emit: max_window = %d outside 1..384", max_window);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(count_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, counts, S, k, ptr);
  hipLaunchKernelGGL(point_emit_kernel, dim3((unsigned)(((long long)S * k + 255) / 256)), dim3(256), 0, s, counts, points, point_clearance, bbox,
                     ptr, S, k, max_window, capacity, xy, label, inner, obj, round);
  DM_LAUNCH_CHECK("dm_point_emit");
  return DM_OK;
}
