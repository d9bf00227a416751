// Per-epoch pair draw (gfx950): the epoch's whole training sample table in ONE launch, already in the per-step blocked layout
// feed.PairFeed consumes -- the device counterpart of the dataset rebuild the reference runs on the host every epoch
// (MyUtils1.py:275-293: one uniform sample point per polygon of every pair, Python `random`) followed by
// DataLoader(shuffle=True) (Train_SMT.py:218-220: a fresh permutation per epoch, torch's global RNG).
// Here both are counter-based and keyed by (seed, epoch), so epoch e draws the same table whether or not the run was
// interrupted (DESIGN.md 3.9 is the contract; tests/train_smt_ref.py restates it in numpy, bit for bit):
//   philox(ctr, key)  Philox4x32-10 (Salmon et al. 2011), key = (seed & 0xffffffff, seed >> 32)
//   shuffle           position j takes pair src = perm(j): a 4-round balanced Feistel network on [0, 2^b) (b = ceil(log2 N)
//                     rounded up to even, >= 2; round r: L, R = R, L ^ (philox((R, epoch, 2, r))[0] & (2^h - 1)), h = b / 2),
//                     cycle-walked until the value is < N
//   draw              r = philox((src, epoch, 1, 0)): left point = poly_pts[poly_off[pl] + umulhi(r[0], cnt_l)], right point
//                     likewise with r[1] -- keyed by the pair, so shuffle and draw are independent
//   orient            dm_pair_epoch_orient: philox((src, epoch, 3, 0))[0] & mask (7: the dihedral group D4, 3: flips only), the
//                     augmentation of dm_pair_batch_gather_oriented, written to both rows of the pair
//   radiometric       dm_pair_epoch_radiometric: counter word 4 -- a gain and an offset per pair, a gain deviation per band (the table of
//                     dm_pair_batch_gather_augmented), written to both rows of the pair
// Weighted sampling with replacement (the `_src` entry points; DESIGN.md 3.9, tests/sampling_ref.py):
//   select            dm_pair_epoch_select: position j of M draws u = umul64hi(R, T), R = r[0] << 32 | r[1], r = philox((j, epoch, 5, 0)),
//                     T = cum[N - 1] the total of the int64 weights, and takes src[j] = the smallest i with cum[i] > u (a binary search
//                     over the inclusive prefix sums; a pair of weight 0 is never taken)
//   streams           a pair can be drawn twice in one epoch, so the sampled epoch keys the three streams by the POSITION j and moves
//                     them to counter words 17, 19 and 20 (the unsampled word + 16): same arithmetic, same layout with M in place of N
// Every kernel below is written once and instantiated per key rule (PairKeyed: today's permuted epoch; PositionKeyed: the sampled one).
// One thread per position: integer VALU work plus a gather of the two 80-byte point rows.  A pair whose polygon id, point list or
// point id is out of range (the host validates them once, at dataset construction) reads nothing out of range: its sample gets
// point_id -1, tile id -1 (which the feed's gather flags) and zeros.
#include "dm_common.h"

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r > 0) { k0 += PHILOX_W0; k1 += PHILOX_W1; }
    const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
  }
  u32x4 out;
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
  return out;
}

// perm(j) for j < n: the Feistel bijection of [0, 2^(2h)), cycle-walked back into [0, n)
__device__ __forceinline__ uint32_t epoch_perm(uint32_t j, uint32_t n, int h, uint32_t epoch, uint32_t k0, uint32_t k1) {
  const uint32_t mask = (1u << h) - 1u;
  uint32_t x = j;
  do {
    uint32_t L = x >> h, R = x & mask;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t f = philox4x32_10(R, epoch, 2u, r, k0, k1)[0] & mask;
      const uint32_t t = L ^ f;
      L = R;
      R = t;
    }
    x = (L << h) | R;
  } while (x >= n);
  return x;
}

// Where a position's pair and the key of its streams come from.  key(): counter word 0 of the draw, orientation and radiometric
// streams; WORD: added to their counter word 2.
struct PairKeyed {                                      // the epoch as a permutation: position j takes pair perm(j), streams keyed by the pair
  int h;
  static constexpr uint32_t WORD = 0u;
  __device__ __forceinline__ uint32_t key(uint32_t j, uint32_t n, uint32_t epoch, uint32_t k0, uint32_t k1) const {
    return epoch_perm(j, n, h, epoch, k0, k1);
  }
};
struct PositionKeyed {                                  // the sampled epoch: the pair comes from a column, streams keyed by the position
  static constexpr uint32_t WORD = 16u;
  __device__ __forceinline__ uint32_t key(uint32_t j, uint32_t, uint32_t, uint32_t, uint32_t) const { return j; }
};
// The draw also needs the pair itself and the number of positions; pair() is -1 for a column entry outside [0, n_pairs).
struct PermPairs : PairKeyed {
  __device__ __forceinline__ int32_t draws(int32_t n_pairs) const { return n_pairs; }
  __device__ __forceinline__ int64_t pair(int64_t, uint32_t key, int32_t) const { return key; }
};
struct ColumnPairs : PositionKeyed {
  const int32_t *src;
  int32_t n_draws;
  __device__ __forceinline__ int32_t draws(int32_t) const { return n_draws; }
  __device__ __forceinline__ int64_t pair(int64_t j, uint32_t, int32_t n_pairs) const {
    const int32_t s = src[j];
    return (s >= 0 && s < n_pairs) ? s : -1;
  }
};

// step s owns rows [2 s batch, 2 s batch + 2 b_s) as [left b_s; right b_s]: position j of n -> its left row and b_s (right row = left + b_s)
struct PairRows {
  int64_t left, b_s;
};
__device__ __forceinline__ PairRows pair_rows(int64_t j, int64_t n, int64_t batch) {
  const int64_t s = j / batch;
  return {s * batch + j, min(batch, n - s * batch)};   // 2 s batch + (j - s batch)
}

// the global point id of the sample drawn from polygon p with random word u; -1 when p or its point list is out of range
__device__ __forceinline__ int32_t draw_point(const DmPairDraw &a, int32_t p, uint32_t u) {
  if (p < 0 || p >= a.n_poly) return -1;
  const int32_t lo = a.poly_off[p], hi = a.poly_off[p + 1];
  if (lo < 0 || hi <= lo || hi > a.n_poly_pts) return -1;
  const int32_t pt = a.poly_pts[lo + (int32_t)__umulhi(u, (uint32_t)(hi - lo))];
  return (pt >= 0 && pt < a.n_pts) ? pt : -1;
}

__device__ __forceinline__ void write_sample(const DmPairDraw &a, int64_t row, int32_t pt) {
  const bool ok = pt >= 0;
  a.tile_id[row] = ok ? a.pt_tile[pt] : -1;
  a.xy[2 * row] = ok ? a.pt_xy[2 * (int64_t)pt] : 0;
  a.xy[2 * row + 1] = ok ? a.pt_xy[2 * (int64_t)pt + 1] : 0;
  a.inner[row] = ok ? a.pt_inner[pt] : 0;
  a.obj[row] = ok ? a.pt_obj[pt] : 0;
  const float *src = a.pt_region + 15 * (int64_t)(ok ? pt : 0);
  float *dst = a.region + 15 * row;
#pragma unroll
  for (int c = 0; c < 15; ++c) dst[c] = ok ? src[c] : 0.0f;
  if (a.point_id) a.point_id[row] = pt;
}

template <typename Pairs>
__global__ __launch_bounds__(256) void pair_epoch_draw_kernel(DmPairDraw a, Pairs from) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int32_t n = from.draws(a.n_pairs);
  if (j >= n) return;
  const uint32_t k0 = (uint32_t)(a.seed & 0xffffffffull), k1 = (uint32_t)(a.seed >> 32);
  const uint32_t epoch = (uint32_t)a.epoch;
  const uint32_t key = from.key((uint32_t)j, (uint32_t)a.n_pairs, epoch, k0, k1);
  const int64_t src = from.pair(j, key, a.n_pairs);
  const u32x4 r = philox4x32_10(key, epoch, 1u + Pairs::WORD, 0u, k0, k1);
  const bool listed = src >= 0;
  const int32_t pl = listed ? a.pairs[2 * src] : -1, pr = listed ? a.pairs[2 * src + 1] : -1;
  const PairRows rows = pair_rows(j, n, a.batch);
  write_sample(a, rows.left, draw_point(a, pl, r[0]));
  write_sample(a, rows.left + rows.b_s, draw_point(a, pr, r[1]));
  a.flag[j] = listed ? (float)a.pair_flag[src] : 0.0f;
}

// the dihedral orientation of every pair of the epoch: counter word 3, a stream neither the draw (1) nor the shuffle (2) uses;
// keyed like the draw, and written to both of the pair's rows
template <typename Key>
__global__ __launch_bounds__(256) void pair_epoch_orient_kernel(uint64_t seed, int32_t epoch_, int32_t n_pairs, int32_t batch, uint32_t mask,
                                                                int32_t *__restrict__ orient, Key from) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_pairs) return;
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
  const uint32_t epoch = (uint32_t)epoch_;
  const uint32_t key = from.key((uint32_t)j, (uint32_t)n_pairs, epoch, k0, k1);
  const int32_t o = (int32_t)(philox4x32_10(key, epoch, 3u + Key::WORD, 0u, k0, k1)[0] & mask);
  const PairRows rows = pair_rows(j, n_pairs, batch);
  orient[rows.left] = o;
  orient[rows.left + rows.b_s] = o;
}

// uniform on -s .. s from one random word (0 when s = 0)
__device__ __forceinline__ int32_t sym_draw(uint32_t r, int32_t s) { return (int32_t)__umulhi(r, 2u * (uint32_t)s + 1u) - s; }

// the radiometric table of every pair of the epoch: counter word 4, keyed like the orientation.  A common gain and offset
// from block 0, one gain deviation per band from blocks 1 + c / 4, the offset pivoting the contrast about mid-grey (128); written to both
// of the pair's rows as [row][band][gain, offset]
template <typename Key>
__global__ __launch_bounds__(256) void pair_epoch_radiometric_kernel(uint64_t seed, int32_t epoch_, int32_t n_pairs, int32_t batch, int32_t bands,
                                                                     int32_t gain_span, int32_t band_span, int32_t offset_span,
                                                                     int32_t *__restrict__ radio, Key from) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_pairs) return;
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
  const uint32_t epoch = (uint32_t)epoch_;
  const uint32_t key = from.key((uint32_t)j, (uint32_t)n_pairs, epoch, k0, k1);
  const u32x4 A = philox4x32_10(key, epoch, 4u + Key::WORD, 0u, k0, k1);
  const int32_t g0 = 256 + sym_draw(A[0], gain_span), b0 = sym_draw(A[1], offset_span);
  const PairRows rows = pair_rows(j, n_pairs, batch);
  int32_t *left = radio + rows.left * bands * 2, *right = radio + (rows.left + rows.b_s) * bands * 2;
  for (int c0 = 0; c0 < bands; c0 += 4) {
    const u32x4 B = philox4x32_10(key, epoch, 4u + Key::WORD, 1u + (uint32_t)(c0 >> 2), k0, k1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + k;
      if (c >= bands) break;
      const int32_t gain = g0 + sym_draw(B[k], band_span), offset = b0 - 128 * (gain - 256);
      left[2 * c] = gain; left[2 * c + 1] = offset;
      right[2 * c] = gain; right[2 * c + 1] = offset;
    }
  }
}

// the weighted select: counter word 5.  u is uniform on [0, T), T = cum[n - 1]; src = the number of prefix sums <= u, found by a
// binary search whose index never leaves [0, n) whatever `cum` holds.  Valid weights (non-negative, T >= 1) give src < n; a table
// that is not one gives at most n, which the draw treats as out of range.  No LDS stage: the table's top levels are shared by
// every thread and stay in L2, and the launch runs once per epoch.
__global__ __launch_bounds__(256) void pair_epoch_select_kernel(const int64_t *__restrict__ cum, int32_t n_pairs, int32_t n_draws, uint64_t seed,
                                                                int32_t epoch_, int32_t *__restrict__ src) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_draws) return;
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
  const u32x4 r = philox4x32_10((uint32_t)j, (uint32_t)epoch_, 5u, 0u, k0, k1);
  const uint64_t R = ((uint64_t)r[0] << 32) | (uint64_t)r[1];
  const uint64_t u = __umul64hi(R, (uint64_t)cum[n_pairs - 1]);
  int32_t lo = 0, hi = n_pairs;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if ((uint64_t)cum[mid] <= u) lo = mid + 1; else hi = mid;
  }
  src[j] = lo;
}

// ceil(log2 N), rounded up to even, >= 2: the width of the shuffle's Feistel network
int feistel_bits(int32_t n_pairs) {
  int b = 2;
  while ((1ll << b) < (long long)n_pairs) b += 2;
  return b;
}

constexpr int THREADS = 256;
int blocks_for(int32_t n) { return (int)((n + THREADS - 1) / THREADS); }

// what every entry point of a family refuses before its launch, stated once (`what` names the caller in the message)
int check_counts(const char *what, int32_t n, int32_t batch, int32_t epoch) {
  DM_REQUIRE(n >= 1 && n <= (1 << 30), DM_ERR_BAD_SHAPE, "%s: %d pairs (1 .. 2^30)", what, n);
  DM_REQUIRE(batch >= 1, DM_ERR_BAD_SHAPE, "%s: batch %d < 1", what, batch);
  DM_REQUIRE(epoch >= 0, DM_ERR_BAD_SHAPE, "%s: epoch %d < 0", what, epoch);
  return DM_OK;
}

int check_draw(const char *what, const DmPairDraw *args) {
  DM_REQUIRE(args != nullptr, DM_ERR_BAD_SHAPE, "%s: null arguments", what);
  const DmPairDraw &a = *args;
  if (int rc = check_counts(what, a.n_pairs, a.batch, a.epoch)) return rc;
  DM_REQUIRE(a.n_poly >= 1 && a.n_poly_pts >= 1 && a.n_pts >= 1, DM_ERR_BAD_SHAPE,
             "%s: empty polygon table (%d polygons, %d polygon points, %d points)", what, a.n_poly, a.n_poly_pts, a.n_pts);
  DM_REQUIRE(a.pairs && a.pair_flag && a.poly_off && a.poly_pts && a.pt_tile && a.pt_xy && a.pt_inner && a.pt_obj && a.pt_region,
             DM_ERR_BAD_SHAPE, "%s: bad arguments (null input)", what);
  DM_REQUIRE(a.tile_id && a.xy && a.inner && a.obj && a.region && a.flag, DM_ERR_BAD_SHAPE, "%s: bad arguments (null output)", what);
  return DM_OK;
}

int check_orient(const char *what, int32_t epoch, int32_t n, int32_t batch, int32_t mask, const int32_t *orient) {
  DM_REQUIRE(mask == 3 || mask == 7, DM_ERR_BAD_SHAPE, "%s: mask %d (3: flips, 7: d4)", what, mask);
  if (int rc = check_counts(what, n, batch, epoch)) return rc;
  DM_REQUIRE(orient != nullptr, DM_ERR_BAD_SHAPE, "%s: bad arguments (null output)", what);
  return DM_OK;
}

int check_radiometric(const char *what, int32_t epoch, int32_t n, int32_t batch, int32_t bands, int32_t gain_span, int32_t band_span,
                      int32_t offset_span, const int32_t *radio) {
  DM_REQUIRE(gain_span >= 0 && gain_span <= DM_RADIO_MAX_GAIN_SPAN, DM_ERR_BAD_SHAPE, "%s: gain span %d outside 0..%d", what, gain_span,
             DM_RADIO_MAX_GAIN_SPAN);
  DM_REQUIRE(band_span >= 0 && band_span <= DM_RADIO_MAX_BAND_SPAN, DM_ERR_BAD_SHAPE, "%s: band span %d outside 0..%d", what, band_span,
             DM_RADIO_MAX_BAND_SPAN);
  DM_REQUIRE(offset_span >= 0 && offset_span <= DM_RADIO_MAX_OFFSET_SPAN, DM_ERR_BAD_SHAPE, "%s: offset span %d outside 0..%d", what, offset_span,
             DM_RADIO_MAX_OFFSET_SPAN);
  DM_REQUIRE(bands >= 1 && bands <= 16, DM_ERR_BAD_SHAPE, "%s: %d bands (1 .. 16)", what, bands);
  if (int rc = check_counts(what, n, batch, epoch)) return rc;
  DM_REQUIRE(radio != nullptr, DM_ERR_BAD_SHAPE, "%s: bad arguments (null output)", what);
  return DM_OK;
}

}  // namespace

extern "C" int dm_pair_epoch_orient(uint64_t seed, int32_t epoch, int32_t n_pairs, int32_t batch, int32_t mask, int32_t *orient, void *stream) {
  if (int rc = check_orient("dm_pair_epoch_orient", epoch, n_pairs, batch, mask, orient)) return rc;
  hipLaunchKernelGGL(pair_epoch_orient_kernel<PairKeyed>, dim3(blocks_for(n_pairs)), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), seed,
                     epoch, n_pairs, batch, (uint32_t)mask, orient, PairKeyed{feistel_bits(n_pairs) / 2});
  DM_LAUNCH_CHECK("dm_pair_epoch_orient");
  return DM_OK;
}

extern "C" int dm_pair_epoch_orient_src(uint64_t seed, int32_t epoch, int32_t n_draws, int32_t batch, int32_t mask, int32_t *orient,
                                        void *stream) {
  if (int rc = check_orient("dm_pair_epoch_orient_src", epoch, n_draws, batch, mask, orient)) return rc;
  hipLaunchKernelGGL(pair_epoch_orient_kernel<PositionKeyed>, dim3(blocks_for(n_draws)), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     seed, epoch, n_draws, batch, (uint32_t)mask, orient, PositionKeyed{});
  DM_LAUNCH_CHECK("dm_pair_epoch_orient_src");
  return DM_OK;
}

extern "C" int dm_pair_epoch_radiometric(uint64_t seed, int32_t epoch, int32_t n_pairs, int32_t batch, int32_t bands, int32_t gain_span,
                                         int32_t band_span, int32_t offset_span, int32_t *radio, void *stream) {
  if (int rc = check_radiometric("dm_pair_epoch_radiometric", epoch, n_pairs, batch, bands, gain_span, band_span, offset_span, radio)) return rc;
  hipLaunchKernelGGL(pair_epoch_radiometric_kernel<PairKeyed>, dim3(blocks_for(n_pairs)), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     seed, epoch, n_pairs, batch, bands, gain_span, band_span, offset_span, radio, PairKeyed{feistel_bits(n_pairs) / 2});
  DM_LAUNCH_CHECK("dm_pair_epoch_radiometric");
  return DM_OK;
}

extern "C" int dm_pair_epoch_radiometric_src(uint64_t seed, int32_t epoch, int32_t n_draws, int32_t batch, int32_t bands, int32_t gain_span,
                                             int32_t band_span, int32_t offset_span, int32_t *radio, void *stream) {
  if (int rc = check_radiometric("dm_pair_epoch_radiometric_src", epoch, n_draws, batch, bands, gain_span, band_span, offset_span, radio)) return rc;
  hipLaunchKernelGGL(pair_epoch_radiometric_kernel<PositionKeyed>, dim3(blocks_for(n_draws)), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), seed, epoch, n_draws, batch, bands, gain_span, band_span, offset_span, radio,
                     PositionKeyed{});
  DM_LAUNCH_CHECK("dm_pair_epoch_radiometric_src");
  return DM_OK;
}

extern "C" int dm_pair_epoch_draw(const DmPairDraw *args, void *stream) {
  if (int rc = check_draw("dm_pair_epoch_draw", args)) return rc;
  PermPairs from;
  from.h = feistel_bits(args->n_pairs) / 2;
  hipLaunchKernelGGL(pair_epoch_draw_kernel<PermPairs>, dim3(blocks_for(args->n_pairs)), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     *args, from);
  DM_LAUNCH_CHECK("dm_pair_epoch_draw");
  return DM_OK;
}

extern "C" int dm_pair_epoch_draw_src(const DmPairDraw *args, const int32_t *src, int32_t n_draws, void *stream) {
  if (int rc = check_draw("dm_pair_epoch_draw_src", args)) return rc;
  DM_REQUIRE(src != nullptr, DM_ERR_BAD_SHAPE, "dm_pair_epoch_draw_src: bad arguments (null src)");
  DM_REQUIRE(n_draws >= 1 && n_draws <= (1 << 30), DM_ERR_BAD_SHAPE, "dm_pair_epoch_draw_src: %d draws (1 .. 2^30)", n_draws);
  ColumnPairs from;
  from.src = src;
  from.n_draws = n_draws;
  hipLaunchKernelGGL(pair_epoch_draw_kernel<ColumnPairs>, dim3(blocks_for(n_draws)), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), *args,
                     from);
  DM_LAUNCH_CHECK("dm_pair_epoch_draw_src");
  return DM_OK;
}

extern "C" int dm_pair_epoch_select(const int64_t *cum, int32_t n_pairs, int32_t n_draws, uint64_t seed, int32_t epoch, int32_t *src,
                                    void *stream) {
  DM_REQUIRE(cum != nullptr && src != nullptr, DM_ERR_BAD_SHAPE, "dm_pair_epoch_select: bad arguments (null pointer)");
  DM_REQUIRE(n_pairs >= 1 && n_pairs <= (1 << 30), DM_ERR_BAD_SHAPE, "dm_pair_epoch_select: %d pairs (1 .. 2^30)", n_pairs);
  DM_REQUIRE(n_draws >= 1 && n_draws <= (1 << 30), DM_ERR_BAD_SHAPE, "dm_pair_epoch_select: %d draws (1 .. 2^30)", n_draws);
  DM_REQUIRE(epoch >= 0, DM_ERR_BAD_SHAPE, "dm_pair_epoch_select: epoch %d < 0", epoch);
  hipLaunchKernelGGL(pair_epoch_select_kernel, dim3(blocks_for(n_draws)), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), cum, n_pairs,
                     n_draws, seed, epoch, src);
  DM_LAUNCH_CHECK("dm_pair_epoch_select");
  return DM_OK;
}
