// Boundary recall / precision of a label raster against a ground-truth raster at a pixel tolerance (gfx950).  The region scores
// of dm_truth.hip say how well regions and objects overlap; these say where the partition's boundaries lie.  The rule is the
// build's own: it is stated in include/deepmerge_hip.h and restated in numpy in tests/boundary_ref.py.
//
// Every quantity is an integer and every reduction an integer add, so the result does not depend on the order in which threads
// arrive: the GPU and the numpy spec agree bit for bit.  No floating point anywhere in this file.
//
//   1. boundary_bits_kernel    one read of a raster: the canonical value of every pixel (the optional mapping applied here),
//                              edge bit = the right or the lower neighbour exists and differs, valid bit = the value is an id;
//                              a wave's ballot is one 64-bit word of the row (as in dm_points.hip, whose 8-neighbour, frame-
//                              included rule is another one and stays there).
//   2. boundary_count_kernel   per tolerance d, on bits only: a workgroup owns 64 rows x 4 words (256 pixels) of the box.  The
//                              label and the truth edge planes are dilated by d along the row (shift-and-OR doubling over the
//                              words w - 1, w, w + 1; d <= 64) into LDS with a halo of d rows, ORed over 2 d + 1 rows by doubling
//                              in LDS, and the four counts are popcounts of ANDs, reduced per wave and added with one 64-bit
//                              atomic per count and workgroup.
#include "dm_raster.h"

namespace {

constexpr int BITS_ROWS = 8;                                   // rows a wave walks down its word column: the row below is read once per 8
constexpr int CT_ROWS = 64, CT_WORDS = 4;                      // the count kernel's tile: 256 words, one per thread
constexpr int MAX_D = 64;                                      // DM_BOUNDARY_MAX_TOLERANCE: a dilation reaches the neighbouring word only
constexpr int CT_LDS_ROWS = CT_ROWS + 2 * MAX_D;

// Canonical value.  With a mapping: mapping[id] when the id lies in [0, n), -1 otherwise and for a negative entry.  Without: the id
// clamped to n as an unsigned number, so every id outside [0, n) is the one value n (one instruction; what counts is which
// values are equal and which stand for "none").
template <bool MAP>
__device__ __forceinline__ int canonical(int l, int n, const int *__restrict__ mapping) {
  if (!MAP) return (int)min((unsigned)l, (unsigned)n);
  return (unsigned)l < (unsigned)n ? max(mapping[l], -1) : -1;
}
template <bool MAP>
__device__ __forceinline__ bool is_id(int v, int n) { return MAP ? v >= 0 : v != n; }

// A workgroup covers 4 words (256 pixels) of BITS_ROWS consecutive rows: four waves, one word column each.
template <bool MAP>
__global__ __launch_bounds__(256) void boundary_bits_kernel(const int *__restrict__ raster, int H, int W, int WW, int groups, int n,
                                                            const int *__restrict__ mapping, u64 *__restrict__ edge,
                                                            u64 *__restrict__ valid) {
  const int yb = (blockIdx.x / groups) * BITS_ROWS, g = blockIdx.x % groups;
  const int w = g * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= WW) return;                                         // wave-uniform
  const int x = w * 64 + lane;
  const bool in = x < W;
  // Every load is inside the raster and none sits behind a branch (the pass is bound by instruction issue, not by HBM): a
  // column behind the last is the last, a row below the last is the last.  A neighbour that does not exist is then the pixel
  // itself, which differs from nothing: the frame rule needs no test of its own.
  // (The loads are a row's uniform address plus a byte offset below 2^11 inside the 256-pixel group: no 64-bit vector arithmetic.)
  const int gx = g * 256;
  const unsigned oc = 4u * (unsigned)(min(x, W - 1) - gx), on = 4u * (unsigned)(min(x + 1, W - 1) - gx);
  int v[BITS_ROWS + 1], right[BITS_ROWS];                      // own column, rows yb .. yb + 8; the right neighbours, rows yb .. yb + 7
#pragma unroll
  for (int r = 0; r <= BITS_ROWS; ++r) {
    const char *row = reinterpret_cast<const char *>(raster + (long long)min(yb + r, H - 1) * W + gx);
    v[r] = *reinterpret_cast<const int *>(row + oc);
    if (r < BITS_ROWS) right[r] = *reinterpret_cast<const int *>(row + on);
  }
#pragma unroll
  for (int r = 0; r <= BITS_ROWS; ++r) {
    v[r] = canonical<MAP>(v[r], n, mapping);
    if (r < BITS_ROWS) right[r] = canonical<MAP>(right[r], n, mapping);
  }
  u64 e_word = 0, ok_word = 0;                                 // lane r < 8: the words of row yb + r, stored by one instruction
#pragma unroll
  for (int r = 0; r < BITS_ROWS; ++r) {
    const u64 e = __ballot(in && (right[r] != v[r] || v[r + 1] != v[r]));
    const u64 ok = __ballot(in && is_id<MAP>(v[r], n));
    if (lane == r) { e_word = e; ok_word = ok; }
  }
  if (lane < BITS_ROWS && yb + lane < H) {
    const long long at = (long long)(yb + lane) * WW + w;
    edge[at] = e_word;
    if (valid) valid[at] = ok_word;
  }
}

// ---- dilation along the row ----------------------------------------------------------------------------------------------------
// A 128-bit value (lo = the word of lower x) shifted by 1 <= s <= 63 towards higher / lower x.
struct U128 { u64 lo, hi; };
__device__ __forceinline__ U128 shl(U128 a, int s) { return U128{a.lo << s, (a.hi << s) | (a.lo >> (64 - s))}; }
__device__ __forceinline__ U128 shr(U128 a, int s) { return U128{(a.lo >> s) | (a.hi << (64 - s)), a.hi >> s}; }

// OR of the shifts 0 .. d of `a` (UP: towards higher x) by doubling: S_2c = S_c | shift(S_c, c), then one shift by d + 1 - c.
// d <= 64: no single shift is longer than 32.
template <bool UP>
__device__ __forceinline__ U128 smear(U128 a, int d) {
  const int n = d + 1;
  int c = 1;
  while (2 * c <= n) {
    const U128 t = UP ? shl(a, c) : shr(a, c);
    a.lo |= t.lo; a.hi |= t.hi;
    c *= 2;
  }
  if (c < n) {
    const U128 t = UP ? shl(a, n - c) : shr(a, n - c);
    a.lo |= t.lo; a.hi |= t.hi;
  }
  return a;
}

// Word w of row `row` dilated by d along the row: every bit within d pixels of a set bit of the words w - 1, w, w + 1.
__device__ __forceinline__ u64 row_dilated(const u64 *__restrict__ row, int w, int WW, int d) {
  const u64 cur = row[w];
  const u64 prev = w > 0 ? row[w - 1] : 0, next = w + 1 < WW ? row[w + 1] : 0;
  if (d == 0) return cur;
  return smear<true>(U128{prev, cur}, d).hi | smear<false>(U128{cur, next}, d).lo;
}

// Bits x0 <= x < x1 of word w.
__device__ __forceinline__ u64 word_mask(int w, int x0, int x1) {
  const int lo = max(x0 - w * 64, 0), hi = min(x1 - w * 64, 64);
  if (hi <= lo) return 0;
  return (~0ULL << lo) & (~0ULL >> (64 - hi));
}

// Tile (ty, tx) of the box: rows y0 + 64 ty .., words (x0 >> 6) + 4 tx ..; counts[4] += n_truth_b, hit_truth, n_label_b, hit_label.
__global__ __launch_bounds__(256) void boundary_count_kernel(const u64 *__restrict__ label_edge, const u64 *__restrict__ truth_edge,
                                                             const u64 *__restrict__ truth_valid, int H, int WW, int d, int y0, int y1,
                                                             int x0, int x1, int tiles_x, long long *__restrict__ counts) {
  __shared__ u64 m_label[CT_LDS_ROWS * CT_WORDS], m_truth[CT_LDS_ROWS * CT_WORDS];
  __shared__ int part[4][4];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int row0 = y0 + ty * CT_ROWS, w0 = (x0 >> 6) + tx * CT_WORDS;
  const int rows = CT_ROWS + 2 * d;                            // LDS row r is raster row row0 - d + r
  const int items = rows * CT_WORDS;
  for (int e = threadIdx.x; e < items; e += 256) {
    const int y = row0 - d + (e >> 2), w = w0 + (e & 3);
    u64 a = 0, b = 0;
    if (y >= 0 && y < H && w < WW) {
      a = row_dilated(label_edge + (long long)y * WW, w, WW, d);
      b = row_dilated(truth_edge + (long long)y * WW, w, WW, d);
    }
    m_label[e] = a;
    m_truth[e] = b;
  }
  __syncthreads();
  // OR over the rows r .. r + 2^k - 1 by doubling, 2^k the largest power of two <= 2 d + 1; rows whose partner lies behind the
  // tile's last row keep what they have: no window of the 64 output rows reads them.
  const int L = 2 * d + 1;
  int span = 1;
  while (2 * span <= L) {
    u64 a[3], b[3];                                            // items <= 192 * 4 = 3 * 256
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int e = threadIdx.x + 256 * i, p = e + span * CT_WORDS;
      const bool on = e < items && p < items;
      a[i] = on ? m_label[p] : 0;
      b[i] = on ? m_truth[p] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int e = threadIdx.x + 256 * i;
      if (e < items) { m_label[e] |= a[i]; m_truth[e] |= b[i]; }
    }
    __syncthreads();
    span *= 2;
  }
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  {
    const int r = threadIdx.x >> 2, y = row0 + r, w = w0 + (threadIdx.x & 3);
    const u64 mask = (y < y1 && w < WW) ? word_mask(w, x0, x1) : 0;
    if (mask) {
      // rows y - d .. y + d are LDS rows r .. r + 2 d: two spans of 2^k rows cover them
      const int e = r * CT_WORDS + (threadIdx.x & 3), f = e + (L - span) * CT_WORDS;
      const u64 ml = m_label[e] | m_label[f], mt = m_truth[e] | m_truth[f];
      const long long at = (long long)y * WW + w;
      const u64 bl = label_edge[at] & mask, bt = truth_edge[at] & mask, vt = truth_valid[at];
      c0 = __popcll(bt);
      c1 = __popcll(bt & ml);
      c2 = __popcll(bl & (vt | mt));
      c3 = __popcll(bl & mt);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c0 += __shfl_xor(c0, o, 64); c1 += __shfl_xor(c1, o, 64); c2 += __shfl_xor(c2, o, 64); c3 += __shfl_xor(c3, o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { part[wave][0] = c0; part[wave][1] = c1; part[wave][2] = c2; part[wave][3] = c3; }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (sum) atomic_add64(counts + threadIdx.x, sum);
  }
}

}  // namespace

extern "C" int dm_boundary_bits(const int32_t *raster, int32_t H, int32_t W, int32_t n_ids, const int32_t *mapping, uint64_t *edge,
                                uint64_t *valid, void *stream) {
  DM_REQUIRE(raster && edge, DM_ERR_BAD_SHAPE, "dm_boundary_bits: null pointer");
  DM_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1LL << 31) && n_ids > 0, DM_ERR_BAD_SHAPE,
             "dm_boundary_bits: bad sizes (H=%d W=%d n_ids=%d; need H*W < 2^31)", H, W, n_ids);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int WW = (W + 63) / 64, groups = (WW + 3) / 4;
  const dim3 grid((unsigned)((long long)groups * ((H + BITS_ROWS - 1) / BITS_ROWS)));
  if (mapping)
    hipLaunchKernelGGL(boundary_bits_kernel<true>, grid, dim3(256), 0, s, raster, H, W, WW, groups, n_ids, mapping, (u64 *)edge, (u64 *)valid);
  else
    hipLaunchKernelGGL(boundary_bits_kernel<false>, grid, dim3(256), 0, s, raster, H, W, WW, groups, n_ids, mapping, (u64 *)edge, (u64 *)valid);
  DM_LAUNCH_CHECK("dm_boundary_bits");
  return DM_OK;
}

extern "C" int dm_boundary_counts(const uint64_t *label_edge, const uint64_t *truth_edge, const uint64_t *truth_valid, int32_t H, int32_t W,
                                  int32_t d, int32_t y0, int32_t y1, int32_t x0, int32_t x1, int64_t *counts, void *stream) {
  DM_REQUIRE(label_edge && truth_edge && truth_valid && counts, DM_ERR_BAD_SHAPE, "dm_boundary_counts: null pointer");
  DM_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1LL << 31), DM_ERR_BAD_SHAPE, "dm_boundary_counts: bad sizes (H=%d W=%d; need H*W < 2^31)", H, W);
  DM_REQUIRE(d >= 0 && d <= MAX_D, DM_ERR_BAD_SHAPE, "dm_boundary_counts: tolerance = %d outside 0..64", d);
  DM_REQUIRE(0 <= y0 && y0 < y1 && y1 <= H && 0 <= x0 && x0 < x1 && x1 <= W, DM_ERR_BAD_SHAPE,
             "dm_boundary_counts: bad box (rows %d..%d, columns %d..%d of %d x %d)", y0, y1, x0, x1, H, W);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int WW = (W + 63) / 64;
  const int tiles_x = (((x1 - 1) >> 6) - (x0 >> 6) + CT_WORDS) / CT_WORDS, tiles_y = (y1 - y0 + CT_ROWS - 1) / CT_ROWS;
  hipLaunchKernelGGL(boundary_count_kernel, dim3((unsigned)((long long)tiles_x * tiles_y)), dim3(256), 0, s, (const u64 *)label_edge,
                     (const u64 *)truth_edge, (const u64 *)truth_valid, H, WW, d, y0, y1, x0, x1, tiles_x, (long long *)counts);
  DM_LAUNCH_CHECK("dm_boundary_counts");
  return DM_OK;
}
