// Multiresolution region merging (gfx950): the two pieces `rag.mrs` adds to the mutual-best merge of dm_merge.hip (DESIGN.md 3.5.8;
// the rule is stated in include/deepmerge_hip.h and restated in numpy in tests/mrs_ref.py).
//   dm_region_merge_cost  the score of a round: the Baatz-Schaepe colour / shape heterogeneity increase of every RAG edge, from
//                         the regions' exact integer statistics.  It takes the place of dm_segment_mean + dm_edge_similarity; the
//                         rest of the round (best, match, the two folds) is dm_merge.hip's, unchanged.
//   dm_pixel_regions      the start state in which every pixel is its own region, in closed form: no pass through the hash table
//                         that dm_rag_edges needs for arbitrary labels.
// The cost is a fixed sequence of IEEE double operations (+, -, *, /, sqrt; this file is built with -ffp-contract=off) on exact
// integers, one thread per edge, no reduction: the GPU and the spec agree bit for bit, as label_features_kernel (dm_rag.hip) does.
#include <cfloat>

#include "dm_raster.h"

namespace {

typedef unsigned __int128 u128;

struct MrsParams { double bw[3], shape, compactness; };

// (n sigma)^2 = n * sumsq - sum^2 as a double.  The integer needs up to 78 bits (n <= 2^31, pixel values <= 255); split at bit
// 32 both halves convert exactly (hi < 2^46) and hi * 2^32 is exact, so only the add rounds: ONE rounding to nearest-even.
__device__ __forceinline__ double nvar(long long n, long long s1, long long s2) {
  const u128 v = (u128)(u64)n * (u128)(u64)s2 - (u128)(u64)s1 * (u128)(u64)s1;
  const u64 hi = (u64)(v >> 32), lo = (u64)v & 0xffffffffULL;
  return (double)hi * 4294967296.0 + (double)lo;
}

__device__ __forceinline__ long long box_len(int x0, int y0, int x1, int y1) {
  return 2LL * (((long long)x1 - x0 + 1) + ((long long)y1 - y0 + 1));
}

__global__ __launch_bounds__(256) void merge_cost_kernel(const long long *__restrict__ count, const long long *__restrict__ sum,
                                                         const long long *__restrict__ sumsq, const int *__restrict__ bbox,
                                                         const long long *__restrict__ peri, const int *__restrict__ edges,
                                                         const int *__restrict__ weights, int E, int C, int nb, MrsParams p,
                                                         float *__restrict__ cost) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (long long)gridDim.x * blockDim.x) {
    const int a = edges[2 * e], b = edges[2 * e + 1];
    float out = __int_as_float(0x7fc00000);                     // NaN: never a candidate (dm_merge_best)
    if ((unsigned)a < (unsigned)C && (unsigned)b < (unsigned)C) {
      const long long na = count[a], nbb = count[b];
      if (na > 0 && nbb > 0) {
        const long long la = peri[2 * (long long)a] + peri[2 * (long long)a + 1], lb = peri[2 * (long long)b] + peri[2 * (long long)b + 1];
        const long long nm = na + nbb, lm = la + lb - 2LL * weights[e];
        const int *ba = bbox + 4 * (long long)a, *bb = bbox + 4 * (long long)b;
        const long long qa = box_len(ba[0], ba[1], ba[2], ba[3]), qb = box_len(bb[0], bb[1], bb[2], bb[3]);
        const long long qm = box_len(min(ba[0], bb[0]), min(ba[1], bb[1]), max(ba[2], bb[2]), max(ba[3], bb[3]));
        double hc = 0.0;
        for (int c = 0; c < nb; ++c) {
          const long long s1a = sum[(long long)a * nb + c], s1b = sum[(long long)b * nb + c];
          const long long s2a = sumsq[(long long)a * nb + c], s2b = sumsq[(long long)b * nb + c];
          const double vm = nvar(nm, s1a + s1b, s2a + s2b), va = nvar(na, s1a, s2a), vb = nvar(nbb, s1b, s2b);
          hc = hc + p.bw[c] * ((sqrt(vm) - sqrt(va)) - sqrt(vb));
        }
        const double dna = (double)na, dnb = (double)nbb, dnm = (double)nm, dla = (double)la, dlb = (double)lb, dlm = (double)lm;
        const double hcm = (dlm * sqrt(dnm) - dla * sqrt(dna)) - dlb * sqrt(dnb);
        const double hsm = ((dnm * dlm) / (double)qm - (dna * dla) / (double)qa) - (dnb * dlb) / (double)qb;
        const double hs = p.compactness * hcm + (1.0 - p.compactness) * hsm;
        const double f = (1.0 - p.shape) * hc + p.shape * hs;
        out = (float)(f > 0.0 ? f : 0.0);
      }
    }
    cost[e] = out;
  }
}

// One thread per pixel a = y * W + x: its statistics, and the edges it owns, (a, a + 1) then (a, a + W), at their row of the
// sorted list.  A full row of the raster owns 2W - 1 edges, the last row W - 1.
__global__ __launch_bounds__(256) void pixel_regions_kernel(const unsigned char *__restrict__ tile, int H, int W, int nb,
                                                            long long *__restrict__ count, long long *__restrict__ sum,
                                                            long long *__restrict__ sumsq, int *__restrict__ bbox,
                                                            long long *__restrict__ peri, int *__restrict__ edges, int *__restrict__ weights) {
  const long long n = (long long)H * W;
  for (long long a = (long long)blockIdx.x * blockDim.x + threadIdx.x; a < n; a += (long long)gridDim.x * blockDim.x) {
    const int y = (int)(a / W), x = (int)(a - (long long)y * W);
    count[a] = 1;
    for (int c = 0; c < nb; ++c) {
      const long long v = tile[(long long)c * n + a];
      sum[a * nb + c] = v;
      sumsq[a * nb + c] = v * v;
    }
    bbox[4 * a] = x; bbox[4 * a + 1] = y; bbox[4 * a + 2] = x; bbox[4 * a + 3] = y;
    const bool right = x + 1 < W, down = y + 1 < H;
    const int inner = (x > 0) + right + (y > 0) + down;
    peri[2 * a] = inner; peri[2 * a + 1] = 4 - inner;
    long long row = (long long)y * (2 * W - 1) + (down ? 2 * x : x);
    if (right) {
      edges[2 * row] = (int)a; edges[2 * row + 1] = (int)a + 1;
      weights[row] = 1;
      ++row;
    }
    if (down) {
      edges[2 * row] = (int)a; edges[2 * row + 1] = (int)a + W;
      weights[row] = 1;
    }
  }
}

inline bool unit_range(double v, bool open_end) { return v >= 0.0 && (open_end ? v < 1.0 : v <= 1.0); }     // false for NaN
inline bool weight_ok(double v) { return v >= 0.0 && v <= DBL_MAX; }                          // finite, >= 0

}  // namespace

extern "C" int dm_region_merge_cost(const int64_t *count, const int64_t *sum, const int64_t *sumsq, const int32_t *bbox, const int64_t *peri,
                                    const int32_t *edges, const int32_t *weights, int32_t E, int32_t C, int32_t bands, double bw0, double bw1,
                                    double bw2, double shape, double compactness, float *cost, void *stream) {
  DM_REQUIRE(count && sum && sumsq && bbox && peri && edges && weights && cost, DM_ERR_BAD_SHAPE, "dm_region_merge_cost: null pointer");
  DM_REQUIRE(E > 0 && C > 0 && C <= (1 << 24), DM_ERR_BAD_SHAPE, "dm_region_merge_cost: bad sizes (E=%d C=%d; need E >= 1, 1 <= C <= 2^24)", E, C);
  DM_REQUIRE(bands >= 1 && bands <= 3, DM_ERR_BAD_SHAPE, "dm_region_merge_cost: bands = %d outside 1..3", bands);
  DM_REQUIRE(unit_range(shape, true) && unit_range(compactness, false), DM_ERR_BAD_SHAPE,
             "dm_region_merge_cost: need 0 <= shape < 1 and 0 <= compactness <= 1 (shape=%g compactness=%g)", shape, compactness);
  DM_REQUIRE(weight_ok(bw0) && weight_ok(bw1) && weight_ok(bw2), DM_ERR_BAD_SHAPE,
             "dm_region_merge_cost: band weights must be finite and >= 0 (%g %g %g)", bw0, bw1, bw2);
  const MrsParams p = {{bw0, bw1, bw2}, shape, compactness};
  hipLaunchKernelGGL(merge_cost_kernel, dim3(grid_for(E)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), (const long long *)count,
                     (const long long *)sum, (const long long *)sumsq, bbox, (const long long *)peri, edges, weights, E, C, bands, p, cost);
  DM_LAUNCH_CHECK("dm_region_merge_cost");
  return DM_OK;
}

extern "C" int dm_pixel_regions(const uint8_t *tile, int32_t bands, int32_t H, int32_t W, int64_t *count, int64_t *sum, int64_t *sumsq,
                                int32_t *bbox, int64_t *peri, int32_t *edges, int32_t *weights, void *stream) {
  DM_REQUIRE(tile && count && sum && sumsq && bbox && peri, DM_ERR_BAD_SHAPE, "dm_pixel_regions: null pointer");
  DM_REQUIRE(H > 0 && W > 0 && bands >= 1 && (long long)H * W <= (1LL << 24), DM_ERR_BAD_SHAPE,
             "dm_pixel_regions: bad sizes (H=%d W=%d bands=%d; need 1 <= H * W <= 2^24, bands >= 1)", H, W, bands);
  DM_REQUIRE((long long)H * W == 1 || (edges && weights), DM_ERR_BAD_SHAPE, "dm_pixel_regions: null edges / weights (only a 1 x 1 raster has no edge)");
  hipLaunchKernelGGL(pixel_regions_kernel, dim3(grid_for((long long)H * W)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), tile, H, W,
                     bands < 3 ? bands : 3, (long long *)count, (long long *)sum, (long long *)sumsq, bbox, (long long *)peri, edges, weights);
  DM_LAUNCH_CHECK("dm_pixel_regions");
  return DM_OK;
}
