// Polygon rings rasterised into a label raster (gfx950): the inverse of dm_vector.hip.  The reference reads its superpixels, and
// its users digitise their ground truth, as polygons written by external GIS software; every raster pass of this build starts from
// a label raster.  The rule is the build's own: stated in include/deepmerge_hip.h, restated in numpy in tests/rasterize_ref.py
// (DESIGN.md 3.5.6).  Coordinates are fixed point with 8 sub-pixel bits and every product is an integer below 2^60, so the device
// and the spec agree bit for bit; the raster is written with integer max alone, so no result depends on the order of arrival.
//
// An event is one crossing of an edge with the centre line of a pixel row inside the raster.
//   count   per edge (vertex v to its successor within its ring): the events it has
//   emit    per EVENT: the edge by an upper-bound search in the scan of the counts, the row, the event's column cx, and the key
//           (label H + row) (W + 1) + cx.  An edge across thousands of rows is thousands of threads, not one thread's loop.
//   fill    per pair (2j, 2j+1) of the SORTED keys: the label over columns [cx_a, cx_b) of the row.  16 consecutive lanes take 16
//           consecutive pixels; a span is cut into pieces of FILL_CHUNK columns over blockIdx.y, so no piece is walked for long.
// The scan of the counts and the sort of the keys between the stages are the caller's (rag.rasterize: torch.cumsum, torch.sort).
#include "dm_raster.h"

namespace {

constexpr int SUB = DM_RASTERIZE_SUBPIXEL, HALF = SUB / 2;     // fixed-point units per pixel; the pixel centre
constexpr int FILL_LANES = 16, FILL_CHUNK = 1024;

__device__ __forceinline__ long long ceil_div(long long a, long long b) {          // b > 0
  const long long q = a / b;
  return q + ((a % b) > 0);
}

// The edge from vertex v to its successor within its ring, ends ordered so that y0 < y1; false for a horizontal edge and for a
// vertex whose ring tables do not hold it.
struct Edge {
  long long x0, y0, x1, y1;
  int ring;
};

__device__ __forceinline__ bool edge_of(const int *__restrict__ xy, const long long *__restrict__ ring_ptr, const int *__restrict__ vert_ring,
                                        int v, int V, int R, Edge &e) {
  const int r = vert_ring[v];
  if (r < 0 || r >= R) return false;
  const long long first = ring_ptr[r], end = ring_ptr[r + 1];
  if (first < 0 || end > V || v < first || v >= end) return false;
  const int w = v + 1 == end ? (int)first : v + 1;              // closed: the last vertex joins the first
  long long x0 = xy[2 * (long long)v], y0 = xy[2 * (long long)v + 1], x1 = xy[2 * (long long)w], y1 = xy[2 * (long long)w + 1];
  if (y0 == y1) return false;
  if (y0 > y1) { long long t = x0; x0 = x1; x1 = t; t = y0; y0 = y1; y1 = t; }
  e.x0 = x0; e.y0 = y0; e.x1 = x1; e.y1 = y1; e.ring = r;
  return true;
}

// Rows r in [0, H) with y0 <= 256 r + 128 < y1: first row and how many.
__device__ __forceinline__ int rows_of(const Edge &e, int H, int &first) {
  long long lo = ceil_div(e.y0 - HALF, SUB), hi = ceil_div(e.y1 - HALF, SUB) - 1;
  if (lo < 0) lo = 0;
  if (hi > H - 1) hi = H - 1;
  first = (int)lo;
  return hi >= lo ? (int)(hi - lo + 1) : 0;
}

__global__ void rasterize_count_kernel(const int *__restrict__ xy, const long long *__restrict__ ring_ptr, const int *__restrict__ vert_ring, int V,
                                       int R, int H, int *__restrict__ count) {
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
    Edge e;
    int first;
    count[v] = edge_of(xy, ring_ptr, vert_ring, v, V, R, e) ? rows_of(e, H, first) : 0;
  }
}

__global__ void rasterize_emit_kernel(const int *__restrict__ xy, const long long *__restrict__ ring_ptr, const int *__restrict__ vert_ring,
                                      const int *__restrict__ ring_label, const long long *__restrict__ scan, int V, int R, long long N, int H,
                                      int W, long long *__restrict__ keys) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
    int lo = 0, hi = V;                                          // the last v with scan[v] <= i: scan[0] = 0 <= i < N = scan[V]
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      if (scan[mid] <= i) lo = mid; else hi = mid;
    }
    Edge e;
    int first;
    long long key = -1;                                          // tables that disagree with the scan: fill reports the pair
    if (edge_of(xy, ring_ptr, vert_ring, lo, V, R, e) && i - scan[lo] < rows_of(e, H, first)) {
      const int row = first + (int)(i - scan[lo]);
      const long long dy = e.y1 - e.y0, yc = (long long)SUB * row + HALF;
      const long long num = e.x0 * dy + (yc - e.y0) * (e.x1 - e.x0);          // the crossing is at num / dy
      long long cx = ceil_div(num - HALF * dy, SUB * dy);                     // first column whose centre is not left of it
      cx = cx < 0 ? 0 : (cx > W ? W : cx);
      key = ((long long)ring_label[e.ring] * H + row) * (W + 1) + cx;
    }
    keys[i] = key;
  }
}

__global__ void rasterize_preset_kernel(int *__restrict__ out, long long n, int fill, int *__restrict__ error) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = fill;
  if (blockIdx.x == 0 && threadIdx.x == 0) *error = 0;
}

__global__ __launch_bounds__(256) void rasterize_fill_kernel(const long long *__restrict__ keys, long long pairs, int H, int W, int *__restrict__ out,
                                                             int *__restrict__ error) {
  const int lane = threadIdx.x & (FILL_LANES - 1);
  const long long groups = (long long)gridDim.x * (256 / FILL_LANES);
  for (long long p = (long long)blockIdx.x * (256 / FILL_LANES) + threadIdx.x / FILL_LANES; p < pairs; p += groups) {
    const long long a = keys[2 * p], b = keys[2 * p + 1];
    const long long ga = a / (W + 1), gb = b / (W + 1);
    const long long label = ga / H;
    if (a < 0 || ga != gb || label >= INT_MAX) {                 // cannot happen for closed rings with labels below 2^31 - 1
      if (lane == 0 && blockIdx.y == 0) atomicExch(error, 1);
      continue;
    }
    const long long base = (ga - label * H) * W;                 // row < H, and both columns are in [0, W]: every write is inside
    const long long c0 = a - ga * (W + 1), c1 = b - gb * (W + 1);
    for (long long c_lo = (long long)blockIdx.y * FILL_CHUNK; c_lo < c1; c_lo += (long long)gridDim.y * FILL_CHUNK) {
      const long long from = c0 > c_lo ? c0 : c_lo, to = c1 < c_lo + FILL_CHUNK ? c1 : c_lo + FILL_CHUNK;
      for (long long c = from + lane; c < to; c += FILL_LANES) atomicMax(out + base + c, (int)label);
    }
  }
}

inline bool raster_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W < (1LL << 31); }

}  // namespace

extern "C" int dm_rasterize_count(const int32_t *xy, const int64_t *ring_ptr, const int32_t *vert_ring, int32_t V, int32_t R, int32_t H, int32_t W,
                                  int32_t *count, void *stream) {
  DM_REQUIRE(xy && ring_ptr && vert_ring && count, DM_ERR_BAD_SHAPE, "dm_rasterize_count: null pointer");
  DM_REQUIRE(raster_ok(H, W) && V > 0 && V <= (1 << 30) && R > 0, DM_ERR_BAD_SHAPE,
             "dm_rasterize_count: bad sizes (H=%d W=%d V=%d R=%d; need H, W, R >= 1, 1 <= V <= 2^30, H*W < 2^31)",
             H, W, V, R);
  hipLaunchKernelGGL(rasterize_count_kernel, dim3(grid_for(V)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), xy,
                     (const long long *)ring_ptr, vert_ring, V, R, H, count);
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
                     (const long long *)ring_ptr, vert_ring, ring_label, (const long long *)scan, V, R, (long long)N, H, W, (long long *)keys);
  DM_LAUNCH_CHECK("dm_rasterize_emit");
  return DM_OK;
}

extern "C" int dm_rasterize_fill(const int64_t *keys, int64_t N, int32_t H, int32_t W, int32_t fill, int32_t *out, int32_t *error, void *stream) {
  DM_REQUIRE(out && error && (N == 0 || keys), DM_ERR_BAD_SHAPE, "dm_rasterize_fill: null pointer");
  DM_REQUIRE(raster_ok(H, W) && N >= 0 && N <= (1LL << 30) && N % 2 == 0 && fill < 0, DM_ERR_BAD_SHAPE,
             "dm_rasterize_fill: bad arguments (H=%d W=%d N=%lld fill=%d; need H, W >= 1, H*W < 2^31, N even in 0..2^30, fill < 0)", H, W,
             (long long)N, fill);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rasterize_preset_kernel, dim3(grid_for((long long)H * W)), dim3(256), 0, s, out, (long long)H * W, fill, error);
  const int chunks = (W - 1) / FILL_CHUNK + 1;
  if (N > 0)
    hipLaunchKernelGGL(rasterize_fill_kernel, dim3(grid_for(N / 2 * FILL_LANES, 1 << 16), chunks < 1024 ? chunks : 1024), dim3(256), 0, s,
                       (const long long *)keys, (long long)(N / 2), H, W, out, error);
  DM_LAUNCH_CHECK("dm_rasterize_fill");
  return DM_OK;
}
