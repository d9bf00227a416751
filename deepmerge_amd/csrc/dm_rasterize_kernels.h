// The device code of polygon rasterisation, shared by dm_rasterize.hip (a whole raster) and dm_scene_rasterize.hip (a band of rows
// and a window of columns of a scene).  The rule is stated in include/deepmerge_hip.h and restated in numpy in
// tests/rasterize_ref.py; its band and window form in tests/scene_rasterize_ref.py.
//
// Every kernel is written for a BAND, the pixel rows [r0, r1) of an H x W raster, and a WINDOW, the columns [x0, x1) of that band;
// the whole raster is the band [0, H) and the window [0, W).  Coordinates, rows and columns are the raster's; only the key and the
// output are relative to the band and the window:
//   key   (label (r1 - r0) + (row - r0)) (W + 1) + cx, cx clamped to [0, W]: one sort of a band's keys serves every window of it
//   out   int32 [r1 - r0, x1 - x0], pixel (row, c) at (row - r0) (x1 - x0) + (c - x0)
// An event is one crossing of an edge with the centre line of a pixel row of the band.
//   count   per edge (vertex v to its successor within its ring): the events it has
//   emit    per EVENT: the edge by an upper-bound search in the scan of the counts, the row, the event's column cx, and the key.
//           An edge across thousands of rows is thousands of threads, not one thread's loop.
//   fill    per pair (2j, 2j+1) of the SORTED keys: the label over columns [cx_a, cx_b) of the row, intersected with the window.
//           16 consecutive lanes take 16 consecutive pixels; a span is cut into pieces of FILL_CHUNK columns over blockIdx.y, the
//           first at max(cx_a, x0), so no piece is walked for long and no lane walks columns left of the window.
#pragma once
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

// Rows r in [r0, r1) with y0 <= 256 r + 128 < y1: first row and how many.
__device__ __forceinline__ int rows_of(const Edge &e, int r0, int r1, int &first) {
  long long lo = ceil_div(e.y0 - HALF, SUB), hi = ceil_div(e.y1 - HALF, SUB) - 1;
  if (lo < r0) lo = r0;
  if (hi > r1 - 1) hi = r1 - 1;
  first = (int)lo;
  return hi >= lo ? (int)(hi - lo + 1) : 0;
}

__global__ void rasterize_count_kernel(const int *__restrict__ xy, const long long *__restrict__ ring_ptr, const int *__restrict__ vert_ring, int V,
                                       int R, int r0, int r1, int *__restrict__ count) {
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
    Edge e;
    int first;
    count[v] = edge_of(xy, ring_ptr, vert_ring, v, V, R, e) ? rows_of(e, r0, r1, first) : 0;
  }
}

__global__ void rasterize_emit_kernel(const int *__restrict__ xy, const long long *__restrict__ ring_ptr, const int *__restrict__ vert_ring,
                                      const int *__restrict__ ring_label, const long long *__restrict__ scan, int V, int R, long long N, int r0,
                                      int r1, int W, long long *__restrict__ keys) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
    int lo = 0, hi = V;                                          // the last v with scan[v] <= i: scan[0] = 0 <= i < N = scan[V]
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      if (scan[mid] <= i) lo = mid; else hi = mid;
    }
    Edge e;
    int first;
    long long key = -1;                                          // tables that disagree with the scan: fill reports the pair
    if (edge_of(xy, ring_ptr, vert_ring, lo, V, R, e) && i - scan[lo] < rows_of(e, r0, r1, first)) {
      const int row = first + (int)(i - scan[lo]);
      const long long dy = e.y1 - e.y0, yc = (long long)SUB * row + HALF;
      const long long num = e.x0 * dy + (yc - e.y0) * (e.x1 - e.x0);          // the crossing is at num / dy
      long long cx = ceil_div(num - HALF * dy, SUB * dy);                     // first column whose centre is not left of it
      cx = cx < 0 ? 0 : (cx > W ? W : cx);
      key = ((long long)ring_label[e.ring] * (r1 - r0) + (row - r0)) * (W + 1LL) + cx;
    }
    keys[i] = key;
  }
}

__global__ void rasterize_preset_kernel(int *__restrict__ out, long long n, int fill, int *__restrict__ error) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = fill;
  if (blockIdx.x == 0 && threadIdx.x == 0) *error = 0;
}

// rows = r1 - r0 of the band the keys were made for; out is [rows, x1 - x0].  The error is reported for every pair, by the
// workgroups of blockIdx.y == 0, whether or not its span meets the window.
__global__ __launch_bounds__(256) void rasterize_fill_kernel(const long long *__restrict__ keys, long long pairs, int rows, int W, int x0, int x1,
                                                             int *__restrict__ out, int *__restrict__ error) {
  const int lane = threadIdx.x & (FILL_LANES - 1);
  const long long groups = (long long)gridDim.x * (256 / FILL_LANES);
  const long long ww = (long long)x1 - x0;
  for (long long p = (long long)blockIdx.x * (256 / FILL_LANES) + threadIdx.x / FILL_LANES; p < pairs; p += groups) {
    const long long a = keys[2 * p], b = keys[2 * p + 1];
    const long long ga = a / (W + 1LL), gb = b / (W + 1LL);
    const long long label = ga / rows;
    if (a < 0 || ga != gb || label >= INT_MAX) {                 // cannot happen for closed rings with labels below 2^31 - 1
      if (lane == 0 && blockIdx.y == 0) atomicExch(error, 1);
      continue;
    }
    const long long base = (ga - label * rows) * ww - x0;        // row < rows, and the columns written are in [x0, x1): every write is inside
    const long long c0 = a - ga * (W + 1LL), c1 = b - gb * (W + 1LL);
    const long long from = c0 > x0 ? c0 : x0, to = c1 < x1 ? c1 : x1;
    for (long long c_lo = from + (long long)blockIdx.y * FILL_CHUNK; c_lo < to; c_lo += (long long)gridDim.y * FILL_CHUNK) {
      const long long end = to < c_lo + FILL_CHUNK ? to : c_lo + FILL_CHUNK;
      for (long long c = c_lo + lane; c < end; c += FILL_LANES) atomicMax(out + base + c, (int)label);
    }
  }
}

// Host: the pre-set and the fill of one window [rows, x1 - x0] on stream s.
inline void launch_fill(const int64_t *keys, int64_t N, int rows, int W, int x0, int x1, int fill, int32_t *out, int32_t *error, hipStream_t s) {
  const long long n = (long long)rows * (x1 - x0);
  hipLaunchKernelGGL(rasterize_preset_kernel, dim3(grid_for(n)), dim3(256), 0, s, out, n, fill, error);
  const int chunks = (x1 - x0 - 1) / FILL_CHUNK + 1;
  if (N > 0)
    hipLaunchKernelGGL(rasterize_fill_kernel, dim3(grid_for(N / 2 * FILL_LANES, 1 << 16), chunks < 1024 ? chunks : 1024), dim3(256), 0, s,
                       (const long long *)keys, (long long)(N / 2), rows, W, x0, x1, out, error);
}

}  // namespace
