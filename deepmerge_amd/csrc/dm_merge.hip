// Mutual-best-neighbour region merging on the device (gfx950): the rounds that follow the ExtractFeatures sweep, down to a
// merged label raster (the rule is stated in include/deepmerge_hip.h and restated in numpy in
// tests/merge_ref.py).  A round is: score (dm_segment_mean + dm_edge_similarity, unchanged) -> dm_merge_best ->
// dm_merge_match -> dm_merge_fold_regions -> dm_merge_edge_keys -> sort of the 64-bit keys -> dm_merge_fold_edges.
// An elimination round (min_area: regions below it propose, their neighbours accept) has dm_merge_best_small + dm_merge_accept
// in the place of dm_merge_best and is the same round from dm_merge_match on.
//
// Every quantity produced here is an integer (or a float copied bit for bit), and every reduction is an integer min or
// add, so the result does not depend on the order in which threads arrive: the GPU and the numpy spec agree bit for bit.
//
// Why a matching needs neither union-find nor a sort of the point lists.  An edge (a, b) is picked iff best[a] is b and
// best[b] is a.  Two picked edges cannot share a region r: both would be "the" best edge of r, and best[r] is one value
// (edges are unique, so one neighbour id names one edge).  Hence every region takes part in at most one merge per round,
// the merged components are single regions and pairs, root[b] = a is already the final labelling (no path to compress),
// and the merged point list of a pair is "segment of a, then segment of b": two block copies to an offset that an exclusive
// scan of the new counts provides.
//
// The scans run on dm_raster.h's block_exclusive (one looping workgroup).
#include "dm_raster.h"

namespace {

constexpr unsigned long long NO_BEST = ~0ULL;
constexpr long long SELF_KEY = LLONG_MAX;                 // relabelled self edge: sorts behind every live key

// ---- best neighbour ----------------------------------------------------------------------------------------------------
__global__ void best_clear_kernel(unsigned long long *__restrict__ best, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < C) best[i] = NO_BEST;
}

// key = (bits(simi) << 32) | other id: simi >= +0 after the sweep's clamp, so the bit pattern orders like the value and a
// tie goes to the smaller neighbour id.  The edge list is sorted by (a, b), so the lanes of a wave that share `a` are
// neighbours: their keys are min-reduced across the run with shuffles and the run's first lane issues ONE atomic for `a`
// (a grown region has tens of edges); the `b` side is scattered and takes one atomic per candidate edge.
//
// Who may take which edge is the kernel's template parameter: `edge(s)` says whether an edge of score s is a candidate at all,
// `side(r)` whether region r chooses among its candidate edges.
struct MarginRule {                                     // the mutual-best rounds: every region chooses among the edges below the margin
  float margin;
  __device__ __forceinline__ bool edge(float s) const { return s < margin; }                   // NaN is no candidate
  __device__ __forceinline__ bool side(int) const { return true; }
};
struct SmallRule {                                      // the elimination rounds: a small region proposes over every edge that has a score
  const long long *__restrict__ count;
  long long min_area;
  __device__ __forceinline__ bool edge(float s) const { return s == s; }                       // NaN is never usable
  __device__ __forceinline__ bool side(int r) const { return count[r] < min_area; }
};

template <typename Rule>
__global__ __launch_bounds__(256) void best_kernel(const int *__restrict__ edges, const float *__restrict__ simi, int E, int C, Rule rule,
                                                   unsigned long long *__restrict__ best) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long base = (long long)blockIdx.x * blockDim.x; base < E; base += stride) {      // uniform trip count per workgroup
    const long long e = base + threadIdx.x;
    int a = -1, b = -1;
    unsigned long long ka = NO_BEST;
    if (e < E) {
      a = edges[2 * e]; b = edges[2 * e + 1];
      const float s = simi[e];
      if (rule.edge(s) && (unsigned)a < (unsigned)C && (unsigned)b < (unsigned)C) {
        const unsigned long long hi = (unsigned long long)__float_as_uint(s) << 32;
        const bool mine = rule.side(a);
        if (mine) ka = hi | (unsigned)b;
        if (rule.side(b)) atomicMin(best + b, hi | (unsigned)a);
        if (!mine) a = -1;
      } else {
        a = -1;
      }
    }
    const int prev = __shfl_up(a, 1, 64);
    const bool head = lane == 0 || prev != a;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                  // segmented min over the run of equal `a` (runs are contiguous lanes)
      const unsigned long long ok = __shfl_down(ka, o, 64);
      const int oa = __shfl_down(a, o, 64);
      if (lane + o < 64 && oa == a && ok < ka) ka = ok;
    }
    if (head && a >= 0 && ka != NO_BEST) atomicMin(best + a, ka);
  }
}

// ---- accept (elimination rounds) ------------------------------------------------------------------------------------------
// A non-small region takes the smallest key (bits(simi) << 32) | s over the small regions s that proposed to it.  The kernel
// reads best[] only at small regions and writes it only at non-small ones, and the proposals of the small regions were all
// written by the launch before this one: every value read here is final when the kernel starts, whatever the thread order.
__global__ __launch_bounds__(256) void accept_kernel(const int *__restrict__ edges, const float *__restrict__ simi, int E, int C,
                                                     const long long *__restrict__ count, long long min_area,
                                                     unsigned long long *best) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (long long)gridDim.x * blockDim.x) {
    const int a = edges[2 * e], b = edges[2 * e + 1];
    if ((unsigned)a >= (unsigned)C || (unsigned)b >= (unsigned)C) continue;
    const bool sa = count[a] < min_area, sb = count[b] < min_area;
    if (sa == sb) continue;                             // two small regions settle it between themselves; two large ones have nothing to settle
    const int s = sa ? a : b, t = sa ? b : a;
    const unsigned long long bs = best[s];
    if (bs != NO_BEST && (unsigned)bs == (unsigned)t)   // edges are unique: the proposal that names t came over this edge
      atomicMin(best + t, ((unsigned long long)__float_as_uint(simi[e]) << 32) | (unsigned)s);
  }
}

// ---- match -------------------------------------------------------------------------------------------------------------
__global__ void match_init_kernel(int *__restrict__ root, int *__restrict__ pick, int C, int *__restrict__ n_picked) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < C) { root[i] = i; pick[i] = -1; }
  if (i == 0) *n_picked = 0;
}

// picked[e] iff best[a] names b and best[b] names a.  Picked edges form a matching (see the head of this file), so
// root[b] = a and pick[a] = e are written by one thread each.
__global__ __launch_bounds__(256) void match_kernel(const int *__restrict__ edges, const unsigned long long *__restrict__ best, int E, int C,
                                                    unsigned char *__restrict__ picked, int *__restrict__ root, int *__restrict__ pick,
                                                    int *__restrict__ n_picked) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (long long)gridDim.x * blockDim.x) {
    const int a = edges[2 * e], b = edges[2 * e + 1];
    bool p = false;
    if ((unsigned)a < (unsigned)C && (unsigned)b < (unsigned)C && a != b) {
      const unsigned long long ba = best[a], bb = best[b];
      p = ba != NO_BEST && bb != NO_BEST && (unsigned)ba == (unsigned)b && (unsigned)bb == (unsigned)a;
    }
    picked[e] = p ? 1 : 0;
    if (p) {
      root[b] = a;
      pick[a] = (int)e;
      atomicAdd(n_picked, 1);                          // one add per wave after the compiler's lane-count coalescing
    }
  }
}

// ---- three int streams scanned together (block_exclusive<I3>) ------------------------------------------------------------------
struct I3 { int x, y, z; };
__device__ __forceinline__ I3 operator+(I3 a, I3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ I3 operator-(I3 a, I3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ I3 shfl_up(I3 v, int o) { return {shfl_up(v.x, o), shfl_up(v.y, o), shfl_up(v.z, o)}; }

// ---- fold regions ------------------------------------------------------------------------------------------------------
// One workgroup walks the C regions in tiles: new dense id of every root (= rank among the roots, so ids stay in order of
// the surviving region's old id), start of its merged point list (scan of len(root) + len(absorbed)), and the rank of every
// absorbing root among the absorbing roots (= the row of its merge inside this round's history: picked edges have distinct
// `a` and the edge list is sorted by a).
__global__ __launch_bounds__(SCAN_THREADS) void fold_scan_kernel(const int *__restrict__ ptr, const int *__restrict__ edges,
                                                                 const int *__restrict__ root, const int *__restrict__ pick, int C, int E,
                                                                 int *__restrict__ new_id, int *__restrict__ hist_rank,
                                                                 int *__restrict__ new_ptr, int *__restrict__ n_regions) {
  __shared__ I3 lds[SCAN_THREADS / 64];
  I3 carry = {0, 0, 0};
  for (long long base = 0; base < C; base += SCAN_TILE) {
    I3 item[SCAN_ITEMS], sum = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      const long long r = base + (long long)threadIdx.x * SCAN_ITEMS + j;
      I3 v = {0, 0, 0};
      if (r < C && root[r] == (int)r) {
        v.x = 1;
        v.y = ptr[r + 1] - ptr[r];
        const int e = pick[r];
        if (e >= 0 && e < E) {
          const int b = edges[2 * (long long)e + 1];
          if ((unsigned)b < (unsigned)C) v.y += ptr[b + 1] - ptr[b];
          v.z = 1;
        }
      }
      item[j] = v;
      sum = sum + v;
    }
    I3 total;
    I3 run = carry + block_exclusive(sum, lds, total);
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      const long long r = base + (long long)threadIdx.x * SCAN_ITEMS + j;
      if (r < C && item[j].x) {
        new_id[r] = run.x;
        new_ptr[run.x] = run.y;
        hist_rank[r] = run.z;
      }
      run = run + item[j];
    }
    carry = carry + total;
  }
  if (threadIdx.x == 0) {
    new_ptr[carry.x] = carry.y;
    *n_regions = carry.x;
  }
}

// 8 lanes per old region copy its point list to its place in the merged list; lane 0 of a surviving region also writes the
// region's representative, its folded statistics and, if it absorbed a neighbour, the merge's history row.  The same grid
// carries the original superpixels' map forward.
__global__ __launch_bounds__(256) void fold_apply_kernel(DmMergeFold f) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nthreads = (long long)gridDim.x * blockDim.x;
  const int j = threadIdx.x & 7;
  for (long long r = t >> 3; r < f.C; r += nthreads >> 3) {
    const int rt = f.root[r];
    if ((unsigned)rt >= (unsigned)f.C) continue;
    const int nid = f.new_id[rt];
    const int beg = f.ptr[r], len = f.ptr[r + 1] - beg;
    long long dst = f.new_ptr[nid];
    if (rt != (int)r) dst += f.ptr[rt + 1] - f.ptr[rt];          // absorbed: behind the surviving region's own points
    for (int k = j; k < len; k += 8)
      if (dst + k < f.P) f.new_idx[dst + k] = f.idx[beg + k];
    if (j != 0 || rt != (int)r) continue;
    f.new_rep[nid] = f.rep[r];
    const int e = f.pick[r];
    const int b = (e >= 0 && e < f.E) ? f.edges[2 * (long long)e + 1] : -1;
    const bool merged = b >= 0 && b < f.C;
    if (merged) {
      const long long row = (long long)f.hist_base + f.hist_rank[r];
      if (row < f.hist_cap) {
        f.history[3 * row + 0] = f.round;
        f.history[3 * row + 1] = f.rep[r];
        f.history[3 * row + 2] = f.rep[b];
        f.history_simi[row] = f.simi[e];
      }
    }
    if (f.count) {
      const int nb = f.bands;
      long long cnt = f.count[r], pin = f.peri[2 * r], pbd = f.peri[2 * r + 1];
      int x0 = f.bbox[4 * r], y0 = f.bbox[4 * r + 1], x1 = f.bbox[4 * r + 2], y1 = f.bbox[4 * r + 3];
      if (merged) {
        cnt += f.count[b];
        pin += f.peri[2 * (long long)b] - 2LL * f.weights[e];      // the shared boundary stops being a boundary, on both sides
        pbd += f.peri[2 * (long long)b + 1];
        x0 = min(x0, f.bbox[4 * b]); y0 = min(y0, f.bbox[4 * b + 1]);
        x1 = max(x1, f.bbox[4 * b + 2]); y1 = max(y1, f.bbox[4 * b + 3]);
      }
      f.new_count[nid] = cnt;
      f.new_peri[2 * (long long)nid] = pin; f.new_peri[2 * (long long)nid + 1] = pbd;
      f.new_bbox[4 * nid] = x0; f.new_bbox[4 * nid + 1] = y0; f.new_bbox[4 * nid + 2] = x1; f.new_bbox[4 * nid + 3] = y1;
      for (int c = 0; c < nb; ++c) {
        long long s1 = f.sum[r * nb + c], s2 = f.sumsq[r * nb + c];
        if (merged) { s1 += f.sum[(long long)b * nb + c]; s2 += f.sumsq[(long long)b * nb + c]; }
        f.new_sum[(long long)nid * nb + c] = s1; f.new_sumsq[(long long)nid * nb + c] = s2;
      }
    }
  }
  for (long long s = t; s < f.S0; s += nthreads) {
    const int r = f.region_of[s];
    f.new_region_of[s] = ((unsigned)r < (unsigned)f.C) ? f.new_id[f.root[r]] : r;
  }
}

// ---- fold edges ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void edge_keys_kernel(const int *__restrict__ edges, const int *__restrict__ root,
                                                        const int *__restrict__ new_id, int E, int C, long long *__restrict__ keys) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (long long)gridDim.x * blockDim.x) {
    const int a = edges[2 * e], b = edges[2 * e + 1];
    long long key = SELF_KEY;
    if ((unsigned)a < (unsigned)C && (unsigned)b < (unsigned)C) {
      const int na = new_id[root[a]], nb = new_id[root[b]];
      if (na != nb) key = ((long long)min(na, nb) << 32) | (long long)max(na, nb);
    }
    keys[e] = key;
  }
}

// One workgroup walks the sorted keys in tiles: a key that differs from its predecessor opens a folded edge, an exclusive scan
// of those head flags is its row, and the head adds up the weights of its run (at most four sources: each endpoint stands
// for at most two old regions).
__global__ __launch_bounds__(SCAN_THREADS) void fold_edges_kernel(const long long *__restrict__ keys, const long long *__restrict__ order,
                                                                  const int *__restrict__ weights, int E, int *__restrict__ new_edges,
                                                                  int *__restrict__ new_weights, int *__restrict__ n_edges) {
  __shared__ int lds[SCAN_THREADS / 64];
  int carry = 0;
  for (long long base = 0; base < E; base += SCAN_TILE) {
    int head[SCAN_ITEMS], sum = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      const long long i = base + (long long)threadIdx.x * SCAN_ITEMS + j;
      head[j] = 0;
      if (i < E) {
        const long long k = keys[i];
        head[j] = (k != SELF_KEY && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
      }
      sum += head[j];
    }
    int total;
    int run = carry + block_exclusive(sum, lds, total);
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      const long long i = base + (long long)threadIdx.x * SCAN_ITEMS + j;
      if (head[j]) {
        const long long k = keys[i];
        new_edges[2 * (long long)run] = (int)(k >> 32);
        new_edges[2 * (long long)run + 1] = (int)(k & 0xffffffffLL);
        if (weights) {
          int w = 0;
          for (long long m = i; m < E && keys[m] == k; ++m) {
            const long long src = order[m];
            if (src >= 0 && src < E) w += weights[src];
          }
          new_weights[run] = w;
        }
      }
      run += head[j];
    }
    carry += total;
  }
  if (threadIdx.x == 0) *n_edges = carry;
}

// ---- relabel a raster ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int relabel_one(int l, const int *__restrict__ map, int S) { return ((unsigned)l < (unsigned)S) ? map[l] : l; }

// Stream: 16-byte loads and stores, four of them in flight per thread; the map (4 S bytes) stays in L2.
__global__ __launch_bounds__(256) void relabel_vec_kernel(const int *__restrict__ labels, const int *__restrict__ map,
                                                          int *__restrict__ out, long long n4, int S) {
  const i32x4 *in4 = reinterpret_cast<const i32x4 *>(labels);
  i32x4 *out4 = reinterpret_cast<i32x4 *>(out);
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    i32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = in4[i + u * stride];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      i32x4 o;
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = relabel_one(v[u][c], map, S);
      out4[i + u * stride] = o;
    }
  }
  for (; i < n4; i += stride) {
    const i32x4 v = in4[i];
    i32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = relabel_one(v[c], map, S);
    out4[i] = o;
  }
}

__global__ __launch_bounds__(256) void relabel_scalar_kernel(const int *__restrict__ labels, const int *__restrict__ map,
                                                             int *__restrict__ out, long long first, long long n, int S) {
  for (long long i = first + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    out[i] = relabel_one(labels[i], map, S);
}

}  // namespace

extern "C" int dm_merge_best(const int32_t *edges, const float *simi, int32_t E, int32_t C, float margin, uint64_t *best, void *stream) {
  DM_REQUIRE(edges && simi && best, DM_ERR_BAD_SHAPE, "dm_merge_best: null pointer");
  DM_REQUIRE(E > 0 && C > 0 && C <= (1 << 24), DM_ERR_BAD_SHAPE, "dm_merge_best: bad sizes (E=%d C=%d; need E >= 1, 1 <= C <= 2^24)", E, C);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(best_clear_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (unsigned long long *)best, C);
  hipLaunchKernelGGL(best_kernel<MarginRule>, dim3(grid_for(E)), dim3(256), 0, s, edges, simi, E, C, MarginRule{margin},
                     (unsigned long long *)best);
  DM_LAUNCH_CHECK("dm_merge_best");
  return DM_OK;
}

extern "C" int dm_merge_best_small(const int32_t *edges, const float *simi, int32_t E, int32_t C, const int64_t *count, int64_t min_area,
                                   uint64_t *best, void *stream) {
  DM_REQUIRE(edges && simi && count && best, DM_ERR_BAD_SHAPE, "dm_merge_best_small: null pointer");
  DM_REQUIRE(E > 0 && C > 0 && C <= (1 << 24), DM_ERR_BAD_SHAPE, "dm_merge_best_small: bad sizes (E=%d C=%d; need E >= 1, 1 <= C <= 2^24)", E, C);
  DM_REQUIRE(min_area >= 1, DM_ERR_BAD_SHAPE, "dm_merge_best_small: min_area = %lld, need >= 1", (long long)min_area);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(best_clear_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (unsigned long long *)best, C);
  hipLaunchKernelGGL(best_kernel<SmallRule>, dim3(grid_for(E)), dim3(256), 0, s, edges, simi, E, C,
                     SmallRule{(const long long *)count, (long long)min_area}, (unsigned long long *)best);
  DM_LAUNCH_CHECK("dm_merge_best_small");
  return DM_OK;
}

extern "C" int dm_merge_accept(const int32_t *edges, const float *simi, int32_t E, int32_t C, const int64_t *count, int64_t min_area,
                               uint64_t *best, void *stream) {
  DM_REQUIRE(edges && simi && count && best, DM_ERR_BAD_SHAPE, "dm_merge_accept: null pointer");
  DM_REQUIRE(E > 0 && C > 0 && C <= (1 << 24), DM_ERR_BAD_SHAPE, "dm_merge_accept: bad sizes (E=%d C=%d; need E >= 1, 1 <= C <= 2^24)", E, C);
  DM_REQUIRE(min_area >= 1, DM_ERR_BAD_SHAPE, "dm_merge_accept: min_area = %lld, need >= 1", (long long)min_area);
  hipLaunchKernelGGL(accept_kernel, dim3(grid_for(E)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), edges, simi, E, C,
                     (const long long *)count, (long long)min_area, (unsigned long long *)best);
  DM_LAUNCH_CHECK("dm_merge_accept");
  return DM_OK;
}

extern "C" int dm_merge_match(const int32_t *edges, const uint64_t *best, int32_t E, int32_t C, uint8_t *picked, int32_t *root,
                              int32_t *pick, int32_t *n_picked, void *stream) {
  DM_REQUIRE(edges && best && picked && root && pick && n_picked, DM_ERR_BAD_SHAPE, "dm_merge_match: null pointer");
  DM_REQUIRE(E > 0 && C > 0 && C <= (1 << 24), DM_ERR_BAD_SHAPE, "dm_merge_match: bad sizes (E=%d C=%d; need E >= 1, 1 <= C <= 2^24)", E, C);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(match_init_kernel, dim3((C + 255) / 256), dim3(256), 0, s, root, pick, C, n_picked);
  hipLaunchKernelGGL(match_kernel, dim3(grid_for(E)), dim3(256), 0, s, edges, (const unsigned long long *)best, E, C, picked, root, pick,
                     n_picked);
  DM_LAUNCH_CHECK("dm_merge_match");
  return DM_OK;
}

extern "C" int dm_merge_fold_regions(const DmMergeFold *args, void *stream) {
  DM_REQUIRE(args, DM_ERR_BAD_SHAPE, "dm_merge_fold_regions: null argument block");
  const DmMergeFold &f = *args;
  DM_REQUIRE(f.ptr && f.edges && f.root && f.pick && f.rep && f.region_of && f.simi && f.new_id && f.hist_rank && f.new_ptr &&
                 f.new_rep && f.new_region_of && f.n_regions && f.history && f.history_simi,
             DM_ERR_BAD_SHAPE, "dm_merge_fold_regions: null pointer");
  DM_REQUIRE(f.C > 0 && f.C <= (1 << 24) && f.P >= 0 && f.E > 0 && f.S0 > 0 && f.round >= 0 && f.hist_base >= 0 && f.hist_cap >= 0,
             DM_ERR_BAD_SHAPE, "dm_merge_fold_regions: bad sizes (C=%d P=%d E=%d S0=%d round=%d hist_base=%d hist_cap=%d)", f.C, f.P, f.E, f.S0,
             f.round, f.hist_base, f.hist_cap);
  DM_REQUIRE(f.P == 0 || (f.idx && f.new_idx), DM_ERR_BAD_SHAPE, "dm_merge_fold_regions: P = %d points but no idx / new_idx", f.P);
  if (f.count) {
    DM_REQUIRE(f.sum && f.sumsq && f.bbox && f.peri && f.weights && f.new_count && f.new_sum && f.new_sumsq && f.new_bbox && f.new_peri,
               DM_ERR_BAD_SHAPE, "dm_merge_fold_regions: statistics need all five arrays, their outputs and the edge weights");
    DM_REQUIRE(f.bands >= 1 && f.bands <= 3, DM_ERR_BAD_SHAPE, "dm_merge_fold_regions: bands = %d outside 1..3", f.bands);
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(fold_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, f.ptr, f.edges, f.root, f.pick, f.C, f.E, f.new_id, f.hist_rank,
                     f.new_ptr, f.n_regions);
  const long long work = (long long)f.C * 8 > f.S0 ? (long long)f.C * 8 : f.S0;
  hipLaunchKernelGGL(fold_apply_kernel, dim3(grid_for(work)), dim3(256), 0, s, f);
  DM_LAUNCH_CHECK("dm_merge_fold_regions");
  return DM_OK;
}

extern "C" int dm_merge_edge_keys(const int32_t *edges, const int32_t *root, const int32_t *new_id, int32_t E, int32_t C, int64_t *keys,
                                  void *stream) {
  DM_REQUIRE(edges && root && new_id && keys, DM_ERR_BAD_SHAPE, "dm_merge_edge_keys: null pointer");
  DM_REQUIRE(E > 0 && C > 0 && C <= (1 << 24), DM_ERR_BAD_SHAPE, "dm_merge_edge_keys: bad sizes (E=%d C=%d; need E >= 1, 1 <= C <= 2^24)", E, C);
  hipLaunchKernelGGL(edge_keys_kernel, dim3(grid_for(E)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), edges, root, new_id, E, C,
                     (long long *)keys);
  DM_LAUNCH_CHECK("dm_merge_edge_keys");
  return DM_OK;
}

extern "C" int dm_merge_fold_edges(const int64_t *sorted_keys, const int64_t *order, const int32_t *weights, int32_t E, int32_t *new_edges,
                                   int32_t *new_weights, int32_t *n_edges, void *stream) {
  DM_REQUIRE(sorted_keys && new_edges && n_edges, DM_ERR_BAD_SHAPE, "dm_merge_fold_edges: null pointer");
  DM_REQUIRE(!weights || (order && new_weights), DM_ERR_BAD_SHAPE, "dm_merge_fold_edges: weights need the sort's order and an output");
  DM_REQUIRE(E > 0, DM_ERR_BAD_SHAPE, "dm_merge_fold_edges: bad size (E=%d; need E >= 1)", E);
  hipLaunchKernelGGL(fold_edges_kernel, dim3(1), dim3(SCAN_THREADS), 0, reinterpret_cast<hipStream_t>(stream), (const long long *)sorted_keys,
                     (const long long *)order, weights, E, new_edges, new_weights, n_edges);
  DM_LAUNCH_CHECK("dm_merge_fold_edges");
  return DM_OK;
}

extern "C" int dm_relabel_raster(const int32_t *labels, const int32_t *map, int32_t *out, int64_t n, int32_t S, void *stream) {
  DM_REQUIRE(labels && map && out, DM_ERR_BAD_SHAPE, "dm_relabel_raster: null pointer");
  DM_REQUIRE(n > 0 && S > 0, DM_ERR_BAD_SHAPE, "dm_relabel_raster: bad sizes (n=%lld S=%d)", (long long)n, S);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  long long done = 0;
  if (dm_aligned16(labels) && dm_aligned16(out) && n >= 4) {
    const long long n4 = n / 4;
    hipLaunchKernelGGL(relabel_vec_kernel, dim3(grid_for(n4, 4096)), dim3(256), 0, s, labels, map, out, n4, S);
    done = n4 * 4;
  }
  if (done < n)                                        // unaligned rasters, and the tail of an aligned one
    hipLaunchKernelGGL(relabel_scalar_kernel, dim3(grid_for(n - done, 4096)), dim3(256), 0, s, labels, map, out, done, (long long)n, S);
  DM_LAUNCH_CHECK("dm_relabel_raster");
  return DM_OK;
}
