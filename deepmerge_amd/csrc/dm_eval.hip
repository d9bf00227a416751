// Held-out pair evaluation (gfx950): the per-pair contrastive terms of Losses.py:34-38 and ONE pass over all N pairs of an
// evaluation that counts merge decisions at a set of thresholds per class and sums the terms -- what train()'s validation reads
// back once per epoch (deepmerge_amd/evaluate.py).  Both results are a contract:
//   dm_contrastive_terms   lane l of the pair's wave sums (a - b)^2 over its columns l, l+64, ... in order (rounded sub, mul, add),
//                          the 64 partials are combined by the xor butterfly 32, 16, ..., 1 (dm_wave_sum's order), then
//                          term = f*d2 + (1-f)*max(margin - d2, 0) left to right; no FMA contraction anywhere.
//   dm_pair_eval_summary   counts are integers (exact, arrival order irrelevant); the loss sum is fp64 over a partition that
//                          depends on N only, reduced in a fixed order: bit-identical from run to run.
#include "dm_common.h"

// The arithmetic order is a bit-exact contract with a numpy restatement: no a*b + c may become an FMA.  (__fmul_rn / __fadd_rn
// are inlined from the HIP headers with the contraction setting of their own context, so the Makefile also compiles this file
// with -ffp-contract=off.)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;          // summary: 4 waves per workgroup
constexpr int kMaxT = 1024;            // thresholds staged in LDS
constexpr int64_t kChunkMin = 4096;    // at least this many pairs per summary workgroup ...
constexpr int64_t kMaxGroups = 2048;   // ... and at most this many workgroups (8 per CU)

// One wave per pair; 4 pairs per 256-thread workgroup.
__global__ __launch_bounds__(256) void contrastive_terms_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                                const float *__restrict__ flag, float margin, float *__restrict__ d2,
                                                                float *__restrict__ term, int32_t B, int32_t D) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;                                        // wave-uniform: the whole wave leaves together
  const float *x = a + r * D, *y = b + r * D;
  float acc = 0.f;
  for (int c = lane; c < D; c += 64) {
    const float d = __fsub_rn(x[c], y[c]);
    acc = __fadd_rn(acc, __fmul_rn(d, d));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, o, 64));
  if (lane == 0) {
    const float f = flag[r];
    const float m = __fsub_rn(margin, acc);
    const float h = (m < 0.f) ? 0.f : m;                     // max(margin - d2, 0); NaN propagates, as torch.clamp does
    term[r] = __fadd_rn(__fmul_rn(f, acc), __fmul_rn(__fsub_rn(1.f, f), h));
    d2[r] = acc;
  }
}

// Workgroup g owns pairs [g chunk, min(N, (g + 1) chunk)).  Per pair: u = #{j : thresholds[j] <= simi} (upper bound; NaN -> T),
// so simi < thresholds[j] <=> u <= j; bin u of its class is counted in LDS, and the nonzero bins are added to the global
// histogram with integer atomics.  The terms are summed in fp64: thread t in index order, then the wave butterfly, then waves 0..3.
__global__ __launch_bounds__(kThreads) void pair_eval_count_kernel(const float *__restrict__ term, const float *__restrict__ simi,
                                                                   const float *__restrict__ flag, int64_t N, int64_t chunk,
                                                                   const float *__restrict__ thresholds, int32_t T,
                                                                   unsigned long long *__restrict__ hist, double *__restrict__ partial) {
  __shared__ float th[kMaxT];
  __shared__ unsigned int bins[2 * (kMaxT + 1)];
  __shared__ double wsum[kThreads / 64];
  const int tid = threadIdx.x;
  const int nb = T + 1;
  for (int j = tid; j < T; j += kThreads) th[j] = thresholds[j];
  for (int j = tid; j < 2 * nb; j += kThreads) bins[j] = 0u;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = min(N, lo + chunk);
  double acc = 0.0;
  for (int64_t i = lo + tid; i < hi; i += kThreads) {
    const float s = simi[i];
    int u = T;
    if (!__builtin_isnan(s)) {
      int l = 0, h = T;
      while (l < h) {
        const int mid = (l + h) >> 1;
        if (th[mid] <= s) l = mid + 1; else h = mid;
      }
      u = l;
    }
    atomicAdd(&bins[(flag[i] == 1.f ? 0 : nb) + u], 1u);
    acc += (double)term[i];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) wsum[tid >> 6] = acc;
  __syncthreads();
  for (int j = tid; j < 2 * nb; j += kThreads) {
    const unsigned int c = bins[j];
    if (c) atomicAdd(&hist[j], (unsigned long long)c);
  }
  if (tid == 0) {
    double s = wsum[0];
    for (int w = 1; w < kThreads / 64; ++w) s += wsum[w];
    partial[blockIdx.x] = s;
  }
}

// One workgroup of 1024 threads: merged[c][j] = prefix sums of the histogram of class c (Hillis-Steele in LDS over j < T),
// n_pos = every bin of class 0, loss_sum = the G partials in a fixed tree order.
__global__ __launch_bounds__(1024) void pair_eval_finish_kernel(const unsigned long long *__restrict__ hist,
                                                                const double *__restrict__ partial, int32_t G, int32_t T,
                                                                double *__restrict__ loss_sum, int64_t *__restrict__ merged,
                                                                int64_t *__restrict__ n_pos) {
  __shared__ unsigned long long scan[kMaxT];
  __shared__ double red[1024];
  const int tid = threadIdx.x;
  const int nb = T + 1;
  for (int c = 0; c < 2; ++c) {
    unsigned long long v = tid < T ? hist[c * nb + tid] : 0ull;
    scan[tid] = v;
    __syncthreads();
    for (int off = 1; off < kMaxT; off <<= 1) {
      const unsigned long long add = tid >= off ? scan[tid - off] : 0ull;
      __syncthreads();
      v += add;
      scan[tid] = v;
      __syncthreads();
    }
    if (tid < T) merged[(int64_t)c * T + tid] = (int64_t)v;
    if (c == 0 && tid == 0) *n_pos = (int64_t)(scan[T - 1] + hist[T]);
    __syncthreads();
  }
  double s = 0.0;
  for (int g = tid; g < G; g += 1024) s += partial[g];
  red[tid] = s;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (tid < w) red[tid] = red[tid] + red[tid + w];
    __syncthreads();
  }
  if (tid == 0) *loss_sum = red[0];
}

int64_t summary_groups(int64_t N, int64_t *chunk) {
  int64_t g = (N + kChunkMin - 1) / kChunkMin;
  if (g > kMaxGroups) g = kMaxGroups;
  *chunk = (N + g - 1) / g;
  return g;
}

}  // namespace

extern "C" int dm_contrastive_terms(const float *a, const float *b, const float *flag, float margin, float *d2, float *term, int32_t B,
                                    int32_t D, void *stream) {
  DM_REQUIRE(B >= 1 && D >= 1, DM_ERR_BAD_SHAPE, "dm_contrastive_terms: B = %d, D = %d (both must be >= 1)", B, D);
  DM_REQUIRE(a && b && flag && d2 && term, DM_ERR_BAD_SHAPE, "dm_contrastive_terms: bad arguments (null pointer)");
  const int64_t grid = ((int64_t)B + 3) / 4;
  hipLaunchKernelGGL(contrastive_terms_kernel, dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a, b, flag,
                     margin, d2, term, B, D);
  DM_LAUNCH_CHECK("dm_contrastive_terms");
  return DM_OK;
}

extern "C" int64_t dm_pair_eval_workspace_bytes(int64_t N, int32_t T) {
  if (N < 1 || T < 1 || T > kMaxT) return 0;
  int64_t chunk;
  const int64_t G = summary_groups(N, &chunk);
  return (int64_t)sizeof(unsigned long long) * 2 * (T + 1) + (int64_t)sizeof(double) * G;
}

extern "C" int dm_pair_eval_summary(const float *term, const float *simi, const float *flag, int64_t N, const float *thresholds, int32_t T,
                                    void *workspace, double *loss_sum, int64_t *merged, int64_t *n_pos, void *stream) {
  DM_REQUIRE(N >= 1 && N <= INT32_MAX, DM_ERR_BAD_SHAPE, "dm_pair_eval_summary: N = %lld pairs (1 .. 2^31 - 1)", (long long)N);
  DM_REQUIRE(T >= 1 && T <= kMaxT, DM_ERR_UNSUPPORTED, "dm_pair_eval_summary: %d thresholds (1 .. %d)", T, kMaxT);
  DM_REQUIRE(term && simi && flag && thresholds && workspace && loss_sum && merged && n_pos, DM_ERR_BAD_SHAPE,
             "dm_pair_eval_summary: bad arguments (null pointer)");
  int64_t chunk;
  const int64_t G = summary_groups(N, &chunk);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  unsigned long long *hist = static_cast<unsigned long long *>(workspace);
  double *partial = reinterpret_cast<double *>(hist + 2 * (T + 1));
  DM_REQUIRE(hipMemsetAsync(hist, 0, sizeof(unsigned long long) * 2 * (T + 1), s) == hipSuccess, DM_ERR_HIP,
             "dm_pair_eval_summary: clearing the histogram failed");
  hipLaunchKernelGGL(pair_eval_count_kernel, dim3((unsigned)G), dim3(kThreads), 0, s, term, simi, flag, N, chunk, thresholds, T, hist, partial);
  DM_LAUNCH_CHECK("dm_pair_eval_summary (count)");
  hipLaunchKernelGGL(pair_eval_finish_kernel, dim3(1), dim3(1024), 0, s, hist, partial, (int32_t)G, T, loss_sum, merged, n_pos);
  DM_LAUNCH_CHECK("dm_pair_eval_summary (finish)");
  return DM_OK;
}
