// Open-addressing table of 64-bit keys with int32 counts in global memory, filled with integer atomics (dm_rag.hip: label pairs,
// dm_truth.hip: (label, truth) cells).  Keys are >= 0; a slot is claimed with one 64-bit CAS and counted with one 32-bit add, so
// the table's content does not depend on the order in which threads arrive.
#pragma once
#include "dm_common.h"

namespace {

constexpr long long EMPTY_KEY = -1;

__device__ __forceinline__ unsigned long long mix64(unsigned long long k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
  return k;
}
__device__ __forceinline__ void table_add(long long *keys, int *cnt, unsigned mask, long long key, int c, int *overflow) {
  unsigned slot = (unsigned)mix64((unsigned long long)key) & mask;
  for (unsigned probe = 0; probe <= mask; ++probe) {
    const long long seen = (long long)atomicCAS(reinterpret_cast<unsigned long long *>(keys + slot), (unsigned long long)EMPTY_KEY,
                                                (unsigned long long)key);
    if (seen == EMPTY_KEY || seen == key) {
      atomicAdd(cnt + slot, c);
      return;
    }
    slot = (slot + 1) & mask;
    if (probe > 4096) break;
  }
  atomicExch(overflow, 1);
}

__global__ void table_clear_kernel(long long *keys, int *cnt, long long n, int *overflow, int *n_out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    keys[i] = EMPTY_KEY;
    cnt[i] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { *overflow = 0; *n_out = 0; }
}

__global__ void table_compact_kernel(const long long *__restrict__ keys, const int *__restrict__ cnt, long long n,
                                     long long *__restrict__ out_keys, int *__restrict__ out_cnt, int *__restrict__ n_out, int max_out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long k = keys[i];
    if (k == EMPTY_KEY) continue;
    const int pos = atomicAdd(n_out, 1);
    if (pos < max_out) { out_keys[pos] = k; out_cnt[pos] = cnt[i]; }
  }
}

inline int grid_for(long long items, int cap = 8192) {
  long long g = (items + 255) / 256;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace
