// The split test of dm_simplify.hip, shared with the host check tools/simplify_host_check.cpp.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DM_HD __host__ __device__
#else
#define DM_HD
#endif

DM_HD static inline uint64_t dm_mul64hi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// 65536 d^2 > q2 len2 for distinct ends (d = |cross| < 2^31, len2 = |v[j] - v[i]|^2 <= 2^31, q2 = q^2 <= 2^40: both sides are
// below 2^78 and compared exactly as (high, low) 64-bit words), or 65536 d > q2 for coinciding ends (len2 == 0; d is then a squared
// distance <= 2^31).
DM_HD static inline bool dm_simplify_exceeds(uint64_t d, uint64_t len2, uint64_t q2) {
  if (len2 == 0) return (d << 16) > q2;
  const uint64_t d2 = d * d;                                     // < 2^62
  const uint64_t l_hi = d2 >> 48, l_lo = d2 << 16;
  const uint64_t r_hi = dm_mul64hi(q2, len2), r_lo = q2 * len2;
  return l_hi > r_hi || (l_hi == r_hi && l_lo > r_lo);
}
