// bf16 NT / NN GEMM on 128 x 128 tiles at FOUR workgroups per CU (gfx950), for the encoder's short-contraction forward and dgrad
// products (K = 768: the qkv / proj / fc1 forwards, the proj / fc2 dgrads of the 16384-token stage).
//
// Why a fourth kernel.  At K = 768 a 128 x 128 tile spends about as long outside its K loop (epilogue stores leaving the CU while the
// matrix pipe idles) as inside it, so the time of these products is set by how many OTHER workgroups of the CU have a K loop to run
// meanwhile.  The register-staged 128 x 128 kernel (dm_gemm.hip) stops at three workgroups per CU because of registers: its staged
// operands (32 VGPRs plus their waits and LDS writes) push it past 128 per lane.  Here the operands go global -> LDS by LDS-DMA
// (buffer_load_dwordx4 ... lds, as in dm_gemm_ring.hip), which needs no data registers at all:
//   * workgroup = 4 waves (2 x 2), 64 x 64 outputs per wave (acc[4][4], 64 accumulator registers), K tile 64;
//   * budget: <= 128 VGPR + AGPR per lane (four waves per SIMD), 32 KiB of LDS (one A and one B image; 4 x 32 <= 160 KiB), no scratch;
//   * one LDS stage: per K tile  vmcnt(0), barrier | k-step 0: fragments, 16 MFMAs | k-step 1: fragments, lgkmcnt(0), barrier,
//     DMA of the next K tile, 16 MFMAs.  The DMA of tile t + 1 runs under the second k-step of tile t and under the other three
//     workgroups' work: the latency this kernel exposes is what the fourth workgroup is for;
//   * LDS images (the layouts of dm_gemm.hip, built by per-lane SOURCE addresses because a DMA writes its 1 KiB lane-linearly):
//       k-contiguous operand (A; B of NT): [128 rows][8 chunks of 16 B], chunk c of row r in slot c ^ (r & 7);
//       m-contiguous operand (B of NN):    [64 k-rows][8 slots of 32 B], slot XOR tr_swz(k), read with ds_read_b64_tr_b16;
//   * same MFMA (v_mfma_f32_16x16x32_bf16, operands swapped), same fragments and same K order per accumulator as the 128 x 128 kernel,
//     and the same whole-line epilogue (dm_gemm_common.h): the outputs are bit-identical to that kernel's.
#include <cstdlib>

#include "dm_common.h"
#include "dm_gemm_common.h"
#include "dm_mfma.h"

namespace dmq4 {

constexpr int BK = 64, TILE = 128, NTHREADS = 256;
constexpr int IMG = TILE * 128;          // one operand image per K tile: 128 rows x 128 B, or 64 k-rows x 256 B
constexpr int LDS = 2 * IMG;
static_assert(LDS <= 40 * 1024, "four workgroups per CU: at most 40 KiB of LDS each");
static_assert(LDS >= 4 * 16 * DM_EPI_PITCH, "epilogue staging (16 rows per wave) must fit the operand images");

// the 32-byte slot swizzle of the m-contiguous image (dm_gemm.hip, tr_swz<4>)
__device__ __forceinline__ int tr_swz(int k) { return (k & 3) | (((k >> 3) & 1) << 2); }

// The accumulators stay pinned in AGPRs (as in dm_gemm_w4.hip): with the builtin the compiler keeps all 64 of them in VGPRs next to the
// fragments and spills at this register budget.  Same instruction and operand order as mma<bf16_t> (dm_mfma.h).  The asm opens with a
// wait state because the compiler cannot see that it is an MFMA (tools/isa_hazards.py checks the listing).
__device__ __forceinline__ void zero_pinned(f32x4 &acc, const u32x4 &z) {
  asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %1, 0" : "=a"(acc) : "v"(z));
}
__device__ __forceinline__ void mma_pinned(f32x4 &acc, const u32x4 &a, const u32x4 &b) {
  asm volatile("s_nop 0\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(b), "v"(a));
}

// descriptor of what is left of an operand (`bytes` from `base`) behind `skip` bytes: empty once nothing is left
#define DM_Q4_PIECE(base, bytes, skip) \
  __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>((base) + (skip)), 0, (int)max(0LL, min((bytes) - (skip), 0x7fffffffLL)), 0x00020000)
#define DM_Q4_DMA(rsrc, dst, voff, soff) \
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(dst), 16, voff, soff, 0, 0)

template <int LAYOUT>
__global__ __launch_bounds__(NTHREADS, 4) void gemm_q4_kernel(const GemmParams p) {
  constexpr bool B_MMAJOR = (LAYOUT == DM_NN);
  __shared__ __attribute__((aligned(16))) char smem[LDS];
  char *const ldsA = smem, *const ldsB = smem + IMG;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, li = lane & 15;

  // ---- tile of this workgroup: the walk of dm_gemm.hip's 128 x 128 kernel (XCD-contiguous ids, bands of group_m row tiles) ----
  int id = dm_xcd_remap(blockIdx.x, gridDim.x);
  int tm, tn;
  if (p.group_m > 0) {
    const int band = id / (p.group_m * p.tiles_n);
    const int within = id - band * (p.group_m * p.tiles_n);
    const int gsz = min(p.group_m, p.tiles_m - band * p.group_m);
    tn = within / gsz;
    tm = band * p.group_m + (within - tn * gsz);
  } else {
    tn = id % p.tiles_n;
    tm = id / p.tiles_n;
  }
  const int m0 = tm * TILE, n0 = tn * TILE;
  const int nk = p.K / BK;

  // ---- DMA addressing ---------------------------------------------------------------------------------------------------
  // The buffer range check covers the vector offset only (soffset is excluded from it), so no tile row or K step goes into soffset:
  // every DMA instruction gets a descriptor of its own whose BASE is moved to the piece's first row and the K tile (scalar work per
  // K tile) and whose extent is what is left of the operand behind that base.  A lane's vector offset is then the same for all
  // pieces and K tiles, and every row past the operand (or k-row past K) lies beyond the extent and reads zero.
  // k-contiguous operand: piece u of this wave = image rows (wave + 4u) * 8 .. +7, i.e. tile rows 32u + wave * 8 + (lane >> 3); the lane
  // fills slot lane & 7 of its row, which holds source chunk (lane & 7) ^ (row & 7).  With base = tile row 32u, column 64 kt and extent
  // = bytes of the operand from there: a row r < nrows has its 16-byte chunk inside (K - 64 kt >= 64 elements remain in its own row),
  // a row r >= nrows starts at least ld >= K elements past the last element.
  // m-contiguous operand (B of NN): piece u = k-rows (wave + 4u) * 4 .. +3 of the K tile, lane -> k-row 16u + wave * 4 + (lane >> 4),
  // byte (lane & 15) * 16 of it = slot (lane & 15) >> 1, half lane & 1; slot s of k-row k holds the 32-byte column group s ^ tr_swz(k).
  // tr_swz(k) depends on k & 3 and bit 1 of the wave only, not on u.  Column chunks past N are killed through the vector offset
  // (they would alias the next k-row).
  const int prow = lane >> 3, csrc = (lane & 7) ^ prow;
  const char *pa = reinterpret_cast<const char *>(p.A) + (long long)m0 * p.lda * 2;
  const long long bytesA = ((long long)(min(TILE, p.M - m0) - 1) * p.lda + p.K) * 2;      // from the tile's first row to the operand's end
  const int voA = (int)((long long)(wave * 8 + prow) * p.lda * 2 + csrc * 16);
  const char *pb;
  long long bytesB;
  int voB;
  if constexpr (!B_MMAJOR) {
    pb = reinterpret_cast<const char *>(p.B) + (long long)n0 * p.ldb * 2;
    bytesB = ((long long)(min(TILE, p.N - n0) - 1) * p.ldb + p.K) * 2;
    voB = (int)((long long)(wave * 8 + prow) * p.ldb * 2 + csrc * 16);
  } else {
    pb = reinterpret_cast<const char *>(p.B) + (long long)n0 * 2;
    bytesB = ((long long)(p.K - 1) * p.ldb + (p.N - n0)) * 2;
    const int k = wave * 4 + (lane >> 4);
    const int col = ((((lane & 15) >> 1) ^ tr_swz(k)) << 4) + ((lane & 1) << 3);
    voB = (n0 + col < p.N) ? (int)(((long long)k * p.ldb + col) * 2) : (int)0x80000000u;
  }
  const long long rowA = 32LL * p.lda * 2, stepB = B_MMAJOR ? 16LL * p.ldb * 2 : 32LL * p.ldb * 2;      // bytes from piece u to u + 1
  auto stage = [&](int kt) __attribute__((always_inline)) {
    // (DM_Q4_PIECE is a macro: as a lambda, the host pass silently fails to instantiate this kernel and emits no launch stub.  The
    // skips are advanced piece by piece behind empty asm statements, device pass only ("s" is no host constraint): otherwise the
    // compiler hoists all eight descriptors out of the K loop, and 32 more live SGPRs spill.)
    long long sa = (long long)kt * (BK * 2);
    long long sb = B_MMAJOR ? (long long)kt * BK * p.ldb * 2 : (long long)kt * (BK * 2);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#ifdef __HIP_DEVICE_COMPILE__
      asm volatile("" : "+s"(sa));
#endif
      DM_Q4_DMA(DM_Q4_PIECE(pa, bytesA, sa), ldsA + (wave + 4 * u) * 1024, voA, 0);
      sa += rowA;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#ifdef __HIP_DEVICE_COMPILE__
      asm volatile("" : "+s"(sb));
#endif
      DM_Q4_DMA(DM_Q4_PIECE(pb, bytesB, sb), ldsB + (wave + 4 * u) * 1024, voB, 0);
      sb += stepB;
    }
  };

  // ---- fragment reads (dm_gemm.hip's frag_kmajor / frag_mmajor for 128 x 128 bf16 tiles) --------------------------------------
  auto frag_k = [&](const char *img, int row, int kb) __attribute__((always_inline)) {
    return *reinterpret_cast<const u32x4 *>(img + row * 128 + (((kb * 4 + g) ^ (row & 7)) << 4));
  };
  auto frag_m = [&](const char *img, int col0, int kb) __attribute__((always_inline)) {
    const int q = (lane >> 2) & 3, pp = lane & 3;
    u32x4 out;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int k = kb * 32 + 8 * g + 4 * half + q;
      const u32x2 w = dm_ds_read_tr16(img + k * 256 + (((col0 >> 4) ^ tr_swz(k)) << 5) + (pp << 3));
      out[2 * half] = w[0];
      out[2 * half + 1] = w[1];
    }
    return out;
  };

  f32x4 acc[4][4];
  {
    u32x4 z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z[0]));
    z[1] = z[2] = z[3] = z[0];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) zero_pinned(acc[i][j], z);
  }

  // Epilogue read operands (fp32 residual; the saved GELU' of the fc2 dgrad) are touched towards L2 a few K tiles before the end, as in
  // the 128 x 128 kernel: one row per lane, one dword per 128-byte line, kept alive by the asm at the top of the epilogue.
  float tv0 = 0.f, tv1 = 0.f;
  const int touch_at = (!(p.debug & DM_DBG_TOUCH_OFF) && (p.residual || (p.aux && (p.epilogue == DM_EPI_DGELU || p.epilogue == DM_EPI_MUL)))) ? max(0, nk - 4) : -1;

  stage(0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of tile kt (and the touch) have landed
    __builtin_amdgcn_s_barrier();                          // ... and every other wave's
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      u32x4 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        fa[i] = frag_k(ldsA, wm * 64 + i * 16 + li, kb);
        if constexpr (B_MMAJOR) fb[i] = frag_m(ldsB, wn * 64 + i * 16, kb);
        else fb[i] = frag_k(ldsB, wn * 64 + i * 16 + li, kb);
      }
      if (kb == 1) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave is done reading tile kt
        __builtin_amdgcn_s_barrier();                            // every wave is: the images may be refilled
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < nk) stage(kt + 1);
        if (kt == touch_at) {
          const int m = m0 + wm * 64 + lane, n = n0 + wn * 64;
          if (m < p.M && n < p.N) {
            const DmGemmRow rw = dm_gemm_row(p, m);
            if (p.residual) {
              tv0 = p.residual[rw.r + n];
              if (n + 32 < p.N) tv1 = p.residual[rw.r + n + 32];
            } else if (p.aux_dtype == DM_F32) {
              tv0 = reinterpret_cast<const float *>(p.aux)[rw.x + n];
              if (n + 32 < p.N) tv1 = reinterpret_cast<const float *>(p.aux)[rw.x + n + 32];
            } else {
              tv0 = __builtin_bit_cast(float, (unsigned)reinterpret_cast<const unsigned short *>(p.aux)[rw.x + n]);
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) mma_pinned(acc[i][j], fa[i], fb[j]);
    }
  }

  // ---- epilogue: the whole-line form of dm_gemm_common.h through a wave-private piece of the (now idle) images --------------------
  // (every wave passed the last K tile's second barrier after its final fragment reads: nobody reads the images any more).  Only the
  // straight-line item forms are instantiated (LEAN_ONLY): the generic ones need more than the 64 VGPRs left beside the accumulators and
  // spill; the host routes only products whose epilogue has such a form (dm_gemm_q4_plan).
  // The compiler does not know the asm statements are MFMAs: without the pad it could copy an accumulator out of its AGPRs before the
  // last MFMA on it has retired; the empty asm makes every copy happen behind the pad.
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "+a"(acc[i][j]));
  asm volatile("" ::"v"(tv0), "v"(tv1));
  dm_epilogue_rows<4, 16, true>(p, acc, smem + wave * (16 * DM_EPI_PITCH), m0 + wm * 64, n0 + wn * 64, lane);
}

}  // namespace dmq4

// Decides whether this family runs the product; fills p.tiles_m / tiles_n / split_k.  Returns true when taken.
//   sw.q4 (DM_GEMM_Q4): 0 = off, 1 = routing rules, 2 = whenever legal.
bool dm_gemm_q4_plan(GemmParams &p, const GemmSwitches &sw, int layout, int ab_dtype, bool aligned8) {
  const int mode = sw.q4;
  if (mode == 0 || (layout != DM_NT && layout != DM_NN) || ab_dtype != DM_BF16 || !aligned8) return false;
  // whole K tiles, plain operands and results, the whole-line epilogue's alignment (dm_gemm.hip's rows_ok)
  if (p.K % dmq4::BK != 0 || p.N % 8 != 0 || p.k_fold > 0 || p.c_dtype == DM_BF16_PAIR) return false;
  // Store guard.  The shared lean epilogue steps its rows through the scalar offset of its buffer instructions, which the range check
  // does not cover: only a wave block that starts past M (an empty descriptor) and columns past N (killed vector offsets) are dropped
  // in hardware.  With M % 64 == 0 every row of a wave block that starts below M is a row of C, so nothing is written past it.
  if (p.M % 64 != 0) return false;
  // the A/B aids that take the whole-line / lean epilogue away from the 128 x 128 kernel (dm_gemm) keep products off this family
  if (dm_gemm_tuning().t128_rows_off || dm_gemm_tuning().epi_lean_off) return false;
  if (p.residual != nullptr && p.ldr % 8 != 0) return false;
  if (!dm_epi_key_specialised(dm_epi_lean_key(p, 64))) return false;      // the kernel instantiates the straight-line epilogues only
  if (128LL * p.lda * 2 >= (1LL << 31) || 128LL * p.ldb * 2 >= (1LL << 31)) return false;
  // In-step per-product times (tools/prof_shapes.py, same box, ms per step, incumbent -> this kernel): fc1 forward 16384 x 3072 + GELU'
  // 0.346 (ring) -> 0.297, fc2 dgrad 16384 x 3072 0.333 -> 0.292, qkv forward 16384 x 2304 0.228 -> 0.208, proj dgrad 16384 x 768
  // 0.096 -> 0.090, 4096 x 3072 forward / dgrad 0.073 / 0.070 -> 0.068 / 0.065: all K = 768, all at least three rounds of 128 x 128
  // tiles on 256 CUs.  The proj forward (NT 16384 x 768 + fp32 residual) measured 0.137 on both and stays where it was: narrow
  // forwards (N < 2304) are not routed.
  if (mode == 1 && !(p.K == 768 && (long long)((p.M + 127) / 128) * ((p.N + 127) / 128) >= 768 && !(layout == DM_NT && p.N < 2304))) return false;
  p.tiles_m = (p.M + dmq4::TILE - 1) / dmq4::TILE;
  p.tiles_n = (p.N + dmq4::TILE - 1) / dmq4::TILE;
  p.split_k = 1;
  p.k_per_split = p.K;
  return true;
}

void dm_gemm_q4_launch(const GemmParams &p, int layout, hipStream_t s) {
  const dim3 grid((unsigned)(p.tiles_m * p.tiles_n));
  if (layout == DM_NN) hipLaunchKernelGGL(dmq4::gemm_q4_kernel<DM_NN>, grid, dim3(dmq4::NTHREADS), 0, s, p);
  else hipLaunchKernelGGL(dmq4::gemm_q4_kernel<DM_NT>, grid, dim3(dmq4::NTHREADS), 0, s, p);
}
