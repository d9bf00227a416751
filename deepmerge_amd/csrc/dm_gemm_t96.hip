// bf16 NT / NN GEMM on 128 x 96 tiles at ONE workgroup per CU over a ring of LDS-DMA stages (gfx950), for the 4096-token stage's
// long-contraction products with a 768-wide output (fc2 forward, fc1 / qkv dgrad, the patch embeds).
//
// Why a fifth kernel.  These products run as 64 x 64 register-staged tiles (768 workgroups, three per CU) and are bound by the bytes a
// tile pulls through L2 into LDS: (64 + 64) x K x 2 B per tile, 604 MB per launch of 4096 x 768 x 3072, 13 TB/s at 46 us.  128 x 128
// tiles halve the bytes but leave 192 workgroups for 256 CUs.  A 128 x 96 tile is exactly one round on a 4096 x 768 output (32 x 8 =
// 256 tiles) and moves 0.58 of the bytes.  One workgroup per CU has nobody to hide its latency behind, so the LDS it does not need for
// a second workgroup is spent on a ring of K-tile stages:
//   * workgroup = 4 waves (2 x 2), 64 x 48 outputs per wave (acc[4][3], 48 accumulator registers pinned in AGPRs), K tile 64;
//   * one stage = A image (128 rows x 128 B) + B image (96 rows x 128 B, or 64 k-rows x 192 B for the m-contiguous B of NN) = 28 KiB;
//     STAGES = 4 of them (112 KiB), filled by LDS-DMA with per-lane SOURCE addresses (a DMA writes its 1 KiB lane-linearly);
//   * per K tile t:  vmcnt(one stage's pieces), barrier      tile t + 1 has landed in every wave, tile t - 1 has been read by every wave
//                    12 MFMAs of (t, k-step 0); behind the first: fragments of (t, k-step 1) -> registers; between the next seven:
//                    the seven DMA pieces of tile t + 3 into the stage of tile t - 1
//                    fragments of (t + 1, k-step 0) -> registers, 12 MFMAs of (t, k-step 1)
//     one barrier per K tile; the fragments are double-buffered in registers so that an LDS read has a k-step of MFMAs to land under,
//     and two K tiles are in flight from L2 behind the one being read;
//   * images: k-contiguous operand [rows][8 chunks of 16 B], chunk c of row r in slot c ^ (r & 7) (dm_gemm_q4.hip's; the bank of a
//     ds_read_b128 depends on the 128-byte pitch and on row & 15 only, and the wave's 16-row blocks start at multiples of 16 also in
//     the 96-row image: each of the four 16-lane groups of the read covers 16 rows x one chunk = all 64 banks once).
//     m-contiguous operand [64 k-rows][6 slots of 32 B]: the 192-byte pitch itself moves k-rows k & 3 = 0..3 to banks 0, 48, 32, 16,
//     and slot s of k-row k holds column group s ^ ((k >> 3) & 1): the 32 lanes of one ds_read_b64_tr_b16 group (4 k-rows x 2 values
//     of bit 3 x 32 B) cover 8 distinct 8-bank blocks = all 64 banks once.  q4's XOR (256-byte pitch) does not carry over;
//   * same MFMA (v_mfma_f32_16x16x32_bf16, operands swapped), same fragments, same K order per accumulator as the register-staged tiles
//     and the same lean whole-line epilogue with a 48-column wave block (dm_gemm_common.h): bit-identical outputs.
#include <cstdlib>

#include "dm_common.h"
#include "dm_gemm_common.h"
#include "dm_mfma.h"

namespace dmt96 {

#ifndef DM_T96_STAGES
#define DM_T96_STAGES 4
#endif
constexpr int BK = 64, BM = 128, BN = 96, NTHREADS = 256, STAGES = DM_T96_STAGES;
constexpr int IMG_A = BM * 128, IMG_B = BN * 128;      // (64 k-rows x 192 B is the same 12 KiB)
constexpr int STAGE = IMG_A + IMG_B;
constexpr int LDS = STAGES * STAGE;
constexpr int NPIECE = 7;                              // DMA instructions per wave and stage: 4 of A, 3 of B
static_assert(LDS <= 160 * 1024, "one workgroup per CU: the whole LDS");
static_assert(STAGE >= 4 * 16 * DM_EPI_PITCH, "epilogue staging (16 rows per wave) must fit a stage");

// accumulators pinned in AGPRs, as in dm_gemm_q4.hip (same instruction and operand order as mma<bf16_t>; the asm opens with a wait state
// because the compiler cannot see that it is an MFMA: tools/isa_hazards.py checks the listing)
__device__ __forceinline__ void zero_pinned(f32x4 &acc, const u32x4 &z) {
  asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %1, 0" : "=a"(acc) : "v"(z));
}
__device__ __forceinline__ void mma_pinned(f32x4 &acc, const u32x4 &a, const u32x4 &b) {
  asm volatile("s_nop 0\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(b), "v"(a));
}

// One LDS-DMA piece: 64 lanes x 16 B from `base` + the lane's `voff` (nothing in soffset: the range check of the `ext` bytes behind
// `base` covers the vector offset only) to the 1 KiB at LDS address `dst`, lane-linear.  Written as asm because the compiler otherwise
// puts vmcnt(0) in front of every ds_read_b64_tr_b16 that follows a DMA it knows of (it cannot tell the stages apart), which would
// wait for the whole ring each K tile; the waits are the kernel's own counted ones.  m0 carries the LDS address; nothing else in this
// kernel uses it.
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void dma_piece(const char *base, int ext, unsigned dst, int voff) {
#ifdef __HIP_DEVICE_COMPILE__
  const unsigned long long a = reinterpret_cast<unsigned long long>(base);
  const u32x4 rsrc = {(unsigned)a, (unsigned)(a >> 32) & 0xffffu, (unsigned)ext, 0x00020000u};
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voff), "s"(rsrc), "s"(dst) : "memory", "m0");
#endif
}
// wait until at most N of this wave's DMA pieces are in flight (vmcnt retires in order: the oldest stages have landed)
template <int N> __device__ __forceinline__ void wait_pieces() {
  static_assert(N == 0 || N == 7 || N == 14 || N == 21, "one immediate per count");
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
  else if constexpr (N == 14) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(21)" ::: "memory");
}
__device__ __forceinline__ int clamp_extent(long long bytes) { return (int)max(0LL, min(bytes, 0x7fffffffLL)); }

template <int LAYOUT>
__global__ __launch_bounds__(NTHREADS, 1) void gemm_t96_kernel(const GemmParams p) {
  constexpr bool B_MMAJOR = (LAYOUT == DM_NN);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, li = lane & 15;

  // ---- tile of this workgroup: q4's walk (XCD-contiguous ids, bands of group_m row tiles) ----
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
  const int m0 = tm * BM, n0 = tn * BN;
  const int nk = p.K / BK;

  // ---- DMA addressing (q4's rules: nothing in soffset; one descriptor per piece, base moved to the piece's first row and the K tile,
  // extent = what is left of the operand behind that base, so rows past M / N and k-rows past K read zero) ------------------------------
  // k-contiguous operand: piece u of this wave = image rows (wave + 4u) * 8 .. +7 (A: u < 4, B of NT: u < 3); the lane fills slot
  // lane & 7 of row lane >> 3, which holds source chunk (lane & 7) ^ (row & 7).
  // m-contiguous operand (B of NN): this wave fills k-rows 16 wave .. +15 of the K tile = 3 KiB of the image in three lane-linear pieces;
  // byte o = 1024 j + 16 lane of them is k-row o / 192, slot (o % 192) >> 5, half (o >> 4) & 1 (192 = 12 x 16: a lane's 16 bytes never
  // straddle a row).  The three pieces share one descriptor (base = the K tile's first k-row and the tile's first column): the k-row
  // goes through the vector offset, which the range check covers; column chunks past N are killed through it (they would alias the
  // next k-row).
  const int prow = lane >> 3, csrc = (lane & 7) ^ prow;
  const char *pa = reinterpret_cast<const char *>(p.A) + (long long)m0 * p.lda * 2;
  const long long bytesA = ((long long)(min(BM, p.M - m0) - 1) * p.lda + p.K) * 2;      // from the tile's first row to the operand's end
  const int voA = (int)((long long)(wave * 8 + prow) * p.lda * 2 + csrc * 16);
  const char *pb;
  long long bytesB;
  int voB[3];
  if constexpr (!B_MMAJOR) {
    pb = reinterpret_cast<const char *>(p.B) + (long long)n0 * p.ldb * 2;
    bytesB = ((long long)(min(BN, p.N - n0) - 1) * p.ldb + p.K) * 2;
    voB[0] = voB[1] = voB[2] = (int)((long long)(wave * 8 + prow) * p.ldb * 2 + csrc * 16);
  } else {
    pb = reinterpret_cast<const char *>(p.B) + (long long)n0 * 2;
    bytesB = ((long long)(p.K - 1) * p.ldb + (p.N - n0)) * 2;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int o = j * 1024 + lane * 16;
      const int kl = o / 192, in = o - kl * 192;
      const int col = (((in >> 5) ^ ((kl >> 3) & 1)) << 4) + (((in >> 4) & 1) << 3);
      voB[j] = (n0 + col < p.N) ? (int)(((long long)(wave * 16 + kl) * p.ldb + col) * 2) : (int)0x80000000u;
    }
  }
  // Descriptors: the pieces' first rows and their extents (what is left of the operand below the piece's first row) do not change from
  // K tile to K tile, only the base moves on by 128 B: a row r below the operand's last keeps its 16 bytes inside the extent (at least
  // 64 elements of its own row remain), a row past it starts ld >= K elements behind the last element, whatever the K tile.  Two scalar
  // adds per piece and K tile; one workgroup per CU has nobody to issue under, so the loop's scalar work counts.
  // `on` = false empties the descriptor: the piece still counts in vmcnt (the waits below are the same for every K tile) and writes zeros
  // into a stage nobody reads any more.
  const char *paU[4], *pbU[3];
  int extA[4], extB[3];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    paU[u] = pa + 32LL * u * p.lda * 2;
    extA[u] = clamp_extent(bytesA - 32LL * u * p.lda * 2);
  }
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    pbU[u] = B_MMAJOR ? pb : pb + 32LL * u * p.ldb * 2;
    extB[u] = B_MMAJOR ? 0 : clamp_extent(bytesB - 32LL * u * p.ldb * 2);
  }
  // piece i of a stage: 0 .. 3 = A, 4 .. 6 = B.  (The empty asm keeps the compiler from carrying every K tile's descriptors in SGPRs.)
  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)reinterpret_cast<size_t>((__attribute__((address_space(3))) char *)smem));
  auto piece = [&](int i, int kt, int dst, bool on) __attribute__((always_inline)) {
    long long sk = (long long)kt * (BK * 2);
#ifdef __HIP_DEVICE_COMPILE__
    asm volatile("" : "+s"(sk));
#endif
    if (i < 4) {
      dma_piece(paU[i] + sk, on ? extA[i] : 0, lds0 + dst + (wave + 4 * i) * 1024, voA);
    } else if constexpr (!B_MMAJOR) {
      const int u = i - 4;
      dma_piece(pbU[u] + sk, on ? extB[u] : 0, lds0 + dst + IMG_A + (wave + 4 * u) * 1024, voB[u]);
    } else {
      const int u = i - 4;
      long long sb = (long long)kt * BK * p.ldb * 2;      // (the m-contiguous operand: base on the K tile's first k-row, extent cut)
#ifdef __HIP_DEVICE_COMPILE__
      asm volatile("" : "+s"(sb));
#endif
      dma_piece(pb + sb, on ? clamp_extent(bytesB - sb) : 0, lds0 + dst + IMG_A + (wave * 3 + u) * 1024, voB[u]);
    }
  };

  // ---- fragment reads ---------------------------------------------------------------------------------------------------------
  auto frag_k = [&](const char *img, int row, int kb) __attribute__((always_inline)) {
    return *reinterpret_cast<const u32x4 *>(img + row * 128 + (((kb * 4 + g) ^ (row & 7)) << 4));
  };
  auto frag_m = [&](const char *img, int col0, int kb) __attribute__((always_inline)) {
    const int q = (lane >> 2) & 3, pp = lane & 3;
    u32x4 out;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int k = kb * 32 + 8 * g + 4 * half + q;
      const u32x2 w = dm_ds_read_tr16(img + k * 192 + (((col0 >> 4) ^ (g & 1)) << 5) + (pp << 3));      // (k >> 3) & 1 == g & 1
      out[2 * half] = w[0];
      out[2 * half + 1] = w[1];
    }
    return out;
  };
  auto read_frags = [&](u32x4 (&fa)[4], u32x4 (&fb)[3], int slot, int kb) __attribute__((always_inline)) {
    const char *ia = smem + slot * STAGE, *ib = ia + IMG_A;
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = frag_k(ia, wm * 64 + i * 16 + li, kb);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if constexpr (B_MMAJOR) fb[j] = frag_m(ib, wn * 48 + j * 16, kb);
      else fb[j] = frag_k(ib, wn * 48 + j * 16 + li, kb);
    }
  };

  f32x4 acc[4][3];
  {
    u32x4 z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z[0]));
    z[1] = z[2] = z[3] = z[0];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) zero_pinned(acc[i][j], z);
  }

  // ---- prologue: three K tiles in flight, the first one's two k-steps in registers ----------------------------------------------------
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
#pragma unroll
    for (int i = 0; i < NPIECE; ++i) piece(i, s, s * STAGE, s < nk);
  wait_pieces<NPIECE * (STAGES - 2)>();      // tile 0 has landed: the other stages' pieces of this wave may still be in flight
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  u32x4 fa0[4], fb0[3], fa1[4], fb1[3];
  read_frags(fa0, fb0, 0, 0);
  __builtin_amdgcn_sched_barrier(0);

  // ---- K loop.  Per K tile kt (fragments of its k-step 0 in fa0 / fb0 since the previous tile's k-step 1):
  //   vmcnt(7), barrier        tile kt + 1 has landed in every wave (only tile kt + 2 may be in flight); every wave has read tile kt - 1
  //   MFMA 0 of k-step 0       (the compiler waits for the LDS reads in flight in front of it: they had the previous k-step to land)
  //   fragments of k-step 1 -> fa1 / fb1
  //   MFMAs 1 .. 11 of k-step 0, behind the first seven of them one DMA piece each of tile kt + 3 -> the stage of tile kt - 1
  //   fragments of (kt + 1, k-step 0) -> fa0 / fb0 (past the last tile: a stage nobody fills any more; never used)
  //   12 MFMAs of k-step 1
  int slot = 0;                                   // stage of tile kt
  for (int kt = 0; kt < nk; ++kt) {
    wait_pieces<NPIECE * (STAGES - 3)>();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    const bool more = kt + STAGES - 1 < nk;
    const int dst = (slot == 0 ? STAGES - 1 : slot - 1) * STAGE;      // the stage of tile kt - 1
    mma_pinned(acc[0][0], fa0[0], fb0[0]);
    __builtin_amdgcn_sched_barrier(0);
    read_frags(fa1, fb1, slot, 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int m = 1; m < 12; ++m) {
      mma_pinned(acc[m / 3][m % 3], fa0[m / 3], fb0[m % 3]);
      if (m <= NPIECE) piece(m - 1, kt + STAGES - 1, dst, more);
    }
    __builtin_amdgcn_sched_barrier(0);
    slot = (slot + 1 == STAGES) ? 0 : slot + 1;
    read_frags(fa0, fb0, slot, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) mma_pinned(acc[i][j], fa1[i], fb1[j]);
    __builtin_amdgcn_sched_barrier(0);
  }
  static_assert(STAGES >= 3 && NPIECE * (STAGES - 2) < 64, "vmcnt counts up to 63");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the emptied pieces of the last three K tiles still write their zeros

  // ---- epilogue: the lean whole-line form through a wave-private piece of the (now idle) ring ----------------------------------------
  // Every DMA of this wave has landed; the barrier below says so of every wave, and that every wave is done reading.  The pad
  // keeps the compiler's accumulator copies behind the last asm MFMA, as in dm_gemm_q4.hip.
  __builtin_amdgcn_s_barrier();
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) asm volatile("" : "+a"(acc[i][j]));
  dm_epilogue_rows<4, 16, true, 3>(p, acc, smem + wave * (16 * DM_EPI_PITCH), m0 + wm * 64, n0 + wn * 48, lane);
}

template <int LAYOUT> bool set_lds_limit() {
  return hipFuncSetAttribute(reinterpret_cast<const void *>(gemm_t96_kernel<LAYOUT>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS) == hipSuccess;
}

}  // namespace dmt96

// Decides whether this family runs the product; fills p.tiles_m / tiles_n / split_k.  Returns true when taken.
//   sw.t96 (DM_GEMM_T96): 0 = off, 1 = routing rule, 2 = whenever legal.
bool dm_gemm_t96_plan(GemmParams &p, const GemmSwitches &sw, int layout, int ab_dtype, bool aligned8) {
  const int mode = sw.t96;
  if (mode == 0 || (layout != DM_NT && layout != DM_NN) || ab_dtype != DM_BF16 || !aligned8) return false;
  if (p.K % dmt96::BK != 0 || p.N % 8 != 0 || p.k_fold > 0 || p.c_dtype == DM_BF16_PAIR) return false;
  // store guard, as in dm_gemm_q4_plan: the lean epilogue drops a wave block that starts past M and columns past N in hardware, its rows
  // step through the scalar offset; with M % 64 == 0 every row of a wave block that starts below M is a row of C
  if (p.M % 64 != 0) return false;
  if (dm_gemm_tuning().t128_rows_off || dm_gemm_tuning().epi_lean_off) return false;
  if (p.residual != nullptr && p.ldr % 8 != 0) return false;
  // the epilogues of the target products: bf16 C, fp32 C, fp32 C + fp32 residual (each with or without bias)
  if (p.epilogue != DM_EPI_NONE || p.accumulate) return false;
  const int key = dm_epi_lean_key(p, 64);
  if (!(key == 0 || key == (1 << 3) || key == (1 | (1 << 3)))) return false;
  if (128LL * p.lda * 2 >= (1LL << 31) || 128LL * p.ldb * 2 >= (1LL << 31)) return false;
  const long long tiles = (long long)((p.M + dmt96::BM - 1) / dmt96::BM) * ((p.N + dmt96::BN - 1) / dmt96::BN);
  if (tiles >= (1LL << 31)) return false;
  if (mode == 1) {
    // One round of tiles (0.75 .. 1.0 of the CUs), whole column tiles, a narrow output with a contraction at least as long as it is wide.
    // In-step per-product times (tools/prof_shapes.py, same box, ms per step over two launches, 64 x 64 tiles -> this kernel; the spread
    // between two passes is 0.001): NT 4096 x 768 x 3072 + fp32 residual 0.094 -> 0.078, NN 4096 x 768 x 3072 0.087 -> 0.074,
    // NN 4096 x 768 x 2304 0.073 -> 0.058, NT 4096 x 768 x 768 + residual 0.041 -> 0.038, NN 4096 x 768 x 768 0.034 -> 0.030
    // (profiles/t96_route_ab.txt).  Wider outputs of one round (1024 x 2304, 1024 x 3072) were not measured and stay where they are;
    // the patch embeds (grouped rows) have no lean epilogue and are refused above.
    const long long cus = dm_gemm_cu_count();
    if (!(p.K >= 768 && p.N <= 768 && p.N % dmt96::BN == 0 && tiles <= cus && 4 * tiles >= 3 * cus)) return false;
  }
  static const bool ok = dmt96::set_lds_limit<DM_NT>() && dmt96::set_lds_limit<DM_NN>();
  if (!ok) return false;
  p.tiles_m = (p.M + dmt96::BM - 1) / dmt96::BM;
  p.tiles_n = (p.N + dmt96::BN - 1) / dmt96::BN;
  p.split_k = 1;
  p.k_per_split = p.K;
  return true;
}

void dm_gemm_t96_launch(const GemmParams &p, int layout, hipStream_t s) {
  const dim3 grid((unsigned)(p.tiles_m * p.tiles_n));
  if (layout == DM_NN) hipLaunchKernelGGL(dmt96::gemm_t96_kernel<DM_NN>, grid, dim3(dmt96::NTHREADS), dmt96::LDS, s, p);
  else hipLaunchKernelGGL(dmt96::gemm_t96_kernel<DM_NT>, grid, dim3(dmt96::NTHREADS), dmt96::LDS, s, p);
}
