// Persistent, LDS-DMA-pipelined attention kernels (dm_attention_pipe.hip); dm_attention.hip routes to them.
#pragma once
#include <hip/hip_runtime.h>

#include "dm_attention_plan.h"

struct AttnPipeParams {
  const void *qkv;      // [B, N, 3, H, 64] bf16
  const float *bias;    // [H, N, N] fp32 or NULL
  void *out;            // [B, N, H*64] bf16
  float *lse;           // [B, H, N]
  int B, N, H;
  float scale;
  const float *table = nullptr;   // [bins, H] fp32 relative-position table of a (cube_s, 8, 8) token cube, instead of `bias` (q32 kernels only)
  int cube_s = 0;
};

// The launchers below launch exactly the instance the plan names (attn_plan_fwd / attn_plan_bwd decided; nothing is tested here).
// The 32-row ones return false if the instance's dynamic LDS size could not be set.
void dm_attn_fwd_pipe(const AttnFwdPlan &pl, const AttnPipeParams &p, hipStream_t s);      // ATTN_PIPE16
bool dm_attn_fwd_q32(const AttnFwdPlan &pl, const AttnPipeParams &p, hipStream_t s);       // ATTN_Q32 (dm_attention_q32.hip)

struct AttnPipeBwdParams {
  const void *qkv;      // [B, N, 3, H, 64] bf16
  const float *bias;    // [H, N, N] fp32 or NULL
  const void *out;      // [B, N, H*64] bf16 (forward output)
  const void *dout;     // [B, N, H*64] bf16
  const float *lse;     // [B, H, N]
  float *delta;         // [B, H, N] scratch: written by the dQ kernel, read by the dK/dV kernel
  void *dqkv;           // [B, N, 3, H, 64] bf16, fully written
  float *slab;          // [chunks, H, N, N] fp32 or NULL: sum over the chunk's samples of dS
  int B, N, H;
  float scale;
  const float *table = nullptr;   // [bins, H] relative-position table of a (cube_s, 8, 8) token cube: the q32 dQ kernel reads it instead of `bias`
  int cube_s = 0;
};

// dK / dV (+ slab) of ATTN_PIPE16, and dQ + delta in front of it where the plan's dQ pass is ATTN_PIPE16 too
void dm_attn_bwd_pipe(const AttnBwdPlan &pl, const AttnPipeBwdParams &p, hipStream_t s);
// dm_attention_q32_bwd.hip.  dQ + delta, ATTN_Q32 (this kernel writes no slab: the plan pairs it with a dK / dV pass that does)
bool dm_attn_bwd_dq_q32(const AttnBwdPlan &pl, const AttnPipeBwdParams &p, hipStream_t s);
// dK / dV, ATTN_Q32 (no bias) or ATTN_Q32_TABKV (table in LDS, + slab); reads p.delta: the dQ pass runs first
bool dm_attn_bwd_dkv_q32(const AttnBwdPlan &pl, const AttnPipeBwdParams &p, hipStream_t s);
