// Which attention kernel serves a call: decided once, here, as a plain value (implementation at the end of dm_attention.hip).
// The entry points validate, build an AttnCall, take the plan and hand it to the family's launcher, which launches exactly
// that instance; the query entries (slab chunks, "table in kernel", split shapes) answer from the same two functions.
#pragma once

// The DM_ATTN_* environment: read by attn_switches(), once per process.  All are A/B aids; the defaults are the product's.
struct AttnSwitches {
  int pipe = 1;            // DM_ATTN_PIPE      0: no 16-row pipeline (and no 32-row backward, which sits behind it); 2: no B * H rule
  int q32 = 1;             // DM_ATTN_Q32       0: no 32-row forward; 2: no B * H rule
  int q32_bwd = 1;         // DM_ATTN_Q32_BWD   0: no 32-row backward; 2: no B * H rule; 3: 32-row dQ, 16-row pipelined dK / dV
  bool q32_tabkv = true;   // DM_ATTN_Q32_TABKV 0: no table-reading dK / dV
  bool q32_w8 = true;      // DM_ATTN_Q32_W8    0: the bias-free 32-row forward / dQ on 4 waves also where 8 fit
  int q32_tabw = 8;        // DM_ATTN_Q32_TABW  4: the table-reading forward on 4 waves
  bool pf = true;          // DM_ATTN_PF        0: the 16-row pipelined forward without its prefetch
  bool xcd = true;         // DM_ATTN_XCD       0: the 16-row pipeline's workgroups in plain (head, block, chunk) order
  bool x3 = true;          // DM_ATTN_X3        0: no split-bf16 kernels
  bool x3_w8 = true;       // DM_ATTN_X3_W8     0: the split-bf16 forward / dQ on 4 waves
};
const AttnSwitches &attn_switches();

// What a routing decision depends on, and nothing else.
struct AttnCall {
  int B, N, H, D, dtype;
  bool dense;              // dense bias rows [H, N, N] are given
  bool table;              // a relative-position table of a (cube_s, 8, 8) token cube is given
  int cube_s;
  bool slab;               // the bias-gradient slab is wanted (backward)
  bool split;              // the split-bf16 ("bf16x3") entry points
};

enum AttnFamily {
  ATTN_GENERIC,            // dm_attention_generic.hip: any head dim, long N
  ATTN_REG16,              // dm_attention.hip: 16 rows per wave, scores in registers
  ATTN_PIPE16,             // dm_attention_pipe.hip: 16 rows per wave, persistent LDS-DMA pipeline
  ATTN_Q32,                // dm_attention_q32.hip / dm_attention_q32_bwd.hip: 32 rows per wave
  ATTN_Q32_TABKV,          // dm_attention_q32_bwd.hip: the table-reading dK / dV (+ slab)
  ATTN_X3,                 // dm_attention_x3.hip: split-bf16 products
};
enum AttnBias { ATTN_BIAS_NONE, ATTN_BIAS_DENSE, ATTN_BIAS_TABLE };
enum AttnRefusal { ATTN_TAKEN = 0, ATTN_SHAPE_NOT_TAKEN, ATTN_TABLE_NEEDS_BF16, ATTN_TABLE_NOT_TAKEN };

// One kernel launch.  nkt: key tiles of the family's width (16 or 32 tokens); ragged: N is not a whole number of tiles (masked
// instance); nblk / chunks / bchunk: row blocks per (sample, head), sample chunks, samples per chunk (attn_chunks, or the register
// kernels' batch_chunk).  Fields a family does not use stay 0.
struct AttnPass {
  AttnFamily family;
  int nkt;
  bool ragged;
  AttnBias bias;
  int waves;
  int nblk, chunks, bchunk;
};
struct AttnFwdPlan {
  AttnRefusal refused;
  AttnPass pass;
  bool pf, xcd;
};
struct AttnBwdPlan {
  AttnRefusal refused;
  AttnPass dq, dkv;        // the two passes may be of different families
  bool xcd;
  int slab_chunks;         // first dimension of the slab the dK / dV pass (register kernels: the dQ pass) fills
};
AttnFwdPlan attn_plan_fwd(const AttnCall &c, const AttnSwitches &sw);
AttnBwdPlan attn_plan_bwd(const AttnCall &c, const AttnSwitches &sw);

// The persistent kernels' chunk rule: `rows` query (key) rows per workgroup, as many sample chunks as fit one round of the 256 CUs.
inline void attn_chunks(int B, int N, int H, int rows, int &nblk, int &chunks, int &bchunk) {
  nblk = (N + rows - 1) / rows;
  chunks = 256 / (H * nblk);
  if (chunks < 1) chunks = 1;
  if (chunks > B) chunks = B;
  bchunk = (B + chunks - 1) / chunks;
  chunks = (B + bchunk - 1) / bchunk;
}
