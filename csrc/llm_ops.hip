// llm_ops.hip — hand-written CDNA4 (gfx950 / MI355X) kernels for the
// Llama-3.2 / Gemma-2 decode + prefill forward pass.
//
// Design notes (MI355X-first, per /opt/skills/guides/cdna_hip_programming.md):
//  - wave64 everywhere; block sizes are multiples of 64
//  - bf16 I/O, fp32 accumulation; all bf16 traffic vectorized 16 B/lane
//  - decode is weight-bandwidth-bound: the GEMV kernel streams W rows with
//    deep unrolled dwordx4 loads straight to VGPRs (no LDS round trip for
//    the streamed operand — guide §5 "GEMV / M<=16 decode weights")
//  - attention never materializes QK^T: online softmax in registers
//  - KV cache is a preallocated pool, written in place (decode: inside
//    the fused attention kernel; prefill: k_rope_cache) — replaces the
//    reference's O(T^2) concat cache (llama3.2_model.py:325)
//  - every kernel is hipGraph-capture-safe (no mallocs/syncs; sequence
//    position and sampled token ids live in device memory)
//
// Replaces (reference parity):
//  K1 softmax RawKernel      -> online softmax in k_attn_dec /
//                               k_attn_prefill_mfma / k_attn
//  K2 cuBLAS GEMM/GEMV       -> k_gemv_{bf16,fp8}_t (decode),
//                               k_gemm_bf16 MFMA (prefill)
//  K3 elementwise ufuncs     -> fused GEMV staging (NORM/GLU/NORM2),
//                               k_rmsnorm, k_glu, k_softcap, k_addinto
//  K4 KV concat              -> in-place pool writes
//  K5 repeat_kv              -> attention indexes kv_head = q_head/groups
//  K7 torch.multinomial      -> k_logit_max + k_sample_pick (last-block commit)

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "common.h"

// ====================================================================
// GEMV: y[N] = W[N,K] @ stage(x)[K]  (+ res)  (optional softcap, f32 out)
// W bf16 row-major; one wave per output row; the input vector is staged
// once into LDS with an optional fused pre-op (this is where the decode
// path's RMSNorm and GLU live — they cost an LDS pass, not a kernel):
//   stage 0 (RAW):  xs = x1
//   stage 1 (NORM): xs = rmsnorm(x1) * g     (g fp32, Gemma +1 prefolded)
//   stage 2 (GLU):  xs = act(x1) * x2        (act 0 = SiLU, 1 = tanh-GELU)
// Decode is bound by streaming W once: target ~HBM roofline.
// ====================================================================

#define GEMV_ROWS_PER_BLOCK 4
#define STAGE_RAW 0
#define STAGE_NORM 1
#define STAGE_GLU 2
// NORM2 (Gemma sandwich fusion): h' = h + rmsnorm(x)*g  (post-norm +
// residual), block 0 persists h' to global, then xs = rmsnorm(h')*g2
// (pre-norm of the projection this GEMV computes).  Removes the two
// standalone k_rmsnorm launches per Gemma layer.
#define STAGE_NORM2 3
// NORM_EMBED: like NORM but x = embedding TABLE base; the row is
// gathered at *tok (device token id) and scaled by escale first —
// fuses the k_embed launch into the first QKV GEMV of the decode step.
#define STAGE_NORM_EMBED 4

// act(gate)*up, bf16-rounded: the one GLU expression (k_glu, STAGE_GLU
// and the paired-row GEMV epilogue all produce the same bits)
DEVINL u16 glu_act(float xx, float u, int act) {
  float a;
  if (act == 0) {
    a = xx / (1.f + __expf(-xx));
  } else {
    float c = 0.7978845608028654f * (xx + 0.044715f * xx * xx * xx);
    a = 0.5f * xx * (1.f + tanhf(c));
  }
  return f2b(a * u);
}

// staging helper shared by bf16/fp8 GEMV (RMSNorm / GLU fused pre-ops)
DEVINL float stage_red_sum(float* red) {
  const int nw = blockDim.x >> 6;
  float t = 0.f;
  for (int w = 0; w < nw; w++) t += red[w];
  return t;
}

// The bf16 staging pass is split in two so the GEMV can put its first
// weight loads between them: gemv_stage_issue() issues every global
// load of the pass's FIRST iteration (i0 = tid*8: all of it for
// K <= 8*blockDim) into registers, the kernel then issues its weight
// prologue, and gemv_stage() does the arithmetic, barriers and LDS
// writes.  vmcnt retires in order, so only loads issued BEFORE the
// weights can be waited for without draining the weight stream too.
// Addresses are clamped instead of predicated (unconditional loads; a
// thread with i0 >= K ignores what it fetched).
struct StagePre {
  s8v v, hv;             // x (GLU: gate) / h (GLU: up) chunk
  f4v ga, gb;            // gamma chunk (fp32)
};

DEVINL void gemv_stage_issue(StagePre& p, const u16*& x, const u16* x2,
                             const float* g, int K, int stage) {
  int i = threadIdx.x * 8;
  if (i > K - 8) i = K - 8;
  if (stage == STAGE_NORM_EMBED)  // x = table: gather row *x2 (token id)
    x += (size_t)(*(const int*)x2) * (size_t)K;
  p.v = *(const s8v*)(x + i);
  if (stage == STAGE_NORM2 || stage == STAGE_GLU)
    p.hv = *(const s8v*)(x2 + i);
  if (stage == STAGE_NORM || stage == STAGE_NORM_EMBED ||
      stage == STAGE_NORM2) {
    p.ga = *(const f4v*)(g + i);
    p.gb = *(const f4v*)(g + i + 4);
  }
  // NORM2's g2 is NOT hoisted: 8 more live VGPRs cost the RPW=1 kernel a
  // wave of occupancy, and its first use sits behind three barriers, by
  // when the prologue loads it then waits for have long landed
}

// x is the pointer gemv_stage_issue left (NORM_EMBED: the gathered row)
DEVINL const u16* gemv_stage(char* smem, const StagePre& p, const u16* x,
                             const u16* x2, const float* g, const float* g2,
                             u16* hout, int K, int stage, int act, float eps,
                             float escale) {
  u16* xs = (u16*)smem;
  const int STRIDE = blockDim.x * 8;
  const int i0 = threadIdx.x * 8;
  float* red = (float*)(smem + (size_t)K * 2);
  if (stage == STAGE_NORM2) {
    // x2 = h_in (read-only here); block 0 persists h' into hout — a
    // DIFFERENT buffer (ping-pong), since other blocks still read h_in
    const u16* h = x2;
    // pass 1: sumsq of x (the un-normed projection output t)
    float ss = 0.f;
    auto p1 = [&](s8v v) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        float f = b2f(((u16*)&v)[j]);
        ss += f * f;
      }
    };
    if (i0 < K) p1(p.v);
    for (int i = i0 + STRIDE; i < K; i += STRIDE) p1(*(const s8v*)(x + i));
    ss = wave_reduce_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    float rnorm_a = rsqrtf(stage_red_sum(red) / (float)K + eps);
    __syncthreads();
    // pass 2: h' = h + norm_a(x)*g (bf16-rounded, matching the
    // standalone k_rmsnorm mode 1), stash h' in LDS, sumsq of h'
    float ss2 = 0.f;
    auto p2 = [&](int i, s8v v, s8v hv, f4v ga, f4v gb) {
      u16 o[8];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        float f = b2f(((u16*)&v)[j]) * rnorm_a * (j < 4 ? ga[j] : gb[j - 4])
                  + b2f(((u16*)&hv)[j]);
        o[j] = f2b(f);
        float fr = b2f(o[j]);
        ss2 += fr * fr;
      }
      *(s8v*)(xs + i) = *(s8v*)o;
      if (blockIdx.x == 0) *(s8v*)(hout + i) = *(s8v*)o;  // persist h'
    };
    if (i0 < K) p2(i0, p.v, p.hv, p.ga, p.gb);
    for (int i = i0 + STRIDE; i < K; i += STRIDE)
      p2(i, *(const s8v*)(x + i), *(const s8v*)(h + i),
         *(const f4v*)(g + i), *(const f4v*)(g + i + 4));
    ss2 = wave_reduce_sum(ss2);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss2;
    __syncthreads();
    float rnorm_b = rsqrtf(stage_red_sum(red) / (float)K + eps);
    // pass 3: xs = norm_b(h')*g2
    auto p3 = [&](int i, f4v ga, f4v gb) {
      s8v v = *(s8v*)(xs + i);
      u16 o[8];
#pragma unroll
      for (int j = 0; j < 8; j++)
        o[j] = f2b(b2f(((u16*)&v)[j]) * rnorm_b *
                   (j < 4 ? ga[j] : gb[j - 4]));
      *(s8v*)(xs + i) = *(s8v*)o;
    };
    for (int i = i0; i < K; i += STRIDE)
      p3(i, *(const f4v*)(g2 + i), *(const f4v*)(g2 + i + 4));
    __syncthreads();
    return xs;
  }
  if (stage == STAGE_NORM || stage == STAGE_NORM_EMBED) {
    // NORM_EMBED: the gathered row is scaled by escale (bf16-rounded,
    // matching the standalone k_embed), and block 0 persists it as the
    // residual-stream h
    float ss = 0.f;
    auto p1 = [&](int i, s8v v) {
      if (stage == STAGE_NORM_EMBED) {
        u16 o[8];
#pragma unroll
        for (int j = 0; j < 8; j++)
          o[j] = f2b(b2f(((u16*)&v)[j]) * escale);
        v = *(s8v*)o;
        if (blockIdx.x == 0) *(s8v*)(hout + i) = v;
      }
      *(s8v*)(xs + i) = v;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        float f = b2f(((u16*)&v)[j]);
        ss += f * f;
      }
    };
    if (i0 < K) p1(i0, p.v);
    for (int i = i0 + STRIDE; i < K; i += STRIDE)
      p1(i, *(const s8v*)(x + i));
    ss = wave_reduce_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    float rnorm = rsqrtf(stage_red_sum(red) / (float)K + eps);
    auto p2 = [&](int i, f4v ga, f4v gb) {
      s8v v = *(s8v*)(xs + i);
      u16 o[8];
#pragma unroll
      for (int j = 0; j < 8; j++)
        o[j] = f2b(b2f(((u16*)&v)[j]) * rnorm *
                   (j < 4 ? ga[j] : gb[j - 4]));
      *(s8v*)(xs + i) = *(s8v*)o;
    };
    if (i0 < K) p2(i0, p.ga, p.gb);
    for (int i = i0 + STRIDE; i < K; i += STRIDE)
      p2(i, *(const f4v*)(g + i), *(const f4v*)(g + i + 4));
  } else {  // STAGE_GLU
    auto p1 = [&](int i, s8v gv, s8v uv) {
      u16 o[8];
#pragma unroll
      for (int j = 0; j < 8; j++)
        o[j] = glu_act(b2f(((u16*)&gv)[j]), b2f(((u16*)&uv)[j]), act);
      *(s8v*)(xs + i) = *(s8v*)o;
    };
    if (i0 < K) p1(i0, p.v, p.hv);
    for (int i = i0 + STRIDE; i < K; i += STRIDE)
      p1(i, *(const s8v*)(x + i), *(const s8v*)(x2 + i));
  }
  __syncthreads();
  return xs;
}

// f32 variant of the staging pass, used by the fp8 GEMV: x lands in LDS
// as fp32 PAIRS so the inner loop can feed v_pk_fma_f32 directly from
// the v_cvt_pk_f32_fp8 outputs (the round-1 fp8 stream was
// conversion-VALU-bound at 4.3 TB/s — this halves the VALU work per
// weight byte).  Semantics match gemv_stage: the NORM2-persisted h' is
// still bf16-rounded (it feeds the residual stream), only the staged
// vector skips the final bf16 round-trip (within GEMV tolerance).
DEVINL const float* gemv_stage_f32(char* smem, const u16* x, const u16* x2,
                                   const float* g, const float* g2,
                                   u16* hout, int K, int stage, int act,
                                   float eps, float escale) {
  float* xs = (float*)smem;
  const int STRIDE = blockDim.x * 8;
  if (stage == STAGE_RAW) {
    for (int i = threadIdx.x * 8; i < K; i += STRIDE) {
      s8v v = *(const s8v*)(x + i);
#pragma unroll
      for (int j = 0; j < 8; j++) xs[i + j] = b2f(((u16*)&v)[j]);
    }
    __syncthreads();
    return xs;
  }
  float* red = (float*)(smem + (size_t)K * 4);
  if (stage == STAGE_NORM2) {
    const u16* h = x2;
    float ss = 0.f;
    for (int i = threadIdx.x * 8; i < K; i += STRIDE) {
      s8v v = *(const s8v*)(x + i);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        float f = b2f(((u16*)&v)[j]);
        ss += f * f;
      }
    }
    ss = wave_reduce_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    float rnorm_a = rsqrtf(stage_red_sum(red) / (float)K + eps);
    __syncthreads();
    float ss2 = 0.f;
    for (int i = threadIdx.x * 8; i < K; i += STRIDE) {
      s8v v = *(const s8v*)(x + i);
      s8v hv = *(const s8v*)(h + i);
      f4v ga = *(const f4v*)(g + i);
      f4v gb = *(const f4v*)(g + i + 4);
      u16 o[8];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        float f = b2f(((u16*)&v)[j]) * rnorm_a * (j < 4 ? ga[j] : gb[j - 4])
                  + b2f(((u16*)&hv)[j]);
        o[j] = f2b(f);           // bf16-rounded h' (residual stream)
        float fr = b2f(o[j]);
        xs[i + j] = fr;
        ss2 += fr * fr;
      }
      if (blockIdx.x == 0) *(s8v*)(hout + i) = *(s8v*)o;
    }
    ss2 = wave_reduce_sum(ss2);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss2;
    __syncthreads();
    float rnorm_b = rsqrtf(stage_red_sum(red) / (float)K + eps);
    for (int i = threadIdx.x * 8; i < K; i += STRIDE) {
#pragma unroll
      for (int j = 0; j < 8; j++)
        xs[i + j] = xs[i + j] * rnorm_b * g2[i + j];
    }
    __syncthreads();
    return xs;
  }
  if (stage == STAGE_NORM || stage == STAGE_NORM_EMBED) {
    const u16* xsrc = x;
    if (stage == STAGE_NORM_EMBED)
      xsrc = x + (size_t)(*(const int*)x2) * (size_t)K;
    float ss = 0.f;
    for (int i = threadIdx.x * 8; i < K; i += STRIDE) {
      s8v v = *(const s8v*)(xsrc + i);
      if (stage == STAGE_NORM_EMBED) {
        u16 o[8];
#pragma unroll
        for (int j = 0; j < 8; j++)
          o[j] = f2b(b2f(((u16*)&v)[j]) * escale);
        v = *(s8v*)o;
        if (blockIdx.x == 0) *(s8v*)(hout + i) = v;
      }
#pragma unroll
      for (int j = 0; j < 8; j++) {
        float f = b2f(((u16*)&v)[j]);
        xs[i + j] = f;
        ss += f * f;
      }
    }
    ss = wave_reduce_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    float rnorm = rsqrtf(stage_red_sum(red) / (float)K + eps);
    for (int i = threadIdx.x * 8; i < K; i += STRIDE) {
#pragma unroll
      for (int j = 0; j < 8; j++) xs[i + j] *= rnorm * g[i + j];
    }
  } else if (stage == STAGE_GLU) {
    for (int i = threadIdx.x * 8; i < K; i += STRIDE) {
      s8v gv = *(const s8v*)(x + i);
      s8v uv = *(const s8v*)(x2 + i);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        float xx = b2f(((u16*)&gv)[j]);
        float a;
        if (act == 0) {
          a = xx / (1.f + __expf(-xx));
        } else {
          float c = 0.7978845608028654f * (xx + 0.044715f * xx * xx * xx);
          a = 0.5f * xx * (1.f + tanhf(c));
        }
        xs[i + j] = a * b2f(((u16*)&uv)[j]);
      }
    }
  }
  __syncthreads();
  return xs;
}

DEVINL void gemv_epilogue(float acc, int row, void* y, const u16* res,
                          int out_f32, float softcap) {
  if (softcap > 0.f) acc = softcap * tanhf(acc / softcap);
  if (res) acc += b2f(res[row]);
  if (out_f32) ((float*)y)[row] = acc;
  else ((u16*)y)[row] = f2b(acc);
}

template <bool NT>
DEVINL s8v gemv_wload(const u16* p) {
  return NT ? __builtin_nontemporal_load((const s8v*)p) : *(const s8v*)p;
}

// One grid-stride iteration's dot products: NR rows in flight against
// the staged vector; acc[r] is the lane's partial sum of row r.
// PRE: the first four 16 B chunks of each row (pw[r][q], at
// lane*8 + 512q clamped to K-8) were loaded ahead of the staging pass
// and stand in for the loads the loops would issue first — the same
// chunks into the same accumulators in the same order, so the sums are
// bit-identical with and without the prologue.
template <bool NT, int NR, bool PRE>
DEVINL void gemv_rows(const u16* (&Wr)[NR], const u16* xv, int K, int lane,
                      const s8v (&pw)[NR][4], float (&acc)[NR]) {
  float a0[NR], a1[NR], a2[NR], a3[NR];
#pragma unroll
  for (int r = 0; r < NR; r++) a0[r] = a1[r] = a2[r] = a3[r] = 0.f;
  int k = lane * 8;
  if (PRE) {
    if (k + 1536 < K) {  // the main loop's first iteration
      s8v x0 = *(const s8v*)(xv + k);
      s8v x1 = *(const s8v*)(xv + k + 512);
      s8v x2v = *(const s8v*)(xv + k + 1024);
      s8v x3 = *(const s8v*)(xv + k + 1536);
#pragma unroll
      for (int r = 0; r < NR; r++) {
        s8v w0 = pw[r][0], w1 = pw[r][1], w2 = pw[r][2], w3 = pw[r][3];
#pragma unroll
        for (int j = 0; j < 8; j++) {
          a0[r] += b2f(((u16*)&w0)[j]) * b2f(((u16*)&x0)[j]);
          a1[r] += b2f(((u16*)&w1)[j]) * b2f(((u16*)&x1)[j]);
          a2[r] += b2f(((u16*)&w2)[j]) * b2f(((u16*)&x2v)[j]);
          a3[r] += b2f(((u16*)&w3)[j]) * b2f(((u16*)&x3)[j]);
        }
      }
      k += 2048;
    } else {  // K too short for it: the tail loop's (at most 3) iterations
#pragma unroll
      for (int q = 0; q < 3; q++) {
        if (k < K) {
          s8v x0 = *(const s8v*)(xv + k);
#pragma unroll
          for (int r = 0; r < NR; r++) {
            s8v w0 = pw[r][q];
#pragma unroll
            for (int j = 0; j < 8; j++)
              a0[r] += b2f(((u16*)&w0)[j]) * b2f(((u16*)&x0)[j]);
          }
          k += 512;
        }
      }
    }
  }
  for (; k + 1536 < K; k += 2048) {
    s8v x0 = *(const s8v*)(xv + k);
    s8v x1 = *(const s8v*)(xv + k + 512);
    s8v x2v = *(const s8v*)(xv + k + 1024);
    s8v x3 = *(const s8v*)(xv + k + 1536);
#pragma unroll
    for (int r = 0; r < NR; r++) {
      s8v w0 = gemv_wload<NT>(Wr[r] + k);
      s8v w1 = gemv_wload<NT>(Wr[r] + k + 512);
      s8v w2 = gemv_wload<NT>(Wr[r] + k + 1024);
      s8v w3 = gemv_wload<NT>(Wr[r] + k + 1536);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        a0[r] += b2f(((u16*)&w0)[j]) * b2f(((u16*)&x0)[j]);
        a1[r] += b2f(((u16*)&w1)[j]) * b2f(((u16*)&x1)[j]);
        a2[r] += b2f(((u16*)&w2)[j]) * b2f(((u16*)&x2v)[j]);
        a3[r] += b2f(((u16*)&w3)[j]) * b2f(((u16*)&x3)[j]);
      }
    }
  }
  for (; k < K; k += 512) {
    s8v x0 = *(const s8v*)(xv + k);
#pragma unroll
    for (int r = 0; r < NR; r++) {
      s8v w0 = gemv_wload<NT>(Wr[r] + k);
#pragma unroll
      for (int j = 0; j < 8; j++)
        a0[r] += b2f(((u16*)&w0)[j]) * b2f(((u16*)&x0)[j]);
    }
  }
#pragma unroll
  for (int r = 0; r < NR; r++) acc[r] = (a0[r] + a1[r]) + (a2[r] + a3[r]);
}

// NT: non-temporal weight loads (read-once stream, keep L2 for x/KV —
// MI355X_MICROARCH "nt-weights").  RPW: rows per wave (ILP: RPW x 4
// weight loads in flight).
// PAIR (fused GLU, W = [2N, K] gate rows then up rows, y[N]): the wave
// that owns output n accumulates gate row n and up row n+N and writes
// act(gate)*up itself — both sums bf16-rounded first, so the bits equal
// "GEMV into 2N, then GLU".  The two rows are in flight together (RPW
// must be 2).
// Every staged launch (stage != RAW) issues the weight loads of its
// first row iteration BEFORE the staging pass's barriers (see
// gemv_stage_issue): the stream's first round trip overlaps the stage's.
// The second launch bound pins the parent kernel's occupancy (5 waves/
// SIMD at RPW 1, 4 at RPW 2): the prologue's live registers sit right at
// those VGPR boundaries, and one wave less leaves a 1024-block grid with
// a partial last round (measured 1398 -> 1320 tok/s).
template <bool NT, int RPW, bool PAIR>
__global__ void __launch_bounds__(512, RPW == 1 ? 5 : 4)
k_gemv_bf16_t(const u16* __restrict__ W, const u16* __restrict__ x,
              const u16* __restrict__ x2, const float* __restrict__ g,
              const float* __restrict__ g2, void* __restrict__ y,
              const u16* __restrict__ res, int N, int K, int stage, int act,
              float eps, int out_f32, float softcap, float escale,
              const int* __restrict__ eidx, long wstride,
              const float* __restrict__ oscale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  static_assert(!PAIR || RPW == 2, "PAIR: gate and up row in flight");
  constexpr int NR = RPW;              // rows in flight
  constexpr int OPW = PAIR ? 1 : RPW;  // outputs per wave iteration
  // MoE: expert-indexed weight base + device output scale (router
  // prob); scalar loads, uniform branch — free on the dense path
  if (eidx) W += (size_t)(*eidx) * wstride;
  const float osc = oscale ? *oscale : 1.0f;
  // NORM2 / NORM_EMBED borrow `res` as the persisted-h output
  const u16* eres = (stage == STAGE_NORM2 || stage == STAGE_NORM_EMBED)
                        ? nullptr : res;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int rstride = gridDim.x * wpb * OPW;  // grid-stride rows
  int row0 = (blockIdx.x * wpb + wave) * OPW;
  // row r of the iteration at `row`: rows row..row+RPW-1, or (PAIR)
  // gate row `row` / up row `row`+N; clamped so idle waves stay in bounds
  auto rowptr = [&](int row, int r) {
    int rr = PAIR ? row : row + r;
    rr = rr < N ? rr : N - 1;
    if (PAIR) rr += r * N;
    return W + (size_t)rr * K;
  };

  const u16* xv = x;  // RAW: L2-hot, no barrier, nothing to overlap
  s8v pw[NR][4];
  if (stage != STAGE_RAW) {
    StagePre sp;
    const u16* xsrc = x;
    gemv_stage_issue(sp, xsrc, x2, g, K, stage);
#pragma unroll
    for (int r = 0; r < NR; r++) {
      const u16* wr = rowptr(row0, r);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        int kq = lane * 8 + 512 * q;
        if (kq > K - 8) kq = K - 8;
        pw[r][q] = gemv_wload<NT>(wr + kq);
      }
    }
    xv = gemv_stage(smem, sp, xsrc, x2, g, g2, (u16*)res, K, stage, act, eps,
                    escale);
  }

  auto body = [&](auto pre, int row) {
    const u16* Wr[NR];
    float acc[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) Wr[r] = rowptr(row, r);
    gemv_rows<NT, NR, decltype(pre)::value>(Wr, xv, K, lane, pw, acc);
    if (PAIR) {
      const float ag = osc * wave_reduce_sum(acc[0]);
      const float au = osc * wave_reduce_sum(acc[NR - 1]);
      if (lane == 0 && row < N)
        ((u16*)y)[row] = glu_act(b2f(f2b(ag)), b2f(f2b(au)), act);
    } else {
#pragma unroll
      for (int r = 0; r < NR; r++) {
        float a = osc * wave_reduce_sum(acc[r]);
        if (lane == 0 && row + r < N)
          gemv_epilogue(a, row + r, y, eres, out_f32, softcap);
      }
    }
  };
  if (stage != STAGE_RAW && row0 < N) {  // consumes the prologue loads
    body(std::true_type{}, row0);
    row0 += rstride;
  }
  for (; row0 < N; row0 += rstride) body(std::false_type{}, row0);
}

// glu_pair: N counts the rows of W ([gate; up]); y gets N/2 outputs
extern "C" hipError_t launch_gemv_bf16(const void* W, const void* x,
                                       const void* x2, const void* g,
                                       const void* g2, void* y,
                                       const void* res, int N, int K,
                                       int stage, int act, float eps,
                                       int out_f32, float softcap,
                                       int nt, int rpw, int maxblocks,
                                       float escale, const void* eidx,
                                       long wstride, const void* oscale,
                                       hipStream_t stream, int glu_pair) {
  size_t lds = (stage == STAGE_RAW) ? 0 : ((size_t)K * 2 + 32);
  static int rpw_env_b = -1;
  if (rpw_env_b < 0) {
    const char* p = getenv("LLM_GEMV_RPW");
    rpw_env_b = p ? atoi(p) : 0;
  }
  if (glu_pair) {
    const bool hres = stage == STAGE_NORM2 || stage == STAGE_NORM_EMBED;
    if ((N & 1) || (res && !hres) || softcap > 0.f || out_f32 || eidx ||
        oscale || stage == STAGE_GLU)
      return hipErrorInvalidValue;
    N /= 2;
    rpw = 2;  // gate row + up row
  } else if (rpw_env_b > 0) rpw = rpw_env_b;
  else if (rpw <= 1)
    // deep-K only: the fp8 GEMV's large-N rpw rule measured NEGATIVE
    // for bf16 (1b 1234->1218, gemma-2b 536->526)
    rpw = (K >= 3584 && N >= 3072) ? 2 : 1;
  int threads = 256;  // 512 measured slower (fp8 1391->1328)
  int wpb = threads / 64;
  int opw = glu_pair ? 1 : rpw;  // outputs per wave iteration
  int blocks = (N + wpb * opw - 1) / (wpb * opw);
  int cap = maxblocks > 0 ? maxblocks : 1024;
  if (blocks > cap) blocks = cap;  // grid-stride the rest (Guideline 11)
#define GEMV_CASE(NTV, RPWV, PV)                                             \
  hipLaunchKernelGGL((k_gemv_bf16_t<NTV, RPWV, PV>), dim3(blocks),           \
                     dim3(threads),                                          \
                     lds, stream, (const u16*)W, (const u16*)x,              \
                     (const u16*)x2, (const float*)g, (const float*)g2, y,   \
                     (const u16*)res, N, K, stage, act, eps, out_f32,        \
                     softcap, escale, (const int*)eidx, wstride,             \
                     (const float*)oscale)
  if (glu_pair && nt) GEMV_CASE(true, 2, true);
  else if (glu_pair) GEMV_CASE(false, 2, true);
  else if (nt && rpw == 2) GEMV_CASE(true, 2, false);
  else if (nt) GEMV_CASE(true, 1, false);
  else if (rpw == 2) GEMV_CASE(false, 2, false);
  else GEMV_CASE(false, 1, false);
#undef GEMV_CASE
  return hipGetLastError();
}

// ====================================================================
// fp8 GEMV: y[N] = scale[n] * (W8[N,K] @ stage(x)[K]) (+res) (softcap)
// W8 = OCP e4m3fn, per-output-row scales (absmax/448 quantization at
// load).  Halves decode weight traffic vs bf16 -> ~2x decode ceiling.
// Same fused staging modes as the bf16 GEMV; x stays bf16.
// HW dequant: v_cvt_pk_f32_fp8 (gfx950, OCP not fnuz).
// ====================================================================

typedef uint32_t u4v __attribute__((ext_vector_type(4)));  // = u4v_ alias

// Inner loop is PACKED: x is staged as fp32 in LDS (gemv_stage_f32),
// each v_cvt_pk_f32_fp8 output pair feeds one v_pk_fma_f32 against an
// LDS fp32 pair — ~16 VALU per 16 weight bytes vs ~40 for the round-1
// scalar form (the fp8 stream was conversion-bound at 4.3 TB/s while
// bf16 hit 6.4; see profiles/decode_kernels_r01.md).
template <bool NT, int RPW, bool XDIR>
__global__ void __launch_bounds__(512)
k_gemv_fp8_t(const uint8_t* __restrict__ W, const float* __restrict__ scales,
             const u16* __restrict__ x, const u16* __restrict__ x2,
             const float* __restrict__ g, const float* __restrict__ g2,
             void* __restrict__ y, const u16* __restrict__ res, int N, int K,
             int stage, int act, float eps, int out_f32, float softcap,
             float escale, const int* __restrict__ eidx, long wstride,
             long sstride, const float* __restrict__ oscale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // XDIR (RAW stage only): x read from global per row iteration — the
  // f32 LDS staging pass costs ~2K B of LDS+global traffic per BLOCK,
  // which rivals the weight bytes when a block covers only a few rows
  // (N~3.5k o/down projections; see profiles/decode_kernels_r02.md)
  const float* xv = XDIR ? nullptr
                         : gemv_stage_f32(smem, x, x2, g, g2, (u16*)res, K,
                                          stage, act, eps, escale);
  const u16* eres = (stage == STAGE_NORM2 || stage == STAGE_NORM_EMBED)
                        ? nullptr : res;
  // MoE: expert-indexed weight/scale base + device output scale
  if (eidx) {
    W += (size_t)(*eidx) * wstride;
    scales += (size_t)(*eidx) * sstride;
  }
  const float osc = oscale ? *oscale : 1.0f;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int rstride = gridDim.x * wpb * RPW;
  for (int row0 = (blockIdx.x * wpb + wave) * RPW; row0 < N;
       row0 += rstride) {
  const uint8_t* Wr[RPW];
  f2v a0[RPW], a1[RPW];
#pragma unroll
  for (int r = 0; r < RPW; r++) {
    int rr = row0 + r < N ? row0 + r : N - 1;
    Wr[r] = W + (size_t)rr * K;
    a0[r] = (f2v){0.f, 0.f};
    a1[r] = (f2v){0.f, 0.f};
  }
  int k = lane * 16;
  for (; k + 1024 + 16 <= K; k += 2048) {
    s8v xda, xdb, xdc, xdd;
    if (XDIR) {
      xda = *(const s8v*)(x + k); xdb = *(const s8v*)(x + k + 8);
      xdc = *(const s8v*)(x + k + 1024); xdd = *(const s8v*)(x + k + 1032);
    }
#pragma unroll
    for (int r = 0; r < RPW; r++) {
      u4v w0 = NT ? __builtin_nontemporal_load((const u4v*)(Wr[r] + k))
                  : *(const u4v*)(Wr[r] + k);
      u4v w1 = NT ? __builtin_nontemporal_load((const u4v*)(Wr[r] + k + 1024))
                  : *(const u4v*)(Wr[r] + k + 1024);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        f2v ca = __builtin_amdgcn_cvt_pk_f32_fp8(w0[q], false);
        f2v cb = __builtin_amdgcn_cvt_pk_f32_fp8(w0[q], true);
        f2v xa, xb, xc, xd;
        if (XDIR) {
          const u16* p0 = (q < 2) ? (const u16*)&xda : (const u16*)&xdb;
          const int o0 = (q & 1) * 4;
          xa = (f2v){b2f(p0[o0]), b2f(p0[o0 + 1])};
          xb = (f2v){b2f(p0[o0 + 2]), b2f(p0[o0 + 3])};
          const u16* p1 = (q < 2) ? (const u16*)&xdc : (const u16*)&xdd;
          xc = (f2v){b2f(p1[o0]), b2f(p1[o0 + 1])};
          xd = (f2v){b2f(p1[o0 + 2]), b2f(p1[o0 + 3])};
        } else {
          xa = *(const f2v*)(xv + k + q * 4);
          xb = *(const f2v*)(xv + k + q * 4 + 2);
          xc = *(const f2v*)(xv + k + 1024 + q * 4);
          xd = *(const f2v*)(xv + k + 1024 + q * 4 + 2);
        }
        a0[r] += ca * xa;
        a1[r] += cb * xb;
        f2v da = __builtin_amdgcn_cvt_pk_f32_fp8(w1[q], false);
        f2v db = __builtin_amdgcn_cvt_pk_f32_fp8(w1[q], true);
        a0[r] += da * xc;
        a1[r] += db * xd;
      }
    }
  }
  for (; k < K; k += 1024) {
    s8v xda, xdb;
    if (XDIR) {
      xda = *(const s8v*)(x + k); xdb = *(const s8v*)(x + k + 8);
    }
#pragma unroll
    for (int r = 0; r < RPW; r++) {
      u4v w0 = NT ? __builtin_nontemporal_load((const u4v*)(Wr[r] + k))
                  : *(const u4v*)(Wr[r] + k);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        f2v ca = __builtin_amdgcn_cvt_pk_f32_fp8(w0[q], false);
        f2v cb = __builtin_amdgcn_cvt_pk_f32_fp8(w0[q], true);
        f2v xa, xb;
        if (XDIR) {
          const u16* p0 = (q < 2) ? (const u16*)&xda : (const u16*)&xdb;
          const int o0 = (q & 1) * 4;
          xa = (f2v){b2f(p0[o0]), b2f(p0[o0 + 1])};
          xb = (f2v){b2f(p0[o0 + 2]), b2f(p0[o0 + 3])};
        } else {
          xa = *(const f2v*)(xv + k + q * 4);
          xb = *(const f2v*)(xv + k + q * 4 + 2);
        }
        a0[r] += ca * xa;
        a1[r] += cb * xb;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RPW; r++) {
    int rr = row0 + r < N ? row0 + r : N - 1;
    f2v s = a0[r] + a1[r];
    float acc = osc * wave_reduce_sum(s[0] + s[1]) * scales[rr];
    if (lane == 0 && row0 + r < N)
      gemv_epilogue(acc, row0 + r, y, eres, out_f32, softcap);
  }
  }  // row0 grid-stride loop
}

extern "C" hipError_t launch_gemv_fp8(const void* W, const void* scales,
                                      const void* x, const void* x2,
                                      const void* g, const void* g2, void* y,
                                      const void* res, int N, int K,
                                      int stage, int act, float eps,
                                      int out_f32, float softcap, int nt,
                                      int rpw, int maxblocks, float escale,
                                      const void* eidx, long wstride,
                                      long sstride, const void* oscale,
                                      hipStream_t stream) {
  static int xdir_raw = -1, rows_min = -1, rpw_env = -1;
  if (xdir_raw < 0) {
    const char* e = getenv("LLM_GEMV_XDIR");
    xdir_raw = e ? atoi(e) : 1;          // default ON for RAW stage
    const char* r = getenv("LLM_GEMV_ROWSMIN");
    rows_min = r ? atoi(r) : 1;
    const char* p = getenv("LLM_GEMV_RPW");
    rpw_env = p ? atoi(p) : 0;
  }
  if (rpw_env > 0) rpw = rpw_env;
  else if (rpw <= 1)
    // deep-K rows: 2x loads in flight (gemma-9b 240->300, llama-8b
    // 393->442, qwen-7b 352->442); N floor keeps small-N shapes (1B
    // down-proj) at full block count.  Very large N (gate+up, lm_head)
    // also gains: waves already grid-stride many rows, RPW doubles the
    // in-flight rows per iteration.
    rpw = ((K >= 3584 && N >= 3072) || N >= 12288) ? 2 : 1;
  const int xdir = (stage == STAGE_RAW) && xdir_raw;
  // fp32 staging for packed math (all non-RAW stages; RAW reads direct)
  size_t lds = xdir ? 0 : ((size_t)K * 4 + 32);
  if (lds > 65536) {
    // gfx950 allows up to 160 KB dynamic LDS with an explicit opt-in
    // (e.g. Gemma-27B down-proj K=36864)
    static bool raised = false;
    if (!raised) {
#define GEMV8_RAISE(NTV, RPWV)                                              \
      hipFuncSetAttribute((const void*)&k_gemv_fp8_t<NTV, RPWV, false>,     \
                          hipFuncAttributeMaxDynamicSharedMemorySize,       \
                          160 * 1024)
      GEMV8_RAISE(true, 1); GEMV8_RAISE(true, 2);
      GEMV8_RAISE(false, 1); GEMV8_RAISE(false, 2);
#undef GEMV8_RAISE
      raised = true;
    }
  }
  int threads = 256;  // 512 measured slower (fp8 1391->1328)
  int wpb = threads / 64;
  int blocks = (N + wpb * rpw - 1) / (wpb * rpw);
  int cap = maxblocks > 0 ? maxblocks : 1024;
  if (rows_min > 1 && !xdir) {
    // amortize the staging pass over >= rows_min rows per wave
    int cap2 = N / (wpb * rpw * rows_min);
    if (cap2 < 64) cap2 = 64;
    if (cap > cap2) cap = cap2;
  }
  if (blocks > cap) blocks = cap;
#define GEMV8_CASE(NTV, RPWV, XD)                                           \
  hipLaunchKernelGGL((k_gemv_fp8_t<NTV, RPWV, XD>), dim3(blocks),           \
                     dim3(threads),                                         \
                     lds, stream, (const uint8_t*)W, (const float*)scales,  \
                     (const u16*)x, (const u16*)x2, (const float*)g,        \
                     (const float*)g2, y, (const u16*)res, N, K, stage,     \
                     act, eps, out_f32, softcap, escale, (const int*)eidx,  \
                     wstride, sstride, (const float*)oscale)
  if (xdir) {
    if (nt && rpw == 4) GEMV8_CASE(true, 4, true);
    else if (nt && rpw == 2) GEMV8_CASE(true, 2, true);
    else if (nt) GEMV8_CASE(true, 1, true);
    else if (rpw == 4) GEMV8_CASE(false, 4, true);
    else if (rpw == 2) GEMV8_CASE(false, 2, true);
    else GEMV8_CASE(false, 1, true);
  } else {
    if (nt && rpw == 4) GEMV8_CASE(true, 4, false);
    else if (nt && rpw == 2) GEMV8_CASE(true, 2, false);
    else if (nt) GEMV8_CASE(true, 1, false);
    else if (rpw == 4) GEMV8_CASE(false, 4, false);
    else if (rpw == 2) GEMV8_CASE(false, 2, false);
    else GEMV8_CASE(false, 1, false);
  }
#undef GEMV8_CASE
  return hipGetLastError();
}

// ====================================================================
// Multi-x fp8 GEMV (batched decode, B = 2..8 lockstep sequences):
// ONE non-temporal weight stream feeds B accumulators — weight reuse
// turns B-way decode into ~single-sequence step time (the 128-row MFMA
// GEMM path wastes >90% of each tile at B<=8).  All staging modes of
// the single-x GEMV, applied per row; XF32 stages fp32 pairs for
// v_pk_fma_f32 (LDS B*K*4), falling back to bf16 staging (B*K*2) for
// deep-K shapes.  BT = compile-time row capacity (2/4/8); the actual
// B <= BT, with clamped source rows.
// ====================================================================

// per-row staging into xs + b*K (f32 or bf16 element type)
template <bool XF32>
DEVINL void gemv_stage_mx_row(char* smem, int b, const u16* xb,
                              const u16* x2b, const float* g,
                              const float* g2, u16* houtb, int K, int BT,
                              int stage, int act, float eps, float escale,
                              float* red, bool persist) {
  const int STRIDE = blockDim.x * 8;
  float* xf = (float*)smem + (size_t)b * K;
  u16* xh = (u16*)smem + (size_t)b * K;
#define MXSTORE(i, v) do { if (XF32) xf[i] = (v); else xh[i] = f2b(v); } while (0)
  if (stage == STAGE_RAW || stage == STAGE_NORM ||
      stage == STAGE_NORM_EMBED) {
    float ss = 0.f;
    for (int i = threadIdx.x * 8; i < K; i += STRIDE) {
      s8v v = *(const s8v*)(xb + i);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        float f = b2f(((u16*)&v)[j]);
        if (stage == STAGE_NORM_EMBED) {
          f = b2f(f2b(f * escale));
          if (persist) houtb[i + j] = f2b(f);
        }
        MXSTORE(i + j, f);
        ss += f * f;
      }
    }
    if (stage == STAGE_RAW) return;
    ss = wave_reduce_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    float rnorm = rsqrtf(stage_red_sum(red) / (float)K + eps);
    __syncthreads();  // red reused by the next row's reduction
    for (int i = threadIdx.x * 8; i < K; i += STRIDE) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        float f = (XF32 ? xf[i + j] : b2f(xh[i + j])) * rnorm * g[i + j];
        MXSTORE(i + j, f);
      }
    }
  } else if (stage == STAGE_GLU) {
    for (int i = threadIdx.x * 8; i < K; i += STRIDE) {
      s8v gv = *(const s8v*)(xb + i);
      s8v uv = *(const s8v*)(x2b + i);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        float xx = b2f(((u16*)&gv)[j]);
        float a;
        if (act == 0) {
          a = xx / (1.f + __expf(-xx));
        } else {
          float c = 0.7978845608028654f * (xx + 0.044715f * xx * xx * xx);
          a = 0.5f * xx * (1.f + tanhf(c));
        }
        MXSTORE(i + j, a * b2f(((u16*)&uv)[j]));
      }
    }
  } else if (stage == STAGE_NORM2) {
    const u16* h = x2b;
    float ss = 0.f;
    for (int i = threadIdx.x * 8; i < K; i += STRIDE) {
      s8v v = *(const s8v*)(xb + i);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        float f = b2f(((u16*)&v)[j]);
        ss += f * f;
      }
    }
    ss = wave_reduce_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    float rnorm_a = rsqrtf(stage_red_sum(red) / (float)K + eps);
    __syncthreads();
    float ss2 = 0.f;
    for (int i = threadIdx.x * 8; i < K; i += STRIDE) {
      s8v v = *(const s8v*)(xb + i);
      s8v hv = *(const s8v*)(h + i);
      f4v ga = *(const f4v*)(g + i);
      f4v gb = *(const f4v*)(g + i + 4);
      u16 o[8];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        float f = b2f(((u16*)&v)[j]) * rnorm_a * (j < 4 ? ga[j] : gb[j - 4])
                  + b2f(((u16*)&hv)[j]);
        o[j] = f2b(f);
        float fr = b2f(o[j]);
        MXSTORE(i + j, fr);
        ss2 += fr * fr;
      }
      if (persist) *(s8v*)(houtb + i) = *(s8v*)o;
    }
    ss2 = wave_reduce_sum(ss2);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss2;
    __syncthreads();
    float rnorm_b = rsqrtf(stage_red_sum(red) / (float)K + eps);
    __syncthreads();
    for (int i = threadIdx.x * 8; i < K; i += STRIDE) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        float f = (XF32 ? xf[i + j] : b2f(xh[i + j])) * rnorm_b * g2[i + j];
        MXSTORE(i + j, f);
      }
    }
  }
#undef MXSTORE
}

template <int BT, bool XF32>
__global__ void __launch_bounds__(256)
k_gemv_fp8_mx(const uint8_t* __restrict__ W,
              const float* __restrict__ scales, const u16* __restrict__ x,
              long xstride, const u16* __restrict__ x2, long x2stride,
              const float* __restrict__ g, const float* __restrict__ g2,
              void* __restrict__ y, long ystride,
              const u16* __restrict__ res, long rstride,
              u16* __restrict__ hout, long hstride, int N, int K, int B,
              int stage, int act, float eps, int out_f32, float softcap,
              float escale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = (float*)(smem + (size_t)BT * K * (XF32 ? 4 : 2));
  for (int b = 0; b < BT; b++) {
    int bs = b < B ? b : B - 1;  // clamp padded rows to a valid source
    const u16* xb = x + (size_t)bs * xstride;
    if (stage == STAGE_NORM_EMBED)  // x = table, x2 = per-row token ids
      xb = x + (size_t)((const int*)x2)[bs] * (size_t)K;
    const u16* x2b = (stage == STAGE_NORM_EMBED || x2 == nullptr)
                         ? nullptr : x2 + (size_t)bs * x2stride;
    u16* houtb = hout ? hout + (size_t)bs * hstride : nullptr;
    __syncthreads();
    gemv_stage_mx_row<XF32>(smem, b, xb, x2b, g, g2, houtb, K, BT, stage,
                            act, eps, escale, red, blockIdx.x == 0);
  }
  __syncthreads();

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const float* xsf = (const float*)smem;
  const u16* xsh = (const u16*)smem;
  for (int row = blockIdx.x * wpb + wave; row < N; row += gridDim.x * wpb) {
    const uint8_t* Wr = W + (size_t)row * K;
    f2v a0[BT], a1[BT];
#pragma unroll
    for (int b = 0; b < BT; b++) {
      a0[b] = (f2v){0.f, 0.f};
      a1[b] = (f2v){0.f, 0.f};
    }
    for (int k = lane * 16; k < K; k += 1024) {
      u4v w0 = __builtin_nontemporal_load((const u4v*)(Wr + k));
#pragma unroll
      for (int q = 0; q < 4; q++) {
        f2v ca = __builtin_amdgcn_cvt_pk_f32_fp8(w0[q], false);
        f2v cb = __builtin_amdgcn_cvt_pk_f32_fp8(w0[q], true);
#pragma unroll
        for (int b = 0; b < BT; b++) {
          f2v xa, xb2;
          if (XF32) {
            xa = *(const f2v*)(xsf + (size_t)b * K + k + q * 4);
            xb2 = *(const f2v*)(xsf + (size_t)b * K + k + q * 4 + 2);
          } else {
            const u16* p = xsh + (size_t)b * K + k + q * 4;
            xa = (f2v){b2f(p[0]), b2f(p[1])};
            xb2 = (f2v){b2f(p[2]), b2f(p[3])};
          }
          a0[b] += ca * xa;
          a1[b] += cb * xb2;
        }
      }
    }
    const float sc = scales[row];
#pragma unroll
    for (int b = 0; b < BT; b++) {
      f2v s = a0[b] + a1[b];
      float acc = wave_reduce_sum(s[0] + s[1]) * sc;
      if (lane == 0 && b < B) {
        if (softcap > 0.f) acc = softcap * tanhf(acc / softcap);
        if (res && stage != STAGE_NORM2 && stage != STAGE_NORM_EMBED)
          acc += b2f(res[(size_t)b * rstride + row]);
        if (out_f32) ((float*)y)[(size_t)b * ystride + row] = acc;
        else ((u16*)y)[(size_t)b * ystride + row] = f2b(acc);
      }
    }
  }
}

extern "C" hipError_t launch_gemv_fp8_mx(
    const void* W, const void* scales, const void* x, long xstride,
    const void* x2, long x2stride, const void* g, const void* g2, void* y,
    long ystride, const void* res, long rstride, void* hout, long hstride,
    int N, int K, int B, int stage, int act, float eps, int out_f32,
    float softcap, float escale, hipStream_t stream) {
  if (B < 1 || B > 8 || K % 16 != 0) return hipErrorInvalidValue;
  int BT = B <= 2 ? 2 : (B <= 4 ? 4 : 8);
  bool xf32 = ((size_t)BT * K * 4 + 64) <= 128 * 1024;
  size_t lds = (size_t)BT * K * (xf32 ? 4 : 2) + 64;
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  static bool raised = false;
  if (lds > 65536 && !raised) {
#define MXRAISE(BTV, XFV)                                                   \
    hipFuncSetAttribute((const void*)&k_gemv_fp8_mx<BTV, XFV>,              \
                        hipFuncAttributeMaxDynamicSharedMemorySize,         \
                        160 * 1024)
    MXRAISE(2, true); MXRAISE(2, false);
    MXRAISE(4, true); MXRAISE(4, false);
    MXRAISE(8, true); MXRAISE(8, false);
#undef MXRAISE
    raised = true;
  }
  int threads = 256;
  int wpb = threads / 64;
  int blocks = (N + wpb - 1) / wpb;
  if (blocks > 1024) blocks = 1024;
#define MX_CASE(BTV, XFV)                                                   \
  hipLaunchKernelGGL((k_gemv_fp8_mx<BTV, XFV>), dim3(blocks),               \
                     dim3(threads), lds, stream, (const uint8_t*)W,         \
                     (const float*)scales, (const u16*)x, xstride,          \
                     (const u16*)x2, x2stride, (const float*)g,             \
                     (const float*)g2, y, ystride, (const u16*)res,         \
                     rstride, (u16*)hout, hstride, N, K, B, stage, act,     \
                     eps, out_f32, softcap, escale)
  if (BT == 2) { if (xf32) MX_CASE(2, true); else MX_CASE(2, false); }
  else if (BT == 4) { if (xf32) MX_CASE(4, true); else MX_CASE(4, false); }
  else { if (xf32) MX_CASE(8, true); else MX_CASE(8, false); }
#undef MX_CASE
  return hipGetLastError();
}

// ====================================================================
// Skinny fp8 MFMA GEMM pair (batched decode, B = 3..16): matrix cores
// own the MACs — the multi-x GEMV above is VALU-ISSUE-bound beyond B=2
// (64 irreducible v_pk_fma per 16 weight bytes at B=8).
//   1. k_stage_quant_mx: per sequence row, apply the staging op
//      (RAW/NORM/GLU/NORM2/NORM_EMBED) and quantize to e4m3 + scale
//      (one block per row; row stats need full-K visibility).
//   2. k_gemm_fp8_skinny: Y[B,N] = (sx_b*sw_n) * Xq[B,K] @ Wq[N,K]^T
//      with ONE 16-row mfma_f32_16x16x32_fp8_fp8 tile per wave — W is
//      nt-streamed exactly once; Xq re-reads stay L2-hot (~N*K/4 B).
// ====================================================================

extern "C" __global__ void k_zero_f32(float* p, long total);

extern "C" __global__ void __launch_bounds__(256)
k_stage_quant_mx(const u16* __restrict__ x, long xstride,
                 const u16* __restrict__ x2, long x2stride,
                 const float* __restrict__ g, const float* __restrict__ g2,
                 uint8_t* __restrict__ xq, float* __restrict__ sx,
                 u16* __restrict__ hout, long hstride, int K, int B,
                 int stage, int act, float eps, float escale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = (float*)(smem + (size_t)K * 4);
  const int b = blockIdx.x;
  const u16* xb = x + (size_t)b * xstride;
  if (stage == STAGE_NORM_EMBED)
    xb = x + (size_t)((const int*)x2)[b] * (size_t)K;
  const u16* x2b = (stage == STAGE_NORM_EMBED || x2 == nullptr)
                       ? nullptr : x2 + (size_t)b * x2stride;
  u16* houtb = hout ? hout + (size_t)b * hstride : nullptr;
  // stage into f32 LDS (row stats via the shared per-row helper)
  gemv_stage_mx_row<true>(smem, 0, xb, x2b, g, g2, houtb, K, 1, stage,
                          act, eps, escale, red, true);
  __syncthreads();
  // absmax -> scale -> quantize to global
  const float* xf = (const float*)smem;
  float am = 0.f;
  for (int i = threadIdx.x; i < K; i += 256) am = fmaxf(am, fabsf(xf[i]));
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) am = fmaxf(am, __shfl_xor(am, w));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = am;
  __syncthreads();
  am = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sc = fmaxf(am, 1e-8f) / 448.0f;
  if (threadIdx.x == 0) sx[b] = sc;
  const float rs = 1.0f / sc;
  uint8_t* q = xq + (size_t)b * K;
  for (int i = threadIdx.x * 8; i < K; i += 2048) {
    uint32_t lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(xf[i] * rs, xf[i + 1] * rs, lo,
                                         false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(xf[i + 2] * rs, xf[i + 3] * rs,
                                         lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(xf[i + 4] * rs, xf[i + 5] * rs,
                                         hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(xf[i + 6] * rs, xf[i + 7] * rs,
                                         hi, true);
    *(uint32_t*)(q + i) = lo;
    *(uint32_t*)(q + i + 4) = hi;
  }
}

extern "C" hipError_t launch_stage_quant_mx(
    const void* x, long xstride, const void* x2, long x2stride,
    const void* g, const void* g2, void* xq, void* sx, void* hout,
    long hstride, int K, int B, int stage, int act, float eps,
    float escale, hipStream_t stream) {
  size_t lds = (size_t)K * 4 + 64;
  if (lds > 160 * 1024 || K % 16 != 0) return hipErrorInvalidValue;
  static bool raised = false;
  if (lds > 65536 && !raised) {
    hipFuncSetAttribute((const void*)&k_stage_quant_mx,
                        hipFuncAttributeMaxDynamicSharedMemorySize,
                        160 * 1024);
    raised = true;
  }
  hipLaunchKernelGGL(k_stage_quant_mx, dim3(B), dim3(256), lds, stream,
                     (const u16*)x, xstride, (const u16*)x2, x2stride,
                     (const float*)g, (const float*)g2, (uint8_t*)xq,
                     (float*)sx, (u16*)hout, hstride, K, B, stage, act,
                     eps, escale);
  return hipGetLastError();
}

// one 16x16 output tile per wave; acc row = X row (B dim), col = W row.
// TWO interleaved 64-byte K-chains per wave (independent mfma
// accumulators — the dependent-chain latency was the v1 bound) and a
// K-split grid.y for small-N occupancy (atomicAdd into an fp32 accbuf,
// scales/epilogue applied by k_skinny_fin).
extern "C" __global__ void __launch_bounds__(256)
k_gemm_fp8_skinny(const uint8_t* __restrict__ Xq,
                  const float* __restrict__ sx,
                  const uint8_t* __restrict__ Wq,
                  const float* __restrict__ sw, void* __restrict__ y,
                  long ystride, const u16* __restrict__ res, long rstride,
                  const u16* __restrict__ bias, float* __restrict__ accbuf,
                  int out_f32, float softcap, int B, int N, int K) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int fr = lane & 15, fk8 = (lane >> 4) * 8;
  const int asrc = fr < B ? fr : 0;  // padded A rows read row 0
  const uint8_t* Xr = Xq + (size_t)asrc * K + fk8;
  const int SK = gridDim.y;
  const int kchunks = (K / 32 + SK - 1) / SK;
  const int k_lo = blockIdx.y * kchunks * 32;
  int k_hi = k_lo + kchunks * 32;
  if (k_hi > K) k_hi = K;
  if (k_hi <= k_lo) return;
  for (int n0 = (blockIdx.x * 4 + wave) * 16; n0 < N;
       n0 += gridDim.x * 4 * 16) {
    int wr = n0 + fr;
    if (wr >= N) wr = N - 1;
    const uint8_t* Wr = Wq + (size_t)wr * K + fk8;
    f4v acc_a = {0.f, 0.f, 0.f, 0.f};
    f4v acc_b = {0.f, 0.f, 0.f, 0.f};
    f4v acc_c = {0.f, 0.f, 0.f, 0.f};
    f4v acc_d = {0.f, 0.f, 0.f, 0.f};
    int k = k_lo;
    // 4 independent chains x 256 B: PMC showed waves PARKED on memory
    // 69% of cycles with only 2 chains in flight
    for (; k + 256 <= k_hi; k += 256) {
      long a0 = *(const long*)(Xr + k);
      long b0 = __builtin_nontemporal_load((const long*)(Wr + k));
      long a1 = *(const long*)(Xr + k + 32);
      long b1 = __builtin_nontemporal_load((const long*)(Wr + k + 32));
      long a2 = *(const long*)(Xr + k + 64);
      long b2 = __builtin_nontemporal_load((const long*)(Wr + k + 64));
      long a3 = *(const long*)(Xr + k + 96);
      long b3 = __builtin_nontemporal_load((const long*)(Wr + k + 96));
      long a4 = *(const long*)(Xr + k + 128);
      long b4 = __builtin_nontemporal_load((const long*)(Wr + k + 128));
      long a5 = *(const long*)(Xr + k + 160);
      long b5 = __builtin_nontemporal_load((const long*)(Wr + k + 160));
      long a6 = *(const long*)(Xr + k + 192);
      long b6 = __builtin_nontemporal_load((const long*)(Wr + k + 192));
      long a7 = *(const long*)(Xr + k + 224);
      long b7 = __builtin_nontemporal_load((const long*)(Wr + k + 224));
      acc_a = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a0, b0, acc_a,
                                                         0, 0, 0);
      acc_b = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a1, b1, acc_b,
                                                         0, 0, 0);
      acc_c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a2, b2, acc_c,
                                                         0, 0, 0);
      acc_d = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a3, b3, acc_d,
                                                         0, 0, 0);
      acc_a = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a4, b4, acc_a,
                                                         0, 0, 0);
      acc_b = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a5, b5, acc_b,
                                                         0, 0, 0);
      acc_c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a6, b6, acc_c,
                                                         0, 0, 0);
      acc_d = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a7, b7, acc_d,
                                                         0, 0, 0);
    }
    for (; k < k_hi; k += 32) {
      long a0 = *(const long*)(Xr + k);
      long b0 = __builtin_nontemporal_load((const long*)(Wr + k));
      acc_a = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a0, b0, acc_a,
                                                         0, 0, 0);
    }
    const int col = n0 + fr;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int b = (lane >> 4) * 4 + r;
      if (b < B && col < N) {
        float v = (acc_a[r] + acc_b[r]) + (acc_c[r] + acc_d[r]);
        if (SK > 1) {
          atomicAdd(accbuf + (size_t)b * N + col, v);
        } else {
          v *= sx[b] * sw[col];
          if (softcap > 0.f) v = softcap * tanhf(v / softcap);
          if (bias) v += b2f(bias[col]);
          if (res) v += b2f(res[(size_t)b * rstride + col]);
          if (out_f32) ((float*)y)[(size_t)b * ystride + col] = v;
          else ((u16*)y)[(size_t)b * ystride + col] = f2b(v);
        }
      }
    }
  }
}

// SK>1 epilogue: raw sums -> scales/softcap/bias/res -> y
extern "C" __global__ void __launch_bounds__(256)
k_skinny_fin(const float* __restrict__ accbuf, const float* __restrict__ sx,
             const float* __restrict__ sw, void* __restrict__ y,
             long ystride, const u16* __restrict__ res, long rstride,
             const u16* __restrict__ bias, int out_f32, float softcap,
             int B, int N) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * N) return;
  const int b = (int)(i / N), col = (int)(i % N);
  float v = accbuf[(size_t)b * N + col] * sx[b] * sw[col];
  if (softcap > 0.f) v = softcap * tanhf(v / softcap);
  if (bias) v += b2f(bias[col]);
  if (res) v += b2f(res[(size_t)b * rstride + col]);
  if (out_f32) ((float*)y)[(size_t)b * ystride + col] = v;
  else ((u16*)y)[(size_t)b * ystride + col] = f2b(v);
}

extern "C" hipError_t launch_gemm_fp8_skinny(
    const void* Xq, const void* sx, const void* Wq, const void* sw,
    void* y, long ystride, const void* res, long rstride, const void* bias,
    void* accbuf, int out_f32, float softcap, int B, int N, int K,
    hipStream_t stream) {
  if (B < 1 || B > 16 || K % 32 != 0) return hipErrorInvalidValue;
  int blocks = (N + 63) / 64;
  if (blocks > 1024) blocks = 1024;
  int sk = 1;
  if (accbuf && blocks < 512) {
    sk = 512 / blocks;
    if (sk > 8) sk = 8;
    while (sk > 1 && K / 32 < sk) sk--;
  }
  if (sk > 1) {
    long total = (long)B * N;
    hipLaunchKernelGGL(k_zero_f32, dim3((uint32_t)((total + 1023) / 1024)),
                       dim3(256), 0, stream, (float*)accbuf, total);
  }
  hipLaunchKernelGGL(k_gemm_fp8_skinny, dim3(blocks, sk), dim3(256), 0,
                     stream, (const uint8_t*)Xq, (const float*)sx,
                     (const uint8_t*)Wq, (const float*)sw, y, ystride,
                     (const u16*)res, rstride, (const u16*)bias,
                     (float*)accbuf, out_f32, softcap, B, N, K);
  if (sk > 1) {
    long total = (long)B * N;
    hipLaunchKernelGGL(k_skinny_fin, dim3((uint32_t)((total + 255) / 256)),
                       dim3(256), 0, stream, (const float*)accbuf,
                       (const float*)sx, (const float*)sw, y, ystride,
                       (const u16*)res, rstride, (const u16*)bias, out_f32,
                       softcap, B, N);
  }
  return hipGetLastError();
}

// ====================================================================
// MXFP4 GEMV: y[N] = W4[N,K] @ stage(x)[K] (+res); 2 fp4/byte with one
// e8m0 scale per 32 elements.  Same packed structure as the fp8 GEMV
// (fp32 x staging or XDIR direct reads feeding v_pk_fma_f32) — the
// block scale rides inside v_cvt_scalef32_pk_f32_fp4, so per-ELEMENT
// VALU matches fp8 at HALF the weight bytes.
// ====================================================================

typedef uint32_t u2v_ __attribute__((ext_vector_type(2)));

DEVINL void fp4x8_to_f32p(uint32_t dw, float sc, f2v* o) {
  o[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(dw, sc, 0);
  o[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(dw, sc, 1);
  o[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(dw, sc, 2);
  o[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(dw, sc, 3);
}

template <bool NT, int RPW, bool XDIR>
__global__ void __launch_bounds__(512)
k_gemv_fp4_t(const uint8_t* __restrict__ W, const uint8_t* __restrict__ E,
             const u16* __restrict__ x, const u16* __restrict__ x2,
             const float* __restrict__ g, const float* __restrict__ g2,
             void* __restrict__ y, const u16* __restrict__ res, int N, int K,
             int stage, int act, float eps, int out_f32, float softcap,
             float escale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const float* xv = XDIR ? nullptr
                         : gemv_stage_f32(smem, x, x2, g, g2, (u16*)res, K,
                                          stage, act, eps, escale);
  const u16* eres = (stage == STAGE_NORM2 || stage == STAGE_NORM_EMBED)
                        ? nullptr : res;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int rstride = gridDim.x * wpb * RPW;
  const int K2 = K / 2, K32 = K / 32;
  for (int row0 = (blockIdx.x * wpb + wave) * RPW; row0 < N;
       row0 += rstride) {
  const uint8_t* Wr[RPW];
  const uint8_t* Er[RPW];
  f2v a0[RPW], a1[RPW];
#pragma unroll
  for (int r = 0; r < RPW; r++) {
    int rr = row0 + r < N ? row0 + r : N - 1;
    Wr[r] = W + (size_t)rr * K2;
    Er[r] = E + (size_t)rr * K32;
    a0[r] = (f2v){0.f, 0.f};
    a1[r] = (f2v){0.f, 0.f};
  }
  int k = lane * 16;
  for (; k + 1024 + 16 <= K; k += 2048) {
    s8v xda, xdb, xdc, xdd;
    if (XDIR) {
      xda = *(const s8v*)(x + k); xdb = *(const s8v*)(x + k + 8);
      xdc = *(const s8v*)(x + k + 1024); xdd = *(const s8v*)(x + k + 1032);
    }
#pragma unroll
    for (int r = 0; r < RPW; r++) {
      u2v_ w0 = NT ? __builtin_nontemporal_load((const u2v_*)(Wr[r] + k / 2))
                    : *(const u2v_*)(Wr[r] + k / 2);
      u2v_ w1 = NT ? __builtin_nontemporal_load(
                          (const u2v_*)(Wr[r] + (k + 1024) / 2))
                    : *(const u2v_*)(Wr[r] + (k + 1024) / 2);
      union { float f; uint32_t u; } s0, s1;
      s0.u = (uint32_t)Er[r][k / 32] << 23;
      s1.u = (uint32_t)Er[r][(k + 1024) / 32] << 23;
      f2v c0[8], c1[8];
      fp4x8_to_f32p(w0[0], s0.f, c0);
      fp4x8_to_f32p(w0[1], s0.f, c0 + 4);
      fp4x8_to_f32p(w1[0], s1.f, c1);
      fp4x8_to_f32p(w1[1], s1.f, c1 + 4);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        f2v ca = c0[q * 2];
        f2v cb = c0[q * 2 + 1];
        f2v xa, xb, xc, xd;
        if (XDIR) {
          const u16* p0 = (q < 2) ? (const u16*)&xda : (const u16*)&xdb;
          const int o0 = (q & 1) * 4;
          xa = (f2v){b2f(p0[o0]), b2f(p0[o0 + 1])};
          xb = (f2v){b2f(p0[o0 + 2]), b2f(p0[o0 + 3])};
          const u16* p1 = (q < 2) ? (const u16*)&xdc : (const u16*)&xdd;
          xc = (f2v){b2f(p1[o0]), b2f(p1[o0 + 1])};
          xd = (f2v){b2f(p1[o0 + 2]), b2f(p1[o0 + 3])};
        } else {
          xa = *(const f2v*)(xv + k + q * 4);
          xb = *(const f2v*)(xv + k + q * 4 + 2);
          xc = *(const f2v*)(xv + k + 1024 + q * 4);
          xd = *(const f2v*)(xv + k + 1024 + q * 4 + 2);
        }
        a0[r] += ca * xa;
        a1[r] += cb * xb;
        a0[r] += c1[q * 2] * xc;
        a1[r] += c1[q * 2 + 1] * xd;
      }
    }
  }
  for (; k < K; k += 1024) {
    s8v xda, xdb;
    if (XDIR) {
      xda = *(const s8v*)(x + k); xdb = *(const s8v*)(x + k + 8);
    }
#pragma unroll
    for (int r = 0; r < RPW; r++) {
      u2v_ w0 = NT ? __builtin_nontemporal_load((const u2v_*)(Wr[r] + k / 2))
                    : *(const u2v_*)(Wr[r] + k / 2);
      union { float f; uint32_t u; } s0;
      s0.u = (uint32_t)Er[r][k / 32] << 23;
      f2v c0[8];
      fp4x8_to_f32p(w0[0], s0.f, c0);
      fp4x8_to_f32p(w0[1], s0.f, c0 + 4);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        f2v ca = c0[q * 2];
        f2v cb = c0[q * 2 + 1];
        f2v xa, xb;
        if (XDIR) {
          const u16* p0 = (q < 2) ? (const u16*)&xda : (const u16*)&xdb;
          const int o0 = (q & 1) * 4;
          xa = (f2v){b2f(p0[o0]), b2f(p0[o0 + 1])};
          xb = (f2v){b2f(p0[o0 + 2]), b2f(p0[o0 + 3])};
        } else {
          xa = *(const f2v*)(xv + k + q * 4);
          xb = *(const f2v*)(xv + k + q * 4 + 2);
        }
        a0[r] += ca * xa;
        a1[r] += cb * xb;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RPW; r++) {
    f2v s = a0[r] + a1[r];
    float acc = wave_reduce_sum(s[0] + s[1]);
    if (lane == 0 && row0 + r < N)
      gemv_epilogue(acc, row0 + r, y, eres, out_f32, softcap);
  }
  }  // row0 grid-stride loop
}

extern "C" hipError_t launch_gemv_fp4(const void* W, const void* E,
                                      const void* x, const void* x2,
                                      const void* g, const void* g2, void* y,
                                      const void* res, int N, int K,
                                      int stage, int act, float eps,
                                      int out_f32, float softcap, int nt,
                                      int rpw, int maxblocks, float escale,
                                      hipStream_t stream) {
  if (K % 32 != 0) return hipErrorInvalidValue;
  static int xdir_raw4 = -1, rpw_env4 = -1;
  if (xdir_raw4 < 0) {
    const char* e = getenv("LLM_GEMV_XDIR");
    xdir_raw4 = e ? atoi(e) : 1;
    const char* p = getenv("LLM_GEMV_RPW");
    rpw_env4 = p ? atoi(p) : 0;
  }
  if (rpw_env4 > 0) rpw = rpw_env4;
  else if (rpw <= 1)
    rpw = (K >= 3584 && N >= 3072) ? 2 : 1;  // same policy as fp8
  const int xdir = (stage == STAGE_RAW) && xdir_raw4;
  size_t lds = xdir ? 0 : ((size_t)K * 4 + 32);
  if (lds > 65536) {
    static bool raised4 = false;
    if (!raised4) {
#define GEMV4_RAISE(NTV, RPWV, XDV)                                         \
      hipFuncSetAttribute((const void*)&k_gemv_fp4_t<NTV, RPWV, XDV>,       \
                          hipFuncAttributeMaxDynamicSharedMemorySize,       \
                          160 * 1024)
      GEMV4_RAISE(true, 1, false); GEMV4_RAISE(true, 2, false);
      GEMV4_RAISE(false, 1, false); GEMV4_RAISE(false, 2, false);
#undef GEMV4_RAISE
      raised4 = true;
    }
  }
  int threads = 256;
  int wpb = threads / 64;
  int blocks = (N + wpb * rpw - 1) / (wpb * rpw);
  int cap = maxblocks > 0 ? maxblocks : 1024;
  if (blocks > cap) blocks = cap;
#define GEMV4_CASE(NTV, RPWV, XD)                                           \
  hipLaunchKernelGGL((k_gemv_fp4_t<NTV, RPWV, XD>), dim3(blocks),           \
                     dim3(threads), lds, stream, (const uint8_t*)W,         \
                     (const uint8_t*)E, (const u16*)x, (const u16*)x2,      \
                     (const float*)g, (const float*)g2, y, (const u16*)res, \
                     N, K, stage, act, eps, out_f32, softcap, escale)
  if (xdir) {
    if (nt && rpw == 2) GEMV4_CASE(true, 2, true);
    else if (nt) GEMV4_CASE(true, 1, true);
    else if (rpw == 2) GEMV4_CASE(false, 2, true);
    else GEMV4_CASE(false, 1, true);
  } else {
    if (nt && rpw == 2) GEMV4_CASE(true, 2, false);
    else if (nt) GEMV4_CASE(true, 1, false);
    else if (rpw == 2) GEMV4_CASE(false, 2, false);
    else GEMV4_CASE(false, 1, false);
  }
#undef GEMV4_CASE
  return hipGetLastError();
}

// ====================================================================
// RMSNorm: mode 0: y = norm(x)*g ; mode 1: y = res + norm(x)*g
// x bf16 [M,H]; g fp32[H] (Gemma's gamma+1 pre-folded on host); one block
// per row; fused single pass (x kept in registers between reduce+scale).
// ====================================================================

extern "C" __global__ void __launch_bounds__(1024)
k_rmsnorm(const u16* __restrict__ x, const float* __restrict__ g,
          const u16* __restrict__ res, u16* __restrict__ y,
          int H, float eps, int mode) {
  __shared__ float warp_sums[16];
  const int row = blockIdx.x;
  const u16* xr = x + (size_t)row * H;
  u16* yr = y + (size_t)row * H;
  const u16* rr = res ? res + (size_t)row * H : nullptr;

  s8v buf[2];  // up to 16384 elems per row at 1024 threads * 8/chunk
  int nchunk = 0;
  float ss = 0.f;
  for (int i = threadIdx.x * 8; i < H; i += 8192) {
    s8v v = *(const s8v*)(xr + i);
    buf[nchunk++] = v;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float f = b2f(((u16*)&v)[j]);
      ss += f * f;
    }
  }
  ss = wave_reduce_sum(ss);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) warp_sums[wave] = ss;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int w = 0; w < 16; w++) tot += warp_sums[w];
  const float rnorm = rsqrtf(tot / (float)H + eps);

  nchunk = 0;
  for (int i = threadIdx.x * 8; i < H; i += 8192) {
    s8v v = buf[nchunk++];
    f4v g0 = *(const f4v*)(g + i);
    f4v g1 = *(const f4v*)(g + i + 4);
    s8v rv;
    if (mode == 1) rv = *(const s8v*)(rr + i);
    u16 o[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float f = b2f(((u16*)&v)[j]) * rnorm * (j < 4 ? g0[j] : g1[j - 4]);
      if (mode == 1) f += b2f(((u16*)&rv)[j]);
      o[j] = f2b(f);
    }
    *(s8v*)(yr + i) = *(s8v*)o;
  }
}

extern "C" hipError_t launch_rmsnorm(const void* x, const void* g,
                                     const void* res, void* y, int M, int H,
                                     float eps, int mode, hipStream_t stream) {
  // the kernel keeps each row in registers: 2 chunks x 1024 threads x 8
  if (H > 16384 || H % 8 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rmsnorm, dim3(M), dim3(1024), 0, stream,
                     (const u16*)x, (const float*)g, (const u16*)res, (u16*)y,
                     H, eps, mode);
  return hipGetLastError();
}

// ====================================================================
// RoPE + KV-pool write.
// q inout [M, nh*hd]; k_in/v_in [M, kvh*hd]; caches [kvh, S, hd].
// Position of row m is *pos_ptr + m (device scalar: graph-replay-safe).
// cos/sin tables fp32 [max_seq, hd/2].
// ====================================================================

extern "C" __global__ void __launch_bounds__(256)
k_rope_cache(u16* __restrict__ q, const u16* __restrict__ kin,
             const u16* __restrict__ vin, u16* __restrict__ kc,
             u16* __restrict__ vc, const float* __restrict__ cost,
             const float* __restrict__ sint, const int* __restrict__ pos_ptr,
             int nh, int kvh, int hd, int S) {
  const int m = blockIdx.x;
  const int pos = *pos_ptr + m;
  const int hd2 = hd / 2;
  const float* cp = cost + (size_t)pos * hd2;
  const float* sp = sint + (size_t)pos * hd2;

  // q rotation in place
  u16* qr = q + (size_t)m * nh * hd;
  for (int idx = threadIdx.x; idx < nh * hd2; idx += 256) {
    int h = idx / hd2, i = idx % hd2;
    float x1 = b2f(qr[h * hd + i]);
    float x2 = b2f(qr[h * hd + i + hd2]);
    float c = cp[i], s = sp[i];
    qr[h * hd + i] = f2b(x1 * c - x2 * s);
    qr[h * hd + i + hd2] = f2b(x2 * c + x1 * s);
  }
  // k rotation -> cache; v copy -> cache
  const u16* kr = kin + (size_t)m * kvh * hd;
  const u16* vr = vin + (size_t)m * kvh * hd;
  for (int idx = threadIdx.x; idx < kvh * hd2; idx += 256) {
    int h = idx / hd2, i = idx % hd2;
    float x1 = b2f(kr[h * hd + i]);
    float x2 = b2f(kr[h * hd + i + hd2]);
    float c = cp[i], s = sp[i];
    u16* dst = kc + ((size_t)h * S + pos) * hd;
    dst[i] = f2b(x1 * c - x2 * s);
    dst[i + hd2] = f2b(x2 * c + x1 * s);
  }
  for (int idx = threadIdx.x; idx < kvh * hd; idx += 256) {
    int h = idx / hd, i = idx % hd;
    vc[((size_t)h * S + pos) * hd + i] = vr[h * hd + i];
  }
}

// fp8 (e4m3) KV-pool variant: K/V stored as bytes with one fp32 scale
// per (kv_head, position) — absmax/448 over the head_dim values, the
// same scheme as the fp8 weights.  Halves the attention read stream
// (the long-context decode bound) at exact-representable dequant.
extern "C" __global__ void __launch_bounds__(256)
k_rope_cache_fp8(u16* __restrict__ q, const u16* __restrict__ kin,
                 const u16* __restrict__ vin, uint8_t* __restrict__ kc,
                 uint8_t* __restrict__ vc, float* __restrict__ kS,
                 float* __restrict__ vS, const float* __restrict__ cost,
                 const float* __restrict__ sint,
                 const int* __restrict__ pos_ptr,
                 int nh, int kvh, int hd, int S) {
  __shared__ float row[256];
  __shared__ float red[4];
  const int m = blockIdx.x;
  const int pos = *pos_ptr + m;
  const int hd2 = hd / 2;
  const float* cp = cost + (size_t)pos * hd2;
  const float* sp = sint + (size_t)pos * hd2;
  const int tid = threadIdx.x;

  // q rotation in place (q stays bf16)
  u16* qr = q + (size_t)m * nh * hd;
  for (int idx = tid; idx < nh * hd2; idx += 256) {
    int h = idx / hd2, i = idx % hd2;
    float x1 = b2f(qr[h * hd + i]);
    float x2 = b2f(qr[h * hd + i + hd2]);
    float c = cp[i], s = sp[i];
    qr[h * hd + i] = f2b(x1 * c - x2 * s);
    qr[h * hd + i + hd2] = f2b(x2 * c + x1 * s);
  }

  const u16* kr = kin + (size_t)m * kvh * hd;
  const u16* vr = vin + (size_t)m * kvh * hd;
  for (int h = 0; h < kvh; h++) {
    // rotated k row -> LDS floats
    __syncthreads();
    if (tid < hd2) {
      float x1 = b2f(kr[h * hd + tid]);
      float x2 = b2f(kr[h * hd + tid + hd2]);
      float c = cp[tid], s = sp[tid];
      row[tid] = x1 * c - x2 * s;
      row[tid + hd2] = x2 * c + x1 * s;
    }
    __syncthreads();
    float am = 0.f;
    for (int i = tid; i < hd; i += 256) am = fmaxf(am, fabsf(row[i]));
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) am = fmaxf(am, __shfl_xor(am, w));
    if ((tid & 63) == 0) red[tid >> 6] = am;
    __syncthreads();
    am = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sc = fmaxf(am, 1e-8f) / 448.0f;
    if (tid == 0) kS[(size_t)h * S + pos] = sc;
    if (tid * 8 < hd)
      *(unsigned long long*)(kc + ((size_t)h * S + pos) * hd + tid * 8) =
          f32x8_to_fp8(&row[tid * 8], 1.0f / sc);
    // v row (no rotation)
    __syncthreads();
    for (int i = tid; i < hd; i += 256) row[i] = b2f(vr[h * hd + i]);
    __syncthreads();
    am = 0.f;
    for (int i = tid; i < hd; i += 256) am = fmaxf(am, fabsf(row[i]));
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) am = fmaxf(am, __shfl_xor(am, w));
    if ((tid & 63) == 0) red[tid >> 6] = am;
    __syncthreads();
    am = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    sc = fmaxf(am, 1e-8f) / 448.0f;
    if (tid == 0) vS[(size_t)h * S + pos] = sc;
    if (tid * 8 < hd)
      *(unsigned long long*)(vc + ((size_t)h * S + pos) * hd + tid * 8) =
          f32x8_to_fp8(&row[tid * 8], 1.0f / sc);
  }
}

extern "C" hipError_t launch_rope_cache(void* q, const void* kin,
                                        const void* vin, void* kc, void* vc,
                                        void* kS, void* vS, int kv8,
                                        const void* cost, const void* sint,
                                        const void* pos_ptr, int M, int nh,
                                        int kvh, int hd, int S,
                                        hipStream_t stream) {
  if (kv8) {
    hipLaunchKernelGGL(k_rope_cache_fp8, dim3(M), dim3(256), 0, stream,
                       (u16*)q, (const u16*)kin, (const u16*)vin,
                       (uint8_t*)kc, (uint8_t*)vc, (float*)kS, (float*)vS,
                       (const float*)cost, (const float*)sint,
                       (const int*)pos_ptr, nh, kvh, hd, S);
  } else {
    hipLaunchKernelGGL(k_rope_cache, dim3(M), dim3(256), 0, stream, (u16*)q,
                       (const u16*)kin, (const u16*)vin, (u16*)kc, (u16*)vc,
                       (const float*)cost, (const float*)sint,
                       (const int*)pos_ptr, nh, kvh, hd, S);
  }
  return hipGetLastError();
}

// ====================================================================
// GQA attention with online softmax (decode + per-query prefill).
// NOTE: with every shipped preset at head_dim in {64,128,256} the MFMA
// prefill kernel below is taken instead; this per-query VALU kernel is
// kept as the reachable fallback for odd head_dims and as the simple
// DEBUGGING reference the fused kernels are compared against in tests
// (SURVEY §2.2 K1).
// grid (nh, M): block = head h, query row m (absolute pos = *len_ptr + m,
// attends keys [start, pos+1)).  4 waves split the KV range; each lane
// owns (sub-position, 8-dim chunk); merge within wave then across waves.
// Sliding window + attention-logit softcap = real Gemma-2 semantics
// (reference omitted both).
// ====================================================================

template <bool KV8>
__global__ void __launch_bounds__(256)
k_attn_t(const u16* __restrict__ q, const void* __restrict__ kc,
         const void* __restrict__ vc, u16* __restrict__ out,
         const int* __restrict__ len_ptr, const float* __restrict__ kS,
         const float* __restrict__ vS, int nh, int kvh, int hd, int S,
         float scale, float softcap, int window) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = (float*)smem;  // [4][hd] acc + [4][2] m,l

  const int h = blockIdx.x, m = blockIdx.y;
  const int kvhead = h / (nh / kvh);
  const int pos = *len_ptr + m;
  const int T = pos + 1;
  int start = 0;
  if (window > 0 && T - window > 0) start = T - window;

  const int LP = hd / 8;        // lanes per position
  const int PP = 64 / LP;       // positions per wave-iteration
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p = lane / LP, d0 = (lane % LP) * 8;

  // q fragment for this head (8 dims), fp32
  float qf[8];
  {
    s8v v = *(const s8v*)(q + ((size_t)m * nh + h) * hd + d0);
#pragma unroll
    for (int j = 0; j < 8; j++) qf[j] = b2f(((u16*)&v)[j]);
  }

  const u16* K0 = (const u16*)kc + (size_t)kvhead * S * hd;
  const u16* V0 = (const u16*)vc + (size_t)kvhead * S * hd;
  const uint8_t* K08 = (const uint8_t*)kc + (size_t)kvhead * S * hd;
  const uint8_t* V08 = (const uint8_t*)vc + (size_t)kvhead * S * hd;
  const float* kS0 = KV8 ? kS + (size_t)kvhead * S : nullptr;
  const float* vS0 = KV8 ? vS + (size_t)kvhead * S : nullptr;

  float mrun = -INFINITY, lrun = 0.f, acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = 0.f;

  {
    int t0 = start + wave * PP;
    if (t0 < T) {
      int t = t0 + p;
      bool valid = t < T;
      int tl = valid ? t : start;
      s8v kv, vv;
      unsigned long long kraw = 0, vraw = 0;
      float ksc = 1.f, vsc = 1.f;
      if (KV8) {
        kraw = *(const unsigned long long*)(K08 + (size_t)tl * hd + d0);
        vraw = *(const unsigned long long*)(V08 + (size_t)tl * hd + d0);
        ksc = kS0[tl]; vsc = vS0[tl];
      } else {
        kv = *(const s8v*)(K0 + (size_t)tl * hd + d0);
        vv = *(const s8v*)(V0 + (size_t)tl * hd + d0);
      }
      for (; t0 < T; t0 += 4 * PP) {
        int t0n = t0 + 4 * PP;
        s8v kvn, vvn;
        unsigned long long krawn = 0, vrawn = 0;
        float kscn = 1.f, vscn = 1.f;
        bool validn = false;
        if (t0n < T) {
          int tn = t0n + p;
          validn = tn < T;
          int tln = validn ? tn : start;
          if (KV8) {
            krawn = *(const unsigned long long*)(K08 + (size_t)tln * hd + d0);
            vrawn = *(const unsigned long long*)(V08 + (size_t)tln * hd + d0);
            kscn = kS0[tln]; vscn = vS0[tln];
          } else {
            kvn = *(const s8v*)(K0 + (size_t)tln * hd + d0);
            vvn = *(const s8v*)(V0 + (size_t)tln * hd + d0);
          }
        }
        float partial = 0.f;
        if (KV8) {
          // dequant straight to f32 in the dot (4 cvt + 8 fma per 8
          // elems — cheaper than the bf16 path's 8 shifts + 8 fma)
          f2v c0_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)kraw, false);
          f2v c1_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)kraw, true);
          f2v c2_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)(kraw >> 32),
                                                    false);
          f2v c3_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)(kraw >> 32),
                                                    true);
          partial = qf[0] * c0_[0] + qf[1] * c0_[1] + qf[2] * c1_[0] +
                    qf[3] * c1_[1] + qf[4] * c2_[0] + qf[5] * c2_[1] +
                    qf[6] * c3_[0] + qf[7] * c3_[1];
        } else {
#pragma unroll
          for (int j = 0; j < 8; j++) partial += qf[j] * b2f(((u16*)&kv)[j]);
        }
        for (int w = 1; w < LP; w <<= 1) partial += __shfl_xor(partial, w);
        float score = partial * (KV8 ? ksc : 1.f) * scale;
        if (softcap > 0.f) score = softcap * tanhf(score / softcap);
        if (!valid) score = -INFINITY;
        float mnew = fmaxf(mrun, score);
        float alpha = (mnew == -INFINITY) ? 0.f : __expf(mrun - mnew);
        float pv = (mnew == -INFINITY) ? 0.f : __expf(score - mnew);
        lrun = lrun * alpha + pv;
        if (KV8) {
          float pvv = pv * vsc;
          f2v d0_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)vraw, false);
          f2v d1_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)vraw, true);
          f2v d2_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)(vraw >> 32),
                                                    false);
          f2v d3_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)(vraw >> 32),
                                                    true);
          float vf[8] = {d0_[0], d0_[1], d1_[0], d1_[1],
                         d2_[0], d2_[1], d3_[0], d3_[1]};
#pragma unroll
          for (int j = 0; j < 8; j++)
            acc[j] = acc[j] * alpha + pvv * vf[j];
        } else {
#pragma unroll
          for (int j = 0; j < 8; j++)
            acc[j] = acc[j] * alpha + pv * b2f(((u16*)&vv)[j]);
        }
        if (mnew != -INFINITY) mrun = mnew;
        kv = kvn; vv = vvn; kraw = krawn; vraw = vrawn;
        valid = validn; ksc = kscn; vsc = vscn;
      }
    }
  }

  // merge across position-groups within the wave (lanes l, l^LP, l^2LP, ...)
  for (int w = LP; w < 64; w <<= 1) {
    float mo = __shfl_xor(mrun, w);
    float lo = __shfl_xor(lrun, w);
    float mn = fmaxf(mrun, mo);
    float sa = (mrun == -INFINITY && mo == -INFINITY) ? 0.f : __expf(mrun - mn);
    float sb = (mrun == -INFINITY && mo == -INFINITY) ? 0.f : __expf(mo - mn);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float ao = __shfl_xor(acc[j], w);
      acc[j] = acc[j] * sa + ao * sb;
    }
    lrun = lrun * sa + lo * sb;
    mrun = mn;
  }

  // merge across the 4 waves via LDS
  float* accs = red;             // [4][hd]
  float* mls = red + 4 * hd;     // [4][2]
  if (lane < LP) {
#pragma unroll
    for (int j = 0; j < 8; j++) accs[wave * hd + d0 + j] = acc[j];
  }
  if (lane == 0) {
    mls[wave * 2] = mrun;
    mls[wave * 2 + 1] = lrun;
  }
  __syncthreads();
  if (wave == 0) {
    float mt = fmaxf(fmaxf(mls[0], mls[2]), fmaxf(mls[4], mls[6]));
    float lt = 0.f, sc[4];
#pragma unroll
    for (int w = 0; w < 4; w++) {
      sc[w] = (mls[w * 2] == -INFINITY) ? 0.f : __expf(mls[w * 2] - mt);
      lt += mls[w * 2 + 1] * sc[w];
    }
    float inv = 1.f / lt;
    for (int d = lane; d < hd; d += 64) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < 4; w++) v += accs[w * hd + d] * sc[w];
      out[((size_t)m * nh + h) * hd + d] = f2b(v * inv);
    }
  }
}

// ====================================================================
// Fused decode attention (M=1): RoPE(q,k) + KV-pool write + online-
// softmax GQA, split over the KV range.  grid = (nh, SPLIT): each block
// scans one chunk of history; partial (m, l, acc) results are combined
// by the LAST-arriving block of each head via the agent-scope
// release/acquire + ticket recipe (guide §6 G16) — placement-independent
// and graph-replay-safe (the merger resets its head's counter).
// For SPLIT 2..4 the in-block form (k_attn_dec_blk_t) puts the SPLIT
// chunks into ONE block of 256 * SPLIT threads and merges through LDS:
// same chunk and merge source, same bits, no global hand-off.
// The SPLIT-1 chunk also handles the current token from registers and
// one block per kv-head persists the new k/v to the pool.
// Gemma-2 semantics included: sliding window + attn-logit softcap.
// ====================================================================

// One chunk of one head, by the four waves `wave` = 0..3 that share the
// LDS region `red` ([4][hd] + [4][2] floats): `chunk` of `SPLIT` for head
// blockIdx.x of row blockIdx.z.  Wave 0 leaves the chunk's partial —
// m, l, then the hd UNnormalized accumulators — in slot `pidx` of `parts`
// ([.][hd + 2] floats: global scratch in the ticket kernels, LDS in the
// in-block ones), or with SPLIT == 1 writes the normalized row to `out`.
// Holds one __syncthreads(): every thread of the block calls it.
template <bool KV8>
DEVINL void attn_dec_chunk(float* red, const int chunk, const int SPLIT,
                           const int wave, const int lane,
                           float* __restrict__ parts, const int pidx,
                           const u16* __restrict__ qkv, void* __restrict__ kc,
                           void* __restrict__ vc, u16* __restrict__ out,
                           const int* __restrict__ len_ptr,
                           const float* __restrict__ cost,
                           const float* __restrict__ sint,
                           float* __restrict__ kS, float* __restrict__ vS,
                           int nh, int kvh, int hd, int S, float scale,
                           float softcap, int window) {
  const int h = blockIdx.x;
  // batch axis (lockstep sequences): per-b qkv/out rows, KV pool and
  // scales; the position is shared
  const int b = blockIdx.z;
  qkv += (size_t)b * (nh + 2 * kvh) * hd;
  out += (size_t)b * nh * hd;
  kc = (char*)kc + (size_t)b * kvh * S * hd * (KV8 ? 1 : 2);
  vc = (char*)vc + (size_t)b * kvh * S * hd * (KV8 ? 1 : 2);
  if (KV8) { kS += (size_t)b * kvh * S; vS += (size_t)b * kvh * S; }
  const int grp = nh / kvh;
  const int kvhead = h / grp;
  // RAGGED batch: each sequence row sits at its own position
  // (len_ptr is a per-row array; the single-sequence path passes its
  // scalar length buffer and reads index 0)
  const int pos = len_ptr[b];
  int start = 0;
  if (window > 0 && pos + 1 - window > 0) start = pos + 1 - window;
  // history chunk [c0, c1) of [start, pos)
  const int hist = pos - start;
  const int clen = (hist + SPLIT - 1) / SPLIT;
  const int c0 = start + chunk * clen;
  const int c1 = min(c0 + clen, pos);
  const bool last_chunk = (chunk == SPLIT - 1);

  const int LP = hd / 8;
  const int PP = 64 / LP;
  const int p = lane / LP, d0 = (lane % LP) * 8;
  const int hd2 = hd / 2;
  const float* cp = cost + (size_t)pos * hd2;
  const float* sp = sint + (size_t)pos * hd2;

  const u16* qh = qkv + (size_t)h * hd;
  const u16* kh = qkv + (size_t)(nh + kvhead) * hd;
  const u16* vh = qkv + (size_t)(nh + kvh + kvhead) * hd;
  const u16* K0 = (const u16*)kc + (size_t)kvhead * S * hd;
  const u16* V0 = (const u16*)vc + (size_t)kvhead * S * hd;
  const uint8_t* K08 = (const uint8_t*)kc + (size_t)kvhead * S * hd;
  const uint8_t* V08 = (const uint8_t*)vc + (size_t)kvhead * S * hd;
  const float* kS0 = KV8 ? kS + (size_t)kvhead * S : nullptr;
  const float* vS0 = KV8 ? vS + (size_t)kvhead * S : nullptr;

  // history loads of iteration tt of this wave's scan (positions tt+p);
  // nothing is loaded past the chunk (tt >= c1 leaves the outputs alone)
  auto ldkv = [&](int tt, bool& vld, s8v& ko, s8v& vo,
                  unsigned long long& kro, unsigned long long& vro,
                  float& kso, float& vso) {
    vld = false;
    if (tt < c1) {
      int t_ = tt + p;
      vld = t_ < c1;
      int tl_ = vld ? t_ : c0;
      if (KV8) {
        kro = *(const unsigned long long*)(K08 + (size_t)tl_ * hd + d0);
        vro = *(const unsigned long long*)(V08 + (size_t)tl_ * hd + d0);
        kso = kS0[tl_]; vso = vS0[tl_];
      } else {
        ko = *(const s8v*)(K0 + (size_t)tl_ * hd + d0);
        vo = *(const s8v*)(V0 + (size_t)tl_ * hd + d0);
      }
    }
  };
  s8v kv{}, vv{}, kvn{}, vvn{};
  unsigned long long kraw = 0, vraw = 0, krawn = 0, vrawn = 0;
  float ksc = 1.f, vsc = 1.f, kscn = 1.f, vscn = 1.f;
  bool valid, validn;

  float qf[8], kn[8], vn[8];
  {
    const bool lo = d0 < hd2;
    const int dp = lo ? d0 + hd2 : d0 - hd2;
    const int ci = lo ? d0 : d0 - hd2;
    s8v qa = *(const s8v*)(qh + d0);
    s8v qb = *(const s8v*)(qh + dp);
    s8v ka = *(const s8v*)(kh + d0);
    s8v kb = *(const s8v*)(kh + dp);
    s8v va = *(const s8v*)(vh + d0);
    f4v c0v = *(const f4v*)(cp + ci);
    f4v c1v = *(const f4v*)(cp + ci + 4);
    f4v s0v = *(const f4v*)(sp + ci);
    f4v s1v = *(const f4v*)(sp + ci + 4);
    // The first two iterations' K/V history go out here, behind the
    // new token's loads and ahead of the RoPE arithmetic and the pool
    // write: [c0, c1) never contains pos, so the write cannot feed
    // them, and their (cold) miss overlaps the cos/sin/qkv miss.
    // vmcnt retires in order: the arithmetic below waits for the loads
    // above only.
    {
      const int t0 = c0 + wave * PP;
      ldkv(t0, valid, kv, vv, kraw, vraw, ksc, vsc);
      ldkv(t0 + 4 * PP, validn, kvn, vvn, krawn, vrawn, kscn, vscn);
    }
    const float sgn = lo ? -1.f : 1.f;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float c = j < 4 ? c0v[j] : c1v[j - 4];
      float s = j < 4 ? s0v[j] : s1v[j - 4];
      qf[j] = b2f(((u16*)&qa)[j]) * c + sgn * b2f(((u16*)&qb)[j]) * s;
      kn[j] = b2f(((u16*)&ka)[j]) * c + sgn * b2f(((u16*)&kb)[j]) * s;
      vn[j] = b2f(((u16*)&va)[j]);
    }
  }
  if (last_chunk && h == kvhead * grp && wave == 0 && p == 0) {
    if (KV8) {
      // per-(head,pos) absmax across the LP lanes (each holds 8 dims)
      float kam = 0.f, vam = 0.f;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        kam = fmaxf(kam, fabsf(kn[j]));
        vam = fmaxf(vam, fabsf(vn[j]));
      }
      for (int w = 1; w < LP; w <<= 1) {
        kam = fmaxf(kam, __shfl_xor(kam, w));
        vam = fmaxf(vam, __shfl_xor(vam, w));
      }
      // the new token's scales (ksc / vsc hold the prefetched history's)
      const float knsc = fmaxf(kam, 1e-8f) / 448.0f;
      const float vnsc = fmaxf(vam, 1e-8f) / 448.0f;
      *(unsigned long long*)((uint8_t*)kc +
          ((size_t)kvhead * S + pos) * hd + d0) = f32x8_to_fp8(kn, 1.f / knsc);
      *(unsigned long long*)((uint8_t*)vc +
          ((size_t)kvhead * S + pos) * hd + d0) = f32x8_to_fp8(vn, 1.f / vnsc);
      if (lane == 0) {
        kS[(size_t)kvhead * S + pos] = knsc;
        vS[(size_t)kvhead * S + pos] = vnsc;
      }
    } else {
      u16 ko[8], vo[8];
#pragma unroll
      for (int j = 0; j < 8; j++) { ko[j] = f2b(kn[j]); vo[j] = f2b(vn[j]); }
      *(s8v*)((u16*)kc + ((size_t)kvhead * S + pos) * hd + d0) = *(s8v*)ko;
      *(s8v*)((u16*)vc + ((size_t)kvhead * S + pos) * hd + d0) = *(s8v*)vo;
    }
  }

  float mrun = -INFINITY, lrun = 0.f, acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = 0.f;

  // software-pipelined history scan: K[i+1]/V[i+1] issue while the
  // score/online-update of iteration i computes (the serial
  // K->dot->softmax->V chain was the latency bottleneck at small T)
  {
    int t0 = c0 + wave * PP;
    if (t0 < c1) {
      // 2-AHEAD software pipeline: K/V for iterations i+1 and i+2 are
      // in flight while iteration i computes (the serial
      // K->dot->softmax->V chain is the latency bound at small T);
      // iterations 0 and 1 were issued at the top of the kernel
      for (; t0 < c1; t0 += 4 * PP) {
        s8v kv2{}, vv2{};
        unsigned long long kraw2 = 0, vraw2 = 0;
        float ksc2 = 1.f, vsc2 = 1.f;
        bool valid2;
        ldkv(t0 + 8 * PP, valid2, kv2, vv2, kraw2, vraw2, ksc2, vsc2);
        float partial = 0.f;
        if (KV8) {
          // dequant straight to f32 in the dot (4 cvt + 8 fma per 8
          // elems — cheaper than the bf16 path's 8 shifts + 8 fma)
          f2v c0_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)kraw, false);
          f2v c1_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)kraw, true);
          f2v c2_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)(kraw >> 32),
                                                    false);
          f2v c3_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)(kraw >> 32),
                                                    true);
          partial = qf[0] * c0_[0] + qf[1] * c0_[1] + qf[2] * c1_[0] +
                    qf[3] * c1_[1] + qf[4] * c2_[0] + qf[5] * c2_[1] +
                    qf[6] * c3_[0] + qf[7] * c3_[1];
        } else {
#pragma unroll
          for (int j = 0; j < 8; j++) partial += qf[j] * b2f(((u16*)&kv)[j]);
        }
        for (int w = 1; w < LP; w <<= 1) partial += __shfl_xor(partial, w);
        float score = partial * (KV8 ? ksc : 1.f) * scale;
        if (softcap > 0.f) score = softcap * tanhf(score / softcap);
        if (!valid) score = -INFINITY;
        float mnew = fmaxf(mrun, score);
        float alpha = (mnew == -INFINITY) ? 0.f : __expf(mrun - mnew);
        float pv = (mnew == -INFINITY) ? 0.f : __expf(score - mnew);
        lrun = lrun * alpha + pv;
        if (KV8) {
          float pvv = pv * vsc;
          f2v d0_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)vraw, false);
          f2v d1_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)vraw, true);
          f2v d2_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)(vraw >> 32),
                                                    false);
          f2v d3_ = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)(vraw >> 32),
                                                    true);
          float vf[8] = {d0_[0], d0_[1], d1_[0], d1_[1],
                         d2_[0], d2_[1], d3_[0], d3_[1]};
#pragma unroll
          for (int j = 0; j < 8; j++)
            acc[j] = acc[j] * alpha + pvv * vf[j];
        } else {
#pragma unroll
          for (int j = 0; j < 8; j++)
            acc[j] = acc[j] * alpha + pv * b2f(((u16*)&vv)[j]);
        }
        if (mnew != -INFINITY) mrun = mnew;
        kv = kvn; vv = vvn; kraw = krawn; vraw = vrawn;
        valid = validn; ksc = kscn; vsc = vscn;
        kvn = kv2; vvn = vv2; krawn = kraw2; vrawn = vraw2;
        validn = valid2; kscn = ksc2; vscn = vsc2;
      }
    }
  }

  // current position from registers (last chunk, p == 0 lanes of wave 0)
  if (last_chunk && wave == 0 && p == 0) {
    float partial = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) partial += qf[j] * kn[j];
    for (int w = 1; w < LP; w <<= 1) partial += __shfl_xor(partial, w);
    float score = partial * scale;
    if (softcap > 0.f) score = softcap * tanhf(score / softcap);
    float mnew = fmaxf(mrun, score);
    float alpha = __expf(mrun - mnew);
    float pv = __expf(score - mnew);
    lrun = lrun * alpha + pv;
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = acc[j] * alpha + pv * vn[j];
    mrun = mnew;
  }

  // merge position-groups within the wave
  for (int w = LP; w < 64; w <<= 1) {
    float mo = __shfl_xor(mrun, w);
    float lo2 = __shfl_xor(lrun, w);
    float mn = fmaxf(mrun, mo);
    float sa = (mrun == -INFINITY && mo == -INFINITY) ? 0.f : __expf(mrun - mn);
    float sb = (mrun == -INFINITY && mo == -INFINITY) ? 0.f : __expf(mo - mn);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float ao = __shfl_xor(acc[j], w);
      acc[j] = acc[j] * sa + ao * sb;
    }
    lrun = lrun * sa + lo2 * sb;
    mrun = mn;
  }

  // merge the 4 waves via LDS -> block partial in red[0..hd)+m,l
  float* accs = red;
  float* mls = red + 4 * hd;
  if (lane < LP) {
#pragma unroll
    for (int j = 0; j < 8; j++) accs[wave * hd + d0 + j] = acc[j];
  }
  if (lane == 0) {
    mls[wave * 2] = mrun;
    mls[wave * 2 + 1] = lrun;
  }
  __syncthreads();

  float* part = parts + (size_t)pidx * (hd + 2);
  if (wave == 0) {
    float mt = fmaxf(fmaxf(mls[0], mls[2]), fmaxf(mls[4], mls[6]));
    float lt = 0.f, sc[4];
#pragma unroll
    for (int w = 0; w < 4; w++) {
      sc[w] = (mls[w * 2] == -INFINITY) ? 0.f : __expf(mls[w * 2] - mt);
      lt += mls[w * 2 + 1] * sc[w];
    }
    if (SPLIT == 1) {
      // single chunk: normalize in registers and write out directly
      float inv = 1.f / lt;
      for (int d = lane; d < hd; d += 64) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 4; w++) v += accs[w * hd + d] * sc[w];
        out[(size_t)h * hd + d] = f2b(v * inv);
      }
    } else {
      for (int d = lane; d < hd; d += 64) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 4; w++) v += accs[w * hd + d] * sc[w];
        part[2 + d] = v;  // UNnormalized chunk acc at max mt, sum lt
      }
      if (lane == 0) { part[0] = mt; part[1] = lt; }
    }
  }
}

// One wave merges a head's SPLIT chunk partials at `base`
// ([SPLIT][hd + 2] floats, as attn_dec_chunk leaves them) into the
// normalized row `out_h`: max over the chunks, then sums for
// c = 0..SPLIT-1 — the order does not depend on who calls it.
DEVINL void attn_dec_merge(const float* base, const int SPLIT, const int lane,
                           const int hd, u16* out_h) {
  float mt = -INFINITY;
  for (int c = 0; c < SPLIT; c++)
    mt = fmaxf(mt, base[(size_t)c * (hd + 2)]);
  float lt = 0.f;
  for (int c = 0; c < SPLIT; c++) {
    float mc = base[(size_t)c * (hd + 2)];
    if (mc != -INFINITY)
      lt += base[(size_t)c * (hd + 2) + 1] * __expf(mc - mt);
  }
  float inv = 1.f / lt;
  for (int d = lane; d < hd; d += 64) {
    float v = 0.f;
    for (int c = 0; c < SPLIT; c++) {
      float mc = base[(size_t)c * (hd + 2)];
      if (mc != -INFINITY)
        v += base[(size_t)c * (hd + 2) + 2 + d] * __expf(mc - mt);
    }
    out_h[d] = f2b(v * inv);
  }
}

// The ticket form's attention block (256 threads), shared by the plain
// and the prefetching kernel: `chunk` of `SPLIT` for head blockIdx.x of
// row blockIdx.z; partials cross blocks through `scratch`, tickets in
// `cnt` (both per batch row).
template <bool KV8>
DEVINL void attn_dec_body(char* smem, const int chunk, const int SPLIT,
                          const u16* __restrict__ qkv, void* __restrict__ kc,
                          void* __restrict__ vc, u16* __restrict__ out,
                          const int* __restrict__ len_ptr,
                          const float* __restrict__ cost,
                          const float* __restrict__ sint,
                          float* __restrict__ kS, float* __restrict__ vS,
                          float* __restrict__ scratch, int* __restrict__ cnt,
                          int nh, int kvh, int hd, int S, float scale,
                          float softcap, int window) {
  float* red = (float*)smem;              // [4][hd] + [4][2] + flag
  int* lastflag = (int*)(red + 4 * hd + 8);
  const int h = blockIdx.x;
  const int b = blockIdx.z;
  scratch += (size_t)b * nh * SPLIT * (hd + 2);
  cnt += b * nh;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  attn_dec_chunk<KV8>(red, chunk, SPLIT, wave, lane, scratch,
                      h * SPLIT + chunk, qkv, kc, vc, out, len_ptr, cost,
                      sint, kS, vS, nh, kvh, hd, S, scale, softcap, window);
  if (SPLIT == 1) return;

  // publish + ticket (G16 R1: plain stores -> per-wave drain -> barrier
  // -> one-lane agent release -> asm drain -> relaxed ticket)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int t = __hip_atomic_fetch_add(&cnt[h], 1, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    *lastflag = (t == SPLIT - 1);
  }
  __syncthreads();
  if (!*lastflag) return;

  // last arriver of this head: acquire, merge all chunk partials
  if (threadIdx.x == 0)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  __syncthreads();
  if (wave == 0)
    attn_dec_merge(scratch + (size_t)h * SPLIT * (hd + 2), SPLIT, lane, hd,
                   out + ((size_t)b * nh + h) * hd);
  __syncthreads();
  if (threadIdx.x == 0) cnt[h] = 0;  // re-arm for the next graph replay
}

// The in-block form: ONE block of 256 * SPLIT threads per (head, row).
// Waves 4c..4c+3 are chunk c's four waves and do what a ticket block
// does, on their own `red` region; the chunk partials stay in LDS and
// wave 0 merges them after one barrier.  No global scratch, no fence, no
// atomic, no ticket: the kernel takes neither `scratch` nor `cnt`.
template <bool KV8, int SPLIT>
DEVINL void attn_dec_body_blk(char* smem, const u16* __restrict__ qkv,
                              void* __restrict__ kc, void* __restrict__ vc,
                              u16* __restrict__ out,
                              const int* __restrict__ len_ptr,
                              const float* __restrict__ cost,
                              const float* __restrict__ sint,
                              float* __restrict__ kS, float* __restrict__ vS,
                              int nh, int kvh, int hd, int S, float scale,
                              float softcap, int window) {
  const int wg = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int chunk = wg >> 2;
  float* red = (float*)smem + chunk * (4 * hd + 8);  // [SPLIT] regions
  float* parts = (float*)smem + SPLIT * (4 * hd + 8);  // [SPLIT][hd + 2]
  attn_dec_chunk<KV8>(red, chunk, SPLIT, wg & 3, lane, parts, chunk,
                      qkv, kc, vc, out, len_ptr, cost, sint, kS, vS, nh, kvh,
                      hd, S, scale, softcap, window);
  __syncthreads();
  if (wg == 0)
    attn_dec_merge(parts, SPLIT, lane, hd,
                   out + ((size_t)blockIdx.z * nh + blockIdx.x) * hd);
}

// --------------------------------------------------------------------
// Weight prefetch from the attention launch.  The attention blocks are
// a latency chain that leaves HBM idle, and the next two kernels'
// weights are known at capture time, so the prefetching kernel variant
// carries extra grid.y rows of blocks that pull up to four byte regions
// through L2 into the Infinity Cache with plain (retaining) loads.
// They synchronise with nothing and touch no attention state (no cnt,
// no scratch, no LDS); the only store is guarded by `never` (always -1)
// and exists to keep the loads alive.
// --------------------------------------------------------------------

struct AttnPf {
  const void* ptr[4];
  long bytes[4];   // rounded DOWN to whole 16 B; 0 or a null ptr skips
  long stride0;    // region 0: bytes one consumer block reads (0 = flat)
  float* sink;
  int never;       // -1: no thread index equals it
};

constexpr int PF_LD = 8;              // independent 16-B loads per lane
constexpr int PF_TRIP = 256 * PF_LD;  // 16-B segments per block trip

// One trip: PF_LD loads per lane, each wave-load 1 KB contiguous.  `seg`
// maps a trip-relative segment number to a segment of the region and is
// clamped here to [0, nseg): no load starts at or beyond ptr + bytes.
template <typename F>
DEVINL uint32_t attn_pf_trip(const u4v* __restrict__ base, long nseg, F seg) {
  u4v v[PF_LD];
#pragma unroll
  for (int j = 0; j < PF_LD; j++) {
    long s = seg(j * 256 + (int)threadIdx.x);
    s = s < nseg ? s : nseg - 1;
    v[j] = base[s];
  }
  uint32_t a = 0;
#pragma unroll
  for (int j = 0; j < PF_LD; j++) {
    // pin all 16 B: with only word 0 live the compiler narrows the load
    // to a dword (measured the same; the wide form is the stated one)
    asm volatile("" ::"v"(v[j]));
    a ^= v[j][0];  // one live word per load
  }
  return a;
}

// `arows`: the grid.y rows ahead of the prefetch rows (the attention
// blocks: `split` in the ticket form, 1 in the in-block form).  Threads
// 0..255 of the block work.
DEVINL void attn_dec_prefetch(const AttnPf& pf, const int arows) {
  const uint32_t nx = gridDim.x;
  const uint32_t pfy = gridDim.y - arows;
  const uint32_t npb = nx * pfy * gridDim.z;  // prefetch blocks in all
  const uint32_t pb =
      (blockIdx.z * pfy + (blockIdx.y - arows)) * nx + blockIdx.x;
  uint32_t acc = 0;
  // The regions form one range, concatenated in whole trips and dealt
  // to the blocks round-robin: `g0` = trips handed out so far, mod npb.
  uint32_t g0 = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const u4v* base = (const u4v*)pf.ptr[r];
    const long nseg = pf.bytes[r] >> 4;
    if (base == nullptr || nseg <= 0) continue;
    const long spu = pf.stride0 >> 4;  // segments per consumer block
    if (r == 0 && spu > 0 && (nx & 7) == 0 && nseg < (1l << 31)) {
      // L2 placement (speed only; nothing depends on it): workgroups
      // are dealt round-robin to the 8 XCDs, so with nx % 8 == 0 this
      // block shares an XCD with the consumer blocks u = c (mod 8).
      // The blocks of class c walk those units as one virtual range.
      const uint32_t c = blockIdx.x & 7;
      const uint32_t nunit = (uint32_t)((nseg + spu - 1) / spu);
      if (nunit <= c) continue;
      const uint32_t uspu = (uint32_t)spu;
      const long vseg = (long)((nunit - c + 7) / 8) * spu;
      const uint32_t rc = (pb / nx) * (nx / 8) + blockIdx.x / 8;
      for (long t = rc; t * PF_TRIP < vseg; t += npb / 8) {
        acc ^= attn_pf_trip(base, nseg, [&](int i) {
          long v = t * PF_TRIP + i;
          v = v < vseg ? v : vseg - 1;
          const uint32_t k = (uint32_t)v / uspu;
          return (long)(c + 8 * k) * spu + ((uint32_t)v - k * uspu);
        });
      }
      continue;
    }
    const long ntrip = (nseg + PF_TRIP - 1) / PF_TRIP;
    for (long t = (pb + npb - g0) % npb; t < ntrip; t += npb)
      acc ^= attn_pf_trip(base, nseg,
                          [&](int i) { return t * PF_TRIP + i; });
    g0 = (uint32_t)((g0 + ntrip) % npb);
  }
  // the fold above needs every load's data, so this also waits for them
  asm volatile("" ::"v"(acc));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if ((int)threadIdx.x == pf.never) pf.sink[pb & 255] = (float)acc;
}

// PF: grid (nh, split + PFY, batch); rows y >= split are prefetch blocks
// (dispatched behind the attention blocks of their batch row), so the
// attention chunking takes `split` from the argument.  The plain kernel
// has no such arguments (PFA is empty: its argument list is the one it
// always had) and chunks by gridDim.y.
struct AttnPfLaunch {
  int split;
  AttnPf pf;
};

template <bool KV8, bool PF, typename... PFA>
__global__ void __launch_bounds__(256)
k_attn_dec_t(const u16* __restrict__ qkv, void* __restrict__ kc,
             void* __restrict__ vc, u16* __restrict__ out,
             const int* __restrict__ len_ptr, const float* __restrict__ cost,
             const float* __restrict__ sint, float* __restrict__ kS,
             float* __restrict__ vS, float* __restrict__ scratch,
             int* __restrict__ cnt, int nh, int kvh, int hd, int S,
             float scale, float softcap, int window, PFA... pfa) {
  static_assert(sizeof...(PFA) == (PF ? 1 : 0), "PF takes one AttnPfLaunch");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int SPLIT = gridDim.y;
  if constexpr (PF) {
    const AttnPfLaunch& a = (pfa, ...);
    if ((int)blockIdx.y >= a.split) {
      attn_dec_prefetch(a.pf, a.split);
      return;
    }
    SPLIT = a.split;
  }
  attn_dec_body<KV8>(smem, blockIdx.y, SPLIT, qkv, kc, vc, out, len_ptr, cost,
                     sint, kS, vS, scratch, cnt, nh, kvh, hd, S, scale,
                     softcap, window);
}

// In-block form: grid (nh, 1 + PFY, batch), 256 * SPLIT threads; row
// y == 0 is the attention block, rows y >= 1 are prefetch blocks in which
// threads 0..255 work and the rest leave at once (the prefetch geometry
// stays nh x 256 threads per row).  No scratch / cnt arguments.
template <bool KV8, int SPLIT, bool PF, typename... PFA>
__global__ void __launch_bounds__(256 * SPLIT)
k_attn_dec_blk_t(const u16* __restrict__ qkv, void* __restrict__ kc,
                 void* __restrict__ vc, u16* __restrict__ out,
                 const int* __restrict__ len_ptr,
                 const float* __restrict__ cost,
                 const float* __restrict__ sint, float* __restrict__ kS,
                 float* __restrict__ vS, int nh, int kvh, int hd, int S,
                 float scale, float softcap, int window, PFA... pfa) {
  static_assert(sizeof...(PFA) == (PF ? 1 : 0), "PF takes one AttnPf");
  static_assert(SPLIT >= 2 && SPLIT <= 4, "256 * SPLIT threads, one block");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if constexpr (PF) {
    if (blockIdx.y >= 1) {
      if (threadIdx.x >= 256) return;
      const AttnPf& pf = (pfa, ...);
      attn_dec_prefetch(pf, 1);
      return;
    }
  }
  attn_dec_body_blk<KV8, SPLIT>(smem, qkv, kc, vc, out, len_ptr, cost, sint,
                                kS, vS, nh, kvh, hd, S, scale, softcap,
                                window);
}

// Launches the attention kernel with `pf_blocks` prefetch blocks (rounded
// to whole grid.y rows of nh blocks) over up to four regions; stride0 is
// "rows per consumer block x row bytes" of region 0's consumer, 0 to walk
// it flat.  pf_blocks == 0 dispatches the plain kernel.
// merge: 0 = in-block form when 2 <= split <= 4, else the ticket form;
// 1 = ticket form; 2 = in-block form (an error where 256 * split threads
// exceed a block).  split == 1 is one chunk either way: the ticket kernel.
static hipError_t attn_dec_launch(const void* qkv, void* kc, void* vc,
                                  void* out, const void* len_ptr,
                                  const void* cost, const void* sint,
                                  void* kS, void* vS, int kv8, void* scratch,
                                  void* cnt, int split, int batch, int nh,
                                  int kvh, int hd, int S, float scale,
                                  float softcap, int window, int pf_blocks,
                                  const AttnPf& pf, int merge,
                                  hipStream_t stream) {
  if (merge < 0 || merge > 2 || split < 1) return hipErrorInvalidValue;
  if (merge == 2 && 256 * split > 1024) return hipErrorInvalidValue;
  size_t lds = (4 * hd + 8) * sizeof(float) + 16;
  const int pfy = pf_blocks > 0 ? (pf_blocks + nh - 1) / nh : 0;
  if (merge != 1 && split >= 2 && split <= 4) {
    const size_t blds =
        (size_t)split * ((4 * hd + 8) + (hd + 2)) * sizeof(float);
#define ATTN_BLK_ARGS                                                        \
  (const u16*)qkv, kc, vc, (u16*)out, (const int*)len_ptr,                   \
      (const float*)cost, (const float*)sint, (float*)kS, (float*)vS, nh,    \
      kvh, hd, S, scale, softcap, window
#define ATTN_BLK_CASE(KV8V, SP)                                              \
  do {                                                                       \
    if (pfy > 0)                                                             \
      hipLaunchKernelGGL((k_attn_dec_blk_t<KV8V, SP, true, AttnPf>),         \
                         dim3(nh, 1 + pfy, batch), dim3(256 * SP), blds,     \
                         stream, ATTN_BLK_ARGS, pf);                         \
    else                                                                     \
      hipLaunchKernelGGL((k_attn_dec_blk_t<KV8V, SP, false>),                \
                         dim3(nh, 1, batch), dim3(256 * SP), blds, stream,   \
                         ATTN_BLK_ARGS);                                     \
  } while (0)
#define ATTN_BLK_SPLIT(KV8V)                                                 \
  do {                                                                       \
    if (split == 2) ATTN_BLK_CASE(KV8V, 2);                                  \
    else if (split == 3) ATTN_BLK_CASE(KV8V, 3);                             \
    else ATTN_BLK_CASE(KV8V, 4);                                             \
  } while (0)
    if (kv8) ATTN_BLK_SPLIT(true);
    else ATTN_BLK_SPLIT(false);
#undef ATTN_BLK_SPLIT
#undef ATTN_BLK_CASE
#undef ATTN_BLK_ARGS
    return hipGetLastError();
  }
#define ATTN_DEC_ARGS                                                        \
  (const u16*)qkv, kc, vc, (u16*)out, (const int*)len_ptr,                   \
      (const float*)cost, (const float*)sint, (float*)kS, (float*)vS,        \
      (float*)scratch, (int*)cnt, nh, kvh, hd, S, scale, softcap, window
#define ATTN_DEC_CASE(KV8V)                                                  \
  hipLaunchKernelGGL((k_attn_dec_t<KV8V, false>), dim3(nh, split, batch),    \
                     dim3(256), lds, stream, ATTN_DEC_ARGS)
#define ATTN_DEC_PF_CASE(KV8V)                                               \
  hipLaunchKernelGGL((k_attn_dec_t<KV8V, true, AttnPfLaunch>),               \
                     dim3(nh, split + pfy, batch), dim3(256), lds, stream,   \
                     ATTN_DEC_ARGS, AttnPfLaunch{split, pf})
  if (pfy > 0) {
    if (kv8) ATTN_DEC_PF_CASE(true);
    else ATTN_DEC_PF_CASE(false);
  } else {
    if (kv8) ATTN_DEC_CASE(true);
    else ATTN_DEC_CASE(false);
  }
#undef ATTN_DEC_PF_CASE
#undef ATTN_DEC_ARGS
#undef ATTN_DEC_CASE
  return hipGetLastError();
}

extern "C" hipError_t launch_attn_dec_pf(
    const void* qkv, void* kc, void* vc, void* out, const void* len_ptr,
    const void* cost, const void* sint, void* kS, void* vS, int kv8,
    void* scratch, void* cnt, int split, int batch, int nh, int kvh, int hd,
    int S, float scale, float softcap, int window, int pf_blocks,
    const void* p0, long n0, const void* p1, long n1, const void* p2,
    long n2, const void* p3, long n3, long stride0, void* sink, int merge,
    hipStream_t stream) {
  AttnPf pf{{p0, p1, p2, p3}, {n0, n1, n2, n3}, stride0, (float*)sink, -1};
  if (pf_blocks > 0 && sink == nullptr) return hipErrorInvalidValue;
  return attn_dec_launch(qkv, kc, vc, out, len_ptr, cost, sint, kS, vS, kv8,
                         scratch, cnt, split, batch, nh, kvh, hd, S, scale,
                         softcap, window, pf_blocks, pf, merge, stream);
}

extern "C" hipError_t launch_attn_dec(const void* qkv, void* kc, void* vc,
                                      void* out, const void* len_ptr,
                                      const void* cost, const void* sint,
                                      void* kS, void* vS, int kv8,
                                      void* scratch, void* cnt, int split,
                                      int batch,
                                      int nh, int kvh, int hd, int S,
                                      float scale, float softcap, int window,
                                      int merge, hipStream_t stream) {
  return attn_dec_launch(qkv, kc, vc, out, len_ptr, cost, sint, kS, vS, kv8,
                         scratch, cnt, split, batch, nh, kvh, hd, S, scale,
                         softcap, window, 0, AttnPf{}, merge, stream);
}

// ====================================================================
// MFMA flash prefill attention: one wave per (head, 16-query tile);
// iterates 16-position KV tiles with online softmax; never materializes
// QK^T.  Swapped-operand form (S^T = mfma(K, Q)) keeps each query's
// max/sum lane-local (guide App.B "swapped QK^T"); PV uses
// v_mfma_f32_16x16x16bf16_1k with O^T accumulators so the per-query
// rescale is also lane-local.  Replaces the per-query VALU scan for
// M > 1 (prefill): ~MFMA-rate QK^T/PV instead of VALU dots.
// ====================================================================

typedef short b4v __attribute__((ext_vector_type(4)));

template <int HD, bool KV8>
__global__ void __launch_bounds__(64)
k_attn_prefill_mfma(const u16* __restrict__ q, const void* __restrict__ kc,
                    const void* __restrict__ vc, u16* __restrict__ out,
                    const int* __restrict__ len_ptr,
                    const float* __restrict__ kS,
                    const float* __restrict__ vS, int M, int nh, int kvh,
                    int S, float scale, float softcap, int window) {
  constexpr int HD32 = HD / 32;
  constexpr int HD16 = HD / 16;
  const int h = blockIdx.x;
  const int qt = blockIdx.y;           // 16-query tile
  const int kvhead = h / (nh / kvh);
  const int pos0 = *len_ptr;
  const int lane = threadIdx.x & 63;
  const int qcol = lane & 15;          // this lane's query (column)
  const int krow4 = (lane >> 4) * 4;   // kv rows (QK) / k-index (PV)

  const int m0 = qt * 16;
  const int my_m = m0 + qcol;          // may be >= M (masked at store)
  const int qpos = pos0 + my_m;        // absolute position of my query

  // Q fragments (B operand): lane: col = qcol, k-chunk = (lane>>4)*8
  s8v qf[HD32];
  {
    int mr = my_m < M ? my_m : M - 1;
    const u16* qp = q + ((size_t)mr * nh + h) * HD;
#pragma unroll
    for (int c = 0; c < HD32; c++)
      qf[c] = *(const s8v*)(qp + c * 32 + (lane >> 4) * 8);
  }

  const u16* K0 = (const u16*)kc + (size_t)kvhead * S * HD;
  const u16* V0 = (const u16*)vc + (size_t)kvhead * S * HD;
  const uint8_t* K08 = (const uint8_t*)kc + (size_t)kvhead * S * HD;
  const uint8_t* V08 = (const uint8_t*)vc + (size_t)kvhead * S * HD;
  const float* kS0 = KV8 ? kS + (size_t)kvhead * S : nullptr;
  const float* vS0 = KV8 ? vS + (size_t)kvhead * S : nullptr;

  float mrun = -INFINITY, lrun = 0.f;
  f4v acc_o[HD16];
#pragma unroll
  for (int d = 0; d < HD16; d++) acc_o[d] = {0.f, 0.f, 0.f, 0.f};

  __shared__ u16 vlds[16 * HD];
  const int T_end = min(pos0 + M, pos0 + m0 + 16);  // causal upper bound
  int t_start = 0;
  if (window > 0) {
    t_start = pos0 + m0 + 1 - window;  // earliest key any tile query sees
    if (t_start < 0) t_start = 0;
  }

  for (int t0 = t_start; t0 < T_end; t0 += 16) {
    // S^T tile: A = K rows (row = lane&15, k-chunk = (lane>>4)*8)
    f4v st = {0.f, 0.f, 0.f, 0.f};
    {
      int tk = t0 + (lane & 15);
      int tkl = tk < T_end ? tk : T_end - 1;
#pragma unroll
      for (int c = 0; c < HD32; c++) {
        s8v kf;
        if (KV8)
          kf = fp8x8_to_bf16(*(const unsigned long long*)(
              K08 + (size_t)tkl * HD + c * 32 + (lane >> 4) * 8));
        else
          kf = *(const s8v*)(K0 + (size_t)tkl * HD + c * 32 +
                             (lane >> 4) * 8);
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[c], st, 0, 0, 0);
      }
    }
    // scale + softcap + causal/window mask; element (kv = t0+krow4+r, qcol)
    // KV8: each S^T output ROW is one kv position -> its k-scale folds
    // here, after the MFMA
    float sv[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      int t = t0 + krow4 + r;
      int tcl = t < T_end ? t : T_end - 1;
      float s = st[r] * (KV8 ? kS0[tcl] : 1.f) * scale;
      if (softcap > 0.f) s = softcap * tanhf(s / softcap);
      bool bad = (t > qpos) || (t >= T_end) ||
                 (window > 0 && t <= qpos - window);
      sv[r] = bad ? -INFINITY : s;
    }
    // column stats across the 4 row-groups (lanes qcol, qcol+16, ...)
    float pmax = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
    pmax = fmaxf(pmax, __shfl_xor(pmax, 16));
    pmax = fmaxf(pmax, __shfl_xor(pmax, 32));
    float mnew = fmaxf(mrun, pmax);
    float alpha = (mnew == -INFINITY) ? 0.f : __expf(mrun - mnew);
    float psum = 0.f;
    u16 pb[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      float p = (mnew == -INFINITY) ? 0.f : __expf(sv[r] - mnew);
      psum += p;
      // KV8: the v-scale of kv position t folds into the P fragment
      // (the PV MFMA's K axis mixes 16 positions, so it cannot fold
      // after the matmul)
      if (KV8) {
        int t = t0 + krow4 + r;
        int tcl = t < T_end ? t : T_end - 1;
        pb[r] = f2b(p * vS0[tcl]);
      } else {
        pb[r] = f2b(p);
      }
    }
    psum += __shfl_xor(psum, 16);
    psum += __shfl_xor(psum, 32);
    lrun = lrun * alpha + psum;
    if (mnew != -INFINITY) mrun = mnew;

    // PV: O^T[d][q] += V^T[d][kv] @ P^T[kv][q].
    // Stage the 16-row V tile in LDS with vector loads (single-wave
    // block: no barrier needed, lgkmcnt orders write->read), then
    // gather the strided V^T fragments from LDS instead of 2-byte
    // global loads (those were ~half the kernel's time).
    {
      const int vrow = lane >> 2;          // 16 rows, 4 lanes each
      int tv = t0 + vrow;
      int tvl = tv < T_end ? tv : T_end - 1;
#pragma unroll
      for (int c = 0; c < HD / 32; c++) {  // lane covers 8 cols per c
        s8v vf;
        if (KV8)
          vf = fp8x8_to_bf16(*(const unsigned long long*)(
              V08 + (size_t)tvl * HD + c * 32 + (lane & 3) * 8));
        else
          vf = *(const s8v*)(V0 + (size_t)tvl * HD + c * 32 +
                             (lane & 3) * 8);
        *(s8v*)(&vlds[vrow * HD + c * 32 + (lane & 3) * 8]) = vf;
      }
    }
    b4v pfrag = *(b4v*)pb;
#pragma unroll
    for (int db = 0; db < HD16; db++) {
      int dg = db * 16 + (lane & 15);
      u16 vt[4];
#pragma unroll
      for (int r = 0; r < 4; r++)
        vt[r] = vlds[(krow4 + r) * HD + dg];
#pragma unroll
      for (int r = 0; r < 4; r++) acc_o[db][r] *= alpha;
      acc_o[db] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
          *(b4v*)vt, pfrag, acc_o[db], 0, 0, 0);
    }
  }

  if (my_m < M) {
    float inv = 1.f / lrun;
    u16* op = out + ((size_t)my_m * nh + h) * HD;
#pragma unroll
    for (int db = 0; db < HD16; db++)
#pragma unroll
      for (int r = 0; r < 4; r++)
        op[db * 16 + krow4 + r] = f2b(acc_o[db][r] * inv);
  }
}

extern "C" hipError_t launch_attn_prefill_mfma(
    const void* q, const void* kc, const void* vc, void* out,
    const void* len_ptr, const void* kS, const void* vS, int kv8, int M,
    int nh, int kvh, int hd, int S, float scale, float softcap, int window,
    hipStream_t stream) {
  dim3 grid(nh, (M + 15) / 16);
#define APF_CASE(HDV, KV8V)                                                 \
  hipLaunchKernelGGL((k_attn_prefill_mfma<HDV, KV8V>), grid, dim3(64), 0,   \
                     stream, (const u16*)q, kc, vc, (u16*)out,              \
                     (const int*)len_ptr, (const float*)kS,                 \
                     (const float*)vS, M, nh, kvh, S, scale, softcap,       \
                     window)
  if (hd == 64) { if (kv8) APF_CASE(64, true); else APF_CASE(64, false); }
  else if (hd == 128) { if (kv8) APF_CASE(128, true); else APF_CASE(128, false); }
  else if (hd == 256) { if (kv8) APF_CASE(256, true); else APF_CASE(256, false); }
  else return hipErrorInvalidValue;
#undef APF_CASE
  return hipGetLastError();
}

extern "C" hipError_t launch_attn(const void* q, const void* kc,
                                  const void* vc, void* out,
                                  const void* len_ptr, const void* kS,
                                  const void* vS, int kv8, int M, int nh,
                                  int kvh, int hd, int S, float scale,
                                  float softcap, int window,
                                  hipStream_t stream) {
  size_t lds = (4 * hd + 8) * sizeof(float);
#define ATTN_CASE(KV8V)                                                     \
  hipLaunchKernelGGL((k_attn_t<KV8V>), dim3(nh, M), dim3(256), lds, stream, \
                     (const u16*)q, kc, vc, (u16*)out,                      \
                     (const int*)len_ptr, (const float*)kS,                 \
                     (const float*)vS, nh, kvh, hd, S, scale, softcap,      \
                     window)
  if (kv8) ATTN_CASE(true);
  else ATTN_CASE(false);
#undef ATTN_CASE
  return hipGetLastError();
}

// ====================================================================
// GLU activations: out = act(gate) * up ; act 0 = SiLU, 1 = tanh-GELU
// ====================================================================

extern "C" __global__ void __launch_bounds__(256)
k_glu(const u16* __restrict__ gate, const u16* __restrict__ up,
      u16* __restrict__ out, long total, int act) {
  long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i >= total) return;
  s8v g = *(const s8v*)(gate + i);
  s8v u = *(const s8v*)(up + i);
  u16 o[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    float x = b2f(((u16*)&g)[j]);
    float a;
    if (act == 0) {
      a = x / (1.f + __expf(-x));
    } else {
      float c = 0.7978845608028654f * (x + 0.044715f * x * x * x);
      a = 0.5f * x * (1.f + tanhf(c));
    }
    o[j] = f2b(a * b2f(((u16*)&u)[j]));
  }
  *(s8v*)(out + i) = *(s8v*)o;
}

extern "C" hipError_t launch_glu(const void* gate, const void* up, void* out,
                                 long total, int act, hipStream_t stream) {
  long blocks = (total / 8 + 255) / 256;
  hipLaunchKernelGGL(k_glu, dim3((uint32_t)blocks), dim3(256), 0, stream,
                     (const u16*)gate, (const u16*)up, (u16*)out, total, act);
  return hipGetLastError();
}

// ====================================================================
// Embedding gather: h[m] = embed[ids[m]] * scale  (ids live on device so
// the decode graph can feed back the sampled token without host sync)
// ====================================================================

extern "C" __global__ void __launch_bounds__(256)
k_embed(const u16* __restrict__ embed, const int* __restrict__ ids,
        u16* __restrict__ out, int H, float scale) {
  const int m = blockIdx.x;
  const int id = ids[m];
  const u16* src = embed + (size_t)id * H;
  u16* dst = out + (size_t)m * H;
  for (int i = threadIdx.x * 8; i < H; i += 2048) {
    s8v v = *(const s8v*)(src + i);
    u16 o[8];
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = f2b(b2f(((u16*)&v)[j]) * scale);
    *(s8v*)(dst + i) = *(s8v*)o;
  }
}

extern "C" hipError_t launch_embed(const void* embed, const void* ids,
                                   void* out, int M, int H, float scale,
                                   hipStream_t stream) {
  hipLaunchKernelGGL(k_embed, dim3(M), dim3(256), 0, stream,
                     (const u16*)embed, (const int*)ids, (u16*)out, H, scale);
  return hipGetLastError();
}

// ====================================================================
// Sampling: greedy argmax or min-p + Gumbel-argmax multinomial.
//   keep tokens with p >= min_p * p_max  <=>  logit >= max + ln(min_p);
//   winner = argmax over kept of (logit + Gumbel noise).
// top-k / top-p: the same pick over {fkey(logit) >= tau}, tau found by
// the k_sample_select radix select (launch_sample_sel).
// Writes the token to *next_token (feeds the next decode graph step),
// appends to out_ring, bumps *len_ptr and *nout — all device-side, so the
// whole decode step is graph-replayable.
// ====================================================================

DEVINL uint32_t hash32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// order-preserving float->u32 key (monotone for max); invertible
DEVINL uint32_t fkey(float f) {
  union { float f; uint32_t u; } c; c.f = f;
  return (c.u & 0x80000000u) ? ~c.u : (c.u ^ 0x80000000u);
}
DEVINL float fkey_inv(uint32_t k) {
  union { float f; uint32_t u; } c;
  c.u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
  return c.f;
}

// pack (key, idx): ties prefer the SMALLEST index (matches np.argmax)
DEVINL uint64_t pack_ki(uint32_t key, int idx) {
  return ((uint64_t)key << 32) | (uint32_t)(0x7fffffff - idx);
}
DEVINL int unpack_idx(uint64_t p) { return 0x7fffffff - (int)(uint32_t)p; }

// pass 1 (min-p only): global max logit -> gmax[b] (packed).
// Batched: grid.y = sequence row b (lbf16: logits stored bf16 — the
// batched lm_head GEMM path emits bf16 rows).
// Grid-wide visit of one logits row: f(i, value) once per element.  Whole
// 16-B vectors (4 fp32 / 8 bf16) go grid-stride, the tail behind the last
// whole vector scalar; a row whose base is not 16-B aligned (rows of a
// batch with V off the vector size) is scalar throughout.  What f does
// with an element depends on its index and value alone, so the visiting
// order is free.
template <typename F>
DEVINL void logits_scan(const float* __restrict__ lf,
                        const u16* __restrict__ lh, int V, int lbf16, F f) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int nt = gridDim.x * 256;
  int done = 0;
  if (lbf16) {
    if (((uintptr_t)lh & 15) == 0) {
      const int nv = V >> 3;
      for (int k = t; k < nv; k += nt) {
        s8v x = ((const s8v*)lh)[k];
#pragma unroll
        for (int j = 0; j < 8; j++) f(k * 8 + j, b2f(((u16*)&x)[j]));
      }
      done = nv << 3;
    }
    for (int i = done + t; i < V; i += nt) f(i, b2f(lh[i]));
  } else {
    if (((uintptr_t)lf & 15) == 0) {
      const int nv = V >> 2;
      for (int k = t; k < nv; k += nt) {
        f4v x = ((const f4v*)lf)[k];
#pragma unroll
        for (int j = 0; j < 4; j++) f(k * 4 + j, x[j]);
      }
      done = nv << 2;
    }
    for (int i = done + t; i < V; i += nt) f(i, lf[i]);
  }
}

DEVINL void logit_max_body(const void* __restrict__ logits, int V, int lbf16,
                           unsigned long long* __restrict__ gmax) {
  const int b = blockIdx.y;
  gmax += b;
  const float* lf = (const float*)logits + (size_t)b * V;
  const u16* lh = (const u16*)logits + (size_t)b * V;
  float mv = -INFINITY;
  int mi = 0;
  logits_scan(lf, lh, V, lbf16, [&](int i, float v) {
    if (v > mv || (v == mv && i < mi)) { mv = v; mi = i; }
  });
  uint64_t pk = pack_ki(fkey(mv), mi);
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) {
    uint64_t o = __shfl_xor((unsigned long long)pk, w);
    if (o > pk) pk = o;
  }
  __shared__ unsigned long long ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = pk;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t b = ws[0];
    for (int w = 1; w < 4; w++) if (ws[w] > b) b = ws[w];
    atomicMax(gmax, (unsigned long long)b);
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_logit_max(const void* __restrict__ logits, int V, int lbf16,
            unsigned long long* __restrict__ gmax,
            uint64_t* __restrict__ ctr) {
  // advance the shared RNG counter HERE: stream order guarantees every
  // k_sample_pick block then reads the same post-bump value (bumping
  // from pick's commit raced with straggler blocks still reading it)
  if (ctr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
    *ctr += 1;
  logit_max_body(logits, V, lbf16, gmax);
}

// Per-row sampler table `samp` [rows, SAMP_WORDS] u32: the sampler's
// parameters as device DATA, so rows with different strategies /
// temperatures / seeds share one launch sequence and one captured graph.
#define SAMP_MODE 0  // 0 greedy, 1 min-p cut, 2 top-k, 3 top-p
#define SAMP_INVT 1  // fp32 1 / temperature
#define SAMP_MINP 2  // fp32 (mode 1; 0 = plain temperature sampling;
                     // modes 2 / 3: > 0 = a min-p cut on top of tau)
#define SAMP_TOPK 3  // int, 1..V (mode 2)
#define SAMP_TOPP 4  // fp32 (mode 3; mode 2: < 1 = top-p WITHIN the top-k
                     // survivors, the second select phase)
#define SAMP_SEED 5  // 5, 6: the row's 64-bit seed (lo, hi)
#define SAMP_CTR 7   // draws so far: zeroed by the host, advanced here
#define SAMP_WORDS 8

// k_logit_max per row of `samp`: each row's own draw counter advances
// (same stream-order argument as above); the shared counter is not used.
extern "C" __global__ void __launch_bounds__(256)
k_logit_max_rows(const void* __restrict__ logits, int V, int lbf16,
                 unsigned long long* __restrict__ gmax, uint32_t* samp) {
  if (blockIdx.x == 0 && threadIdx.x == 0)
    samp[(size_t)blockIdx.y * SAMP_WORDS + SAMP_CTR] += 1u;
  logit_max_body(logits, V, lbf16, gmax);
}

// pass 2: winner = argmax over kept tokens of (logit/T [+ Gumbel]) -> *pick,
// and the LAST-arriving block (G16 ticket) commits it: write *next_token,
// append to out_ring, bump len/ctr, re-zero the scratch — the former
// k_sample_fin's 1-thread launch (~4 us) folded away.
// Temperature folds into both the min-p keep-set and the Gumbel score:
//   p_i(T) >= min_p * p_max(T)  <=>  l_i >= l_max + T*ln(min_p)
//   Gumbel-argmax over p(T)     <=>  argmax of l_i/T + G_i
// SEL: the keep-set cut comes from the selection stage (k_sample_select)
// as an fkey in sel[SEL_TAU] instead of the min-p expression; compared in
// key space so the kept set is exactly the one the radix select counted.
#define SEL_TAU 0     // out: threshold key tau (armed 0 = keep everything)
#define SEL_PREFIX 1  // key bits fixed by the passes so far
#define SEL_TARGET 2  // count / fixed-point mass still to cover in-bin
#define SEL_TICKET 3  // last-arriver ticket of the running pass
#define SEL_HIST 4    // 256-bin u64 histogram (count or fixed-point mass)
#define SEL_WORDS 260

// block winner (bv, bi) -> *pick; the last-arriving block commits.  All
// pointers are the ROW's own except next_token / len_ptr (indexed by b);
// sel != nullptr: the row ran the selection stage, re-arm its result words.
DEVINL void sample_pick_commit(
    float bv, int bi, int V, unsigned long long* __restrict__ gmax,
    unsigned long long* __restrict__ pick, int* __restrict__ cnt,
    int* __restrict__ next_token, int* __restrict__ out_ring,
    int* __restrict__ nout, int* __restrict__ len_ptr, int bump_len,
    unsigned long long* __restrict__ sel) {
  const int b = blockIdx.y;
  uint64_t pk = pack_ki(fkey(bv), bi);
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) {
    uint64_t o = __shfl_xor((unsigned long long)pk, w);
    if (o > pk) pk = o;
  }
  __shared__ unsigned long long ws[4];
  __shared__ int lastflag;
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = pk;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t b = ws[0];
    for (int w = 1; w < 4; w++) if (ws[w] > b) b = ws[w];
    atomicMax(pick, (unsigned long long)b);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    int t = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_ACQ_REL,
                                   __HIP_MEMORY_SCOPE_AGENT);
    lastflag = (t == (int)gridDim.x - 1);
  }
  __syncthreads();
  if (!lastflag || threadIdx.x != 0) return;
  // last arriver: commit the winner, reset scratch, advance state
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  *cnt = 0;
  int winner = unpack_idx(
      __hip_atomic_load(pick, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  if (winner < 0 || winner >= V) winner = 0;  // NaN-logit insurance
  next_token[b] = winner;
  int n = *nout;
  out_ring[n] = winner;
  *nout = n + 1;
  // per-row position advances (ragged batch); the shared RNG counter
  // was already advanced by k_logit_max ahead of this kernel
  if (bump_len) len_ptr[b] += 1;
  *pick = 0ull;
  *gmax = 0ull;
  if (sel) {
    sel[SEL_TAU] = 0ull;
    sel[SEL_PREFIX] = 0ull;
    sel[SEL_TARGET] = 0ull;
  }
}

template <bool SEL>
DEVINL void sample_pick_body(
    const void* __restrict__ logits, int V, int lbf16,
    long ring_stride, float min_p,
    int greedy, uint64_t seed, float inv_temp,
    unsigned long long* __restrict__ gmax,
    uint64_t* __restrict__ ctr,
    unsigned long long* __restrict__ pick,
    int* __restrict__ cnt, int* __restrict__ next_token,
    int* __restrict__ out_ring, int* __restrict__ nout,
    int* __restrict__ len_ptr, int bump_len,
    unsigned long long* __restrict__ sel) {
  const int b = blockIdx.y;
  gmax += b; pick += b; cnt += b; nout += b;
  out_ring += (size_t)b * ring_stride;
  const float* lf = (const float*)logits + (size_t)b * V;
  const u16* lh = (const u16*)logits + (size_t)b * V;
  float thresh = -INFINITY;
  uint32_t tau = 0;
  if (SEL) {
    sel += (size_t)b * SEL_WORDS;
    tau = (uint32_t)sel[SEL_TAU];
  } else if (!greedy) {
    thresh = fkey_inv((uint32_t)(*gmax >> 32)) + __logf(min_p) / inv_temp;
  }
  const uint32_t c = (uint32_t)(*ctr) ^ ((uint32_t)b * 0x85ebca6bu);
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  logits_scan(lf, lh, V, lbf16, [&](int i, float v) {
    if (SEL ? (fkey(v) < tau) : (v < thresh)) return;
    float sc = v;
    if (!greedy) {
      uint32_t r = hash32(hash32((uint32_t)i ^ (c * 0x9e3779b9u)) ^
                          (uint32_t)seed);
      float u = (r + 1.0f) * 2.3283064e-10f;  // (0,1]
      sc = v * inv_temp - __logf(-__logf(u));
    }
    if (sc > bv || (sc == bv && i < bi)) { bv = sc; bi = i; }
  });
  sample_pick_commit(bv, bi, V, gmax, pick, cnt, next_token, out_ring, nout,
                     len_ptr, bump_len, SEL ? sel : nullptr);
}

extern "C" __global__ void __launch_bounds__(256)
k_sample_pick(const void* __restrict__ logits, int V, int lbf16,
              long ring_stride, float min_p,
              int greedy, uint64_t seed, float inv_temp,
              unsigned long long* __restrict__ gmax,
              uint64_t* __restrict__ ctr,
              unsigned long long* __restrict__ pick,
              int* __restrict__ cnt, int* __restrict__ next_token,
              int* __restrict__ out_ring, int* __restrict__ nout,
              int* __restrict__ len_ptr, int bump_len) {
  sample_pick_body<false>(logits, V, lbf16, ring_stride, min_p, greedy, seed,
                          inv_temp, gmax, ctr, pick, cnt, next_token,
                          out_ring, nout, len_ptr, bump_len, nullptr);
}

// top-k / top-p variant: same Gumbel pick, keep-set = {fkey(l) >= tau}
extern "C" __global__ void __launch_bounds__(256)
k_sample_pick_sel(const void* __restrict__ logits, int V, int lbf16,
                  long ring_stride, uint64_t seed, float inv_temp,
                  unsigned long long* __restrict__ gmax,
                  uint64_t* __restrict__ ctr,
                  unsigned long long* __restrict__ pick,
                  int* __restrict__ cnt, int* __restrict__ next_token,
                  int* __restrict__ out_ring, int* __restrict__ nout,
                  int* __restrict__ len_ptr, int bump_len,
                  unsigned long long* __restrict__ sel) {
  sample_pick_body<true>(logits, V, lbf16, ring_stride, 0.0f, 0, seed,
                         inv_temp, gmax, ctr, pick, cnt, next_token,
                         out_ring, nout, len_ptr, bump_len, sel);
}

// Per-row variant: mode, temperature, cut and seed come from samp[b], so
// one launch serves rows of every strategy.  Keep-set per mode: 0 all
// (plain argmax), 1 the min-p expression of k_sample_pick, 2 / 3
// {fkey(l) >= tau} with tau from k_sample_select_rows, intersected with
// the min-p expression where the row carries min_p > 0 (composed rows):
// fkey is monotone, so l >= cut is fkey(l) >= fkey(cut) and the two cuts
// fold into one key, tau = max(tau, fkey(cut)).  The noise of
// element i is a function of (i, row seed, row counter) alone — neither
// the slot b nor a shared counter enters — so a request's stream does not
// depend on where it sits or on what its neighbours do.  MINP: the
// variant that reads the min-p word of selected rows, launched only when
// the host says such a row is present, so groups of today's modes run the
// code they ran (a kernel template, not a shared inline body: the
// arguments keep their __restrict__ as kernel arguments).
template <bool MINP>
__global__ void __launch_bounds__(256)
k_sample_pick_rows(const void* __restrict__ logits, int V, int lbf16,
                   long ring_stride, const uint32_t* __restrict__ samp,
                   unsigned long long* __restrict__ gmax,
                   unsigned long long* __restrict__ pick,
                   int* __restrict__ cnt, int* __restrict__ next_token,
                   int* __restrict__ out_ring, int* __restrict__ nout,
                   int* __restrict__ len_ptr, int bump_len,
                   unsigned long long* __restrict__ sel) {
  const int b = blockIdx.y;
  gmax += b; pick += b; cnt += b; nout += b;
  out_ring += (size_t)b * ring_stride;
  sel += (size_t)b * SEL_WORDS;
  samp += (size_t)b * SAMP_WORDS;
  const float* lf = (const float*)logits + (size_t)b * V;
  const u16* lh = (const u16*)logits + (size_t)b * V;
  const uint32_t mode = samp[SAMP_MODE];
  const float inv_temp = __uint_as_float(samp[SAMP_INVT]);
  const bool greedy = mode == 0u;
  const bool selected = mode >= 2u;
  float thresh = -INFINITY;
  uint32_t tau = 0;
  if (selected)
    tau = (uint32_t)sel[SEL_TAU];
  else if (!greedy)
    thresh = fkey_inv((uint32_t)(*gmax >> 32)) +
             __logf(__uint_as_float(samp[SAMP_MINP])) / inv_temp;
  if (MINP && selected) {
    const float min_p = __uint_as_float(samp[SAMP_MINP]);
    if (min_p > 0.0f) {
      float cut = fkey_inv((uint32_t)(*gmax >> 32)) + __logf(min_p) / inv_temp;
      if (cut == 0.0f) cut = -0.0f;  // -0 >= +0, but fkey(-0) < fkey(+0)
      const uint32_t kc = fkey(cut);
      if (kc > tau) tau = kc;
    }
  }
  // two per-draw keys: k0 mixes counter and seed lo, k1 adds seed hi
  const uint32_t k0 =
      hash32(hash32(samp[SAMP_CTR] ^ 0x9e3779b9u) ^ samp[SAMP_SEED]);
  const uint32_t k1 = hash32(k0 ^ samp[SAMP_SEED + 1] ^ 0x85ebca6bu);
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  logits_scan(lf, lh, V, lbf16, [&](int i, float v) {
    if (selected ? (fkey(v) < tau) : (v < thresh)) return;
    float sc = v;
    if (!greedy) {
      uint32_t r = hash32(hash32((uint32_t)i ^ k0) ^ k1);
      float u = (r + 1.0f) * 2.3283064e-10f;  // (0,1]
      sc = v * inv_temp - __logf(-__logf(u));
    }
    if (sc > bv || (sc == bv && i < bi)) { bv = sc; bi = i; }
  });
  sample_pick_commit(bv, bi, V, gmax, pick, cnt, next_token, out_ring, nout,
                     len_ptr, bump_len, selected ? sel : nullptr);
}

// Selection stage for top-k / top-p: one pass of an MSB-first radix
// select over fkey(logit), 8 bits per pass (launched 4x: shift 24,16,8,0;
// bf16 rows 2x: their keys' low 16 bits are zero, so bin 0 is known).
// Both filters are "smallest suffix of the sorted row whose WEIGHT reaches
// a target": weight 1 / target k for top-k; weight
// w_i = exp((l_i - l_max) * inv_temp) in 2^40 fixed point / target
// ceil(top_p * sum w) for top-p (integers: the sums do not depend on the
// order the atomics arrive in, so tau is reproducible).  Each block
// histograms the elements whose key matches the prefix found so far into
// LDS, merges the non-empty bins into the row's global histogram, and the
// last-arriving block (ticket) suffix-scans the 256 bins, descends into
// the bin holding the boundary and re-zeroes histogram + ticket.  After
// the `last` pass the prefix is the threshold key tau (ties at tau are
// kept).  A row that cannot reach its target (all-NaN / zero mass) falls
// to bin 0 every pass: tau = 0 keeps everything, nothing loops.
//
// Composed top-k -> top-p (per-row sampler only) is two such descents.
// Phase 1 is the count descent, unchanged; its last pass leaves tau_k in
// SEL_TAU and in SEL_PREFIX.  Phase 2 (PHASE2) is the mass descent over
// the WHOLE row, with the first-pass target ceil(top_p * M_k), M_k = the
// fixed-point mass of {key >= tau_k}: the first pass sums M_k ON TOP of
// the tau_k in SEL_PREFIX beside its histogram (a first pass reads no
// prefix and only writes that word at its end, from the last arriver,
// which subtracts tau_k again).  The same integer weights feed M_k and
// the bins, so the suffix at tau_k holds exactly M_k >= target and the
// descent ends at tau >= tau_k: no restriction to the survivors is
// needed.
template <bool PHASE2>
DEVINL void sample_select_body(
    const void* __restrict__ logits, int V, int lbf16,
    int top_k, float top_p, float inv_temp, int shift,
    int last, const unsigned long long* __restrict__ gmax,
    unsigned long long* __restrict__ sel) {
  const int b = blockIdx.y;
  const int t = threadIdx.x;
  sel += (size_t)b * SEL_WORDS;
  unsigned long long* hist = sel + SEL_HIST;
  const float* lf = (const float*)logits + (size_t)b * V;
  const u16* lh = (const u16*)logits + (size_t)b * V;
  __shared__ unsigned long long sh[256];
  __shared__ unsigned long long shm;  // PHASE2, first pass: block's M_k
  __shared__ int lastflag;
  sh[t] = 0ull;
  if (PHASE2 && t == 0) shm = 0ull;
  __syncthreads();
  const bool first = shift == 24;
  const uint32_t tau_k = (PHASE2 && first) ? (uint32_t)sel[SEL_TAU] : 0u;
  unsigned long long mk = 0ull;
  const uint32_t prefix = first ? 0u : (uint32_t)sel[SEL_PREFIX];
  const uint32_t himask = first ? 0u : (0xffffffffu << (shift + 8));
  const float lmax = fkey_inv((uint32_t)(gmax[b] >> 32));
  for (int i = blockIdx.x * 256 + t; i < V; i += gridDim.x * 256) {
    float v = lbf16 ? b2f(lh[i]) : lf[i];
    uint32_t key = fkey(v);
    if ((key & himask) != prefix) continue;
    unsigned long long w = 1ull;
    if (top_k == 0) {
      float e = __expf((v - lmax) * inv_temp);
      e = e >= 0.0f ? fminf(e, 1.0f) : 0.0f;  // NaN -> 0
      w = (unsigned long long)(e * 1099511627776.0f);  // 2^40
    }
    if (w) atomicAdd(&sh[(key >> shift) & 255u], w);
    if (PHASE2 && first && key >= tau_k) mk += w;
  }
  if (PHASE2 && mk) atomicAdd(&shm, mk);
  __syncthreads();
  // wave 0 merges all 256 bins, so ONE wave's release fence (an L2
  // write-back) orders the whole block's contribution ahead of its
  // ticket: measured 16 us/pass at B=8, 27 us when every wave fenced
  // (profiles/sampler_select.md)
  if (t < 64) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      unsigned long long hj = sh[t + 64 * j];
      if (hj)
        __hip_atomic_fetch_add(&hist[t + 64 * j], hj, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    if (PHASE2 && first && t == 0 && shm)
      __hip_atomic_fetch_add(&sel[SEL_PREFIX], shm, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (t == 0) {
      unsigned long long tk = __hip_atomic_fetch_add(
          &sel[SEL_TICKET], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      lastflag = (tk == (unsigned long long)gridDim.x - 1);
    }
  }
  __syncthreads();
  if (!lastflag) return;
  // last arriver: every block's bins are in; scan, descend, re-arm
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  unsigned long long h =
      __hip_atomic_load(&hist[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  hist[t] = 0ull;
  if (t == 0) sel[SEL_TICKET] = 0ull;
  sh[t] = h;
  __syncthreads();
  // inclusive suffix sums: sh[t] = weight of all keys in bins >= t
  for (int off = 1; off < 256; off <<= 1) {
    unsigned long long a = (t + off < 256) ? sh[t + off] : 0ull;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  unsigned long long target;
  if (!first) {
    target = sel[SEL_TARGET];
  } else if (PHASE2) {
    const unsigned long long m_k =
        __hip_atomic_load(&sel[SEL_PREFIX], __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT) - tau_k;
    target = (unsigned long long)ceil((double)top_p * (double)m_k);
    if (target == 0ull) target = 1ull;
  } else if (top_k > 0) {
    target = (unsigned long long)top_k;
  } else {
    target = (unsigned long long)ceil((double)top_p * (double)sh[0]);
    if (target == 0ull) target = 1ull;
  }
  __syncthreads();  // everyone holds the old target before it is replaced
  const unsigned long long above = (t < 255) ? sh[t + 1] : 0ull;
  // exactly one bin: the highest whose suffix reaches the target (bin 0
  // when none does)
  if (above < target && (t == 0 || sh[t] >= target)) {
    const uint32_t p = prefix | ((uint32_t)t << shift);
    sel[SEL_PREFIX] = p;
    sel[SEL_TARGET] = target - above;
    if (last) sel[SEL_TAU] = p;
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_sample_select(const void* __restrict__ logits, int V, int lbf16,
                int top_k, float top_p, float inv_temp, int shift,
                int last, const unsigned long long* __restrict__ gmax,
                unsigned long long* __restrict__ sel) {
  sample_select_body<false>(logits, V, lbf16, top_k, top_p, inv_temp, shift,
                            last, gmax, sel);
}

// Per-row variant: weight and first-pass target follow samp[b]'s mode
// (2: count / top_k, 3: fixed-point mass / top_p at the row's own
// temperature), so top-k and top-p rows share the same passes.  A row in
// mode 0 / 1 returns at once: neither its sel words nor its ticket are
// touched (the whole block leaves, so no barrier is left waiting).
extern "C" __global__ void __launch_bounds__(256)
k_sample_select_rows(const void* __restrict__ logits, int V, int lbf16,
                     const uint32_t* __restrict__ samp, int shift, int last,
                     const unsigned long long* __restrict__ gmax,
                     unsigned long long* __restrict__ sel) {
  samp += (size_t)blockIdx.y * SAMP_WORDS;
  const uint32_t mode = samp[SAMP_MODE];
  if (mode < 2u) return;
  sample_select_body<false>(logits, V, lbf16,
                            mode == 2u ? (int)samp[SAMP_TOPK] : 0,
                            __uint_as_float(samp[SAMP_TOPP]),
                            __uint_as_float(samp[SAMP_INVT]), shift, last,
                            gmax, sel);
}

// Second select phase of composed rows (mode 2 with top_p < 1): the mass
// descent whose first-pass target is top_p of the top-k survivors' mass.
// Launched only when the host says such a row is present; every other row
// returns at once and keeps the tau phase 1 gave it.
extern "C" __global__ void __launch_bounds__(256)
k_sample_select_rows2(const void* __restrict__ logits, int V, int lbf16,
                      const uint32_t* __restrict__ samp, int shift, int last,
                      const unsigned long long* __restrict__ gmax,
                      unsigned long long* __restrict__ sel) {
  samp += (size_t)blockIdx.y * SAMP_WORDS;
  const float top_p = __uint_as_float(samp[SAMP_TOPP]);
  if (samp[SAMP_MODE] != 2u || !(top_p < 1.0f)) return;
  sample_select_body<true>(logits, V, lbf16, 0, top_p,
                           __uint_as_float(samp[SAMP_INVT]), shift, last,
                           gmax, sel);
}

// Blocks per row of the launches whose blocks end in atomics on one word
// per row (k_logit_max*: atomicMax; k_sample_pick*: atomicMax + returning
// ticket).  Those serialize at 11-13 ns each, so the block count is the
// kernel's duration once it is in the hundreds: one block per
// SAMPLE_PICK_SPAN elements (one 16-B fp32 load per thread), at most
// SAMPLE_PICK_CAP (profiles/attn_inblock_merge.md has the sweep).
// `blocks` > 0 overrides.  Any count gives the same winner: it is defined
// over element indices.
constexpr int SAMPLE_PICK_SPAN = 1024;
constexpr int SAMPLE_PICK_CAP = 64;
static int sample_pick_blocks(int V, int batch, int blocks) {
  if (blocks > 0) return blocks;
  blocks = (V + SAMPLE_PICK_SPAN - 1) / SAMPLE_PICK_SPAN;
  if (blocks > SAMPLE_PICK_CAP) blocks = SAMPLE_PICK_CAP;
  // batched rows: keep TOTAL thread count constant (the B=8 sampler
  // measured 102 us with a full grid per row, and 10 us at 16 blocks
  // per row against 15 at 64)
  if (batch > 1) {
    const int floor_ = blocks < 16 ? blocks : 16;
    blocks = blocks / batch + 1;
    if (blocks < floor_) blocks = floor_;
  }
  return blocks < 1 ? 1 : blocks;
}

extern "C" hipError_t launch_sample(const void* logits, int V, int lbf16,
                                    int batch, long ring_stride, float min_p,
                                    int greedy, uint64_t seed, float inv_temp,
                                    void* ctr, void* gmax, void* pick,
                                    void* cnt, void* next_token,
                                    void* out_ring, void* nout,
                                    void* len_ptr, int bump_len, int blocks,
                                    hipStream_t stream) {
  if (blocks < 0 || blocks > 65535) return hipErrorInvalidValue;
  blocks = sample_pick_blocks(V, batch, blocks);
  if (!greedy)
    hipLaunchKernelGGL(k_logit_max, dim3(blocks, batch), dim3(256), 0,
                       stream, logits, V, lbf16, (unsigned long long*)gmax,
                       (uint64_t*)ctr);
  hipLaunchKernelGGL(k_sample_pick, dim3(blocks, batch), dim3(256), 0,
                     stream, logits, V, lbf16, ring_stride, min_p, greedy,
                     seed, inv_temp,
                     (unsigned long long*)gmax, (uint64_t*)ctr,
                     (unsigned long long*)pick, (int*)cnt, (int*)next_token,
                     (int*)out_ring, (int*)nout, (int*)len_ptr, bump_len);
  return hipGetLastError();
}

// launch_sample + device-side top-k / top-p.  top_k > 0: keep the k
// largest logits (ties at the k-th kept); else top_p < 1: keep the
// smallest highest-probability prefix whose mass reaches top_p; neither
// (or greedy): exactly launch_sample.  sel: SEL_WORDS u64 per row,
// zeroed once, re-armed on device.
extern "C" hipError_t launch_sample_sel(
    const void* logits, int V, int lbf16, int batch, long ring_stride,
    float min_p, int greedy, uint64_t seed, float inv_temp, void* ctr,
    void* gmax, void* pick, void* cnt, void* next_token, void* out_ring,
    void* nout, void* len_ptr, int bump_len, int top_k, float top_p,
    void* sel, hipStream_t stream) {
  if (greedy || (top_k <= 0 && !(top_p < 1.0f)))
    return launch_sample(logits, V, lbf16, batch, ring_stride, min_p, greedy,
                         seed, inv_temp, ctr, gmax, pick, cnt, next_token,
                         out_ring, nout, len_ptr, bump_len, 0, stream);
  if (top_k > V) top_k = V;
  const int blocks = sample_pick_blocks(V, batch, 0);
  // few blocks per row: every block merges its bins into the same handful
  // of hot histogram words, so the merge cost grows with the block count
  int sblocks = (V + 2047) / 2048;
  if (sblocks > 64) sblocks = 64;
  hipLaunchKernelGGL(k_logit_max, dim3(blocks, batch), dim3(256), 0, stream,
                     logits, V, lbf16, (unsigned long long*)gmax,
                     (uint64_t*)ctr);
  const int last_shift = lbf16 ? 16 : 0;
  for (int shift = 24; shift >= last_shift; shift -= 8)
    hipLaunchKernelGGL(k_sample_select, dim3(sblocks, batch), dim3(256), 0,
                       stream, logits, V, lbf16, top_k, top_p, inv_temp,
                       shift, shift == last_shift ? 1 : 0,
                       (const unsigned long long*)gmax,
                       (unsigned long long*)sel);
  hipLaunchKernelGGL(k_sample_pick_sel, dim3(blocks, batch), dim3(256), 0,
                     stream, logits, V, lbf16, ring_stride, seed, inv_temp,
                     (unsigned long long*)gmax, (uint64_t*)ctr,
                     (unsigned long long*)pick, (int*)cnt, (int*)next_token,
                     (int*)out_ring, (int*)nout, (int*)len_ptr, bump_len,
                     (unsigned long long*)sel);
  return hipGetLastError();
}

// Sampler driven by the per-row table `samp` ([batch, SAMP_WORDS] u32).
// The host knows the union of the rows' modes and launches only what it
// needs, with the grids of launch_sample / launch_sample_sel:
//   no sampled row (all mode 0):   k_sample_pick greedy — exactly the
//                                  launch_sample greedy launch
//   no row in mode 2 / 3:          max + pick
//   else:                          max + 4 (bf16: 2) select passes + pick
//   chain & 1 (a mode-2 row with   the same, with 4 (bf16: 2) phase-2
//   top_p < 1 is present):         passes between select and pick
//   chain & 2 (a mode-2 / 3 row    the pick is the variant that reads the
//   with min_p > 0 is present):    rows' min-p word
// so a uniform group costs the launches it costs through the legacy
// launchers.  A row whose mode the flags do not cover is a host error
// (its keep-set would be the whole row).
extern "C" hipError_t launch_sample_rows(
    const void* logits, int V, int lbf16, int batch, long ring_stride,
    void* samp, int any_sampled, int any_select, int chain, void* gmax,
    void* pick, void* cnt, void* next_token, void* out_ring, void* nout,
    void* len_ptr, int bump_len, void* sel, hipStream_t stream) {
  const int blocks = sample_pick_blocks(V, batch, 0);
  if (!any_sampled && !any_select) {
    // greedy reads neither seed nor counter value; `samp` only stands in
    // as a readable 8-byte word for the kernel's counter load
    hipLaunchKernelGGL(k_sample_pick, dim3(blocks, batch), dim3(256), 0,
                       stream, logits, V, lbf16, ring_stride, 0.0f, 1,
                       (uint64_t)0, 1.0f, (unsigned long long*)gmax,
                       (uint64_t*)samp, (unsigned long long*)pick, (int*)cnt,
                       (int*)next_token, (int*)out_ring, (int*)nout,
                       (int*)len_ptr, bump_len);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_logit_max_rows, dim3(blocks, batch), dim3(256), 0,
                     stream, logits, V, lbf16, (unsigned long long*)gmax,
                     (uint32_t*)samp);
  if (any_select) {
    int sblocks = (V + 2047) / 2048;
    if (sblocks > 64) sblocks = 64;
    const int last_shift = lbf16 ? 16 : 0;
    for (int shift = 24; shift >= last_shift; shift -= 8)
      hipLaunchKernelGGL(k_sample_select_rows, dim3(sblocks, batch),
                         dim3(256), 0, stream, logits, V, lbf16,
                         (const uint32_t*)samp, shift,
                         shift == last_shift ? 1 : 0,
                         (const unsigned long long*)gmax,
                         (unsigned long long*)sel);
    if (chain & 1)
      for (int shift = 24; shift >= last_shift; shift -= 8)
        hipLaunchKernelGGL(k_sample_select_rows2, dim3(sblocks, batch),
                           dim3(256), 0, stream, logits, V, lbf16,
                           (const uint32_t*)samp, shift,
                           shift == last_shift ? 1 : 0,
                           (const unsigned long long*)gmax,
                           (unsigned long long*)sel);
  }
  hipLaunchKernelGGL((chain & 2) ? k_sample_pick_rows<true>
                                 : k_sample_pick_rows<false>,
                     dim3(blocks, batch), dim3(256), 0,
                     stream, logits, V, lbf16, ring_stride,
                     (const uint32_t*)samp, (unsigned long long*)gmax,
                     (unsigned long long*)pick, (int*)cnt, (int*)next_token,
                     (int*)out_ring, (int*)nout, (int*)len_ptr, bump_len,
                     (unsigned long long*)sel);
  return hipGetLastError();
}

// ====================================================================
// Logit processors: repetition / frequency / presence penalties and
// logit_bias, applied IN PLACE to the logits row the sampler reads next
// (after the lm_head's softcap, before temperature / any filter).
// Per-row device state, so rows with different settings share one graph:
//   stat [rows, V] i32  bit 30 (TOKSTAT_PROMPT): id occurs in the prompt;
//                       low 30 bits: times the id was generated
//   proc [rows, 4] f32  {repetition r, frequency f, presence p, bias_on}
//   bias [rows, V] f32  dense logit_bias (read only when bias_on != 0)
// Order per element i (runtime/sampling.py apply_logit_processors):
//   stat != 0:  l = l > 0 ? l / r : l * r
//   count c>0:  l -= f * c + p
//   bias_on:    l += bias[i]
// ====================================================================
#define TOKSTAT_PROMPT 0x40000000
#define TOKSTAT_COUNT 0x3fffffff

// prompt ids -> flag words of one freshly zeroed stat row.  Every writer
// of a word stores the same value, so duplicates need no atomics.
extern "C" __global__ void __launch_bounds__(256)
k_tokstat_mark(int* __restrict__ stat_row, const int* __restrict__ ids,
               int n, int V) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int t = ids[i];
    if (t >= 0 && t < V) stat_row[t] = TOKSTAT_PROMPT;
  }
}

DEVINL float logit_adjust_val(float l, int s, float r, float f, float p,
                              float bv) {
  if (s != 0) {
    l = l > 0.0f ? l / r : l * r;
    const int c = s & TOKSTAT_COUNT;
    if (c) l -= f * (float)c + p;
  }
  return l + bv;
}

// one element, any alignment: row heads / tails and misaligned rows
template <bool BF>
DEVINL void logit_adjust_elem(void* lrow, int* srow, const float* brow,
                              int i, int tok, float r, float f, float p,
                              bool bias_on) {
  int s = srow[i];
  if (i == tok) { s += 1; srow[i] = s; }
  const float bv = bias_on ? brow[i] : 0.0f;
  if (s == 0 && bv == 0.0f) return;
  if (BF) {
    u16* lh = (u16*)lrow;
    lh[i] = f2b(logit_adjust_val(b2f(lh[i]), s, r, f, p, bv));
  } else {
    float* lf = (float*)lrow;
    lf[i] = logit_adjust_val(lf[i], s, r, f, p, bv);
  }
}

// The dense pass over stat doubles as the history update: with
// count_input the one thread that owns element next_token[b] (the token
// the previous sampler launch committed) bumps its count before using it
// — no atomics, no ordering between blocks, the sampler kernels untouched.
// Groups of G elements (16 B of logits per lane) whose stat words are all
// zero and that carry no bias never load their logits; touched elements
// are stored one by one, so untouched neighbours keep their bits.
template <bool BF>
DEVINL void logit_adjust_body(void* logits, int V, int* stat,
                              const float* proc, const float* bias,
                              const int* next_token, int count_input) {
  constexpr int G = BF ? 8 : 4;
  const int b = blockIdx.y;
  const float r = proc[b * 4 + 0];
  const float f = proc[b * 4 + 1];
  const float p = proc[b * 4 + 2];
  const bool bias_on = proc[b * 4 + 3] != 0.0f;
  if (r == 1.0f && f == 0.0f && p == 0.0f && !bias_on) return;  // identity
  const int tok = count_input ? next_token[b] : -1;
  const size_t row0 = (size_t)b * V;
  int* srow = stat + row0;
  const float* brow = bias + row0;
  void* lrow = BF ? (void*)((u16*)logits + row0)
                  : (void*)((float*)logits + row0);
  const int tid = blockIdx.x * 256 + threadIdx.x;
  const int nthr = gridDim.x * 256;
  // element h is the first whose logits AND stat / bias words sit on a
  // 16 B boundary (bf16 rows with odd V start 2-byte aligned); unaligned
  // base pointers take the scalar path for the whole row
  const bool aligned = (((uintptr_t)logits | (uintptr_t)stat |
                         (uintptr_t)bias) & 15) == 0;
  int h = aligned ? (int)((G - row0 % G) % G) : V;
  if (h > V) h = V;
  const int ngroups = (V - h) / G;
  const int t0 = h + ngroups * G;
  for (int i = tid; i < h; i += nthr)
    logit_adjust_elem<BF>(lrow, srow, brow, i, tok, r, f, p, bias_on);
  for (int i = t0 + tid; i < V; i += nthr)
    logit_adjust_elem<BF>(lrow, srow, brow, i, tok, r, f, p, bias_on);
  for (int g = tid; g < ngroups; g += nthr) {
    const int i0 = h + g * G;
    int s[G];
    float bv[G];
#pragma unroll
    for (int q = 0; q < G / 4; q++) {
      const int4 sv = *(const int4*)(srow + i0 + 4 * q);
      s[4 * q + 0] = sv.x; s[4 * q + 1] = sv.y;
      s[4 * q + 2] = sv.z; s[4 * q + 3] = sv.w;
    }
    if (tok >= i0 && tok < i0 + G) {
#pragma unroll
      for (int j = 0; j < G; j++)
        if (i0 + j == tok) { s[j] += 1; srow[tok] = s[j]; }
    }
    if (bias_on) {
#pragma unroll
      for (int q = 0; q < G / 4; q++) {
        const float4 b4 = *(const float4*)(brow + i0 + 4 * q);
        bv[4 * q + 0] = b4.x; bv[4 * q + 1] = b4.y;
        bv[4 * q + 2] = b4.z; bv[4 * q + 3] = b4.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < G; j++) bv[j] = 0.0f;
    }
    bool any = false;
#pragma unroll
    for (int j = 0; j < G; j++) any |= (s[j] != 0) | (bv[j] != 0.0f);
    if (!any) continue;
    if (BF) {
      u16* lh = (u16*)lrow + i0;
      const uint4 lv = *(const uint4*)lh;
      const uint32_t w[4] = {lv.x, lv.y, lv.z, lv.w};
#pragma unroll
      for (int j = 0; j < G; j++) {
        if (s[j] == 0 && bv[j] == 0.0f) continue;
        const u16 hv = (u16)(w[j >> 1] >> ((j & 1) * 16));
        lh[j] = f2b(logit_adjust_val(b2f(hv), s[j], r, f, p, bv[j]));
      }
    } else {
      float* lf = (float*)lrow + i0;
      const float4 lv = *(const float4*)lf;
      const float l[4] = {lv.x, lv.y, lv.z, lv.w};
#pragma unroll
      for (int j = 0; j < G; j++) {
        if (s[j] == 0 && bv[j] == 0.0f) continue;
        lf[j] = logit_adjust_val(l[j], s[j], r, f, p, bv[j]);
      }
    }
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_logit_adjust(void* logits, int V, int lbf16, int* stat,
               const float* __restrict__ proc,
               const float* __restrict__ bias,
               const int* __restrict__ next_token, int count_input) {
  if (lbf16)
    logit_adjust_body<true>(logits, V, stat, proc, bias, next_token,
                            count_input);
  else
    logit_adjust_body<false>(logits, V, stat, proc, bias, next_token,
                             count_input);
}

extern "C" hipError_t launch_tokstat_mark(void* stat_row, const void* ids,
                                          int n, int V, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  int blocks = (n + 255) / 256;
  if (blocks > 64) blocks = 64;
  hipLaunchKernelGGL(k_tokstat_mark, dim3(blocks), dim3(256), 0, stream,
                     (int*)stat_row, (const int*)ids, n, V);
  return hipGetLastError();
}

// grid: one thread per 16 B group of a row (4 fp32 / 8 bf16 elements),
// capped at 512 blocks; the loops are grid-stride, so the scalar
// fallback of a misaligned row is covered by the same grid
extern "C" hipError_t launch_logit_adjust(void* logits, int V, int lbf16,
                                          int batch, void* stat,
                                          const void* proc, const void* bias,
                                          const void* next_token,
                                          int count_input,
                                          hipStream_t stream) {
  const int groups = V / (lbf16 ? 8 : 4) + 1;
  int blocks = (groups + 255) / 256;
  if (blocks > 512) blocks = 512;
  hipLaunchKernelGGL(k_logit_adjust, dim3(blocks, batch), dim3(256), 0,
                     stream, logits, V, lbf16, (int*)stat,
                     (const float*)proc, (const float*)bias,
                     (const int*)next_token, count_input);
  return hipGetLastError();
}

// ====================================================================
// Logprobs: log-softmax of the RAW logits row (after the lm_head, before
// k_logit_adjust) reduced to {chosen logprob, top-N ids + logprobs} per
// token, inside the decode step.  Per-row device data, so rows with
// different N (and rows without logprobs) share one graph:
//   lp_cfg [rows]        i32  -1 = row off (nothing of it is touched),
//                             0..LOGPROBS_MAX_TOP = the row's top-N
//   part   [rows, stride] u64 scan scratch: [0] ticket, [1, 1+nblk) one
//                             (m, s) pair per block, then nblk x 20 packed
//                             (fkey, id) words; all zero between launches
//   stage  [rows, 48]    f32  [0] M = row max, [1..20] top logits,
//                             [21] log S (S = sum exp(l - M)), [24..43] top
//                             ids; lse = M + log S is never formed: the
//                             logprob is (l - M) - log S, so a uniformly
//                             shifted row loses nothing to the size of M
//   raw    [rows, V]     f32  optional copy of the row (steps that adjust
//                             the logits in place before sampling)
//   lp_val [rows, LP_RING, 21] f32  {chosen, top_0 .. top_19} logprobs
//   lp_idx [rows, LP_RING, 20] i32  top ids
// k_logprob_scan: block x owns logits [x*2048, x*2048+2048), 8 per thread,
// kept in registers: local max m, s = sum exp(l - m), and its top-N as
// packed (fkey(l), id) words (ties -> smaller id).  Packed words are
// unique, so "not yet taken" is "below the previous winner": N rounds of a
// wave arg-max per wave, then wave 0 merges the 4 wave lists.  The
// last-arriving block (ticket) merges the partials in a fixed order over
// the BLOCK INDEX — never the arrival order — so two launches on the same
// row give the same bits: M = max_b m_b, S = sum_b s_b * exp(m_b - M).
// k_logprob_commit (after the sampler): record (nout-1) mod LP_RING gets
// (l - M) - log S for the sampled token and the row's top-N.
// ====================================================================
#define LOGPROBS_MAX_TOP 20
#define LP_RING 256
#define LP_SLICE 2048       // logits per scan block
#define LP_EPT 8            // = LP_SLICE / 256
#define LP_MERGE_EPT 16     // merge candidates per thread of the last block
#define LP_MAX_BLOCKS 204   // 204 * 20 <= 256 * LP_MERGE_EPT
#define LP_STAGE_WORDS 48
#define LP_STAGE_LOGS 21
#define LP_STAGE_IDS 24

// lane r (r < N) returns the r-th largest of the wave's packed words
// (K per lane, 0 = empty slot; 0 is below every real word); 0 when the
// wave holds fewer than r+1
template <int K>
DEVINL uint64_t lp_wave_topn(const uint64_t (&k)[K], int N) {
  const int lane = threadIdx.x & 63;
  uint64_t prev = ~0ull, mine = 0ull;
  for (int r = 0; r < N; r++) {
    uint64_t best = 0ull;
#pragma unroll
    for (int j = 0; j < K; j++)
      if (k[j] < prev && k[j] > best) best = k[j];
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) {
      uint64_t o = __shfl_xor((unsigned long long)best, w);
      if (o > best) best = o;
    }
    if (lane == r) mine = best;
    prev = best;
  }
  return mine;
}

DEVINL float lp_wave_max(float v) {
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) v = fmaxf(v, __shfl_xor(v, w));
  return v;
}

// 4 wave lists (N words each, in wl) -> wave 0's lanes r < N hold the
// block's r-th largest word
DEVINL uint64_t lp_merge_waves(const unsigned long long* wl, int N) {
  const int lane = threadIdx.x & 63;
  uint64_t c[2];
  c[0] = lane < 4 * N ? wl[lane] : 0ull;
  c[1] = lane + 64 < 4 * N ? wl[lane + 64] : 0ull;
  return lp_wave_topn<2>(c, N);
}

template <bool BF>
DEVINL void logprob_scan_body(const void* logits, int V, const int* lp_cfg,
                              unsigned long long* part, long part_stride,
                              float* stage, float* raw) {
  const int b = blockIdx.y;
  int N = lp_cfg[b];
  if (N < 0) return;  // row off
  if (N > LOGPROBS_MAX_TOP) N = LOGPROBS_MAX_TOP;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int nblk = gridDim.x;
  const size_t row0 = (size_t)b * V;
  part += (size_t)b * part_stride;
  unsigned long long* pms = part + 1;
  unsigned long long* ptop = part + 1 + nblk;
  stage += (size_t)b * LP_STAGE_WORDS;
  __shared__ float wm[4], wsum[4];
  __shared__ unsigned long long wl[4 * LOGPROBS_MAX_TOP];
  __shared__ int lastflag;

  // scalar loads: bf16 rows with odd V start 2-byte aligned
  float v[LP_EPT];
  uint64_t k[LP_EPT];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < LP_EPT; j++) {
    const int i = blockIdx.x * LP_SLICE + j * 256 + t;
    v[j] = -INFINITY;
    k[j] = 0ull;
    if (i < V) {
      const float x = BF ? b2f(((const u16*)logits)[row0 + i])
                         : ((const float*)logits)[row0 + i];
      v[j] = x;
      k[j] = pack_ki(fkey(x), i);
      m = fmaxf(m, x);
      if (raw) raw[row0 + i] = x;
    }
  }
  m = lp_wave_max(m);
  if (lane == 0) wm[wv] = m;
  __syncthreads();
  m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
  float s = 0.0f;
  if (m > -INFINITY) {
#pragma unroll
    for (int j = 0; j < LP_EPT; j++) s += expf(v[j] - m);
  }
  s = wave_reduce_sum(s);
  if (lane == 0) wsum[wv] = s;
  const uint64_t mine = lp_wave_topn<LP_EPT>(k, N);
  if (lane < N) wl[wv * N + lane] = mine;
  __syncthreads();
  // wave 0 writes the whole partial, so ONE wave's release fence orders
  // it ahead of the ticket (as in k_sample_select)
  if (wv == 0) {
    const uint64_t top = lp_merge_waves(wl, N);
    if (lane < N) ptop[blockIdx.x * LOGPROBS_MAX_TOP + lane] = top;
    if (lane == 0) {
      const float bs = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
      pms[blockIdx.x] = ((unsigned long long)__float_as_uint(bs) << 32) |
                        __float_as_uint(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (lane == 0) {
      unsigned long long tk = __hip_atomic_fetch_add(
          &part[0], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      lastflag = (tk == (unsigned long long)nblk - 1);
    }
  }
  __syncthreads();
  if (!lastflag) return;
  // last arriver: every block's partial is in; merge by block index,
  // re-arm ticket and scratch
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (wv == 0) {
    float M = -INFINITY;
    for (int i = lane; i < nblk; i += 64) {
      const unsigned long long u = __hip_atomic_load(
          &pms[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      M = fmaxf(M, __uint_as_float((uint32_t)u));
    }
    M = lp_wave_max(M);
    float S = 0.0f;
    for (int i = lane; i < nblk; i += 64) {
      const unsigned long long u = __hip_atomic_load(
          &pms[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const float mi = __uint_as_float((uint32_t)u);
      const float si = __uint_as_float((uint32_t)(u >> 32));
      if (mi > -INFINITY) S += si * expf(mi - M);
      pms[i] = 0ull;
    }
    S = wave_reduce_sum(S);
    if (lane == 0) {
      stage[0] = M;
      stage[LP_STAGE_LOGS] = M > -INFINITY ? logf(S) : 0.0f;
      part[0] = 0ull;
    }
  }
  if (N == 0) return;
  const int total = nblk * N;
  uint64_t c[LP_MERGE_EPT];
#pragma unroll
  for (int j = 0; j < LP_MERGE_EPT; j++) {
    const int ci = j * 256 + t;
    c[j] = 0ull;
    if (ci < total) {
      const int blk = ci / N;
      unsigned long long* p = ptop + blk * LOGPROBS_MAX_TOP + (ci - blk * N);
      c[j] = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *p = 0ull;
    }
  }
  const uint64_t mine2 = lp_wave_topn<LP_MERGE_EPT>(c, N);
  if (lane < N) wl[wv * N + lane] = mine2;
  __syncthreads();
  if (wv == 0) {
    const uint64_t top = lp_merge_waves(wl, N);
    if (lane < N) {
      // fewer than N logits in the row: id -1, logit -inf
      stage[1 + lane] =
          top ? fkey_inv((uint32_t)(top >> 32)) : -INFINITY;
      ((int*)stage)[LP_STAGE_IDS + lane] = top ? unpack_idx(top) : -1;
    }
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_logprob_scan(const void* __restrict__ logits, int V, int lbf16,
               const int* __restrict__ lp_cfg, unsigned long long* part,
               long part_stride, float* __restrict__ stage,
               float* __restrict__ raw) {
  if (lbf16)
    logprob_scan_body<true>(logits, V, lp_cfg, part, part_stride, stage, raw);
  else
    logprob_scan_body<false>(logits, V, lp_cfg, part, part_stride, stage,
                             raw);
}

DEVINL float lp_sub(float l, float M, float logS) {
  return l == -INFINITY ? -INFINITY : (l - M) - logS;
}

// one wave per row, after the sampler committed next_token / nout
extern "C" __global__ void __launch_bounds__(64)
k_logprob_commit(const void* __restrict__ logits, int V, int lbf16,
                 const int* __restrict__ lp_cfg,
                 const float* __restrict__ stage,
                 const float* __restrict__ raw,
                 const int* __restrict__ next_token,
                 const int* __restrict__ nout, float* __restrict__ lp_val,
                 int* __restrict__ lp_idx) {
  const int b = blockIdx.y;
  int N = lp_cfg[b];
  if (N < 0) return;
  if (N > LOGPROBS_MAX_TOP) N = LOGPROBS_MAX_TOP;
  const int t = threadIdx.x;
  stage += (size_t)b * LP_STAGE_WORDS;
  const int slot = (nout[b] - 1) & (LP_RING - 1);
  const size_t rec = (size_t)b * LP_RING + slot;
  float* val = lp_val + rec * (1 + LOGPROBS_MAX_TOP);
  int* idx = lp_idx + rec * LOGPROBS_MAX_TOP;
  const float M = stage[0], logS = stage[LP_STAGE_LOGS];
  if (t == 0) {
    int tok = next_token[b];
    if (tok < 0 || tok >= V) tok = 0;
    const size_t at = (size_t)b * V + tok;
    const float l = raw ? raw[at]
                        : lbf16 ? b2f(((const u16*)logits)[at])
                                : ((const float*)logits)[at];
    val[0] = lp_sub(l, M, logS);
  }
  if (t < N) {
    val[1 + t] = lp_sub(stage[1 + t], M, logS);
    idx[t] = ((const int*)stage)[LP_STAGE_IDS + t];
  }
}

// part_stride: u64 words per scratch row, >= 1 + 21 * ceil(V / 2048)
extern "C" hipError_t launch_logprob_scan(const void* logits, int V,
                                          int lbf16, int batch,
                                          const void* lp_cfg, void* part,
                                          long part_stride, void* stage,
                                          void* raw, hipStream_t stream) {
  const int nblk = (V + LP_SLICE - 1) / LP_SLICE;
  if (V <= 0 || nblk > LP_MAX_BLOCKS ||
      part_stride < 1 + (long)nblk * (1 + LOGPROBS_MAX_TOP))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_logprob_scan, dim3(nblk, batch), dim3(256), 0, stream,
                     logits, V, lbf16, (const int*)lp_cfg,
                     (unsigned long long*)part, part_stride, (float*)stage,
                     (float*)raw);
  return hipGetLastError();
}

extern "C" hipError_t launch_logprob_commit(const void* logits, int V,
                                            int lbf16, int batch,
                                            const void* lp_cfg,
                                            const void* stage,
                                            const void* raw,
                                            const void* next_token,
                                            const void* nout, void* lp_val,
                                            void* lp_idx,
                                            hipStream_t stream) {
  hipLaunchKernelGGL(k_logprob_commit, dim3(1, batch), dim3(64), 0, stream,
                     logits, V, lbf16, (const int*)lp_cfg,
                     (const float*)stage, (const float*)raw,
                     (const int*)next_token, (const int*)nout,
                     (float*)lp_val, (int*)lp_idx);
  return hipGetLastError();
}

// ====================================================================
// Prompt logprobs: k_logprob_rows scores M teacher-forced rows at once —
// the opposite shape of the decode stage above (hundreds to thousands of
// rows, one number each and optionally a top-N, no ring, no sampler).
// One 256-thread block per row, grid = M: no global atomics, no ticket,
// no fences, no scratch to re-arm.
//   logits  [M, V]  bf16 / fp32, contiguous rows
//   targets [M]     i32   token whose logprob goes to val[r, 0]; < 0 = none
//                         (0.0f is written; the host never reports it)
//   val [M, 21] f32, idx [M, 20] i32: the ring's record layout; slots past
//                         N are not touched
// Element -> thread mapping is fixed by the element index alone: thread t
// owns the 8 logits [s*2048 + 8t, +8) of every 2048-slice s.  A 16-byte
// aligned row loads them as one 16 B vector (two for fp32), any other row
// (bf16 with odd V: every second row) with scalar loads INTO THE SAME
// SLOTS, so the arithmetic — and with it the output bits — depends on the
// row's contents, V, the dtype and N only, never on the row's address.
// Per thread an online (m, s): s = sum exp(l - m), rescaled when m grows;
// at most ceil(V / 2048) groups of 8 pairwise-summed terms in sequence.
// Block: M = max m_t, S = sum_t s_t * exp(m_t - M) through the fixed
// wave-xor tree and ((w0 + w1) + w2) + w3.  exp is v_exp_f32 (__expf):
// terms that matter have arguments near 0, where x * log2(e) rounds to
// ~1e-7; log S is one accurate logf.
// N = 0 is that single streaming pass and nothing else (no LDS list, no
// barrier in the loop).  N > 0 keeps the row's best words in LDS behind a
// running N-th-largest threshold tau: a slice appends only words > tau to
// a 4096-word candidate list (tau = 0 before the first merge, so slice 0
// appends everything); when fewer than 2048 free slots remain the list is
// reduced to its top N (lp_wave_topn over 16 words per thread, then
// lp_merge_waves) and tau becomes the N-th.  On unsorted data that is two
// reductions per row — after slice 0 and at the end — instead of one per
// slice; an ascending row degrades to one per slice and stays correct.
// Appends land in arrival order, but packed words are unique, so the top
// N of the list does not depend on that order.
// ====================================================================
#define LPR_CAP 4096        // candidate words in LDS (N > 0)
#define LPR_EPT 16          // = LPR_CAP / 256

template <bool BF>
DEVINL void lpr_load8(const void* row, int i0, int V, bool al,
                      float (&x)[8]) {
  if (al && i0 + 8 <= V) {
    if (BF) {
      const u4v_ q = *(const u4v_*)((const u16*)row + i0);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        x[2 * j] = __uint_as_float(q[j] << 16);
        x[2 * j + 1] = __uint_as_float(q[j] & 0xffff0000u);
      }
    } else {
      const f4v a = *(const f4v*)((const float*)row + i0);
      const f4v b = *(const f4v*)((const float*)row + i0 + 4);
#pragma unroll
      for (int j = 0; j < 4; j++) { x[j] = a[j]; x[4 + j] = b[j]; }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int i = i0 + j;
      x[j] = i < V ? (BF ? b2f(((const u16*)row)[i])
                         : ((const float*)row)[i])
                   : -INFINITY;
    }
  }
}

DEVINL void lpr_accum(const float (&x)[8], float& m, float& s) {
  const float g = fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])),
                        fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
  if (g > m) { s *= __expf(m - g); m = g; }
  if (m > -INFINITY)
    s += ((__expf(x[0] - m) + __expf(x[1] - m)) +
          (__expf(x[2] - m) + __expf(x[3] - m))) +
         ((__expf(x[4] - m) + __expf(x[5] - m)) +
          (__expf(x[6] - m) + __expf(x[7] - m)));
}

// candidate list -> its top N in cand[0, N) (0 = empty slot), *cnt = N;
// returns the N-th (0 while the list is shorter).  Every thread calls it,
// after a barrier that follows the last append.
DEVINL uint64_t lpr_merge(unsigned long long* cand, unsigned long long* wl,
                          int* cnt, int N) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int n = *cnt;
  uint64_t c[LPR_EPT];
#pragma unroll
  for (int j = 0; j < LPR_EPT; j++) {
    const int ci = j * 256 + t;
    c[j] = ci < n ? cand[ci] : 0ull;
  }
  const uint64_t mine = lp_wave_topn<LPR_EPT>(c, N);
  if (lane < N) wl[wv * N + lane] = mine;
  __syncthreads();
  if (wv == 0) {
    const uint64_t top = lp_merge_waves(wl, N);
    if (lane < N) cand[lane] = top;
    if (lane == 0) *cnt = N;
  }
  __syncthreads();
  return cand[N - 1];
}

template <bool BF, bool TOP>
DEVINL void logprob_rows_body(const void* logits, int V,
                              const int* targets, int N, float* val,
                              int* idx) {
  extern __shared__ unsigned long long lpr_cand[];  // LPR_CAP words if TOP
  __shared__ float wm[4], wsum[4];
  __shared__ unsigned long long wl[4 * LOGPROBS_MAX_TOP];
  __shared__ int cnt;
  const int r = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const char* row = (const char*)logits + (size_t)r * V * (BF ? 2 : 4);
  const bool al = ((uintptr_t)row & 15) == 0;
  val += (size_t)r * (1 + LOGPROBS_MAX_TOP);
  idx += (size_t)r * LOGPROBS_MAX_TOP;
  float m = -INFINITY, s = 0.0f;
  float x[8];

  if (!TOP) {
    // two slices per trip, both loads in flight before the arithmetic
    int base = 0;
    for (; base + LP_SLICE < V; base += 2 * LP_SLICE) {
      float y[8];
      lpr_load8<BF>(row, base + t * 8, V, al, x);
      lpr_load8<BF>(row, base + LP_SLICE + t * 8, V, al, y);
      lpr_accum(x, m, s);
      lpr_accum(y, m, s);
    }
    if (base < V) {
      lpr_load8<BF>(row, base + t * 8, V, al, x);
      lpr_accum(x, m, s);
    }
  } else {
    uint64_t tau = 0ull;
    if (t == 0) cnt = 0;
    __syncthreads();
    for (int base = 0; base < V; base += LP_SLICE) {
      // cnt only grows between merges and the thread that appended last
      // reads it after its own append, so the OR sees the full count; the
      // barrier also orders the appends ahead of the merge's reads
      if (__syncthreads_or(cnt > LPR_CAP - LP_SLICE))
        tau = lpr_merge(lpr_cand, wl, &cnt, N);
      const int i0 = base + t * 8;
      lpr_load8<BF>(row, i0, V, al, x);
      lpr_accum(x, m, s);
      uint64_t w[8];
      int np = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        w[j] = i0 + j < V ? pack_ki(fkey(x[j]), i0 + j) : 0ull;
        np += w[j] > tau;
      }
      if (np) {
        int pos = atomicAdd(&cnt, np);
#pragma unroll
        for (int j = 0; j < 8; j++)
          if (w[j] > tau) lpr_cand[pos++] = w[j];
      }
    }
    __syncthreads();
    lpr_merge(lpr_cand, wl, &cnt, N);
  }

  const float wmax = lp_wave_max(m);
  if (lane == 0) wm[wv] = wmax;
  __syncthreads();
  const float M = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
  s = m > -INFINITY ? s * __expf(m - M) : 0.0f;
  s = wave_reduce_sum(s);
  if (lane == 0) wsum[wv] = s;
  __syncthreads();
  const float S = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  const float logS = M > -INFINITY ? logf(S) : 0.0f;
  if (t == 0) {
    const int tok = targets[r];
    float lp = 0.0f;
    if (tok >= 0 && tok < V) {
      const float l = BF ? b2f(((const u16*)row)[tok])
                         : ((const float*)row)[tok];
      lp = lp_sub(l, M, logS);
    }
    val[0] = lp;
  }
  if (TOP && t < N) {
    // fewer than N logits in the row: id -1, logprob -inf
    const uint64_t top = lpr_cand[t];
    val[1 + t] = top ? lp_sub(fkey_inv((uint32_t)(top >> 32)), M, logS)
                     : -INFINITY;
    idx[t] = top ? unpack_idx(top) : -1;
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_logprob_rows(const void* __restrict__ logits, int V, int lbf16,
               const int* __restrict__ targets, int N,
               float* __restrict__ val, int* __restrict__ idx) {
  if (N > 0) {
    if (lbf16) logprob_rows_body<true, true>(logits, V, targets, N, val, idx);
    else logprob_rows_body<false, true>(logits, V, targets, N, val, idx);
  } else {
    if (lbf16) logprob_rows_body<true, false>(logits, V, targets, 0, val, idx);
    else logprob_rows_body<false, false>(logits, V, targets, 0, val, idx);
  }
}

// rows: M >= 1 contiguous rows of V logits; top_n in 0..LOGPROBS_MAX_TOP
extern "C" hipError_t launch_logprob_rows(const void* logits, int V,
                                          int lbf16, int rows,
                                          const void* targets, int top_n,
                                          void* val, void* idx,
                                          hipStream_t stream) {
  if (V <= 0 || V > (1 << 30) || rows <= 0 || top_n < 0 ||
      top_n > LOGPROBS_MAX_TOP)
    return hipErrorInvalidValue;
  const size_t lds = top_n > 0 ? LPR_CAP * sizeof(unsigned long long) : 0;
  hipLaunchKernelGGL(k_logprob_rows, dim3(rows), dim3(256), lds, stream,
                     logits, V, lbf16, (const int*)targets, top_n,
                     (float*)val, (int*)idx);
  return hipGetLastError();
}

// ====================================================================
// Greedy speculative decoding, verify + commit: k_spec_verify reduces the
// k+1 logits rows of a target verify pass to their argmax, finds the
// accepted prefix of the k draft tokens and commits the outcome into the
// device state of BOTH engines — the host sees no logit.
//   logits  [k+1, V]  bf16 / fp32, contiguous rows; row i scores draft i,
//                     row k is the bonus position
//   drafts  [k]       i32 proposals (the target's ids_buf[1..k])
//   scratch [SPEC_SCRATCH_WORDS] u64: [0..SPEC_MAX_K] packed (fkey, id) row
//                     maxima, [SPEC_MAX_K + 1] the launch-wide ticket; all
//                     zero between launches (zeroed once by the host, every
//                     word a launch touched is re-armed by its commit)
// Grid (blocks, k+1): the blocks of a row split it in LP_SLICE-wide slices
// (thread t owns the 8 logits [s*2048 + 8t, +8) of a slice, loaded as in
// k_logprob_rows), reduce to one packed word and atomicMax it into the
// row's scratch word — ties go to the SMALLEST id, as k_logit_max and
// np.argmax.  ONE ticket over the whole launch (release fence before the
// add, acquire fence in the last arriver, as sample_pick_commit); thread 0
// of the last-arriving block then commits:
//   a_i = argmax of row i (outside [0, V): 0, the NaN-logit insurance)
//   m   = the largest j <= k with drafts[i] == a_i for all i < j
//   n   = *t_len — the verify pass leaves the target's length at the
//         position it started from (_layers_forward reads it, nobody
//         advances it), so the kernel reads n there and takes no argument
//   target: out_ring[nout .. nout+m] = drafts[0..m-1], a_m; nout += m + 1;
//           next_token = a_m; len = n + m + 1
//   draft:  len = n + m + 1; next_token = a_m; nout = 0 (the next cycle's
//           proposals land in its out_ring[0..k] again)
//   rec[*nrec % rec_cap] = {m, drafts[0..k-1], -1 ...}; *nrec += 1
// m <= k by construction, so no length above n + k + 1 is ever written;
// ring writes past ring_cap are dropped.  Plain stores only.
// ====================================================================
#define SPEC_MAX_K 16
#define SPEC_SCRATCH_WORDS (SPEC_MAX_K + 2)
#define SPEC_REC_WORDS (SPEC_MAX_K + 1)
#define SPEC_AUTO_BLOCKS 8

template <bool BF>
DEVINL uint64_t spec_slice_max(const void* logits, int V) {
  const char* row =
      (const char*)logits + (size_t)blockIdx.y * V * (BF ? 2 : 4);
  const bool al = ((uintptr_t)row & 15) == 0;
  float mv = -INFINITY;
  int mi = 0x7fffffff;  // nothing seen: loses every tie, clamped if it wins
  const long step = (long)gridDim.x * LP_SLICE;
  for (long base = (long)blockIdx.x * LP_SLICE; base < V; base += step) {
    const int i0 = (int)base + threadIdx.x * 8;
    if (i0 >= V) continue;
    float x[8];
    lpr_load8<BF>(row, i0, V, al, x);
    // ascending ids: a strict > keeps the smallest id of equal values
#pragma unroll
    for (int j = 0; j < 8; j++)
      if (i0 + j < V && x[j] > mv) { mv = x[j]; mi = i0 + j; }
  }
  return pack_ki(fkey(mv), mi);
}

extern "C" __global__ void __launch_bounds__(256)
k_spec_verify(const void* __restrict__ logits, int V, int lbf16, int k,
              const int* drafts, unsigned long long* scratch,
              int* t_len, int* t_next, int* t_ring, int* t_nout, int ring_cap,
              int* d_len, int* d_next, int* d_nout,
              int* rec, int* nrec, int rec_cap) {
  uint64_t pk = lbf16 ? spec_slice_max<true>(logits, V)
                      : spec_slice_max<false>(logits, V);
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) {
    uint64_t o = __shfl_xor((unsigned long long)pk, w);
    if (o > pk) pk = o;
  }
  __shared__ unsigned long long ws[4];
  __shared__ int lastflag;
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = pk;
  __syncthreads();
  int* ticket = (int*)(scratch + SPEC_MAX_K + 1);
  if (threadIdx.x == 0) {
    uint64_t b = ws[0];
    for (int w = 1; w < 4; w++) if (ws[w] > b) b = ws[w];
    atomicMax(scratch + blockIdx.y, (unsigned long long)b);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL,
                                   __HIP_MEMORY_SCOPE_AGENT);
    lastflag = (t == (int)(gridDim.x * gridDim.y) - 1);
  }
  __syncthreads();
  if (!lastflag || threadIdx.x != 0) return;
  // last arriver: every row's maximum is in; commit and re-arm
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  *ticket = 0;
  if (k < 1) k = 1;
  if (k > SPEC_MAX_K) k = SPEC_MAX_K;
  int m = -1, am = 0;
  for (int i = 0; i <= k; i++) {
    int a = unpack_idx(__hip_atomic_load(scratch + i, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT));
    scratch[i] = 0ull;
    if (a < 0 || a >= V) a = 0;
    if (m < 0 && (i == k || drafts[i] != a)) { m = i; am = a; }
  }
  const int n = *t_len;
  const int no = *t_nout;
  for (int j = 0; j <= m; j++) {
    // accepted drafts equal an in-range argmax, so they are in [0, V)
    const int tok = j < m ? drafts[j] : am;
    if (no + j >= 0 && no + j < ring_cap) t_ring[no + j] = tok;
  }
  *t_nout = no + m + 1;
  *t_next = am;
  *t_len = n + m + 1;
  *d_len = n + m + 1;
  *d_next = am;
  *d_nout = 0;
  const int nr = *nrec;
  int* r = rec + (size_t)((nr < 0 ? 0 : nr) % rec_cap) * SPEC_REC_WORDS;
  r[0] = m;
  for (int i = 0; i < SPEC_MAX_K; i++) r[1 + i] = i < k ? drafts[i] : -1;
  *nrec = nr + 1;
}

// blocks <= 0: SPEC_AUTO_BLOCKS per row; never more than the row has slices
extern "C" hipError_t launch_spec_verify(
    const void* logits, int V, int lbf16, int rows, int k, int blocks,
    const void* drafts, void* scratch, void* t_len, void* t_next,
    void* t_ring, void* t_nout, int ring_cap, void* d_len, void* d_next,
    void* d_nout, void* rec, void* nrec, int rec_cap, hipStream_t stream) {
  if (k < 1 || k > SPEC_MAX_K || V <= 0 || V > (1 << 30) || rows != k + 1 ||
      ring_cap <= 0 || rec_cap <= 0)
    return hipErrorInvalidValue;
  const int slices = (V + LP_SLICE - 1) / LP_SLICE;
  if (blocks <= 0) blocks = SPEC_AUTO_BLOCKS;
  if (blocks > slices) blocks = slices;
  hipLaunchKernelGGL(k_spec_verify, dim3(blocks, rows), dim3(256), 0, stream,
                     logits, V, lbf16, k, (const int*)drafts,
                     (unsigned long long*)scratch, (int*)t_len, (int*)t_next,
                     (int*)t_ring, (int*)t_nout, ring_cap, (int*)d_len,
                     (int*)d_next, (int*)d_nout, (int*)rec, (int*)nrec,
                     rec_cap);
  return hipGetLastError();
}

// ids of a verify pass, on the stream: ids[0] = the target's pending token,
// ids[1..k] = the draft's proposals (its out_ring[0..k-1]).  k = 0 stages
// the pending token alone (a plain step through the verify pass).
extern "C" __global__ void __launch_bounds__(64)
k_spec_stage(int* ids, const int* t_next, const int* d_ring, int k) {
  const int t = threadIdx.x;
  if (t == 0) ids[0] = t_next[0];
  else if (t <= k) ids[t] = d_ring[t - 1];
}

extern "C" hipError_t launch_spec_stage(void* ids, const void* t_next,
                                        const void* d_ring, int k,
                                        hipStream_t stream) {
  if (k < 0 || k > SPEC_MAX_K) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_spec_stage, dim3(1), dim3(64), 0, stream, (int*)ids,
                     (const int*)t_next, (const int*)d_ring, k);
  return hipGetLastError();
}

// ====================================================================
// Prefill GEMM: Y[M,N] = X[M,K] @ W[N,K]^T (+res), bf16 in/out, fp32 acc.
// MFMA v_mfma_f32_16x16x32_bf16; 128x128 tile, BK=32, 4 waves (2x2),
// each wave a 64x64 sub-tile (4x4 fragments).  LDS staged, padded rows.
// Correctness-first structure (guide §5 ladder step ~0-2); prefill only —
// decode uses k_gemv_bf16.
// ====================================================================

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define BM 128
#define BN 128
#define BK 64

// TS=BM=BN tile template (128 or 64), BK=64, 4 waves (2x2), each wave
// a (TS/2)^2 sub-tile of 16x16 fragments.  Double-buffered LDS filled
// by global_load_lds (async global->LDS DMA, 16 B/lane), one barrier
// per K-tile (guide §5 "Minimum 2-phase": STAGE next ahead of
// ds_read+MFMA).  LDS rows are XOR-swizzled st_8x16 (slot ^= row&7) so
// ds_read_b128 fragment reads stay conflict-free; glds writes
// lane-linear, so the swizzle is applied to the per-lane GLOBAL source
// address (guide §5.4 rule 21) and to the read offsets — never the LDS
// dest.  The 64-tile variant exists because M=N=2048-class prefill
// GEMMs give the 128-tile only ~256 blocks = 1 block/CU — no occupancy
// to hide the DMA/barrier latency (measured 250 TF; see
// profiles/prefill_gemm_r02.md).
template <int TS>
__global__ void __launch_bounds__(256)
k_gemm_bf16_t(const u16* __restrict__ X, const u16* __restrict__ W,
              u16* __restrict__ Y, const u16* __restrict__ res,
              float* __restrict__ accbuf, int M, int N, int K) {
  constexpr int F = TS / 32;        // 16x16 frags per wave dim
  constexpr int SUB = TS / 2;       // wave sub-tile span
  __shared__ u16 As[2][TS * 64];
  __shared__ u16 Bs[2][TS * 64];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wrow = wave >> 1, wcol = wave & 1;  // 2x2 waves
  const int bm = blockIdx.x * TS, bn = blockIdx.y * TS;

  const int SK = gridDim.z;
  const int kslices = (K / BK + SK - 1) / SK;
  const int k_lo = blockIdx.z * kslices * BK;
  int k_hi = k_lo + kslices * BK;
  if (k_hi > K) k_hi = K;
  const int nt = (k_hi - k_lo) / BK;
  if (nt <= 0) return;

  f4v acc[F][F];
#pragma unroll
  for (int i = 0; i < F; i++)
#pragma unroll
    for (int j = 0; j < F; j++) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // glds staging: per call a wave fills 8 rows x 128 B (lane: row
  // lane/8, slot lane%8); source col-slot pre-swizzled by row&7.
  const int g_r = lane >> 3;             // row within the 8-row group
  const int g_s = lane & 7;              // LDS slot
  auto stage = [&](int buf, int kt) {
    const int k0 = k_lo + kt * BK;
#pragma unroll
    for (int i = 0; i < TS / 32; i++) {
      int r = wave * (TS / 4) + i * 8 + g_r;   // tile row 0..TS-1
      int cs = g_s ^ (r & 7);            // source col-slot (involution)
      int gr = bm + r;
      int grc = gr < M ? gr : (M > 0 ? M - 1 : 0);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) uint32_t*)(
              X + (size_t)grc * K + k0 + cs * 8),
          (__attribute__((address_space(3))) uint32_t*)(
              &As[buf][(wave * (TS / 4) + i * 8) * 64]),
          16, 0, 0);
      int gb = bn + r;
      int gbc = gb < N ? gb : N - 1;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) uint32_t*)(
              W + (size_t)gbc * K + k0 + cs * 8),
          (__attribute__((address_space(3))) uint32_t*)(
              &Bs[buf][(wave * (TS / 4) + i * 8) * 64]),
          16, 0, 0);
    }
  };

  stage(0, 0);
  __syncthreads();

  const int fr = lane & 15, fk = lane >> 4;  // fragment row / k-slot
  int cur = 0;
  for (int t = 0; t < nt; t++) {
    if (t + 1 < nt) stage(cur ^ 1, t + 1);   // issue next tile's DMA
#pragma unroll
    for (int sl = 0; sl < 2; sl++) {         // two 32-deep k-slices
      bf16x8 a[F], b[F];
#pragma unroll
      for (int i = 0; i < F; i++) {
        int ra = wrow * SUB + i * 16 + fr;
        int sa = (sl * 4 + fk) ^ (ra & 7);
        a[i] = *(bf16x8*)(&As[cur][ra * 64 + sa * 8]);
        int rb = wcol * SUB + i * 16 + fr;
        int sb = (sl * 4 + fk) ^ (rb & 7);
        b[i] = *(bf16x8*)(&Bs[cur][rb * 64 + sb * 8]);
      }
#pragma unroll
      for (int i = 0; i < F; i++)
#pragma unroll
        for (int j = 0; j < F; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();  // drains the in-flight DMA (vmcnt0) + read fence
    cur ^= 1;
  }

  // epilogue: C layout col = lane&15, row = (lane>>4)*4 + reg
  const int cc = lane & 15, cr = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < F; i++) {
#pragma unroll
    for (int j = 0; j < F; j++) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        int row = bm + wrow * SUB + i * 16 + cr + r;
        int col = bn + wcol * SUB + j * 16 + cc;
        if (row < M && col < N) {
          float v = acc[i][j][r];
          if (SK > 1) {
            atomicAdd(accbuf + (size_t)row * N + col, v);
          } else {
            if (res) v += b2f(res[(size_t)row * N + col]);
            Y[(size_t)row * N + col] = f2b(v);
          }
        }
      }
    }
  }
}

// convert split-K fp32 accumulator to bf16 (+res); also used to zero it
extern "C" __global__ void __launch_bounds__(256)
k_gemm_fin(const float* __restrict__ accbuf, const u16* __restrict__ res,
           u16* __restrict__ Y, long total) {
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float v = accbuf[i];
  if (res) v += b2f(res[i]);
  Y[i] = f2b(v);
}

extern "C" __global__ void __launch_bounds__(256)
k_zero_f32(float* __restrict__ p, long total) {
  long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 4 <= total) {
    *(f4v*)(p + i) = {0.f, 0.f, 0.f, 0.f};
  } else {
    for (; i < total; i++) p[i] = 0.f;  // tail: no over-write past total
  }
}

extern "C" hipError_t launch_gemm_bf16(const void* X, const void* W, void* Y,
                                       const void* res, void* accbuf, int M,
                                       int N, int K, hipStream_t stream) {
  int gm = (M + BM - 1) / BM, gn = (N + BN - 1) / BN;
  int ts = 128;
  // small grids underfill 256 CUs at 1 block/CU with the 128-tile;
  // the 64-tile doubles DMA traffic per output, so only when K is
  // shallow enough that occupancy dominates (A/B: llama-1b 2k TTFT
  // 11.8->10.4 ms; deep-K gemma shapes prefer the 128-tile)
  if (gm * gn < 300 && K <= 2048 && K % 64 == 0) {
    ts = 64;
    gm = (M + 63) / 64;
    gn = (N + 63) / 64;
  }
  int sk = 1;
  if (accbuf && gm * gn < 160) {  // split K while the grid underfills
    while (sk < 8 && gm * gn * sk * 2 <= 512 && (K / BK) % (sk * 2) == 0)
      sk *= 2;
  }
  if (sk > 1) {
    long total = (long)M * N;
    hipLaunchKernelGGL(k_zero_f32, dim3((uint32_t)((total + 1023) / 1024)),
                       dim3(256), 0, stream, (float*)accbuf, total);
  }
  dim3 grid(gm, gn, sk);
  if (ts == 64)
    hipLaunchKernelGGL((k_gemm_bf16_t<64>), grid, dim3(256), 0, stream,
                       (const u16*)X, (const u16*)W, (u16*)Y, (const u16*)res,
                       (float*)accbuf, M, N, K);
  else
    hipLaunchKernelGGL((k_gemm_bf16_t<128>), grid, dim3(256), 0, stream,
                       (const u16*)X, (const u16*)W, (u16*)Y, (const u16*)res,
                       (float*)accbuf, M, N, K);
  if (sk > 1) {
    long total = (long)M * N;
    hipLaunchKernelGGL(k_gemm_fin, dim3((uint32_t)((total + 255) / 256)),
                       dim3(256), 0, stream, (const float*)accbuf,
                       (const u16*)res, (u16*)Y, total);
  }
  return hipGetLastError();
}

// ====================================================================
// MXFP4 weight quantization: 4-bit e2m1 values packed 2/byte with one
// e8m0 (power-of-two) scale per 32-element block — the OCP MX format.
// Decode is weights-only quantization: the GEMV dequantizes via
// v_cvt_scalef32_pk_f32_fp4, which applies the block scale INSIDE the
// hardware convert (same VALU per element as the fp8 path, HALF the
// weight bytes -> ~1.5x on stream-bound shapes).
// ====================================================================

extern "C" __global__ void __launch_bounds__(256)
k_quant_fp4_rows(const u16* __restrict__ X, uint8_t* __restrict__ Q,
                 uint8_t* __restrict__ E, int K) {
  const int row = blockIdx.x;
  const u16* xr = X + (size_t)row * K;
  uint8_t* qr = Q + (size_t)row * (K / 2);
  uint8_t* er = E + (size_t)row * (K / 32);
  // each thread owns whole 32-element blocks
  for (int blk = threadIdx.x; blk < K / 32; blk += 256) {
    float v[32];
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < 32; j++) {
      v[j] = b2f(xr[blk * 32 + j]);
      am = fmaxf(am, fabsf(v[j]));
    }
    // e2m1 max magnitude = 6.0: scale = 2^e with absmax/2^e <= 6
    int e = 0;
    if (am > 0.f) {
      int ee;
      frexpf(am / 6.0f, &ee);  // am/6 = m * 2^ee, m in [0.5, 1)
      e = ee;                  // 2^ee >= am/6
      if (ldexpf(6.0f, e - 1) >= am) e -= 1;  // exact-power tightening
    }
    if (e < -126) e = -126;
    if (e > 127) e = 127;
    union { float f; uint32_t u; } sc;
    sc.u = (uint32_t)(e + 127) << 23;       // 2^e
    er[blk] = (uint8_t)(e + 127);
#pragma unroll
    for (int d = 0; d < 4; d++) {           // 4 dwords of 8 nibbles
      // HW semantics (device-verified): encode fp4 = RNE(v / scale),
      // decode = v * scale -> pass the SAME 2^e both ways; the pair
      // selector must be a literal
      uint32_t w = 0;
      w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(
          w, v[d * 8 + 0], v[d * 8 + 1], sc.f, 0);
      w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(
          w, v[d * 8 + 2], v[d * 8 + 3], sc.f, 1);
      w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(
          w, v[d * 8 + 4], v[d * 8 + 5], sc.f, 2);
      w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(
          w, v[d * 8 + 6], v[d * 8 + 7], sc.f, 3);
      *(uint32_t*)(qr + blk * 16 + d * 4) = w;
    }
  }
}

extern "C" hipError_t launch_quant_fp4(const void* X, void* Q, void* E,
                                       int M, int K, hipStream_t stream) {
  if (K % 32 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_quant_fp4_rows, dim3(M), dim3(256), 0, stream,
                     (const u16*)X, (uint8_t*)Q, (uint8_t*)E, K);
  return hipGetLastError();
}

// ====================================================================
// fp8 row quantization: Q[N,K] = e4m3(X / s_n), s_n = absmax_n / 448.
// One block per row.  Used (a) at load time to quantize weights ON
// DEVICE (drops the round-1 host-quant ~90 s for 9B and the duplicate
// bf16 copy — VERDICT r1 item 3), (b) per prefill GEMM to quantize the
// activation rows so BOTH MFMA operands are fp8.
// HW convert: v_cvt_pk_fp8_f32 (OCP e4m3fn on gfx950, saturating).
// ====================================================================

extern "C" __global__ void __launch_bounds__(256)
k_quant_fp8_rows(const u16* __restrict__ X, uint8_t* __restrict__ Q,
                 float* __restrict__ S, int K) {
  __shared__ float wmax[4];
  const int row = blockIdx.x;
  const u16* xr = X + (size_t)row * K;
  uint8_t* qr = Q + (size_t)row * K;

  float amax = 0.f;
  for (int i = threadIdx.x * 8; i < K; i += 2048) {
    s8v v = *(const s8v*)(xr + i);
#pragma unroll
    for (int j = 0; j < 8; j++) amax = fmaxf(amax, fabsf(b2f(((u16*)&v)[j])));
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  const float s = fmaxf(amax, 1e-8f) / 448.0f;
  const float rs = 1.0f / s;
  if (threadIdx.x == 0) S[row] = s;

  for (int i = threadIdx.x * 8; i < K; i += 2048) {
    s8v v = *(const s8v*)(xr + i);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; j++) f[j] = b2f(((u16*)&v)[j]) * rs;
    uint32_t lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    *(uint32_t*)(qr + i) = lo;
    *(uint32_t*)(qr + i + 4) = hi;
  }
}

extern "C" hipError_t launch_quant_fp8(const void* X, void* Q, void* S,
                                       int M, int K, hipStream_t stream) {
  if (K % 8 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_quant_fp8_rows, dim3(M), dim3(256), 0, stream,
                     (const u16*)X, (uint8_t*)Q, (float*)S, K);
  return hipGetLastError();
}

// ====================================================================
// fp8 MFMA prefill GEMM: Y[M,N] = (sx_m * sy_n) * Xq[M,K] @ Wq[N,K]^T,
// both operands OCP e4m3 with per-row scales (north star "CDNA4 fp8
// MFMA").  v_mfma_f32_16x16x32_fp8_fp8; BM=BN=128, BK=64 (two K=32
// slices), 4 waves (2x2), 64x64 per wave; LDS rows padded to 80 B so
// 16-B stores stay aligned and b64 fragment reads spread banks.
// Same split-K scheme as the bf16 GEMM (scales folded before the
// atomicAdd so k_gemm_fin stays shared).
// ====================================================================

typedef long i64frag;

extern "C" __global__ void __launch_bounds__(256)
k_gemm_fp8(const uint8_t* __restrict__ X, const float* __restrict__ sx,
           const uint8_t* __restrict__ W, const float* __restrict__ sw,
           u16* __restrict__ Y, const u16* __restrict__ res,
           float* __restrict__ accbuf, int M, int N, int K) {
  constexpr int LDR = 80;  // padded LDS row stride (bytes)
  __shared__ uint8_t As[2][128 * LDR];
  __shared__ uint8_t Bs[2][128 * LDR];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wrow = wave >> 1, wcol = wave & 1;
  const int bm = blockIdx.x * 128, bn = blockIdx.y * 128;

  const int SK = gridDim.z;
  const int kslices = (K / 64 + SK - 1) / SK;
  const int k_lo = blockIdx.z * kslices * 64;
  int k_hi = k_lo + kslices * 64;
  if (k_hi > K) k_hi = K;
  const int nt = (k_hi - k_lo) / 64;
  if (nt <= 0) return;

  f4v acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // stage: 128 rows x 64 B per operand; 256 threads x 2 iters x 16 B
  auto stage = [&](int buf, int kt) {
    const int k0 = k_lo + kt * 64;
    for (int i = tid; i < 128 * 4; i += 256) {
      int r = i >> 2, seg = i & 3;
      int gr = bm + r;
      int grc = gr < M ? gr : (M > 0 ? M - 1 : 0);
      *(u4v_*)(&As[buf][r * LDR + seg * 16]) =
          *(const u4v_*)(X + (size_t)grc * K + k0 + seg * 16);
      int gb = bn + r;
      int gbc = gb < N ? gb : N - 1;
      *(u4v_*)(&Bs[buf][r * LDR + seg * 16]) =
          *(const u4v_*)(W + (size_t)gbc * K + k0 + seg * 16);
    }
  };

  stage(0, 0);
  __syncthreads();

  const int fr = lane & 15, fk8 = (lane >> 4) * 8;  // frag row / k-offset
  int cur = 0;
  for (int t = 0; t < nt; t++) {
    if (t + 1 < nt) stage(cur ^ 1, t + 1);  // fill other buf during MFMA
#pragma unroll
    for (int sl = 0; sl < 2; sl++) {  // two K=32 slices per 64-B tile
      i64frag a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        int ra = wrow * 64 + i * 16 + fr;
        a[i] = *(const i64frag*)(&As[cur][ra * LDR + sl * 32 + fk8]);
        int rb = wcol * 64 + i * 16 + fr;
        b[i] = *(const i64frag*)(&Bs[cur][rb * LDR + sl * 32 + fk8]);
      }
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
              a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();  // next iter writes cur / reads cur^1
    cur ^= 1;
  }

  // epilogue: C col = lane&15, row = (lane>>4)*4 + reg (same map as bf16)
  const int cc = lane & 15, cr = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        int row = bm + wrow * 64 + i * 16 + cr + r;
        int col = bn + wcol * 64 + j * 16 + cc;
        if (row < M && col < N) {
          float v = acc[i][j][r] * sx[row] * sw[col];
          if (SK > 1) {
            atomicAdd(accbuf + (size_t)row * N + col, v);
          } else {
            if (res) v += b2f(res[(size_t)row * N + col]);
            Y[(size_t)row * N + col] = f2b(v);
          }
        }
      }
    }
  }
}

extern "C" hipError_t launch_gemm_fp8(const void* X, const void* sx,
                                      const void* W, const void* sw, void* Y,
                                      const void* res, void* accbuf, int M,
                                      int N, int K, hipStream_t stream) {
  if (K % 64 != 0) return hipErrorInvalidValue;
  int gm = (M + 127) / 128, gn = (N + 127) / 128;
  int sk = 1;
  if (accbuf && gm * gn < 160) {
    while (sk < 8 && gm * gn * sk * 2 <= 512 && (K / 64) % (sk * 2) == 0)
      sk *= 2;
  }
  if (sk > 1) {
    long total = (long)M * N;
    hipLaunchKernelGGL(k_zero_f32, dim3((uint32_t)((total + 1023) / 1024)),
                       dim3(256), 0, stream, (float*)accbuf, total);
  }
  dim3 grid(gm, gn, sk);
  hipLaunchKernelGGL(k_gemm_fp8, grid, dim3(256), 0, stream,
                     (const uint8_t*)X, (const float*)sx, (const uint8_t*)W,
                     (const float*)sw, (u16*)Y, (const u16*)res,
                     (float*)accbuf, M, N, K);
  if (sk > 1) {
    long total = (long)M * N;
    hipLaunchKernelGGL(k_gemm_fin, dim3((uint32_t)((total + 255) / 256)),
                       dim3(256), 0, stream, (const float*)accbuf,
                       (const u16*)res, (u16*)Y, total);
  }
  return hipGetLastError();
}

// ====================================================================
// Prefill GEMM with MXFP4 weights: Y[M,N] = X[M,K] @ dequant(W4)[N,K]^T
// (+res).  bf16 MFMA (activations stay bf16 — no activation quant, so
// this path is MORE accurate than the fp8 prefill); the B operand is
// dequantized fp4 -> bf16 in the staging pass (register loads + scaled
// hardware converts), A keeps the async glds DMA.  Completes the
// single-copy MXFP4 story for max_batch=1 engines.
// ====================================================================

extern "C" __global__ void __launch_bounds__(256)
k_gemm_fp4w(const u16* __restrict__ X, const uint8_t* __restrict__ W4,
            const uint8_t* __restrict__ WE, u16* __restrict__ Y,
            const u16* __restrict__ res, float* __restrict__ accbuf,
            int M, int N, int K) {
  __shared__ u16 As[2][128 * 64];
  __shared__ u16 Bs[2][128 * 64];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wrow = wave >> 1, wcol = wave & 1;
  const int bm = blockIdx.x * BM, bn = blockIdx.y * BN;

  const int SK = gridDim.z;
  const int kslices = (K / BK + SK - 1) / SK;
  const int k_lo = blockIdx.z * kslices * BK;
  int k_hi = k_lo + kslices * BK;
  if (k_hi > K) k_hi = K;
  const int nt = (k_hi - k_lo) / BK;
  if (nt <= 0) return;

  f4v acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int g_r = lane >> 3;
  const int g_s = lane & 7;
  // A side: async glds DMA with pre-swizzled source slots (as bf16 GEMM)
  auto stage_a = [&](int buf, int kt) {
    const int k0 = k_lo + kt * BK;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      int r = wave * 32 + i * 8 + g_r;
      int cs = g_s ^ (r & 7);
      int gr = bm + r;
      int grc = gr < M ? gr : (M > 0 ? M - 1 : 0);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) uint32_t*)(
              X + (size_t)grc * K + k0 + cs * 8),
          (__attribute__((address_space(3))) uint32_t*)(
              &As[buf][(wave * 32 + i * 8) * 64]),
          16, 0, 0);
    }
  };
  // B side: 2 threads per row (halves of BK=64), fp4 -> bf16 into the
  // swizzled LDS slots
  auto stage_b = [&](int buf, int kt) {
    const int k0 = k_lo + kt * BK;
    const int r = tid >> 1, h = tid & 1;
    int gb = bn + r;
    int gbc = gb < N ? gb : N - 1;
    const uint8_t* wp = W4 + (size_t)gbc * (K / 2) + (k0 + h * 32) / 2;
    union { float f; uint32_t u; } sc;
    sc.u = (uint32_t)WE[(size_t)gbc * (K / 32) + (k0 + h * 32) / 32] << 23;
    u4v_ pk = *(const u4v_*)wp;          // 16 bytes = 32 fp4 values
#pragma unroll
    for (int d = 0; d < 4; d++) {        // 8 values -> one 16-B slot
      f2v p[4];
      fp4x8_to_f32p(pk[d], sc.f, p);
      u16 o[8];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        o[j * 2] = f2b(p[j][0]);
        o[j * 2 + 1] = f2b(p[j][1]);
      }
      const int slot = (h * 4 + d) ^ (r & 7);
      *(s8v*)(&Bs[buf][r * 64 + slot * 8]) = *(s8v*)o;
    }
  };

  stage_a(0, 0);
  stage_b(0, 0);
  __syncthreads();

  const int fr = lane & 15, fk = lane >> 4;
  int cur = 0;
  for (int t = 0; t < nt; t++) {
    if (t + 1 < nt) {
      stage_a(cur ^ 1, t + 1);
      stage_b(cur ^ 1, t + 1);
    }
#pragma unroll
    for (int sl = 0; sl < 2; sl++) {
      bf16x8 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        int ra = wrow * 64 + i * 16 + fr;
        int sa = (sl * 4 + fk) ^ (ra & 7);
        a[i] = *(bf16x8*)(&As[cur][ra * 64 + sa * 8]);
        int rb = wcol * 64 + i * 16 + fr;
        int sb = (sl * 4 + fk) ^ (rb & 7);
        b[i] = *(bf16x8*)(&Bs[cur][rb * 64 + sb * 8]);
      }
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
    cur ^= 1;
  }

  const int cc = lane & 15, cr = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        int row = bm + wrow * 64 + i * 16 + cr + r;
        int col = bn + wcol * 64 + j * 16 + cc;
        if (row < M && col < N) {
          float v = acc[i][j][r];
          if (SK > 1) {
            atomicAdd(accbuf + (size_t)row * N + col, v);
          } else {
            if (res) v += b2f(res[(size_t)row * N + col]);
            Y[(size_t)row * N + col] = f2b(v);
          }
        }
      }
    }
  }
}

extern "C" hipError_t launch_gemm_fp4w(const void* X, const void* W4,
                                       const void* WE, void* Y,
                                       const void* res, void* accbuf, int M,
                                       int N, int K, hipStream_t stream) {
  if (K % 64 != 0) return hipErrorInvalidValue;
  int gm = (M + BM - 1) / BM, gn = (N + BN - 1) / BN;
  int sk = 1;
  if (accbuf && gm * gn < 160) {
    while (sk < 8 && gm * gn * sk * 2 <= 512 && (K / BK) % (sk * 2) == 0)
      sk *= 2;
  }
  if (sk > 1) {
    long total = (long)M * N;
    hipLaunchKernelGGL(k_zero_f32, dim3((uint32_t)((total + 1023) / 1024)),
                       dim3(256), 0, stream, (float*)accbuf, total);
  }
  dim3 grid(gm, gn, sk);
  hipLaunchKernelGGL(k_gemm_fp4w, grid, dim3(256), 0, stream, (const u16*)X,
                     (const uint8_t*)W4, (const uint8_t*)WE, (u16*)Y,
                     (const u16*)res, (float*)accbuf, M, N, K);
  if (sk > 1) {
    long total = (long)M * N;
    hipLaunchKernelGGL(k_gemm_fin, dim3((uint32_t)((total + 255) / 256)),
                       dim3(256), 0, stream, (const float*)accbuf,
                       (const u16*)res, (u16*)Y, total);
  }
  return hipGetLastError();
}

// ====================================================================
// elementwise tanh soft-cap: y = cap * tanh(x / cap)  (bf16)
// (Gemma-2 final-logit capping on the all-positions GEMM path; the
// decode GEMV fuses this into its epilogue instead)
// ====================================================================

extern "C" __global__ void __launch_bounds__(256)
k_softcap(u16* __restrict__ y, long total, float cap) {
  long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i >= total) return;
  s8v v = *(const s8v*)(y + i);
  u16 o[8];
#pragma unroll
  for (int j = 0; j < 8; j++)
    o[j] = f2b(cap * tanhf(b2f(((u16*)&v)[j]) / cap));
  *(s8v*)(y + i) = *(s8v*)o;
}

extern "C" hipError_t launch_softcap(void* y, long total, float cap,
                                     hipStream_t stream) {
  long blocks = (total / 8 + 255) / 256;
  hipLaunchKernelGGL(k_softcap, dim3((uint32_t)blocks), dim3(256), 0, stream,
                     (u16*)y, total, cap);
  return hipGetLastError();
}

// ====================================================================
// y[M,N] += bias[N] (bf16): Qwen-2 qkv-bias epilogue on the prefill /
// batched GEMM path (the decode GEMV adds bias via its `res` slot).
// ====================================================================

extern "C" __global__ void __launch_bounds__(256)
k_bias_add(u16* __restrict__ y, const u16* __restrict__ bias, long total,
           int N) {
  long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i >= total) return;
  s8v yv = *(const s8v*)(y + i);
  s8v bv = *(const s8v*)(bias + (i % N));
  u16 o[8];
#pragma unroll
  for (int j = 0; j < 8; j++)
    o[j] = f2b(b2f(((u16*)&yv)[j]) + b2f(((u16*)&bv)[j]));
  *(s8v*)(y + i) = *(s8v*)o;
}

extern "C" hipError_t launch_bias_add(void* y, const void* bias, int M,
                                      int N, hipStream_t stream) {
  if (N % 8 != 0) return hipErrorInvalidValue;
  long total = (long)M * N;
  hipLaunchKernelGGL(k_bias_add, dim3((uint32_t)((total / 8 + 255) / 256)),
                     dim3(256), 0, stream, (u16*)y, (const u16*)bias, total,
                     N);
  return hipGetLastError();
}

// ====================================================================
// y += a (bf16, fp32 math).  Used on the TP path where the RCCL
// all-reduce sits between the row-parallel GEMV and the residual add.
// ====================================================================

extern "C" __global__ void __launch_bounds__(256)
k_addinto(u16* __restrict__ y, const u16* __restrict__ a, long total) {
  long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i >= total) return;
  s8v yv = *(const s8v*)(y + i);
  s8v av = *(const s8v*)(a + i);
  u16 o[8];
#pragma unroll
  for (int j = 0; j < 8; j++)
    o[j] = f2b(b2f(((u16*)&yv)[j]) + b2f(((u16*)&av)[j]));
  *(s8v*)(y + i) = *(s8v*)o;
}

extern "C" hipError_t launch_addinto(void* y, const void* a, long total,
                                     hipStream_t stream) {
  long blocks = (total / 8 + 255) / 256;
  hipLaunchKernelGGL(k_addinto, dim3((uint32_t)blocks), dim3(256), 0, stream,
                     (u16*)y, (const u16*)a, total);
  return hipGetLastError();
}

// ====================================================================
// Grid-wide barrier (device-side, graph-replay-safe).  Used by the
// fused-layer decode path: phases of one layer run inside ONE kernel
// with barriers instead of kernel boundaries (~4 us launch/ramp floor
// each — profiles/decode_kernels_r01.md).
//
// Protocol: `cnt` is a MONOTONIC u64 arrive counter (never reset — the
// launch invariant is cnt % nblocks == 0, preserved because every
// launch/replay runs the same barrier count with the same grid);
// `seq` is the completed-barrier counter.  Each block reads base_seq
// once at kernel start (stable: seq cannot change until every block
// has arrived at barrier 0, which implies every block already read it)
// and spins for seq > base_seq + bar_idx.  Bounded spin -> err flag,
// not a hung GPU.
// ====================================================================

DEVINL int grid_barrier(unsigned long long* cnt, unsigned long long* seq,
                        unsigned long long base_seq, int bar_idx,
                        int nblocks, long spin_limit,
                        uint32_t* err) {
  __shared__ int ok;
  __syncthreads();
  if (threadIdx.x == 0) {
    ok = 1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    unsigned long long t = __hip_atomic_fetch_add(
        cnt, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (t % (unsigned long long)nblocks ==
        (unsigned long long)nblocks - 1ull) {
      __hip_atomic_store(seq, base_seq + bar_idx + 1, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_AGENT);
    } else {
      long spins = 0;
      while (__hip_atomic_load(seq, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT) <=
             base_seq + bar_idx) {
        if (++spins > spin_limit) {
          __hip_atomic_store(err, 1u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
          ok = 0;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  return ok;
}

// microbenchmark: nbar back-to-back barriers (measures the phase-
// boundary cost that replaces a kernel launch in the fused path)
extern "C" __global__ void __launch_bounds__(256)
k_gbar_bench(unsigned long long* cnt, unsigned long long* seq,
             uint32_t* err, int nbar, long spin_limit) {
  const unsigned long long base =
      __hip_atomic_load(seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int b = 0; b < nbar; b++)
    if (!grid_barrier(cnt, seq, base, b, gridDim.x, spin_limit, err))
      return;
}

extern "C" hipError_t launch_gbar_bench(void* cnt, void* seq, void* err,
                                        int nblocks, int nbar,
                                        long spin_limit,
                                        hipStream_t stream) {
  hipLaunchKernelGGL(k_gbar_bench, dim3(nblocks), dim3(256), 0, stream,
                     (unsigned long long*)cnt, (unsigned long long*)seq,
                     (uint32_t*)err, nbar, spin_limit);
  return hipGetLastError();
}

// ====================================================================
// Utility: device-side int32 set/add (for seq-length bookkeeping inside
// graphs where needed)
// ====================================================================

extern "C" __global__ void k_i32_set(int* p, int v) { *p = v; }

extern "C" hipError_t launch_i32_set(void* p, int v, hipStream_t stream) {
  hipLaunchKernelGGL(k_i32_set, dim3(1), dim3(1), 0, stream, (int*)p, v);
  return hipGetLastError();
}
// ====================================================================
// Mixtral sparse-MoE helpers (beyond-parity: the reference has no MoE;
// ROADMAP §5).  k_moe_route fuses the per-row RMSNorm, the router dots
// against Wg[E,H] (f32 accum — bf16 router logits would risk top-k
// flips), the softmax over E, and the HF top-k renormalization
// (modeling_mixtral MixtralTopKRouter), emitting compact (idx, w)
// pairs for the expert-indexed decode GEMVs and optionally a dense
// M x E weight grid for the prefill per-expert GEMM loop.
// One block per row; E <= 64, topk <= 8.
// ====================================================================

extern "C" __global__ void __launch_bounds__(256)
k_moe_route(const u16* __restrict__ h, const float* __restrict__ g,
            const u16* __restrict__ wg, int M, int H, int E, int topk,
            float eps, int* __restrict__ idx, float* __restrict__ wout,
            float* __restrict__ dense) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xf = (float*)smem;           // H floats: normed row
  float* red = xf + H;                // 4 wave partials
  float* el = red + 4;                // E router probs
  const int m = blockIdx.x;
  const u16* hr = h + (size_t)m * H;
  float ss = 0.f;
  for (int i = threadIdx.x; i < H; i += 256) {
    float v = b2f(hr[i]);
    xf[i] = v;
    ss += v * v;
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) ss += __shfl_xor(ss, s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  ss = (red[0] + red[1]) + (red[2] + red[3]);
  const float rn = __frsqrt_rn(ss / H + eps);
  for (int i = threadIdx.x; i < H; i += 256) xf[i] = xf[i] * rn * g[i];
  __syncthreads();
  for (int e = 0; e < E; e++) {
    const u16* wr = wg + (size_t)e * H;
    float d = 0.f;
    for (int i = threadIdx.x; i < H; i += 256) d += xf[i] * b2f(wr[i]);
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) d += __shfl_xor(d, s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) el[e] = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  float mx = el[0];
  for (int e = 1; e < E; e++) mx = fmaxf(mx, el[e]);
  float sum = 0.f;
  for (int e = 0; e < E; e++) { el[e] = __expf(el[e] - mx); sum += el[e]; }
  if (dense)
    for (int e = 0; e < E; e++) dense[(size_t)m * E + e] = 0.f;
  // top-k by repeated argmax (ties -> smallest index, matching the
  // oracle's stable argsort); renormalize the kept probs by their sum
  int sel[8];
  float sw[8];
  float wsum = 0.f;
  for (int j = 0; j < topk; j++) {
    int be = -1;
    float bv = -1.f;
    for (int e = 0; e < E; e++) {
      bool taken = false;
      for (int q = 0; q < j; q++) taken |= (sel[q] == e);
      if (!taken && el[e] > bv) { bv = el[e]; be = e; }
    }
    sel[j] = be;
    sw[j] = bv;
    wsum += bv;
  }
  for (int j = 0; j < topk; j++) {
    idx[(size_t)m * topk + j] = sel[j];
    const float wv = sw[j] / wsum;
    wout[(size_t)m * topk + j] = wv;
    if (dense) dense[(size_t)m * E + sel[j]] = wv;
  }
}

extern "C" hipError_t launch_moe_route(const void* h, const void* g,
                                       const void* wg, int M, int H, int E,
                                       int topk, float eps, void* idx,
                                       void* wout, void* dense,
                                       hipStream_t stream) {
  if (E < 1 || E > 64 || topk < 1 || topk > 8 || topk > E)
    return hipErrorInvalidValue;
  size_t lds = (size_t)H * 4 + 16 + (size_t)E * 4;
  if (lds > 64 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_moe_route, dim3(M), dim3(256), lds, stream,
                     (const u16*)h, (const float*)g, (const u16*)wg, M, H,
                     E, topk, eps, (int*)idx, (float*)wout, (float*)dense);
  return hipGetLastError();
}

// y[m, :H] += w[m * wstride] * x[m, :H]  (bf16 I/O, f32 math) — the
// prefill MoE combine: each expert's GEMM output is folded into the
// residual stream weighted by that row's router prob (0 if unrouted).
extern "C" __global__ void __launch_bounds__(256)
k_moe_scale_add(u16* __restrict__ y, const u16* __restrict__ xin,
                const float* __restrict__ w, long wstride, int M, int H) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)M * H) return;
  const float wv = w[(size_t)(i / H) * wstride];
  if (wv != 0.f) y[i] = f2b(b2f(y[i]) + wv * b2f(xin[i]));
}

extern "C" hipError_t launch_moe_scale_add(void* y, const void* x,
                                           const void* w, long wstride,
                                           int M, int H,
                                           hipStream_t stream) {
  long total = (long)M * H;
  hipLaunchKernelGGL(k_moe_scale_add,
                     dim3((uint32_t)((total + 255) / 256)), dim3(256), 0,
                     stream, (u16*)y, (const u16*)x, (const float*)w,
                     wstride, M, H);
  return hipGetLastError();
}
