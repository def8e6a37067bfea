// spec_sample.hip — stochastic speculative sampling on the device: the
// accept / reject rule of speculative decoding, the residual draw and the
// commit into both engines' state (docs/KERNELS.md "Speculative sampling").
//
//   trows  [k+1, V] bf16   the target's verify-pass logits (softcap applied);
//                          row i scores draft i, row k is the bonus position
//   drows  [>=k, V] fp32   the draft's logits of the steps that drew
//                          drafts[0..k-1] (k_spec_keep keeps them)
//   drafts [k]      i32    the proposals
// Row r of the launch grid is target row r for r <= k and draft row r-k-1
// above.  For a row with maximum M the keep-set is l >= cut = M + T ln(min_p)
// (the expression of k_sample_pick), the weight w_j = exp((l_j - M) / T)
// inside it and 0 outside, Z = sum w_j, the row's probability w_j / Z.
//
// Three launches on one stream, no host read between them:
//   A  k_spec_sample_max   grid (blocks, 2k+1): packed (key, id) row maxima by
//      atomicMax; one thread advances the path's draw counter (stream order
//      puts the bump ahead of every reader).
//   B  k_spec_sample_mass  same grid: the weight sum of every 2048-wide SLICE
//      of every row goes to part[row][slice] with a plain store — per slice,
//      not per block, and reduced in a fixed tree, so Z has the same bits for
//      every block count and every arrival order.  The last-arriving block
//      (ticket) sums each row's slices in slice order, walks the drafts
//         p = w_t(x) / Z_t,  q = w_q(x) / Z_q,  accept iff q > 0, u_i q < p
//      to the first rejected slot m (k: none) and leaves m with the constants
//      of target row m and draft row m in the decision words.
//   C  k_spec_sample_draw  grid (blocks, 1) over row m: Gumbel-argmax of
//      r_j = max(p_j - q_j, 0) (m < k) or p_j (m == k), and in the same pass
//      a second candidate over p_j for a residual that is empty at fp32
//      precision; smallest id wins ties.  The last arriver commits
//      k_spec_verify's commit with the drawn token in place of the argmax and
//      re-arms every scratch word the three launches used.
//
// Random numbers: u_i and the Gumbel noise G_j are hashed from (seed,
// counter, index) under two constant pairs of their own, both unlike the pair
// k_sample_pick_rows derives the draft's noise from — the draft draw, the
// accept test and the residual draw are independent streams even for an
// equal seed and an equal counter.
//
//   scratch [SPEC_SAMPLE_SCRATCH_WORDS] u64, zeroed once by the host:
//     [0 .. 2 SPEC_MAX_K]  row maxima     SS_TICKET_B / SS_TICKET_C  tickets
//     SS_PICK_R / SS_PICK_P  winners      SS_DEC ..  m, then 6 fp32 constants
//   part    [(2 SPEC_MAX_K + 1) * ceil(V / 2048)] fp32, zeroed once
//   ctr     [1] u64: draws so far (never re-armed)
#include "common.h"
#include <math.h>

#define SS_ROWS (2 * SPEC_MAX_K + 1)
#define SS_SLICE 2048
#define SS_TICKET_B (SS_ROWS)
#define SS_TICKET_C (SS_ROWS + 1)
#define SS_PICK_R (SS_ROWS + 2)
#define SS_PICK_P (SS_ROWS + 3)
#define SS_DEC (SS_ROWS + 4)       // u64 word 0: m; words 1..3: 6 fp32
#define SPEC_SAMPLE_SCRATCH_WORDS (SS_DEC + 4)
#define SS_AUTO_BLOCKS 16  // profiles/spec_sample.md
// fp32 slots of the decision area (from word SS_DEC + 1)
#define SS_MT 0
#define SS_ZT 1
#define SS_CUTT 2
#define SS_MQ 3
#define SS_ZQ 4
#define SS_CUTQ 5

DEVINL uint64_t ss_ld(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the two keys of one stream of one launch: c0 / c1 name the stream
DEVINL void ss_keys(uint64_t seed, uint64_t ctr, uint32_t c0, uint32_t c1,
                    uint32_t& k0, uint32_t& k1) {
  k0 = hash32(hash32((uint32_t)ctr ^ c0) ^ (uint32_t)seed);
  k1 = hash32(k0 ^ (uint32_t)(seed >> 32) ^ (uint32_t)(ctr >> 32) ^ c1);
}
#define SS_U_C0 0x9b05688cu   // accept uniforms
#define SS_U_C1 0x1f83d9abu
#define SS_G_C0 0xa54ff53au   // residual Gumbel noise
#define SS_G_C1 0x510e527fu
DEVINL uint32_t ss_rand(uint32_t i, uint32_t k0, uint32_t k1) {
  return hash32(hash32(i ^ k0) ^ k1);
}

struct SsRow {
  const char* p;   // row base
  bool bf;         // bf16 (target) or fp32 (draft)
  bool al;         // 16-byte aligned base
};
DEVINL SsRow ss_row(const u16* trows, const float* drows, int V, int k,
                    int r) {
  SsRow o;
  o.bf = r <= k;
  o.p = o.bf ? (const char*)(trows + (size_t)r * V)
             : (const char*)(drows + (size_t)(r - k - 1) * V);
  o.al = ((uintptr_t)o.p & 15) == 0;
  return o;
}
DEVINL float ss_at(const SsRow& r, int i) {
  return r.bf ? b2f(((const u16*)r.p)[i]) : ((const float*)r.p)[i];
}
// the 8 logits [i0, i0 + 8) of a row: one (bf16) or two (fp32) 16-byte
// vectors where the row is aligned and the octet whole, scalar loads into
// the same slots otherwise; slots at or past V hold -inf
DEVINL void ss_load8(const SsRow& r, int i0, int V, float (&x)[8]) {
  if (r.al && i0 + 8 <= V) {
    if (r.bf) {
      const u4v_ q = *(const u4v_*)((const u16*)r.p + i0);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        x[2 * j] = __uint_as_float(q[j] << 16);
        x[2 * j + 1] = __uint_as_float(q[j] & 0xffff0000u);
      }
    } else {
      const f4v a = *(const f4v*)((const float*)r.p + i0);
      const f4v b = *(const f4v*)((const float*)r.p + i0 + 4);
#pragma unroll
      for (int j = 0; j < 4; j++) { x[j] = a[j]; x[4 + j] = b[j]; }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++)
      x[j] = i0 + j < V ? ss_at(r, i0 + j) : -INFINITY;
  }
}

// weight of logit v in a row with maximum M and keep-set cut `cut`
DEVINL float ss_w(float v, float M, float cut, float inv_temp) {
  return v >= cut ? __expf((v - M) * inv_temp) : 0.0f;
}

DEVINL uint64_t ss_block_max(uint64_t pk, unsigned long long* ws) {
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) {
    const uint64_t o = __shfl_xor((unsigned long long)pk, w);
    if (o > pk) pk = o;
  }
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = pk;
  __syncthreads();
  uint64_t b = ws[0];
  for (int w = 1; w < 4; w++) if (ws[w] > b) b = ws[w];
  return b;
}

// ---------------------------------------------------------------- A
extern "C" __global__ void __launch_bounds__(256)
k_spec_sample_max(const u16* __restrict__ trows,
                  const float* __restrict__ drows, int V, int k,
                  unsigned long long* __restrict__ scratch,
                  unsigned long long* __restrict__ ctr) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *ctr += 1ull;
  const SsRow row = ss_row(trows, drows, V, k, blockIdx.y);
  float mv = -INFINITY;
  int mi = 0x7fffffff;
  const long step = (long)gridDim.x * SS_SLICE;
  for (long base = (long)blockIdx.x * SS_SLICE; base < V; base += step) {
    const int i0 = (int)base + threadIdx.x * 8;
    if (i0 >= V) continue;
    float x[8];
    ss_load8(row, i0, V, x);
#pragma unroll
    for (int j = 0; j < 8; j++)
      if (x[j] > mv) { mv = x[j]; mi = i0 + j; }
  }
  __shared__ unsigned long long ws[4];
  const uint64_t b = ss_block_max(pack_ki(fkey(mv), mi), ws);
  if (threadIdx.x == 0)
    atomicMax(scratch + blockIdx.y, (unsigned long long)b);
}

// ---------------------------------------------------------------- B
extern "C" __global__ void __launch_bounds__(256)
k_spec_sample_mass(const u16* __restrict__ trows,
                   const float* __restrict__ drows, int V, int k,
                   const int* __restrict__ drafts, float inv_temp,
                   float min_p, uint64_t seed,
                   const unsigned long long* __restrict__ ctr,
                   unsigned long long* scratch, float* part) {
  const int r = blockIdx.y, t = threadIdx.x;
  const int nsl = (V + SS_SLICE - 1) / SS_SLICE;
  const SsRow row = ss_row(trows, drows, V, k, r);
  const float lcut = __logf(min_p) / inv_temp;
  const float M = fkey_inv((uint32_t)(ss_ld(scratch + r) >> 32));
  const float cut = M + lcut;
  __shared__ float wsum[2][4];
  __shared__ float Zs[SS_ROWS];
  __shared__ int lastflag;
  int it = 0;
  for (int s = blockIdx.x; s < nsl; s += gridDim.x, it ^= 1) {
    const int i0 = s * SS_SLICE + t * 8;
    float a = 0.0f;
    if (i0 < V) {
      float x[8];
      ss_load8(row, i0, V, x);
#pragma unroll
      for (int j = 0; j < 8; j++) a += ss_w(x[j], M, cut, inv_temp);
    }
    a = wave_reduce_sum(a);
    if ((t & 63) == 0) wsum[it][t >> 6] = a;
    __syncthreads();   // wsum[it] is next written two iterations on
    if (t == 0)
      part[(size_t)r * nsl + s] =
          ((wsum[it][0] + wsum[it][1]) + wsum[it][2]) + wsum[it][3];
  }
  int* ticket = (int*)(scratch + SS_TICKET_B);
  if (t == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const int n = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL,
                                         __HIP_MEMORY_SCOPE_AGENT);
    lastflag = (n == (int)(gridDim.x * gridDim.y) - 1);
  }
  __syncthreads();
  if (!lastflag) return;
  // last arriver: every partial is in.  Thread r sums row r in slice order.
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (t < 2 * k + 1) {
    float z = 0.0f;
    for (int s = 0; s < nsl; s++)
      z += __hip_atomic_load(part + (size_t)t * nsl + s, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    Zs[t] = z;
  }
  __syncthreads();
  if (t != 0) return;
  *ticket = 0;
  uint32_t k0, k1;
  ss_keys(seed, *ctr, SS_U_C0, SS_U_C1, k0, k1);
  int m = k;
  for (int i = 0; i < k; i++) {
    const int x = drafts[i];
    bool ok = false;
    if (x >= 0 && x < V) {
      const float Mt = fkey_inv((uint32_t)(ss_ld(scratch + i) >> 32));
      const float Mq =
          fkey_inv((uint32_t)(ss_ld(scratch + k + 1 + i) >> 32));
      const float p = ss_w(ss_at(ss_row(trows, drows, V, k, i), x), Mt,
                           Mt + lcut, inv_temp) / Zs[i];
      const float q = ss_w(ss_at(ss_row(trows, drows, V, k, k + 1 + i), x),
                           Mq, Mq + lcut, inv_temp) / Zs[k + 1 + i];
      // 24-bit uniform in [0, 1)
      const float u = (float)(ss_rand((uint32_t)i, k0, k1) >> 8) *
                      5.9604645e-8f;
      ok = q > 0.0f && u * q < p;
    }
    if (!ok) { m = i; break; }
  }
  float* dec = (float*)(scratch + SS_DEC + 1);
  const float Mt = fkey_inv((uint32_t)(ss_ld(scratch + m) >> 32));
  dec[SS_MT] = Mt;
  dec[SS_ZT] = Zs[m];
  dec[SS_CUTT] = Mt + lcut;
  if (m < k) {
    const float Mq = fkey_inv((uint32_t)(ss_ld(scratch + k + 1 + m) >> 32));
    dec[SS_MQ] = Mq;
    dec[SS_ZQ] = Zs[k + 1 + m];
    dec[SS_CUTQ] = Mq + lcut;
  }
  *(int*)(scratch + SS_DEC) = m;
}

// ---------------------------------------------------------------- C
extern "C" __global__ void __launch_bounds__(256)
k_spec_sample_draw(const u16* __restrict__ trows,
                   const float* __restrict__ drows, int V, int k,
                   const int* __restrict__ drafts, float inv_temp,
                   uint64_t seed, const unsigned long long* __restrict__ ctr,
                   unsigned long long* scratch, float* part, int nclear,
                   int* t_len, int* t_next, int* t_ring, int* t_nout,
                   int ring_cap, int* d_len, int* d_next, int* d_nout,
                   int* rec, int* nrec, int rec_cap) {
  const int t = threadIdx.x;
  int m = *(const int*)(scratch + SS_DEC);
  m = m < 0 ? 0 : (m > k ? k : m);
  const float* dec = (const float*)(scratch + SS_DEC + 1);
  const float Mt = dec[SS_MT], cutt = dec[SS_CUTT];
  const float rZt = 1.0f / dec[SS_ZT];
  const bool resid = m < k;
  const float Mq = resid ? dec[SS_MQ] : 0.0f;
  const float cutq = resid ? dec[SS_CUTQ] : INFINITY;
  const float rZq = resid ? 1.0f / dec[SS_ZQ] : 0.0f;
  const SsRow trow = ss_row(trows, drows, V, k, m);
  const SsRow qrow = ss_row(trows, drows, V, k, resid ? k + 1 + m : m);
  uint32_t k0, k1;
  ss_keys(seed, *ctr, SS_G_C0, SS_G_C1, k0, k1);
  float rv = -INFINITY, pv = -INFINITY;
  int ri = 0x7fffffff, pi = 0x7fffffff;
  const long step = (long)gridDim.x * SS_SLICE;
  for (long base = (long)blockIdx.x * SS_SLICE; base < V; base += step) {
    const int i0 = (int)base + t * 8;
    if (i0 >= V) continue;
    float x[8], y[8];
    ss_load8(trow, i0, V, x);
    if (resid) ss_load8(qrow, i0, V, y);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      // past the row's end, or outside p's keep-set (NaN included)
      if (i0 + j >= V || !(x[j] >= cutt)) continue;
      const float p = __expf((x[j] - Mt) * inv_temp) * rZt;
      const float q = resid ? ss_w(y[j], Mq, cutq, inv_temp) * rZq : 0.0f;
      // u = (2n + 1) 2^-24 with n < 2^23: every step is exact in fp32, so
      // u lies in [2^-24, 1 - 2^-24] and the noise is finite
      const float u =
          (float)(ss_rand((uint32_t)(i0 + j), k0, k1) >> 9) * 1.1920929e-7f +
          5.9604645e-8f;
      const float g = -__logf(-__logf(u));
      // ascending ids: a strict > keeps the smallest id of equal keys
      const float kp = __logf(p) + g;
      if (kp > pv) { pv = kp; pi = i0 + j; }
      const float rr = p - q;
      if (rr > 0.0f) {
        const float kr = __logf(rr) + g;
        if (kr > rv) { rv = kr; ri = i0 + j; }
      }
    }
  }
  __shared__ unsigned long long ws[2][4];
  __shared__ int lastflag;
  const uint64_t br = ss_block_max(pack_ki(fkey(rv), ri), ws[0]);
  const uint64_t bp = ss_block_max(pack_ki(fkey(pv), pi), ws[1]);
  int* ticket = (int*)(scratch + SS_TICKET_C);
  if (t == 0) {
    atomicMax(scratch + SS_PICK_R, (unsigned long long)br);
    atomicMax(scratch + SS_PICK_P, (unsigned long long)bp);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const int n = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL,
                                         __HIP_MEMORY_SCOPE_AGENT);
    lastflag = (n == (int)gridDim.x - 1);
  }
  __syncthreads();
  if (!lastflag) return;
  // last arriver: both winners are in; re-arm, then thread 0 commits
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  for (int i = t; i < nclear; i += 256) part[i] = 0.0f;
  if (t != 0) return;
  const uint64_t wr = ss_ld(scratch + SS_PICK_R);
  const uint64_t wp = ss_ld(scratch + SS_PICK_P);
  for (int i = 0; i < SPEC_SAMPLE_SCRATCH_WORDS; i++) scratch[i] = 0ull;
  int tok = fkey_inv((uint32_t)(wr >> 32)) > -INFINITY ? unpack_idx(wr)
                                                          : unpack_idx(wp);
  if (tok < 0 || tok >= V) tok = 0;  // NaN-logit insurance
  const int n = *t_len;
  const int no = *t_nout;
  for (int j = 0; j <= m; j++) {
    // accepted drafts passed the range check of the decision walk
    const int x = j < m ? drafts[j] : tok;
    if (no + j >= 0 && no + j < ring_cap) t_ring[no + j] = x;
  }
  *t_nout = no + m + 1;
  *t_next = tok;
  *t_len = n + m + 1;
  *d_len = n + m + 1;
  *d_next = tok;
  *d_nout = 0;
  const int nr = *nrec;
  int* rr = rec + (size_t)((nr < 0 ? 0 : nr) % rec_cap) * SPEC_REC_WORDS;
  rr[0] = m;
  for (int i = 0; i < SPEC_MAX_K; i++) rr[1 + i] = i < k ? drafts[i] : -1;
  *nrec = nr + 1;
}

// blocks <= 0: SS_AUTO_BLOCKS per row; never more than the row has slices
extern "C" hipError_t launch_spec_sample(
    const void* trows, const void* drows, int V, int k, int blocks,
    const void* drafts, float inv_temp, float min_p, uint64_t seed, void* ctr,
    void* scratch, void* part, void* t_len, void* t_next, void* t_ring,
    void* t_nout, int ring_cap, void* d_len, void* d_next, void* d_nout,
    void* rec, void* nrec, int rec_cap, hipStream_t stream) {
  if (k < 1 || k > SPEC_MAX_K || V <= 0 || V > (1 << 30) || ring_cap <= 0 ||
      rec_cap <= 0 || !(inv_temp > 0.0f) || !(min_p >= 0.0f && min_p <= 1.0f))
    return hipErrorInvalidValue;
  const int nsl = (V + SS_SLICE - 1) / SS_SLICE;
  if (blocks <= 0) blocks = SS_AUTO_BLOCKS;
  if (blocks > nsl) blocks = nsl;
  const dim3 grid(blocks, 2 * k + 1);
  hipLaunchKernelGGL(k_spec_sample_max, grid, dim3(256), 0, stream,
                     (const u16*)trows, (const float*)drows, V, k,
                     (unsigned long long*)scratch, (unsigned long long*)ctr);
  hipLaunchKernelGGL(k_spec_sample_mass, grid, dim3(256), 0, stream,
                     (const u16*)trows, (const float*)drows, V, k,
                     (const int*)drafts, inv_temp, min_p, seed,
                     (const unsigned long long*)ctr,
                     (unsigned long long*)scratch, (float*)part);
  hipLaunchKernelGGL(k_spec_sample_draw, dim3(blocks), dim3(256), 0, stream,
                     (const u16*)trows, (const float*)drows, V, k,
                     (const int*)drafts, inv_temp, seed,
                     (const unsigned long long*)ctr,
                     (unsigned long long*)scratch, (float*)part,
                     (2 * k + 1) * nsl, (int*)t_len, (int*)t_next,
                     (int*)t_ring, (int*)t_nout, ring_cap, (int*)d_len,
                     (int*)d_next, (int*)d_nout, (int*)rec, (int*)nrec,
                     rec_cap);
  return hipGetLastError();
}

// ---------------------------------------------------------------- keep
// The end of a sampled draft step: b_logits (fp32 [V]) -> row nout - 1 of the
// kept rows [rows, V], nout read here, after the sampler's commit.  Grid
// covers V once, 4 logits per thread; a row outside [0, rows) is dropped.
extern "C" __global__ void __launch_bounds__(256)
k_spec_keep(const float* __restrict__ src, float* __restrict__ kept, int V,
            int rows, const int* __restrict__ nout) {
  const int r = *nout - 1;
  if (r < 0 || r >= rows) return;
  float* dst = kept + (size_t)r * V;
  const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= V) return;
  if (i0 + 4 <= V && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    *(f4v*)(dst + i0) = *(const f4v*)(src + i0);
  } else {
    for (int i = i0; i < V && i < i0 + 4; i++) dst[i] = src[i];
  }
}

extern "C" hipError_t launch_spec_keep(const void* src, void* kept, int V,
                                       int rows, const void* nout,
                                       hipStream_t stream) {
  if (V <= 0 || V > (1 << 30) || rows < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_spec_keep, dim3((V + 1023) / 1024), dim3(256), 0,
                     stream, (const float*)src, (float*)kept, V, rows,
                     (const int*)nout);
  return hipGetLastError();
}
