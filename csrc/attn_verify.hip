// attn_verify.hip — fused multi-row causal decode attention for the
// speculative verify pass (docs/KERNELS.md "k_attn_verify").
//
// R = 1..16 new rows of ONE sequence at positions n .. n+R-1 (n = *len_ptr,
// read on the device, never written): RoPE of q and k, the KV-pool write and
// the attention over history + the causal triangle of the new rows, in one
// launch plus a small merge launch.
//
// Work split: grid (kv head, KV chunk).  A block owns one kv head and the
// absolute positions [c*chunk, (c+1)*chunk); `chunk` is a multiple of 16 the
// host derives from the pool capacity alone.  Blocks whose chunk starts at or
// past n+R, or lies wholly before every row's window, exit at once.  The 4
// waves of a block divide the G = nh/kvh query heads (wave w owns heads
// w, w+4, ...; TPW = heads per wave); every wave walks the chunk's 16-position
// tiles in lockstep, so a K/V tile is fetched ONCE per block into LDS and
// shared by all G heads' query tiles (the next tile's loads are in flight in
// registers while the current one computes).
//
// New rows: every block ropes the R new K rows into LDS (fp8 pool: quantised
// with k_rope_cache_fp8's absmax/448 rule and converted back, so LDS holds
// what the pool will return) and keeps the R new V rows beside them.  Keys at
// positions >= n always come from that LDS copy, never from the pool; chunk
// 0's block writes them to the pool.  Positions >= n+R are zero-filled.
//
// Math = k_attn_prefill_mfma's: S^T = mfma_16x16x32_bf16(K, Q) (each query's
// max / sum lane-local), P rounded to bf16, fp8 k-scale folded after the QK
// MFMA and v-scale into P, O^T accumulators.  Each live block stores fp32
// (O[hd], m, l) partials per (query head, row) with plain stores;
// k_attn_verify_merge combines a row's chunks in ascending order.  Tiles and
// chunks are position-aligned and masked keys contribute exact zeros, so the
// bits of an output row depend on its position, its q, the pool below it and
// `chunk` only — not on R or on its neighbours.
#include "common.h"
#include <math.h>
#include <type_traits>

typedef short b4v __attribute__((ext_vector_type(4)));
typedef unsigned long long u64b;

#define AV_PSTRIDE(HD) ((HD) + 4)  // fp32 words per partial: O[HD], m, l, pad

template <int HD, bool KV8, int TPW>
__global__ void __launch_bounds__(256)
k_attn_verify(const u16* __restrict__ qkv, void* __restrict__ kc,
              void* __restrict__ vc, float* __restrict__ kS,
              float* __restrict__ vS, const float* __restrict__ cost,
              const float* __restrict__ sint, const int* __restrict__ len_ptr,
              float* __restrict__ scratch, int R, int nh, int kvh, int S,
              int chunk, float scale, float softcap, int window) {
  constexpr int HD2 = HD / 2, HD8 = HD / 8, HD16 = HD / 16, HD32 = HD / 32;
  constexpr int HDP = HD + 8;            // padded LDS row (bank spread)
  constexpr int UNITS = 16 * HD8;        // 8-element units of one tile
  constexpr int UPT = (UNITS + 255) / 256;
  using raw_t = typename std::conditional<KV8, u64b, s8v>::type;

  __shared__ __attribute__((aligned(16))) u16 knew[16 * HDP];
  __shared__ __attribute__((aligned(16))) u16 vnew[16 * HDP];
  __shared__ __attribute__((aligned(16))) u16 ktile[2][16 * HDP];
  __shared__ __attribute__((aligned(16))) u16 vtile[2][16 * HDP];
  __shared__ float knew_s[16], vnew_s[16];
  __shared__ float ktile_s[2][16], vtile_s[2][16];

  const int kvhead = blockIdx.x, c = blockIdx.y, nchunks = gridDim.y;
  const int G = nh / kvh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = *len_ptr;
  const int hi = n + R;                  // one past the last new row
  const int c0 = c * chunk;
  const bool live = c0 < hi && !(window > 0 && c0 + chunk - 1 <= n - window);
  if (!live && c != 0) return;           // chunk 0 still writes the pool

  const int qkvw = (nh + 2 * kvh) * HD;
  const u16* kin = qkv + (size_t)(nh + kvhead) * HD;
  const u16* vin = qkv + (size_t)(nh + kvh + kvhead) * HD;
  const size_t prow = (size_t)kvhead * S;  // this head's first pool row
  const bool writer = c == 0;

  // ---- new K / V rows -> LDS (and, chunk 0, the pool) -----------------
  // fp8 pool: fp32 staging rows alias the (not yet used) K tile buffers
  float* fst = (float*)&ktile[0][0];
  for (int idx = tid; idx < 16 * HD2; idx += 256) {
    const int r = idx / HD2, i = idx % HD2;
    if (r < R) {
      const int pos = min(n + r, S - 1);
      const float c_ = cost[(size_t)pos * HD2 + i];
      const float s_ = sint[(size_t)pos * HD2 + i];
      const u16* kr = kin + (size_t)r * qkvw;
      const float x1 = b2f(kr[i]), x2 = b2f(kr[i + HD2]);
      if (KV8) {
        fst[r * HD + i] = x1 * c_ - x2 * s_;
        fst[r * HD + i + HD2] = x2 * c_ + x1 * s_;
      } else {
        knew[r * HDP + i] = f2b(x1 * c_ - x2 * s_);
        knew[r * HDP + i + HD2] = f2b(x2 * c_ + x1 * s_);
      }
    } else if (!KV8) {
      knew[r * HDP + i] = 0;
      knew[r * HDP + i + HD2] = 0;
    }
  }
  if (!KV8) {
    for (int u = tid; u < UNITS; u += 256) {
      const int r = u / HD8, col = (u % HD8) * 8;
      s8v v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (r < R) v = *(const s8v*)(vin + (size_t)r * qkvw + col);
      *(s8v*)&vnew[r * HDP + col] = v;
    }
    __syncthreads();
    if (writer) {
      for (int u = tid; u < UNITS; u += 256) {
        const int r = u / HD8, col = (u % HD8) * 8;
        if (r < R && n + r < S) {
          const size_t o = (prow + n + r) * HD + col;
          *(s8v*)((u16*)kc + o) = *(const s8v*)&knew[r * HDP + col];
          *(s8v*)((u16*)vc + o) = *(const s8v*)&vnew[r * HDP + col];
        }
      }
    }
  } else {
    // 16 threads per row: absmax, scale, e4m3 bytes, bf16 round trip
    const int r = tid >> 4, sub = tid & 15;
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
      u16* dst = pass ? vnew : knew;
      float* dst_s = pass ? vnew_s : knew_s;
      uint8_t* pool = (uint8_t*)(pass ? vc : kc);
      float* pool_s = pass ? vS : kS;
      if (pass) {
        __syncthreads();                 // K staging consumed
        for (int idx = tid; idx < 16 * HD; idx += 256) {
          const int rr = idx / HD, i = idx % HD;
          if (rr < R) fst[idx] = b2f(vin[(size_t)rr * qkvw + i]);
        }
      }
      __syncthreads();
      float am = 0.f;
      if (r < R)
        for (int i = sub; i < HD; i += 16)
          am = fmaxf(am, fabsf(fst[r * HD + i]));
#pragma unroll
      for (int w = 1; w < 16; w <<= 1) am = fmaxf(am, __shfl_xor(am, w));
      const float sc = fmaxf(am, 1e-8f) / 448.0f;
      for (int u = sub; u < HD8; u += 16) {
        s8v o = {0, 0, 0, 0, 0, 0, 0, 0};
        if (r < R) {
          const u64b b = f32x8_to_fp8(&fst[r * HD + u * 8], 1.0f / sc);
          o = fp8x8_to_bf16(b);
          if (writer && n + r < S)
            *(u64b*)(pool + (prow + n + r) * HD + u * 8) = b;
        }
        *(s8v*)&dst[r * HDP + u * 8] = o;
      }
      if (sub == 0) {
        dst_s[r] = r < R ? sc : 0.f;
        if (r < R && writer && n + r < S) pool_s[prow + n + r] = sc;
      }
    }
  }
  __syncthreads();
  if (!live) return;

  // ---- roped Q fragments (B operand), TPW query heads per wave --------
  const int qcol = lane & 15;            // this lane's query row
  const int kgrp = lane >> 4;
  const int krow4 = kgrp * 4;            // kv rows (QK) / k-index (PV)
  const int qpos = n + qcol;
  s8v qf[TPW][HD32];
#pragma unroll
  for (int j = 0; j < TPW; j++) {
    const int g = wave + 4 * j;
    const bool has = g < G && qcol < R;
    const u16* qp = qkv + (size_t)(has ? qcol : 0) * qkvw +
                    (size_t)(kvhead * G + (g < G ? g : 0)) * HD;
    const int pos = min(has ? qpos : n, S - 1);
    const float* cp = cost + (size_t)pos * HD2;
    const float* sp = sint + (size_t)pos * HD2;
#pragma unroll
    for (int c2 = 0; c2 < HD32; c2++) {
      const int d0 = c2 * 32 + kgrp * 8;
      const bool up = d0 >= HD2;
      const int lo = up ? d0 - HD2 : d0;
      const s8v a = *(const s8v*)(qp + lo);
      const s8v b = *(const s8v*)(qp + lo + HD2);
      u16 o[8];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const float x1 = b2f((u16)a[i]), x2 = b2f((u16)b[i]);
        const float c_ = cp[lo + i], s_ = sp[lo + i];
        const u16 olo = f2b(x1 * c_ - x2 * s_);
        const u16 ohi = f2b(x2 * c_ + x1 * s_);
        o[i] = has ? (up ? ohi : olo) : (u16)0;
      }
      qf[j][c2] = *(s8v*)o;
    }
  }

  // ---- tile walk ------------------------------------------------------
  int t_begin = c0;
  if (window > 0) {
    const int w0 = n - window + 1;       // first key row 0 sees
    if (w0 > t_begin) t_begin = w0 & ~15;
  }
  const int t_end = min(c0 + chunk, hi);
  const int ntiles = (t_end - t_begin + 15) / 16;

  const u16* K0 = (const u16*)kc + prow * HD;
  const u16* V0 = (const u16*)vc + prow * HD;
  const uint8_t* K08 = (const uint8_t*)kc + prow * HD;
  const uint8_t* V08 = (const uint8_t*)vc + prow * HD;

  raw_t kreg[UPT], vreg[UPT];
  float ksr = 0.f, vsr = 0.f;
  // pool rows below n of tile t0 -> registers (nothing at or past n is read)
  auto load_tile = [&](int t0) {
#pragma unroll
    for (int j = 0; j < UPT; j++) {
      const int u = tid + 256 * j;
      const int row = u / HD8, col = (u % HD8) * 8;
      const int t = t0 + row;
      if (u < UNITS && t < n) {
        const size_t o = (size_t)t * HD + col;
        if (KV8) {
          kreg[j] = *(const raw_t*)(K08 + o);
          vreg[j] = *(const raw_t*)(V08 + o);
        } else {
          kreg[j] = *(const raw_t*)(K0 + o);
          vreg[j] = *(const raw_t*)(V0 + o);
        }
      }
    }
    if (KV8 && tid < 16 && t0 + tid < n) {
      ksr = kS[prow + t0 + tid];
      vsr = vS[prow + t0 + tid];
    }
  };
  // registers / the new rows / zeros -> LDS tile `buf`
  auto store_tile = [&](int buf, int t0) {
#pragma unroll
    for (int j = 0; j < UPT; j++) {
      const int u = tid + 256 * j;
      const int row = u / HD8, col = (u % HD8) * 8;
      const int t = t0 + row;
      if (u < UNITS) {
        s8v kv = {0, 0, 0, 0, 0, 0, 0, 0}, vv = {0, 0, 0, 0, 0, 0, 0, 0};
        if (t < n) {
          if constexpr (KV8) {
            kv = fp8x8_to_bf16(kreg[j]);
            vv = fp8x8_to_bf16(vreg[j]);
          } else {
            kv = kreg[j];
            vv = vreg[j];
          }
        } else if (t < hi) {
          kv = *(const s8v*)&knew[(t - n) * HDP + col];
          vv = *(const s8v*)&vnew[(t - n) * HDP + col];
        }
        *(s8v*)&ktile[buf][row * HDP + col] = kv;
        *(s8v*)&vtile[buf][row * HDP + col] = vv;
      }
    }
    if (KV8 && tid < 16) {
      const int t = t0 + tid;
      ktile_s[buf][tid] = t < n ? ksr : t < hi ? knew_s[t - n] : 0.f;
      vtile_s[buf][tid] = t < n ? vsr : t < hi ? vnew_s[t - n] : 0.f;
    }
  };

  float mrun[TPW], lrun[TPW];
  f4v acc_o[TPW][HD16];
#pragma unroll
  for (int j = 0; j < TPW; j++) {
    mrun[j] = -INFINITY;
    lrun[j] = 0.f;
#pragma unroll
    for (int d = 0; d < HD16; d++) acc_o[j][d] = {0.f, 0.f, 0.f, 0.f};
  }

  load_tile(t_begin);
  store_tile(0, t_begin);
  __syncthreads();
  for (int it = 0; it < ntiles; it++) {
    const int t0 = t_begin + 16 * it, buf = it & 1;
    const bool more = it + 1 < ntiles;
    if (more) load_tile(t0 + 16);        // in flight during the compute

    if (wave < G) {
      // S^T tiles: A = K rows from LDS, shared by this wave's heads
      f4v st[TPW];
#pragma unroll
      for (int j = 0; j < TPW; j++) st[j] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c2 = 0; c2 < HD32; c2++) {
        const s8v kf =
            *(const s8v*)&ktile[buf][qcol * HDP + c2 * 32 + kgrp * 8];
#pragma unroll
        for (int j = 0; j < TPW; j++)
          st[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[j][c2],
                                                          st[j], 0, 0, 0);
      }
      float ksc[4], vsc[4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        ksc[r] = KV8 ? ktile_s[buf][krow4 + r] : 1.f;
        vsc[r] = KV8 ? vtile_s[buf][krow4 + r] : 1.f;
      }
      float alpha[TPW];
      b4v pfrag[TPW];
#pragma unroll
      for (int j = 0; j < TPW; j++) {
        // scale + softcap + causal / window mask; element (kv row, qcol)
        float sv[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int t = t0 + krow4 + r;
          float s = st[j][r] * ksc[r] * scale;
          if (softcap > 0.f) s = softcap * tanhf(s / softcap);
          const bool bad = (t > qpos) || (window > 0 && t <= qpos - window);
          sv[r] = bad ? -INFINITY : s;
        }
        float pmax = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
        pmax = fmaxf(pmax, __shfl_xor(pmax, 16));
        pmax = fmaxf(pmax, __shfl_xor(pmax, 32));
        const float mnew = fmaxf(mrun[j], pmax);
        alpha[j] = (mnew == -INFINITY) ? 0.f : __expf(mrun[j] - mnew);
        float psum = 0.f;
        u16 pb[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const float p = (mnew == -INFINITY) ? 0.f : __expf(sv[r] - mnew);
          psum += p;
          pb[r] = KV8 ? f2b(p * vsc[r]) : f2b(p);
        }
        psum += __shfl_xor(psum, 16);
        psum += __shfl_xor(psum, 32);
        lrun[j] = lrun[j] * alpha[j] + psum;
        if (mnew != -INFINITY) mrun[j] = mnew;
        pfrag[j] = *(b4v*)pb;
      }
      // PV: O^T[d][q] += V^T[d][kv] @ P^T[kv][q]
#pragma unroll
      for (int db = 0; db < HD16; db++) {
        u16 vt[4];
#pragma unroll
        for (int r = 0; r < 4; r++)
          vt[r] = vtile[buf][(krow4 + r) * HDP + db * 16 + qcol];
#pragma unroll
        for (int j = 0; j < TPW; j++) {
#pragma unroll
          for (int r = 0; r < 4; r++) acc_o[j][db][r] *= alpha[j];
          acc_o[j][db] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
              *(b4v*)vt, pfrag[j], acc_o[j][db], 0, 0, 0);
        }
      }
    }

    if (more) store_tile(buf ^ 1, t0 + 16);
    __syncthreads();
  }

  // ---- fp32 partials (O, m, l) per (query head, row) -----------------
  if (qcol < R) {
#pragma unroll
    for (int j = 0; j < TPW; j++) {
      const int g = wave + 4 * j;
      if (g < G) {
        float* p = scratch +
                   ((((size_t)kvhead * nchunks + c) * G + g) * R + qcol) *
                       AV_PSTRIDE(HD);
#pragma unroll
        for (int db = 0; db < HD16; db++)
          *(f4v*)(p + db * 16 + krow4) = acc_o[j][db];
        if (kgrp == 0) {
          p[HD] = mrun[j];
          p[HD + 1] = lrun[j];
        }
      }
    }
  }
}

// One block per (query head, row): the row's live chunks combined in
// ascending chunk order (max, rescale, sum), then the bf16 output.
template <int HD>
__global__ void __launch_bounds__(64)
k_attn_verify_merge(const float* __restrict__ scratch, u16* __restrict__ out,
                    const int* __restrict__ len_ptr, int R, int nh, int kvh,
                    int nchunks, int chunk, int window) {
  constexpr int E = HD / 64;
  const int h = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  const int G = nh / kvh, kvhead = h / G, g = h % G;
  const int pos = *len_ptr + r;
  int c_hi = pos / chunk, c_lo = 0;
  if (c_hi > nchunks - 1) c_hi = nchunks - 1;
  if (window > 0 && pos - window + 1 > 0) c_lo = (pos - window + 1) / chunk;
  float m = -INFINITY, l = 0.f, o[E];
#pragma unroll
  for (int e = 0; e < E; e++) o[e] = 0.f;
  for (int c = c_lo; c <= c_hi; c++) {
    const float* p = scratch +
                     ((((size_t)kvhead * nchunks + c) * G + g) * R + r) *
                         AV_PSTRIDE(HD);
    const float mc = p[HD], lc = p[HD + 1];
    if (mc == -INFINITY) continue;       // nothing of this chunk is visible
    const float mn = fmaxf(m, mc);
    const float a = __expf(m - mn), b = __expf(mc - mn);
    l = l * a + lc * b;
#pragma unroll
    for (int e = 0; e < E; e++) o[e] = o[e] * a + p[tid + 64 * e] * b;
    m = mn;
  }
  const float inv = 1.f / l;
  u16* op = out + ((size_t)r * nh + h) * HD;
#pragma unroll
  for (int e = 0; e < E; e++) op[tid + 64 * e] = f2b(o[e] * inv);
}

// scratch: ceil(S / chunk) * nh * R * (hd + 4) fp32 words (checked by the
// binding, `attn_verify_scratch_words`)
extern "C" hipError_t launch_attn_verify(
    const void* qkv, void* kc, void* vc, void* kS, void* vS, int kv8,
    const void* cost, const void* sint, const void* len_ptr, void* out,
    void* scratch, int R, int nh, int kvh, int hd, int S, int chunk,
    float scale, float softcap, int window, hipStream_t stream) {
  if (R < 1 || R > 16 || kvh < 1 || nh % kvh != 0 || S < 1 || chunk < 16 ||
      chunk % 16 != 0)
    return hipErrorInvalidValue;
  const int G = nh / kvh;
  const int tpw = G <= 4 ? 1 : G <= 8 ? 2 : 4;
  if (G > 16 || (hd == 256 && tpw == 4)) return hipErrorInvalidValue;
  const int nchunks = (S + chunk - 1) / chunk;
  dim3 grid(kvh, nchunks);
#define AV_CASE(HDV, KV8V, TPWV)                                             \
  hipLaunchKernelGGL((k_attn_verify<HDV, KV8V, TPWV>), grid, dim3(256), 0,   \
                     stream, (const u16*)qkv, kc, vc, (float*)kS,            \
                     (float*)vS, (const float*)cost, (const float*)sint,     \
                     (const int*)len_ptr, (float*)scratch, R, nh, kvh, S,    \
                     chunk, scale, softcap, window)
#define AV_TPW(HDV, KV8V)                                                    \
  do {                                                                       \
    if (tpw == 1) AV_CASE(HDV, KV8V, 1);                                     \
    else if (tpw == 2) AV_CASE(HDV, KV8V, 2);                                \
    else if (HDV < 256) AV_CASE(HDV < 256 ? HDV : 128, KV8V, 4);             \
  } while (0)
#define AV_HD(HDV)                                                           \
  do {                                                                       \
    if (kv8) AV_TPW(HDV, true); else AV_TPW(HDV, false);                     \
    hipLaunchKernelGGL((k_attn_verify_merge<HDV>), dim3(nh, R), dim3(64), 0, \
                       stream, (const float*)scratch, (u16*)out,             \
                       (const int*)len_ptr, R, nh, kvh, nchunks, chunk,      \
                       window);                                              \
  } while (0)
  if (hd == 64) AV_HD(64);
  else if (hd == 128) AV_HD(128);
  else if (hd == 256) AV_HD(256);
  else return hipErrorInvalidValue;
#undef AV_HD
#undef AV_TPW
#undef AV_CASE
  return hipGetLastError();
}
