// K7 additive-attention scores (fused tanh, never materialising [B,T,S,H]), K11 copy/pointer
// scatter-add, K12 NLL gather, K13 row argmax.
//
// K7 is transcendental-issue bound (B*T*S*H tanh per pass; 2.5 G at cfg2), not MFMA or HBM work:
//   forward   lanes = source position j (the H-sum stays in a register), uh tile transposed through LDS
//   backward  two sweeps with lanes = h (coalesced uh reads, no cross-lane reductions, no atomics on the
//             large tensors): sweep 1 owns (j, h) and sums over t -> d_uh and the d_v partials;
//             sweep 2 owns (t, h) and sums over j -> d_wq.  tanh is recomputed in both.
#include <type_traits>

#include "common.h"

namespace {

template <bool FAST>
__device__ __forceinline__ float tanh_t(float x) {
  if constexpr (FAST) {
    // 1 - 2 / (exp(2x) + 1); saturates cleanly for |x| large (exp -> inf gives 1, exp -> 0 gives -1)
    const float e = __expf(2.f * x);
    return 1.f - __fdividef(2.f, e + 1.f);
  } else {
    return tanhf(x);
  }
}

// Fast path (bf16 operands): with xs = 2 log2(e) (w + u) folded into the operands when they are staged,
//   r = 1 / (2^xs + 1),  tanh = 1 - 2 r,  1 - tanh^2 = 4 r (1 - r):
// one add, v_exp, one add, v_rcp per element; the affine parts (1 - 2 r, the factor 4) are applied to the sums.
// Round 5: the exponential is FACTORED, 2^(w + u) = 2^w 2^u: 2^{ws} is taken once per (target row, feature) and 2^{us} once per (source
// position, feature) where the operands are staged, so the inner loops pay one FMA and ONE quarter-rate instruction (v_rcp) per element
// instead of two (v_exp + v_rcp): 28 -> 16 issue cycles per element in the forward sweep.  Each prescaled argument is clamped at
// +-EXP2_CLAMP so that the product of the two factors stays finite and normal (2^+-124); that alters tanh(wq + uh) only where |wq| or
// |uh| exceeds 21.5 (bf16 fast path only; the f32 parity path calls tanhf).
constexpr float TANH_PRESCALE = 2.8853900817779268f;  // 2 / ln 2
constexpr float EXP2_CLAMP = 62.f;
__device__ __forceinline__ float exp2_factor(float xs) { return __builtin_amdgcn_exp2f(fminf(fmaxf(xs, -EXP2_CLAMP), EXP2_CLAMP)); }
__device__ __forceinline__ float half_sigmoid_prod(float ew, float eu) { return __builtin_amdgcn_rcpf(fmaf(ew, eu, 1.f)); }

constexpr int AJ = 64;   // source positions per workgroup (forward)
constexpr int AH = 64;   // h chunk staged in LDS
constexpr int ATW = 8;   // target rows per wave per chunk (4 waves -> 32 per chunk)

template <typename T, bool FAST>
__global__ __launch_bounds__(256) void additive_fwd_kernel(const float* __restrict__ wq, const T* __restrict__ uh,
                                                           const float* __restrict__ v, float* __restrict__ s, int64_t Tn,
                                                           int64_t S, int64_t H) {
  __shared__ float U[AJ][AH + 1];
  __shared__ float W[4 * ATW][AH];
  __shared__ float V[AH];
  const int64_t b = blockIdx.y, j0 = (int64_t)blockIdx.x * AJ;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t tc = (int64_t)blockIdx.z * 4 * ATW; tc < Tn; tc += (int64_t)gridDim.z * 4 * ATW) {  // (target chunks over blockIdx.z: short memories)
    constexpr float PS = FAST ? TANH_PRESCALE : 1.f;
    float acc[ATW];
#pragma unroll
    for (int i = 0; i < ATW; ++i) acc[i] = 0.f;
    float vsum = 0.f;
    for (int64_t hc = 0; hc < H; hc += AH) {
      __syncthreads();
      for (int e = threadIdx.x; e < AJ * AH; e += 256) {
        const int jj = e / AH, hh = e % AH;
        const int64_t j = j0 + jj, h = hc + hh;
        const float uv = (j < S && h < H) ? PS * Elem<T>::ld(uh + (b * S + j) * H + h) : 0.f;
        U[jj][hh] = FAST ? exp2_factor(uv) : uv;
      }
      for (int e = threadIdx.x; e < 4 * ATW * AH; e += 256) {
        const int tt = e / AH, hh = e % AH;
        const int64_t t = tc + tt, h = hc + hh;
        const float wv = (t < Tn && h < H) ? PS * wq[(b * Tn + t) * H + h] : 0.f;
        W[tt][hh] = FAST ? exp2_factor(wv) : wv;
      }
      if (threadIdx.x < AH) V[threadIdx.x] = (hc + threadIdx.x < H) ? v[hc + threadIdx.x] : 0.f;
      __syncthreads();
#pragma unroll 4
      for (int hh = 0; hh < AH; ++hh) {
        const float u = U[lane][hh], vv = V[hh];
        if constexpr (FAST) {
          vsum += vv;  // sum_h v_h (1 - 2 r_h) = sum_h v_h - 2 sum_h v_h r_h
#pragma unroll
          for (int i = 0; i < ATW; ++i) acc[i] += vv * half_sigmoid_prod(W[wave * ATW + i][hh], u);
        } else {
#pragma unroll
          for (int i = 0; i < ATW; ++i) acc[i] += vv * tanh_t<FAST>(W[wave * ATW + i][hh] + u);
        }
      }
    }
    const int64_t j = j0 + lane;
    if (j < S) {
#pragma unroll
      for (int i = 0; i < ATW; ++i) {
        const int64_t t = tc + wave * ATW + i;
        if (t < Tn) s[(b * Tn + t) * S + j] = FAST ? vsum - 2.f * acc[i] : acc[i];
      }
    }
  }
}

// Few target rows (greedy decoding: T = 1 per step): one wave per source position j, lanes = h (16-byte coalesced read of
// the uh row, no LDS transpose), shuffle reduction of the H-sum.  The tiled kernel above would spend 31/32 of its tanh work
// on absent target rows; this one is bound by streaming uh once (B*S*H*esz bytes).
template <typename T, bool FAST, int TT, int NCH>
__global__ __launch_bounds__(256) void additive_fwd_rowwise_kernel(const float* __restrict__ wq, const T* __restrict__ uh,
                                                                   const float* __restrict__ v, float* __restrict__ s,
                                                                   int64_t Tn, int64_t S, int64_t H) {
  constexpr int E = Vec16<T>::N;
  const int64_t b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  // this lane's slice of the query projection and of v stays in registers for every source position
  float wreg[NCH][TT][E], vreg[NCH][E];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int64_t h0 = ((int64_t)c * 64 + lane) * E;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      vreg[c][e] = h0 < H ? v[h0 + e] : 0.f;
#pragma unroll
      for (int t = 0; t < TT; ++t) wreg[c][t][e] = (h0 < H && t < Tn) ? wq[(b * Tn + t) * H + h0 + e] : 0.f;
    }
  }
  for (int64_t j = wave; j < S; j += nwaves) {
    float acc[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) acc[t] = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int64_t h0 = ((int64_t)c * 64 + lane) * E;
      if (h0 < H) {
        float u[E];
        Vec16<T>::load(uh + (b * S + j) * H + h0, u);
#pragma unroll
        for (int e = 0; e < E; ++e)
#pragma unroll
          for (int t = 0; t < TT; ++t) acc[t] += vreg[c][e] * tanh_t<FAST>(wreg[c][t][e] + u[e]);
      }
    }
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const float r = wave_sum(acc[t]);
      if (lane == 0 && t < Tn) s[(b * Tn + t) * S + j] = r;
    }
  }
}

// sweep 1: thread owns h (256 per workgroup), workgroup owns BJ source positions; sums over t.
constexpr int BJ = 16;
constexpr int BTC = 32;  // t chunk staged in LDS

template <typename T, bool FAST>
__global__ __launch_bounds__(256) void additive_bwd_uh_kernel(const float* __restrict__ ds, const float* __restrict__ wq,
                                                              const T* __restrict__ uh, const float* __restrict__ v,
                                                              float* __restrict__ d_uh, float* __restrict__ d_v, int64_t Tn,
                                                              int64_t S, int64_t H) {
  __shared__ float DS[BTC][BJ];
  const int64_t b = blockIdx.z, j0 = (int64_t)blockIdx.x * BJ, h = (int64_t)blockIdx.y * 256 + threadIdx.x;
  const bool h_ok = h < H;
  float u[BJ], acc[BJ];
#pragma unroll
  for (int jj = 0; jj < BJ; ++jj) {
    const int64_t j = j0 + jj;
    u[jj] = (h_ok && j < S) ? (FAST ? TANH_PRESCALE : 1.f) * Elem<T>::ld(uh + (b * S + j) * H + h) : 0.f;
    if constexpr (FAST) u[jj] = exp2_factor(u[jj]);  // 2^{us}: the factored form (see exp2_factor)
    acc[jj] = 0.f;
  }
  float dv = 0.f, gsum = 0.f;
  for (int64_t tc = 0; tc < Tn; tc += BTC) {
    __syncthreads();
    for (int e = threadIdx.x; e < BTC * BJ; e += 256) {
      const int tt = e / BJ, jj = e % BJ;
      const int64_t t = tc + tt, j = j0 + jj;
      DS[tt][jj] = (t < Tn && j < S) ? ds[(b * Tn + t) * S + j] : 0.f;
    }
    __syncthreads();
    const int tmax = (int)((Tn - tc) < BTC ? (Tn - tc) : BTC);
    for (int tt = 0; tt < tmax; ++tt) {
      float w = h_ok ? (FAST ? TANH_PRESCALE : 1.f) * wq[(b * Tn + tc + tt) * H + h] : 0.f;
      if constexpr (FAST) w = exp2_factor(w);
#pragma unroll
      for (int jj = 0; jj < BJ; ++jj) {
        const float g = DS[tt][jj];
        if constexpr (FAST) {
          const float r = half_sigmoid_prod(w, u[jj]);
          const float gr = g * r;
          acc[jj] += gr - gr * r;  // g r (1 - r); the factor 4 is applied once at the end
          dv += gr;                // sum g tanh = sum g - 2 sum g r
          gsum += g;
        } else {
          const float th = tanh_t<FAST>(w + u[jj]);
          acc[jj] += g * (1.f - th * th);
          dv += g * th;
        }
      }
    }
  }
  if (h_ok) {
    const float vh = FAST ? 4.f * v[h] : v[h];
#pragma unroll
    for (int jj = 0; jj < BJ; ++jj) {
      const int64_t j = j0 + jj;
      if (j < S) d_uh[(b * S + j) * H + h] = vh * acc[jj];
    }
    atomicAdd(d_v + h, FAST ? gsum - 2.f * dv : dv);
  }
}

// sweep 2: thread owns h, workgroup owns CT target rows; sums over all j.
constexpr int CT = 8;
constexpr int CJC = 64;  // j chunk staged in LDS

template <typename T, bool FAST>
__global__ __launch_bounds__(256) void additive_bwd_wq_kernel(const float* __restrict__ ds, const float* __restrict__ wq,
                                                              const T* __restrict__ uh, const float* __restrict__ v,
                                                              float* __restrict__ d_wq, int64_t Tn, int64_t S, int64_t H,
                                                              int tblocks, int64_t j_per) {
  // blockIdx.x = (source-position chunk, target-row block): with few target rows (T = 40 -> 5 blocks) one workgroup per
  // (t block, h block, b) left the chip at one wave per SIMD; the j range is split and partial sums are added atomically
  // into the pre-zeroed d_wq when there is more than one chunk.
  __shared__ float DS[CT][CJC];
  const int64_t b = blockIdx.z, t0 = (int64_t)(blockIdx.x % tblocks) * CT, h = (int64_t)blockIdx.y * 256 + threadIdx.x;
  const int64_t j_begin = (int64_t)(blockIdx.x / tblocks) * j_per, j_end = (j_begin + j_per < S) ? j_begin + j_per : S;
  const bool split = j_per < S;
  const bool h_ok = h < H;
  float w[CT], acc[CT];
#pragma unroll
  for (int tt = 0; tt < CT; ++tt) {
    const int64_t t = t0 + tt;
    w[tt] = (h_ok && t < Tn) ? (FAST ? TANH_PRESCALE : 1.f) * wq[(b * Tn + t) * H + h] : 0.f;
    if constexpr (FAST) w[tt] = exp2_factor(w[tt]);
    acc[tt] = 0.f;
  }
  for (int64_t jc = j_begin; jc < j_end; jc += CJC) {
    __syncthreads();
    for (int e = threadIdx.x; e < CT * CJC; e += 256) {
      const int tt = e / CJC, jj = e % CJC;
      const int64_t t = t0 + tt, j = jc + jj;
      DS[tt][jj] = (t < Tn && j < j_end) ? ds[(b * Tn + t) * S + j] : 0.f;
    }
    __syncthreads();
    const int jmax = (int)((j_end - jc) < CJC ? (j_end - jc) : CJC);
    for (int jj = 0; jj < jmax; ++jj) {
      float u = h_ok ? (FAST ? TANH_PRESCALE : 1.f) * Elem<T>::ld(uh + (b * S + jc + jj) * H + h) : 0.f;
      if constexpr (FAST) u = exp2_factor(u);
#pragma unroll
      for (int tt = 0; tt < CT; ++tt) {
        if constexpr (FAST) {
          const float r = half_sigmoid_prod(w[tt], u);
          const float gr = DS[tt][jj] * r;
          acc[tt] += gr - gr * r;
        } else {
          const float th = tanh_t<FAST>(w[tt] + u);
          acc[tt] += DS[tt][jj] * (1.f - th * th);
        }
      }
    }
  }
  if (h_ok) {
    const float vh = FAST ? 4.f * v[h] : v[h];
#pragma unroll
    for (int tt = 0; tt < CT; ++tt) {
      const int64_t t = t0 + tt;
      if (t < Tn) {
        if (split) atomicAdd(d_wq + (b * Tn + t) * H + h, vh * acc[tt]);
        else d_wq[(b * Tn + t) * H + h] = vh * acc[tt];
      }
    }
  }
}

// ---- K22 (round 5): the greedy step's additive attention as ONE launch ------------------------------------------------------------
// tanh(a + b) = 1 - 2 / (e^{2a} e^{2b} + 1): with EU = e^{2 uh} cached per (source position, feature) when the memory is encoded (uh is
// the same in all T steps) and EW = e^{2 wq} computed once per (item, feature) per step, an element costs one FMA, ONE reciprocal and
// one FMA -- the exponentials move from O(T S H) to O((T + S) H).  Both arguments are clamped at +-EXP_CLAMP so that the product stays
// finite and normal in f32 (e^{+-86}); that changes tanh(wq + uh) only where |wq| or |uh| exceeds 21.5, far outside what a linear map of
// LayerNorm outputs produces (and there tanh is saturated unless the two nearly cancel).
// One workgroup of 16 waves per item: (1) scores over the EU rows into LDS, (2) masked softmax in LDS (+ the copy prior's
// renormalisation p w / (1e-8 + sum p w), CaSE/Model.py:81-82), (3) ctx = sum_j p_j value_j over the memory rows -- the score sweep, the
// softmax, the cast and the [1, S] x [S, H] product of the four-launch form, and the four ATen launches of the prior.  Rows of masked
// source positions are never loaded.  HBM-bound: S H (2 + 2) bytes per item.
constexpr float EXP_CLAMP = 43.f;
constexpr int PA_WAVES = 16, PA_H = 512;

__global__ __launch_bounds__(256) void additive_key_exp_kernel(const float* __restrict__ uh, bf16_t* __restrict__ eu, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    const float4 a = reinterpret_cast<const float4*>(uh)[2 * i], b = reinterpret_cast<const float4*>(uh)[2 * i + 1];
    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    float y[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = __expf(fminf(fmaxf(2.f * x[e], -EXP_CLAMP), EXP_CLAMP));
    Vec16<bf16_t>::store(eu + 8 * i, y);
  }
}

// sums of four per-lane values over the 64 lanes, all at once: two v_permlane32_swap + one v_permlane16_swap fold the wave's four
// 16-lane rows so that lane row g keeps value g, four rotate-adds inside the row finish it.  Returns the total of r<g> in every lane of
// lane row g (lanes 16 g .. 16 g + 15).
__device__ __forceinline__ float row_sum4(float r0, float r1, float r2, float r3) {
  const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(r0), __float_as_uint(r2), false, false);  // [r0.lo | r2.lo], [r0.hi | r2.hi]
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(r1), __float_as_uint(r3), false, false);
  const float A = __uint_as_float(a[0]) + __uint_as_float(a[1]);  // lanes 0-31: r0 over {l, l + 32}; lanes 32-63: r2
  const float B = __uint_as_float(b[0]) + __uint_as_float(b[1]);  // r1 | r3
  const auto c = __builtin_amdgcn_permlane16_swap(__float_as_uint(A), __float_as_uint(B), false, false);
  float t = __uint_as_float(c[0]) + __uint_as_float(c[1]);        // lane row 0: r0, 1: r1, 2: r2, 3: r3 (16 partial sums each)
  t += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(t), 0x128, 0xf, 0xf, false));  // row_ror:8
  t += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(t), 0x124, 0xf, 0xf, false));  // row_ror:4
  t += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(t), 0x122, 0xf, 0xf, false));  // row_ror:2
  t += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(t), 0x121, 0xf, 0xf, false));  // row_ror:1
  return t;
}

// K22's two sweeps (e^{2 uh} rows, then the value rows: 1 GB each at cfg 4, every byte once per launch) are read NON-TEMPORAL for the same
// reason as K21's stream (attn_mqa.hip): the step's reusable data stays in the Infinity Cache.  -DCASE_STREAM_DEFAULT_POLICY: default policy (A/B).
#ifndef CASE_STREAM_DEFAULT_POLICY
typedef unsigned int pa_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 pa_nt_load(const void* p) {
  const pa_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const pa_u32x4*>(p));
  return make_uint4(v[0], v[1], v[2], v[3]);
}
#define PA_STREAM_LOAD(P) pa_nt_load(P)
#else
#define PA_STREAM_LOAD(P) (*reinterpret_cast<const uint4*>(P))
#endif
__global__ __launch_bounds__(64 * PA_WAVES) void pointer_attend_decode_kernel(
    const float* __restrict__ wq, const float* __restrict__ wq_add, const bf16_t* __restrict__ eu, const float* __restrict__ v, const bf16_t* __restrict__ mem,
    const uint8_t* __restrict__ col_valid, const uint8_t* __restrict__ row_valid, const float* __restrict__ prior, bf16_t* __restrict__ ctx,
    float* __restrict__ p_out, float* __restrict__ copy_out, const int64_t S) {
  extern __shared__ __attribute__((aligned(16))) float pa_smem[];
  float* sc = pa_smem;                              // [S] scores, then probabilities
  float* red = pa_smem + ((S + 3) & ~(int64_t)3);   // [PA_WAVES][PA_H] partial contexts; its head doubles as the reduction scratch
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = blockIdx.x;
  const uint8_t* cv = col_valid ? col_valid + b * S : nullptr;
  const bool row_ok = row_valid ? row_valid[b] != 0 : true;
  float ew[8], vv[8];
  {
    float w8[8];
    Vec16<float>::load(wq + b * PA_H + 8 * lane, *reinterpret_cast<float(*)[4]>(w8));
    Vec16<float>::load(wq + b * PA_H + 8 * lane + 4, *reinterpret_cast<float(*)[4]>(w8 + 4));
    if (wq_add) {  // the step-invariant part of the query projection (its feature columns and the bias), kept in f32
      float c8[8];
      Vec16<float>::load(wq_add + b * PA_H + 8 * lane, *reinterpret_cast<float(*)[4]>(c8));
      Vec16<float>::load(wq_add + b * PA_H + 8 * lane + 4, *reinterpret_cast<float(*)[4]>(c8 + 4));
#pragma unroll
      for (int e = 0; e < 8; ++e) w8[e] += c8[e];
    }
    Vec16<float>::load(v + 8 * lane, *reinterpret_cast<float(*)[4]>(vv));
    Vec16<float>::load(v + 8 * lane + 4, *reinterpret_cast<float(*)[4]>(vv + 4));
#pragma unroll
    for (int e = 0; e < 8; ++e) ew[e] = __expf(fminf(fmaxf(2.f * w8[e], -EXP_CLAMP), EXP_CLAMP));
  }
  float vs = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) vs += vv[e];
  vs = wave_sum(vs);
  // (1) s_j = sum_h v_h tanh(wq_h + uh_jh) = sum_h v_h - 2 sum_h v_h / (EW_h EU_jh + 1).  A wave takes four rows at a time (16 bytes of
  // each per lane) and sums them with ONE transposing reduction (row_sum4): six ds_bpermute steps per row were costing the stage
  // more than its reciprocals -- the first build spent 0.28 ms per launch in them, above its HBM time.  The next four rows are
  // requested before the current four are evaluated.
  const bf16_t* eub = eu + b * S * PA_H + 8 * lane;
  uint4 raw[4], nxt[4];
  bool ok[4], nok[4];
#define PA_LOAD(R, OK, J0)                                                     \
  _Pragma("unroll") for (int u = 0; u < 4; ++u) {                              \
    const int64_t j = (J0) + u * PA_WAVES;                                     \
    OK[u] = j < S && (!cv || cv[j]); /* wave-uniform */                        \
    if (OK[u]) R[u] = PA_STREAM_LOAD(eub + j * PA_H);                          \
  }
  PA_LOAD(raw, ok, (int64_t)wave)
  for (int64_t j0 = wave; j0 < S; j0 += 4 * PA_WAVES) {
    PA_LOAD(nxt, nok, j0 + 4 * PA_WAVES)
    float r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      r[u] = 0.f;
      if (ok[u]) {
        float x[8];
        Vec16<bf16_t>::unpack(raw[u], x);
#pragma unroll
        for (int e = 0; e < 8; ++e) r[u] += vv[e] * __builtin_amdgcn_rcpf(fmaf(ew[e], x[e], 1.f));
      }
    }
    const float tot = row_sum4(r[0], r[1], r[2], r[3]);  // lane row g holds the sum of r[g]
    const int g = lane >> 4;
    const int64_t j = j0 + g * PA_WAVES;
    const bool okg = g == 0 ? ok[0] : g == 1 ? ok[1] : g == 2 ? ok[2] : ok[3];
    if ((lane & 15) == 0 && j < S) sc[j] = okg ? vs - 2.f * tot : -INFINITY;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      raw[u] = nxt[u];
      ok[u] = nok[u];
    }
  }
#undef PA_LOAD
  __syncthreads();
  // (2) masked softmax over the S scores (exact zeros for a row without a valid key or an invalid target row)
  float mx = -INFINITY;
  for (int64_t j = threadIdx.x; j < S; j += 64 * PA_WAVES) mx = fmaxf(mx, sc[j]);
  mx = block_max(mx, red);
  float sum = 0.f;
  for (int64_t j = threadIdx.x; j < S; j += 64 * PA_WAVES) {
    const float e = mx == -INFINITY ? 0.f : __expf(sc[j] - mx);
    sc[j] = e;
    sum += e;
  }
  sum = block_sum(sum, red);
  const float inv = (row_ok && sum > 0.f) ? 1.f / sum : 0.f;
  float wsum = 0.f;
  for (int64_t j = threadIdx.x; j < S; j += 64 * PA_WAVES) {
    const float pj = sc[j] * inv;
    sc[j] = pj;
    p_out[b * S + j] = pj;
    if (prior) wsum += pj * prior[b * S + j];
  }
  if (prior) {
    wsum = block_sum(wsum, red);
    const float winv = 1.f / (1e-8f + wsum);
    for (int64_t j = threadIdx.x; j < S; j += 64 * PA_WAVES) copy_out[b * S + j] = sc[j] * prior[b * S + j] * winv;
  }
  __syncthreads();
  // (3) ctx = sum_j p_j value_j; rows with p_j == 0 (masked positions) are not read
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  const bf16_t* mb = mem + b * S * PA_H + 8 * lane;
  // as in sweep (1): the next four rows are requested before the current four are accumulated
  uint4 vraw[4], vnxt[4];
  float pj[4], pn[4];
#define PA_VLOAD(R, P, J0)                                                     \
  _Pragma("unroll") for (int u = 0; u < 4; ++u) {                              \
    const int64_t j = (J0) + u * PA_WAVES;                                     \
    P[u] = j < S ? sc[j] : 0.f; /* wave-uniform */                             \
    if (P[u] != 0.f) R[u] = PA_STREAM_LOAD(mb + j * PA_H);                     \
  }
  PA_VLOAD(vraw, pj, (int64_t)wave)
  for (int64_t j0 = wave; j0 < S; j0 += 4 * PA_WAVES) {
    PA_VLOAD(vnxt, pn, j0 + 4 * PA_WAVES)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (pj[u] != 0.f) {
        float x[8];
        Vec16<bf16_t>::unpack(vraw[u], x);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj[u], x[e], acc[e]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      vraw[u] = vnxt[u];
      pj[u] = pn[u];
    }
  }
#undef PA_VLOAD
#pragma unroll
  for (int e = 0; e < 8; ++e) red[wave * PA_H + 8 * lane + e] = acc[e];
  __syncthreads();
  if (threadIdx.x < PA_H) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < PA_WAVES; ++w) t += red[w * PA_H + threadIdx.x];  // fixed order: bit-identical from launch to launch
    ctx[b * PA_H + threadIdx.x] = f32_to_bf16(t);
  }
}

// ---- K23 (round 5): the greedy step's pointer-generator head in one launch ----------------------------------------------------------
// gen = softmax(logits); pm = softmax(mix logits); dist = pm_0 gen + scatter(pm_k copy_k over the sorted source keys); id = argmax dist
// (CaSE/Model.py:34-48, :112-117, common/Utils.py:156-168 with the lowest index on ties).  One workgroup per answer row keeps the whole
// vocabulary row in LDS (V <= 36 000 floats): the five passes over the [B, V] matrix of the separate launches (softmax, p0 x gen,
// zero-fill + scatter, sum, argmax: ~0.2 ms per step at B 256 x V 30 522) become one read of the logits and one write of each output.
constexpr int PH_THREADS = 1024, PH_MAX_MEM = 4;
struct HeadArgs {
  const float* logits;      // [B, V]
  const float* mix_logits;  // [B, 1 + nmem]
  const uint32_t* keys;     // [B, S] sorted (token << 15 | position), 0xFFFFFFFF = no token
  const float* copy[PH_MAX_MEM];  // copy_k [B, len_k]: pointer weights of memory k (positions offset by the lengths before it)
  int64_t len[PH_MAX_MEM];
  float* gen;               // [B, V] or null
  float* dist;              // [B, V]
  int64_t* ids;             // [B]
  float* top;               // [B] or null: dist[id]
  int64_t V, S;
  int nmem;
  float* row_ws;            // the wide forms: [B, row_stride] f32 rows in device memory (null: the LDS forms)
  int64_t row_stride;
};

// ---- K32: the n-gram ban behind the row build ------------------------------------------------------------------------------------------
// hist [R, Tmax] int32 holds what a row has emitted so far (BOS excluded); at step t with n = no_repeat_ngram, token v is banned when some
// j <= t - n has hist[j .. j + n - 2] == hist[t - n + 1 .. t - 1] and hist[j + n - 1] == v (n = 1: every token of the history).  A banned
// entry of the row becomes 0.0; nothing else changes and nothing is renormalised.  No ban for t < n, for a history that holds `eos`, or (the
// caller's check) for a sampler row that has ended.  Ids outside [0, V) are ignored.  The history is staged in `stage` (t <= NB_MAX_T ints:
// the value half of the key staging, dead behind the row build); thread j owns window j; several threads may write the same 0.0.
constexpr int NB_MAX_T = 256;
struct BanArgs {
  int32_t* hist;         // [R, Tmax]; K23 / K28 append their emitted id at [r, t]
  int64_t Tmax, eos;
  int t, n;
};

// Every thread of the block calls it; `row` is readable by every thread before and after (barriers inside).
__device__ __forceinline__ void ngram_ban_row(float* row, const int64_t V, const int32_t* __restrict__ h, const int t, const int n, const int64_t eos,
                                              int* stage) {
  if (n < 1 || t < n || t > NB_MAX_T) return;  // (block-uniform)
  const int tid = threadIdx.x, nt = blockDim.x;
  int has_eos = 0;
  for (int i = tid; i < t; i += nt) {
    const int x = h[i];
    stage[i] = x;
    has_eos |= (int64_t)x == eos;
  }
  if (__syncthreads_or(has_eos)) return;  // (the barrier that publishes the staged history)
  const int s0 = t - n + 1;               // the suffix hist[s0 .. t - 1]: n - 1 tokens
  for (int j = tid; j <= t - n; j += nt) {
    bool same = true;
    for (int k = 0; k < n - 1; ++k) same = same && stage[j + k] == stage[s0 + k];
    const int v = stage[j + n - 1];
    if (same && v >= 0 && (int64_t)v < V) row[v] = 0.f;
  }
  __syncthreads();
}

// ---- the decoding rules behind K32: min_length and banned ids ---------------------------------------------------------------------------------
// At step t (= the tokens the row has emitted) row[eos] becomes 0.0 while t < min_len, and row[v] becomes 0.0 for every v of the row's item's
// list bad[0 .. nbad) (the list of item r / rows_per_item: bad + item * bad_stride; stride 0 = one list for every item).  Ids outside [0, V) are
// ignored (-1 pads a list), duplicates are harmless, nothing is renormalised; a row left all zero behaves as an all-zero row does (id 0,
// value 0).  Unlike K32 there is no "history holds eos" clause and no step bound.  The `_rules` instances take the ban's operands too, with
// n = 0 (and hist == nullptr) allowed: no ban, and nothing is appended.
constexpr int RR_MAX_BAD = 256;
struct RuleArgs {
  const int32_t* bad;  // [nbad] or [items, nbad] int32, null with nbad = 0
  int64_t eos, bad_stride, rows_per_item;
  int t, min_len, nbad;
};
struct RuleBanArgs : BanArgs {
  RuleArgs rl;
};
template <bool RULES>
struct TailArgs {
  typedef BanArgs type;
};
template <>
struct TailArgs<true> {
  typedef RuleBanArgs type;
};

// Every thread of the block calls it; `row` is readable by every thread before and after (the barrier inside).  Plain stores of 0.f; several
// threads may write the same zero.
__device__ __forceinline__ void row_rules_row(float* row, const int64_t V, const RuleArgs& rl, const int64_t r) {
  const int32_t* __restrict__ bad = rl.bad + (r / rl.rows_per_item) * rl.bad_stride;
  if (threadIdx.x == 0 && rl.t < rl.min_len && rl.eos >= 0 && rl.eos < V) row[rl.eos] = 0.f;
  for (int i = threadIdx.x; i < rl.nbad; i += blockDim.x) {
    const int v = bad[i];
    if (v >= 0 && (int64_t)v < V) row[v] = 0.f;
  }
  __syncthreads();
}

// the row build shared by K23 and its beam form: row[0 .. V) = pm_0 softmax(logits) + the pointer mass of the sorted source keys (gen written
// on the way when asked for).  Ends behind a barrier: every thread may read the whole row.
// WIDE (the row in device memory): the exponentials are formed from the logits again where the LDS form reads them back from the row -- the
// same instructions on the same operands, so the same bits, with one write of the row where the LDS form makes three.
template <bool WIDE = false>
__device__ __forceinline__ void pointer_head_build_row(const HeadArgs& a, float* row, uint32_t* tk, float* tv, float* red, const int64_t b) {
  const int64_t V = a.V;
  const int tid = threadIdx.x;
  // the mixing probabilities (1 + nmem <= 5 values; every thread computes them)
  float pm[1 + PH_MAX_MEM];
  {
    float mm = -INFINITY, ss = 0.f;
#pragma unroll
    for (int k = 0; k <= PH_MAX_MEM; ++k) pm[k] = k <= a.nmem ? a.mix_logits[b * (a.nmem + 1) + k] : -INFINITY;
#pragma unroll
    for (int k = 0; k <= PH_MAX_MEM; ++k) mm = fmaxf(mm, pm[k]);
#pragma unroll
    for (int k = 0; k <= PH_MAX_MEM; ++k) {
      pm[k] = __expf(pm[k] - mm);  // exp(-inf) = 0 for the slots behind nmem
      ss += pm[k];
    }
#pragma unroll
    for (int k = 0; k <= PH_MAX_MEM; ++k) pm[k] /= ss;
  }
  const float* lg = a.logits + b * V;
  float mx = -INFINITY;
  for (int64_t i = tid; i < V; i += PH_THREADS) {
    const float x = lg[i];
    if constexpr (!WIDE) row[i] = x;
    mx = fmaxf(mx, x);
  }
  mx = block_max(mx, red);
  float sum = 0.f;
  for (int64_t i = tid; i < V; i += PH_THREADS) {
    const float e = __expf((WIDE ? lg[i] : row[i]) - mx);
    if constexpr (!WIDE) row[i] = e;
    sum += e;
  }
  sum = block_sum(sum, red);
  const float inv = 1.f / sum;
  for (int64_t i = tid; i < V; i += PH_THREADS) {
    const float g = (WIDE ? __expf(lg[i] - mx) : row[i]) * inv;
    if (a.gen) a.gen[b * V + i] = g;
    row[i] = pm[0] * g;
  }
  __syncthreads();
  // pointer mass: the keys of a row are sorted by token, so a token's positions form runs; the last lane of a run inside a chunk sums it
  // (fixed order) and adds it to the row -- a token's run in a later chunk is added by a later iteration: no atomics, scheduling-free
  const uint32_t* k = a.keys + b * a.S;
  for (int64_t base = 0; base < a.S; base += PH_THREADS) {
    const int64_t i = base + tid;
    const uint32_t key = i < a.S ? k[i] : 0xFFFFFFFFu;
    const bool valid = key != 0xFFFFFFFFu;
    float w = 0.f;
    if (valid) {
      int64_t pos = key & 0x7FFFu;
      bool done = false;
#pragma unroll
      for (int m = 0; m < PH_MAX_MEM; ++m) {  // (compile-time m: pm[] stays in registers)
        if (m < a.nmem && !done) {
          if (pos < a.len[m]) {
            w = pm[m + 1] * a.copy[m][b * a.len[m] + pos];
            done = true;
          }
          pos -= a.len[m];
        }
      }
    }
    tk[tid] = valid ? (key >> 15) : 0xFFFFFFFFu;
    tv[tid] = w;
    if (tid == 0) tk[PH_THREADS] = 0xFFFFFFFEu;
    __syncthreads();
    const uint32_t tok = tk[tid];
    if (valid && tok != tk[tid + 1]) {
      int j = tid;
      while (j > 0 && tk[j - 1] == tok) --j;
      float s2 = 0.f;
      for (; j <= tid; ++j) s2 += tv[j];
      if (s2 != 0.f && tok < (uint32_t)V) row[tok] += s2;
    }
    __syncthreads();
  }
}

// WIDE: the row lives in a.row_ws (device memory) and LDS holds the staging and scratch only.  A workgroup reads back its own global stores
// behind __syncthreads() (one CU, one L1); no row is shared between workgroups.
// RULES (the `_rules` instances; BAN is set there too): `nb` carries the rules behind the ban's operands, and n = 0 / hist == nullptr means no ban.
template <bool BAN, bool WIDE = false, bool RULES = false>
__global__ __launch_bounds__(PH_THREADS) void pointer_head_decode_kernel(const HeadArgs a, const typename TailArgs<RULES>::type nb) {
  extern __shared__ __attribute__((aligned(16))) float ph_smem[];
  float* row = WIDE ? a.row_ws + (int64_t)blockIdx.x * a.row_stride : ph_smem;  // [V]
  uint32_t* tk = reinterpret_cast<uint32_t*>(WIDE ? ph_smem : ph_smem + ((a.V + 3) & ~(int64_t)3));  // [PH_THREADS + 1]
  float* tv = reinterpret_cast<float*>(tk + PH_THREADS + 4);                       // [PH_THREADS]
  float* red = tv + PH_THREADS;                                                    // [64] reduction scratch
  __shared__ int64_t best_i[16];
  __shared__ float best_v[16];
  const int64_t b = blockIdx.x, V = a.V;
  const int tid = threadIdx.x;
  pointer_head_build_row<WIDE>(a, row, tk, tv, red, b);
  if constexpr (BAN) ngram_ban_row(row, V, nb.hist + b * nb.Tmax, nb.t, nb.n, nb.eos, reinterpret_cast<int*>(tv));  // (n = 0: returns before it reads)
  if constexpr (RULES) row_rules_row(row, V, nb.rl, b);
  // outputs: the distribution row and its argmax (lowest index on ties)
  float bv = -INFINITY;
  int64_t bi = V;
  for (int64_t i = tid; i < V; i += PH_THREADS) {
    const float x = row[i];
    if (a.dist) a.dist[b * V + i] = x;
    if (x > bv) {  // indices ascend within a thread: the first maximum is kept
      bv = x;
      bi = i;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int64_t oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if ((tid & 63) == 0) {
    best_v[tid >> 6] = bv;
    best_i[tid >> 6] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < PH_THREADS / 64; ++w)
      if (best_v[w] > bv || (best_v[w] == bv && best_i[w] < bi)) {
        bv = best_v[w];
        bi = best_i[w];
      }
    a.ids[b] = bi < V ? bi : 0;
    if (a.top) a.top[b] = bv;
    if constexpr (BAN) {
      if (!RULES || nb.hist) nb.hist[b * nb.Tmax + nb.t] = (int32_t)(bi < V ? bi : 0);
    }
  }
}

// ---- K24: the beam step's head = K23 with a top-W tail ---------------------------------------------------------------------------
// The same row build; instead of one argmax, W rounds of the block argmax over the LDS row, round r restricted to the entries that come
// strictly after round r-1's winner in the order (probability descending, id ascending).  That order is total, so the W winners are the
// W largest entries with the lowest id first on ties, whatever the scheduling; round 0 is K23's argmax comparison for comparison, so W = 1
// returns K23's id and value bit for bit.  Scratch on top of K23's: two words for the previous winner.
constexpr int PH_MAX_W = 8;
template <bool BAN, bool WIDE = false, bool RULES = false>
__global__ __launch_bounds__(PH_THREADS) void pointer_head_beam_kernel(const HeadArgs a, float* __restrict__ cand_p, int64_t* __restrict__ cand_id,
                                                                       const int W, const typename TailArgs<RULES>::type nb) {
  extern __shared__ __attribute__((aligned(16))) float ph_smem[];
  float* row = WIDE ? a.row_ws + (int64_t)blockIdx.x * a.row_stride : ph_smem;
  uint32_t* tk = reinterpret_cast<uint32_t*>(WIDE ? ph_smem : ph_smem + ((a.V + 3) & ~(int64_t)3));
  float* tv = reinterpret_cast<float*>(tk + PH_THREADS + 4);
  float* red = tv + PH_THREADS;
  __shared__ int64_t best_i[16];
  __shared__ float best_v[16];
  __shared__ int64_t win_i;
  __shared__ float win_v;
  const int64_t b = blockIdx.x, V = a.V;
  const int tid = threadIdx.x;
  pointer_head_build_row<WIDE>(a, row, tk, tv, red, b);
  if constexpr (BAN) ngram_ban_row(row, V, nb.hist + b * nb.Tmax, nb.t, nb.n, nb.eos, reinterpret_cast<int*>(tv));  // (K25 appends: a slot's history is its hypothesis)
  if constexpr (RULES) row_rules_row(row, V, nb.rl, b);
  float pv = INFINITY;  // the previous round's winner: round 0 admits every entry
  int64_t pi = -1;
  for (int r = 0; r < W; ++r) {
    float bv = -INFINITY;
    int64_t bi = V;
    for (int64_t i = tid; i < V; i += PH_THREADS) {
      const float x = row[i];
      if (r == 0 && a.dist) a.dist[b * V + i] = x;
      if (x > bv && (x < pv || (x == pv && i > pi))) {  // indices ascend within a thread: the first maximum is kept
        bv = x;
        bi = i;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int64_t oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if ((tid & 63) == 0) {
      best_v[tid >> 6] = bv;
      best_i[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < PH_THREADS / 64; ++w)
        if (best_v[w] > bv || (best_v[w] == bv && best_i[w] < bi)) {
          bv = best_v[w];
          bi = best_i[w];
        }
      cand_id[b * W + r] = bi < V ? bi : 0;
      cand_p[b * W + r] = bv;
      win_v = bv;
      win_i = bi;
    }
    __syncthreads();
    pv = win_v;
    pi = win_i;
  }
}

// ---- K28: the sampled step's head = K23's row with a filtered draw ------------------------------------------------------------------
// The same row build (or a ready distribution row, `dist_in`), then one token drawn from it: q = p^(1/temperature), the order of K24 (q
// descending, id ascending), top-k, top-p, and an inverse-CDF draw in id order with one uniform per row.  The row stays in LDS UNCHANGED: q
// is formed from p wherever it is needed (temperature 1: q = p; otherwise 2^((log2 p - log2 pmax) / temperature), i.e. q scaled so that its
// largest entry is 1 (v_log_f32 / v_exp_f32) -- the draw does not depend on the scale, and a low temperature cannot flush every entry to zero), so the returned
// probability is the row's own entry and no second V-sized buffer exists.
//
// Selection is a radix select over the bit pattern of q (q >= 0: the pattern orders like the value), 8 bits per level, with ONE 256-bin
// histogram of 64-bit integers in the dead key-staging area: entry counts for top-k, fixed-point masses (2^-40 of the largest entry's
// binade) for top-p.  Integer sums do not depend on the order of the LDS atomics, so the cuts are the same on every run.  The entries that
// equal the cut value are taken in id order up to a cut id found by a prefix count.  kept(i) <=> bits(q_i) > cut bits, or equal and i <= cut id.
//
// Every pass walks the row by wave: wave w owns the consecutive ids [w C, (w + 1) C) (conflict-free LDS reads).  The draw is a prefix sum
// in that order: a lane sums four consecutive ids of a 256-id tile (one 16-byte read), a shuffle scan over the lanes' totals, a running
// carry over the wave's tiles, the 16 wave totals summed in wave order -- a fixed summation tree of depth 3 + 7 + ceil(V / 4096) + 16, run
// twice with the same instructions (totals, then the search), so the last prefix IS the mass Z and u Z < Z always finds a token.  (One id
// per lane and tile made the two sweeps 19 us of dependent shuffle latency at V = 30 522; four make them a quarter of that.)  No float
// atomics anywhere.
constexpr int SM_WAVES = PH_THREADS / 64;
struct SampleArgs {
  const float* dist_in;     // [R, V] when HeadArgs.logits is null
  const float* uniforms;    // [R] or null: overrides the counter RNG
  const CaseStepState* state;
  uint64_t seed, offset;
  uint8_t* ended;           // [R] in / out
  int64_t* ids;             // [R] the emitted token
  float* prob;              // [R] row[drawn token]; 1 for a row that had ended
  int64_t eos, unk, pad;
  float temperature, top_p;
  int top_k, first, last;
};

struct SampleView {  // how a pass sees the row: the wave's id range, the q transform, the current cut
  const float* row;
  int w0, w1, lane;
  bool unit;
  float inv_tau, l2max, scale;
  uint32_t cbits;
  int cid;
  __device__ __forceinline__ float qf(float p) const {
    if (unit) return p;
    return p > 0.f ? __builtin_amdgcn_exp2f((__builtin_amdgcn_logf(p) - l2max) * inv_tau) : 0.f;
  }
  __device__ __forceinline__ float q(int i) const { return qf(row[i]); }
  // x[0 .. 3] = the own kept mass q of each of the four consecutive ids base + 4 lane + (0 .. 3), 0 for an id the cuts dropped or one at or
  // behind w1 (one 16-byte LDS read per lane; the row is padded to a multiple of four floats).  The caller forms the running sums.
  __device__ __forceinline__ void quad(int base, float (&x)[4]) const {
    const int i0 = base + 4 * lane;
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = 0.f;
    if (i0 < w1) {
      const float4 p4 = *reinterpret_cast<const float4*>(row + i0);
      const float p[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float qe = qf(p[e]);
        if (i0 + e < w1 && kept(__float_as_uint(qe), i0 + e)) x[e] = qe;
      }
    }
  }
  __device__ __forceinline__ bool kept(uint32_t qb, int i) const { return qb > cbits || (qb == cbits && i <= cid); }
};

template <bool MASS>
__device__ __forceinline__ void sample_hist_pass(const SampleView& v, unsigned long long* hist, uint32_t prefix, uint32_t pmask, int shift) {
  uint32_t cb = 0;  // a thread adds a run of entries that share a digit with one atomic
  unsigned long long acc = 0;
  for (int base = v.w0; base < v.w1; base += 256) {  // four consecutive ids per lane: one 16-byte LDS read (the row is padded to a multiple of 4)
    const int i0 = base + 4 * v.lane;
    if (i0 < v.w1) {
      const float4 p4 = *reinterpret_cast<const float4*>(v.row + i0);
      const float p[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float q = v.qf(p[e]);
        const uint32_t qb = __float_as_uint(q);
        if (i0 + e < v.w1 && (qb & pmask) == prefix && v.kept(qb, i0 + e)) {
          const uint32_t d = (qb >> shift) & 255u;
          if (d != cb) {
            if (acc) atomicAdd(&hist[cb], acc);
            cb = d;
            acc = 0;
          }
          acc += MASS ? (unsigned long long)(q * v.scale) : 1ull;
        }
      }
    }
  }
  if (acc) atomicAdd(&hist[cb], acc);
}

// wave 0: the digit d, highest first, with  above(d) < target <= above(d) + hist[d];  sel = {weight above the prefix, target, digit}
__device__ __forceinline__ void sample_select(const unsigned long long* hist, unsigned long long* sel, int lane, bool set_target, double top_p) {
  unsigned long long h[4], s = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h[e] = hist[255 - 4 * lane - e];
    s += h[e];
  }
  unsigned long long inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  const unsigned long long total = __shfl(inc, 63, 64);
  unsigned long long above = sel[0], target = sel[1];
  if (set_target) {  // top-p: the first level's histogram holds the whole mass
    target = (unsigned long long)(top_p * (double)total);
    if (target > total) target = total;
    if (target < 1) target = 1;  // at least one entry
  }
  unsigned long long run = above + inc - s;
  int found = -1;
  unsigned long long found_above = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (found < 0 && run < target && target <= run + h[e]) {
      found = 255 - 4 * lane - e;
      found_above = run;
    }
    run += h[e];
  }
  const bool any = __ballot(found >= 0) != 0ull;
  if (found >= 0) {
    sel[0] = found_above;
    sel[2] = (unsigned long long)found;
  }
  if (lane == 0) {
    sel[1] = target;
    if (!any) sel[2] = 0;  // an empty or all-zero row: the lowest digit, i.e. no cut
  }
}

// the cut value: the bit pattern v with  weight(q > v) < target <= weight(q >= v)  over the kept entries; leaves sel[0] = weight(q > v), sel[1] = target
template <bool MASS>
__device__ __forceinline__ uint32_t sample_radix(const SampleView& v, unsigned long long* hist, unsigned long long* sel, unsigned long long target,
                                                 double top_p) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid == 0) {
    sel[0] = 0;
    sel[1] = target;
  }
  uint32_t prefix = 0, pmask = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    sample_hist_pass<MASS>(v, hist, prefix, pmask, shift);
    __syncthreads();
    if (tid < 64) sample_select(hist, sel, tid, MASS && shift == 24, top_p);
    __syncthreads();
    prefix |= (uint32_t)sel[2] << shift;
    pmask |= 255u << shift;
  }
  return prefix;
}

// the id of the r-th kept entry (r >= 1, id order) whose q has the bit pattern `bits`; the last id of the row when there are fewer
__device__ __forceinline__ int sample_nth_tie(const SampleView& v, uint32_t bits, unsigned long long r, uint32_t* wcnt, int* tie_id, int V) {
  const int wave = threadIdx.x >> 6;
  uint32_t c = 0;
  for (int base = v.w0; base < v.w1; base += 64) {
    const int i = base + v.lane;
    bool flag = false;
    if (i < v.w1) {
      const uint32_t qb = __float_as_uint(v.q(i));
      flag = qb == bits && v.kept(qb, i);
    }
    c += (uint32_t)__popcll(__ballot(flag));
  }
  __syncthreads();
  if (v.lane == 0) wcnt[wave] = c;
  if (threadIdx.x == 0) *tie_id = V - 1;
  __syncthreads();
  unsigned long long off = 0;
  for (int w = 0; w < wave; ++w) off += wcnt[w];
  if (off < r && r <= off + c) {  // (wave-uniform) this wave holds it
    const uint32_t need = (uint32_t)(r - off);
    uint32_t run = 0;
    for (int base = v.w0; base < v.w1; base += 64) {
      const int i = base + v.lane;
      bool flag = false;
      if (i < v.w1) {
        const uint32_t qb = __float_as_uint(v.q(i));
        flag = qb == bits && v.kept(qb, i);
      }
      const unsigned long long m = __ballot(flag);
      const uint32_t n = (uint32_t)__popcll(m);
      if (run + n >= need) {
        const unsigned long long upto = m & ((2ull << v.lane) - 1ull);  // the flags of the lanes <= this one
        if (flag && (uint32_t)__popcll(upto) == need - run) *tie_id = i;
        break;
      }
      run += n;
    }
  }
  __syncthreads();
  return *tie_id;
}

__device__ __forceinline__ float sample_scan64(float x, int lane) {  // inclusive prefix sum over the wave, fixed tree
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(x, o, 64);
    if (lane >= o) x += t;
  }
  return x;
}

// WIDE: the row in a.row_ws, or -- a ready distribution with no workspace given (the host's choice: 16-byte aligned rows, no ban) -- `dist_in`
// itself, which no pass writes.  The quads read up to three floats behind V inside the row's stride; those entries are never kept.
template <bool BAN, bool WIDE = false, bool RULES = false>
__global__ __launch_bounds__(PH_THREADS) void pointer_head_sample_kernel(const HeadArgs a, const SampleArgs s, const typename TailArgs<RULES>::type nb) {
  extern __shared__ __attribute__((aligned(16))) float ph_smem[];
  const bool in_place = WIDE && !a.row_ws;  // (block-uniform)
  float* row = !WIDE ? ph_smem : in_place ? const_cast<float*>(s.dist_in) + (int64_t)blockIdx.x * a.V : a.row_ws + (int64_t)blockIdx.x * a.row_stride;
  uint32_t* tk = reinterpret_cast<uint32_t*>(WIDE ? ph_smem : ph_smem + ((a.V + 3) & ~(int64_t)3));
  float* tv = reinterpret_cast<float*>(tk + PH_THREADS + 4);
  float* red = tv + PH_THREADS;
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(tk);  // [256]: the key staging is dead behind the row build
  __shared__ unsigned long long sel[3];
  __shared__ uint32_t wcnt[SM_WAVES];
  __shared__ float wsum[SM_WAVES];
  __shared__ int wmin[SM_WAVES], wmax[SM_WAVES];
  __shared__ int tie_id;
  const int64_t b = blockIdx.x;
  const int V = (int)a.V, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (a.logits) {
    pointer_head_build_row<WIDE>(a, row, tk, tv, red, b);
  } else if (!in_place) {
    for (int i = tid; i < V; i += PH_THREADS) row[i] = s.dist_in[b * a.V + i];
    __syncthreads();
  }
  if constexpr (BAN) {
    if (!s.ended[b]) ngram_ban_row(row, a.V, nb.hist + b * nb.Tmax, nb.t, nb.n, s.eos, reinterpret_cast<int*>(tv));  // (block-uniform; tid 0 rewrites ended[b] behind the last barrier)
  }
  if constexpr (RULES) {
    if (!s.ended[b]) row_rules_row(row, a.V, nb.rl, b);  // (block-uniform, as above; an ended row keeps emitting PAD with probability 1)
  }
  float pmax = 0.f;
  for (int i = tid; i < V; i += PH_THREADS) {
    const float x = row[i];
    if (a.dist) a.dist[b * a.V + i] = x;
    pmax = fmaxf(pmax, x);
  }
  pmax = block_max(pmax, red);

  SampleView v;
  v.row = row;
  const int chunk = (((V + SM_WAVES - 1) / SM_WAVES) + 255) & ~255;  // whole 256-id tiles: 16-byte aligned quads
  v.w0 = min(V, wave * chunk);
  v.w1 = min(V, v.w0 + chunk);
  v.lane = lane;
  v.unit = s.temperature == 1.f;
  v.inv_tau = 1.f / s.temperature;
  v.l2max = v.unit ? 0.f : __builtin_amdgcn_logf(pmax);
  {
    int e = 0;
    frexpf(v.unit ? pmax : 1.f, &e);  // largest q < 2^e
    v.scale = ldexpf(1.f, min(40 - e, 120));
  }
  v.cbits = 0;  // no cut: every entry is kept
  v.cid = V - 1;

  if (s.top_k > 0 && s.top_k < V) {
    const uint32_t bits = sample_radix<false>(v, hist, sel, (unsigned long long)s.top_k, 0.0);
    const unsigned long long r = sel[1] - sel[0];  // entries still to take among those that equal the cut value
    const int id = sample_nth_tie(v, bits, r, wcnt, &tie_id, V);
    v.cbits = bits;
    v.cid = id;
  }
  if (s.top_p < 1.f) {
    const uint32_t bits = sample_radix<true>(v, hist, sel, 0ull, (double)s.top_p);
    const unsigned long long m = (unsigned long long)(__uint_as_float(bits) * v.scale), lack = sel[1] - sel[0];
    const unsigned long long r = m > 0 ? (lack + m - 1) / m : 1ull;
    const int id = sample_nth_tie(v, bits, r < 1 ? 1ull : r, wcnt, &tie_id, V);
    v.cbits = bits;
    v.cid = id;
  }

  // the draw: Z, then the smallest kept id whose prefix exceeds u Z.  A lane owns four consecutive ids of a 256-id tile: its running sums,
  // the shuffle scan of the lanes' totals, the carry over the wave's tiles, the wave's offset -- the same adds in both sweeps
  float carry = 0.f;
  for (int base = v.w0; base < v.w1; base += 256) {
    float x[4];
    v.quad(base, x);
    const float mine = ((x[0] + x[1]) + x[2]) + x[3];
    const float inc = sample_scan64(mine, lane);
    float before = __shfl_up(inc, 1, 64);
    if (lane == 0) before = 0.f;
    carry += __shfl(before + mine, 63, 64);
  }
  if (lane == 0) wsum[wave] = carry;
  __syncthreads();
  float off = 0.f, Z = 0.f;
  for (int w = 0; w < SM_WAVES; ++w) {
    if (w == wave) off = Z;
    Z += wsum[w];
  }
  const float u = s.uniforms ? s.uniforms[b] : rng_uniform24(s.seed, rng_base_of(s.state) + s.offset + (uint64_t)b);
  const float thr = u * Z;
  int mn = 0x7fffffff, mx = -1;
  carry = 0.f;
  for (int base = v.w0; base < v.w1; base += 256) {
    float x[4];
    v.quad(base, x);
    const float mine = ((x[0] + x[1]) + x[2]) + x[3];
    const float inc = sample_scan64(mine, lane);
    float before = __shfl_up(inc, 1, 64);
    if (lane == 0) before = 0.f;
    float run = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      run = e == 0 ? x[0] : run + x[e];  // (x0 + x1) + x2 ... : the association of `mine`
      const int i = base + 4 * lane + e;
      if (x[e] > 0.f) {  // an entry without mass is never drawn, whatever the rounding of its prefix
        mx = i;          // (ids ascend within a lane)
        if (off + (carry + (before + run)) > thr && i < mn) mn = i;
      }
    }
    carry += __shfl(before + mine, 63, 64);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, __shfl_xor(mn, o, 64));
    mx = max(mx, __shfl_xor(mx, o, 64));
  }
  if (lane == 0) {
    wmin[wave] = mn;
    wmax[wave] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 0; w < SM_WAVES; ++w) {
      mn = min(mn, wmin[w]);
      mx = max(mx, wmax[w]);
    }
    const int x = mn < V ? mn : (mx >= 0 ? mx : 0);  // rounding left none: the largest kept id with mass
    const bool e = s.ended[b] != 0, this_end = (int64_t)x == s.eos;
    int64_t emit;
    if (s.first) emit = this_end ? s.unk : (int64_t)x;
    else if (s.last) emit = e ? s.pad : s.eos;
    else emit = e ? s.pad : (int64_t)x;
    s.ids[b] = emit;
    if constexpr (BAN) {
      if (!RULES || nb.hist) nb.hist[b * nb.Tmax + nb.t] = (int32_t)emit;
    }
    s.prob[b] = e ? 1.f : row[x];
    s.ended[b] = (uint8_t)(e || this_end);
  }
}

// K32 on a distribution row in global memory (the unfused head): one wave per row
__global__ __launch_bounds__(64) void ngram_ban_kernel(float* __restrict__ dist, const uint8_t* __restrict__ ended, const int64_t V, const BanArgs nb) {
  __shared__ int stage[NB_MAX_T];
  const int64_t b = blockIdx.x;
  if (ended && ended[b]) return;
  ngram_ban_row(dist + b * V, V, nb.hist + b * nb.Tmax, nb.t, nb.n, nb.eos, stage);
}

// the decoding rules on a distribution row in global memory (the unfused head): one wave per row
__global__ __launch_bounds__(64) void row_rules_kernel(float* __restrict__ dist, const uint8_t* __restrict__ ended, const int64_t V, const RuleArgs rl) {
  const int64_t b = blockIdx.x;
  if (ended && ended[b]) return;
  row_rules_row(dist + b * V, V, rl, b);
}

// ---- K29: the head of a teacher-forced SCORING pass: one probability per row, no vocabulary row -------------------------------------------
// prob[r] = pm_0 softmax(logits[r])[y] + sum_k pm_{1+k} sum_{positions s of memory k whose source id is y} copy_k[r, s],  y = targets[r].
// One workgroup of 256 threads per row.  The logits row is read ONCE with a per-thread online (max, sum): 16-byte loads over the aligned
// body, scalar peels before and behind it (V = 30 522 leaves rows 8-byte aligned, an odd V 4-byte aligned).  The stream is read
// NON-TEMPORAL for K22's reason: every byte is used once and the buffer is rewritten by the next row chunk's vocabulary GEMM, so it should
// not displace that GEMM's weights (the reusable data) from the caches.  -DCASE_STREAM_DEFAULT_POLICY: default policy (A/B).
// The (max, sum) pairs meet in a fixed xor tree per wave and in wave order across the four waves; logit[y] is one direct load.  Pointer
// mass: wave 0 finds the lower bound of y << 15 in the row's sorted keys (every lane the same search), lane l takes entries lo + l,
// lo + l + 64, ... of the run of equal tokens, and the lanes meet in the same fixed tree.  No atomics, no LDS beyond 8 floats: V is
// limited by the key format alone, and two launches give the same bits.
constexpr int PS_THREADS = 256;
struct ScoreArgs {
  const float* logits;      // [R, V]
  const float* mix_logits;  // [R, 1 + nmem]
  const uint32_t* keys;     // [R / rows_per_source, S] sorted (token << 15 | position), 0xFFFFFFFF = no token
  const float* copy[PH_MAX_MEM];  // copy_k [R, len_k]
  int64_t len[PH_MAX_MEM];
  const int64_t* targets;   // [R]
  float* prob;              // [R]
  float* ptr;               // [R] or null: the pointer part of prob
  float* stats;             // [R, 2] or null: the row's final (max, sum) of the online softmax (case_pointer_head_score_stats)
  float* nll;               // [R] the loss form only: -log(prob + 1e-8), 0 for a PAD row
  int64_t V, S, rows_per_source, pad;
  int64_t ld;               // the loss form only: floats between two logits rows (>= V; K29 itself reads rows V apart)
  int nmem;
};

typedef float ps_f32x4 __attribute__((ext_vector_type(4)));
typedef float ps_f32x4u __attribute__((ext_vector_type(4), aligned(4)));  // a 16-byte access on a 4-byte boundary
#ifndef CASE_STREAM_DEFAULT_POLICY
#define PS_LOAD1(P) __builtin_nontemporal_load(P)
#define PS_LOAD4(P) __builtin_nontemporal_load(reinterpret_cast<const ps_f32x4*>(P))
#else
#define PS_LOAD1(P) (*(P))
#define PS_LOAD4(P) (*reinterpret_cast<const ps_f32x4*>(P))
#endif
// The loss form (the training head) reads its logits with the DEFAULT policy: K41's loss form reads the same 157 MB again a few launches
// later, and they fit the Infinity Cache.  -DCASE_LOSS_STREAM_NT: non-temporal as K29 (A/B; DESIGN 9.7 has the pair of timings).
#ifdef CASE_LOSS_STREAM_NT
#define PL_LOAD1(P) __builtin_nontemporal_load(P)
#define PL_LOAD4(P) __builtin_nontemporal_load(reinterpret_cast<const ps_f32x4u*>(P))
#else
#define PL_LOAD1(P) (*(P))
#define PL_LOAD4(P) (*reinterpret_cast<const ps_f32x4u*>(P))
#endif

// (m, s) <- (m, s) (+) (om, os) with s = sum exp(x - m); an empty side is (-inf, 0)
__device__ __forceinline__ void ps_merge(float& m, float& s, const float om, const float os) {
  const float M = fmaxf(m, om);
  const float ref = M == -INFINITY ? 0.f : M;  // both sides empty: exp(-inf - 0) = 0, never inf - inf
  s = s * __expf(m - ref) + os * __expf(om - ref);
  m = M;
}

// LOSS: the head of the TRAINING step (case_pointer_head_loss).  The same body with three differences.  Row r starts at logits + r * ld
// (ld >= V: the vocabulary GEMM writes rows padded to its 256-wide tiles; columns [V, ld) are never read).  nll[r] = -log(prob + 1e-8),
// 0 for a PAD row, is written beside prob.  And the row is split over the threads as K29 splits row r of a CONTIGUOUS [R, V] buffer on a
// 16-byte boundary -- (-r V) mod 4 peeled floats, then groups of four -- whatever ld is, so prob / copy / stats carry K29's bits for the
// same logits; where that split is out of phase with the padded row (V = 30 522: every odd row, by 8 bytes) the 16-byte loads are
// unaligned, which costs one more cache line per wave and load.
template <bool LOSS>
__global__ __launch_bounds__(PS_THREADS) void pointer_head_score_kernel(const ScoreArgs a) {
  __shared__ float red_m[PS_THREADS / 64], red_s[PS_THREADS / 64];
  const int64_t r = blockIdx.x, V = a.V;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t y = a.targets[r];
  const bool is_pad = a.pad >= 0 && y == a.pad;
  if (is_pad || y < 0 || y >= V) {  // (uniform over the workgroup) PAD: not scored, p = 1; an id outside the vocabulary: p = 0
    if (tid == 0) {
      a.prob[r] = is_pad ? 1.f : 0.f;
      if (a.ptr) a.ptr[r] = 0.f;
      if (a.stats) a.stats[2 * r] = a.stats[2 * r + 1] = 0.f;
      if constexpr (LOSS) {
        float p0 = 0.f;
        asm volatile("" : "+v"(p0));  // (opaque: logf of a constant would be folded with the host's libm, whose last bit can differ)
        a.nll[r] = is_pad ? 0.f : -logf(p0 + 1e-8f);
      }
    }
    return;
  }
  const float* lg = a.logits + r * (LOSS ? a.ld : V);
  int64_t head;
  if constexpr (LOSS) head = (-(r * V)) & 3;
  else head = (int64_t)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(lg) & 15u)) & 15u) >> 2);  // floats in front of the first 16-byte boundary
  if (head > V) head = V;
  const int64_t n4 = (V - head) >> 2, tail = head + 4 * n4;
  float m = -INFINITY, s = 0.f;
  if (tid < head) ps_merge(m, s, LOSS ? PL_LOAD1(lg + tid) : PS_LOAD1(lg + tid), 1.f);
  const float* body = lg + head;
#pragma unroll 2
  for (int64_t i = tid; i < n4; i += PS_THREADS) {
    ps_f32x4 x;
    if constexpr (LOSS) x = PL_LOAD4(body + 4 * i);
    else x = PS_LOAD4(body + 4 * i);
    const float m4 = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
    if (m4 > m) {
      s *= __expf(m - m4);  // (m = -inf: s = 0 stays 0)
      m = m4;
    }
    s += (__expf(x[0] - m) + __expf(x[1] - m)) + (__expf(x[2] - m) + __expf(x[3] - m));
  }
  if (tail + tid < V) ps_merge(m, s, LOSS ? PL_LOAD1(lg + tail + tid) : PS_LOAD1(lg + tail + tid), 1.f);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
    ps_merge(m, s, om, os);
  }
  if (lane == 0) {
    red_m[tid >> 6] = m;
    red_s[tid >> 6] = s;
  }
  __syncthreads();
  if (tid >= 64) return;  // wave 0 finishes the row
  m = red_m[0];
  s = red_s[0];
#pragma unroll
  for (int w = 1; w < PS_THREADS / 64; ++w) ps_merge(m, s, red_m[w], red_s[w]);
  const float gen_y = __expf(lg[y] - m) / s;
  // the mixing probabilities, as in pointer_head_build_row
  float pm[1 + PH_MAX_MEM];
  {
    float mm = -INFINITY, ss = 0.f;
#pragma unroll
    for (int k = 0; k <= PH_MAX_MEM; ++k) pm[k] = k <= a.nmem ? a.mix_logits[r * (a.nmem + 1) + k] : -INFINITY;
#pragma unroll
    for (int k = 0; k <= PH_MAX_MEM; ++k) mm = fmaxf(mm, pm[k]);
#pragma unroll
    for (int k = 0; k <= PH_MAX_MEM; ++k) {
      pm[k] = __expf(pm[k] - mm);
      ss += pm[k];
    }
#pragma unroll
    for (int k = 0; k <= PH_MAX_MEM; ++k) pm[k] /= ss;
  }
  const uint32_t* keys = a.keys + (r / a.rows_per_source) * a.S;
  const uint32_t want = (uint32_t)y << 15;  // y < V <= 131071: fits
  int64_t lo = 0, hi = a.S;
  while (lo < hi) {  // the first entry with key >= y << 15 (uniform over the wave)
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  float acc = 0.f;
  for (int64_t i = lo + lane; i < a.S; i += 64) {
    const uint32_t key = keys[i];
    if (key == 0xFFFFFFFFu || (key >> 15) != (uint32_t)y) break;  // the run of y has ended (keys ascend)
    int64_t pos = key & 0x7FFFu;
    bool done = false;
#pragma unroll
    for (int k = 0; k < PH_MAX_MEM; ++k) {
      if (k < a.nmem && !done) {
        if (pos < a.len[k]) {
          acc += pm[k + 1] * a.copy[k][r * a.len[k] + pos];
          done = true;
        }
        pos -= a.len[k];
      }
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    const float p = pm[0] * gen_y + acc;
    a.prob[r] = p;
    if (a.ptr) a.ptr[r] = acc;
    if (a.stats) {
      a.stats[2 * r] = m;
      a.stats[2 * r + 1] = s;
    }
    if constexpr (LOSS) a.nll[r] = -logf(p + 1e-8f);
  }
}

// ---- K41: the backward of K29 ---------------------------------------------------------------------------------------------------------------
// d prob[r] / d (logits, mix_logits, copy_k) times g[r], from the forward's saved (max, sum) and prob.  One workgroup of 256 threads per
// row.  A short pass over the S source positions reads the item's UNSORTED ids: position s of memory k holds y or it does not, so
// d_copy_k[r, s] is one compare (no search, no read-after-write on the row) and c_k, the copy mass of y in memory k, is a per-thread sum
// that meets in the fixed xor tree per wave and in wave order across the four waves.  Then one pass over V: gen_v = exp(l_v - m) / s is
// K29's own expression for gen_y, read with K29's head / body / tail peel (non-temporal: the logits are used once here too) and stored
// 16 bytes wide with the DEFAULT policy -- the two vocabulary GEMMs of the Linear backward read d_logits next.  Where the gradient row
// does not share the logits row's 16-byte phase (a caller's offset view) the pass falls back to 4-byte accesses.  Every output element
// is written, a row that is not scored writes zeros; no atomics: two launches give the same bits.
struct ScoreBwdArgs {
  const float* logits;      // [R, V]
  const float* mix_logits;  // [R, 1 + nmem]
  const int64_t* ids;       // [R / rows_per_source, S] the unsorted source ids
  const float* copy[PH_MAX_MEM];  // copy_k [R, len_k]
  int64_t len[PH_MAX_MEM];
  const int64_t* targets;   // [R]
  const float* stats;       // [R, 2] the forward's (max, sum)
  const float* prob;        // [R] the forward's output
  const float* g;           // [R] dL / dprob; the loss form: dL / dnll
  void* d_logits;           // [R, V] f32; the loss form: [R, ld] f32 or bf16
  int64_t ld;               // the loss form only: elements between two rows of logits and of d_logits (>= V, a multiple of 8)
  float* d_mix;             // [R, 1 + nmem]
  float* d_copy[PH_MAX_MEM];  // [R, len_k]
  int64_t V, S, rows_per_source, pad;
  int nmem;
};

// the memory that holds source position s and the position inside it
__device__ __forceinline__ int ps_locate(const ScoreBwdArgs& a, int64_t& pos) {
  int k = 0;
#pragma unroll
  for (int j = 0; j < PH_MAX_MEM - 1; ++j) {
    if (k == j && j + 1 < a.nmem && pos >= a.len[j]) {
      pos -= a.len[j];
      k = j + 1;
    }
  }
  return k;
}

// LOSS: the backward of the TRAINING head (case_pointer_head_loss_bwd).  The upstream gradient is that of nll = -log(prob + 1e-8), so
// the kernel forms dL / dprob = -g / (prob + 1e-8) itself; logits and d_logits rows lie ld apart (a multiple of 8 elements on 16-byte
// bases, so every row is 16-byte aligned and nothing is peeled in front); d_logits is stored in the operand dtype of the two GEMMs that
// read it next -- OutT = bf16: the f32 value rounded once to nearest even, 8 elements per 16-byte store -- and the pad columns [V, ld)
// are WRITTEN as zeros: the dX GEMM reduces over them.  The group of 8 that holds column V is computed element by element and stored
// whole.  The logits are read with the default policy, as the forward reads them (measured equal to non-temporal: -DCASE_LOSS_STREAM_NT).
template <typename OutT>
__device__ __forceinline__ void ps_store8(OutT* p, const float (&d)[8]);
template <> __device__ __forceinline__ void ps_store8<float>(float* p, const float (&d)[8]) {
  *reinterpret_cast<ps_f32x4*>(p) = ps_f32x4{d[0], d[1], d[2], d[3]};
  *reinterpret_cast<ps_f32x4*>(p + 4) = ps_f32x4{d[4], d[5], d[6], d[7]};
}
template <> __device__ __forceinline__ void ps_store8<bf16_t>(bf16_t* p, const float (&d)[8]) { Vec16<bf16_t>::store(p, d); }

template <typename OutT, bool LOSS>
__global__ __launch_bounds__(PS_THREADS) void pointer_head_score_bwd_kernel(const ScoreBwdArgs a) {
  __shared__ float red_c[PS_THREADS / 64][PH_MAX_MEM];
  const int64_t r = blockIdx.x, V = a.V, S = a.S;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t y = a.targets[r];
  const bool is_pad = a.pad >= 0 && y == a.pad;
  const bool scored = !(is_pad || y < 0 || y >= V);  // (uniform over the workgroup)
  const float* lg = a.logits + r * (LOSS ? a.ld : V);
  OutT* dl = reinterpret_cast<OutT*>(a.d_logits) + r * (LOSS ? a.ld : V);
  const float gr = !scored ? 0.f : LOSS ? -a.g[r] / (a.prob[r] + 1e-8f) : a.g[r];
  // the mixing probabilities, as in K29
  float pm[1 + PH_MAX_MEM];
  {
    float mm = -INFINITY, ss = 0.f;
#pragma unroll
    for (int k = 0; k <= PH_MAX_MEM; ++k) pm[k] = k <= a.nmem ? a.mix_logits[r * (a.nmem + 1) + k] : -INFINITY;
#pragma unroll
    for (int k = 0; k <= PH_MAX_MEM; ++k) mm = fmaxf(mm, pm[k]);
#pragma unroll
    for (int k = 0; k <= PH_MAX_MEM; ++k) {
      pm[k] = __expf(pm[k] - mm);
      ss += pm[k];
    }
#pragma unroll
    for (int k = 0; k <= PH_MAX_MEM; ++k) pm[k] /= ss;
  }
  // the pass over S: d_copy_k and the per-memory copy mass of y
  float c[PH_MAX_MEM];
#pragma unroll
  for (int k = 0; k < PH_MAX_MEM; ++k) c[k] = 0.f;
  const int64_t* ids = a.ids + (r / a.rows_per_source) * S;
  for (int64_t s0 = tid; s0 < S; s0 += PS_THREADS) {
    int64_t pos = s0;
    const int k = ps_locate(a, pos);
    const bool hit = scored && ids[s0] == y;
#pragma unroll
    for (int j = 0; j < PH_MAX_MEM; ++j) {
      if (j == k) {
        const int64_t at = r * a.len[j] + pos;
        a.d_copy[j][at] = hit ? gr * pm[j + 1] : 0.f;
        if (hit) c[j] += a.copy[j][at];
      }
    }
  }
  if (!scored) {  // zeros everywhere (d_copy is done)
    if (tid <= a.nmem) a.d_mix[r * (a.nmem + 1) + tid] = 0.f;
    if constexpr (LOSS) {
      const float zero[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int64_t v0 = 8 * (int64_t)tid; v0 < a.ld; v0 += 8 * PS_THREADS) ps_store8<OutT>(dl + v0, zero);
    } else {
      for (int64_t v = tid; v < V; v += PS_THREADS) dl[v] = 0.f;
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < PH_MAX_MEM; ++k) {
    c[k] = wave_sum(c[k]);
    if (lane == 0) red_c[tid >> 6][k] = c[k];
  }
  __syncthreads();
  const float m = a.stats[2 * r], s = a.stats[2 * r + 1];
  const float gen_y = __expf(lg[y] - m) / s;
  if (tid == 0) {
    const float p = a.prob[r];
    a.d_mix[r * (a.nmem + 1)] = (gr * pm[0]) * (gen_y - p);
#pragma unroll
    for (int k = 0; k < PH_MAX_MEM; ++k) {
      if (k < a.nmem) {
        float ck = red_c[0][k];
#pragma unroll
        for (int w = 1; w < PS_THREADS / 64; ++w) ck += red_c[w][k];
        a.d_mix[r * (a.nmem + 1) + 1 + k] = (gr * pm[1 + k]) * (ck - p);
      }
    }
  }
  // the pass over V
  const float coef = gr * pm[0] * gen_y;
  if constexpr (LOSS) {
#pragma unroll 2
    for (int64_t v0 = 8 * (int64_t)tid; v0 < a.ld; v0 += 8 * PS_THREADS) {
      float d[8];
      if (v0 + 8 <= V) {
#ifdef CASE_LOSS_STREAM_NT
        const ps_f32x4 x0 = PS_LOAD4(lg + v0), x1 = PS_LOAD4(lg + v0 + 4);
#else
        const ps_f32x4 x0 = *reinterpret_cast<const ps_f32x4*>(lg + v0), x1 = *reinterpret_cast<const ps_f32x4*>(lg + v0 + 4);
#endif
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          d[e] = coef * ((v0 + e == y ? 1.f : 0.f) - __expf(x0[e] - m) / s);
          d[4 + e] = coef * ((v0 + 4 + e == y ? 1.f : 0.f) - __expf(x1[e] - m) / s);
        }
      } else {  // the group that holds column V, and the pad behind it: nothing at or behind column V is read
#pragma unroll
        for (int e = 0; e < 8; ++e) d[e] = v0 + e < V ? coef * ((v0 + e == y ? 1.f : 0.f) - __expf(lg[v0 + e] - m) / s) : 0.f;
      }
      ps_store8<OutT>(dl + v0, d);
    }
  } else {  // K41 itself: f32 rows V apart at any phase
    if (((reinterpret_cast<uintptr_t>(lg) ^ reinterpret_cast<uintptr_t>(dl)) & 15u) != 0) {  // rows out of phase: 4-byte accesses
      for (int64_t v = tid; v < V; v += PS_THREADS) dl[v] = coef * ((v == y ? 1.f : 0.f) - __expf(PS_LOAD1(lg + v) - m) / s);
      return;
    }
    int64_t head = (int64_t)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(lg) & 15u)) & 15u) >> 2);  // floats in front of the first 16-byte boundary
    if (head > V) head = V;
    const int64_t n4 = (V - head) >> 2, tail = head + 4 * n4;
    if (tid < head) dl[tid] = coef * ((tid == y ? 1.f : 0.f) - __expf(PS_LOAD1(lg + tid) - m) / s);
    const float* body = lg + head;
#pragma unroll 2
    for (int64_t i = tid; i < n4; i += PS_THREADS) {
      const ps_f32x4 x = PS_LOAD4(body + 4 * i);
      const int64_t v0 = head + 4 * i;
      ps_f32x4 d;
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = coef * ((v0 + e == y ? 1.f : 0.f) - __expf(x[e] - m) / s);
      *reinterpret_cast<ps_f32x4*>(dl + v0) = d;
    }
    if (tail + tid < V) dl[tail + tid] = coef * ((tail + tid == y ? 1.f : 0.f) - __expf(PS_LOAD1(lg + tail + tid) - m) / s);
  }
}

// ---- K11 ---------------------------------------------------------------------------------------
__global__ void copy_scatter_fwd_kernel(const int64_t* __restrict__ src, const float* __restrict__ w,
                                        float* __restrict__ dist, int64_t B, int64_t Tn, int64_t S, int64_t V) {
  const int64_t n = B * Tn * S;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t sidx = i % S, bt = i / S, b = bt / Tn;
    const int64_t tok = src[b * S + sidx];
    const float val = w[i];
    if (tok >= 0 && tok < V && val != 0.f) atomicAdd(dist + bt * V + tok, val);
  }
}

__global__ void copy_scatter_bwd_kernel(const int64_t* __restrict__ src, const float* __restrict__ d_dist,
                                        float* __restrict__ d_w, int64_t B, int64_t Tn, int64_t S, int64_t V) {
  const int64_t n = B * Tn * S;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t sidx = i % S, bt = i / S, b = bt / Tn;
    const int64_t tok = src[b * S + sidx];
    d_w[i] = (tok >= 0 && tok < V) ? d_dist[bt * V + tok] : 0.f;
  }
}

// ---- K11, sorted form (the source map sorted on the device once per batch) -----------
// keys[b, i] = (token << 15 | position), ascending; out-of-vocabulary ids become 0xFFFFFFFF and sort behind every valid key.
// One workgroup per batch row, bitonic network over the next power of two in LDS (S <= 32768: 128 KiB).
__global__ __launch_bounds__(1024) void source_sort_kernel(const int64_t* __restrict__ src, uint32_t* __restrict__ keys, int64_t S,
                                                            int64_t V, int n) {
  extern __shared__ uint32_t sk[];
  const int64_t b = blockIdx.x;
  for (int i = threadIdx.x; i < n; i += 1024) {
    uint32_t k = 0xFFFFFFFFu;
    if (i < S) {
      const int64_t tok = src[b * S + i];
      if (tok >= 0 && tok < V) k = ((uint32_t)tok << 15) | (uint32_t)i;
    }
    sk[i] = k;
  }
  __syncthreads();
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += 1024) {
        const int p = i ^ j;
        if (p > i) {
          const uint32_t x = sk[i], y = sk[p];
          if ((x > y) == ((i & k) == 0)) {
            sk[i] = y;
            sk[p] = x;
          }
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < S; i += 1024) keys[b * S + i] = sk[i];
}

// dist[b, t, token] += sum of w[b, t, position] over each run of equal tokens in the sorted keys: one workgroup per (b, t) row
// walks the keys in chunks of 256; the last lane of a run sums it (fixed order) and adds it to the row with a plain
// read-modify-write -- a token's run in a later chunk is added by a later iteration of the same workgroup, so there are no
// atomics and the result does not depend on scheduling.
__global__ __launch_bounds__(256) void copy_scatter_sorted_kernel(const uint32_t* __restrict__ keys, const float* __restrict__ w,
                                                                  float* __restrict__ dist, int64_t Tn, int64_t S, int64_t V) {
  __shared__ uint32_t tk[257];
  __shared__ float tv[256];
  const int64_t bt = blockIdx.x, b = bt / Tn;
  const uint32_t* k = keys + b * S;
  const float* wr = w + bt * S;
  float* d = dist + bt * V;
  for (int64_t base = 0; base < S; base += 256) {
    const int64_t i = base + threadIdx.x;
    const uint32_t key = i < S ? k[i] : 0xFFFFFFFFu;
    const bool valid = key != 0xFFFFFFFFu;
    tk[threadIdx.x] = valid ? (key >> 15) : 0xFFFFFFFFu;
    tv[threadIdx.x] = valid ? wr[key & 0x7FFFu] : 0.f;
    if (threadIdx.x == 0) tk[256] = 0xFFFFFFFEu;  // differs from every token and from the invalid marker: lane 255 always ends a run
    __syncthreads();
    const uint32_t tok = tk[threadIdx.x];
    if (valid && tok != tk[threadIdx.x + 1]) {
      int j = threadIdx.x;
      while (j > 0 && tk[j - 1] == tok) --j;
      float sum = 0.f;
      for (; j <= (int)threadIdx.x; ++j) sum += tv[j];
      if (sum != 0.f) d[tok] += sum;
    }
    __threadfence_block();
    __syncthreads();
  }
}

// ---- K12 / K13 ---------------------------------------------------------------------------------
__global__ void nll_fwd_kernel(const float* __restrict__ dist, const int64_t* __restrict__ target,
                               float* __restrict__ per_row, int64_t rows, int64_t V) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t y = target[r];
    per_row[r] = (y > 0 && y < V) ? -logf(dist[r * V + y] + 1e-8f) : 0.f;
  }
}

__global__ void nll_bwd_kernel(const float* __restrict__ dist, const int64_t* __restrict__ target,
                               const float* __restrict__ g_row, float* __restrict__ d_dist, int64_t rows, int64_t V) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t y = target[r];
    if (y > 0 && y < V) d_dist[r * V + y] = -g_row[r] / (dist[r * V + y] + 1e-8f);
  }
}

__global__ __launch_bounds__(256) void row_argmax_kernel(const float* __restrict__ x, int64_t* __restrict__ idx,
                                                         float* __restrict__ val, int64_t rows, int64_t cols, int64_t ld) {
  __shared__ float sv[4];
  __shared__ int64_t si[4];
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    float best = -INFINITY;
    int64_t bi = cols;  // sentinel larger than any index so the lowest index wins ties
    for (int64_t c = threadIdx.x; c < cols; c += 256) {
      const float vv = x[r * ld + c];
      if (vv > best || (vv == best && c < bi)) {
        best = vv;
        bi = c;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int64_t oi = __shfl_xor(bi, o, 64);
      if (ob > best || (ob == best && oi < bi)) {
        best = ob;
        bi = oi;
      }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
      sv[threadIdx.x >> 6] = best;
      si[threadIdx.x >> 6] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < 4; ++w)
        if (sv[w] > best || (sv[w] == best && si[w] < bi)) {
          best = sv[w];
          bi = si[w];
        }
      idx[r] = bi < cols ? bi : 0;
      if (val) val[r] = best;
    }
  }
}

}  // namespace

extern "C" int case_additive_scores_fwd(const float* wq, const void* uh, const float* v, float* s, int64_t B, int64_t T,
                                        int64_t S, int64_t H, int32_t dtype, case_stream_t stream) {
  CASE_REQUIRE(wq && uh && v && s && B > 0 && T > 0 && S > 0 && H > 0 && B < 65536, "case_additive_scores_fwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const int ev = dtype == CASE_F32 ? 4 : 8;
  if (T <= 2 && H % ev == 0 && H <= 2 * 64 * ev && (uintptr_t)uh % 16 == 0) {  // decode steps (T = 1)
    const dim3 g((unsigned)((S + 15) / 16 < 64 ? (S + 15) / 16 : 64), (unsigned)B);
    const bool one = H <= 64 * ev;
    // T = 1 (every greedy step) gets its own instantiation: the kernel is bound by the tanh issue rate, and the two-row form
    // evaluates the absent second row as well
#define ROWWISE(TY, FAST, TT, NCH) hipLaunchKernelGGL((additive_fwd_rowwise_kernel<TY, FAST, TT, NCH>), g, dim3(256), 0, st, wq, (const TY*)uh, v, s, T, S, H)
    if (dtype == CASE_F32) {
      if (T == 1) { if (one) ROWWISE(float, false, 1, 1); else ROWWISE(float, false, 1, 2); }
      else { if (one) ROWWISE(float, false, 2, 1); else ROWWISE(float, false, 2, 2); }
    } else {
      if (T == 1) { if (one) ROWWISE(bf16_t, true, 1, 1); else ROWWISE(bf16_t, true, 1, 2); }
      else { if (one) ROWWISE(bf16_t, true, 2, 1); else ROWWISE(bf16_t, true, 2, 2); }
    }
#undef ROWWISE
    return case_check_launch("case_additive_scores_fwd");
  }
  // a short memory (the 64-token query: one j block per item) leaves most CUs idle: spread the target chunks over workgroups too
  const int64_t jb = (S + AJ - 1) / AJ, tchunks = (T + 4 * ATW - 1) / (4 * ATW);
  const dim3 grid((unsigned)jb, (unsigned)B, (unsigned)(jb * B < 512 ? tchunks : 1));
  if (dtype == CASE_F32)
    hipLaunchKernelGGL((additive_fwd_kernel<float, false>), grid, dim3(256), 0, st, wq, (const float*)uh, v, s, T, S, H);
  else
    hipLaunchKernelGGL((additive_fwd_kernel<bf16_t, true>), grid, dim3(256), 0, st, wq, (const bf16_t*)uh, v, s, T, S, H);
  return case_check_launch("case_additive_scores_fwd");
}

extern "C" int case_additive_scores_bwd(const float* ds, const float* wq, const void* uh, const float* v, float* d_wq,
                                        float* d_uh, float* d_v, int64_t B, int64_t T, int64_t S, int64_t H, int32_t dtype,
                                        case_stream_t stream) {
  CASE_REQUIRE(ds && wq && uh && v && d_wq && d_uh && d_v && B > 0 && T > 0 && S > 0 && H > 0 && B < 65536,
               "case_additive_scores_bwd: bad argument");
  const unsigned hb = (unsigned)((H + 255) / 256);
  const int tblocks = (int)((T + CT - 1) / CT);
  // split the source positions of sweep 2 until ~2048 workgroups exist (whole CJC chunks per workgroup)
  const int64_t base_wgs = (int64_t)tblocks * hb * B, j_chunks = (S + CJC - 1) / CJC;
  int64_t sch = base_wgs >= 2048 ? 1 : (2048 + base_wgs - 1) / base_wgs;
  if (sch > j_chunks) sch = j_chunks;
  const int64_t j_per = ((j_chunks + sch - 1) / sch) * CJC;
  sch = (S + j_per - 1) / j_per;
  const dim3 g1((unsigned)((S + BJ - 1) / BJ), hb, (unsigned)B), g2((unsigned)(tblocks * sch), hb, (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (sch > 1 && hipMemsetAsync(d_wq, 0, (size_t)(B * T * H) * sizeof(float), st) != hipSuccess)
    return case_set_error(CASE_E_LAUNCH, "case_additive_scores_bwd: hipMemsetAsync failed");
  if (dtype == CASE_F32) {
    hipLaunchKernelGGL((additive_bwd_uh_kernel<float, false>), g1, dim3(256), 0, st, ds, wq, (const float*)uh, v, d_uh, d_v, T, S, H);
    hipLaunchKernelGGL((additive_bwd_wq_kernel<float, false>), g2, dim3(256), 0, st, ds, wq, (const float*)uh, v, d_wq, T, S, H, tblocks, j_per);
  } else {
    hipLaunchKernelGGL((additive_bwd_uh_kernel<bf16_t, true>), g1, dim3(256), 0, st, ds, wq, (const bf16_t*)uh, v, d_uh, d_v, T, S, H);
    hipLaunchKernelGGL((additive_bwd_wq_kernel<bf16_t, true>), g2, dim3(256), 0, st, ds, wq, (const bf16_t*)uh, v, d_wq, T, S, H, tblocks, j_per);
  }
  return case_check_launch("case_additive_scores_bwd");
}

extern "C" int case_additive_key_exp(const float* uh, void* eu, int64_t n, case_stream_t stream) {
  CASE_REQUIRE(uh && eu && n > 0 && n % 8 == 0 && (uintptr_t)uh % 16 == 0 && (uintptr_t)eu % 16 == 0, "case_additive_key_exp: bad argument");
  hipLaunchKernelGGL(additive_key_exp_kernel, dim3(grid_for(n / 8, 256, 1, 256 * 32)), dim3(256), 0, (hipStream_t)stream, uh,
                     reinterpret_cast<bf16_t*>(eu), n / 8);
  return case_check_launch("case_additive_key_exp");
}

extern "C" int case_pointer_attend_decode(const float* wq, const float* wq_add, const void* eu, const float* v, const void* value, const uint8_t* col_valid,
                                          const uint8_t* row_valid, const float* prior, void* ctx, float* p, float* copy, int64_t B, int64_t S,
                                          int64_t H, case_stream_t stream) {
  CASE_REQUIRE(wq && eu && v && value && ctx && p && B > 0 && S > 0 && B < (1ll << 31) && (copy != nullptr) == (prior != nullptr),
               "case_pointer_attend_decode: bad argument");
  if (H != PA_H || S > 28000)
    return case_set_error(CASE_E_UNSUPPORTED, "case_pointer_attend_decode: built for H = %d and S <= 28000 (run case_additive_scores_fwd + "
                                              "case_softmax_fwd + case_gemm)", PA_H);
  for (const void* q : {(const void*)wq, (const void*)wq_add, eu, (const void*)v, value})
    CASE_REQUIRE((reinterpret_cast<uintptr_t>(q) & 15) == 0, "case_pointer_attend_decode: tensors must be 16-byte aligned");
  const size_t lds = (size_t)(((S + 3) & ~(int64_t)3) + PA_WAVES * PA_H) * sizeof(float);
  static bool attr = false;
  if (!attr) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&pointer_attend_decode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
        hipSuccess)
      return case_set_error(CASE_E_LAUNCH, "case_pointer_attend_decode: cannot reserve LDS");
    attr = true;
  }
  hipLaunchKernelGGL(pointer_attend_decode_kernel, dim3((unsigned)B), dim3(64 * PA_WAVES), lds, (hipStream_t)stream, wq, wq_add,
                     reinterpret_cast<const bf16_t*>(eu), v, reinterpret_cast<const bf16_t*>(value), col_valid, row_valid, prior,
                     reinterpret_cast<bf16_t*>(ctx), p, copy, S);
  return case_check_launch("case_pointer_attend_decode");
}

// the operands K23 / K24 / K28 (HeadArgs) and K29 (ScoreArgs) share: logits, mixing logits, sorted keys and the copy weights of every memory,
// whose lengths must add up to the source map's
template <typename Args>
static int pointer_head_fill(Args& a, const char* who, const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                             const int64_t* lens, int32_t nmem, int64_t R, int64_t V, int64_t S, int64_t max_v, const char* instead) {
  CASE_REQUIRE(logits && mix_logits && keys && copies && lens && R > 0 && V > 0 && S > 0 && nmem >= 1 && R < (1ll << 31), "%s: bad argument", who);
  if (nmem > PH_MAX_MEM || V > max_v || S > 32768)
    return case_set_error(CASE_E_UNSUPPORTED, "%s: built for <= %d memories, V <= %lld, S <= 32768%s", who, PH_MAX_MEM, (long long)max_v, instead);
  a.logits = logits;
  a.mix_logits = mix_logits;
  a.keys = keys;
  int64_t total = 0;
  for (int m = 0; m < PH_MAX_MEM; ++m) {
    a.copy[m] = m < nmem ? copies[m] : nullptr;
    a.len[m] = m < nmem ? lens[m] : 0;
    total += a.len[m];
    CASE_REQUIRE(m >= nmem || (copies[m] && lens[m] > 0), "%s: null copy weights", who);
  }
  CASE_REQUIRE(total == S, "%s: the memories hold %lld positions, the source map %lld", who, (long long)total, (long long)S);
  a.V = V;
  a.S = S;
  a.nmem = nmem;
  return CASE_OK;
}

constexpr int64_t PH_MAX_V = 36000, PS_MAX_V = 131071;  // the vocabulary row in LDS; the key format alone
// K28's wide `dist_in` form: a histogram bin sums at most V fixed-point masses, each below 2^40 (the largest q lies below 2^e and the scale is
// 2^(40 - e)), so V <= 2^24 keeps every 64-bit sum below 2^64; the entry counts and the int ids need less
constexpr int64_t PW_MAX_DIST_V = 1ll << 24;

// the LDS forms: the row, the key staging and the reduction scratch; the wide forms (V = 0): the staging and the scratch alone
static size_t pointer_head_lds(int64_t V) { return (size_t)(((V + 3) & ~(int64_t)3) + (PH_THREADS + 4) + PH_THREADS + 64) * 4; }

// the history operands of K32: hist [R, Tmax] int32, step t, n >= 1
static int pointer_head_ban(BanArgs& nb, const char* who, const int32_t* hist, int64_t Tmax, int64_t t, int32_t n, int64_t eos) {
  CASE_REQUIRE(hist && n >= 1 && t >= 0 && t < Tmax, "%s: bad history argument", who);
  if (t > NB_MAX_T) return case_set_error(CASE_E_UNSUPPORTED, "%s: the n-gram ban stages histories of up to %d tokens (step %lld)", who, NB_MAX_T, (long long)t);
  nb.hist = const_cast<int32_t*>(hist);
  nb.Tmax = Tmax;
  nb.eos = eos;
  nb.t = (int)t;
  nb.n = (int)n;
  return CASE_OK;
}

// the operands of the decoding rules (CASE_FEAT_DECODE_RULES)
static int pointer_head_rule_args(RuleArgs& rl, const char* who, int64_t rows, int64_t t, int64_t eos, int32_t min_length, const int32_t* banned, int32_t K,
                                  int64_t banned_stride, int64_t rows_per_item) {
  CASE_REQUIRE(t >= 0 && t < (1ll << 31) && min_length >= 0 && K >= 0 && (K == 0 || banned) && rows_per_item >= 1 &&
                   (banned_stride == 0 || (banned_stride == K && rows % rows_per_item == 0)),
               "%s: bad rule argument (t >= 0, min_length >= 0, banned [K] with stride 0 or [rows / rows_per_item, K] with stride K)", who);
  if (K > RR_MAX_BAD) return case_set_error(CASE_E_UNSUPPORTED, "%s: at most %d banned ids per item (got %d)", who, RR_MAX_BAD, K);
  rl.bad = K ? banned : nullptr;
  rl.eos = eos;
  rl.bad_stride = K ? banned_stride : 0;
  rl.rows_per_item = rows_per_item;
  rl.t = (int)t;
  rl.min_len = (int)min_length;
  rl.nbad = (int)K;
  return CASE_OK;
}

// ---- one call of a fused head (K23 argmax, K24 top-W, K28 draw), as any of their 15 entry points states it -------------------------------------
// The entry points differ in which of the optional parts they carry; what a head kind adds (its outputs, W, the draw) goes to its launcher.
struct HeadWorkspace {  // the row of a `_wide` form: [R, stride] f32 in device memory
  float* ws;
  int64_t stride;
};
struct HeadHistory {  // K32's operands; hist == NULL or n == 0 means no ban unless the entry point (a `_ban` form) requires one
  const int32_t* hist;
  int64_t Tmax, t;
  int32_t n;
  int64_t eos;
  bool required;
};
struct HeadRules {  // the operands of a `_rules` form (which always brings a HeadHistory: the step t is there)
  int64_t eos;
  int32_t min_length;
  const int32_t* banned;
  int32_t K;
  int64_t banned_stride, rows_per_item;
};
struct HeadCall {
  const char* who;
  // the row source: the operands of the row build, or (K28 alone, logits null) a ready distribution
  const float *logits, *mix_logits;
  const uint32_t* keys;
  const float* const* copies;
  const int64_t* lens;
  int32_t nmem;
  const float* dist_in;
  float *gen, *dist;  // each [R, V] or null
  int64_t R, V, S;
  case_stream_t stream;
  const HeadWorkspace* wide;  // null: the row in LDS (V <= 36 000)
  const HeadHistory* ban;     // null: the entry point takes no history
  const HeadRules* rules;     // null: the entry point takes no rules
};

// the history and the rules as the kernels' trailing argument (the instances without rules take its BanArgs part); ban: a history is applied
static int pointer_head_tail(const HeadCall& c, RuleBanArgs& nb, bool& ban) {
  nb = RuleBanArgs();
  ban = c.ban && (c.ban->required || (c.ban->hist != nullptr && c.ban->n != 0));
  if (ban)
    if (const int rc = pointer_head_ban(nb, c.who, c.ban->hist, c.ban->Tmax, c.ban->t, c.ban->n, c.ban->eos)) return rc;
  if (!c.rules) return CASE_OK;
  const HeadRules& r = *c.rules;
  return pointer_head_rule_args(nb.rl, c.who, c.R, c.ban->t, r.eos, r.min_length, r.banned, r.K, r.banned_stride, r.rows_per_item);
}

// the row's operands: built from the logits or (`dist_in`) read as it is; the wide forms' workspace [R, row_stride] f32, row_stride >= V and a
// multiple of 4, 16-byte aligned (K28 reads float4), unless the row is read where it lies
static int pointer_head_row(const HeadCall& c, HeadArgs& a, bool in_place = false) {
  a = HeadArgs();
  if (!c.dist_in) {
    const int rc = pointer_head_fill(a, c.who, c.logits, c.mix_logits, c.keys, c.copies, c.lens, c.nmem, c.R, c.V, c.S, c.wide ? PS_MAX_V : PH_MAX_V,
                                     c.wide ? "" : " (run the softmax / scatter / argmax launches)");
    if (rc != CASE_OK) return rc;
    a.gen = c.gen;
  } else {
    const int64_t max_v = c.wide ? PW_MAX_DIST_V : PH_MAX_V;
    if (c.V > max_v) return case_set_error(CASE_E_UNSUPPORTED, "%s: built for V <= %lld", c.who, (long long)max_v);
    a.V = c.V;
  }
  a.dist = c.dist;
  if (!c.wide || in_place) return CASE_OK;
  CASE_REQUIRE(c.wide->ws && c.wide->stride >= c.V && c.wide->stride % 4 == 0 && (reinterpret_cast<uintptr_t>(c.wide->ws) & 15) == 0,
               "%s: the row workspace must be 16-byte aligned f32 [rows, row_stride], row_stride >= V and a multiple of 4", c.who);
  a.row_ws = c.wide->ws;
  a.row_stride = c.wide->stride;
  return CASE_OK;
}

// The three runtime flags as compile-time constants for a generic lambda: the six instances every head kernel has.
//   plain <false, false, false>   `_ban` <true, false, false>   `_wide` <ban given, true, false>   `_rules` <true, false, true>   `_wide_rules` <true, true, true>
// (the rules instances take n = 0 for "no ban", so there is no <false, *, true>)
template <typename F>
static int pointer_head_pick(bool ban, bool wide, bool rules, F&& f) {
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (rules) return wide ? f(yes, yes, yes) : f(yes, no, yes);
  if (wide) return ban ? f(yes, yes, no) : f(no, yes, no);
  return ban ? f(yes, no, no) : f(no, no, no);
}

// One workgroup per row.  An instance that keeps the vocabulary row in LDS has its dynamic-LDS ceiling raised once per process.
template <auto KERNEL, bool WIDE, typename... Args>
static int pointer_head_launch(const HeadCall& c, const Args&... args) {
  if constexpr (!WIDE) {
    static bool reserved = false;
    if (!reserved && hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, 158 * 1024) != hipSuccess)
      return case_set_error(CASE_E_LAUNCH, "%s: cannot reserve LDS", c.who);
    reserved = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)c.R), dim3(PH_THREADS), pointer_head_lds(WIDE ? 0 : c.V), (hipStream_t)c.stream, args...);
  return case_check_launch(c.who);
}

// K23
static int pointer_head_argmax(const HeadCall& c, int64_t* ids, float* top) {
  RuleBanArgs nb;
  bool ban;
  if (const int rc = pointer_head_tail(c, nb, ban)) return rc;
  CASE_REQUIRE(ids, "%s: bad argument", c.who);
  HeadArgs a;
  if (const int rc = pointer_head_row(c, a)) return rc;
  a.ids = ids;
  a.top = top;
  return pointer_head_pick(ban, c.wide != nullptr, c.rules != nullptr, [&](auto BAN, auto WIDE, auto RULES) {
    return pointer_head_launch<&pointer_head_decode_kernel<BAN(), WIDE(), RULES()>, WIDE()>(c, a, nb);
  });
}

// K24
static int pointer_head_top(const HeadCall& c, float* cand_p, int64_t* cand_id, int32_t W) {
  RuleBanArgs nb;
  bool ban;
  if (const int rc = pointer_head_tail(c, nb, ban)) return rc;
  CASE_REQUIRE(cand_p && cand_id, "%s: bad argument", c.who);
  if (W < 1 || W > PH_MAX_W || W > c.V) return case_set_error(CASE_E_UNSUPPORTED, "%s: width %d outside 1 .. min(%d, V)", c.who, W, PH_MAX_W);
  HeadArgs a;
  if (const int rc = pointer_head_row(c, a)) return rc;
  return pointer_head_pick(ban, c.wide != nullptr, c.rules != nullptr, [&](auto BAN, auto WIDE, auto RULES) {
    return pointer_head_launch<&pointer_head_beam_kernel<BAN(), WIDE(), RULES()>, WIDE()>(c, a, cand_p, cand_id, (int)W, nb);
  });
}

// K28 (s.dist_in is the call's)
static int pointer_head_draw(const HeadCall& c, SampleArgs s) {
  RuleBanArgs nb;
  bool ban;
  if (const int rc = pointer_head_tail(c, nb, ban)) return rc;
  CASE_REQUIRE(s.ids && s.prob && s.ended && c.R > 0 && c.V > 0 && c.R < (1ll << 31), "%s: bad argument", c.who);
  CASE_REQUIRE(s.temperature > 0.f && s.top_k >= 0 && s.top_p > 0.f && s.top_p <= 1.f, "%s: temperature must be > 0, top_k >= 0 and top_p in (0, 1]", c.who);
  CASE_REQUIRE((c.logits != nullptr) != (c.dist_in != nullptr), "%s: give either the logits or a ready distribution", c.who);
  // the wide form reads a ready distribution where it lies when its rows are 16-byte aligned and nothing is to be zeroed in them
  const bool in_place = c.wide && !c.logits && !ban && !c.rules && c.V % 4 == 0 && (reinterpret_cast<uintptr_t>(c.dist_in) & 15) == 0;
  HeadArgs a;
  if (const int rc = pointer_head_row(c, a, in_place)) return rc;
  s.dist_in = c.dist_in;
  return pointer_head_pick(ban, c.wide != nullptr, c.rules != nullptr, [&](auto BAN, auto WIDE, auto RULES) {
    return pointer_head_launch<&pointer_head_sample_kernel<BAN(), WIDE(), RULES()>, WIDE()>(c, a, s, nb);
  });
}

static SampleArgs sample_args(int64_t* ids, float* prob, uint8_t* ended, const float* uniforms, float temperature, int32_t top_k, float top_p,
                              uint64_t seed, uint64_t offset, const CaseStepState* state, int64_t eos, int64_t unk, int64_t pad, int32_t first,
                              int32_t last) {
  // (the fields in SampleArgs' order; dist_in is the call's)
  return {nullptr, uniforms, state, seed, offset, ended, ids, prob, eos, unk, pad, temperature, top_p, top_k, first, last};
}

// ---- the 15 entry points: each states its call and hands it to its head's launcher --------------------------------------------------------------
extern "C" int case_pointer_head_decode(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                        const int64_t* lens, int32_t nmem, float* gen, float* dist, int64_t* ids, float* top, int64_t B, int64_t V,
                                        int64_t S, case_stream_t stream) {
  return pointer_head_argmax({"case_pointer_head_decode", logits, mix_logits, keys, copies, lens, nmem, nullptr, gen, dist, B, V, S, stream}, ids, top);
}

extern "C" int case_pointer_head_decode_ban(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                            const int64_t* lens, int32_t nmem, float* gen, float* dist, int64_t* ids, float* top, int64_t B,
                                            int64_t V, int64_t S, int32_t* hist, int64_t Tmax, int64_t t, int32_t n, int64_t eos,
                                            case_stream_t stream) {
  const HeadHistory ban = {hist, Tmax, t, n, eos, true};
  return pointer_head_argmax({"case_pointer_head_decode_ban", logits, mix_logits, keys, copies, lens, nmem, nullptr, gen, dist, B, V, S, stream, nullptr, &ban},
                             ids, top);
}

extern "C" int case_pointer_head_decode_wide(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                             const int64_t* lens, int32_t nmem, float* gen, float* dist, int64_t* ids, float* top, int64_t B,
                                             int64_t V, int64_t S, float* row_ws, int64_t row_stride, int32_t* hist, int64_t Tmax, int64_t t,
                                             int32_t n, int64_t eos, case_stream_t stream) {
  const HeadWorkspace ws = {row_ws, row_stride};
  const HeadHistory ban = {hist, Tmax, t, n, eos, false};
  return pointer_head_argmax({"case_pointer_head_decode_wide", logits, mix_logits, keys, copies, lens, nmem, nullptr, gen, dist, B, V, S, stream, &ws, &ban},
                             ids, top);
}

extern "C" int case_pointer_head_decode_rules(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                              const int64_t* lens, int32_t nmem, float* gen, float* dist, int64_t* ids, float* top, int64_t B,
                                              int64_t V, int64_t S, int32_t* hist, int64_t Tmax, int64_t t, int32_t n, int64_t ban_eos, int64_t eos,
                                              int32_t min_length, const int32_t* banned, int32_t K, int64_t banned_stride, int64_t rows_per_item,
                                              case_stream_t stream) {
  const HeadHistory ban = {hist, Tmax, t, n, ban_eos, false};
  const HeadRules rules = {eos, min_length, banned, K, banned_stride, rows_per_item};
  return pointer_head_argmax(
      {"case_pointer_head_decode_rules", logits, mix_logits, keys, copies, lens, nmem, nullptr, gen, dist, B, V, S, stream, nullptr, &ban, &rules}, ids, top);
}

extern "C" int case_pointer_head_decode_wide_rules(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                                   const int64_t* lens, int32_t nmem, float* gen, float* dist, int64_t* ids, float* top, int64_t B,
                                                   int64_t V, int64_t S, float* row_ws, int64_t row_stride, int32_t* hist, int64_t Tmax, int64_t t,
                                                   int32_t n, int64_t ban_eos, int64_t eos, int32_t min_length, const int32_t* banned, int32_t K,
                                                   int64_t banned_stride, int64_t rows_per_item, case_stream_t stream) {
  const HeadWorkspace ws = {row_ws, row_stride};
  const HeadHistory ban = {hist, Tmax, t, n, ban_eos, false};
  const HeadRules rules = {eos, min_length, banned, K, banned_stride, rows_per_item};
  return pointer_head_argmax(
      {"case_pointer_head_decode_wide_rules", logits, mix_logits, keys, copies, lens, nmem, nullptr, gen, dist, B, V, S, stream, &ws, &ban, &rules}, ids, top);
}

extern "C" int case_pointer_head_beam(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                      const int64_t* lens, int32_t nmem, float* gen, float* dist, float* cand_p, int64_t* cand_id, int64_t R,
                                      int64_t V, int64_t S, int32_t W, case_stream_t stream) {
  return pointer_head_top({"case_pointer_head_beam", logits, mix_logits, keys, copies, lens, nmem, nullptr, gen, dist, R, V, S, stream}, cand_p, cand_id, W);
}

extern "C" int case_pointer_head_beam_ban(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                          const int64_t* lens, int32_t nmem, float* gen, float* dist, float* cand_p, int64_t* cand_id, int64_t R,
                                          int64_t V, int64_t S, int32_t W, const int32_t* hist, int64_t Tmax, int64_t t, int32_t n, int64_t eos,
                                          case_stream_t stream) {
  const HeadHistory ban = {hist, Tmax, t, n, eos, true};
  return pointer_head_top({"case_pointer_head_beam_ban", logits, mix_logits, keys, copies, lens, nmem, nullptr, gen, dist, R, V, S, stream, nullptr, &ban},
                          cand_p, cand_id, W);
}

extern "C" int case_pointer_head_beam_wide(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                           const int64_t* lens, int32_t nmem, float* gen, float* dist, float* cand_p, int64_t* cand_id, int64_t R,
                                           int64_t V, int64_t S, int32_t W, float* row_ws, int64_t row_stride, const int32_t* hist, int64_t Tmax,
                                           int64_t t, int32_t n, int64_t eos, case_stream_t stream) {
  const HeadWorkspace ws = {row_ws, row_stride};
  const HeadHistory ban = {hist, Tmax, t, n, eos, false};
  return pointer_head_top({"case_pointer_head_beam_wide", logits, mix_logits, keys, copies, lens, nmem, nullptr, gen, dist, R, V, S, stream, &ws, &ban},
                          cand_p, cand_id, W);
}

extern "C" int case_pointer_head_beam_rules(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                            const int64_t* lens, int32_t nmem, float* gen, float* dist, float* cand_p, int64_t* cand_id, int64_t R,
                                            int64_t V, int64_t S, int32_t W, const int32_t* hist, int64_t Tmax, int64_t t, int32_t n, int64_t ban_eos,
                                            int64_t eos, int32_t min_length, const int32_t* banned, int32_t K, int64_t banned_stride,
                                            int64_t rows_per_item, case_stream_t stream) {
  const HeadHistory ban = {hist, Tmax, t, n, ban_eos, false};
  const HeadRules rules = {eos, min_length, banned, K, banned_stride, rows_per_item};
  return pointer_head_top(
      {"case_pointer_head_beam_rules", logits, mix_logits, keys, copies, lens, nmem, nullptr, gen, dist, R, V, S, stream, nullptr, &ban, &rules}, cand_p,
      cand_id, W);
}

extern "C" int case_pointer_head_beam_wide_rules(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                                 const int64_t* lens, int32_t nmem, float* gen, float* dist, float* cand_p, int64_t* cand_id, int64_t R,
                                                 int64_t V, int64_t S, int32_t W, float* row_ws, int64_t row_stride, const int32_t* hist, int64_t Tmax,
                                                 int64_t t, int32_t n, int64_t ban_eos, int64_t eos, int32_t min_length, const int32_t* banned, int32_t K,
                                                 int64_t banned_stride, int64_t rows_per_item, case_stream_t stream) {
  const HeadWorkspace ws = {row_ws, row_stride};
  const HeadHistory ban = {hist, Tmax, t, n, ban_eos, false};
  const HeadRules rules = {eos, min_length, banned, K, banned_stride, rows_per_item};
  return pointer_head_top(
      {"case_pointer_head_beam_wide_rules", logits, mix_logits, keys, copies, lens, nmem, nullptr, gen, dist, R, V, S, stream, &ws, &ban, &rules}, cand_p,
      cand_id, W);
}

// K28: the history's `eos` is the loop's; the rules bring their own (`rule_eos`)
extern "C" int case_pointer_head_sample(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                        const int64_t* lens, int32_t nmem, const float* dist_in, float* gen, float* dist, int64_t* ids, float* prob,
                                        uint8_t* ended, const float* uniforms, int64_t R, int64_t V, int64_t S, float temperature, int32_t top_k,
                                        float top_p, uint64_t seed, uint64_t offset, const CaseStepState* state, int64_t eos, int64_t unk,
                                        int64_t pad, int32_t first, int32_t last, case_stream_t stream) {
  return pointer_head_draw({"case_pointer_head_sample", logits, mix_logits, keys, copies, lens, nmem, dist_in, gen, dist, R, V, S, stream},
                           sample_args(ids, prob, ended, uniforms, temperature, top_k, top_p, seed, offset, state, eos, unk, pad, first, last));
}

extern "C" int case_pointer_head_sample_ban(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                            const int64_t* lens, int32_t nmem, const float* dist_in, float* gen, float* dist, int64_t* ids,
                                            float* prob, uint8_t* ended, const float* uniforms, int64_t R, int64_t V, int64_t S, float temperature,
                                            int32_t top_k, float top_p, uint64_t seed, uint64_t offset, const CaseStepState* state, int64_t eos,
                                            int64_t unk, int64_t pad, int32_t first, int32_t last, int32_t* hist, int64_t Tmax, int64_t t, int32_t n,
                                            case_stream_t stream) {
  const HeadHistory ban = {hist, Tmax, t, n, eos, true};
  return pointer_head_draw({"case_pointer_head_sample_ban", logits, mix_logits, keys, copies, lens, nmem, dist_in, gen, dist, R, V, S, stream, nullptr, &ban},
                           sample_args(ids, prob, ended, uniforms, temperature, top_k, top_p, seed, offset, state, eos, unk, pad, first, last));
}

extern "C" int case_pointer_head_sample_wide(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                             const int64_t* lens, int32_t nmem, const float* dist_in, float* gen, float* dist, int64_t* ids,
                                             float* prob, uint8_t* ended, const float* uniforms, int64_t R, int64_t V, int64_t S, float temperature,
                                             int32_t top_k, float top_p, uint64_t seed, uint64_t offset, const CaseStepState* state, int64_t eos,
                                             int64_t unk, int64_t pad, int32_t first, int32_t last, float* row_ws, int64_t row_stride, int32_t* hist,
                                             int64_t Tmax, int64_t t, int32_t n, case_stream_t stream) {
  const HeadWorkspace ws = {row_ws, row_stride};
  const HeadHistory ban = {hist, Tmax, t, n, eos, false};
  return pointer_head_draw({"case_pointer_head_sample_wide", logits, mix_logits, keys, copies, lens, nmem, dist_in, gen, dist, R, V, S, stream, &ws, &ban},
                           sample_args(ids, prob, ended, uniforms, temperature, top_k, top_p, seed, offset, state, eos, unk, pad, first, last));
}

extern "C" int case_pointer_head_sample_rules(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                              const int64_t* lens, int32_t nmem, const float* dist_in, float* gen, float* dist, int64_t* ids,
                                              float* prob, uint8_t* ended, const float* uniforms, int64_t R, int64_t V, int64_t S, float temperature,
                                              int32_t top_k, float top_p, uint64_t seed, uint64_t offset, const CaseStepState* state, int64_t eos,
                                              int64_t unk, int64_t pad, int32_t first, int32_t last, int32_t* hist, int64_t Tmax, int64_t t, int32_t n,
                                              int64_t rule_eos, int32_t min_length, const int32_t* banned, int32_t K, int64_t banned_stride,
                                              int64_t rows_per_item, case_stream_t stream) {
  const HeadHistory ban = {hist, Tmax, t, n, eos, false};
  const HeadRules rules = {rule_eos, min_length, banned, K, banned_stride, rows_per_item};
  return pointer_head_draw(
      {"case_pointer_head_sample_rules", logits, mix_logits, keys, copies, lens, nmem, dist_in, gen, dist, R, V, S, stream, nullptr, &ban, &rules},
      sample_args(ids, prob, ended, uniforms, temperature, top_k, top_p, seed, offset, state, eos, unk, pad, first, last));
}

extern "C" int case_pointer_head_sample_wide_rules(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                                   const int64_t* lens, int32_t nmem, const float* dist_in, float* gen, float* dist, int64_t* ids,
                                                   float* prob, uint8_t* ended, const float* uniforms, int64_t R, int64_t V, int64_t S,
                                                   float temperature, int32_t top_k, float top_p, uint64_t seed, uint64_t offset,
                                                   const CaseStepState* state, int64_t eos, int64_t unk, int64_t pad, int32_t first, int32_t last,
                                                   float* row_ws, int64_t row_stride, int32_t* hist, int64_t Tmax, int64_t t, int32_t n,
                                                   int64_t rule_eos, int32_t min_length, const int32_t* banned, int32_t K, int64_t banned_stride,
                                                   int64_t rows_per_item, case_stream_t stream) {
  const HeadWorkspace ws = {row_ws, row_stride};
  const HeadHistory ban = {hist, Tmax, t, n, eos, false};
  const HeadRules rules = {rule_eos, min_length, banned, K, banned_stride, rows_per_item};
  return pointer_head_draw(
      {"case_pointer_head_sample_wide_rules", logits, mix_logits, keys, copies, lens, nmem, dist_in, gen, dist, R, V, S, stream, &ws, &ban, &rules},
      sample_args(ids, prob, ended, uniforms, temperature, top_k, top_p, seed, offset, state, eos, unk, pad, first, last));
}

// K32 as a launch of its own (the unfused head): one wave per row zeroes the banned entries of dist [R, V] in place
extern "C" int case_ngram_ban(float* dist, const int32_t* hist, const uint8_t* ended, int64_t R, int64_t V, int64_t Tmax, int64_t t, int32_t n,
                              int64_t eos, case_stream_t stream) {
  CASE_REQUIRE(dist && R > 0 && R < (1ll << 31) && V > 0, "case_ngram_ban: bad argument");
  BanArgs nb;
  const int rc = pointer_head_ban(nb, "case_ngram_ban", hist, Tmax, t, n, eos);
  if (rc != CASE_OK) return rc;
  hipLaunchKernelGGL(ngram_ban_kernel, dim3((unsigned)R), dim3(64), 0, (hipStream_t)stream, dist, ended, V, nb);
  return case_check_launch("case_ngram_ban");
}

// the rules as a launch of their own (the unfused head): one wave per row zeroes the entries of dist [R, V] in place
extern "C" int case_row_rules(float* dist, const uint8_t* ended, int64_t R, int64_t V, int64_t t, int64_t eos, int32_t min_length,
                              const int32_t* banned, int32_t K, int64_t banned_stride, int64_t rows_per_item, case_stream_t stream) {
  CASE_REQUIRE(dist && R > 0 && R < (1ll << 31) && V > 0, "case_row_rules: bad argument");
  RuleArgs rl;
  const int rc = pointer_head_rule_args(rl, "case_row_rules", R, t, eos, min_length, banned, K, banned_stride, rows_per_item);
  if (rc != CASE_OK) return rc;
  hipLaunchKernelGGL(row_rules_kernel, dim3((unsigned)R), dim3(64), 0, (hipStream_t)stream, dist, ended, V, rl);
  return case_check_launch("case_row_rules");
}

static int pointer_head_score_launch(const char* who, const float* logits, const float* mix_logits, const uint32_t* keys, int64_t rows_per_source,
                                     const float* const* copies, const int64_t* lens, int32_t nmem, const int64_t* targets, int64_t pad,
                                     float* prob, float* copy, float* stats, int64_t R, int64_t V, int64_t S, case_stream_t stream,
                                     float* nll = nullptr, int64_t ld = 0) {
  CASE_REQUIRE(targets && prob, "%s: bad argument", who);
  CASE_REQUIRE(rows_per_source >= 1 && R % rows_per_source == 0, "%s: %lld rows are no multiple of rows_per_source %lld", who, (long long)R,
               (long long)rows_per_source);
  ScoreArgs a;
  const int rc = pointer_head_fill(a, who, logits, mix_logits, keys, copies, lens, nmem, R, V, S, PS_MAX_V, "");
  if (rc != CASE_OK) return rc;
  a.targets = targets;
  a.prob = prob;
  a.ptr = copy;
  a.stats = stats;
  a.nll = nll;
  a.ld = ld;
  a.rows_per_source = rows_per_source;
  a.pad = pad;
  if (nll) hipLaunchKernelGGL(pointer_head_score_kernel<true>, dim3((unsigned)R), dim3(PS_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(pointer_head_score_kernel<false>, dim3((unsigned)R), dim3(PS_THREADS), 0, (hipStream_t)stream, a);
  return case_check_launch(who);
}

extern "C" int case_pointer_head_score(const float* logits, const float* mix_logits, const uint32_t* keys, int64_t rows_per_source,
                                       const float* const* copies, const int64_t* lens, int32_t nmem, const int64_t* targets, int64_t pad,
                                       float* prob, float* copy, int64_t R, int64_t V, int64_t S, case_stream_t stream) {
  return pointer_head_score_launch("case_pointer_head_score", logits, mix_logits, keys, rows_per_source, copies, lens, nmem, targets, pad, prob, copy,
                                   nullptr, R, V, S, stream);
}

extern "C" int case_pointer_head_score_stats(const float* logits, const float* mix_logits, const uint32_t* keys, int64_t rows_per_source,
                                             const float* const* copies, const int64_t* lens, int32_t nmem, const int64_t* targets, int64_t pad,
                                             float* prob, float* copy, float* stats, int64_t R, int64_t V, int64_t S, case_stream_t stream) {
  return pointer_head_score_launch("case_pointer_head_score_stats", logits, mix_logits, keys, rows_per_source, copies, lens, nmem, targets, pad, prob,
                                   copy, stats, R, V, S, stream);
}

// K41 and its loss form: ld < 0 = K41 itself (f32 rows V apart); else the loss form with rows ld apart and d_logits of `d_dtype`
static int pointer_head_score_bwd_launch(const char* who, const float* logits, const float* mix_logits, const int64_t* ids, int64_t rows_per_source,
                                         const float* const* copies, const int64_t* lens, int32_t nmem, const int64_t* targets, int64_t pad,
                                         const float* stats, const float* prob, const float* g, void* d_logits, float* d_mix,
                                         float* const* d_copies, int64_t R, int64_t V, int64_t S, case_stream_t stream, int64_t ld, int32_t d_dtype) {
  CASE_REQUIRE(logits && mix_logits && ids && copies && lens && targets && stats && prob && g && d_logits && d_mix && d_copies && R > 0 && V > 0 &&
                   S > 0 && nmem >= 1 && R < (1ll << 31),
               "%s: bad argument", who);
  CASE_REQUIRE(rows_per_source >= 1 && R % rows_per_source == 0, "%s: %lld rows are no multiple of rows_per_source %lld", who, (long long)R,
               (long long)rows_per_source);
  if (nmem > PH_MAX_MEM || V > PS_MAX_V || S > 32768)
    return case_set_error(CASE_E_UNSUPPORTED, "%s: built for <= %d memories, V <= %lld, S <= 32768", who, PH_MAX_MEM, (long long)PS_MAX_V);
  ScoreBwdArgs a;
  int64_t total = 0;
  for (int m = 0; m < PH_MAX_MEM; ++m) {
    CASE_REQUIRE(m >= nmem || (copies[m] && d_copies[m] && lens[m] > 0), "%s: null copy weights", who);
    a.copy[m] = m < nmem ? copies[m] : nullptr;
    a.d_copy[m] = m < nmem ? d_copies[m] : nullptr;
    a.len[m] = m < nmem ? lens[m] : 0;
    total += a.len[m];
  }
  CASE_REQUIRE(total == S, "%s: the memories hold %lld positions, the source map %lld", who, (long long)total, (long long)S);
  a.logits = logits;
  a.mix_logits = mix_logits;
  a.ids = ids;
  a.targets = targets;
  a.stats = stats;
  a.prob = prob;
  a.g = g;
  a.d_logits = d_logits;
  a.d_mix = d_mix;
  a.V = V;
  a.S = S;
  a.rows_per_source = rows_per_source;
  a.pad = pad;
  a.nmem = nmem;
  a.ld = ld;
  const dim3 grid((unsigned)R), block(PS_THREADS);
  if (ld < 0) hipLaunchKernelGGL((pointer_head_score_bwd_kernel<float, false>), grid, block, 0, (hipStream_t)stream, a);
  else if (d_dtype == CASE_BF16) hipLaunchKernelGGL((pointer_head_score_bwd_kernel<bf16_t, true>), grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((pointer_head_score_bwd_kernel<float, true>), grid, block, 0, (hipStream_t)stream, a);
  return case_check_launch(who);
}

extern "C" int case_pointer_head_score_bwd(const float* logits, const float* mix_logits, const int64_t* ids, int64_t rows_per_source,
                                           const float* const* copies, const int64_t* lens, int32_t nmem, const int64_t* targets, int64_t pad,
                                           const float* stats, const float* prob, const float* g, float* d_logits, float* d_mix,
                                           float* const* d_copies, int64_t R, int64_t V, int64_t S, case_stream_t stream) {
  return pointer_head_score_bwd_launch("case_pointer_head_score_bwd", logits, mix_logits, ids, rows_per_source, copies, lens, nmem, targets, pad, stats,
                                       prob, g, d_logits, d_mix, d_copies, R, V, S, stream, -1, CASE_F32);
}

// the training head: K29 with row statistics plus the per-row loss, over logits rows `ld_logits` apart
extern "C" int case_pointer_head_loss(const float* logits, int64_t ld_logits, const float* mix_logits, const uint32_t* keys, int64_t rows_per_source,
                                      const float* const* copies, const int64_t* lens, int32_t nmem, const int64_t* targets, int64_t pad,
                                      float* prob, float* copy, float* stats, float* nll, int64_t R, int64_t V, int64_t S, case_stream_t stream) {
  const char* who = "case_pointer_head_loss";
  CASE_REQUIRE(stats && nll, "%s: bad argument", who);
  CASE_REQUIRE(ld_logits >= V && ld_logits % 4 == 0 && (uintptr_t)logits % 16 == 0,
               "%s: logits rows must lie ld_logits >= V floats apart, a multiple of 4, on a 16-byte base (got ld %lld, V %lld)", who,
               (long long)ld_logits, (long long)V);
  return pointer_head_score_launch(who, logits, mix_logits, keys, rows_per_source, copies, lens, nmem, targets, pad, prob, copy, stats, R, V, S, stream,
                                   nll, ld_logits);
}

extern "C" int case_pointer_head_loss_bwd(const float* logits, int64_t ld_logits, const float* mix_logits, const int64_t* ids, int64_t rows_per_source,
                                          const float* const* copies, const int64_t* lens, int32_t nmem, const int64_t* targets, int64_t pad,
                                          const float* stats, const float* prob, const float* g_nll, void* d_logits, int32_t d_dtype, float* d_mix,
                                          float* const* d_copies, int64_t R, int64_t V, int64_t S, case_stream_t stream) {
  const char* who = "case_pointer_head_loss_bwd";
  CASE_REQUIRE(d_dtype == CASE_F32 || d_dtype == CASE_BF16, "%s: d_logits is f32 or bf16 (got dtype %d)", who, (int)d_dtype);
  CASE_REQUIRE(ld_logits >= V && ld_logits % 8 == 0 && (uintptr_t)logits % 16 == 0 && (uintptr_t)d_logits % 16 == 0,
               "%s: logits / d_logits rows must lie ld_logits >= V elements apart, a multiple of 8, on 16-byte bases (got ld %lld, V %lld)", who,
               (long long)ld_logits, (long long)V);
  return pointer_head_score_bwd_launch(who, logits, mix_logits, ids, rows_per_source, copies, lens, nmem, targets, pad, stats, prob, g_nll, d_logits,
                                       d_mix, d_copies, R, V, S, stream, ld_logits, d_dtype);
}

extern "C" int case_copy_scatter_fwd(const int64_t* src, const float* w, float* dist, int64_t B, int64_t T, int64_t S,
                                     int64_t V, case_stream_t stream) {
  CASE_REQUIRE(src && w && dist && B > 0 && T > 0 && S > 0 && V > 0, "case_copy_scatter_fwd: bad argument");
  hipLaunchKernelGGL(copy_scatter_fwd_kernel, dim3(grid_for(B * T * S, 256, 2)), dim3(256), 0, (hipStream_t)stream, src, w,
                     dist, B, T, S, V);
  return case_check_launch("case_copy_scatter_fwd");
}

extern "C" int case_copy_scatter_bwd(const int64_t* src, const float* d_dist, float* d_w, int64_t B, int64_t T, int64_t S,
                                     int64_t V, case_stream_t stream) {
  CASE_REQUIRE(src && d_dist && d_w && B > 0 && T > 0 && S > 0 && V > 0, "case_copy_scatter_bwd: bad argument");
  hipLaunchKernelGGL(copy_scatter_bwd_kernel, dim3(grid_for(B * T * S, 256, 2)), dim3(256), 0, (hipStream_t)stream, src,
                     d_dist, d_w, B, T, S, V);
  return case_check_launch("case_copy_scatter_bwd");
}

extern "C" int case_source_sort(const int64_t* src, uint32_t* keys, int64_t B, int64_t S, int64_t V, case_stream_t stream) {
  CASE_REQUIRE(src && keys && B > 0 && S > 0 && V > 0, "case_source_sort: bad argument");
  CASE_REQUIRE(S <= 32768 && V <= 131071, "case_source_sort: S <= 32768 and V <= 131071 (token << 15 | position must fit 32 bits)");
  int n = 2;
  while (n < S) n <<= 1;
  // opt-in to > 64 KiB of dynamic LDS: idempotent host call, once per batch (no library state kept)
  if (n > 16384 && hipFuncSetAttribute((const void*)source_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * 4) != hipSuccess)
    return case_set_error(CASE_E_LAUNCH, "case_source_sort: cannot reserve 128 KiB of LDS");
  hipLaunchKernelGGL(source_sort_kernel, dim3((unsigned)B), dim3(1024), (size_t)n * 4, (hipStream_t)stream, src, keys, S, V, n);
  return case_check_launch("case_source_sort");
}

extern "C" int case_copy_scatter_sorted_fwd(const uint32_t* keys, const float* w, float* dist, int64_t B, int64_t T, int64_t S,
                                            int64_t V, case_stream_t stream) {
  CASE_REQUIRE(keys && w && dist && B > 0 && T > 0 && S > 0 && V > 0 && B * T < (1ll << 31), "case_copy_scatter_sorted_fwd: bad argument");
  CASE_REQUIRE(S <= 32768 && V <= 131071, "case_copy_scatter_sorted_fwd: S <= 32768 and V <= 131071");
  hipLaunchKernelGGL(copy_scatter_sorted_kernel, dim3((unsigned)(B * T)), dim3(256), 0, (hipStream_t)stream, keys, w, dist, T, S, V);
  return case_check_launch("case_copy_scatter_sorted_fwd");
}

extern "C" int case_nll_gather_fwd(const float* dist, const int64_t* target, float* per_row, int64_t rows, int64_t V,
                                   case_stream_t stream) {
  CASE_REQUIRE(dist && target && per_row && rows > 0 && V > 0, "case_nll_gather_fwd: bad argument");
  hipLaunchKernelGGL(nll_fwd_kernel, dim3(grid_for(rows, 256)), dim3(256), 0, (hipStream_t)stream, dist, target, per_row, rows, V);
  return case_check_launch("case_nll_gather_fwd");
}

extern "C" int case_nll_gather_bwd(const float* dist, const int64_t* target, const float* g_row, float* d_dist,
                                   int64_t rows, int64_t V, case_stream_t stream) {
  CASE_REQUIRE(dist && target && g_row && d_dist && rows > 0 && V > 0, "case_nll_gather_bwd: bad argument");
  hipLaunchKernelGGL(nll_bwd_kernel, dim3(grid_for(rows, 256)), dim3(256), 0, (hipStream_t)stream, dist, target, g_row, d_dist, rows, V);
  return case_check_launch("case_nll_gather_bwd");
}

namespace {
// ---- greedy post-processing (common/Utils.py:200-217 to_sentence): per answer row drop BOS / PAD, stop at the first EOS ----
// one thread per row (T <= a few hundred); out [B, T] receives the kept ids front-packed (pad behind), len [B] their count
__global__ void sentence_compact_kernel(const int64_t* __restrict__ ids, int64_t* __restrict__ out, int32_t* __restrict__ len,
                                        int64_t B, int64_t T, int64_t bos, int64_t pad, int64_t eos) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int n = 0;
  bool open = true;
  for (int64_t t = 0; t < T; ++t) {
    const int64_t id = ids[b * T + t];
    if (open && id == eos) open = false;
    if (open && id != bos && id != pad) out[b * T + n++] = id;
  }
  len[b] = n;
  for (int64_t t = n; t < T; ++t) out[b * T + t] = pad;
}

// ---- K33: the reference's remove_duplicate (common/Utils.py:170-193) on front-packed ids ------------------------------------------------
// One pass of remove_duplicate_once cuts a sentence of length L at the LARGEST i in [1, L - n] whose tail [i, L) holds only tokens that also
// occur in [0, i); the pass repeats until nothing is cut or L <= n.  With first[p] = the first position of token out[p] (unchanged by a cut),
// "every token of the tail occurs in the prefix" is  g(i) = max_{p >= i} first[p] < i.  One wave per row, T <= 256: lane l owns the four
// positions 4 l .. 4 l + 3, first[] stays in registers, and a pass is a suffix maximum over the wave (local, then a shuffle scan).
constexpr int RD_MAX_T = 256;
__global__ __launch_bounds__(64) void remove_duplicate_kernel(int64_t* __restrict__ out, int32_t* __restrict__ len, const int64_t T, const int n,
                                                              const int64_t pad) {
  __shared__ int64_t tok[RD_MAX_T];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  int64_t* row = out + b * T;
  int L = len[b];
  L = L < 0 ? 0 : (L > (int)T ? (int)T : L);
  const int L0 = L;
  for (int i = lane; i < L0; i += 64) tok[i] = row[i];
  __syncthreads();
  int first[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int p = 4 * lane + e;
    first[e] = p;
    if (p < L0) {
      const int64_t mine = tok[p];
      for (int q = 0; q < p; ++q)
        if (tok[q] == mine) {
          first[e] = q;
          break;
        }
    }
  }
  while (L > n) {  // (wave-uniform)
    int s[4];
#pragma unroll
    for (int e = 3; e >= 0; --e) {
      const int p = 4 * lane + e;
      const int x = p < L ? first[e] : -1;
      s[e] = e == 3 ? x : max(x, s[e + 1]);
    }
    int tot = s[0];  // the inclusive suffix maximum over the lanes' totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int other = __shfl_down(tot, o, 64);
      if (lane + o < 64) tot = max(tot, other);
    }
    int after = __shfl_down(tot, 1, 64);
    if (lane == 63) after = -1;
    int best = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * lane + e;
      if (i >= 1 && i <= L - n && max(s[e], after) < i) best = i;  // (i ascends: the lane's largest)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
    if (best < 1) break;
    L = best;
  }
  for (int i = L + lane; i < L0; i += 64) row[i] = pad;
  if (lane == 0) len[b] = L;
}
}  // namespace

extern "C" int case_sentence_compact(const int64_t* ids, int64_t* out, int32_t* len, int64_t B, int64_t T, int64_t bos, int64_t pad,
                                     int64_t eos, case_stream_t stream) {
  CASE_REQUIRE(ids && out && len && B > 0 && T > 0, "case_sentence_compact: bad argument");
  hipLaunchKernelGGL(sentence_compact_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, ids, out, len, B, T, bos,
                     pad, eos);
  return case_check_launch("case_sentence_compact");
}

extern "C" int case_remove_duplicate_ids(int64_t* out, int32_t* len, int64_t B, int64_t T, int32_t n, int64_t pad, case_stream_t stream) {
  CASE_REQUIRE(out && len && B > 0 && B < (1ll << 31) && T > 0 && n >= 1, "case_remove_duplicate_ids: bad argument");
  if (T > RD_MAX_T) return case_set_error(CASE_E_UNSUPPORTED, "case_remove_duplicate_ids: rows of up to %d positions (got %lld)", RD_MAX_T, (long long)T);
  hipLaunchKernelGGL(remove_duplicate_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, out, len, T, (int)n, pad);
  return case_check_launch("case_remove_duplicate_ids");
}

extern "C" int case_row_argmax(const float* x, int64_t* idx, float* val, int64_t rows, int64_t cols, int64_t ld,
                               case_stream_t stream) {
  CASE_REQUIRE(x && idx && rows > 0 && cols > 0 && ld >= cols, "case_row_argmax: bad argument");
  hipLaunchKernelGGL(row_argmax_kernel, dim3(grid_for(rows, 1)), dim3(256), 0, (hipStream_t)stream, x, idx, val, rows, cols, ld);
  return case_check_launch("case_row_argmax");
}
