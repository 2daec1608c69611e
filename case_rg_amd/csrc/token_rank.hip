// Threshold-free ranking metrics of the supporting-token stage.
//   K45 case_token_rank  per item: average precision, AUC (ties counted half) and the best F1 cut of a row of keys against 0 / 1 labels,
//                        every figure a function of the groups of equal key alone (evaluation/token_rank.py states the definitions)
// One workgroup per item, instantiated by the row length padded to a power of two N (64 .. 16384).  Every position becomes one u64
//     (key << 1) | positive          key = K38's order-preserving u32 (token.hip's token_score_bits), 0 = invalid or padding
// and the row is sorted descending by a bitonic network.  Thread t holds the elements e * THREADS + t in registers, so a step with partner
// distance j stays inside the thread for j >= THREADS, inside the wave (shuffles, no barrier) for j < 64, and goes through LDS only for
// 64 <= j < THREADS.  The sorted row is then left in LDS and read back in chunks of PER consecutive elements per thread; two workgroup
// prefix scans (the cumulative positives; the last group end before a position) give every group end its terms.
// Nothing here waits for the host, the kernel uses no atomic, and the library keeps no state.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "case_hip.h"
#include "common.h"

namespace {

constexpr int RANK_MAX_S = 16384;  // positions per item (K38's limit)
constexpr int RANK_MAX_WAVES = 16;

typedef unsigned long long u64;

__device__ __forceinline__ uint32_t rank_key_bits(const float x) {  // token.hip's token_score_bits
  uint32_t u = __float_as_uint(x);
  if (x != x) u = 0xff800000u;  // NaN compares as -inf
  if (x == 0.f) u = 0u;         // -0.0 == +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float rank_key_value(const uint32_t k) {  // the canonical f32 of a key: +0.0 for either zero, -inf for NaN
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ u64 rank_shfl_xor(const u64 v, const int mask) {
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask, 64), lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask, 64);
  return ((u64)hi << 32) | lo;
}

template <int N>
struct RankShape {
  static constexpr int THREADS = N <= 256 ? 64 : (N <= 2048 ? 256 : 1024);
  static constexpr int PER = N / THREADS;
  static constexpr int WAVES = THREADS / 64;
  // The chunked read of the sorted row has a stride of PER u64 between lanes; the slots of a chunk are rotated by an XOR that differs
  // between the lanes that would share a bank (32 u64 banks: 32 / PER neighbouring chunks differ in the low bits already)
  static constexpr int SWZ_SHIFT = PER >= 32 ? 0 : (PER == 16 ? 1 : (PER == 8 ? 2 : (PER == 4 ? 3 : 4)));
  static __device__ __forceinline__ int slot(const int i) { return PER == 1 ? i : i ^ (((i / PER) >> SWZ_SHIFT) & (PER - 1)); }
};

// The best F1 cut seen so far: the fraction 2 tp / den, compared exactly, then the lower sorted index
struct RankCut {
  int tp, den, idx;
};
__device__ __forceinline__ bool rank_cut_better(const RankCut& a, const RankCut& b) {
  const int l = a.tp * b.den, r = b.tp * a.den;  // < 2^14 * 2^15
  return l > r || (l == r && a.idx < b.idx);
}

template <int N>
__global__ __launch_bounds__(RankShape<N>::THREADS) void token_rank_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ valid,
                                                                           const float* __restrict__ labels, double* __restrict__ stats,
                                                                           int32_t* __restrict__ counts, float* __restrict__ threshold,
                                                                           const int S) {
#pragma clang fp contract(off)
  typedef RankShape<N> Sh;
  constexpr int THREADS = Sh::THREADS, PER = Sh::PER, WAVES = Sh::WAVES;
  extern __shared__ __attribute__((aligned(16))) u64 row[];  // N
  __shared__ int wave_int[4][RANK_MAX_WAVES];
  __shared__ double wave_ap[RANK_MAX_WAVES];
  __shared__ RankCut wave_cut[RANK_MAX_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t item = blockIdx.x;

  u64 v[PER];
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const int i = e * THREADS + tid;
    u64 x = 0ull;
    if (i < S && (valid == nullptr || valid[item * S + i] != 0))
      x = ((u64)rank_key_bits(scores[item * S + i]) << 1) | (labels[item * S + i] > 0.5f ? 1ull : 0ull);
    v[e] = x;
  }

  // ---- the bitonic network, descending --------------------------------------------------------------------------------------------
  for (int k = 2; k <= N; k <<= 1) {
    // partners in other registers of this thread
#pragma unroll
    for (int je = PER >> 1; je > 0; je >>= 1) {
      if (je * THREADS < k) {
#pragma unroll
        for (int e = 0; e < PER; ++e) {
          if ((e & je) == 0) {
            const bool desc = ((e * THREADS + tid) & k) == 0;
            const u64 a = v[e], b = v[e | je];
            const u64 hi = a > b ? a : b, lo = a > b ? b : a;
            v[e] = desc ? hi : lo;
            v[e | je] = desc ? lo : hi;
          }
        }
      }
    }
    // partners in other waves
    for (int j = (k >> 1) < (THREADS >> 1) ? (k >> 1) : (THREADS >> 1); j >= 64; j >>= 1) {
#pragma unroll
      for (int e = 0; e < PER; ++e) row[e * THREADS + tid] = v[e];
      __syncthreads();
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const u64 o = row[e * THREADS + (tid ^ j)];
        const bool take_max = ((tid & j) == 0) == (((e * THREADS + tid) & k) == 0);
        v[e] = (o > v[e]) == take_max ? o : v[e];
      }
      __syncthreads();
    }
    // partners in other lanes of the wave
    for (int j = (k >> 1) < 32 ? (k >> 1) : 32; j > 0; j >>= 1) {
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const u64 o = rank_shfl_xor(v[e], j);
        const bool take_max = ((tid & j) == 0) == (((e * THREADS + tid) & k) == 0);
        v[e] = (o > v[e]) == take_max ? o : v[e];
      }
    }
  }

  // ---- the sorted row: thread t now takes the elements t * PER .. t * PER + PER - 1 ---------------------------------------------
#pragma unroll
  for (int e = 0; e < PER; ++e) row[Sh::slot(e * THREADS + tid)] = v[e];
  __syncthreads();
  const int first = tid * PER;
#pragma unroll
  for (int e = 0; e < PER; ++e) v[e] = row[Sh::slot(first + e)];
  const u64 next = first + PER < N ? row[Sh::slot(first + PER)] : 0ull;

  // scan 1: the positives (low half) and the valid positions (high half) before this thread, and in the row
  int mine = 0;
#pragma unroll
  for (int e = 0; e < PER; ++e) mine += (int)(v[e] & 1ull) + (v[e] != 0ull ? 1 << 16 : 0);
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wave_int[0][wave] = incl;
  __syncthreads();
  int before = incl - mine, total = 0;
#pragma unroll
  for (int q = 0; q < WAVES; ++q) {
    const int w = wave_int[0][q];
    before += q < wave ? w : 0;
    total += w;
  }
  const int n_pos = total & 0xffff, n_valid = total >> 16, n_neg = n_valid - n_pos;

  // the group ends of this thread, each as ((index + 1) << 16) | cumulative positives: both grow along the row
  uint32_t end[PER];
  uint32_t last = 0u;
  {
    int tp = before & 0xffff;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const u64 after = e + 1 < PER ? v[e + 1 < PER ? e + 1 : e] : next;
      tp += (int)(v[e] & 1ull);
      const bool is_end = v[e] != 0ull && (v[e] >> 1) != (after >> 1);
      end[e] = is_end ? ((uint32_t)(first + e + 1) << 16) | (uint32_t)tp : 0u;
      last = end[e] > last ? end[e] : last;
    }
  }
  // scan 2: the last group end before this thread (0: none)
  uint32_t run = last;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)run, o, 64);
    if (lane >= o) run = up > run ? up : run;
  }
  if (lane == 63) wave_int[1][wave] = (int)run;
  uint32_t prev = (uint32_t)__shfl_up((int)run, 1, 64);
  if (lane == 0) prev = 0u;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < WAVES; ++q) {
    const uint32_t w = (uint32_t)wave_int[1][q];
    if (q < wave) prev = w > prev ? w : prev;
  }

  // the terms of this thread's group ends, in index order
  double ap = 0.0;
  int auc = 0, groups = 0;
  RankCut cut = {0, 1, 0x7fffffff};
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    if (end[e] != 0u) {
      const int n = (int)(end[e] >> 16), tp = (int)(end[e] & 0xffffu), n_before = (int)(prev >> 16), tp_before = (int)(prev & 0xffffu);
      const int pos_g = tp - tp_before, negcum = n - tp, neg_g = negcum - (n_before - tp_before);
      ap += (double)(pos_g * tp) / (double)n;  // the product is exact (< 2^28): one rounding per term
      auc += pos_g * (2 * (n_neg - negcum) + neg_g);
      groups += 1;
      const RankCut c = {tp, n + n_pos, first + e};
      if (rank_cut_better(c, cut)) cut = c;
      prev = end[e];
    }
  }

  // a fixed xor tree inside the wave, then the waves in order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ap += __shfl_xor(ap, o, 64);
    auc += __shfl_xor(auc, o, 64);
    groups += __shfl_xor(groups, o, 64);
    const RankCut c = {__shfl_xor(cut.tp, o, 64), __shfl_xor(cut.den, o, 64), __shfl_xor(cut.idx, o, 64)};
    if (rank_cut_better(c, cut)) cut = c;
  }
  if (lane == 0) {
    wave_ap[wave] = ap;
    wave_int[2][wave] = auc;
    wave_int[3][wave] = groups;
    wave_cut[wave] = cut;
  }
  __syncthreads();
  if (tid == 0) {
    double ap_sum = wave_ap[0];
    int auc_num2 = wave_int[2][0], n_groups = wave_int[3][0];
    RankCut best = wave_cut[0];
#pragma unroll
    for (int q = 1; q < WAVES; ++q) {
      ap_sum += wave_ap[q];
      auc_num2 += wave_int[2][q];
      n_groups += wave_int[3][q];
      if (rank_cut_better(wave_cut[q], best)) best = wave_cut[q];
    }
    const bool ranked = n_pos > 0;
    stats[item * 2 + 0] = ranked ? ap_sum / (double)n_pos : 0.0;
    stats[item * 2 + 1] = (ranked && n_neg > 0) ? (double)auc_num2 / (double)(2ll * n_pos * n_neg) : 0.0;
    counts[item * 6 + 0] = n_valid;
    counts[item * 6 + 1] = n_pos;
    counts[item * 6 + 2] = auc_num2;
    counts[item * 6 + 3] = ranked ? best.tp : 0;
    counts[item * 6 + 4] = ranked ? best.den - n_pos : 0;
    counts[item * 6 + 5] = n_groups;
    threshold[item] = ranked ? rank_key_value((uint32_t)(row[Sh::slot(best.idx)] >> 1)) : INFINITY;
  }
}

template <int N>
int token_rank_launch(const float* scores, const uint8_t* valid, const float* labels, double* stats, int32_t* counts, float* threshold, int64_t B,
                      int64_t S, hipStream_t stream) {
  constexpr int LDS = N * (int)sizeof(u64);
  if constexpr (LDS > 65536) {
    static bool attr = false;
    if (!attr) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&token_rank_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS) != hipSuccess)
        return case_set_error(CASE_E_LAUNCH, "case_token_rank: cannot reserve %d bytes of LDS", LDS);
      attr = true;
    }
  }
  hipLaunchKernelGGL(token_rank_kernel<N>, dim3((unsigned)B), dim3(RankShape<N>::THREADS), LDS, stream, scores, valid, labels, stats, counts,
                     threshold, (int)S);
  return case_check_launch("case_token_rank");
}

}  // namespace

extern "C" int case_token_rank(const float* scores, const uint8_t* valid, const float* labels, double* stats, int32_t* counts, float* threshold,
                               int64_t B, int64_t S, case_stream_t stream) {
  CASE_REQUIRE(B >= 0 && B < (1ll << 31) && S > 0, "case_token_rank: bad argument");
  if (S > RANK_MAX_S)
    return case_set_error(CASE_E_UNSUPPORTED, "case_token_rank: rows of up to %d positions (got %lld)", RANK_MAX_S, (long long)S);
  if (B == 0) return 0;
  CASE_REQUIRE(scores && labels && stats && counts && threshold, "case_token_rank: bad argument");
  hipStream_t s = (hipStream_t)stream;
#define TOKEN_RANK(N) \
  if (S <= N) return token_rank_launch<N>(scores, valid, labels, stats, counts, threshold, B, S, s)
  TOKEN_RANK(64);
  TOKEN_RANK(128);
  TOKEN_RANK(256);
  TOKEN_RANK(512);
  TOKEN_RANK(1024);
  TOKEN_RANK(2048);
  TOKEN_RANK(4096);
  TOKEN_RANK(8192);
  TOKEN_RANK(16384);
#undef TOKEN_RANK
  return case_set_error(CASE_E_UNSUPPORTED, "case_token_rank: rows of up to %d positions (got %lld)", RANK_MAX_S, (long long)S);
}
