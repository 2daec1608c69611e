// Consensus (minimum-Bayes-risk) answer selection over a pool of decoded candidates, and ROUGE-L on token ids.
//   K30 case_lcs_pairs       LCS length and ROUGE-L F of every (hypothesis, reference) pair of an item: the bit-parallel LCS recurrence on
//                            the wave's 64-bit match masks (evaluation/rouge.py lcs_length / rouge_l restated on ids)
//   K31 case_consensus_pick  the per-item expected utility of every candidate against the pool, its argmax and the picked row
// Nothing here waits for the host, and the library keeps no state.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "case_hip.h"
#include "common.h"
#include "id_rows.h"

constexpr int CONSENSUS_MAX_N = 64;

// ---- K30 -------------------------------------------------------------------------------------------------------------------------
// One wave per hypothesis (b, n), held as id_rows.h states (id_hold), so one __ballot of "my token == t" is the 64-bit match mask M_j of the
// reference token t.  With V all ones at the start, every reference token takes  V = (V + (V & M)) | (V & ~M)  (the addition carries from
// word j to word j + 1); the LCS length is the number of zero bits of V.  A sentinel bit has M = 0, so V & ~M sets it again whatever the
// carry did to it: no length mask.  V, M and the carry are wave-uniform 64-bit integers.  The reference row is streamed (id_stream).
template <int WORDS>
__global__ __launch_bounds__(64 * ID_WAVES) void lcs_pairs_kernel(const int64_t* __restrict__ a, const int32_t* __restrict__ a_len,
                                                                  const int64_t* __restrict__ b, const int32_t* __restrict__ b_len,
                                                                  int32_t* __restrict__ lcs, float* __restrict__ f, const int64_t BN, const int N,
                                                                  const int M, const int Ta, const int Tb) {
  const int lane = threadIdx.x & 63;
  const int64_t h = id_wave_row();
  if (h >= BN) return;
  const int64_t item = h / N;
  const int la = id_clamp(a_len[h], Ta);
  int32_t tok[WORDS];
  id_hold<WORDS>(a + h * Ta, 0, la, lane, tok);
  for (int m = 0; m < M; ++m) {
    const int64_t r = item * M + m;
    const int lb = id_clamp(b_len[r], Tb);
    unsigned long long V[WORDS];
#pragma unroll
    for (int j = 0; j < WORDS; ++j) V[j] = ~0ull;
    if (la > 0)
      id_stream(b + r * Tb, lb, lane, [&](const int t, int) {
        unsigned long long carry = 0;
#pragma unroll
        for (int j = 0; j < WORDS; ++j) {
          const unsigned long long Mj = __ballot(tok[j] == t);
          const unsigned long long Vj = V[j];
          const unsigned long long s1 = Vj + (Vj & Mj);
          const unsigned long long s2 = s1 + carry;
          carry = (s1 < Vj || s2 < s1) ? 1ull : 0ull;
          V[j] = s2 | (Vj & ~Mj);
        }
      });
    int len = 0;
#pragma unroll
    for (int j = 0; j < WORDS; ++j) len += __popcll(~V[j]);
    if (lane == 0) {
      // the host's F in f64, in its order (evaluation/rouge.py rouge_l), rounded once to f32
#pragma clang fp contract(off)
      double F = 0.0;
      if (la > 0 && lb > 0) {
        const double rr = (double)len / (double)lb, pp = (double)len / (double)la;
        const double beta = pp / (rr + 1e-12);
        F = (1.0 + beta * beta) * rr * pp / (rr + beta * beta * pp + 1e-12);
      } else {
        len = 0;
      }
      lcs[h * M + m] = len;
      f[h * M + m] = (float)F;
    }
  }
}

// ---- K31 -------------------------------------------------------------------------------------------------------------------------
// One wave per item.  Lane n < N: utility = sum_m w[m] f[n, m] / sum_m w[m] over the valid m in index order (f32; every lane adds in the same
// order, so equal rows of f give equal bits), -inf for an invalid n.  The argmax over the lanes prefers the lower index among equals
// (row_argmax's rule); an item without a valid candidate is all -inf and gets index 0.  Then the wave copies the picked row.
__global__ __launch_bounds__(64) void consensus_pick_kernel(const float* __restrict__ f, const float* __restrict__ w, const uint8_t* __restrict__ valid,
                                                            const int64_t* __restrict__ cand, float* __restrict__ utility,
                                                            int64_t* __restrict__ index, int64_t* __restrict__ answer, const int N, const int T) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const bool mine = lane < N && (!valid || valid[b * N + lane]);
  const float* __restrict__ frow = f + (b * N + (lane < N ? lane : 0)) * N;
  float num = 0.0f, den = 0.0f;
  for (int m = 0; m < N; ++m) {
    if (valid && !valid[b * N + m]) continue;  // (wave-uniform)
    const float wm = w ? w[b * N + m] : 1.0f;
    num += wm * frow[m];
    den += wm;
  }
  float u = mine ? (den > 0.0f ? num / den : 0.0f) : -INFINITY;
  if (lane < N) utility[b * N + lane] = u;
  int at = lane < N ? lane : CONSENSUS_MAX_N;
  if (!(u > -INFINITY)) u = -INFINITY;  // (a NaN utility never wins)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ou = __shfl_xor(u, off);
    const int oa = __shfl_xor(at, off);
    if (ou > u || (ou == u && oa < at)) {
      u = ou;
      at = oa;
    }
  }
  if (!(u > -INFINITY)) at = 0;
  if (lane == 0) index[b] = at;
  const int64_t* __restrict__ src = cand + (b * N + at) * T;
  for (int i = lane; i < T; i += 64) answer[b * T + i] = src[i];
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
extern "C" int case_lcs_pairs(const int64_t* a, const int32_t* a_len, const int64_t* b, const int32_t* b_len, int32_t* lcs, float* f, int64_t B,
                              int64_t N, int64_t M, int64_t Ta, int64_t Tb, case_stream_t stream) {
  CASE_REQUIRE(a && a_len && b && b_len && lcs && f && id_pairs_in_range(B, N, M, Ta, Tb), "case_lcs_pairs: bad argument");
  if (Ta > ID_MAX_T)
    return case_set_error(CASE_E_UNSUPPORTED, "case_lcs_pairs: hypotheses of up to %d positions (got %lld)", ID_MAX_T, (long long)Ta);
  const int64_t BN = B * N;
  id_dispatch_words(BN, Ta, [&](auto words, const dim3 grid, const dim3 block) {
    hipLaunchKernelGGL(lcs_pairs_kernel<decltype(words)::value>, grid, block, 0, (hipStream_t)stream, a, a_len, b, b_len, lcs, f, BN, (int)N,
                       (int)M, (int)Ta, (int)Tb);
  });
  return case_check_launch("case_lcs_pairs");
}

extern "C" int case_consensus_pick(const float* f, const float* w, const uint8_t* valid, const int64_t* cand, float* utility, int64_t* index,
                                   int64_t* answer, int64_t B, int64_t N, int64_t T, case_stream_t stream) {
  CASE_REQUIRE(f && cand && utility && index && answer && B > 0 && B < (1ll << 31) && N > 0 && T > 0 && T < (1ll << 30),
               "case_consensus_pick: bad argument");
  if (N > CONSENSUS_MAX_N)
    return case_set_error(CASE_E_UNSUPPORTED, "case_consensus_pick: pools of up to %d candidates (got %lld)", CONSENSUS_MAX_N, (long long)N);
  hipLaunchKernelGGL(consensus_pick_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, f, w, valid, cand, utility, index, answer, (int)N,
                     (int)T);
  return case_check_launch("case_consensus_pick");
}
