// BLEU and n-gram overlap on token ids (evaluation/bleu.py restated on ids; the reference's Eval_Bleu.py / Eval_Overlap.py).
//   K34 case_ngram_counts  per (hypothesis, reference) and per order k = 1..4: the clipped k-gram matches, the number of distinct hypothesis
//                          k-grams that occur in the reference, and both against all present references at once; exact integers
//   K35 case_bleu_scores   the counts -> sentence BLEU of every pair and against all present references (f64, fixed order)
// and ROUGE-N, the set measure of the reference's Rouge.py rouge_n, from K34's hit / distinct and
//   K43 case_ngram_distinct  the distinct k-grams of a row of any length (the reference side of ROUGE-N), k = 1..4; exact integers
//   K44 case_rouge_n_scores  the counts -> F of every pair and F / P / R against the best present reference (f64, fixed order)
// Nothing here waits for the host, and the library keeps no state.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "case_hip.h"
#include "common.h"
#include "id_rows.h"

constexpr int NGRAM_ORDERS = 4;

// ---- K34 -------------------------------------------------------------------------------------------------------------------------
// One wave per hypothesis (b, n), held as id_rows.h states (id_hold).  For a token t at position p of some sequence s,
// M(p) = __ballot(tok == t)  marks the hypothesis positions that hold t, and
//     D_1(p) = M(p),   D_k(p) = M(p) & (D_{k-1}(p - 1) << 1)        (the shift carries bit 63 of word j into bit 0 of word j + 1)
// has bit i set exactly when the k-gram of the hypothesis that ENDS at i equals the k-gram of s that ends at p.  The D_k are wave-uniform and
// live from one token to the next (and from one 64-token load of s to the next); lane i adds its own bit of D_k(p) to a counter, which
// after the last token is the number of times the k-gram ending at i occurs in s.  A bit below k - 1 or from a_len on is never set.
//   s = the hypothesis itself gives c_hyp; a set bit with p < i says "this k-gram occurred earlier", and every lane but the one at the first
//   occurrence then drops its count to 0, so a distinct k-gram is counted once.
//   s = reference m gives c_ref:  clip = sum over the lanes of min(c_hyp, c_ref),  hit = the number of lanes with both > 0;  the per-lane
//   maximum of c_ref over the present references gives clip_any / hit_any after the last one.
struct NgramMasks {
  unsigned long long d[NGRAM_ORDERS - 1];  // D_1 .. D_3 of the previous position, one word
};

// The lane's own bit of a wave-uniform mask: the mask is used as a lane condition directly (one v_cndmask), no 64-bit shift per lane.
__device__ __forceinline__ int ngram_own_bit(const unsigned long long d) { return __builtin_amdgcn_inverse_ballot_w64(d) ? 1 : 0; }

// One token: the orders go downwards, so that D_k(p) is built from D_{k-1}(p - 1) before that is overwritten; use(k - 1, j, word j of D_k(p)).
template <int WORDS, typename Use>
__device__ __forceinline__ void ngram_step(const int32_t (&tok)[WORDS], const int t, NgramMasks (&prev)[WORDS], Use use) {
  unsigned long long match[WORDS];
#pragma unroll
  for (int j = 0; j < WORDS; ++j) match[j] = __ballot(tok[j] == t);
#pragma unroll
  for (int k = NGRAM_ORDERS - 1; k > 0; --k)
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
      const unsigned long long below = j > 0 ? prev[j - 1].d[k - 1] >> 63 : 0ull;
      const unsigned long long d = match[j] & ((prev[j].d[k - 1] << 1) | below);
      use(k, j, d);
      if (k + 1 < NGRAM_ORDERS) prev[j].d[k] = d;
    }
#pragma unroll
  for (int j = 0; j < WORDS; ++j) {
    use(0, j, match[j]);
    prev[j].d[0] = match[j];
  }
}

__device__ __forceinline__ int ngram_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the wave of min(c_hyp, c) per order (each at most 256: two orders share one 32-bit sum) and the count of lanes with both > 0
template <int WORDS>
__device__ __forceinline__ void ngram_totals(const int (&c_hyp)[NGRAM_ORDERS][WORDS], const int (&c)[NGRAM_ORDERS][WORDS], int (&clip)[NGRAM_ORDERS],
                                             int (&hit)[NGRAM_ORDERS]) {
  int part[NGRAM_ORDERS];
#pragma unroll
  for (int k = 0; k < NGRAM_ORDERS; ++k) {
    part[k] = 0;
    hit[k] = 0;
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
      part[k] += c_hyp[k][j] < c[k][j] ? c_hyp[k][j] : c[k][j];
      hit[k] += __popcll(__ballot(c_hyp[k][j] > 0 && c[k][j] > 0));
    }
  }
  const int lo = ngram_wave_sum(part[0] | (part[1] << 16)), hi = ngram_wave_sum(part[2] | (part[3] << 16));
  clip[0] = lo & 0xffff;
  clip[1] = lo >> 16;
  clip[2] = hi & 0xffff;
  clip[3] = hi >> 16;
}

__device__ __forceinline__ void ngram_store(int32_t* __restrict__ out, const int (&v)[NGRAM_ORDERS]) {
#pragma unroll
  for (int k = 0; k < NGRAM_ORDERS; ++k) out[k] = v[k];
}

template <int WORDS>
__global__ __launch_bounds__(64 * ID_WAVES) void ngram_counts_kernel(const int64_t* __restrict__ a, const int32_t* __restrict__ a_len,
                                                                    const int64_t* __restrict__ b, const int32_t* __restrict__ b_len,
                                                                    int32_t* __restrict__ clip, int32_t* __restrict__ clip_any,
                                                                    int32_t* __restrict__ hit, int32_t* __restrict__ hit_any,
                                                                    int32_t* __restrict__ distinct, const int64_t BN, const int N, const int M,
                                                                    const int Ta, const int Tb, const int max_n) {
  const int lane = threadIdx.x & 63;
  const int64_t h = id_wave_row();
  if (h >= BN) return;
  const int64_t item = h / N;
  const int la = id_clamp(a_len[h], Ta);
  int32_t tok[WORDS];
  id_hold<WORDS>(a + h * Ta, 0, la, lane, tok);
  NgramMasks prev[WORDS];
  int c_hyp[NGRAM_ORDERS][WORDS], c_ref[NGRAM_ORDERS][WORDS], c_max[NGRAM_ORDERS][WORDS], earlier[NGRAM_ORDERS][WORDS];
#pragma unroll
  for (int j = 0; j < WORDS; ++j) {
#pragma unroll
    for (int k = 0; k + 1 < NGRAM_ORDERS; ++k) prev[j].d[k] = 0ull;
#pragma unroll
    for (int k = 0; k < NGRAM_ORDERS; ++k) c_hyp[k][j] = c_max[k][j] = earlier[k][j] = 0;
  }
  // the hypothesis against itself
  id_stream_held<WORDS>(tok, la, [&](const int t, const int p) {
    ngram_step<WORDS>(tok, t, prev, [&](const int k, const int j, const unsigned long long d) {
      const int bit = ngram_own_bit(d);
      c_hyp[k][j] += bit;
      earlier[k][j] |= p < lane + 64 * j ? bit : 0;
    });
  });
  int total[NGRAM_ORDERS];
#pragma unroll
  for (int k = 0; k < NGRAM_ORDERS; ++k) {
    total[k] = 0;
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
      if (earlier[k][j] || k >= max_n) c_hyp[k][j] = 0;
      total[k] += __popcll(__ballot(c_hyp[k][j] > 0));
    }
  }
  if (lane == 0) ngram_store(distinct + h * NGRAM_ORDERS, total);

  int got_clip[NGRAM_ORDERS], got_hit[NGRAM_ORDERS];
  for (int m = 0; m < M; ++m) {
    const int64_t r = item * M + m;
    const int lb = id_clamp(b_len[r], Tb);
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
#pragma unroll
      for (int k = 0; k + 1 < NGRAM_ORDERS; ++k) prev[j].d[k] = 0ull;
#pragma unroll
      for (int k = 0; k < NGRAM_ORDERS; ++k) c_ref[k][j] = 0;
    }
    if (la > 0)
      id_stream(b + r * Tb, lb, lane, [&](const int t, int) {  // (prev carries D_k(p - 1) from one position, and one load, to the next)
        ngram_step<WORDS>(tok, t, prev, [&](const int k, const int j, const unsigned long long d) { c_ref[k][j] += ngram_own_bit(d); });
      });
    ngram_totals<WORDS>(c_hyp, c_ref, got_clip, got_hit);
#pragma unroll
    for (int k = 0; k < NGRAM_ORDERS; ++k)
#pragma unroll
      for (int j = 0; j < WORDS; ++j) c_max[k][j] = c_ref[k][j] > c_max[k][j] ? c_ref[k][j] : c_max[k][j];
    if (lane == 0) {
      ngram_store(clip + (h * M + m) * NGRAM_ORDERS, got_clip);
      ngram_store(hit + (h * M + m) * NGRAM_ORDERS, got_hit);
    }
  }
  ngram_totals<WORDS>(c_hyp, c_max, got_clip, got_hit);
  if (lane == 0) {
    ngram_store(clip_any + h * NGRAM_ORDERS, got_clip);
    ngram_store(hit_any + h * NGRAM_ORDERS, got_hit);
  }
}

// ---- K35 -------------------------------------------------------------------------------------------------------------------------
// nltk's sentence_bleu with uniform weights over the orders 1..max_n (evaluation/bleu.py sentence_bleu, in its order): p_k = clip_k / max(1, la - k + 1),
// add1: (clip_k + 1) / (max(1, la - k + 1) + 1) for k >= 2;  score = BP exp(sum_k ln p_k / max_n),  BP = 1 if la > r else exp(1 - r / la);
// 0 when a precision it takes the logarithm of is 0 (none: any order; add1: the first), and without a present reference.
__device__ __forceinline__ double bleu_of(const int32_t* __restrict__ clip, const int la, const int r, const int max_n, const int smoothing, double* bp_out) {
#pragma clang fp contract(off)
  double bp = 0.0;
  if (la > 0 && r > 0) bp = la > r ? 1.0 : exp(1.0 - (double)r / (double)la);
  if (bp_out) *bp_out = bp;
  if (la <= 0 || r <= 0) return 0.0;
  double s = 0.0;
  for (int k = 0; k < max_n; ++k) {
    int num = clip[k], den = la - k > 1 ? la - k : 1;
    if (smoothing == 1 && k > 0) {
      num += 1;
      den += 1;
    }
    if (num <= 0) return 0.0;
    s += log((double)num / (double)den);
  }
  return bp * exp(s / (double)max_n);
}

// One thread per (hypothesis (b, n), m): m < M is the pair score against reference m; m == M is the score against all present references
// (r = the present length closest to la, the shorter one on a tie).
__global__ __launch_bounds__(256) void bleu_scores_kernel(const int32_t* __restrict__ clip, const int32_t* __restrict__ clip_any,
                                                          const int32_t* __restrict__ a_len, const int32_t* __restrict__ b_len,
                                                          float* __restrict__ bleu_pair, double* __restrict__ bleu_any, double* __restrict__ bp,
                                                          const int64_t total, const int N, const int M, const int max_n, const int smoothing) {
  const int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (at >= total) return;
  const int64_t h = at / (M + 1);
  const int m = (int)(at - h * (M + 1));
  const int64_t item = h / N;
  const int la = a_len[h] < 0 ? 0 : a_len[h];  // (no Ta here: the caller keeps the lengths within K34's 0 .. Ta / Tb, see case_hip.h)
  if (m < M) {
    bleu_pair[h * M + m] = (float)bleu_of(clip + (h * M + m) * NGRAM_ORDERS, la, b_len[item * M + m], max_n, smoothing, nullptr);
    return;
  }
  int best = 0, gap = 0;
  for (int i = 0; i < M; ++i) {
    const int lb = b_len[item * M + i];
    if (lb <= 0) continue;
    const int d = lb > la ? lb - la : la - lb;
    if (best == 0 || d < gap || (d == gap && lb < best)) {
      best = lb;
      gap = d;
    }
  }
  double item_bp;
  bleu_any[h] = bleu_of(clip_any + h * NGRAM_ORDERS, la, best, max_n, smoothing, &item_bp);
  if (bp) bp[h] = item_bp;
}

// ---- K43 -------------------------------------------------------------------------------------------------------------------------
// The distinct k-grams of a row of any length (ROUGE-N's |R|): K34's self-pass over a row that does not fit 64 WORDS positions.  One wave per
// row.  A WINDOW of 64 WORDS positions starting at s is held as id_rows.h states (id_hold with first = s), and the row is streamed from
// position 0 to the window's end through ngram_step: a set bit of D_k(p) with
// p below the bit's own position says "the k-gram that ends here ended at p already", and that position drops out (the masks are
// wave-uniform, so D_k, the "behind p" masks and the dropped-out sets all live in scalar registers).  What is left is counted.
// The seam: the D_k recurrence never sets a bit below k - 1 of a window, because that k-gram starts in the window before.  So consecutive
// windows overlap by NGRAM_ORDERS - 1 = 3 positions (stride 64 WORDS - 3) and every window but the first counts its positions from 3 on: each
// position of the row is counted in exactly one window, and there with its whole k-gram inside the window.  In the first window the
// recurrence itself keeps order k from counting the positions below k - 1 of the row.
// A row of L ids takes about L^2 / (2 (64 WORDS - 3)) token steps: quadratic, with the small constant of wave-wide mask arithmetic.
constexpr int NGRAM_SEAM = NGRAM_ORDERS - 1;

template <int WORDS>
__global__ __launch_bounds__(64 * ID_WAVES) void ngram_distinct_kernel(const int64_t* __restrict__ b, const int32_t* __restrict__ b_len,
                                                                      int32_t* __restrict__ distinct, const int64_t rows, const int Tb,
                                                                      const int max_n) {
  constexpr int STRIDE = 64 * WORDS - NGRAM_SEAM;
  const int lane = threadIdx.x & 63;
  const int64_t r = id_wave_row();
  if (r >= rows) return;
  const int len = id_clamp(b_len[r], Tb);
  const int64_t* __restrict__ row = b + r * Tb;
  int total[NGRAM_ORDERS];
#pragma unroll
  for (int k = 0; k < NGRAM_ORDERS; ++k) total[k] = 0;
  int s = 0;
  do {
    const int first = s > 0 ? NGRAM_SEAM : 0;                       // the window's first counted position
    const int end = len - s < 64 * WORDS ? len : s + 64 * WORDS;  // one past the last position of the row that the window holds
    int32_t tok[WORDS];
    NgramMasks prev[WORDS];
    unsigned long long earlier[NGRAM_ORDERS][WORDS];  // (wave-uniform like the D_k: the whole self-pass stays in scalar registers)
    id_hold<WORDS>(row, s, end, lane, tok);
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
#pragma unroll
      for (int k = 0; k + 1 < NGRAM_ORDERS; ++k) prev[j].d[k] = 0ull;
#pragma unroll
      for (int k = 0; k < NGRAM_ORDERS; ++k) earlier[k][j] = 0ull;
    }
    id_stream(row, end, lane, [&](const int t, const int at) {  // (prev carries D_k(p - 1) from one position, and one load, to the next)
      const int p = at - s;  // the stream's position seen from the window: negative before it
      unsigned long long above[WORDS];  // the positions of word j that lie behind p
#pragma unroll
      for (int j = 0; j < WORDS; ++j) {
        const int q = p - 64 * j;
        above[j] = q < 0 ? ~0ull : q >= 63 ? 0ull : ~0ull << (q + 1);
      }
      ngram_step<WORDS>(tok, t, prev, [&](const int k, const int j, const unsigned long long d) { earlier[k][j] |= d & above[j]; });
    });
#pragma unroll
    for (int k = 0; k < NGRAM_ORDERS; ++k)
#pragma unroll
      for (int j = 0; j < WORDS; ++j) {
        const int at = lane + 64 * j;
        total[k] += __popcll(__ballot(at >= first && at >= k && s + at < end) & ~earlier[k][j]);
      }
    s += STRIDE;
  } while (s + NGRAM_SEAM < len);
  if (lane < NGRAM_ORDERS) {
    int mine = 0;
#pragma unroll
    for (int k = 0; k < NGRAM_ORDERS; ++k) mine = lane == k && k < max_n ? total[k] : mine;
    distinct[r * NGRAM_ORDERS + lane] = mine;
  }
}

// ---- K44 -------------------------------------------------------------------------------------------------------------------------
// The reference's rouge_n (evaluation/rouge.py rouge_n, in its order) from the counts: o = hit, P = o / |E|, R = o / |R| (0.0 where the
// denominator is 0), F = 2.0 * ((P * R) / (P + R + 1e-8)).  One thread per (hypothesis (b, n), order k): the pair F of every present reference
// (f32, rounded once) and the values against the one with the largest F, the lowest index among equals.
__global__ __launch_bounds__(256) void rouge_n_scores_kernel(const int32_t* __restrict__ hit, const int32_t* __restrict__ hyp_distinct,
                                                             const int32_t* __restrict__ ref_distinct, const int32_t* __restrict__ b_len,
                                                             float* __restrict__ f_pair, double* __restrict__ f, double* __restrict__ p,
                                                             double* __restrict__ r, int32_t* __restrict__ best_ref, const int64_t total,
                                                             const int N, const int M, const int max_n) {
#pragma clang fp contract(off)
  const int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (at >= total) return;
  const int64_t h = at / NGRAM_ORDERS;
  const int k = (int)(at - h * NGRAM_ORDERS);
  const int64_t item = h / N;
  const int e = hyp_distinct[at];
  double best_f = 0.0, best_p = 0.0, best_r = 0.0;
  int best = -1;
  for (int m = 0; m < M; ++m) {
    const int64_t pair = (h * M + m) * NGRAM_ORDERS + k;
    if (k >= max_n || b_len[item * M + m] <= 0) {
      f_pair[pair] = 0.0f;
      continue;
    }
    const int o = hit[pair], d = ref_distinct[(item * M + m) * NGRAM_ORDERS + k];
    const double pm = e == 0 ? 0.0 : (double)o / (double)e;
    const double rm = d == 0 ? 0.0 : (double)o / (double)d;
    const double fm = 2.0 * ((pm * rm) / (pm + rm + 1e-8));
    f_pair[pair] = (float)fm;
    if (best < 0 || fm > best_f) {
      best = m;
      best_f = fm;
      best_p = pm;
      best_r = rm;
    }
  }
  f[at] = best_f;
  p[at] = best_p;
  r[at] = best_r;
  best_ref[at] = best;
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
extern "C" int case_ngram_distinct(const int64_t* b, const int32_t* b_len, int32_t* distinct, int64_t rows, int64_t Tb, int32_t max_n,
                                   case_stream_t stream) {
  CASE_REQUIRE(b && b_len && distinct && rows > 0 && Tb > 0 && rows < (1ll << 31) && Tb < (1ll << 30) && max_n >= 1 && max_n <= NGRAM_ORDERS,
               "case_ngram_distinct: bad argument");
  id_dispatch_words(rows, Tb, [&](auto words, const dim3 grid, const dim3 block) {
    hipLaunchKernelGGL(ngram_distinct_kernel<decltype(words)::value>, grid, block, 0, (hipStream_t)stream, b, b_len, distinct, rows, (int)Tb,
                       (int)max_n);
  });
  return case_check_launch("case_ngram_distinct");
}

extern "C" int case_rouge_n_scores(const int32_t* hit, const int32_t* hyp_distinct, const int32_t* ref_distinct, const int32_t* b_len,
                                   float* f_pair, double* f, double* p, double* r, int32_t* best_ref, int64_t B, int64_t N, int64_t M,
                                   int32_t max_n, case_stream_t stream) {
  CASE_REQUIRE(hit && hyp_distinct && ref_distinct && b_len && f_pair && f && p && r && best_ref && id_pairs_in_range(B, N, M) &&
                   B * N * M < (1ll << 37) && max_n >= 1 && max_n <= NGRAM_ORDERS,
               "case_rouge_n_scores: bad argument");
  const int64_t total = B * N * NGRAM_ORDERS;
  hipLaunchKernelGGL(rouge_n_scores_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, hit, hyp_distinct,
                     ref_distinct, b_len, f_pair, f, p, r, best_ref, total, (int)N, (int)M, (int)max_n);
  return case_check_launch("case_rouge_n_scores");
}

extern "C" int case_ngram_counts(const int64_t* a, const int32_t* a_len, const int64_t* b, const int32_t* b_len, int32_t* clip, int32_t* clip_any,
                                 int32_t* hit, int32_t* hit_any, int32_t* distinct, int64_t B, int64_t N, int64_t M, int64_t Ta, int64_t Tb,
                                 int32_t max_n, case_stream_t stream) {
  CASE_REQUIRE(a && a_len && b && b_len && clip && clip_any && hit && hit_any && distinct && id_pairs_in_range(B, N, M, Ta, Tb) && max_n >= 1 &&
                   max_n <= NGRAM_ORDERS,
               "case_ngram_counts: bad argument");
  if (Ta > ID_MAX_T)
    return case_set_error(CASE_E_UNSUPPORTED, "case_ngram_counts: hypotheses of up to %d positions (got %lld)", ID_MAX_T, (long long)Ta);
  const int64_t BN = B * N;
  id_dispatch_words(BN, Ta, [&](auto words, const dim3 grid, const dim3 block) {
    hipLaunchKernelGGL(ngram_counts_kernel<decltype(words)::value>, grid, block, 0, (hipStream_t)stream, a, a_len, b, b_len, clip, clip_any, hit,
                       hit_any, distinct, BN, (int)N, (int)M, (int)Ta, (int)Tb, (int)max_n);
  });
  return case_check_launch("case_ngram_counts");
}

extern "C" int case_bleu_scores(const int32_t* clip, const int32_t* clip_any, const int32_t* a_len, const int32_t* b_len, float* bleu_pair,
                                double* bleu_any, double* bp, int64_t B, int64_t N, int64_t M, int32_t max_n, int32_t smoothing,
                                case_stream_t stream) {
  CASE_REQUIRE(clip && clip_any && a_len && b_len && bleu_pair && bleu_any && id_pairs_in_range(B, N, M) && B * N * (M + 1) < (1ll << 39) &&
                   max_n >= 1 && max_n <= NGRAM_ORDERS && (smoothing == 0 || smoothing == 1),
               "case_bleu_scores: bad argument");
  const int64_t total = B * N * (M + 1);
  hipLaunchKernelGGL(bleu_scores_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, clip, clip_any, a_len, b_len,
                     bleu_pair, bleu_any, bp, total, (int)N, (int)M, (int)max_n, (int)smoothing);
  return case_check_launch("case_bleu_scores");
}
