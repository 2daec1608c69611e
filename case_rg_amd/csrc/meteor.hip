// METEOR on token ids (evaluation/meteor.py restated on ids; the reference's Eval_Meteor.py calls nltk's meteor_score).
//   K40 case_meteor  per (hypothesis, reference): the alignment (exact stage, then an optional class stage over one caller-provided table), the
//                    number of matches, of exact matches and of chunks, the score of the pair, and per hypothesis the best score over the
//                    present references
// Nothing here waits for the host, and the library keeps no state.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "case_hip.h"
#include "common.h"
#include "id_rows.h"

// ---- K40 -------------------------------------------------------------------------------------------------------------------------
// One wave per hypothesis (b, n), held as id_rows.h states (id_hold).
// The rule (evaluation/meteor.py) walks the hypothesis from its last position to its first and gives each position the LAST still-unmatched
// reference position that holds the same id.  Read per id, that pairs the k-th-from-last occurrence in the hypothesis with the k-th-from-last
// occurrence in the reference, so the transposed walk gives the same matches with wave-uniform state only: the reference is streamed
// BACKWARDS (id_stream_back); for the token t at position p,
//     M_j = __ballot(tok_j == t) & ~matched_j
// marks the unmatched hypothesis positions that hold t, the HIGHEST set bit over the words is p's partner, its bit goes into `matched` and
// its lane keeps p in `ref`.  The class stage is a second backward pass over what the first left: p was consumed by the exact stage exactly
// when some lane holds ref == p (a lane that the class stage matched holds a position behind p, which is visited once), and otherwise p
// takes the highest unmatched position whose class key equals its own.  A token without a class (an id outside [0, V) or a negative entry)
// has the key -1 in the hypothesis and is skipped in the reference.
// A chunk starts at a matched position i unless i - 1 is matched to ref[i] - 1: the neighbour's value comes by a lane shift, lane 63 of word
// j - 1 carries into lane 0 of word j.  Everything up to the score is integer; the score is f64 in a fixed order.
__device__ __forceinline__ double meteor_score_of(const int m, const int chunks, const int la, const int lb, const double alpha, const double beta,
                                                  const double gamma) {
#pragma clang fp contract(off)
  if (m <= 0) return 0.0;
  const double P = (double)m / (double)la, R = (double)m / (double)lb;
  const double fmean = P * R / (alpha * P + (1.0 - alpha) * R);
  const double pen = gamma * pow((double)chunks / (double)m, beta);
  return (1.0 - pen) * fmean;
}

// One reference position p with key t against the keys of the hypothesis: the highest unmatched position that holds t takes p.
template <int WORDS>
__device__ __forceinline__ void meteor_take(const int32_t (&key)[WORDS], const int t, const int p, const int lane, unsigned long long (&matched)[WORDS],
                                            int32_t (&ref)[WORDS]) {
  bool done = false;
#pragma unroll
  for (int j = WORDS - 1; j >= 0; --j) {
    const unsigned long long M = __ballot(key[j] == t) & ~matched[j];
    if (!done && M != 0ull) {  // (wave-uniform)
      const int bit = 63 - __builtin_clzll(M);
      matched[j] |= 1ull << bit;
      if (lane == bit) ref[j] = p;
      done = true;
    }
  }
}

template <int WORDS, bool CLASSES>
__global__ __launch_bounds__(64 * ID_WAVES) void meteor_kernel(const int64_t* __restrict__ a, const int32_t* __restrict__ a_len,
                                                               const int64_t* __restrict__ b, const int32_t* __restrict__ b_len,
                                                               const int32_t* __restrict__ classes, const int V, const double alpha,
                                                               const double beta, const double gamma, int32_t* __restrict__ counts,
                                                               float* __restrict__ pair, double* __restrict__ best_out,
                                                               int32_t* __restrict__ best_ref_out, int32_t* __restrict__ align, const int64_t BN,
                                                               const int N, const int M, const int Ta, const int Tb) {
  const int lane = threadIdx.x & 63;
  const int64_t h = id_wave_row();
  if (h >= BN) return;
  const int64_t item = h / N;
  const int la = id_clamp(a_len[h], Ta);
  int32_t tok[WORDS], cls[WORDS];
  id_hold<WORDS>(a + h * Ta, 0, la, lane, tok);
  const auto class_of = [&](const int id) { return CLASSES && id >= 0 && id < V ? classes[id] : -1; };  // (an id without a class: negative)
#pragma unroll
  for (int j = 0; j < WORDS; ++j) {
    const int c = class_of(tok[j]);
    cls[j] = c < 0 ? -1 : c;
  }
  double best = 0.0;
  int best_ref = -1;
  for (int m = 0; m < M; ++m) {
    const int64_t r = item * M + m;
    const int lb = id_clamp(b_len[r], Tb);
    const int64_t* __restrict__ row = b + r * Tb;
    unsigned long long matched[WORDS];
    int32_t ref[WORDS];
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
      matched[j] = 0ull;
      ref[j] = -1;
    }
    int exact = 0, total = 0, chunks = 0;
    if (la > 0 && lb > 0) {
      // the exact stage
      id_stream_back(row, lb, lane, [](const int id) { return id; }, [&](const int t, const int p) {
        if (t >= 0) meteor_take<WORDS>(tok, t, p, lane, matched, ref);  // (a negative id is no token: it must not meet the sentinel)
      });
#pragma unroll
      for (int j = 0; j < WORDS; ++j) exact += __popcll(matched[j]);
      total = exact;
      if (CLASSES) {
        id_stream_back(row, lb, lane, class_of, [&](const int c, const int p) {
          if (c < 0) return;  // (uniform)
          unsigned long long taken = 0ull;
#pragma unroll
          for (int j = 0; j < WORDS; ++j) taken |= __ballot(ref[j] == p);
          if (taken == 0ull) meteor_take<WORDS>(cls, c, p, lane, matched, ref);
        });
        total = 0;
#pragma unroll
        for (int j = 0; j < WORDS; ++j) total += __popcll(matched[j]);
      }
#pragma unroll
      for (int j = 0; j < WORDS; ++j) {
        int before = __shfl_up(ref[j], 1, 64);
        const int carry = j > 0 ? __shfl(ref[j > 0 ? j - 1 : 0], 63, 64) : -1;
        if (lane == 0) before = carry;
        chunks += __popcll(__ballot(ref[j] >= 0 && !(before >= 0 && before + 1 == ref[j])));
      }
    }
    const double score = lb > 0 ? meteor_score_of(total, chunks, la, lb, alpha, beta, gamma) : 0.0;
    if (lb > 0 && (best_ref < 0 || score > best)) {  // (the lowest index among equals)
      best = score;
      best_ref = m;
    }
    if (lane == 0) {
      int32_t* __restrict__ out = counts + (h * M + m) * 3;
      out[0] = total;
      out[1] = exact;
      out[2] = chunks;
      pair[h * M + m] = (float)score;
    }
    if (align) {
#pragma unroll
      for (int j = 0; j < WORDS; ++j) {
        const int pos = lane + 64 * j;
        if (pos < Ta) align[(h * M + m) * Ta + pos] = ref[j];
      }
    }
  }
  if (lane == 0) {
    best_out[h] = best;
    best_ref_out[h] = best_ref;
  }
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
extern "C" int case_meteor(const int64_t* a, const int32_t* a_len, const int64_t* b, const int32_t* b_len, const int32_t* classes, int64_t V,
                           double alpha, double beta, double gamma, int32_t* counts, float* meteor_pair, double* meteor, int32_t* best_ref,
                           int32_t* align, int64_t B, int64_t N, int64_t M, int64_t Ta, int64_t Tb, case_stream_t stream) {
  CASE_REQUIRE(a && a_len && b && b_len && counts && meteor_pair && meteor && best_ref && id_pairs_in_range(B, N, M, Ta, Tb),
               "case_meteor: bad argument");
  CASE_REQUIRE(classes ? (V > 0 && V < (1ll << 31)) : V == 0, "case_meteor: a class table of V = %lld entries (0 without a table)", (long long)V);
  CASE_REQUIRE(alpha >= 0.0 && alpha <= 1.0 && gamma >= 0.0 && gamma <= 1.0 && beta >= 0.0 && isfinite(beta),
               "case_meteor: alpha and gamma in [0, 1], beta >= 0 and finite (got %g, %g, %g)", alpha, beta, gamma);
  if (Ta > ID_MAX_T)
    return case_set_error(CASE_E_UNSUPPORTED, "case_meteor: hypotheses of up to %d positions (got %lld)", ID_MAX_T, (long long)Ta);
  const int64_t BN = B * N;
  id_dispatch_words(BN, Ta, [&](auto words, const dim3 grid, const dim3 block) {
    const auto launch = [&](auto with_classes) {
      hipLaunchKernelGGL((meteor_kernel<decltype(words)::value, decltype(with_classes)::value>), grid, block, 0, (hipStream_t)stream, a, a_len, b,
                         b_len, classes, (int)V, alpha, beta, gamma, counts, meteor_pair, meteor, best_ref, align, BN, (int)N, (int)M, (int)Ta,
                         (int)Tb);
    };
    if (classes)
      launch(std::true_type());
    else
      launch(std::false_type());
  });
  return case_check_launch("case_meteor");
}
