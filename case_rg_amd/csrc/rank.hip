// TREC ranking metrics of score rows (evaluation/trec.py restated on tensors; the reference's Eval_Trec.py asks pytrec_eval for them).
//   K36 case_rank_metrics  per query: the rank order of its retrieved documents and map, ndcg, recall@k, recip_rank, P_1 (f64)
// Nothing here waits for the host, and the library keeps no state.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "case_hip.h"
#include "common.h"

constexpr int RANK_MAX_P = 1024;       // retrieved documents per query
constexpr int RANK_MAX_JUDGED = 2048;  // retrieved + judged-but-unretrieved grades per query
constexpr int RANK_NUM_METRICS = 13;
__constant__ const int RANK_CUTOFFS[9] = {5, 10, 15, 20, 30, 100, 200, 500, 1000};

// ---- K36 -------------------------------------------------------------------------------------------------------------------------
// One workgroup per query; everything of the query lives in LDS.  A retrieved document is the pair
//     sk  = (the score as an order-preserving u32) << 32 | (the tie key with its sign bit flipped)      idx = its column
// and a comes before b when sk_a > sk_b, or sk_a == sk_b and idx_a < idx_b: score descending, the larger key first, then the lower column --
// a total order, so the bitonic network needs no stability.  The score map is the usual one (negative: all bits flipped, else the sign bit
// set) after -0.0 -> +0.0 and NaN -> -inf; -inf maps to 0x007fffff, so every retrieved document has sk > 0 and sk = 0 marks a slot that is not
// retrieved (invalid, or padding up to the power of two): those sort behind every retrieved one.
__device__ __forceinline__ uint32_t rank_score_bits(const float x) {
  uint32_t u = __float_as_uint(x);
  if (x != x) u = 0xff800000u;  // NaN compares as -inf
  if (x == 0.f) u = 0u;         // -0.0 == +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Bitonic network over n (a power of two) slots: ``first(i, l)`` says whether slot l's element belongs before slot i's (i < l).
template <int THREADS, typename First, typename Swap>
__device__ __forceinline__ void rank_bitonic(const int n, First first, Swap swap) {
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = threadIdx.x; p < (n >> 1); p += THREADS) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
        const bool forward = (i & k) == 0;  // this run is built in rank order, its neighbour reversed
        if (first(i, l) == forward) swap(i, l);
      }
      __syncthreads();
    }
}

// The sum of one f64 per thread through a tree of fixed shape (the same bits on every run); every thread gets it.
template <int THREADS>
__device__ __forceinline__ double rank_block_sum(const double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = THREADS >> 1; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void rank_metrics_kernel(const float* __restrict__ scores, const int32_t* __restrict__ keys,
                                                               const int32_t* __restrict__ rel, const uint8_t* __restrict__ valid,
                                                               const int32_t* __restrict__ extra_rel, int32_t* __restrict__ order,
                                                               double* __restrict__ metrics, int32_t* __restrict__ num_rel_out, const int P,
                                                               const int R, const int NP, const int NG) {
#pragma clang fp contract(off)
  constexpr int WAVES = THREADS / 64;
  constexpr int SLOTS = THREADS == 64 ? 64 : RANK_MAX_P;  // (the one-wave form serves P <= 64)
  __shared__ unsigned long long sk[SLOTS];
  __shared__ int idx[SLOTS];
  __shared__ int seen[SLOTS];               // relevant documents in the top r + 1
  __shared__ int grade[RANK_MAX_JUDGED];    // the gains of the ranked list, then the judged-but-unretrieved ones: sorted for IDCG
  __shared__ double red[THREADS];
  __shared__ int wave_count[WAVES];
  __shared__ int first_rel;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = blockIdx.x;
  const float* __restrict__ s_row = scores + q * P;
  const int32_t* __restrict__ rel_row = rel + q * P;

  for (int i = tid; i < NP; i += THREADS) {
    unsigned long long v = 0ull;
    if (i < P && (valid == nullptr || valid[q * P + i] != 0)) {
      const int key = keys ? keys[q * P + i] : i;
      v = ((unsigned long long)rank_score_bits(s_row[i]) << 32) | (unsigned long long)((uint32_t)key ^ 0x80000000u);
    }
    sk[i] = v;
    idx[i] = i;
  }
  if (tid == 0) first_rel = 0;
  __syncthreads();
  rank_bitonic<THREADS>(
      NP, [&](const int i, const int l) { return sk[l] > sk[i] || (sk[l] == sk[i] && idx[l] < idx[i]); },
      [&](const int i, const int l) {
        const unsigned long long a = sk[i];
        sk[i] = sk[l];
        sk[l] = a;
        const int b = idx[i];
        idx[i] = idx[l];
        idx[l] = b;
      });

  // the order, the gains, and the running count of relevant documents: a ballot prefix inside a wave, a carry across waves and chunks
  double ap = 0.0, dcg = 0.0;
  int carry = 0;
  for (int base = 0; base < NP; base += THREADS) {  // (NP is a multiple of THREADS or below it: whole waves reach the barriers)
    const int r = base + tid;
    int g = 0;
    if (r < P) {
      const bool retrieved = sk[r] != 0ull;
      const int col = idx[r];
      order[q * P + r] = retrieved ? col : -1;
      if (retrieved) g = rel_row[col];
      g = g > 0 ? g : 0;
    }
    if (r < P) grade[r] = g;
    const unsigned long long hits = __ballot(g >= 1);
    if (lane == 0) wave_count[wave] = __popcll(hits);
    __syncthreads();
    int before = carry, total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      before += w < wave ? wave_count[w] : 0;
      total += wave_count[w];
    }
    carry += total;
    const int upto = before + __popcll(hits & (~0ull >> (63 - lane)));
    if (r < P) seen[r] = upto;
    if (g >= 1) {
      if (upto == 1) first_rel = r + 1;  // (one thread of the workgroup)
      ap += (double)upto / (double)(r + 1);
      dcg += (double)g / log2((double)(r + 2));
    }
    __syncthreads();
  }
  // the judged but unretrieved grades behind the ranked ones, zeros up to the power of two
  int extra = 0;
  for (int i = P + tid; i < NG; i += THREADS) {
    int g = 0;
    if (i - P < R) g = extra_rel[q * R + (i - P)];
    g = g > 0 ? g : 0;
    grade[i] = g;
    extra += g >= 1;
  }
  const int num_rel = carry + (int)rank_block_sum<THREADS>((double)extra, red);
  ap = rank_block_sum<THREADS>(ap, red);
  dcg = rank_block_sum<THREADS>(dcg, red);
  rank_bitonic<THREADS>(
      NG, [&](const int i, const int l) { return grade[l] > grade[i]; },
      [&](const int i, const int l) {
        const int a = grade[i];
        grade[i] = grade[l];
        grade[l] = a;
      });
  double idcg = 0.0;
  for (int i = tid; i < NG; i += THREADS) {
    const int g = grade[i];
    if (g >= 1) idcg += (double)g / log2((double)(i + 2));
  }
  idcg = rank_block_sum<THREADS>(idcg, red);

  double* __restrict__ out = metrics + q * RANK_NUM_METRICS;
  if (tid == 0) {
    num_rel_out[q] = num_rel;
    out[0] = num_rel > 0 ? ap / (double)num_rel : 0.0;
    out[1] = num_rel > 0 ? dcg / idcg : 0.0;
    out[11] = first_rel > 0 ? 1.0 / (double)first_rel : 0.0;
    out[12] = seen[0] >= 1 ? 1.0 : 0.0;
  }
  if (tid < 9) {
    const int k = RANK_CUTOFFS[tid] < P ? RANK_CUTOFFS[tid] : P;  // (the slots behind the retrieved ones add nothing to the count)
    out[2 + tid] = num_rel > 0 ? (double)seen[k - 1] / (double)num_rel : 0.0;
  }
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
static int rank_pow2(const int64_t n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

extern "C" int case_rank_metrics(const float* scores, const int32_t* keys, const int32_t* rel, const uint8_t* valid, const int32_t* extra_rel,
                                 int32_t* order, double* metrics, int32_t* num_rel, int64_t B, int64_t P, int64_t R, case_stream_t stream) {
  CASE_REQUIRE(scores && rel && order && metrics && num_rel && B > 0 && B < (1ll << 31) && P > 0 && R >= 0 && (extra_rel || R == 0),
               "case_rank_metrics: bad argument");
  if (P > RANK_MAX_P || P + R > RANK_MAX_JUDGED)
    return case_set_error(CASE_E_UNSUPPORTED, "case_rank_metrics: up to %d retrieved and %d judged documents per query (got %lld and %lld)",
                          RANK_MAX_P, RANK_MAX_JUDGED, (long long)P, (long long)(P + R));
  const int NP = rank_pow2(P), NG = rank_pow2(P + R);  // the slots of the two sorts: NP <= 1024, NP <= NG <= 2048
  if (P <= 64)
    hipLaunchKernelGGL(rank_metrics_kernel<64>, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, scores, keys, rel, valid, extra_rel, order,
                       metrics, num_rel, (int)P, (int)R, NP, NG);
  else
    hipLaunchKernelGGL(rank_metrics_kernel<256>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, scores, keys, rel, valid, extra_rel,
                       order, metrics, num_rel, (int)P, (int)R, NP, NG);
  return case_check_launch("case_rank_metrics");
}
