// The supporting-token stage outside the training loss: its supervision and the selection of its best tokens.
//   K37 case_token_labels  per passage row: which tokens occur in the answer and how much each one weighs (the reference's
//                          CaSEDataset.py token_label, restated in common/Utils.py token_label)
//   K38 case_token_select  per item: the K best positions of a row of keys in a total order, and the token-level counts of the row
// Nothing here waits for the host, no kernel uses an atomic, and the library keeps no state.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "case_hip.h"
#include "common.h"

constexpr int TOKEN_THREADS = 256;
constexpr int TOKEN_MAX_L = 16384;  // tokens per passage row (K37) and keys per item (K38)
constexpr int TOKEN_MAX_T = 1024;   // answer ids per item
constexpr int TOKEN_MAX_K = 256;    // selected positions per item

// The sum of one f64 per thread through a tree of fixed shape (rank.hip's rank_block_sum): the same bits on every run; every thread gets it.
__device__ __forceinline__ double token_block_sum(const double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = TOKEN_THREADS >> 1; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// ---- K37 -------------------------------------------------------------------------------------------------------------------------
// One workgroup per passage row.  The item's answer ids sit in LDS as int32 (PAD and the slots up to a multiple of four hold -1, which no
// passage id equals); every position scans them with 16-byte broadcast reads -- L 384 x T 80 is 30 k compares, so nothing is sorted -- and
// leaves its membership flag in LDS with two zero flags on either side of the row: a window never leaves the array.  The window counts
// come from the flags and ids of the neighbours: a member counts when no earlier slot of the window holds the same id.
template <typename F>
__device__ __forceinline__ double token_log_freq(const F* __restrict__ freq, const int64_t nfreq, const int64_t id) {
  const double f = (id >= 0 && id < nfreq) ? (double)freq[id] : 0.0;
  return log(f + 2.0);
}

template <typename F>
__global__ __launch_bounds__(TOKEN_THREADS) void token_labels_kernel(const int64_t* __restrict__ passage, const int64_t* __restrict__ response,
                                                                     const F* __restrict__ freq, float* __restrict__ label,
                                                                     float* __restrict__ weight, const int P, const int L, const int T,
                                                                     const int64_t nfreq, const int64_t pad) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) int answer[TOKEN_MAX_T];
  __shared__ uint8_t member[TOKEN_MAX_L + 4];
  __shared__ double red[TOKEN_THREADS];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x, item = row / P;
  const int64_t* __restrict__ x = passage + row * L;
  const int64_t* __restrict__ y = response + item * T;
  const int T4 = (T + 3) & ~3;

  for (int t = tid; t < T4; t += TOKEN_THREADS) {
    const int64_t id = t < T ? y[t] : pad;
    answer[t] = (id == pad || id < 0 || id > 0x7fffffffll) ? -1 : (int)id;
  }
  if (tid < 2) {
    member[tid] = 0;
    member[L + 2 + tid] = 0;
  }
  __syncthreads();

  double part = 0.0;  // this thread's positions in ascending order, then the tree: a fixed order of additions
  for (int i = tid; i < L; i += TOKEN_THREADS) {
    const int64_t id = x[i];
    part += token_log_freq(freq, nfreq, id);
    bool hit = false;
    if (id != pad && id >= 0 && id <= 0x7fffffffll) {
      const int v = (int)id;
      for (int t = 0; t < T4; t += 4) {
        const int4 a = *reinterpret_cast<const int4*>(&answer[t]);  // one address for the wave: a broadcast
        hit |= (a.x == v) | (a.y == v) | (a.z == v) | (a.w == v);
      }
    }
    member[i + 2] = hit ? 1 : 0;
  }
  const double total = token_block_sum(part, red);  // (its barriers also publish the flags)

  for (int i = tid; i < L; i += TOKEN_THREADS) {
    const bool g1 = member[i + 2] != 0;
    float w = 1.f;
    if (g1) {
      int64_t id[5];
      bool in[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int p = i + j - 2;
        id[j] = (p >= 0 && p < L) ? x[p] : pad;
        in[j] = member[p + 2] != 0;
      }
      int g3 = 0, g5 = 0;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        bool first5 = in[j], first3 = in[j] && j >= 1 && j <= 3;
#pragma unroll
        for (int k = 0; k < j; ++k) {
          const bool same = id[k] == id[j];
          first5 = first5 && !same;
          first3 = first3 && !(same && k >= 1);
        }
        g5 += first5;
        g3 += first3;
      }
      const double lf = token_log_freq(freq, nfreq, id[2]);
      w = (float)pow(total / lf * (double)g3 * (double)g5, 0.2);
    }
    label[row * L + i] = g1 ? 1.f : 0.f;
    weight[row * L + i] = w;
  }
}

// ---- K38 -------------------------------------------------------------------------------------------------------------------------
// One workgroup per item.  Thread t holds the keys of positions t, t + 256, ... in registers as K36's order-preserving u32 (0 = invalid or
// already taken: every valid key is at least 0x007fffff), and the best one it still holds as
//     (key << 32) | (0xffffffff - position)
// so that the larger u64 is the better token: value descending, then the lower position.  A round takes the maximum over the workgroup
// (shuffles inside a wave, one LDS word per wave, alternating between two sets so that one barrier per round is enough); its owner writes
// the slot, clears the key and looks through its own keys again.  K rounds, or fewer when nothing valid is left.
__device__ __forceinline__ uint32_t token_score_bits(const float x) {  // rank.hip's rank_score_bits
  uint32_t u = __float_as_uint(x);
  if (x != x) u = 0xff800000u;  // NaN compares as -inf
  if (x == 0.f) u = 0u;         // -0.0 == +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long token_wave_max(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64), lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    v = other > v ? other : v;
  }
  return v;
}

__device__ __forceinline__ int token_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int PER>
__device__ __forceinline__ unsigned long long token_local_best(const uint32_t (&key)[PER]) {
  uint32_t best = 0;
  int at = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j)
    if (key[j] > best) {  // (strictly: the lowest position among equal keys)
      best = key[j];
      at = j;
    }
  const uint32_t position = (uint32_t)(at * TOKEN_THREADS + (int)threadIdx.x);
  return best ? ((unsigned long long)best << 32) | (0xffffffffu - position) : 0ull;
}

template <int PER>
__global__ __launch_bounds__(TOKEN_THREADS) void token_select_kernel(const float* __restrict__ values, const uint8_t* __restrict__ valid,
                                                                     const float* __restrict__ scores, const float* __restrict__ labels,
                                                                     int32_t* __restrict__ pos, float* __restrict__ val,
                                                                     int32_t* __restrict__ counts, const int S, const int K) {
  constexpr int WAVES = TOKEN_THREADS / 64;
  __shared__ unsigned long long wave_best[2][WAVES];
  __shared__ int wave_count[5][WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t item = blockIdx.x;
  const float* __restrict__ v_row = values + item * S;
  const float* __restrict__ s_row = scores ? scores + item * S : v_row;
  const float* __restrict__ l_row = labels ? labels + item * S : nullptr;

  uint32_t key[PER];
  int n_valid = 0, n_pos = 0, n_pred = 0, tp = 0, hits = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = j * TOKEN_THREADS + tid;
    uint32_t k = 0u;
    if (i < S && (valid == nullptr || valid[item * S + i] != 0)) {
      k = token_score_bits(v_row[i]);
      if (l_row) {
        const bool positive = l_row[i] > 0.5f, predicted = s_row[i] > 0.f;
        n_valid += 1;
        n_pos += positive;
        n_pred += predicted;
        tp += positive && predicted;
      }
    }
    key[j] = k;
  }

  unsigned long long mine = token_local_best<PER>(key);
  int r = 0;
  for (; r < K; ++r) {  // (every thread leaves the loop in the same round: the barrier is reached by all)
    const unsigned long long w = token_wave_max(mine);
    if (lane == 0) wave_best[r & 1][wave] = w;
    __syncthreads();
    unsigned long long best = wave_best[r & 1][0];
#pragma unroll
    for (int q = 1; q < WAVES; ++q) best = wave_best[r & 1][q] > best ? wave_best[r & 1][q] : best;
    if (best == 0ull) break;
    if (mine == best) {  // (one thread: the position is part of the key)
      const int i = (int)(0xffffffffu - (uint32_t)best);
      pos[item * K + r] = i;
      val[item * K + r] = v_row[i];
      if (l_row) hits += l_row[i] > 0.5f;
      const int at = i / TOKEN_THREADS;
#pragma unroll
      for (int j = 0; j < PER; ++j)
        if (j == at) key[j] = 0u;
      mine = token_local_best<PER>(key);
    }
  }
  for (int q = r + tid; q < K; q += TOKEN_THREADS) {  // behind the valid positions of the item
    pos[item * K + q] = -1;
    val[item * K + q] = 0.f;
  }

  if (counts) {
    const int c[5] = {token_wave_sum(n_valid), token_wave_sum(n_pos), token_wave_sum(n_pred), token_wave_sum(tp), token_wave_sum(hits)};
    if (lane == 0)
#pragma unroll
      for (int m = 0; m < 5; ++m) wave_count[m][wave] = c[m];
    __syncthreads();
    if (tid < 5) {
      int total = 0;
#pragma unroll
      for (int q = 0; q < WAVES; ++q) total += wave_count[tid][q];
      counts[item * 5 + tid] = total;
    }
  }
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
extern "C" int case_token_labels(const int64_t* passage, const int64_t* response, const void* freq, int32_t freq_is_i64, float* label,
                                 float* weight, int64_t B, int64_t P, int64_t L, int64_t T, int64_t F, int64_t pad, case_stream_t stream) {
  CASE_REQUIRE(passage && response && label && weight && B > 0 && P > 0 && L > 0 && T > 0 && F >= 0 && (freq || F == 0) && B * P < (1ll << 31),
               "case_token_labels: bad argument");
  if (L > TOKEN_MAX_L || T > TOKEN_MAX_T)
    return case_set_error(CASE_E_UNSUPPORTED, "case_token_labels: rows of up to %d tokens and answers of up to %d ids (got %lld and %lld)",
                          TOKEN_MAX_L, TOKEN_MAX_T, (long long)L, (long long)T);
  const dim3 grid((unsigned)(B * P)), block(TOKEN_THREADS);
  if (freq_is_i64)
    hipLaunchKernelGGL(token_labels_kernel<int64_t>, grid, block, 0, (hipStream_t)stream, passage, response, (const int64_t*)freq, label, weight,
                       (int)P, (int)L, (int)T, F, pad);
  else
    hipLaunchKernelGGL(token_labels_kernel<float>, grid, block, 0, (hipStream_t)stream, passage, response, (const float*)freq, label, weight,
                       (int)P, (int)L, (int)T, F, pad);
  return case_check_launch("case_token_labels");
}

extern "C" int case_token_select(const float* values, const uint8_t* valid, const float* scores, const float* labels, int32_t* pos, float* val,
                                 int32_t* counts, int64_t B, int64_t S, int32_t K, case_stream_t stream) {
  CASE_REQUIRE(values && pos && val && B > 0 && B < (1ll << 31) && S > 0 && K > 0 && (counts == nullptr) == (labels == nullptr),
               "case_token_select: bad argument");
  if (S > TOKEN_MAX_L || K > TOKEN_MAX_K)
    return case_set_error(CASE_E_UNSUPPORTED, "case_token_select: rows of up to %d keys and up to %d selected positions (got %lld and %d)",
                          TOKEN_MAX_L, TOKEN_MAX_K, (long long)S, (int)K);
  const dim3 grid((unsigned)B), block(TOKEN_THREADS);
#define TOKEN_SELECT(PER)                                                                                                                  \
  hipLaunchKernelGGL(token_select_kernel<PER>, grid, block, 0, (hipStream_t)stream, values, valid, scores, labels, pos, val, counts, (int)S, \
                     (int)K)
  if (S <= 1 * TOKEN_THREADS)
    TOKEN_SELECT(1);
  else if (S <= 4 * TOKEN_THREADS)
    TOKEN_SELECT(4);
  else if (S <= 16 * TOKEN_THREADS)
    TOKEN_SELECT(16);
  else
    TOKEN_SELECT(64);
#undef TOKEN_SELECT
  return case_check_launch("case_token_select");
}
