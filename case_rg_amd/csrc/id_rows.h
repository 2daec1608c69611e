// The frame of the token-id metric kernels (K30 in lcs.hip, K34 and K43 in ngram.hip, K40 in meteor.hip): one wave per row, the row HELD in
// the wave's lanes, another row STREAMED past it.  Device side: the wave's row, the length clamp, the hold and the streams.  Host side: the
// range of a pair call and the dispatch on the number of held words.  No LDS and no barrier anywhere: a wave keeps to itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

constexpr int ID_MAX_T = 256;  // 4 words of 64 held positions
constexpr int ID_WAVES = 4;    // rows per workgroup, one wave each

// ---- device ----------------------------------------------------------------------------------------------------------------------
// The wave's row.  The readfirstlane makes it provably uniform, so the lengths, the masks and the loop bounds derived from it stay in
// scalar registers.  A kernel returns on `row >= rows` right away: whole waves leave, and no barrier follows.
__device__ __forceinline__ int64_t id_wave_row() { return (int64_t)blockIdx.x * ID_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

// A stated length, taken as 0 .. T.
__device__ __forceinline__ int id_clamp(const int len, const int T) { return len < 0 ? 0 : len > T ? T : len; }

// The held row: lane l, word j holds position first + l + 64 j of `row`, and the sentinel -1 from `end` on.  A valid id is >= 0 and never
// equals the sentinel, so one  __ballot(tok[j] == t)  is the 64-bit mask of the held positions of word j that hold the token t, with a zero
// bit at every position from `end` on: the kernels need no length mask.  (A streamed id below 0 is no token; a kernel whose rule would let
// it meet the sentinel skips it, as K40 does.)
template <int WORDS>
__device__ __forceinline__ void id_hold(const int64_t* __restrict__ row, const int first, const int end, const int lane, int32_t (&tok)[WORDS]) {
#pragma unroll
  for (int j = 0; j < WORDS; ++j) {
    const int pos = first + lane + 64 * j;
    tok[j] = pos < end ? (int32_t)row[pos] : -1;
  }
}

// The streamed row: `len` ids are read 64 per load, one per lane, and handed round by readlane; body(t, p) runs once per position p with
// its id t, both wave-uniform.  State that lives from one position to the next (and from one load to the next) belongs to the body.
template <typename Body>
__device__ __forceinline__ void id_stream(const int64_t* __restrict__ row, const int len, const int lane, Body body) {
  for (int t0 = 0; t0 < len; t0 += 64) {
    const int mine = t0 + lane < len ? (int32_t)row[t0 + lane] : -1;
    const int n = len - t0 < 64 ? len - t0 : 64;
    for (int i = 0; i < n; ++i) body(__builtin_amdgcn_readlane(mine, i), t0 + i);
  }
}

// ... from the last position to the first: the same aligned loads, the last (a partial one) first.  map(id) turns the lane's id into the key
// that is handed round (K40's class stage looks it up in its table once per lane, not once per position).
template <typename Map, typename Body>
__device__ __forceinline__ void id_stream_back(const int64_t* __restrict__ row, const int len, const int lane, Map map, Body body) {
  for (int t0 = (len - 1) & ~63; t0 >= 0; t0 -= 64) {
    const int mine = map(t0 + lane < len ? (int32_t)row[(unsigned)(t0 + lane)] : -1);  // (t0 + lane >= 0: no sign extension per load)
    const int n = len - t0 < 64 ? len - t0 : 64;
    for (int i = n - 1; i >= 0; --i) body(__builtin_amdgcn_readlane(mine, i), t0 + i);
  }
}

// The held row streamed past itself (its first `len` positions; first = 0): no load, the words are handed round as they are.
template <int WORDS, typename Body>
__device__ __forceinline__ void id_stream_held(const int32_t (&tok)[WORDS], const int len, Body body) {
#pragma unroll
  for (int w = 0; w < WORDS; ++w) {
    const int n = len - 64 * w < 64 ? len - 64 * w : 64;
    for (int i = 0; i < n; ++i) body(__builtin_amdgcn_readlane(tok[w], i), 64 * w + i);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// The range of a call on B items of N held rows and M streamed rows: the kernels index rows and pairs with these products.  The entry
// points that take counts instead of rows have no Ta / Tb.
static inline bool id_pairs_in_range(int64_t B, int64_t N, int64_t M, int64_t Ta = 1, int64_t Tb = 1) {
  return B > 0 && N > 0 && M > 0 && Ta > 0 && Tb > 0 && B < (1ll << 31) && N < (1ll << 24) && M < (1ll << 24) && B * N < (1ll << 31) &&
         Tb < (1ll << 30);
}

// One wave per row, ID_WAVES rows per workgroup, and the kernel instance that holds T positions (4 words from 129 on: K43's window):
// launch(std::integral_constant<int, WORDS>, grid, block) with WORDS = 1, 2 or 4.
template <typename Launch>
static inline void id_dispatch_words(const int64_t rows, const int64_t T, Launch launch) {
  const dim3 grid((unsigned)((rows + ID_WAVES - 1) / ID_WAVES)), block(64 * ID_WAVES);
  if (T <= 64)
    launch(std::integral_constant<int, 1>(), grid, block);
  else if (T <= 128)
    launch(std::integral_constant<int, 2>(), grid, block);
  else
    launch(std::integral_constant<int, 4>(), grid, block);
}
