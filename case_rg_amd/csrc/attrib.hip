// Answer attribution: where the pointer mass of a target token comes from.
//   K39 case_copy_attribution  per row: the pointer mass of the target split over segments of the source (the conversation context and
//                              every passage of the pool), the single source position with the largest term, that term, and the run length
// K29 (attn_pointer.hip) walks the same run of the item's sorted keys and collapses it into one float; this kernel keeps the parts.
// Nothing here waits for the host, no kernel uses an atomic, and the library keeps no state.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "case_hip.h"
#include "common.h"

constexpr int CA_WAVES = 4;                  // rows per workgroup: one wave each
constexpr int CA_THREADS = 64 * CA_WAVES;
constexpr int CA_MAX_MEM = 4;                // K29's limit (PH_MAX_MEM)
constexpr int CA_MAX_G = 64;                 // lane g carries segment g's mass
constexpr int64_t CA_MAX_V = 131071, CA_MAX_S = 32768;  // the key format of case_source_sort

struct AttribArgs {
  const float* mix_logits;  // [R, 1 + nmem]
  const uint32_t* keys;     // [R / rows_per_source, S] sorted (token << 15 | position), 0xFFFFFFFF = no token
  const float* copy[CA_MAX_MEM];  // copy_k [R, len_k]
  int64_t len[CA_MAX_MEM];
  const int64_t* targets;   // [R]
  const int32_t* seg_dev;   // [G + 1] in device memory, or null: seg_val holds the boundaries
  int32_t seg_val[CA_MAX_G + 1];
  float* mass;              // [R, G]
  int32_t* pos;             // [R]
  float* pos_mass;          // [R]
  int32_t* count;           // [R]
  int64_t R, V, S, rows_per_source, pad;
  int nmem, G;
};

// the first index in [lo, hi) whose key is >= want (uniform over the wave: every lane runs the same search)
__device__ __forceinline__ int64_t ca_lower_bound(const uint32_t* __restrict__ keys, int64_t lo, int64_t hi, const uint32_t want) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- K39 -------------------------------------------------------------------------------------------------------------------------
// One wave per row, four rows per workgroup; the segment boundaries sit in LDS (one barrier, before any wave leaves).  pm is K29's: f32,
// __expf, the same order.  The run of y in the row's sorted keys is [lo, hi): two searches.  Lane l takes entries lo + l, lo + l + 64, ...:
// their positions ascend, so a lane meets the segments in ascending order.  The wave walks the segments from the one that holds the run's
// first position (a search of the boundaries in LDS); in segment g every lane adds the terms of its entries below seg_start[g + 1] in f64,
// the 64 partial sums meet in a fixed xor tree, and lane g keeps the sum rounded to f32 once.  The walk ends when no lane has an entry
// left.  The arg-max is a fixed tree over (term, lower position); a lane's first entry always enters, so an all-zero run gives its lowest
// position.  Two launches give the same bits.
__global__ __launch_bounds__(CA_THREADS) void copy_attribution_kernel(const AttribArgs a) {
  __shared__ int seg[CA_MAX_G + 1];
  const int tid = threadIdx.x, lane = tid & 63, G = a.G;
  if (tid <= G) seg[tid] = a.seg_dev ? a.seg_dev[tid] : a.seg_val[tid];
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * CA_WAVES + (tid >> 6);
  if (r >= a.R) return;  // (whole waves; no barrier behind this point)

  const int64_t y = a.targets[r];
  int64_t lo = 0, hi = 0;
  const uint32_t* __restrict__ keys = a.keys + (r / a.rows_per_source) * a.S;
  if (!(a.pad >= 0 && y == a.pad) && y >= 0 && y < a.V) {  // (uniform over the wave)
    lo = ca_lower_bound(keys, 0, a.S, (uint32_t)y << 15);  // y < V <= 131071: fits
    hi = ca_lower_bound(keys, lo, a.S, (uint32_t)(y + 1) << 15);  // <= 0xFFFF8000: the keys without a token lie behind it
  }
  if (hi == lo) {  // PAD, an id outside the vocabulary, or a token the item's source does not hold
    if (lane < G) a.mass[r * G + lane] = 0.f;
    if (lane == 0) {
      a.pos[r] = -1;
      a.pos_mass[r] = 0.f;
      a.count[r] = 0;
    }
    return;
  }

  // the mixing probabilities, as in pointer_head_score_kernel
  float pm[1 + CA_MAX_MEM];
  {
    float mm = -INFINITY, ss = 0.f;
#pragma unroll
    for (int k = 0; k <= CA_MAX_MEM; ++k) pm[k] = k <= a.nmem ? a.mix_logits[r * (a.nmem + 1) + k] : -INFINITY;
#pragma unroll
    for (int k = 0; k <= CA_MAX_MEM; ++k) mm = fmaxf(mm, pm[k]);
#pragma unroll
    for (int k = 0; k <= CA_MAX_MEM; ++k) {
      pm[k] = __expf(pm[k] - mm);
      ss += pm[k];
    }
#pragma unroll
    for (int k = 0; k <= CA_MAX_MEM; ++k) pm[k] /= ss;
  }

  // the segment of the run's first position: the last g with seg[g] <= p0, kept inside [0, G - 1]
  int g0 = 0;
  {
    const int p0 = (int)(keys[lo] & 0x7FFFu);
    int l = 0, h = G;  // the first g in [0, G) with seg[g + 1] > p0
    while (l < h) {
      const int mid = (l + h) >> 1;
      if (seg[mid + 1] <= p0) l = mid + 1;
      else h = mid;
    }
    g0 = l < G ? l : G - 1;
  }

  int64_t i = lo + lane;     // this lane's next entry
  int cur_p = INT_MAX;       // its position (INT_MAX: the lane has none left) and term
  float cur_t = 0.f;
  int best_p = INT_MAX;      // the lane's largest term so far, at its lowest position
  float best_t = -INFINITY;
  auto fetch = [&]() {
    if (i >= hi) {
      cur_p = INT_MAX;
      return;
    }
    const int p = (int)(keys[i] & 0x7FFFu);
    int64_t q = p;
    float t = 0.f;  // (a position behind every memory cannot come from case_source_sort; it would count with a term of 0)
    bool done = false;
#pragma unroll
    for (int k = 0; k < CA_MAX_MEM; ++k) {
      if (k < a.nmem && !done) {
        if (q < a.len[k]) {
          t = pm[k + 1] * a.copy[k][r * a.len[k] + q];
          done = true;
        }
        q -= a.len[k];
      }
    }
    cur_p = p;
    cur_t = t;
    if (best_p == INT_MAX || t > best_t) {  // (strictly: the lane's positions ascend, the lower one stays)
      best_p = p;
      best_t = t;
    }
  };
  fetch();

  float mine = 0.f;  // lane g: the mass of segment g
  for (int g = g0; g < G; ++g) {
    if (__ballot(cur_p != INT_MAX) == 0ull) break;  // (uniform) the run is used up
    const int end = seg[g + 1];
    double acc = 0.0;
    bool took = false;
    while (cur_p < end) {
      acc += (double)cur_t;
      took = true;
      i += 64;
      fetch();
    }
    if (__ballot(took) == 0ull) continue;  // (uniform) nothing of the run lies in this segment
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == g) mine = (float)acc;
  }

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ot = __shfl_xor(best_t, o, 64);
    const int op = __shfl_xor(best_p, o, 64);
    if (op != INT_MAX && (best_p == INT_MAX || ot > best_t || (ot == best_t && op < best_p))) {
      best_t = ot;
      best_p = op;
    }
  }
  if (lane < G) a.mass[r * G + lane] = mine;
  if (lane == 0) {
    a.pos[r] = best_p;
    a.pos_mass[r] = best_t;
    a.count[r] = (int32_t)(hi - lo);
  }
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
extern "C" int case_copy_attribution(const float* mix_logits, const uint32_t* keys, int64_t rows_per_source, const float* const* copies,
                                     const int64_t* lens, int32_t nmem, const int64_t* targets, int64_t pad, const int32_t* seg_start,
                                     const int32_t* seg_start_host, int32_t G, float* mass, int32_t* pos, float* pos_mass, int32_t* count,
                                     int64_t R, int64_t V, int64_t S, case_stream_t stream) {
  CASE_REQUIRE(mix_logits && keys && copies && lens && targets && mass && pos && pos_mass && count && R > 0 && R < (1ll << 31) && V > 0 && S > 0 &&
                   nmem >= 1 && (seg_start || seg_start_host),
               "case_copy_attribution: bad argument");
  CASE_REQUIRE(rows_per_source >= 1 && R % rows_per_source == 0, "case_copy_attribution: %lld rows are no multiple of rows_per_source %lld",
               (long long)R, (long long)rows_per_source);
  if (nmem > CA_MAX_MEM || V > CA_MAX_V || S > CA_MAX_S || G < 1 || G > CA_MAX_G)
    return case_set_error(CASE_E_UNSUPPORTED, "case_copy_attribution: built for <= %d memories, V <= %lld, S <= %lld and 1 .. %d segments (got %d, %lld, %lld, %d)",
                          CA_MAX_MEM, (long long)CA_MAX_V, (long long)CA_MAX_S, CA_MAX_G, (int)nmem, (long long)V, (long long)S, (int)G);
  AttribArgs a;
  a.mix_logits = mix_logits;
  a.keys = keys;
  int64_t total = 0;
  for (int m = 0; m < CA_MAX_MEM; ++m) {
    CASE_REQUIRE(m >= nmem || (copies[m] && lens[m] > 0), "case_copy_attribution: null copy weights");
    a.copy[m] = m < nmem ? copies[m] : nullptr;
    a.len[m] = m < nmem ? lens[m] : 0;
    total += a.len[m];
  }
  CASE_REQUIRE(total == S, "case_copy_attribution: the memories hold %lld positions, the source map %lld", (long long)total, (long long)S);
  for (int g = 0; g <= CA_MAX_G; ++g) a.seg_val[g] = 0;
  if (seg_start_host) {  // host memory: checked here, and handed to the kernel by value
    for (int g = 0; g <= G; ++g) a.seg_val[g] = seg_start_host[g];
    bool ascending = true;
    for (int g = 0; g < G; ++g) ascending = ascending && seg_start_host[g] < seg_start_host[g + 1];
    CASE_REQUIRE(ascending && seg_start_host[0] == 0 && seg_start_host[G] == S,
                 "case_copy_attribution: seg_start must ascend strictly from 0 to S = %lld", (long long)S);
    a.seg_dev = nullptr;
  } else {  // device memory: the caller has checked it; the kernel's walk is bounded by G whatever it holds
    a.seg_dev = seg_start;
  }
  a.targets = targets;
  a.mass = mass;
  a.pos = pos;
  a.pos_mass = pos_mass;
  a.count = count;
  a.R = R;
  a.V = V;
  a.S = S;
  a.rows_per_source = rows_per_source;
  a.pad = pad;
  a.nmem = nmem;
  a.G = G;
  const int64_t blocks = (R + CA_WAVES - 1) / CA_WAVES;
  hipLaunchKernelGGL(copy_attribution_kernel, dim3((unsigned)blocks), dim3(CA_THREADS), 0, (hipStream_t)stream, a);
  return case_check_launch("case_copy_attribution");
}
