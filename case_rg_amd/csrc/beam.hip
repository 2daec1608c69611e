// Beam search around the cached decode step (common/Generations.py:112-190 of the reference, restated per item on the device).
//   K25 case_beam_advance    the per-item merge of the W x W candidates, EOS / last-step retirement into the finished pool, history append
//   K26 case_beam_gather     reorder of every decoder layer's self-attention cache (+ the prefix validity) by the chosen parents
//   K27 case_beam_backtrack  the finished pool's hypotheses followed back through the history
// A hypothesis is a slot w of item b; row b * W + w of the step's batch.  Nothing here waits for the host.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "case_hip.h"
#include "common.h"

constexpr int BEAM_MAX_W = 8;

// ---- K25 -------------------------------------------------------------------------------------------------------------------------
// One wave per item.  Lane l < W * W holds candidate (parent slot l / W, candidate rank l % W): key = (cum[slot] - log(p + 1e-10)) / (len[slot] + 1),
// +inf for a dead parent.  A lane's place in the stable ascending order is the number of lanes that come before it (smaller key, or the same
// key and a lower lane: Python's sorted() over the (parent slot, candidate rank) sequence); places 0 .. W-1 become the new slots.
// FLAT (K32's beam state): flat_old / flat_new int32 [B, W, Tmax] hold every slot's hypothesis so far, one buffer read and the other written
// (a copy by parent cannot run in place): new[b, w, 0 .. t) = old[b, parent, 0 .. t), new[b, w, t] = the slot's token -- W t <= 2048 ints per
// item.  With the ban on, a candidate of probability exactly 0 (a banned entry that reached the top W) is dead: it can neither take a slot nor
// retire into the pool.
// ALPHA (the length penalty): key = cost / (len[slot] + 1)^alpha, powf in f32, once per live candidate; a retiring hypothesis takes its
// candidate's key as it is (the same cost and length), so the finished pool is ranked by the same formula.  Without ALPHA the key is the
// division above and the code that of the kernels below, instruction for instruction.
template <bool FLAT, bool ALPHA>
__device__ __forceinline__ void beam_advance_body(const float* __restrict__ cand_p, const int64_t* __restrict__ cand_id,
                                                  uint8_t* __restrict__ alive, float* __restrict__ cum, int32_t* __restrict__ len,
                                                  int32_t* __restrict__ parent, int64_t* __restrict__ token,
                                                  int32_t* __restrict__ hist_parent, int64_t* __restrict__ hist_token,
                                                  float* __restrict__ fin_key, int32_t* __restrict__ fin_step, int32_t* __restrict__ fin_slot,
                                                  const int t, const int T, const int64_t B, const int W, const int64_t eos,
                                                  const int32_t* __restrict__ flat_old, int32_t* __restrict__ flat_new,
                                                  const int64_t Tmax, const float alpha) {
  __shared__ int src[BEAM_MAX_W];
  __shared__ int n_par[BEAM_MAX_W], n_tok[BEAM_MAX_W];
  __shared__ float s_key[64], s_cum[64];
  __shared__ int64_t s_tok[64];
  __shared__ int s_len[64];
  __shared__ float n_key[BEAM_MAX_W];
  __shared__ int n_retire[BEAM_MAX_W];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x, n = W * W;
  const int slot = lane / W;
  float key = INFINITY, c = INFINITY;
  int64_t tok = 0;
  int plen = 0;
  if (lane < n) {
    const int64_t row = b * W + slot;
    tok = cand_id[row * W + (lane - slot * W)];
    plen = len[row];
    if (alive[row]) {
      const float p = cand_p[row * W + (lane - slot * W)];
      if (!(FLAT && p == 0.f)) {
        c = cum[row] - logf(p + 1e-10f);
        key = ALPHA ? c / powf((float)(plen + 1), alpha) : c / (float)(plen + 1);
      }
    }
  }
  if (!(key < INFINITY)) key = INFINITY;  // (a NaN probability counts as a dead candidate)
  s_key[lane] = key;
  s_cum[lane] = c;
  s_tok[lane] = tok;
  s_len[lane] = plen;
  if (lane < BEAM_MAX_W) src[lane] = -1;
  __syncthreads();
  int place = 0;
  for (int j = 0; j < n; ++j) {
    const float kj = s_key[j];
    place += (kj < key || (kj == key && j < lane)) ? 1 : 0;
  }
  if (lane < n && place < W && key < INFINITY) src[place] = lane;
  __syncthreads();
  // every candidate's inputs are in registers / LDS by now: the state is rewritten in place
  if (lane < W) {
    const int s = src[lane];
    const int64_t row = b * W + lane;
    const int sp = s < 0 ? lane : s / W;  // an empty slot keeps its own history (the gather then copies the row onto itself)
    const int64_t stok = s < 0 ? 0 : s_tok[s];
    const int slen = s < 0 ? 0 : s_len[s] + 1;
    const bool live = s >= 0;
    const bool retire = live && (stok == eos || t == T - 1);
    parent[row] = sp;
    token[row] = (live && !retire) ? stok : 0;  // PAD feeds the rows that no longer count
    alive[row] = (live && !retire) ? 1 : 0;
    cum[row] = live ? s_cum[s] : INFINITY;
    len[row] = live ? slen : 0;
    hist_parent[((int64_t)t * B + b) * W + lane] = sp;
    hist_token[((int64_t)t * B + b) * W + lane] = stok;
    n_key[lane] = live ? s_key[s] : INFINITY;
    n_retire[lane] = retire ? 1 : 0;
    if constexpr (FLAT) {
      n_par[lane] = sp;
      n_tok[lane] = (int)stok;
    }
  }
  __syncthreads();
  if constexpr (FLAT) {
    for (int w = 0; w < W; ++w) {
      const int32_t* from = flat_old + (b * W + n_par[w]) * Tmax;
      int32_t* to = flat_new + (b * W + w) * Tmax;
      for (int i = lane; i < t; i += 64) to[i] = from[i];
      if (lane == 0) to[t] = n_tok[w];
    }
  }
  // the finished pool: ascending by key, a newcomer behind its equals (list.sort is stable over the order of retirement); a key is final
  // when its hypothesis retires, so whatever falls off the end could never have been among the best W
  if (lane == 0) {
    float fk[BEAM_MAX_W];
    int fs[BEAM_MAX_W], fl[BEAM_MAX_W];
#pragma unroll
    for (int i = 0; i < BEAM_MAX_W; ++i) {
      fk[i] = i < W ? fin_key[b * W + i] : INFINITY;
      fs[i] = i < W ? fin_step[b * W + i] : -1;
      fl[i] = i < W ? fin_slot[b * W + i] : 0;
    }
    bool changed = false;
    for (int r = 0; r < W; ++r) {
      if (!n_retire[r]) continue;
      const float k = n_key[r];
      int at = 0;
      while (at < W && fs[at] >= 0 && fk[at] <= k) ++at;
      if (at >= W) continue;
#pragma unroll
      for (int i = BEAM_MAX_W - 1; i > 0; --i)
        if (i > at && i < W) {
          fk[i] = fk[i - 1];
          fs[i] = fs[i - 1];
          fl[i] = fl[i - 1];
        }
#pragma unroll
      for (int i = 0; i < BEAM_MAX_W; ++i)
        if (i == at) {
          fk[i] = k;
          fs[i] = t;
          fl[i] = r;
        }
      changed = true;
    }
    if (changed) {
#pragma unroll
      for (int i = 0; i < BEAM_MAX_W; ++i)
        if (i < W) {
          fin_key[b * W + i] = fk[i];
          fin_step[b * W + i] = fs[i];
          fin_slot[b * W + i] = fl[i];
        }
    }
  }
}

template <bool FLAT>
__global__ __launch_bounds__(64) void beam_advance_kernel(const float* __restrict__ cand_p, const int64_t* __restrict__ cand_id,
                                                          uint8_t* __restrict__ alive, float* __restrict__ cum, int32_t* __restrict__ len,
                                                          int32_t* __restrict__ parent, int64_t* __restrict__ token,
                                                          int32_t* __restrict__ hist_parent, int64_t* __restrict__ hist_token,
                                                          float* __restrict__ fin_key, int32_t* __restrict__ fin_step, int32_t* __restrict__ fin_slot,
                                                          const int t, const int T, const int64_t B, const int W, const int64_t eos,
                                                          const int32_t* __restrict__ flat_old, int32_t* __restrict__ flat_new,
                                                          const int64_t Tmax) {
  beam_advance_body<FLAT, false>(cand_p, cand_id, alive, cum, len, parent, token, hist_parent, hist_token, fin_key, fin_step, fin_slot, t, T, B, W, eos,
                                 flat_old, flat_new, Tmax, 1.f);
}

// K25 with the length penalty (flat history)
__global__ __launch_bounds__(64) void beam_advance_alpha_kernel(const float* __restrict__ cand_p, const int64_t* __restrict__ cand_id,
                                                                uint8_t* __restrict__ alive, float* __restrict__ cum, int32_t* __restrict__ len,
                                                                int32_t* __restrict__ parent, int64_t* __restrict__ token,
                                                                int32_t* __restrict__ hist_parent, int64_t* __restrict__ hist_token,
                                                                float* __restrict__ fin_key, int32_t* __restrict__ fin_step,
                                                                int32_t* __restrict__ fin_slot, const int t, const int T, const int64_t B, const int W,
                                                                const int64_t eos, const int32_t* __restrict__ flat_old,
                                                                int32_t* __restrict__ flat_new, const int64_t Tmax, const float alpha) {
  beam_advance_body<true, true>(cand_p, cand_id, alive, cum, len, parent, token, hist_parent, hist_token, fin_key, fin_step, fin_slot, t, T, B, W, eos,
                                flat_old, flat_new, Tmax, alpha);
}

// ---- K26 -------------------------------------------------------------------------------------------------------------------------
// dst[l][b * W + w, 0 .. t] = src[l][b * W + parent[b, w], 0 .. t] for every layer l of the table, 16 bytes per lane and access; the last
// grid row copies the prefix validity bytes.  Source and destination are different buffers (the caller ping-pongs).
// The by-value pointer table holds BG_MAX_LAYERS layers: one launch up to that many (the models here have 8), one launch per 16 layers beyond.
constexpr int BG_MAX_LAYERS = 16;
struct GatherArgs {
  const uint4* src[BG_MAX_LAYERS];
  uint4* dst[BG_MAX_LAYERS];
  const uint8_t* valid_src;
  uint8_t* valid_dst;
  const int32_t* parent;
  int64_t row_vecs;   // uint4s per cache row [Tmax, 2E]
  int64_t copy_vecs;  // uint4s of positions 0 .. t
  int64_t Tmax;
  int nlayers, W, t;
};

__global__ __launch_bounds__(256) void beam_gather_kernel(const GatherArgs a) {
  const int64_t row = blockIdx.x;
  const int p = a.parent[row];
  const int64_t from = row - row % a.W + (p < 0 ? 0 : p >= a.W ? a.W - 1 : p);  // (a slot index of the same item, whatever the caller wrote)
  const int l = blockIdx.y;
  if (l == a.nlayers) {
    if (a.valid_src)
      for (int i = threadIdx.x; i <= a.t; i += 256) a.valid_dst[row * a.Tmax + i] = a.valid_src[from * a.Tmax + i];
    return;
  }
  const uint4* __restrict__ s = a.src[l] + from * a.row_vecs;
  uint4* __restrict__ d = a.dst[l] + row * a.row_vecs;
  for (int64_t i = threadIdx.x; i < a.copy_vecs; i += 256) d[i] = s[i];
}

// ---- K27 -------------------------------------------------------------------------------------------------------------------------
// One thread per (item, pool entry): the entry retired as slot fin_slot of step fin_step; its tokens are hist_token[s, b, slot] for s going down,
// slot = hist_parent[s, b, slot] on the way.  PAD behind the last token; an empty entry is all PAD with score +inf.
__global__ __launch_bounds__(64) void beam_backtrack_kernel(const int32_t* __restrict__ hist_parent, const int64_t* __restrict__ hist_token,
                                                            const float* __restrict__ fin_key, const int32_t* __restrict__ fin_step,
                                                            const int32_t* __restrict__ fin_slot, int64_t* __restrict__ answer,
                                                            int64_t* __restrict__ beam_answers, float* __restrict__ beam_scores, const int64_t B,
                                                            const int W, const int T) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= B * W) return;
  const int64_t b = i / W;
  const int k = (int)(i - b * W);
  const int last = fin_step[i];
  int slot = fin_slot[i];
  int64_t* out = beam_answers + i * T;
  for (int s = T - 1; s >= 0; --s) {
    int64_t tok = 0;
    if (s <= last && last < T && slot >= 0 && slot < W) {
      tok = hist_token[((int64_t)s * B + b) * W + slot];
      slot = hist_parent[((int64_t)s * B + b) * W + slot];
    }
    out[s] = tok;
    if (k == 0) answer[b * T + s] = tok;
  }
  beam_scores[i] = last >= 0 ? fin_key[i] : INFINITY;
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
// K25's three entry points share one check and one launch.  `flat`: the entry point takes the flat-history pair (required then); `alpha`: the length
// penalty, or null for the plain key.  `who` names the entry point in every message.
static int beam_advance_launch(const char* who, const float* cand_p, const int64_t* cand_id, uint8_t* alive, float* cum, int32_t* len, int32_t* parent,
                               int64_t* token, int32_t* hist_parent, int64_t* hist_token, float* fin_key, int32_t* fin_step, int32_t* fin_slot,
                               int64_t t, int64_t T, int64_t B, int32_t W, int64_t eos, bool flat, const int32_t* flat_old, int32_t* flat_new,
                               int64_t Tmax, const float* alpha, case_stream_t stream) {
  CASE_REQUIRE(cand_p && cand_id && alive && cum && len && parent && token && hist_parent && hist_token && fin_key && fin_step && fin_slot &&
                   B > 0 && B < (1ll << 31) && T > 0 && T < (1ll << 30) && t >= 0 && t < T &&
                   (!flat || (flat_old && flat_new && flat_old != flat_new && t < Tmax)),
               "%s: bad argument", who);
  if (W < 1 || W > BEAM_MAX_W) return case_set_error(CASE_E_UNSUPPORTED, "%s: width %d outside 1 .. %d", who, W, BEAM_MAX_W);
  const auto launch = [&](auto kernel, auto... tail) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, cand_p, cand_id, alive, cum, len, parent, token, hist_parent,
                       hist_token, fin_key, fin_step, fin_slot, (int)t, (int)T, B, (int)W, eos, flat_old, flat_new, Tmax, tail...);
  };
  if (alpha)
    launch(beam_advance_alpha_kernel, *alpha);
  else if (flat)
    launch(beam_advance_kernel<true>);
  else
    launch(beam_advance_kernel<false>);
  return case_check_launch(who);
}

extern "C" int case_beam_advance(const float* cand_p, const int64_t* cand_id, uint8_t* alive, float* cum, int32_t* len, int32_t* parent,
                                 int64_t* token, int32_t* hist_parent, int64_t* hist_token, float* fin_key, int32_t* fin_step,
                                 int32_t* fin_slot, int64_t t, int64_t T, int64_t B, int32_t W, int64_t eos, case_stream_t stream) {
  return beam_advance_launch("case_beam_advance", cand_p, cand_id, alive, cum, len, parent, token, hist_parent, hist_token, fin_key, fin_step, fin_slot, t,
                             T, B, W, eos, false, nullptr, nullptr, 0, nullptr, stream);
}

extern "C" int case_beam_advance_ban(const float* cand_p, const int64_t* cand_id, uint8_t* alive, float* cum, int32_t* len, int32_t* parent,
                                     int64_t* token, int32_t* hist_parent, int64_t* hist_token, float* fin_key, int32_t* fin_step,
                                     int32_t* fin_slot, int64_t t, int64_t T, int64_t B, int32_t W, int64_t eos, const int32_t* flat_old,
                                     int32_t* flat_new, int64_t Tmax, case_stream_t stream) {
  return beam_advance_launch("case_beam_advance_ban", cand_p, cand_id, alive, cum, len, parent, token, hist_parent, hist_token, fin_key, fin_step, fin_slot,
                             t, T, B, W, eos, true, flat_old, flat_new, Tmax, nullptr, stream);
}

// K25 with the length penalty alpha (CASE_FEAT_DECODE_RULES): the flat-history form; alpha == 1 is case_beam_advance_ban's call itself
extern "C" int case_beam_advance_rules(const float* cand_p, const int64_t* cand_id, uint8_t* alive, float* cum, int32_t* len, int32_t* parent,
                                       int64_t* token, int32_t* hist_parent, int64_t* hist_token, float* fin_key, int32_t* fin_step,
                                       int32_t* fin_slot, int64_t t, int64_t T, int64_t B, int32_t W, int64_t eos, const int32_t* flat_old,
                                       int32_t* flat_new, int64_t Tmax, float length_penalty, case_stream_t stream) {
  CASE_REQUIRE(length_penalty >= 0.f && length_penalty < INFINITY, "case_beam_advance_rules: the length penalty must be a finite float >= 0");
  const bool plain = length_penalty == 1.f;
  return beam_advance_launch(plain ? "case_beam_advance_ban" : "case_beam_advance_rules", cand_p, cand_id, alive, cum, len, parent, token, hist_parent,
                             hist_token, fin_key, fin_step, fin_slot, t, T, B, W, eos, true, flat_old, flat_new, Tmax, plain ? nullptr : &length_penalty,
                             stream);
}

extern "C" int case_beam_gather(const void* const* src, void* const* dst, int32_t nlayers, const int32_t* parent, const uint8_t* valid_src,
                                uint8_t* valid_dst, int64_t B, int32_t W, int64_t Tmax, int64_t row_bytes, int64_t t, case_stream_t stream) {
  CASE_REQUIRE(src && dst && parent && nlayers >= 1 && B > 0 && W >= 1 && B * W < (1ll << 31) && Tmax > 0 && row_bytes > 0 && t >= 0 && t < Tmax &&
                   (valid_src == nullptr) == (valid_dst == nullptr),
               "case_beam_gather: bad argument");
  if (W > BEAM_MAX_W || row_bytes % 16 != 0)
    return case_set_error(CASE_E_UNSUPPORTED, "case_beam_gather: width <= %d and cache positions of a multiple of 16 bytes (got %d, %lld)", BEAM_MAX_W, W,
                          (long long)row_bytes);
  for (int32_t l0 = 0; l0 < nlayers; l0 += BG_MAX_LAYERS) {
    GatherArgs a;
    a.nlayers = nlayers - l0 < BG_MAX_LAYERS ? nlayers - l0 : BG_MAX_LAYERS;
    for (int l = 0; l < BG_MAX_LAYERS; ++l) {
      a.src[l] = l < a.nlayers ? static_cast<const uint4*>(src[l0 + l]) : nullptr;
      a.dst[l] = l < a.nlayers ? static_cast<uint4*>(dst[l0 + l]) : nullptr;
      if (l < a.nlayers) {
        CASE_REQUIRE(a.src[l] && a.dst[l] && a.src[l] != a.dst[l], "case_beam_gather: layer %d needs two different cache buffers", l0 + l);
        CASE_REQUIRE(((uintptr_t)a.src[l] | (uintptr_t)a.dst[l]) % 16 == 0, "case_beam_gather: layer %d is not 16-byte aligned", l0 + l);
      }
    }
    const bool last = l0 + BG_MAX_LAYERS >= nlayers;
    a.valid_src = last ? valid_src : nullptr;
    a.valid_dst = last ? valid_dst : nullptr;
    CASE_REQUIRE(!a.valid_src || a.valid_src != a.valid_dst, "case_beam_gather: the validity needs two different buffers");
    a.parent = parent;
    a.row_vecs = Tmax * row_bytes / 16;
    a.copy_vecs = (t + 1) * row_bytes / 16;
    a.Tmax = Tmax;
    a.W = W;
    a.t = (int)t;
    hipLaunchKernelGGL(beam_gather_kernel, dim3((unsigned)(B * W), (unsigned)(a.nlayers + (a.valid_src ? 1 : 0))), dim3(256), 0, (hipStream_t)stream, a);
    if (const int rc = case_check_launch("case_beam_gather")) return rc;
  }
  return CASE_OK;
}

extern "C" int case_beam_backtrack(const int32_t* hist_parent, const int64_t* hist_token, const float* fin_key, const int32_t* fin_step,
                                   const int32_t* fin_slot, int64_t* answer, int64_t* beam_answers, float* beam_scores, int64_t B, int32_t W,
                                   int64_t T, case_stream_t stream) {
  CASE_REQUIRE(hist_parent && hist_token && fin_key && fin_step && fin_slot && answer && beam_answers && beam_scores && B > 0 && B < (1ll << 31) &&
                   T > 0 && T < (1ll << 30),
               "case_beam_backtrack: bad argument");
  if (W < 1 || W > BEAM_MAX_W) return case_set_error(CASE_E_UNSUPPORTED, "case_beam_backtrack: width %d outside 1 .. %d", W, BEAM_MAX_W);
  hipLaunchKernelGGL(beam_backtrack_kernel, dim3((unsigned)((B * W + 63) / 64)), dim3(64), 0, (hipStream_t)stream, hist_parent, hist_token, fin_key,
                     fin_step, fin_slot, answer, beam_answers, beam_scores, B, (int)W, (int)T);
  return case_check_launch("case_beam_backtrack");
}
