// Minimum-risk training: the expected cost of a pool of candidates under the renormalised model posterior, and its gradient.
//   K42 case_sequence_risk  per item: l_n = sum over the scored positions of ln max(p[n, t], 1e-30), Q = softmax_n(alpha l) over the valid
//                           candidates, risk = sum_n Q_n cost_n, grad_p[n, t] = alpha Q_n (cost_n - risk) / p[n, t]
//                           (evaluation/risk.py states the rule and is the host form)
// Nothing here waits for the host, and the library keeps no state.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "case_hip.h"
#include "common.h"

constexpr int RISK_MAX_N = 64, RISK_MAX_T = 1024;
constexpr double RISK_P_MIN = 1e-30;

// ---- K42 -------------------------------------------------------------------------------------------------------------------------
// One wave per item; lane n owns candidate n.  l_n is summed in f64 in position order; the maximum and the two sums over the candidates
// meet in a fixed xor tree in f64, so every lane ends with the same bits and two launches agree.  Every output is the f64 value rounded to
// f32 once.  Then the wave writes grad_p row by row (the lanes along t), the row's factor handed round by a lane read.
__global__ __launch_bounds__(64) void sequence_risk_kernel(const float* __restrict__ p, const uint8_t* __restrict__ scored,
                                                           const float* __restrict__ cost, const uint8_t* __restrict__ valid, const double alpha,
                                                           float* __restrict__ risk, float* __restrict__ q, float* __restrict__ grad_p, const int N,
                                                           const int T) {
#pragma clang fp contract(off)
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const bool mine = lane < N && (!valid || valid[b * N + lane]);
  double l = 0.0;
  if (mine) {
    const float* __restrict__ row = p + (b * N + lane) * T;
    const uint8_t* __restrict__ on = scored + (b * N + lane) * T;
    for (int t = 0; t < T; ++t)
      if (on[t]) l += log(fmax((double)row[t], RISK_P_MIN));
  }
  const double z = mine ? alpha * l : -INFINITY;
  double zmax = z;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) zmax = fmax(zmax, __shfl_xor(zmax, o, 64));
  const bool any = zmax > -INFINITY;  // (uniform) an item without a valid candidate: zeros
  const double e = mine && any ? exp(z - zmax) : 0.0;
  double den = e;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) den += __shfl_xor(den, o, 64);
  const double Q = any ? e / den : 0.0;
  const double c = lane < N ? (double)cost[b * N + lane] : 0.0;
  double rk = mine ? Q * c : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rk += __shfl_xor(rk, o, 64);
  if (lane == 0) risk[b] = (float)rk;
  if (lane < N) q[b * N + lane] = (float)Q;
  const double dl = mine ? alpha * Q * (c - rk) : 0.0;
  for (int n = 0; n < N; ++n) {
    const double dn = __shfl(dl, n, 64);
    const int64_t at = (b * N + n) * T;
    for (int t = lane; t < T; t += 64) {
      const double pt = (double)p[at + t];
      grad_p[at + t] = scored[at + t] && pt > RISK_P_MIN ? (float)(dn / pt) : 0.f;
    }
  }
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
extern "C" int case_sequence_risk(const float* token_probs, const uint8_t* scored, const float* cost, const uint8_t* valid, double alpha, float* risk,
                                  float* q, float* grad_p, int64_t B, int64_t N, int64_t T, case_stream_t stream) {
  CASE_REQUIRE(token_probs && scored && cost && risk && q && grad_p && B > 0 && B < (1ll << 31) && N > 0 && T > 0, "case_sequence_risk: bad argument");
  CASE_REQUIRE(alpha >= 0.0 && isfinite(alpha), "case_sequence_risk: alpha must be >= 0 and finite (got %g)", alpha);
  if (N > RISK_MAX_N || T > RISK_MAX_T)
    return case_set_error(CASE_E_UNSUPPORTED, "case_sequence_risk: pools of up to %d candidates of up to %d positions (got %lld x %lld)", RISK_MAX_N,
                          RISK_MAX_T, (long long)N, (long long)T);
  hipLaunchKernelGGL(sequence_risk_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, token_probs, scored, cost, valid, alpha, risk, q,
                     grad_p, (int)N, (int)T);
  return case_check_launch("case_sequence_risk");
}
