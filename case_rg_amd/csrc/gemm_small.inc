// Small-problem bf16 GEMM (included by gemm.hip): 64x64 output tiles whose WHOLE K panel (<= 10 K tiles of 64) is brought into
// LDS by LDS-DMA in one burst.  For the decoder- and query-side projections of training (M = 1280 / 2048 rows) and the greedy
// step (M = batch) the 128x128 kernel runs 8-40 workgroups, each walking its K tiles behind a two-tile prefetch: one exposed
// L2 / HBM round trip per tile, 16-35 us per launch for < 1 GFLOP.  Here every byte of the panel is requested up front
// (32 DMAs per wave, counted waits release the K tiles in order), four times as many workgroups exist, and the launch is one
// memory round trip + 8 MFMAs per K tile and wave.
// Images, swizzles and fragment reads are those of the 8-wave kernel (gemm8w.inc, Op<>): k-contiguous [64 rows][128 B] with
// chunk c of row r at slot c ^ ((r >> 1) & 7); k-major pieces of [8 k-rows][64 columns] read by ds_read_b64_tr_b16.
// Scope: bf16 operands, M % 64 == N % 64 == 0, K % 64 == 0, K tiles per split <= 10, unbatched, 16-byte aligned; every epilogue
// word of case_gemm (per-element form), split-K as f32 atomics.
namespace gemm_sm {

using gemm_t8w::dma16;
using gemm_t8w::i32x4;
using gemm_t8w::make_rsrc;
using gemm_t8w::Op;

constexpr int TM = 64, TN = 64, BKE = 64, NTHR = 256, MAXKT = 10;
constexpr int IMG = 8192, KT_BYTES = 2 * IMG;

template <bool KMAJOR>
__device__ __forceinline__ void piece_voff(int p, int l, int64_t ld, unsigned& v) {
  if constexpr (!KMAJOR) {
    const int r = p * 8 + (l >> 3);  // row of the 64-row tile; slot l & 7 holds chunk (l & 7) ^ ((row >> 1) & 7)
    v = (unsigned)(r * ld * 2 + (((l & 7) ^ ((r >> 1) & 7)) * 16));
  } else {
    const int j = l >> 3, f = ((j >> 1) & 1) + 2 * (p & 1);  // k-block p of the K tile, k-row j
    v = (unsigned)((p * 8 + j) * ld * 2 + (((l & 7) ^ (2 * f)) * 16));
  }
}

// LN = true (case_gemm_ln): the A panel is normalised in LDS before the MFMA loop (K = 512 = 8 K tiles, A k-contiguous).
template <typename OutT, bool AK, bool BK_, bool LN = false>
__global__ __launch_bounds__(NTHR) void gemm_small_kernel(const Args g, const int epi, const int tiles_m, const int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  const int per_slab = tiles_m * tiles_n;
  const int pid = blockIdx.x, in_slab = pid % per_slab, split = pid / per_slab;
  const int tm = in_slab / tiles_n, tn = in_slab - tm * tiles_n;
  const int64_t m0 = (int64_t)tm * TM, n0 = (int64_t)tn * TN;
  const int kt_total = (int)(g.K / BKE);
  const int kt_begin = split * g.k_tiles_per_split, kt_end = min(kt_begin + g.k_tiles_per_split, kt_total);
  const int nk = kt_end - kt_begin;

  const i32x4 rsa = make_rsrc(Op<AK>::origin(reinterpret_cast<const bf16_t*>(g.A), g.lda, m0, (int64_t)kt_begin * BKE));
  const i32x4 rsb = make_rsrc(Op<BK_>::origin(reinterpret_cast<const bf16_t*>(g.B), g.ldb, n0, (int64_t)kt_begin * BKE));
  unsigned va[2], vb[2];
  piece_voff<AK>(wave, l, g.lda, va[0]);
  piece_voff<AK>(wave + 4, l, g.lda, va[1]);
  piece_voff<BK_>(wave, l, g.ldb, vb[0]);
  piece_voff<BK_>(wave + 4, l, g.ldb, vb[1]);
  const unsigned kga = Op<AK>::kt_goff(g.lda), kgb = Op<BK_>::kt_goff(g.ldb);
  const unsigned wv = __builtin_amdgcn_readfirstlane(wave);
  // the whole panel, K tile by K tile: 4 DMAs per wave and tile (pieces wave, wave + 4 of each operand image)
  for (int kt = 0; kt < nk; ++kt) {
    const unsigned sb = lds0 + kt * KT_BYTES;
    dma16(rsa, va[0], kt * kga, sb + wv * 1024);
    dma16(rsa, va[1], kt * kga, sb + (wv + 4) * 1024);
    dma16(rsb, vb[0], kt * kgb, sb + IMG + wv * 1024);
    dma16(rsb, vb[1], kt * kgb, sb + IMG + (wv + 4) * 1024);
  }
  Op<AK> fa;
  Op<BK_> fb;
  fa.init(l);
  fb.init(l);
  const int la[2] = {fa.lane_base_of(wr, 0), fa.lane_base_of(wr, 1)}, lb[2] = {fb.lane_base_of(wc, 0), fb.lane_base_of(wc, 1)};
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

  if constexpr (LN && !AK) {
    // gamma | beta (2 x 2 KiB) behind the panel: one 16-byte load per thread, issued while the DMAs are in flight (the first build read
    // them from global memory chunk by chunk -- 64 dependent 16-byte loads per thread -- and ran ~8 us LONGER per launch than the
    // LayerNorm launch it replaced)
    float* gb = reinterpret_cast<float*>(smem + nk * KT_BYTES);
    {
      const float4 t4 = tid < 128 ? reinterpret_cast<const float4*>(g.ln_gamma)[tid] : reinterpret_cast<const float4*>(g.ln_beta)[tid - 128];
      reinterpret_cast<float4*>(gb)[tid] = t4;
    }
    // LayerNorm of the 64 A rows in place.  Four threads per row, each owns two K tiles (16 chunks of 8 features); chunk c of row r of K
    // tile kt sits at kt * KT_BYTES + r * 128 + ((c ^ ((r >> 1) & 7)) << 4) (the DMA's source swizzle).  Arithmetic as ln_fwd_vec_kernel:
    // mean, then the sum of squared deviations, both in f32; (x - mu) * rstd * gamma + beta rounded to bf16 once.
    __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0): this wave's share of the panel has landed, its gamma / beta words are written
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    const int r = tid >> 2, qd = tid & 3, sw = (r >> 1) & 7;
    float v[16][8];
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int kt = 2 * qd + (u >> 3), c = u & 7;
      Vec16<bf16_t>::load(reinterpret_cast<const bf16_t*>(smem + kt * KT_BYTES + r * 128 + ((c ^ sw) << 4)), v[u]);
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += v[u][e];
    }
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    const float mu = sum * (1.f / 512.f);
    float sq = 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u)
#pragma unroll
      for (int e = 0; e < 8; ++e) sq += (v[u][e] - mu) * (v[u][e] - mu);
    sq += __shfl_xor(sq, 1, 64);
    sq += __shfl_xor(sq, 2, 64);
    const float rs = rsqrtf(sq * (1.f / 512.f) + g.ln_eps);
    bf16_t* lo = (tn == 0 && g.ln_out) ? reinterpret_cast<bf16_t*>(g.ln_out) + (m0 + r) * 512 : nullptr;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int kt = 2 * qd + (u >> 3), c = u & 7, f = kt * 64 + c * 8;
      float gm[8], bt[8], o[8];
      Vec16<float>::load(gb + f, *reinterpret_cast<float(*)[4]>(gm));
      Vec16<float>::load(gb + f + 4, *reinterpret_cast<float(*)[4]>(gm + 4));
      Vec16<float>::load(gb + 512 + f, *reinterpret_cast<float(*)[4]>(bt));
      Vec16<float>::load(gb + 512 + f + 4, *reinterpret_cast<float(*)[4]>(bt + 4));
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (v[u][e] - mu) * rs * gm[e] + bt[e];
      Vec16<bf16_t>::store(reinterpret_cast<bf16_t*>(smem + kt * KT_BYTES + r * 128 + ((c ^ sw) << 4)), o);
      if (lo) Vec16<bf16_t>::store(lo + f, o);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the normalised rows are written (the loop's first barrier publishes them)
  }
  for (int kt = 0; kt < nk; ++kt) {
    // K tile kt has landed once at most 4 (nk - 1 - kt) of this wave's DMAs are outstanding (vmcnt is a 6-bit count: nk <= 10)
    if constexpr (LN) {
      if (kt == 0) {  // everything landed before the prologue; the stores of ln_out may stay in flight
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
    } else
    switch (nk - 1 - kt) {
      case 0: __builtin_amdgcn_s_waitcnt(0x0f70); break;   // vmcnt(0)
      case 1: __builtin_amdgcn_s_waitcnt(0x0f74); break;   // 4
      case 2: __builtin_amdgcn_s_waitcnt(0x0f78); break;   // 8
      case 3: __builtin_amdgcn_s_waitcnt(0x0f7c); break;   // 12
      case 4: __builtin_amdgcn_s_waitcnt(0x4f70); break;   // 16
      case 5: __builtin_amdgcn_s_waitcnt(0x4f74); break;   // 20
      case 6: __builtin_amdgcn_s_waitcnt(0x4f78); break;   // 24
      case 7: __builtin_amdgcn_s_waitcnt(0x4f7c); break;   // 28
      case 8: __builtin_amdgcn_s_waitcnt(0x8f70); break;   // 32
      default: __builtin_amdgcn_s_waitcnt(0x8f74); break;  // 36
    }
    if constexpr (!LN) {
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    }
    const char* st = smem + kt * KT_BYTES;
    bf16x8 a[2][2], b[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        a[i][kh] = fa.frag_at(st, la[i], wr * 2 + i, kh);
        b[i][kh] = fb.frag_at(st + IMG, lb[i], wc * 2 + i, kh);
      }
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][kh], b[j][kh], acc[i][j], 0, 0, 0);
  }

  // per-element epilogue (the problem is small: store width does not matter); accumulator element e of block (i, j) is
  // C[32 wr + 16 i + 4 (l >> 4) + e][32 wc + 16 j + (l & 15)]
  gemm_w4::Epilogue<bf16_t, OutT> E;
  E.C = reinterpret_cast<OutT*>(g.C); E.aux = reinterpret_cast<const bf16_t*>(g.aux); E.aux_out = reinterpret_cast<bf16_t*>(g.aux_out);
  E.bias_row = g.bias_row; E.bias_col = g.bias_col; E.ldc = g.ldc; E.ld_aux = g.ld_aux; E.M = g.M; E.N = g.N;
  E.alpha = g.alpha; E.drop_p = g.drop_p; E.drop_scale = (epi & CASE_EPI_DROPOUT) ? 1.f / (1.f - g.drop_p) : 1.f;
  E.seed = g.seed; E.rng_base = g.offset + rng_base_of(g.state);
  E.epi = (split == 0) ? epi : (epi & ~(CASE_EPI_BIAS_COL | CASE_EPI_BIAS_ROW));  // split-K: the biases arrive once (as in gemm_impl.inc)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t col = n0 + wc * 32 + j * 16 + (l & 15);
      const float bc = (E.epi & CASE_EPI_BIAS_COL) ? g.bias_col[col] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) E.emit(acc[i][j][e], m0 + wr * 32 + i * 16 + 4 * (l >> 4) + e, col, bc);
    }
}

template <typename OutT, bool LN>
int launch(const Args& a, int epi, bool ak, bool bk, hipStream_t s) {
  const int tiles_m = (int)(a.M / TM), tiles_n = (int)(a.N / TN);
  const int64_t nwg = (int64_t)tiles_m * tiles_n * a.split_k;
  const int lds = a.k_tiles_per_split * KT_BYTES + (LN ? 4096 : 0);
  const dim3 grid((unsigned)nwg), block(NTHR);
#define GO(AKV, BKV)                                                                                       \
  do {                                                                                                     \
    if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_small_kernel<OutT, AKV, BKV, LN>), \
                                           hipFuncAttributeMaxDynamicSharedMemorySize, LN ? 8 * KT_BYTES + 4096 : MAXKT * KT_BYTES) != hipSuccess) \
      return case_set_error(CASE_E_LAUNCH, "case_gemm: cannot reserve %d bytes of LDS", LN ? 8 * KT_BYTES + 4096 : MAXKT * KT_BYTES); \
    hipLaunchKernelGGL((gemm_small_kernel<OutT, AKV, BKV, LN>), grid, block, lds, s, a, epi, tiles_m, tiles_n); \
  } while (0)
  if constexpr (LN) {  // k-contiguous A only
    if (!bk) GO(false, false);
    else GO(false, true);
  } else {
    if (!ak && !bk) GO(false, false);
    else if (!ak && bk) GO(false, true);
    else if (ak && !bk) GO(true, false);
    else GO(true, true);
  }
#undef GO
  return case_check_launch("case_gemm");
}

}  // namespace gemm_sm
