/*
 * case_hip.h -- C ABI of libcase_hip.so, the MI355X (gfx950) kernel library behind the CaSE_RG
 * encoder-decoder hot path.
 *
 * The reference (PengjieRen/CaSE_RG) has no native layer: every operation below replaces an ATen op
 * chain called from the reference's Python modules; the chain is cited as <file>:<line> relative to
 * the reference root.  Host code (case_rg_amd/, Python) binds these entry points with ctypes
 * (case_rg_amd/_abi.py); INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers owned by the caller
 *     (PyTorch caching allocator).  The library never allocates, frees, retains a pointer or
 *     synchronises: every call only enqueues work on the caller's stream, so the whole path is
 *     hipGraph-capturable.
 *   - return 0 on success, a negative CASE_E_* code otherwise; case_last_error() gives the text.
 *     Launch errors are read with hipGetLastError() right after enqueue (no sync).
 *   - dtype arguments are case_dtype_t: activations are f32 (parity mode, exact-f32 MFMA) or bf16
 *     (throughput mode, bf16 MFMA with f32 accumulate); parameters, statistics, losses and
 *     gradients of parameters are always f32.
 *   - masks are uint8 (torch.bool storage), 1 = VALID token unless a name says "pad".
 */
#ifndef CASE_HIP_H
#define CASE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* case_stream_t; /* hipStream_t */

typedef enum { CASE_F32 = 0, CASE_BF16 = 1 } case_dtype_t;

enum {
  CASE_OK = 0,
  CASE_E_ARG = -1,         /* bad shape / stride / null pointer */
  CASE_E_UNSUPPORTED = -2, /* combination not built */
  CASE_E_LAUNCH = -3       /* hipGetLastError() after enqueue */
};

/* ABI generation.  case_version() returns the CASE_ABI_VERSION the library was built from; a binder compares it with the header it was
 * written against (case_rg_amd/_abi.py refuses any other library).  Bumped with every struct or signature change:
 *   100 round 1 | 200 round 2 (case_gemm_dw_bias, decode, optimizer) | 300 round 3 (CaseOptTensor 56 -> 64 bytes, K16 / K17)
 *   400 round 4 (K18 / K19 resident attention, case_attention_bwd scratch = 2 N heads Lq floats, workspace query, reserved CUs)
 *   500 round 5 (K21 case_attention_decode_mqa, K22 case_pointer_attend_decode, K23 case_pointer_head_decode, case_gemm_ln)
 *   600 round 6 (CaseStepState: the per-step scalars -- dropout counter base, Adam step size / bias correction -- may live in caller-owned
 *       DEVICE memory instead of riding in the arguments, so that a hipGraph-captured training step draws new masks and takes the right
 *       Adam step on every replay; `state` members / arguments on every dropout site and on case_optim_adam_ema; case_step_advance;
 *       K8 case_interaction_fwd). */
#define CASE_ABI_VERSION 600
int case_version(void);
/* what the build contains, as a bit mask */
enum {
  CASE_FEAT_GEMM_256 = 1u << 0,        /* 256 x 256 eight-wave GEMM tiling (+ case_gemm_dw_bias) */
  CASE_FEAT_GEMM_SMALL = 1u << 1,      /* 64 x 64 small-problem tiling */
  CASE_FEAT_ENCODER_CHAIN = 1u << 2,   /* K16 case_encoder_chain */
  CASE_FEAT_ATTN_SCORES = 1u << 3,     /* K17 case_attention_scores_* / case_attention_product */
  CASE_FEAT_ATTN_DECODE = 1u << 4,     /* case_attention_decode */
  CASE_FEAT_OPTIM = 1u << 5,           /* K15 case_optim_* */
  CASE_FEAT_ATTN_RESIDENT = 1u << 6,   /* K18 / K19 behind case_attention_fwd / _bwd */
  CASE_FEAT_RESERVED_CUS = 1u << 7,    /* case_set_reserved_cus */
  CASE_FEAT_GEMM_DW_SLABS = 1u << 8,   /* case_gemm_dw_slabs: atomics-free, run-to-run deterministic split-K weight gradients */
  CASE_FEAT_DECODER_CHAIN = 1u << 9,   /* (reserved: K20 case_decoder_chain, retired in round 5 -- never set) */
  CASE_FEAT_ATTN_DECODE_MQA = 1u << 10, /* K21 case_attention_decode_mqa */
  CASE_FEAT_POINTER_DECODE = 1u << 11,  /* K22 case_pointer_attend_decode / case_additive_key_exp */
  CASE_FEAT_POINTER_HEAD = 1u << 12,    /* K23 case_pointer_head_decode */
  CASE_FEAT_GEMM_LN = 1u << 13,         /* case_gemm_ln: LayerNorm prologue of the small-problem GEMM */
  CASE_FEAT_STEP_STATE = 1u << 14,      /* ABI 600: CaseStepState on the dropout sites and the optimizer, case_step_advance */
  CASE_FEAT_INTERACTION = 1u << 15,     /* K8 case_interaction_fwd: the dual co-attention as two kernels */
  CASE_FEAT_ATTN_DECODE_APPEND = 1u << 16, /* case_attention_decode_append: the greedy step's cache append inside the attention launch */
  CASE_FEAT_LINEAR_SKINNY = 1u << 17,     /* case_linear_skinny */
  CASE_FEAT_BEAM_DECODE = 1u << 18,       /* K24-K27 case_pointer_head_beam / case_beam_advance / case_beam_gather / case_beam_backtrack */
  CASE_FEAT_SAMPLE_DECODE = 1u << 19,     /* K28 case_pointer_head_sample */
  CASE_FEAT_POINTER_SCORE = 1u << 20,     /* K29 case_pointer_head_score */
  CASE_FEAT_CONSENSUS = 1u << 21,         /* K30 / K31 case_lcs_pairs / case_consensus_pick */
  CASE_FEAT_NGRAM_BAN = 1u << 22,         /* K32 / K33 case_ngram_ban, the `_ban` forms of K23 / K24 / K25 / K28, case_remove_duplicate_ids */
  CASE_FEAT_NGRAM_COUNTS = 1u << 23,      /* K34 / K35 case_ngram_counts / case_bleu_scores */
  CASE_FEAT_RANK_METRICS = 1u << 24,      /* K36 case_rank_metrics */
  CASE_FEAT_POINTER_HEAD_WIDE = 1u << 25, /* the global-row forms of K23 / K24 / K28: case_pointer_head_decode_wide / _beam_wide / _sample_wide */
  CASE_FEAT_DECODE_RULES = 1u << 26,      /* min_length / banned ids / beam length penalty: the `_rules` forms of K23 / K24 / K25 / K28, case_row_rules */
  CASE_FEAT_TOKEN_LABELS = 1u << 27,      /* K37 / K38 case_token_labels / case_token_select */
  CASE_FEAT_COPY_ATTRIBUTION = 1u << 28,  /* K39 case_copy_attribution */
  CASE_FEAT_METEOR = 1u << 29,            /* K40 case_meteor */
  CASE_FEAT_RISK_TRAIN = 1u << 30,        /* K41 / K42 case_pointer_head_score_stats / _bwd, case_sequence_risk */
  CASE_FEAT_ROUGE_N = 1u << 31            /* K43 / K44 case_ngram_distinct / case_rouge_n_scores.  The LAST free bit of the 32-bit mask: the
                                             next feature needs a second query (or a generation), not a 33rd bit */
};
uint32_t case_abi_features(void);
const char* case_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Device-resident step state (round 6).  A training step of common/CumulativeTrainer.py:52-78 has three kinds of scalars that change
 * from step to step: the position of the dropout counter stream (every nn.Dropout / F.dropout site: common/TransformerEncoder.py:68,72,75
 * ...), the learning rate the scheduler set (CaSE/Run.py:28) and Adam's bias corrections (torch.optim.Adam, CaSE/Run.py:27).  As kernel
 * ARGUMENTS they are frozen into a captured hipGraph -- a replayed step would redraw the same masks.  Every entry point that takes
 * (seed, offset) or the Adam scalars therefore also takes a nullable `const CaseStepState* state`, a DEVICE pointer to 64 caller-owned
 * bytes that the kernels read when they run:
 *   - dropout sites hash (seed, offset + state->rng_base + element index): the caller numbers the sites of ONE step from offset 0 and
 *     moves rng_base by the step's consumption between steps (rng_base must stay even: the kernels hash element pairs);
 *   - case_optim_adam_ema takes step_size / bc2_sqrt from the state instead of the table entries.
 * state == NULL is the round-5 behaviour (arguments only).  The caller writes the struct -- a 64-byte hipMemcpyAsync from pinned memory
 * ahead of the step (exact for any scheduler), or case_step_advance on the stream (no host involvement per step).  The library only
 * reads it; like every pointer here it is never retained.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  uint64_t rng_base; /* added to the `offset` of every dropout site that is given this state; even */
  float step_size;   /* lr / (1 - beta1^step)   -- as CaseOptTensor.step_size */
  float bc2_sqrt;    /* sqrt(1 - beta2^step)    -- as CaseOptTensor.bc2_sqrt */
  float lr;          /* the learning rate step_size was formed from (read by case_step_advance only) */
  int32_t step;      /* optimizer steps taken, INCLUDING the one these scalars belong to */
  uint64_t reserved[5];
} CaseStepState;     /* 64 bytes */
int case_sizeof_step_state(void);
/* One single-thread launch that moves the state to the next step: step += 1, rng_base += rng_stride (even), and, with the state's lr,
 * step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step), formed in double and rounded to f32 once (what
 * case_rg_amd/optim.py does on the host).  For replay loops that never return to the host; a scheduler that changes lr writes state->lr. */
int case_step_advance(CaseStepState* state, uint64_t rng_stride, double beta1, double beta2, case_stream_t stream);

/* Compute units the persistent kernels (256 x 256 GEMM, K16 .. K19) leave free -- the ONE piece of mutable library configuration:
 * with world_size > 1 RCCL's kernels must be resident beside them for the gradient all-reduce to overlap backward
 * (common/CumulativeTrainer.py:45-47).  0 .. 128, rounded so that the grids stay whole XCD rounds; initial value from the environment
 * variable CASE_RESERVE_CUS (default 0). */
int case_set_reserved_cus(int n);
int case_get_reserved_cus(void);

/* Caller-owned scratch of the entry points that need one, in bytes:
 *   CASE_WS_ATTENTION_SPLITKV  desc = CaseAttnDesc*, arg = ksplit     (workspace of case_attention_fwd_splitkv)
 *   CASE_WS_ATTENTION_BWD      desc = CaseAttnDesc*                   (the `delta` argument of case_attention_bwd)
 *   CASE_WS_OPTIM_SUMSQ        arg = nchunks                          (the `partials` argument of case_optim_sumsq)
 *   CASE_WS_ENCODER_CHAIN_PACK                                        (the packed weights of case_encoder_chain_pack)
 *   CASE_WS_GEMM_DW_SLABS      desc = CaseGemmDesc*                   (the `slabs` argument of case_gemm_dw_slabs; 0 = no split)
 * negative = CASE_E_ARG. */
typedef enum { CASE_WS_ATTENTION_SPLITKV = 1, CASE_WS_ATTENTION_BWD = 2, CASE_WS_OPTIM_SUMSQ = 3, CASE_WS_ENCODER_CHAIN_PACK = 4, CASE_WS_GEMM_DW_SLABS = 5 } case_workspace_kind_t;
int64_t case_workspace_bytes(int32_t kind, const void* desc, int64_t arg);

/* ---------------------------------------------------------------------------------------------
 * K3  strided-batched GEMM on MFMA:   C = epilogue(alpha * op(A) op(B))
 * replaces every nn.Linear / MHA in_proj / out_proj / bmm on the path:
 *   common/TransformerEncoder.py:67,72  common/TransformerDecoder.py:77,81,86
 *   common/TransformerBlock.py:26,28-29  common/Interaction.py:36,50-54  common/BilinearAttention.py:31,34,57
 *   CaSE/Model.py:34,36,43,242  (and their autograd backward)
 * A is M x K, B is N x K ("NT": C = A B^T) unless *_kmajor says the operand is stored K x M / K x N.
 * Batch index b in [0, batch1*batch2): b1 = b / batch2, b2 = b % batch2 (b2 = attention head);
 * operand offset = b1*s?1 + b2*s?2 elements.
 * ------------------------------------------------------------------------------------------- */
enum {
  CASE_EPI_BIAS_COL = 1,   /* + bias_col[n] (f32)                                   */
  CASE_EPI_BIAS_ROW = 2,   /* + bias_row[b*M + m] (f32)  (Interaction rank-1 terms) */
  CASE_EPI_GELU = 4,       /* erf GELU; pre-activation also stored to aux_out if non-null */
  CASE_EPI_RELU = 8,
  CASE_EPI_RESIDUAL = 16,  /* + aux[m, n]                                           */
  CASE_EPI_MUL_DGELU = 32, /* * gelu'(aux[m, n])   (backward through GELU)          */
  CASE_EPI_MUL_DRELU = 64, /* * (aux[m, n] > 0)    (backward through ReLU; aux = activation output) */
  CASE_EPI_ATOMIC = 128,   /* split-K: atomicAdd f32 into pre-zeroed C (out_dtype must be f32) */
  CASE_EPI_DROPOUT = 256   /* * keep(seed, offset + (b*M + m)*N + n) / (1 - drop_p); nn.Dropout / F.dropout sites:
                              TransformerEncoder.py:68,72,75 TransformerDecoder.py:78,82,86,88 TransformerBlock.py:27-28
                              CaSE/Model.py:34.  The same flag regenerates the mask in the backward GEMM. */
};
/* epilogue order: alpha*acc + bias -> GELU|RELU -> MUL_DGELU|MUL_DRELU -> DROPOUT -> + RESIDUAL */

typedef struct {
  int64_t M, N, K;
  int64_t lda, ldb, ldc, ld_aux; /* leading dimensions in elements */
  int64_t batch1, batch2;
  int64_t sa1, sa2, sb1, sb2, sc1, sc2, saux1, saux2;
  int32_t a_kmajor, b_kmajor;
  int32_t in_dtype;  /* dtype of A, B, aux, aux_out */
  int32_t out_dtype; /* dtype of C */
  int32_t epilogue;  /* CASE_EPI_* mask */
  int32_t split_k;   /* >= 1 */
  int32_t tile;      /* 0 = pick the tiling per call (cost model); 128 = the 128x128 tiling; 256 = the 256x256 persistent tiling,
                        64 = the small-problem tiling (whole K panel in LDS) whenever the call is eligible (otherwise 128x128) */
  float alpha;
  float drop_p;
  uint64_t seed, offset;
  const CaseStepState* state; /* nullable: offset += state->rng_base on the device (ABI 600) */
} CaseGemmDesc;

int case_gemm(const CaseGemmDesc* d, const void* A, const void* B, void* C, const float* bias_col,
              const float* bias_row, const void* aux, void* aux_out, case_stream_t stream);
/* LayerNorm as a PROLOGUE of the small-problem GEMM (round 5): C = epilogue(LN(A) B^T), ln_out = LN(A) -- the greedy step's
 * LN1 -> QKV, LN2 -> cross-attention query and LN3 -> feed-forward pairs (common/TransformerDecoder.py:76-89 at one position per sequence)
 * as one launch each.  d describes the GEMM as for case_gemm (bf16, k-contiguous A with K = lda = 512, M and N multiples of 64, unsplit,
 * unbatched; epilogue words BIAS_COL / GELU / RELU / RESIDUAL); gamma / beta f32 [512]; ln_out [M, 512] bf16 or null.  The statistics are
 * the two-pass f32 mean / variance of case_layernorm_fwd.  CASE_E_UNSUPPORTED for anything else (run case_layernorm_fwd + case_gemm). */
int case_gemm_ln(const CaseGemmDesc* d, const void* A, const float* gamma, const float* beta, float eps, void* ln_out, const void* B, void* C,
                 const float* bias_col, const void* aux, case_stream_t stream);

/* case_gemm owns three tilings: 128x128 (every shape / dtype / batch), 256x256 (bf16, M % 256 == N % 256 == 0,
 * K % 64 == 0, unbatched, 16-byte aligned; eight waves, operands by LDS-DMA, persistent: csrc/gemm8w.inc) and 64x64 for small
 * problems (bf16, multiples of 64, <= 10 K tiles per split, the 128x128 grid smaller than the chip: csrc/gemm_small.inc).  CaseGemmDesc.tile selects per call; results
 * of the tilings agree to f32 summation order.  case_gemm_tile_for() returns the tile edge (64, 128 or 256) case_gemm would
 * launch for exactly these arguments (or a negative CASE_E_* code): a pure function of its arguments, no launch, no state --
 * bench.py uses it to attribute each launch to the kernel name rocprofv3 reports. */
/* Weight-gradient GEMM that also produces the bias gradient (replaces a separate pass over dY, case_colsum; reference:
 * autograd of nn.Linear, e.g. common/TransformerBlock.py:13-14): C[M, N] += op(A) op(B) as case_gemm with the bare ATOMIC epilogue,
 * and d_bias[m] += sum_k op(A)[m, k] (f32 [M], pre-zeroed, atomics).  Only for calls the 256x256 tiling takes with a k-major A
 * (case_gemm_tile_for(...) == 256, d->a_kmajor): CASE_E_UNSUPPORTED otherwise, and the caller runs case_gemm + case_colsum. */
int case_gemm_dw_bias(const CaseGemmDesc* d, const void* A, const void* B, void* C, float* d_bias, case_stream_t stream);
/* The same weight-gradient GEMM without atomics on C: every K split stores its partial [M, N] f32 tile into its own slab of the
 * caller's workspace (16-byte aligned, >= case_gemm_dw_slab_bytes(d) bytes, free again when the stream has passed the call) and a
 * second launch adds the slabs to C in split order -- C[M, N] += op(A) op(B), bit-identical from run to run.  For the small,
 * deeply split outputs (a 512 x 512 weight gradient over 122,880 tokens = 64 splits) it is also ~2x faster: 64 MiB of f32 red ops
 * retire at ~1.3 TB/s, plain stores + one read at HBM rate.  d_bias may be NULL; otherwise as in case_gemm_dw_bias (atomics, [M]).
 * Needs the 256x256 tiling, split_k > 1 after clamping, ldc == N; CASE_E_UNSUPPORTED otherwise.  case_gemm_dw_slab_bytes returns
 * 0 when the clamped split is 1. */
int case_gemm_dw_slabs(const CaseGemmDesc* d, const void* A, const void* B, void* C, float* d_bias, void* slabs, int64_t slab_bytes,
                       case_stream_t stream);
int64_t case_gemm_dw_slab_bytes(const CaseGemmDesc* d);

int case_gemm_tile_for(const CaseGemmDesc* d, const void* A, const void* B, const void* C, const float* bias_col,
                       const void* aux, const void* aux_out);

/* ---------------------------------------------------------------------------------------------
 * K1  embedding gather * sqrt(H) + sinusoid position (+ dropout)
 *   common/TransformerSeqEncoderDecoder.py:21,36  common/PositionalEmbedding.py:44-48  CaSE/Model.py:21,67
 * ids int64 [rows]; position of a row = row % seq_len; table f32 [V, H]; pe f32 [>= seq_len, H].
 * bwd: d_table[id] += scale * d_out[row] (f32 atomics; id 0 = padding_idx receives nothing).
 * ------------------------------------------------------------------------------------------- */
int case_embed_pos_fwd(const int64_t* ids, const float* table, const float* pe, void* out, int64_t rows,
                       int64_t seq_len, int64_t H, int64_t vocab, float scale, float drop_p, uint64_t seed,
                       uint64_t offset, const CaseStepState* state, int32_t dtype, case_stream_t stream);
int case_embed_pos_bwd(const int64_t* ids, const void* d_out, float* d_table, int64_t rows, int64_t H,
                       int64_t vocab, float scale, float drop_p, uint64_t seed, uint64_t offset, const CaseStepState* state,
                       int32_t dtype, case_stream_t stream);

/* stand-alone PositionalEmbedding.forward (common/PositionalEmbedding.py:44-48): y = x*scale + pe[row % seq_len]
 * (pe may be null: plain scaling, used as its backward) */
int case_scale_add_rows(const void* x, const float* pe, void* y, int64_t rows, int64_t seq_len, int64_t H, float scale,
                        int32_t dtype, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K2  LayerNorm (eps inside sqrt, affine), optional fused input add: y = LN(x + x2)
 *   common/TransformerEncoder.py:66,70  common/TransformerDecoder.py:76,80,84  common/TransformerBlock.py:25,28
 *   CaSE/Model.py:69,84,209-210
 * mean / rstd f32 [rows] are saved for backward.  bwd accumulates d_gamma / d_beta with f32 atomics
 * into pre-zeroed buffers; dx is also the gradient of x2 when the add was fused.
 * ------------------------------------------------------------------------------------------- */
int case_layernorm_fwd(const void* x, const void* x2, const float* gamma, const float* beta, void* y, float* mean,
                       float* rstd, int64_t rows, int64_t cols, float eps, int32_t dtype, case_stream_t stream);
/* dx_add (nullable, same layout as dx): a second gradient of the same input -- its residual use, as in
 * x + MHA(LN(x)) of common/TransformerBlock.py:26-27 -- added to dx in the same pass. */
int case_layernorm_bwd(const void* dy, const void* x, const void* x2, const float* gamma, const float* mean,
                       const float* rstd, void* dx, const void* dx_add, float* d_gamma, float* d_beta, int64_t rows,
                       int64_t cols, int32_t dtype, case_stream_t stream);
/* The backward of LN(dropout(x W^T + b) + r) -- out-projection / feed-forward followed by a LayerNorm, common/TransformerEncoder.py:68-69,
 * 72-75, common/TransformerBlock.py:27-28 -- with TWO outputs: dx (the gradient of the LayerNorm's input = of the residual r) and
 * dx_dropped = mask * dx / (1 - p), the gradient of the Linear's pre-dropout output that its dX / dW GEMMs read.  The mask is case_dropout's
 * (element index row * cols + column behind (seed, offset)) applied to the ROUNDED dx: the same bits as case_layernorm_bwd followed by
 * case_dropout, one tensor pass less.  Rows of k x 64 lanes x 16 bytes (k <= 8), no x2 / dx_add; CASE_E_UNSUPPORTED otherwise.
 * `offset` must be EVEN (the mask is drawn per element pair; CASE_E_ARG otherwise -- case_dropout itself accepts odd offsets). */
int case_layernorm_bwd_dropout(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
                               void* dx_dropped, float* d_gamma, float* d_beta, int64_t rows, int64_t cols, float p, uint64_t seed,
                               uint64_t offset, const CaseStepState* state, int32_t dtype, case_stream_t stream);
/* The backward of LN(G), G = concat5(E, A1, A2) = [E | A1 | A2 | E o A1 | E o A2] with padded rows zeroed (common/Interaction.py:65-72 feeding
 * common/TransformerBlock.py:25), fused with the backward of the concatenation: dE, dA1, dA2 [rows, H] come out directly, dG (5H wide)
 * is never written.  x = G as the forward wrote it; dx_add (nullable, [rows, 5H]) a second gradient of G (its residual use, block :27).
 * dG is rounded to bf16 before the products, as the two-kernel path (case_layernorm_bwd + case_concat5_bwd) stores it.  bf16, H = 512
 * only; CASE_E_UNSUPPORTED otherwise. */
int case_layernorm_bwd_concat5(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dx_add,
                               const void* e, const void* a1, const void* a2, const uint8_t* row_valid, void* de, void* da1, void* da2,
                               float* d_gamma, float* d_beta, int64_t rows, int64_t H, int32_t dtype, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K4/K5/K6 (softmax stage) and the masked softmaxes of K7/K8/K10/K11
 *   torch MHA softmax (common/TransformerEncoder.py:67, TransformerDecoder.py:77,81, TransformerBlock.py:26),
 *   common/Interaction.py:43-47, common/BilinearAttention.py:16-19, CaSE/Model.py:34,39
 * x is [outer, inner, R, C] contiguous; softmax over C.  col_valid u8 [outer, C] (or null), row_valid u8
 * [outer, R] (or null), causal: column > row masked.  A row with no admissible column yields exact 0
 * (the reference's NaN -> masked_fill(0) path) and zero gradient.
 * p_out: probabilities (saved for backward); y_out: after dropout (may alias p_out when drop_p == 0).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t outer, inner, R, C;
  int32_t causal;
  int32_t in_dtype, out_dtype;
  float drop_p;
  uint64_t seed, offset;
  const CaseStepState* state; /* nullable: offset += state->rng_base on the device (ABI 600) */
} CaseSoftmaxDesc;

int case_softmax_fwd(const CaseSoftmaxDesc* d, const void* x, const uint8_t* col_valid, const uint8_t* row_valid,
                     void* p_out, void* y_out, case_stream_t stream);
int case_softmax_bwd(const CaseSoftmaxDesc* d, const void* dy, const void* p, void* dx, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K4 / K5 / K6  fused multi-head attention (bf16): softmax(scale * Q K^T + masks) V without materialising the scores
 *   nn.MultiheadAttention call sites: common/TransformerEncoder.py:67, common/TransformerBlock.py:26 (self-attention
 *   with key padding, head_dim 64 and 5H/8 = 320), common/TransformerDecoder.py:77 (causal + key padding), :81 (cross
 *   attention over the S = P*Lp token memory).
 * q / k / v point at the first head's columns inside the (packed) projection tensors: element (n, l, head, j) is at
 * base[n*s? + l*ld? + head*head_dim + j].  key_valid u8 [N, Lk] (1 = token) or null; causal masks key > query.
 * out bf16 [N, Lq, heads*head_dim] (row stride ldo, sequence stride so); lse f32 [N, heads, Lq] is saved for backward.
 * Dropout acts on the probabilities with the same counter RNG / element index as case_softmax_fwd on [N, heads, Lq, Lk].
 * Backward: delta f32 [N, heads, Lq] is scratch (rowsum(dO * O), written by the call); dq / dk / dv are bf16 slices of
 * the gradient of the packed projections, addressed with the same strides as q / k / v.
 * case_attention_supported(head_dim) != 0 tells whether a head size has a fused FORWARD (32, 64, 96, 160 = 5 x 256 / 8, 320 = 5 x 512 / 8,
 * 480 = 5 x 768 / 8), case_attention_bwd_supported whether it also has a fused backward (32, 64, 96, 160; round 6 dropped 320 / 480, whose
 * training path is K17's saved-probability form); other sizes use the unfused GEMM + softmax path.  Head sizes above
 * 128 split the head dim over 2-3 waves per block of 32 rows (partial score tiles are exchanged through LDS).
 * case_attention_fwd_splitkv: same result for long memories with few (sequence, head) pairs (cfg 5 cross-attention: 40
 * queries x 20 480 keys): the keys are cut into `ksplit` chunks handled by different workgroups, whose unnormalised partials
 * go through the caller-owned `workspace` (size from case_attention_splitkv_workspace) and a merge kernel.  Not causal.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t N, heads, Lq, Lk, head_dim;
  int64_t ldq, ldk, ldv, sq, sk, sv;
  int64_t ldo, so;
  int32_t causal;
  float scale, drop_p;
  uint64_t seed, offset;
  const CaseStepState* state; /* nullable: offset += state->rng_base on the device (ABI 600) */
} CaseAttnDesc;

int case_attention_supported(int64_t head_dim);
int case_attention_fwd(const CaseAttnDesc* d, const void* q, const void* k, const void* v, const uint8_t* key_valid,
                       void* out, float* lse, case_stream_t stream);
int case_attention_splitkv_workspace(const CaseAttnDesc* d, int32_t ksplit, int64_t* bytes);
int case_attention_fwd_splitkv(const CaseAttnDesc* d, const void* q, const void* k, const void* v, const uint8_t* key_valid,
                               void* out, float* lse, void* workspace, int64_t workspace_bytes, int32_t ksplit,
                               case_stream_t stream);
/* Decode step (greedy inference, CaSE/Model.py:94-123 with cached projections): ONE query per sequence (d->Lq == 1) against
 * Lk cached keys / values, no causal mask, no dropout, no LSE (nothing to differentiate).  HBM-bound streaming kernel, one
 * workgroup per (sequence, head); out [N, 1, heads*head_dim].  Rows without a valid key give exact zeros. */
int case_attention_decode_supported(int64_t head_dim);
int case_attention_decode(const CaseAttnDesc* d, const void* q, const void* k, const void* v, const uint8_t* key_valid,
                          void* out, case_stream_t stream);
/* The same step WITH the cache append (round 6; common/TransformerDecoder.py:77 at one position: the reference re-projects the whole prefix, the
 * cached form writes position `pos`'s K / V projections into the layer's caches and attends positions <= pos): the keys / values of position
 * `pos` are read from new_k / new_v (row n at n * new_stride elements, head h at column h * head_dim) instead of the caches and stored into
 * k_cache / v_cache at that position by the workgroup that owns the (sequence, head) slice -- one launch instead of a strided copy + the attention.
 * key_valid must mark `pos` as the caller wants it attended.  CASE_FEAT_ATTN_DECODE_APPEND. */
int case_attention_decode_append(const CaseAttnDesc* d, const void* q, void* k_cache, void* v_cache, const void* new_k, const void* new_v,
                                 int64_t new_stride, int64_t pos, const uint8_t* key_valid, void* out, case_stream_t stream);
/* K21, the decode step's cross-attention over a LONG memory with absorbed projections (round 5): multi-query attention of 8 query rows
 * per item against the RAW memory rows [B, S, 512] (bf16), K = V = memory.  Replaces, for the layers of the passage-memory stack,
 * in_proj(q) -> case_attention_decode over the layer's cached K / V projections -> (common/TransformerDecoder.py:81-82 at one position,
 * CaSE/Model.py:94-123): with qp[b, h, :] = log2(e) / sqrt(d) * Wk_h^T q_h the scores q_h . K_h[j] equal qp_h . mem_j up to a term that
 * is constant over j, and sum_j p_hj V_h[j] = Wv_h (sum_j p_hj mem_j) + bv_h -- the caller applies Wv_h (and its bias) to the result.
 * One stream of S x 512 x 2 bytes per item instead of the two cached projections.  qp [B, 8, 512] bf16 (16-byte aligned), out [B, ldo] bf16
 * (head h at columns 512 h .. 512 h + 511), key_valid [B, S] bytes or null; items without a valid key give exact zeros.  nsplit key
 * ranges per item (case_attention_decode_mqa_splits picks one for (B, S); > 1 needs a workspace of case_attention_decode_mqa_workspace
 * bytes, 16-byte aligned).  bf16, 8 heads, width 512 only. */
int64_t case_attention_decode_mqa_workspace(int64_t B, int64_t S, int32_t nsplit);
int case_attention_decode_mqa_splits(int64_t B, int64_t S);
int case_attention_decode_mqa(const void* qp, const void* mem, const uint8_t* key_valid, void* out, int64_t B, int64_t S, int64_t ldo,
                              int32_t nsplit, void* workspace, int64_t workspace_bytes, case_stream_t stream);
int case_attention_bwd_supported(int64_t head_dim);
/* floats of scratch case_attention_bwd needs behind `delta` (2 N heads Lq: the resident single-pass backward of head_dim 64, K19,
 * keeps -lse / scale and -rowsum(dO * O) per query) */
int64_t case_attention_bwd_scratch_floats(const CaseAttnDesc* d);
int case_attention_bwd(const CaseAttnDesc* d, const void* q, const void* k, const void* v, const uint8_t* key_valid,
                       const void* out, const float* lse, const void* dout, float* delta, void* dq, void* dk, void* dv,
                       case_stream_t stream);

/* K17  probabilities of the GEMM -> softmax -> GEMM attention path (the training path of the head_dim 320 blocks,
 * common/TransformerBlock.py:26; F.multi_head_attention_forward's bmm -> softmax -> dropout -> bmm) with the softmax in the score
 * GEMM: one workgroup holds 128 query rows x all Lk keys, so no score tensor reaches memory.
 *   case_attention_scores_fwd: p = softmax(scale q k^T | key_valid) as bf16 [N, heads, Lq, Lk]; with drop_p > 0 also
 *     p_dropped = keep ? p / (1 - drop_p) : 0 (same counter RNG / element index as case_softmax_fwd); replaces case_gemm (f32
 *     scores) + case_softmax_fwd.  Rows without a valid key give exact zeros.
 *   case_attention_scores_bwd: ds = p (g - rowsum(g p)), g = keep ? (dout v^T) / (1 - drop_p) : 0, bf16 [N, heads, Lq, Lk];
 *     replaces case_gemm (dP) + case_softmax_bwd.  dout is addressed with ldo / so, v with ldv / sv of the descriptor.
 * Scope (case_attention_scores_supported(d) != 0): bf16, head_dim a multiple of 64 and >= 128, Lk <= 384 and a multiple of 8, not causal. */
int case_attention_scores_supported(const CaseAttnDesc* d);
int case_attention_scores_fwd(const CaseAttnDesc* d, const void* q, const void* k, const uint8_t* key_valid, void* p,
                              void* p_dropped, case_stream_t stream);
int case_attention_scores_bwd(const CaseAttnDesc* d, const void* dout, const void* v, const void* p, void* ds,
                              case_stream_t stream);
/* The four batched products around those probabilities at head_dim 320 (F.multi_head_attention_forward's second bmm and the three
 * bmm of its backward): c[n, row, head, 0..319] = alpha * sum_k A[n, head][row, k] * b[n, k, head, 0..319], where A is the [L, L] matrix a
 * (a_transposed = 0: O = Pd V, dQ = alpha dS K) or its transpose (a_transposed = 1: dV = Pd^T dO, dK = alpha dS^T Q).  Element
 * (n, head, r, col) of a at a[n sa_seq + head sa_head + r lda + col]; k-row k of b at b[n sb_seq + head sb_head + k ldb + 0..319];
 * output row at c[n sc_seq + head sc_head + row ldc + 0..319].  M output rows, Kc = contraction length (a multiple of 64, >= 128).
 * One workgroup owns 128 rows x all 320 columns (a is read once); replaces case_gemm's batched 128x128 tiling for these shapes. */
typedef struct {
  int64_t N, heads, M, Kc, head_dim;
  int64_t lda, sa_seq, sa_head;
  int64_t ldb, sb_seq, sb_head;
  int64_t ldc, sc_seq, sc_head;
  int32_t a_transposed;
  float alpha;
} CaseAttnProductDesc;
int case_attention_product_supported(const CaseAttnProductDesc* d);
int case_attention_product(const CaseAttnProductDesc* d, const void* a, const void* b, void* c, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * elementwise / small reductions
 * ------------------------------------------------------------------------------------------- */
/* out = a + b  (residual adds: TransformerEncoder.py:68,75 etc.) */
int case_add(const void* a, const void* b, void* out, int64_t n, int32_t dtype, case_stream_t stream);
/* out = srcs[0] + ... + srcs[count - 1] (2 <= count <= 8; srcs is a HOST array of device pointers), summed in f32 and rounded once:
 * the gradient of a tensor with several consumers in one pass (what autograd forms with count - 1 binary adds, e.g. the Interaction
 * tensors of common/Interaction.py:32-63, each read by 2-5 products).  n a multiple of 16 bytes' worth of elements, 16-byte aligned. */
int case_add_n(const void* const* srcs, int32_t count, void* out, int64_t n, int32_t dtype, case_stream_t stream);
/* dropout with a counter RNG keyed by (seed, offset + element index); same call regenerates the mask in bwd */
int case_dropout(const void* x, void* y, int64_t n, float p, uint64_t seed, uint64_t offset, const CaseStepState* state,
                 int32_t dtype, case_stream_t stream);
/* zero rows whose valid flag is 0: TransformerBlock.py:31, Interaction.py:68-70.  y may BE x (round 6): then only the invalid rows are
 * written and the valid ones are not touched at all (inference: a full-length batch costs one flag byte per vector instead of a copy). */
int case_mask_rows(const void* x, const uint8_t* row_valid, void* y, int64_t rows, int64_t cols, int32_t dtype,
                   case_stream_t stream);
/* column sums of a [rows, cols] matrix into f32 [cols] (bias gradients); out must be pre-zeroed */
int case_colsum(const void* x, float* out, int64_t rows, int64_t cols, int32_t dtype, case_stream_t stream);
/* dtype conversion (f32 master weights -> bf16 operands) */
int case_cast(const void* x, void* y, int64_t n, int32_t src_dtype, int32_t dst_dtype, case_stream_t stream);
/* y[r, :] = x[r, :] * w[:]  (Interaction: Ep * w3); bwd dx = dy * w, dw += colsum(dy * x) */
int case_scale_cols(const void* x, const float* w, void* y, int64_t rows, int64_t cols, int32_t dtype,
                    case_stream_t stream);
int case_scale_cols_bwd(const void* dy, const void* x, const float* w, void* dx, float* dw, int64_t rows,
                        int64_t cols, int32_t dtype, case_stream_t stream);
/* single-output linear y[r] = x[r, :] . w (+ b[0]): the scorers (CaSE/Model.py:161,201, Masque/Model.py:157) and the
 * rank-1 terms of the Interaction score (common/Interaction.py:36).  y, g f32 [rows]; w f32 [cols].
 * bwd: dx[r, :] = g[r] * w (dx may be null), dw[c] += sum_r g[r] x[r, c], db[0] += sum_r g[r] (dw / db pre-zeroed). */
int case_rowdot_fwd(const void* x, const float* w, const float* b, float* y, int64_t rows, int64_t cols, int32_t dtype,
                    case_stream_t stream);
int case_rowdot_bwd(const float* g, const void* x, const float* w, void* dx, float* dw, float* db, int64_t rows,
                    int64_t cols, int32_t dtype, case_stream_t stream);
/* few-output linear over a column-wise concatenation that is never formed (round 6): the greedy step's mixing logits, Linear(3H, 1 + nmem) on
 * [dec_out | ctx_1 | .. ] (CaSE/Model.py:116, Masque/Model.py:42; common/TransformerSeqEncoderDecoder.py:141-142 of the reference's generic
 * decoder): y[r, o] = sum_k xs[k][r, :] . w[o, off_k .. off_k + widths[k]) + b[o].  xs / widths: HOST arrays of nseg (1..4) device pointers
 * ([rows, widths[k]] contiguous, `dtype`) and their widths; w f32 [nout, sum widths], b f32 [nout] (nullable), y f32 [rows, nout], nout 1..8.
 * Inference only (no backward).  CASE_FEAT_LINEAR_SKINNY. */
int case_linear_skinny(const void* const* xs, const int64_t* widths, int32_t nseg, const float* w, const float* b, float* y, int64_t rows,
                       int32_t nout, int32_t dtype, case_stream_t stream);
/* masked mean over the sequence: common/Utils.py:455-470.  x [n, L, H], valid u8 [n, L] -> out [n, H] */
int case_masked_mean_fwd(const void* x, const uint8_t* valid, void* out, int64_t n, int64_t L, int64_t H,
                         int32_t dtype, case_stream_t stream);
int case_masked_mean_bwd(const void* d_out, const uint8_t* valid, void* dx, int64_t n, int64_t L, int64_t H,
                         int32_t dtype, case_stream_t stream);
/* Highway gate: y = sigmoid(g) * tanh(nl) + (1 - sigmoid(g)) * lin  (common/Highway.py:29-35).
 * gnl is [rows, 3*cols] = [g | nl | lin] (one fused GEMM output). */
int case_highway_gate_fwd(const void* gnl, void* y, int64_t rows, int64_t cols, int32_t dtype, case_stream_t stream);
int case_highway_gate_bwd(const void* dy, const void* gnl, void* d_gnl, int64_t rows, int64_t cols, int32_t dtype,
                          case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K8  Interaction feature assembly: common/Interaction.py:65-74
 *   out[r, :] = valid[r] ? [e, a1, a2, e*a1, e*a2] : 0     (each [rows, H] -> [rows, 5H])
 *   bwd returns de, da1, da2.
 *   max over passages for the query side (num_q == 1): x [B, P, L, W] -> out [B, L, W], argmax int32
 * ------------------------------------------------------------------------------------------- */
/* K8 as kernels (round 6): everything between the encoder outputs and the two 5H-wide feature tensors of common/Interaction.py:32-74 in TWO
 * launches -- scores + both masked softmaxes, then the four products and the concatenations -- instead of 16 (two rank-1 projections, the
 * column scaling, U and U^T, two broadcast adds, two softmaxes, four batched products, two concatenations):
 *   U[i, j] = w1 . Eq[j] + w2 . Ep[i] + (w3 o Ep[i]) . Eq[j];  A = softmax_j U;  Bm = softmax_i U  (masked positions and all-masked rows: 0)
 *   A1 = A Eq,  B1 = Bm^T Ep,  A2 = A B1,  B2 = Bm^T A1
 *   g_q_p[n, i, :] = p_valid ? [Ep, A1, A2, Ep o A1, Ep o A2] : 0      g_p_q[n, j, :] = q_valid ? [Eq, B1, B2, Eq o B1, Eq o B2] : 0
 * eq [n / eq_div, Lq, H] (eq_div = P when one query faces P passages: pair n reads query n / eq_div, common/Interaction.py:26-29), ep [n, Lp, H],
 * q_valid [n / eq_div, Lq], p_valid [n, Lp] bytes, w f32 [3H] = dual_att_linear.weight; outputs a [n, Lp, Lq] and bt [n, Lq, Lp] (the two
 * probability matrices, what a backward pass reads), g_q_p [n, Lp, 5H], g_p_q [n, Lq, 5H] (the max over passages of :73-74 is
 * case_max_over_p_fwd on it).  bf16, H = 512, Lq = 64, Lp a multiple of 32 up to 512 (case_interaction_supported); CASE_E_UNSUPPORTED otherwise
 * (run the single launches).  The row term w2 . Ep[i] rides in the product (the query operand is w3 o Eq[j] + w2, rounded to bf16 once). */
typedef struct {
  int64_t n, Lp, Lq, H, eq_div;
  int32_t dtype;
} CaseInteractionDesc;
int case_interaction_supported(const CaseInteractionDesc* d);
int case_interaction_fwd(const CaseInteractionDesc* d, const void* eq, const void* ep, const uint8_t* q_valid, const uint8_t* p_valid, const float* w,
                         void* a, void* bt, void* g_q_p, void* g_p_q, case_stream_t stream);
int case_concat5_fwd(const void* e, const void* a1, const void* a2, const uint8_t* row_valid, void* out,
                     int64_t rows, int64_t H, int32_t dtype, case_stream_t stream);
int case_concat5_bwd(const void* d_out, const void* e, const void* a1, const void* a2, const uint8_t* row_valid,
                     void* de, void* da1, void* da2, int64_t rows, int64_t H, int32_t dtype, case_stream_t stream);
int case_max_over_p_fwd(const void* x, void* out, int32_t* argmax, int64_t B, int64_t P, int64_t inner, int32_t dtype,
                        case_stream_t stream);
int case_max_over_p_bwd(const void* d_out, const int32_t* argmax, void* dx, int64_t B, int64_t P, int64_t inner,
                        int32_t dtype, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K7  additive (Bahdanau) attention scores: common/BilinearAttention.py:24-46
 *   s[b, t, j] = sum_h v[h] * tanh(wq[b, t, h] + uh[b, j, h])      (never materialises [B, T, S, H])
 * wq f32 [B, T, H] (small: the query projection is produced in f32), uh [B, S, H] in dtype; v f32 [H];
 * s f32 [B, T, S].
 * bwd: given ds f32 [B, T, S]:  d_wq[b,t,h] = sum_j g, d_uh[b,j,h] = sum_t g, d_v[h] = sum ds*tanh,
 *      g = ds * v[h] * (1 - tanh^2);  d_wq, d_uh are f32 and fully written; d_v is f32 and must be
 *      pre-zeroed (one coalesced atomic per h per workgroup).
 * ------------------------------------------------------------------------------------------- */
int case_additive_scores_fwd(const float* wq, const void* uh, const float* v, float* s, int64_t B, int64_t T,
                             int64_t S, int64_t H, int32_t dtype, case_stream_t stream);
int case_additive_scores_bwd(const float* ds, const float* wq, const void* uh, const float* v, float* d_wq,
                             float* d_uh, float* d_v, int64_t B, int64_t T, int64_t S, int64_t H, int32_t dtype,
                             case_stream_t stream);

/* K22 (round 5), the greedy step's additive attention in one launch (common/BilinearAttention.py:31-59 at T = 1, CaSE/Model.py:79-82):
 *   s_j = v . tanh(wq + uh_j),  p = softmax_j(s | col_valid) (0 where masked, all 0 for an invalid target row),  ctx = sum_j p_j value_j,
 *   copy_j = p_j prior_j / (1e-8 + sum_j p_j prior_j)   (when prior is given)
 * with tanh(a + b) = 1 - 2 / (e^{2a} e^{2b} + 1) and eu = e^{2 uh} CACHED across the steps (case_additive_key_exp: f32 uh -> bf16 eu, both
 * exponents clamped at +-43): one reciprocal per element instead of an exponential and a reciprocal.  wq [B, H] f32 (query projection incl.
 * bias), eu / value [B, S, H] bf16, v [H] f32, col_valid [B, S] / row_valid [B] bytes (nullable), prior [B, S] f32 (nullable, with copy);
 * outputs ctx [B, H] bf16, p [B, S] f32, copy [B, S] f32.  One workgroup per item; H = 512, S <= 28000; CASE_E_UNSUPPORTED otherwise.
 * wq_add [B, H] f32 (nullable, round 6): added to wq -- the step-invariant part of the query projection when the query is [x_t | feature] with a
 * feature that does not change over the steps (CaSE/Model.py:77-78: the answer representation), so that a step projects x_t alone. */
int case_additive_key_exp(const float* uh, void* eu, int64_t n, case_stream_t stream);
/* K23 (round 5), the greedy step's pointer-generator head in one launch (CaSE/Model.py:34-48, :112-117; Masque/Model.py:29-44; argmax as
 * common/Utils.py:156-168, lowest index on ties):  gen = softmax(logits);  pm = softmax(mix_logits);
 *   dist[b, :] = pm[b, 0] gen[b, :] + sum_k scatter(pm[b, 1 + k] copies[k][b, :] over the source tokens);  ids[b] = argmax dist[b, :].
 * logits / gen / dist [B, V] f32 (gen and dist nullable: a greedy step before the last one needs ids only -- 2 x B x V x 4 bytes of writes
 * per step less), mix_logits [B, 1 + nmem] f32, keys [B, S] the sorted (token << 15 | position) keys of
 * case_source_sort over the concatenated source map, copies = nmem device pointers (host array) to [B, lens[k]] f32 weights, sum lens = S,
 * ids [B] int64, top [B] f32 (nullable) = dist[b, ids[b]].  One workgroup per row, the vocabulary row in LDS: V <= 36000, nmem <= 4,
 * S <= 32768; CASE_E_UNSUPPORTED otherwise (run case_softmax_fwd / case_copy_scatter_sorted_fwd / case_row_argmax). */
int case_pointer_head_decode(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                             const int64_t* lens, int32_t nmem, float* gen, float* dist, int64_t* ids, float* top, int64_t B, int64_t V,
                             int64_t S, case_stream_t stream);
/* Beam search around the cached decode step (the reference's common/Generations.py:112-190, per item on the device; CASE_FEAT_BEAM_DECODE).
 * A hypothesis is slot w of item b and row b * W + w of the step's batch; W <= 8.  All four launches are asynchronous on `stream`.
 *
 * K24 case_pointer_head_beam: K23's row (same arguments, R = B * W rows) with a top-W tail instead of the argmax: cand_p / cand_id [R, W] = the W
 *   largest entries of the row in descending order, the lowest id first among equals; deterministic; W = 1 gives K23's id and value bit for
 *   bit.  gen / dist [R, V] nullable.  Same limits as K23, and W <= V.
 * K25 case_beam_advance: one step of the search for every item, in place on the caller's state.  Candidate (w, j) of a live slot w has the key
 *   (cum[b, w] - log(cand_p[b*W + w, j] + 1e-10)) / (len[b, w] + 1); dead slots (alive == 0) contribute +inf.  The W smallest keys -- stable
 *   in (w, j) order -- become the new slots: parent [B, W] int32 (slot of the same item), token [B, W] int64 (PAD for a slot that is not
 *   live afterwards), cum f32, len int32, alive u8 are rewritten; hist_parent / hist_token [T, B, W] receive row t.  A new slot whose token
 *   is `eos`, and every new slot at t == T - 1, retires into the finished pool fin_key / fin_step / fin_slot [B, W] (ascending by key, a
 *   newcomer behind its equals, the worst dropped; initialise to +inf / -1 / 0).  Start state: alive = cum = 0 but alive[b, 0] = 1, len = 1.
 * K26 case_beam_gather: dst[l][b*W + w, 0 .. t] = src[l][b*W + parent[b, w], 0 .. t] for the nlayers caches [B*W, Tmax, row_bytes] named by the
 *   HOST arrays src / dst (two different buffers per layer; row_bytes a multiple of 16, pointers 16-byte aligned) and, when given, for the
 *   prefix validity valid_src -> valid_dst u8 [B*W, Tmax].  One launch for up to 16 layers; one launch per 16 layers beyond that.
 * K27 case_beam_backtrack: the pool's hypotheses followed back through the history: beam_answers [B, W, T] int64 best first (BOS dropped, EOS
 *   kept, PAD behind it), beam_scores [B, W] f32 = cum / len (+inf for an empty entry), answer [B, T] = beam_answers[:, 0]. */
int case_pointer_head_beam(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies, const int64_t* lens,
                           int32_t nmem, float* gen, float* dist, float* cand_p, int64_t* cand_id, int64_t R, int64_t V, int64_t S, int32_t W,
                           case_stream_t stream);
int case_beam_advance(const float* cand_p, const int64_t* cand_id, uint8_t* alive, float* cum, int32_t* len, int32_t* parent, int64_t* token,
                      int32_t* hist_parent, int64_t* hist_token, float* fin_key, int32_t* fin_step, int32_t* fin_slot, int64_t t, int64_t T,
                      int64_t B, int32_t W, int64_t eos, case_stream_t stream);
int case_beam_gather(const void* const* src, void* const* dst, int32_t nlayers, const int32_t* parent, const uint8_t* valid_src,
                     uint8_t* valid_dst, int64_t B, int32_t W, int64_t Tmax, int64_t row_bytes, int64_t t, case_stream_t stream);
int case_beam_backtrack(const int32_t* hist_parent, const int64_t* hist_token, const float* fin_key, const int32_t* fin_step,
                        const int32_t* fin_slot, int64_t* answer, int64_t* beam_answers, float* beam_scores, int64_t B, int32_t W, int64_t T,
                        case_stream_t stream);
/* K28 case_pointer_head_sample (CASE_FEAT_SAMPLE_DECODE): K23's row (same arguments and limits, R rows) with one token DRAWN from it instead of
 * the argmax.  With logits == NULL the row is read from dist_in [R, V] instead of being built (mix_logits / keys / copies / lens / gen unused,
 * V <= 36000).  The draw rule, per row p[0 .. V) and one uniform u in [0, 1):
 *   1. q_i = p_i^(1 / temperature), 0 where p_i = 0 (temperature 1: q = p bit for bit; otherwise q is scaled so that its largest entry is 1);
 *   2. the order is K24's: q descending, the lower id first among equals;
 *   3. top_k > 0 keeps the first min(top_k, V) entries of the order;
 *   4. top_p < 1 keeps, among those, the shortest prefix of the order whose mass is >= top_p x the mass after step 3 (at least one entry);
 *   5. with Z the kept mass, the token is the smallest kept id j, in ID order, with sum_{kept i <= j} q_i > u Z (the largest kept id with
 *      q > 0 if rounding leaves none); an entry with q = 0 is never drawn;
 *   6. prob [R] = p_j.
 * u = uniforms[r] when uniforms is given, else (hash(seed, state->rng_base + offset + r) >> 8) 2^-24 (state nullable, as on a dropout site:
 * with a device state a captured launch draws anew whenever rng_base has moved).  Deterministic: the same inputs and u give the same id.
 * Loop conventions of the reference's common/Generations.py `sample`, on ended u8 [R] (in / out) with x the drawn id and e = ended[r]:
 * ids[r] = first ? (x == eos ? unk : x) : last ? (e ? pad : eos) : (e ? pad : x); prob[r] = 1 where e; then ended[r] |= (x == eos).
 * gen / dist [R, V] nullable as in K23 (dist is the unfiltered row). */
int case_pointer_head_sample(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies, const int64_t* lens,
                             int32_t nmem, const float* dist_in, float* gen, float* dist, int64_t* ids, float* prob, uint8_t* ended,
                             const float* uniforms, int64_t R, int64_t V, int64_t S, float temperature, int32_t top_k, float top_p, uint64_t seed,
                             uint64_t offset, const CaseStepState* state, int64_t eos, int64_t unk, int64_t pad, int32_t first, int32_t last,
                             case_stream_t stream);
/* K32, the n-gram ban (CASE_FEAT_NGRAM_BAN; purely additive, generation 600 unchanged).  hist [R, Tmax] int32 holds what every row has emitted
 * so far, BOS excluded.  At step t (0 <= t < Tmax, t <= 256) with n >= 1, token v of row r is banned when some j <= t - n has
 * hist[r, j .. j + n - 2] == hist[r, t - n + 1 .. t - 1] and hist[r, j + n - 1] == v (n = 1: every token of the history).  A banned entry of the
 * mixed distribution row is set to 0.0 BEFORE the selection (argmax, top-W, pmax / cuts / draw); nothing else changes and the row is not
 * renormalised, so top / cand_p / prob stay the model's own probabilities and a returned dist is the row after the ban.  No ban for t < n, for a
 * history that holds `eos` (-1: none), or for a sampler row with ended[r] != 0; ids outside [0, V) in a history are ignored.
 * case_pointer_head_decode_ban / _sample_ban: the K23 / K28 arguments, then hist, Tmax, t, n (and eos for K23; K28 uses its own); the kernel
 *   APPENDS the id it emits (K23: the argmax; K28: ids[r] after the first / last / ended conventions) at hist[r, t].
 * case_pointer_head_beam_ban: K24 likewise; it only reads hist (row b * W + w = the hypothesis of slot w), case_beam_advance_ban appends.
 * case_beam_advance_ban: K25 with the flat history: flat_old / flat_new int32 [B, W, Tmax], two different buffers;
 *   flat_new[b, w, 0 .. t) = flat_old[b, parent[b, w], 0 .. t), flat_new[b, w, t] = the slot's token (hist_token's).  A candidate of probability
 *   exactly 0 is dead here (it takes no slot and does not retire).
 * case_ngram_ban: the same rule on dist f32 [R, V] in place (one wave per row; ended u8 [R] nullable); it appends nothing. */
int case_pointer_head_decode_ban(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                 const int64_t* lens, int32_t nmem, float* gen, float* dist, int64_t* ids, float* top, int64_t B, int64_t V,
                                 int64_t S, int32_t* hist, int64_t Tmax, int64_t t, int32_t n, int64_t eos, case_stream_t stream);
int case_pointer_head_beam_ban(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies, const int64_t* lens,
                               int32_t nmem, float* gen, float* dist, float* cand_p, int64_t* cand_id, int64_t R, int64_t V, int64_t S, int32_t W,
                               const int32_t* hist, int64_t Tmax, int64_t t, int32_t n, int64_t eos, case_stream_t stream);
int case_pointer_head_sample_ban(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies, const int64_t* lens,
                                 int32_t nmem, const float* dist_in, float* gen, float* dist, int64_t* ids, float* prob, uint8_t* ended,
                                 const float* uniforms, int64_t R, int64_t V, int64_t S, float temperature, int32_t top_k, float top_p, uint64_t seed,
                                 uint64_t offset, const CaseStepState* state, int64_t eos, int64_t unk, int64_t pad, int32_t first, int32_t last,
                                 int32_t* hist, int64_t Tmax, int64_t t, int32_t n, case_stream_t stream);
int case_beam_advance_ban(const float* cand_p, const int64_t* cand_id, uint8_t* alive, float* cum, int32_t* len, int32_t* parent, int64_t* token,
                          int32_t* hist_parent, int64_t* hist_token, float* fin_key, int32_t* fin_step, int32_t* fin_slot, int64_t t, int64_t T,
                          int64_t B, int32_t W, int64_t eos, const int32_t* flat_old, int32_t* flat_new, int64_t Tmax, case_stream_t stream);
int case_ngram_ban(float* dist, const int32_t* hist, const uint8_t* ended, int64_t R, int64_t V, int64_t Tmax, int64_t t, int32_t n, int64_t eos,
                   case_stream_t stream);
/* The decoding rules (CASE_FEAT_DECODE_RULES; purely additive, generation 600 unchanged): min_length, banned ids and the beam length penalty.
 * The row rules act on the mixed distribution row of step t (t = the 0-based step = the tokens the row has emitted, BOS excluded), AFTER K32 and
 * BEFORE the selection (argmax, top-W, pmax / cuts / draw), with plain stores of 0.0 and no renormalisation -- K32's contract, so top / cand_p /
 * prob stay the model's own probabilities and a returned dist is the row after the ban and the rules:
 *   min_length: row[eos] = 0.0 while t < min_length (min_length >= 0, 0 = off; eos outside [0, V), e.g. -1: no effect);
 *   banned:     row[v] = 0.0 at every step for every v in the row's item's list.  banned int32 [K] with banned_stride = 0 (one list for every
 *               row) or [R / rows_per_item, K] with banned_stride = K (row r takes list r / rows_per_item; R a multiple of rows_per_item >= 1).
 *               0 <= K <= 256 (K = 0: off, banned may be NULL); entries outside [0, V) are ignored (-1 pads a ragged list); duplicates are legal.
 * Limits, all of them: K <= 256 (CASE_E_UNSUPPORTED beyond).  The rules need no history and have NO step bound; K32's t <= 256 binds a call
 * only when it also asks for the n-gram ban.  The rules apply to every row at every step, whatever its history holds; the one exception is a K28
 * row with ended[r] != 0, which is left alone (it emits PAD with probability 1).  A row whose every entry ends up 0.0 behaves as an all-zero row
 * does: id 0, value 0.
 * Each `_rules` head takes the arguments of its `_ban` / `_wide` sibling, with the ban OPTIONAL (hist == NULL or n == 0: no ban, nothing is
 * appended, Tmax is not read; otherwise K32 exactly as above, appends included), then the rule operands: eos, min_length, banned, K,
 * banned_stride, rows_per_item.  `ban_eos` is K32's eos (its "history holds eos" clause); K28's own eos plays that part in the sample forms,
 * whose rule eos is `rule_eos`.  With min_length = 0 and K = 0 a `_rules` head returns the bits of its sibling.  The wide `_rules` forms always
 * need row_ws (dist_in is never read in place).
 * case_row_rules: the same rules on dist f32 [R, V] in place (one wave per row; ended u8 [R] nullable: rows with ended != 0 are left alone).
 * case_beam_advance_rules: case_beam_advance_ban (flat history; a candidate of probability exactly 0 is dead, so a zeroed entry never enters a
 *   hypothesis even when fewer than W entries survive) with the key cost / (len + 1)^length_penalty for candidates and retiring hypotheses
 *   (powf in f32; cost = cum - log(p + 1e-10), len counts BOS), so fin_key / beam_scores are these keys.  length_penalty finite and >= 0;
 *   exactly 1.0 is case_beam_advance_ban's own launch (the division, bit for bit). */
int case_pointer_head_decode_rules(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                   const int64_t* lens, int32_t nmem, float* gen, float* dist, int64_t* ids, float* top, int64_t B, int64_t V,
                                   int64_t S, int32_t* hist, int64_t Tmax, int64_t t, int32_t n, int64_t ban_eos, int64_t eos, int32_t min_length,
                                   const int32_t* banned, int32_t K, int64_t banned_stride, int64_t rows_per_item, case_stream_t stream);
int case_pointer_head_beam_rules(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies, const int64_t* lens,
                                 int32_t nmem, float* gen, float* dist, float* cand_p, int64_t* cand_id, int64_t R, int64_t V, int64_t S, int32_t W,
                                 const int32_t* hist, int64_t Tmax, int64_t t, int32_t n, int64_t ban_eos, int64_t eos, int32_t min_length,
                                 const int32_t* banned, int32_t K, int64_t banned_stride, int64_t rows_per_item, case_stream_t stream);
int case_pointer_head_sample_rules(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                   const int64_t* lens, int32_t nmem, const float* dist_in, float* gen, float* dist, int64_t* ids, float* prob,
                                   uint8_t* ended, const float* uniforms, int64_t R, int64_t V, int64_t S, float temperature, int32_t top_k,
                                   float top_p, uint64_t seed, uint64_t offset, const CaseStepState* state, int64_t eos, int64_t unk, int64_t pad,
                                   int32_t first, int32_t last, int32_t* hist, int64_t Tmax, int64_t t, int32_t n, int64_t rule_eos,
                                   int32_t min_length, const int32_t* banned, int32_t K, int64_t banned_stride, int64_t rows_per_item,
                                   case_stream_t stream);
int case_pointer_head_decode_wide_rules(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                        const int64_t* lens, int32_t nmem, float* gen, float* dist, int64_t* ids, float* top, int64_t B, int64_t V,
                                        int64_t S, float* row_ws, int64_t row_stride, int32_t* hist, int64_t Tmax, int64_t t, int32_t n,
                                        int64_t ban_eos, int64_t eos, int32_t min_length, const int32_t* banned, int32_t K, int64_t banned_stride,
                                        int64_t rows_per_item, case_stream_t stream);
int case_pointer_head_beam_wide_rules(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                      const int64_t* lens, int32_t nmem, float* gen, float* dist, float* cand_p, int64_t* cand_id, int64_t R,
                                      int64_t V, int64_t S, int32_t W, float* row_ws, int64_t row_stride, const int32_t* hist, int64_t Tmax,
                                      int64_t t, int32_t n, int64_t ban_eos, int64_t eos, int32_t min_length, const int32_t* banned, int32_t K,
                                      int64_t banned_stride, int64_t rows_per_item, case_stream_t stream);
int case_pointer_head_sample_wide_rules(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                        const int64_t* lens, int32_t nmem, const float* dist_in, float* gen, float* dist, int64_t* ids, float* prob,
                                        uint8_t* ended, const float* uniforms, int64_t R, int64_t V, int64_t S, float temperature, int32_t top_k,
                                        float top_p, uint64_t seed, uint64_t offset, const CaseStepState* state, int64_t eos, int64_t unk,
                                        int64_t pad, int32_t first, int32_t last, float* row_ws, int64_t row_stride, int32_t* hist, int64_t Tmax,
                                        int64_t t, int32_t n, int64_t rule_eos, int32_t min_length, const int32_t* banned, int32_t K,
                                        int64_t banned_stride, int64_t rows_per_item, case_stream_t stream);
int case_row_rules(float* dist, const uint8_t* ended, int64_t R, int64_t V, int64_t t, int64_t eos, int32_t min_length, const int32_t* banned,
                   int32_t K, int64_t banned_stride, int64_t rows_per_item, case_stream_t stream);
int case_beam_advance_rules(const float* cand_p, const int64_t* cand_id, uint8_t* alive, float* cum, int32_t* len, int32_t* parent, int64_t* token,
                            int32_t* hist_parent, int64_t* hist_token, float* fin_key, int32_t* fin_step, int32_t* fin_slot, int64_t t, int64_t T,
                            int64_t B, int32_t W, int64_t eos, const int32_t* flat_old, int32_t* flat_new, int64_t Tmax, float length_penalty,
                            case_stream_t stream);
/* The wide forms of K23 / K24 / K28 (CASE_FEAT_POINTER_HEAD_WIDE; purely additive, generation 600 unchanged): the same kernels with the
 * vocabulary row of a workgroup in device memory instead of LDS, for vocabularies beyond 36000 ids.  Each takes the arguments of its LDS
 * sibling, then row_ws, row_stride, then the history operands of the `_ban` form (hist == NULL or n == 0: no ban; otherwise K32 exactly as above).
 * row_ws f32 [rows, row_stride] is the caller's workspace: 16-byte aligned, row_stride >= V and a multiple of 4; its contents on entry do not
 * matter and on return are unspecified.  One workgroup per row, as in the LDS forms; a workgroup touches its own row only.
 * Every V from 1 up to the limit is accepted, and at any V the LDS form accepts the wide form returns the same bits in every output (the same
 * per-thread strides, reduction order and tie rules), so everything stated for K23 / K24 / K28 / K32 holds here.
 * Limits: a built row (logits != NULL) takes V <= 131071 (the key format of case_source_sort), nmem <= 4, S <= 32768; CASE_E_UNSUPPORTED beyond.
 * case_pointer_head_sample_wide with logits == NULL draws from dist_in [R, V] for any V <= 16777216 = 2^24: the top-p cut sums fixed-point masses
 * of 2^-40 of the largest entry's binade, each below 2^40, in 64-bit integers, and 2^24 of them cannot pass 2^64.  K28 leaves the row unchanged,
 * so dist_in is read where it lies when it is 16-byte aligned, V is a multiple of 4 and no ban is asked (row_ws may then be NULL); otherwise
 * it is copied into row_ws first.  dist_in itself is never written. */
int case_pointer_head_decode_wide(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies,
                                  const int64_t* lens, int32_t nmem, float* gen, float* dist, int64_t* ids, float* top, int64_t B, int64_t V,
                                  int64_t S, float* row_ws, int64_t row_stride, int32_t* hist, int64_t Tmax, int64_t t, int32_t n, int64_t eos,
                                  case_stream_t stream);
int case_pointer_head_beam_wide(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies, const int64_t* lens,
                                int32_t nmem, float* gen, float* dist, float* cand_p, int64_t* cand_id, int64_t R, int64_t V, int64_t S, int32_t W,
                                float* row_ws, int64_t row_stride, const int32_t* hist, int64_t Tmax, int64_t t, int32_t n, int64_t eos,
                                case_stream_t stream);
int case_pointer_head_sample_wide(const float* logits, const float* mix_logits, const uint32_t* keys, const float* const* copies, const int64_t* lens,
                                  int32_t nmem, const float* dist_in, float* gen, float* dist, int64_t* ids, float* prob, uint8_t* ended,
                                  const float* uniforms, int64_t R, int64_t V, int64_t S, float temperature, int32_t top_k, float top_p, uint64_t seed,
                                  uint64_t offset, const CaseStepState* state, int64_t eos, int64_t unk, int64_t pad, int32_t first, int32_t last,
                                  float* row_ws, int64_t row_stride, int32_t* hist, int64_t Tmax, int64_t t, int32_t n, case_stream_t stream);
/* K29 case_pointer_head_score (CASE_FEAT_POINTER_SCORE): the head of a teacher-forced scoring pass.  For row r with target y = targets[r]:
 *   gen_y = exp(logits[r, y] - max) / sum_i exp(logits[r, i] - max);   pm = softmax(mix_logits[r, 0 .. nmem]);
 *   ptr   = sum_k pm[1 + k] sum_{positions s of memory k whose source id is y} copies[k][r, s];
 *   prob[r] = pm[0] gen_y + ptr;   copy[r] = ptr   (copy nullable).
 * y == pad (pad >= 0; -1 = score every target) gives prob 1, copy 0: the position is not scored.  y outside [0, V) gives prob 0, copy 0.
 * logits [R, V] f32, mix_logits [R, 1 + nmem] f32, targets [R] int64, copies / lens as in K23 with R rows (positions offset by the lengths
 * before them, sum lens = S).  keys [R / rows_per_source, S]: row r reads key row r / rows_per_source -- the candidates of one item are
 * consecutive rows and share its sorted keys unrepeated; R must be a multiple of rows_per_source.  One workgroup per row reads the logits
 * once and keeps no vocabulary row: nmem <= 4, S <= 32768, V <= 131071 (the key format); CASE_E_UNSUPPORTED otherwise.  No atomics:
 * two launches give the same bits. */
int case_pointer_head_score(const float* logits, const float* mix_logits, const uint32_t* keys, int64_t rows_per_source,
                            const float* const* copies, const int64_t* lens, int32_t nmem, const int64_t* targets, int64_t pad, float* prob,
                            float* copy, int64_t R, int64_t V, int64_t S, case_stream_t stream);
int case_pointer_attend_decode(const float* wq, const float* wq_add, const void* eu, const float* v, const void* value, const uint8_t* col_valid,
                               const uint8_t* row_valid, const float* prior, void* ctx, float* p, float* copy, int64_t B, int64_t S, int64_t H,
                               case_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * K11 copy / pointer distribution: CaSE/Model.py:38-48 with common/Utils.py:344-355
 *   dist[b, t, src[b, s]] += w[b, t, s]        (scatter-add instead of the dense one-hot bmm)
 * src int64 [B, S]; w f32 [B, T, S]; dist f32 [B, T, V] (caller zero-fills or pre-loads dist1).
 * bwd: d_w[b, t, s] = d_dist[b, t, src[b, s]].
 * ------------------------------------------------------------------------------------------- */
int case_copy_scatter_fwd(const int64_t* src, const float* w, float* dist, int64_t B, int64_t T, int64_t S,
                          int64_t V, case_stream_t stream);
int case_copy_scatter_bwd(const int64_t* src, const float* d_dist, float* d_w, int64_t B, int64_t T, int64_t S,
                          int64_t V, case_stream_t stream);
/* Sorted form (on-device source_map sort, once per batch; the reference rebuilds a [B, S, V] one-hot per call,
 * common/Utils.py:344-355).  case_source_sort: keys u32 [B, S] = (src[b, s] << 15 | s) ascending per row, ids outside [0, V)
 * last as 0xFFFFFFFF; needs S <= 32768, V <= 131071.  case_copy_scatter_sorted_fwd adds each run of equal tokens to dist in a
 * fixed order with plain stores: no atomics, bit-reproducible.  Same dist contract as case_copy_scatter_fwd; the backward is
 * case_copy_scatter_bwd (a gather, order-free). */
int case_source_sort(const int64_t* src, uint32_t* keys, int64_t B, int64_t S, int64_t V, case_stream_t stream);
int case_copy_scatter_sorted_fwd(const uint32_t* keys, const float* w, float* dist, int64_t B, int64_t T, int64_t S,
                                 int64_t V, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K12 losses
 *   NLL of log(dist + 1e-8) at the target, ignore_index = 0 (CaSE/Model.py:306, Masque/Model.py:239):
 *     per_row[r] = target[r] ? -log(dist[r, target[r]] + 1e-8) : 0 ; bwd writes only the target column
 *     into a pre-zeroed d_dist: d_dist[r, y] = -g_row[r] / (dist[r, y] + 1e-8)
 *   Row argmax with lowest-index tie break (common/Utils.py:167) for greedy decoding (K13).
 * ------------------------------------------------------------------------------------------- */
int case_nll_gather_fwd(const float* dist, const int64_t* target, float* per_row, int64_t rows, int64_t V,
                        case_stream_t stream);
int case_nll_gather_bwd(const float* dist, const int64_t* target, const float* g_row, float* d_dist, int64_t rows,
                        int64_t V, case_stream_t stream);
int case_row_argmax(const float* x, int64_t* idx, float* val, int64_t rows, int64_t cols, int64_t ld,
                    case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K15  optimizer-side multi-tensor kernels: common/CumulativeTrainer.py:70-76 clip_grad_norm_(params, 1) ->
 *   optim.Adam.step() (CaSE/Run.py:27: default betas / eps, no weight decay) -> EMA.update() (common/EMA.py:13-18), plus the
 *   refresh of the bf16 operand copies, in two launches over all parameter tensors.
 * `table` (device): one CaseOptTensor per tensor, f32 p / g / m (exp_avg) / v (exp_avg_sq) / shadow (EMA, may be null),
 *   p_bf16 (may be null), numel, and the tensor's step-dependent scalars step_size = lr / (1 - beta1^step), bc2_sqrt =
 *   sqrt(1 - beta2^step) (torch.optim.Adam keeps one step count per parameter; formed in double on the host and rounded to f32
 *   once, as torch does).  An entry with g == null is a parameter without a gradient this step: only its EMA shadow moves
 *   (common/EMA.py:13-18 touches every trainable parameter).  `chunks` (device): int32 pairs (tensor index, chunk index), one
 *   per workgroup, chunk = case_optim_chunk_elems() elements.
 * case_optim_sumsq: partials f32 [nchunks] (workspace) receives one sum of squares per chunk; sumsq (f32 scalar) their sum,
 *   added by one workgroup in a fixed order: bit-reproducible and identical on every data-parallel rank, like the reference's
 *   clip_grad_norm_.  Pass sumsq to case_optim_adam_ema to apply the clip coefficient min(1, max_norm / (sqrt(sumsq) + 1e-6))
 *   without a host round trip (null: no clipping).  ema_w = 1 - decay (0: no EMA update).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  void* p;
  const void* g;
  void* m;
  void* v;
  void* shadow;
  void* p_bf16;
  int64_t numel;
  float step_size;
  float bc2_sqrt;
} CaseOptTensor;
int case_optim_chunk_elems(void);
int case_sizeof_opt_tensor(void); /* sizeof(CaseOptTensor) as the library was built: a binder checks its own layout against it */
int case_optim_sumsq(const CaseOptTensor* table, const int32_t* chunks, int64_t nchunks, float* partials, float* sumsq,
                     case_stream_t stream);
/* state (nullable, ABI 600): step_size / bc2_sqrt of EVERY entry with a gradient are read from the device struct instead of the table
 * (all such parameters then share one step count -- a captured step keeps its table static). */
int case_optim_adam_ema(const CaseOptTensor* table, const int32_t* chunks, int64_t nchunks, const float* sumsq, float max_norm,
                        double beta1, double beta2, double eps, double ema_w, const CaseStepState* state, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K16  the row-local half of an encoder layer in ONE launch (inference form, bf16, d_model = dim_feedforward = 512):
 *   common/TransformerEncoder.py:66-75 around the attention core, and the next layer's :66-67:
 *     y = x_in Wo^T + bo + resid;  s2 = LN2(y);  o = gelu(s2 W1^T + b1) W2^T + b2 + s2;  s' = LN1_next(o);  qkv' = s' Wqkv'^T + bqkv'
 *   variant 0 (full):  x_in = this layer's attention output [rows, 512], resid = its normed input s; writes s_out = s', qkv_out = qkv'
 *   variant 1 (tail):  the last layer: writes s_out = o (the encoder output); LN1_next / QKV arguments may be null
 *   variant 2 (head):  layer 0: x_in = embedding output; writes s_out = LN1(x_in), qkv_out; the layer-stage arguments may be null
 * Weights are passed PRE-PACKED (case_encoder_chain_pack: bf16 row-major [512, 512] x 3 and [1536, 512] -> MFMA fragment order,
 * case_encoder_chain_packed_bytes() bytes; any matrix may be null for the variants that do not read it); biases and LayerNorm
 * parameters f32.  Of the 20 activation passes over HBM that the same chain makes as single GEMM / LayerNorm launches, 6 remain
 * (x_in, resid in; s', qkv' out).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t rows;   /* tokens (sequences x length) */
  int32_t width;  /* 512 */
  int32_t variant;
  float eps_ln2, eps_ln1_next;
} CaseEncoderChainDesc;
int64_t case_encoder_chain_packed_bytes(void);
int case_encoder_chain_pack(const void* wo, const void* w1, const void* w2, const void* wqkv, void* packed, case_stream_t stream);
int case_encoder_chain(const CaseEncoderChainDesc* d, const void* x_in, const void* resid, const void* packed, const float* bo,
                       const float* b1, const float* b2, const float* bqkv, const float* ln2_g, const float* ln2_b,
                       const float* ln1n_g, const float* ln1n_b, void* s_out, void* qkv_out, case_stream_t stream);

/* (K20, case_decoder_chain -- the fused decoder step chain of round 4 -- was retired in round 5: measured slower than the single launches
 * it replaced, 3.93 against 3.43 ms per cached step; the greedy step's time went to K21 - K23 instead.  Its feature bit stays reserved.) */

/* Greedy post-processing on the device (common/Utils.py:200-217 to_sentence): per row of ids [B, T] drop the BOS / PAD ids and
 * everything from the first EOS on; out [B, T] holds the kept ids front-packed (pad behind), len [B] their count.  One host
 * copy of (out, len) replaces the reference's `.item()` per generated token.  Pass -1 for a special id the vocabulary lacks. */
int case_sentence_compact(const int64_t* ids, int64_t* out, int32_t* len, int64_t B, int64_t T, int64_t bos, int64_t pad,
                          int64_t eos, case_stream_t stream);

/* K33 (CASE_FEAT_NGRAM_BAN): the reference's remove_duplicate (common/Utils.py:170-193) on case_sentence_compact's outputs, in place.  Per row,
 * with L = len[b]: while L > n, cut at the largest i in [1, L - n] such that every token of out[b, i .. L) also occurs in out[b, 0 .. i); stop
 * when there is none.  PAD is written behind the new length and len[b] updated.  One wave per row; T <= 256 (CASE_E_UNSUPPORTED beyond), n >= 1. */
int case_remove_duplicate_ids(int64_t* out, int32_t* len, int64_t B, int64_t T, int32_t n, int64_t pad, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Consensus (minimum-Bayes-risk) selection over a pool of candidates, and ROUGE-L on token ids (CASE_FEAT_CONSENSUS; purely additive,
 * generation 600 unchanged).  The metric is evaluation/Rouge.py:65-108 (LCS) and :186-206 (F-measure) on ids instead of words.
 * K30 case_lcs_pairs: for every item b, hypothesis n and reference m
 *     lcs[b, n, m] = the length of the longest common subsequence of a[b, n, 0 .. a_len[b, n]) and b[b, m, 0 .. b_len[b, m]);
 *     r = lcs / b_len, p = lcs / a_len, beta = p / (r + 1e-12), f[b, n, m] = (1 + beta^2) r p / (r + beta^2 p + 1e-12)
 *   evaluated in f64 in this order and rounded once to f32; a_len == 0 or b_len == 0 gives lcs = 0 and f = 0.
 *   a int64 [B, N, Ta], b int64 [B, M, Tb]: front-packed ids (what case_sentence_compact writes); a_len [B, N], b_len [B, M] int32 (clamped to
 *   0 .. Ta / Tb); lcs int32 and f f32 [B, N, M].  Ids are compared on their low 32 bits: the caller guarantees 0 <= id < 2^31 (not checked).
 *   One wave per hypothesis holds it as 64-bit match masks, so Ta <= 256 (CASE_E_UNSUPPORTED beyond); Tb is a loop count without such a
 *   limit.  Integer arithmetic up to the one F evaluation: two launches give the same bits.
 * K31 case_consensus_pick: with f [B, N, N] the pairwise utility of a pool against itself (candidate n as the hypothesis, m as the reference,
 *   the self term included), w f32 [B, N] (NULL: uniform) and valid u8 [B, N] (NULL: all valid)
 *     utility[b, n] = sum_{valid m} w[b, m] f[b, n, m] / sum_{valid m} w[b, m]   (f32, m ascending; 0 when the weights sum to 0);
 *     -inf for an invalid n;  index[b] (int64) = the argmax with the lowest index among equals, 0 for an item without a valid candidate;
 *     answer[b, 0 .. T) = cand[b, index[b], 0 .. T)   (cand int64 [B, N, T]: the raw rows, copied bit for bit).
 *   One wave per item: N <= 64 (CASE_E_UNSUPPORTED beyond).
 * ------------------------------------------------------------------------------------------- */
int case_lcs_pairs(const int64_t* a, const int32_t* a_len, const int64_t* b, const int32_t* b_len, int32_t* lcs, float* f, int64_t B,
                   int64_t N, int64_t M, int64_t Ta, int64_t Tb, case_stream_t stream);
int case_consensus_pick(const float* f, const float* w, const uint8_t* valid, const int64_t* cand, float* utility, int64_t* index,
                        int64_t* answer, int64_t B, int64_t N, int64_t T, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * BLEU and n-gram overlap on token ids (CASE_FEAT_NGRAM_COUNTS; purely additive, generation 600 unchanged).  The metrics are nltk's
 * sentence_bleu, which evaluation/Eval_Bleu.py calls with default arguments, and evaluation/Eval_Overlap.py's distinct-set overlap.
 * K34 case_ngram_counts: a, a_len, b, b_len exactly as case_lcs_pairs takes them (front-packed ids, lengths clamped to 0 .. Ta / Tb, ids
 *   compared on their low 32 bits, Ta <= 256 or CASE_E_UNSUPPORTED, Tb without such a limit); max_n in 1 .. 4.  With count_s(g) the number of
 *   times the k-gram g occurs in sequence s, for every order k = 1 .. max_n (index k - 1 of the last axis; the orders above max_n read 0):
 *     clip[b, n, m, k]   = sum over the distinct k-grams g of hypothesis n of min(count_hyp(g), count_ref_m(g))
 *     clip_any[b, n, k]  = the same sum with max over the present references m (b_len > 0) of count_ref_m(g) in place of count_ref_m(g)
 *     hit[b, n, m, k]    = the number of distinct hypothesis k-grams that occur in reference m;  hit_any[b, n, k]: in any present reference
 *     distinct[b, n, k]  = the number of distinct hypothesis k-grams
 *   all int32 and exact; an absent reference (b_len == 0) reads 0.  The k-gram total of a hypothesis is max(a_len - k + 1, 0).
 * K35 case_bleu_scores: with la = a_len[b, n], p_k = clip_k / max(1, la - k + 1) (smoothing 1, "add one": (clip_k + 1) / (max(1, la - k + 1) + 1)
 *   for k >= 2) and r a reference length
 *     score = BP exp(sum_{k = 1 .. max_n} ln p_k / max_n),   BP = 1 if la > r, else exp(1 - r / la)
 *   in f64, k ascending, without contraction; exactly 0 when a p_k is 0 and when la == 0 or there is no reference.
 *     bleu_pair[b, n, m] (f32, rounded once) from clip[b, n, m, :] with r = b_len[b, m];
 *     bleu_any[b, n] (f64) from clip_any[b, n, :] with r = the present b_len[b, m] closest to la, the shorter one on a tie;
 *     bp[b, n] (f64, may be NULL) = the BP of bleu_any (0 without a present reference).
 *   smoothing: 0 none, 1 add one (Lin & Och 2004; nltk's SmoothingFunction.method2).
 *   K35 has no Ta / Tb and takes the lengths as they are (a negative one as 0), where K34 clamps them to 0 .. Ta / Tb: pass lengths within
 *   those ranges (case_sentence_compact's always are), or the two kernels see different lengths for the same row.
 * ------------------------------------------------------------------------------------------- */
int case_ngram_counts(const int64_t* a, const int32_t* a_len, const int64_t* b, const int32_t* b_len, int32_t* clip, int32_t* clip_any,
                      int32_t* hit, int32_t* hit_any, int32_t* distinct, int64_t B, int64_t N, int64_t M, int64_t Ta, int64_t Tb,
                      int32_t max_n, case_stream_t stream);
int case_bleu_scores(const int32_t* clip, const int32_t* clip_any, const int32_t* a_len, const int32_t* b_len, float* bleu_pair,
                     double* bleu_any, double* bp, int64_t B, int64_t N, int64_t M, int32_t max_n, int32_t smoothing, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * ROUGE-1 .. ROUGE-4 on token ids (CASE_FEAT_ROUGE_N; purely additive, generation 600 unchanged).  The metric is evaluation/Rouge.py:140-183
 * (rouge_n), a SET measure: with E and R the distinct k-grams of the hypothesis and of the reference and o = |E & R|,
 *     P = o / |E|,  R = o / |R|  (0.0 where the denominator is 0),  F = 2.0 * ((P * R) / (P + R + 1e-8)).
 * K34 gives o (hit) and |E| (distinct); K43 gives |R| for rows of any length.
 * K43 case_ngram_distinct: b int64 [rows, Tb] front-packed ids, b_len int32 [rows] (clamped to 0 .. Tb), ids compared on their low 32 bits
 *   (the caller guarantees 0 <= id < 2^31, not checked); max_n in 1 .. 4.  distinct int32 [rows, 4]: entry k - 1 = the number of distinct
 *   k-grams of the row's first b_len ids for k <= max_n; the orders above max_n read 0, and so does a row shorter than k.  Exact.
 *   One wave per row, several rows per workgroup, no atomics, nothing read back: capturable, and two launches give the same bits.  Tb has no
 *   limit: the row is counted in windows of 256 positions (64 / 128 for Tb <= 64 / 128) that overlap by 3, and every window is compared with
 *   the whole row before it, so a row of L ids costs about L^2 / 500 token steps of wave-wide mask arithmetic -- quadratic in L.
 *   On rows of at most 256 positions the result is K34's distinct[b, n, :] bit for bit.
 * K44 case_rouge_n_scores: hit int32 [B, N, M, 4] and hyp_distinct int32 [B, N, 4] (K34's hit and distinct), ref_distinct int32 [B, M, 4]
 *   (K43's, or K34's distinct when the references are the hypotheses), b_len int32 [B, M] (<= 0: the reference is absent).  For every order
 *   k <= max_n (index k - 1 of the last axis), in f64 in the order above, without contraction:
 *     f_pair[b, n, m, k] (f32, rounded once) = F of hypothesis n against reference m; 0 for an absent reference;
 *     f, p, r [b, n, k] (f64) = F, P, R against the present reference with the largest F, the lowest index among equals;
 *     best_ref[b, n, k] (int32) = that index; -1 without a present reference, and then f = p = r = 0.
 *   The orders above max_n are not evaluated: f_pair, f, p, r read 0 and best_ref -1.
 * ------------------------------------------------------------------------------------------- */
int case_ngram_distinct(const int64_t* b, const int32_t* b_len, int32_t* distinct, int64_t rows, int64_t Tb, int32_t max_n,
                        case_stream_t stream);
int case_rouge_n_scores(const int32_t* hit, const int32_t* hyp_distinct, const int32_t* ref_distinct, const int32_t* b_len, float* f_pair,
                        double* f, double* p, double* r, int32_t* best_ref, int64_t B, int64_t N, int64_t M, int32_t max_n,
                        case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * TREC ranking metrics of score rows (CASE_FEAT_RANK_METRICS; purely additive, generation 600 unchanged): what evaluation/Eval_Trec.py
 * asks pytrec_eval for (map, ndcg, recall), plus recip_rank and P_1; evaluation/trec.py states the definitions.
 * K36 case_rank_metrics: every row b of scores f32 [B, P] is one query with P document slots; keys int32 [B, P] (NULL: the column index)
 *   breaks ties, rel int32 [B, P] holds the grades, valid u8 [B, P] (NULL: all) says which slots were retrieved (the rel of any other is
 *   ignored), extra_rel int32 [B, R] (NULL with R = 0) the grades of judged documents that were not retrieved (<= 0: padding).
 *   Rank order: score descending, the larger key first among equal scores, the lower column among equal (score, key); -0.0 == +0.0, a NaN
 *   score compares as -inf.  A document is relevant when its grade is >= 1, a negative grade counts as 0; num_rel counts the relevant ones
 *   among the retrieved slots and extra_rel.
 *     order[b, r]   int32: the column at rank r (0-based), -1 behind the retrieved ones
 *     metrics[b, :] f64 x 13: map, ndcg (gain = grade, discount log2(rank + 1), ideal list over all judged grades), recall_5, _10, _15, _20,
 *                   _30, _100, _200, _500, _1000 (relevant in the top min(k, retrieved) / num_rel), recip_rank, P_1; all 0 where num_rel == 0
 *     num_rel[b]    int32
 *   Counts are exact, every ratio is one f64 division, the f64 sums of map and ndcg go through a tree of fixed shape: two launches give the
 *   same bits.  P <= 1024 and P + R <= 2048, or CASE_E_UNSUPPORTED.  Asynchronous on `stream`; every output element is written.
 * ------------------------------------------------------------------------------------------- */
int case_rank_metrics(const float* scores, const int32_t* keys, const int32_t* rel, const uint8_t* valid, const int32_t* extra_rel,
                      int32_t* order, double* metrics, int32_t* num_rel, int64_t B, int64_t P, int64_t R, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The supporting-token stage (CASE_FEAT_TOKEN_LABELS; purely additive, generation 600 unchanged): its supervision and its best tokens.
 * K37 case_token_labels: the reference's CaSEDataset.py token_label on tensors (common/Utils.py token_label states the rule).  For every row
 *   x[0..L) of passage int64 [B, P, L], with A = the ids of response int64 [b, 0..T) other than `pad` and f = freq ([F], f32, or int64 with
 *   freq_is_i64 != 0; f[v] = 0 for v >= F):
 *     label[i]  = g1[i] = 1 where x[i] is in A (pad never is), else 0
 *     g3[i], g5[i] = the number of DISTINCT ids in A among x[i-1 .. i+1] and x[i-2 .. i+2] (positions outside the row read pad)
 *     lf[i] = ln(f[x[i]] + 2),  S = the sum of lf over all L positions (PAD positions included)
 *     weight[i] = (S / lf[i] * g3[i] * g5[i]) ^ 0.2 where g1[i] = 1, exactly 1 elsewhere
 *   label, weight f32 [B, P, L].  ln, the sum (a tree of fixed shape) and the power are f64, the result is rounded once: two launches give
 *   the same bits.  Ids must lie in [0, 2^31); L <= 16384 and T <= 1024, or CASE_E_UNSUPPORTED.
 * K38 case_token_select: every row of values f32 [B, S] is one item; valid u8 [B, S] (NULL: all) says which positions hold a token.
 *     pos[b, r] int32: the position at rank r (0-based) in the order: value descending (K36's map: -0.0 == +0.0, NaN as -inf), then the
 *                      LOWER position; an invalid position is never selected; -1 behind the valid ones.    val[b, r] f32: values at pos, 0 there
 *   With labels f32 [B, S] (then counts must be given, else both NULL) counts int32 [B, 5] = n_valid, n_pos (valid and label > 0.5), n_pred
 *   (valid and score > 0; scores f32 [B, S], NULL: values), tp (both), hits (label > 0.5 among the selected).
 *   S <= 16384 and K <= 256, or CASE_E_UNSUPPORTED.
 * Both are asynchronous on `stream`, use no atomics and write every output element.
 * ------------------------------------------------------------------------------------------- */
int case_token_labels(const int64_t* passage, const int64_t* response, const void* freq, int32_t freq_is_i64, float* label, float* weight,
                      int64_t B, int64_t P, int64_t L, int64_t T, int64_t F, int64_t pad, case_stream_t stream);
int case_token_select(const float* values, const uint8_t* valid, const float* scores, const float* labels, int32_t* pos, float* val,
                      int32_t* counts, int64_t B, int64_t S, int32_t K, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Threshold-free ranking metrics of the supporting-token stage (no feature bit: the 32-bit mask is full, so ask the library for the
 * symbol; purely additive, generation 600 unchanged).  evaluation/token_rank.py states the definitions.
 * K45 case_token_rank: every row of scores f32 [B, S] is one item; valid u8 [B, S] (NULL: all) says which positions hold a token, a valid
 *   position is positive where labels f32 [B, S] exceeds 0.5.  Scores compare as K38's key (-0.0 == +0.0, NaN as -inf); the valid
 *   positions fall into groups of equal key, g = 1 .. G from the highest key down, with tp_g / n_g the positives / positions through group g.
 *   No figure depends on the order inside a group, hence none on where in the row a token sits.
 *     counts[b, :] int32 x 6: n_valid, n_pos, auc_num2 = sum_g pos_g (2 (n_neg - negcum_g) + neg_g), best_tp, best_n (tp_g and n_g of the
 *                  lowest g that maximises 2 tp_g / (n_g + n_pos), fractions compared exactly), n_groups
 *     stats[b, :]  f64 x 2: ap = (1 / n_pos) sum_g (tp_g - tp_{g-1}) tp_g / n_g (0 where n_pos == 0); auc = auc_num2 / (2 n_pos n_neg), one
 *                  division of exact integers (0 where n_pos n_neg == 0)
 *     threshold[b] f32: the score of the best group in canonical form (+0.0 for either zero, -inf for NaN); n_pos == 0: best_tp = best_n
 *                  = 0 and +inf
 *   One workgroup per item sorts the row's (key, label) pairs in LDS (8 bytes per position of the row length padded to a power of two,
 *   128 KiB at 16384); every AP term is rounded once and summed through a tree of fixed shape, no atomics: two launches give the same bits.
 *   S <= 16384, or CASE_E_UNSUPPORTED; B == 0 returns without a launch.  Asynchronous on `stream`; every output element is written.
 * ------------------------------------------------------------------------------------------- */
int case_token_rank(const float* scores, const uint8_t* valid, const float* labels, double* stats, int32_t* counts, float* threshold,
                    int64_t B, int64_t S, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Answer attribution (CASE_FEAT_COPY_ATTRIBUTION; purely additive, generation 600 unchanged).
 * K39 case_copy_attribution: where the pointer mass of a target comes from.  Operands as in K29 (case_pointer_head_score) without the logits:
 *   mix_logits [R, 1 + nmem] f32, keys [R / rows_per_source, S] (row r reads key row r / rows_per_source), copies / lens with R rows and
 *   sum lens = S, targets [R] int64, pad (-1: none).  seg_start int32 [G + 1] cuts the source positions 0 .. S - 1 into G segments
 *   [seg_start[g], seg_start[g + 1]): strictly ascending, seg_start[0] = 0, seg_start[G] = S; the cuts need not coincide with the
 *   memories'.  With y = targets[r], pm = softmax(mix_logits[r]) (f32, as K29), the run = the source positions s whose id is y and
 *   term(s) = pm[1 + k(s)] copies[k(s)][r, s - the lengths before k(s)] (an f32 product):
 *     mass[r, g]  f32  the sum of term(s) over the run's positions in segment g (f64 per lane, a fixed tree, rounded once)
 *     pos[r]      int32  the run's position with the largest term, the LOWER position among equal terms (an all-zero run: its first)
 *     pos_mass[r] f32  that term        count[r] int32  the length of the run
 *   y == pad, y outside [0, V) or a y the item's source does not hold: mass 0, pos -1, pos_mass 0, count 0.
 *   The boundaries come from `seg_start_host` (host memory: checked here, CASE_E_ARG when they do not ascend from 0 to S, and handed to the
 *   kernel by value; `seg_start` is then ignored) or, when that is NULL, from `seg_start` in DEVICE memory, which is not read back: the
 *   caller has checked it (whatever it holds, the kernel reads and writes inside its operands).  One wave per row, no logits row is read,
 *   no atomics: two launches give the same bits.  nmem <= 4, S <= 32768, V <= 131071, 1 <= G <= 64, or CASE_E_UNSUPPORTED.
 *   Asynchronous on `stream`; every output element is written.
 * ------------------------------------------------------------------------------------------- */
int case_copy_attribution(const float* mix_logits, const uint32_t* keys, int64_t rows_per_source, const float* const* copies, const int64_t* lens,
                          int32_t nmem, const int64_t* targets, int64_t pad, const int32_t* seg_start, const int32_t* seg_start_host, int32_t G,
                          float* mass, int32_t* pos, float* pos_mass, int32_t* count, int64_t R, int64_t V, int64_t S, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * METEOR on token ids (CASE_FEAT_METEOR; purely additive, generation 600 unchanged).  The metric is nltk's meteor_score, which
 * evaluation/Eval_Meteor.py calls, with its exact stage on ids and its stem / synonym stages as ONE caller-provided table of equivalence
 * classes; evaluation/meteor.py states the rule.
 * K40 case_meteor: a, a_len, b, b_len exactly as case_lcs_pairs takes them (front-packed ids, lengths clamped to 0 .. Ta / Tb, ids compared
 *   on their low 32 bits, Ta <= 256 or CASE_E_UNSUPPORTED, Tb without such a limit).  For hypothesis h = a[b, n, 0 .. la) and reference
 *   r = b[b, m, 0 .. lb):
 *     stage 1: for i = la - 1 .. 0, the LAST still-unmatched j with r[j] == h[i] is matched to i;
 *     stage 2 (classes != NULL: int32 [V] in device memory, id -> class): the same over the positions stage 1 left, comparing classes[id]; an
 *              id outside [0, V) or with a negative entry has no class and never matches here.  classes == NULL requires V == 0;
 *     chunks:  over the matches sorted by i, 1 + the number of consecutive pairs (i, j), (i', j') that are not i' == i + 1 and j' == j + 1;
 *     score:   with mt = the number of matches, 0 when mt == 0, else P = mt / la, R = mt / lb, fmean = P R / (alpha P + (1 - alpha) R),
 *              pen = gamma pow(chunks / mt, beta), score = (1 - pen) fmean, in f64 in this order without contraction.
 *   counts int32 [B, N, M, 3] = (mt, the matches of stage 1, chunks), all 0 for an absent reference (lb == 0) and for la == 0; chunks 0 when
 *   mt == 0.  meteor_pair f32 [B, N, M] = the score rounded once.  meteor f64 [B, N] = the maximum over the present references, best_ref
 *   int32 [B, N] the lowest index that reaches it; 0 and -1 without a present reference.  align int32 [B, N, M, Ta] (may be NULL) = the matched
 *   reference position of every hypothesis position, -1 where there is none.
 *   alpha and gamma in [0, 1], beta >= 0, all finite (CASE_E_ARG otherwise); nltk's defaults are 0.9, 3.0, 0.5.
 *   One wave per hypothesis, no atomics, integer arithmetic up to the one score evaluation: two launches give the same bits.
 *   Asynchronous on `stream`; every output element is written.
 * ------------------------------------------------------------------------------------------- */
int case_meteor(const int64_t* a, const int32_t* a_len, const int64_t* b, const int32_t* b_len, const int32_t* classes, int64_t V, double alpha,
                double beta, double gamma, int32_t* counts, float* meteor_pair, double* meteor, int32_t* best_ref, int32_t* align, int64_t B,
                int64_t N, int64_t M, int64_t Ta, int64_t Tb, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Minimum-risk training (CASE_FEAT_RISK_TRAIN; purely additive, generation 600 unchanged): the differentiable score head and the
 * expected cost of a pool of candidates under the renormalised model posterior (evaluation/risk.py states the rule).
 * case_pointer_head_score_stats: K29 (case_pointer_head_score: same operands, same kernel, same prob / copy bits) with one more nullable
 *   output, stats f32 [R, 2] = the row's final (max, sum exp(logit - max)) of the online softmax; (0, 0) for a row that is not scored
 *   (target == pad or outside [0, V)).
 * K41 case_pointer_head_score_bwd: the gradient of prob.  K29's operands; ids int64 [R / rows_per_source, S] = the UNSORTED source ids the
 *   keys were sorted from; stats and prob as the forward wrote them; g f32 [R] = dL/dprob.  For row r with y = targets[r] scored, pm and
 *   gen_v = exp(logits[r, v] - stats[r, 0]) / stats[r, 1] as in K29, c_k = sum of copies[k][r, s] over the positions s of memory k with id y:
 *     d_logits[r, v] = g pm[0] gen_y ((v == y) - gen_v)                          f32 [R, V]
 *     d_mix[r, j]    = g pm[j] (a_j - prob[r]),  a_0 = gen_y, a_{1+k} = c_k      f32 [R, 1 + nmem]
 *     d_copies[k][r, s] = g pm[1 + k] where the id at that position is y, else 0 f32 [R, len_k]
 *   A row that is not scored writes zeros everywhere: every output element is written.  One workgroup per row, the logits read once,
 *   no atomics, reductions in a fixed order: two launches give the same bits.  Limits as K29 (nmem <= 4, S <= 32768, V <= 131071;
 *   CASE_E_UNSUPPORTED otherwise).
 * K42 case_sequence_risk: token_probs f32 [B, N, T], scored uint8 [B, N, T], cost f32 [B, N], valid uint8 [B, N] (NULL: all).  Per item,
 *   over the valid candidates n:  l_n = sum_{scored t} ln max(p[n, t], 1e-30);  Q_n = softmax_n(alpha l_n) (0 where invalid);
 *   risk = sum_n Q_n cost_n;  grad_p[n, t] = alpha Q_n (cost_n - risk) / p[n, t] on scored positions with p > 1e-30, else 0.  f64
 *   throughout, every output rounded to f32 once: risk [B], q [B, N], grad_p [B, N, T].  An item without a valid candidate: all zeros.
 *   alpha >= 0 and finite (CASE_E_ARG otherwise); N <= 64, T <= 1024 (CASE_E_UNSUPPORTED otherwise).  One wave per item, no atomics:
 *   two launches give the same bits.
 * All three are asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------- */
int case_pointer_head_score_stats(const float* logits, const float* mix_logits, const uint32_t* keys, int64_t rows_per_source,
                                  const float* const* copies, const int64_t* lens, int32_t nmem, const int64_t* targets, int64_t pad,
                                  float* prob, float* copy, float* stats, int64_t R, int64_t V, int64_t S, case_stream_t stream);
int case_pointer_head_score_bwd(const float* logits, const float* mix_logits, const int64_t* ids, int64_t rows_per_source,
                                const float* const* copies, const int64_t* lens, int32_t nmem, const int64_t* targets, int64_t pad,
                                const float* stats, const float* prob, const float* g, float* d_logits, float* d_mix, float* const* d_copies,
                                int64_t R, int64_t V, int64_t S, case_stream_t stream);
int case_sequence_risk(const float* token_probs, const uint8_t* scored, const float* cost, const uint8_t* valid, double alpha, float* risk,
                       float* q, float* grad_p, int64_t B, int64_t N, int64_t T, case_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The loss-only head of the training step (purely additive, generation 600 unchanged).  The 32-bit feature mask is full: a caller
 * detects the pair by symbol lookup (dlsym of case_pointer_head_loss).
 * case_pointer_head_loss: case_pointer_head_score_stats over logits rows `ld_logits` floats apart (ld_logits >= V, a multiple of 4, on a
 *   16-byte base: the rows of a vocabulary GEMM whose N is padded to its tile; columns [V, ld_logits) are never read), with one more
 *   output: nll f32 [R] = -log(prob + 1e-8), 0 for a row whose target is `pad`.  prob / copy / stats carry the bits
 *   case_pointer_head_score_stats gives for the same logits values in a contiguous [R, V] buffer on a 16-byte boundary.  stats and nll
 *   are required.
 * case_pointer_head_loss_bwd: K41 for that loss.  g_nll f32 [R] = dL/dnll; the kernel uses g = -g_nll / (prob + 1e-8) where K41 takes
 *   dL/dprob.  logits and d_logits rows lie `ld_logits` elements apart (>= V, a multiple of 8, 16-byte bases).  d_logits has `d_dtype`
 *   (CASE_F32 or CASE_BF16: K41's f32 expression rounded once to nearest even) and EVERY element of it is written: columns
 *   [V, ld_logits) as zeros, so a GEMM may reduce over the padded width.  d_mix and d_copies as K41.
 * Limits, determinism and error codes as K29 / K41.  Both are asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------- */
int case_pointer_head_loss(const float* logits, int64_t ld_logits, const float* mix_logits, const uint32_t* keys, int64_t rows_per_source,
                           const float* const* copies, const int64_t* lens, int32_t nmem, const int64_t* targets, int64_t pad, float* prob,
                           float* copy, float* stats, float* nll, int64_t R, int64_t V, int64_t S, case_stream_t stream);
int case_pointer_head_loss_bwd(const float* logits, int64_t ld_logits, const float* mix_logits, const int64_t* ids, int64_t rows_per_source,
                               const float* const* copies, const int64_t* lens, int32_t nmem, const int64_t* targets, int64_t pad,
                               const float* stats, const float* prob, const float* g_nll, void* d_logits, int32_t d_dtype, float* d_mix,
                               float* const* d_copies, int64_t R, int64_t V, int64_t S, case_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CASE_HIP_H */
