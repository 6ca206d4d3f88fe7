/* icka_hip.h -- C-ABI of libicka_hip.so: the MI355X (gfx950) kernels behind the ICKA MNER hot path.
 *
 * The reference (buctcurry/ICKA) has no FFI / plugin layer: its hot path is PyTorch nn.Module code that lowers to
 * ATen kernels.  Each entry point below therefore names the reference *Python* interface
 * (file:line under /root/reference) whose ATen kernel sequence it replaces.  Plain pointers and sizes only; no
 * torch types.  Every pointer is a DEVICE pointer unless stated; `stream` is a hipStream_t passed as void*.
 * bf16 tensors are passed as `const void*` to 2-byte elements; "f32" means float.
 *
 * Return value: 0 on success, a positive hipError_t from the launch, or a negative ICKA_E_* argument error.
 * Nothing here allocates, frees or synchronises: every call is stream-ordered and hipGraph-capturable.
 *
 * Re-entrancy: the compute entry points read NO mutable process state.  What varies between launches of
 * one shape -- the alternative kernels the tests exercise, A/B runs of a heuristic -- is an explicit per-call argument
 * (icka_gemm_desc.tune, the `flags` of icka_attn_* / icka_lstm_*) or an ICKA_TUNE_* environment variable read ONCE when the
 * library is loaded; there are no tuning setters.  The only process-wide controls left are documented where they are declared:
 * the dropout nonce registration (icka_set_dropout_nonce), the error words of the persistent kernels
 * (icka_lstm_clear_error, icka_dp_clear_error), the CU reservation beside RCCL (icka_lstm_set_reserved_cus) and the test hooks
 * of the give-up paths (icka_lstm_test_hooks, icka_gemm_ln_test_hooks).
 */
#ifndef ICKA_HIP_H
#define ICKA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICKA_E_SHAPE (-1)   /* dimension out of the supported range */
#define ICKA_E_ALIGN (-2)   /* pointer / leading dimension not 16-byte aligned where vector access needs it */
#define ICKA_E_ARG (-3)     /* null pointer or inconsistent descriptor */

/* library / ABI version, and the code-object architecture it was built for ("gfx950") */
/* 2: round 2 -- icka_gemm_desc grew (ab_f16, C3, ldc3, aux_f16), c_is_f32 may be 2 (fp16 output); new entry points
 * icka_ln_fwd_h, icka_embed_fwd_h, icka_attn_fwd_ex, icka_cls_head_fwd_h, icka_cast_*f16, icka_conv3x3_gemm.
 * 3: icka_lstm_set_handoff, icka_lstm_set_batch_split, icka_attn_dropout_mask (additive).
 * 4: round 3 -- icka_lstm_clear_error, icka_lstm_set_reserved_cus, icka_lstm_test_hooks; a hand-off wait that gives up now
 *    NaN-poisons the recurrence and raises a host-visible error word; icka_gemm_desc.C3 may accompany an f32 main output
 *    (the data-parallel wire copy, c3_only); icka_dp_*; icka_regions_to_tokens_h, icka_sample_gate_fwd_h, icka_optim_* (additive).
 * 5: round 4 -- icka_dp_flag_wait's third argument is the bucket's BAD WORD (it no longer writes the NaN itself);
 *    icka_dp_poison_if, icka_dp_poison_final, icka_copy_many, icka_embed_bwd_rows, icka_embed_scatter_rows,
 *    icka_ln_set_rows_per_wave, icka_gemm_set_square_tiles, icka_gemm_set_persistent (additive); icka_gemm refuses an f32 output with a wire copy (C3) unless op == TN.
 * 6: round 5 -- every tuning setter is GONE (icka_gemm_set_*, icka_ln_set_rows_per_wave, icka_attn_set_whole_head,
 *    icka_lstm_set_persistent / _handoff / _batch_split): icka_gemm_desc grew `tune`; icka_attn_fwd_ex's `fp8` argument became
 *    `flags`; icka_attn_bwd, icka_lstm_fwd and icka_lstm_bwd take `flags`; the 256x256-tile and persistent 12-wave GEMM kernels
 *    those setters switched on left the library (profiles/NEGATIVE_RESULTS.md); icka_gemm_ln, icka_gemm_ln_sync_words, icka_gemm_ln_test_hooks, icka_gemm_qkv_attn (additive).
 *    Later, still 6: icka_contrastive_fwd, icka_contrastive_bwd, icka_contrastive_workspace_floats, icka_relu_bwd,
 *    icka_sample_swap (additive: the auxiliary objective of the gated taggers, csrc/objective.hip); icka_optim_prepare,
 *    icka_optim_adamw_dev and the icka_optim_state block (additive: the capturable parameter update); icka_optim_average,
 *    icka_optim_average_prepare, icka_optim_average_dev, icka_optim_swap and the icka_average_state block (additive: EMA / SWA
 *    weight averaging); icka_sam_sqnorm, icka_sam_prepare, icka_sam_ascend, icka_sam_restore and the icka_sam_state block
 *    (additive: sharpness-aware minimisation, csrc/sam.hip). */
#define ICKA_ABI_VERSION 6
int icka_abi_version(void);
const char* icka_build_arch(void);

/* n <= 8 device-to-device copies (dst[i] <- src[i], bytes[i] bytes; src / dst / bytes are HOST arrays) in one launch: the
 * per-call input refresh of a captured step (icka_amd/graph.py: StaticInputs), which stands where the reference's loop
 * moves a new batch to the device every step (My_cross_attention.py:797-798).  16-byte words when pointers and size allow. */
int icka_copy_many(const void* const* src, void* const* dst, const int64_t* bytes, int32_t n, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * GEMM on MFMA (v_mfma_f32_16x16x32_bf16), bf16 operands, fp32 accumulate.
 *   op NT :  C[M,N] = A[M,K]   . B[N,K]^T      (nn.Linear forward: x @ W^T, W is [out,in])
 *   op NN :  C[M,N] = A[M,K]   . B[K,N]        (input gradient: dY @ W)
 *   op TN :  C[M,N] = A[K,M]^T . B[K,N]        (weight gradient: dY^T @ X, K = tokens)
 * Replaces nn.Linear / torch.matmul call sites: Cross_Modal_Interaction_Module.py:479-481 (Q,K,V), :533,:549,:562
 * (dense layers), :958 (vismap2text), my_bert/cl_modeling.py:1363,:1371 (gates, classifier) and their autograd.
 * The reduction may be split in two segments read from different buffers (k < K1 from A/B, k >= K1 from A2/B2):
 * that is how cat(seq, cross) operands (cl_modeling.py:1363-1370) are consumed without materialising the concat.
 */
enum { ICKA_GEMM_NT = 0, ICKA_GEMM_NN = 1, ICKA_GEMM_TN = 2 };
enum {
    ICKA_EPI_NONE = 0,  /* C = alpha*acc (+bias) (+beta*C)                                                  */
    ICKA_EPI_GELU = 1,  /* z = acc+bias ; C2 = z ; C = z*0.5*(1+erf(z/sqrt2))   (BertIntermediate, :548-551)   */
    ICKA_EPI_DGELU = 2, /* C = acc * gelu'(aux)                                  (its backward)                */
    ICKA_EPI_ADD = 3,   /* C = acc (+bias) + aux                                 (gradient fan-in)             */
    ICKA_EPI_GATE = 4,  /* g = sigmoid(acc+bias) ; C2 = g ; C = g*aux            (cl_modeling.py:1363-1367)    */
    ICKA_EPI_TANH = 5,  /* C = tanh(acc+bias)                                    (BertPooler, :675-681)        */
    ICKA_EPI_RELU = 6,  /* C = max(acc+bias, 0)                 (conv+BN+ReLU, resnet/resnet.py:75-81)          */
    ICKA_EPI_ADD_RELU = 7 /* C = max(acc+bias+aux, 0)           (bottleneck residual, resnet/resnet.py:83-90)   */
};
typedef struct icka_gemm_desc {
    int32_t op;            /* ICKA_GEMM_* */
    int32_t M, N, K;
    int32_t K1;            /* 0 = single segment; else multiple of 64, 0 < K1 < K */
    const void* A;  int64_t lda;    /* bf16 */
    const void* B;  int64_t ldb;    /* bf16 */
    const void* A2; int64_t lda2;   /* second-segment operands (K1 > 0) */
    const void* B2; int64_t ldb2;
    void* C;  int64_t ldc;  int32_t c_is_f32;   /* output bf16 (0), f32 (1) or fp16 (2, see ab_f16 below) */
    void* C2; int64_t ldc2;                     /* bf16 second output (GELU: z, GATE: g) */
    const void* aux; int64_t ldaux;             /* bf16 epilogue operand */
    const float* bias;                          /* f32 [N] or NULL */
    const float* bias2;                         /* optional second f32 [N] bias (two Linear layers summed) */
    float alpha, beta;
    int32_t epilogue;      /* ICKA_EPI_* */
    float* colsum_out;     /* op TN only, fast path (M,N %128, K %64): colsum_out[m] (+)= sum_k A[k,m]  -- the bias
                              gradient db = colsum(dY) produced by the weight-gradient GEMM dW = dY^T.X itself */
    int32_t colsum_accumulate;
    /* "mixed16" forward GEMMs (op NT only): operands A, B (A2, B2) are IEEE fp16 instead of bf16
     * (v_mfma_f32_16x16x32_f16, same rate); c_is_f32 == 2 makes the main output fp16 (saturating at +-65504, beta must
     * be 0) and C3, if not NULL, receives a bf16 copy of it (the operand the bf16 weight-gradient GEMM reads later).
     * With an f32 main output (c_is_f32 == 1, op TN ONLY: other ops return ICKA_E_ARG) C3 is the DATA-PARALLEL WIRE COPY: a bf16 copy of the final value
     * (after beta-accumulation) written by the same epilogue -- the weight-gradient GEMMs fill the bf16 all-reduce buffer
     * of icka_amd/dp.py themselves instead of a separate cast pass over the gradients (see icka_dp_* below). */
    int32_t ab_f16;
    void* C3; int64_t ldc3;
    int32_t aux_f16;       /* the epilogue operand `aux` is fp16 instead of bf16 (mixed16 gate: sigmoid(.) * cross_fp16) */
    int32_t c3_only;       /* f32 C with a wire copy C3, beta == 0, no epilogue: store ONLY C3 (2 bytes per element instead of
                              4 + 2); C is left untouched -- icka_amd/dp.py writes it from the reduced wire buffer
                              (icka_dp_cast_back_scaled), which is the only consumer of such a gradient before that point */
    uint64_t tune;         /* 0 = the library's per-shape heuristics (the ICKA_TUNE_GEMM_* environment read at load, if set);
                              else an OR of ICKA_TUNE_* words that force single choices for THIS call (tests of the alternative
                              kernels, probes).  Results never depend on it; a code outside a field's range is ICKA_E_ARG.
                              A grouped launch takes the word of its first problem. */
} icka_gemm_desc;
/* icka_gemm_desc.tune fields (4 bits each; environment equivalents in parentheses):
 *   RING(n)        LDS-DMA ring depth of the fast path, n = 2 .. 5 (ICKA_TUNE_GEMM_RING): 2 = 64 KiB, two blocks per CU; 3 / 4 =
 *                  96 / 128 KiB, one block per CU, one / two k-tiles of DMA kept in flight across the barrier.  Default: ring 2
 *                  with two co-resident blocks for short-K grids of >= ~2 tiles per CU, ring 3 otherwise.
 *   TILE_N(n)      output-tile width of the warp-specialised path, n = 96 | 128 (ICKA_TUNE_GEMM_TILE_N).  Default: the narrower
 *                  tile when it quantises better onto the 256 CUs (N = 768: 256 tiles instead of 192); 96 needs N % 96 == 0.
 *   WIDE_TILES(b)  256x192 / 256x128 tiles of the 12-wave kernel for wide outputs with a short reduction whose tile grid
 *                  covers the CUs in one round (ICKA_TUNE_GEMM_WIDE_TILES; default on).
 *   DIRECT_EPILOGUE(b)  f32 outputs without activation / fan-in operand / accumulate stored straight from the MFMA
 *                  accumulators (default on); off: every epilogue goes through the LDS C tile (ICKA_TUNE_GEMM_DIRECT_EPILOGUE).
 *   WARP_SPECIALIZED(v)  1 (default): 512-thread fast path (4 loader + 4 compute waves; two blocks per CU for large grids),
 *                  0: 256-thread single-role path, 2: force two blocks, 3: never two (ICKA_TUNE_GEMM_WARP_SPECIALIZED).
 *   W3_GRID(pm)    XCD cut of the 12-wave kernel's tile grid, pm = 1 | 2 | 4 | 8 where it divides the grid: the 8 XCDs (private
 *                  L2s) take a pm x pn patch grid of the tiles, the chip then fetches pn * |A| + pm * |B|
 *                  (ICKA_TUNE_GEMM_W3_GRID).  Default: the dividing cut with the smallest pn * M + pm * N.
 *   BIG_TILES(v)   grouped TN launches of plain f32 outputs with M % 256 == 0 (the weight gradients of a layer): 2 (default)
 *                  = 256x128 tiles in 12-wave blocks with the fused column sums in extra blocks of the grid, 1 = 8-wave
 *                  blocks, 0 = 128x128 tiles (ICKA_TUNE_GEMM_BIG_TILES).
 *   ABLATION(m)    diagnostic builds only, WRONG results: 1 = skip MFMA + LDS reads, 2 = skip the LDS-DMA staging. */
#define ICKA_TUNE_RING(n) ((uint64_t)(n) << 0)
#define ICKA_TUNE_TILE_N(n) ((uint64_t)((n) == 96 ? 1 : ((n) == 128 ? 2 : 15)) << 4)
#define ICKA_TUNE_WIDE_TILES(b) ((uint64_t)((b) ? 2 : 1) << 8)
#define ICKA_TUNE_DIRECT_EPILOGUE(b) ((uint64_t)((b) ? 2 : 1) << 12)
#define ICKA_TUNE_WARP_SPECIALIZED(v) ((uint64_t)((v) + 1) << 16)
#define ICKA_TUNE_W3_GRID(pm) ((uint64_t)(pm) << 20)
#define ICKA_TUNE_BIG_TILES(v) ((uint64_t)((v) + 1) << 24)
#define ICKA_TUNE_ABLATION(m) ((uint64_t)(m) << 28)
int icka_gemm(const icka_gemm_desc* d, void* stream);
/* icka_gemm with row-liveness flags of the A operand (op NN or NT: A is [M, K] row-major): a_row_live is NULL or M bytes,
 * 16-byte aligned; byte t may be 0 only if row t of A is all zero (icka_ln_bwd_slabs_live writes such bytes for the gradient
 * rows of a BERT layer).  The flags are a permission, never an obligation: the NN launches on 256x192 tiles (12-wave kernel)
 * and on 128x96 tiles (8-wave kernel, ring of 3) -- the input-gradient GEMMs of the encoder backward -- stage the 8-row pieces of
 * A that have no live row from a line of zeros instead of fetching them; every other launch, and a NULL pointer, is exactly
 * icka_gemm.  The staged tile holds the same zeros either way, so the result is bitwise that of icka_gemm for any B (non-finite
 * values included); the epilogue and its aux reads run for every row. */
int icka_gemm_live(const icka_gemm_desc* d, const uint8_t* a_row_live, void* stream);
/* n independent GEMMs; consecutive fast-path problems of one layout are packed (up to 4) into ONE launch so that
 * several partially-filling grids (the weight-gradient GEMMs of a layer) fill the chip together. */
int icka_gemm_grouped(const icka_gemm_desc* descs, int32_t n, void* stream);
/* Same, plus up to 4 slab reductions  out[slot][c] (+)= sum_b partials[b*slab_stride + slot*H + c]  (b < nslab,
 * slot < nslots <= 4, c < H; fixed summation order) that ride on the launch: the LayerNorm dgamma / dbeta slabs left
 * by icka_ln_bwd_slabs are summed by extra blocks of the layer's weight-gradient grid instead of a launch of their
 * own.  A 128x128 TN group takes them along the same way; without any eligible launch (or with n == 0) they share ONE small launch. */
typedef struct icka_slab_reduction {
    const float* partials; int64_t slab_stride; int32_t nslab, H, nslots, accumulate;
    float* out[4];
} icka_slab_reduction;
int icka_gemm_grouped_ex(const icka_gemm_desc* descs, int32_t n, const icka_slab_reduction* reds, int32_t n_red,
                         void* stream);
/* Same, plus optional row-liveness flags per problem: k_live (NULL, or n pointers, each NULL or K bytes, 16-byte
 * aligned) -- byte t of k_live[i] may be 0 only if row t of one of problem i's two operands is all zero (the weight
 * gradients: a token whose output gradient is zero; icka_ln_bwd_slabs_live writes such bytes).  The 12-wave 256x128
 * launch of TN problems then reduces over the 64-row k-tiles that have a live row; the result is bitwise the full
 * reduction whenever the other operand is finite (a skipped tile only adds +-0 to accumulators that started at +0;
 * with Inf / NaN there the full reduction gives NaN and the shortened one may not).  Every other path ignores the
 * flags and reduces over all of K.  The column sums and slab reductions of the launch are not affected. */
int icka_gemm_grouped_live(const icka_gemm_desc* descs, int32_t n, const icka_slab_reduction* reds, int32_t n_red,
                           const uint8_t* const* k_live, void* stream);
/* ---------------------------------------------------------------------------------------------------------------
 * Fused  y = LayerNorm(dropout(x + bias) + residual)   (BertSelfOutput.forward :561-565, BertOutput.forward
 * :532-536, BertLayerNorm.forward :518-522: biased variance, eps inside the sqrt).  One wave per row.
 *   x [M,H] bf16 or f32 (x_is_f32; row stride ldx in elements), bias f32[H] or NULL, residual [M,H] bf16 or f32
 *   (res_is_f32; ldr) or NULL, gamma/beta f32[H];  y [M,H] bf16 (ldy) is the MFMA operand of the next GEMM; y2
 *   optional second bf16 copy (ldy2); y_f32 optional contiguous f32 copy (the residual stream is carried in f32
 *   so bf16 rounding does not accumulate over layers); xhat [M,H] bf16 contiguous and rstd f32[M] are the saved
 *   statistics for backward (may be NULL in inference).
 * A forward wave owns two rows from 4096 rows on (the loads of its next row are issued before the current row is reduced and
 *   stored), else one; ICKA_TUNE_LN_ROWS_PER_WAVE = 1 .. 16 (read once at load) replaces that choice for A/B runs.
 */
int icka_ln_fwd(const void* x, int64_t ldx, int32_t x_is_f32, const float* bias, const void* residual, int64_t ldr,
                int32_t res_is_f32, const float* gamma, const float* beta, void* y, int64_t ldy, void* y2,
                int64_t ldy2, float* y_f32, void* xhat, float* rstd, int32_t M, int32_t H, float eps, float p_drop,
                uint64_t seed, void* stream);
/* dense -> bias + dropout + residual -> LayerNorm as ONE launch (BertSelfOutput.forward :561-565, BertOutput.forward :532-536 =
 * icka_gemm + icka_ln_fwd with the launch boundary replaced by a per-stripe arrival counter inside the kernel).  `d` describes the
 * dense GEMM exactly as icka_gemm would take it for this site: op NT, bf16 operands, C = the f32 intermediate [M, N] (written,
 * then read back by the LayerNorm phase), no bias / epilogue / accumulate in `d` (bias is the LayerNorm phase's, as in
 * icka_ln_fwd).  The remaining arguments are icka_ln_fwd's (x = d->C): residual [M, N] of kind res_kind (0 bf16, 1 f32,
 * 2 fp16; ldr), gamma / beta f32 [N], y bf16 [M, N] (ldy), y_twin contiguous f32 (twin_f16 = 0) or fp16 (1) or NULL, xhat
 * bf16 contiguous and rstd f32 [M] or NULL.  Results are BITWISE those of the two calls.
 * Eligible shapes: the aligned fast path (M % 128 == 0) with eight column tiles per 128-row stripe (N = 768 or 1024) and at most
 * one block per CU (the 8 blocks of a stripe wait for each other: all must be resident; M <= 4096 on a whole MI355X).  Anything
 * else returns ICKA_E_SHAPE and launches nothing: the caller takes the two calls.
 * and M / 128 * 8 blocks <= the device's CUs MINUS the caller's reserve (icka_lstm_set_reserved_cus: dp.GradReducer reserves
 * the CUs RCCL's workgroups may hold, so the fused form is not taken beside a collective).
 * sync_words: icka_gemm_ln_sync_words() 32-bit words of device memory, zero before the first use; every launch leaves them
 * zero again (the counters reset themselves, also after a failed launch), so one buffer serves all fused launches of a stream.
 * error_word: one 32-bit word the device can write -- HOST-MAPPED memory if the host wants to poll it without a device
 * synchronisation (icka_amd/kernels.py keeps a pinned word).  A stripe wait that gave up (bounded spin, ~7 ms: never a hang)
 * stores 1 there and turns the rows it finished into NaN: a failed launch never passes for a result.
 * icka_gemm_ln_test_hooks (tests of that path): polls > 0 replaces the poll budget (0 restores it); drop_block >= 0 makes
 * that block never arrive, so its stripe's waits give up (-1: off). */
int icka_gemm_ln(const icka_gemm_desc* d, const float* bias, const void* residual, int64_t ldr, int32_t res_kind,
                 const float* gamma, const float* beta, void* y, int64_t ldy, void* y_twin, int32_t twin_f16, void* xhat,
                 float* rstd, float eps, float p_drop, uint64_t seed, uint32_t* sync_words, uint32_t* error_word, void* stream);
int64_t icka_gemm_ln_sync_words(void);
int icka_gemm_ln_test_hooks(int32_t polls, int32_t drop_block);
/* The fused QKV projection and the self-attention of BertSelfAttention.forward (Cross_Modal_Interaction_Module.py:478-506:
 * query / key / value Linear, transpose_for_scores, scores / sqrt(d) + mask, softmax, dropout, context) as ONE launch, for
 * sequences of 128 tokens (the reference's max_seq_length) or 256 (BASELINE config c4) and head size 64.  `d` is the projection
 * exactly as icka_gemm takes it: op NT, A = hidden states [B * S, K], B = the stacked [Wq; Wk; Wv] [3 H, K] (both bf16, or both
 * fp16: the "mixed16" forward operands), bias = the stacked f32 bias, C = the bf16 [B * S, 3 H] activation [q | k | v] (WRITTEN
 * as by icka_gemm: the backward reads it), no epilogue / accumulate / copies.  The rest is icka_attn_fwd_ex's with Q / K / V = the
 * three column blocks of C: add_mask f32 [B, S], ctx bf16 [B * S, H] (ldo) and its optional fp16 copy ctx_f16 (same ldo), lse
 * f32 [B, heads, S] or NULL, scale, p_drop, seed (same dropout counters: icka_attn_bwd regenerates the same mask), keep_bits
 * (icka_attn_keepbits_words words or NULL; S = 256 only).
 * Each 256 x 192 tile of the 12-wave GEMM kernel is laid over 256 / S samples x ONE head's 64 + 64 + 64 columns, so the block
 * that produced q, k, v of a head runs that head's attention from LDS.  Results are BITWISE those of icka_gemm +
 * icka_attn_fwd_ex.  Eligible: S == 128 or 256, H = 64 * heads, B * S % 256 == 0, K % 64 == 0 and <= 1024, (B * S / 256) * heads
 * a multiple of 8 and >= 128; anything else returns ICKA_E_SHAPE and launches nothing: the caller makes the two calls. */
int icka_gemm_qkv_attn(const icka_gemm_desc* d, const float* add_mask, void* ctx, void* ctx_f16, int64_t ldo, float* lse,
                       int32_t B, int32_t heads, int32_t S, float scale, float p_drop, uint64_t seed, void* keep_bits, void* stream);
/* "mixed16" form of the same call: x_kind / res_kind are 0 = bf16, 1 = f32, 2 = fp16, and the twin copy of the output is
 * fp16 (y_f16, contiguous, saturating at +-65504): it is both the fp16 MFMA operand of the next forward GEMM and the
 * residual input of the next block, while y (bf16) stays the operand of the bf16 weight-gradient GEMM in backward. */
int icka_ln_fwd_h(const void* x, int64_t ldx, int32_t x_kind, const float* bias, const void* residual, int64_t ldr,
                  int32_t res_kind, const float* gamma, const float* beta, void* y, int64_t ldy, void* y2,
                  int64_t ldy2, void* y_f16, void* xhat, float* rstd, int32_t M, int32_t H, float eps, float p_drop,
                  uint64_t seed, void* stream);
/* Backward of the above.  dy (+ optional dy2) are the incoming gradients of y.  Outputs: dres = gradient of the
 * residual input (bf16, may be NULL), dx = gradient of x (dropout mask re-generated from seed; may be NULL),
 * and the f32 parameter gradients dgamma[H], dbeta[H], dbias[H] (dbias may be NULL): added to the existing values
 * when accumulate != 0, overwritten otherwise.  `partials` is f32 workspace of icka_ln_bwd_workspace_floats(H). */
int64_t icka_ln_bwd_workspace_floats(int32_t H);
int icka_ln_bwd(const void* dy, int64_t lddy, const void* dy2, int64_t lddy2, const void* xhat, const float* rstd,
                const float* gamma, void* dres, int64_t lddres, void* dx, int64_t lddx, float* dgamma, float* dbeta,
                float* dbias, float* partials, int32_t M, int32_t H, float p_drop, uint64_t seed, int32_t accumulate,
                void* stream);
/* The same backward without the parameter-gradient finalize: only dres / dx and the column slabs
 * partials[icka_ln_bwd_nslab(M)][icka_ln_slab_slots()][H] (slot 0: sum dy*xhat -> dgamma, slot 1: sum dy -> dbeta),
 * to be summed later by icka_gemm_grouped_ex. */
int icka_ln_bwd_slabs(const void* dy, int64_t lddy, const void* dy2, int64_t lddy2, const void* xhat, const float* rstd,
                      const float* gamma, void* dres, int64_t lddres, void* dx, int64_t lddx, float* partials, int32_t M,
                      int32_t H, float p_drop, uint64_t seed, void* stream);
/* icka_ln_bwd_slabs + row-liveness bytes of the rows it produced: row_live[row] (u8 [M], required) = 1 if any element
 * of the row's residual gradient (dres, BEFORE the dropout mask of dx) is non-zero, else 0 -- dx == 0 follows.
 * row_live_kv (u8 [M], optional; needs the additive key mask add_mask f32 [M / mask_S, mask_S]) additionally keeps a row
 * live while it can receive attention probability as a KEY: no key of its sample has a mask value 5000 or more
 * above its own (mask values are compared with each other, not with 0: exact for graded masks and for a sample whose
 * keys are all masked).  dres / dx / partials are bitwise those of icka_ln_bwd_slabs. */
int icka_ln_bwd_slabs_live(const void* dy, int64_t lddy, const void* dy2, int64_t lddy2, const void* xhat,
                           const float* rstd, const float* gamma, void* dres, int64_t lddres, void* dx, int64_t lddx,
                           float* partials, uint8_t* row_live, uint8_t* row_live_kv, const float* add_mask,
                           int32_t mask_S, int32_t M, int32_t H, float p_drop, uint64_t seed, void* stream);
int32_t icka_ln_bwd_nslab(int32_t M);
int32_t icka_ln_slab_slots(void);

/* ---------------------------------------------------------------------------------------------------------------
 * BertEmbeddings.forward (:398-412): y = dropout(LayerNorm(word[ids] + pos[arange(S)] + type[tt])).
 * Tables are the fp32 master parameters (gathered directly, no shadow copy).  ids/tt are int64 [B*S].
 */
int icka_embed_fwd(const int64_t* ids, const int64_t* token_type, const float* word, const float* pos,
                   const float* type, const float* gamma, const float* beta, void* y, float* y_f32, void* xhat,
                   float* rstd, int32_t B, int32_t S, int32_t H, int32_t vocab, int32_t n_type, float eps,
                   float p_drop, uint64_t seed, void* stream);
/* "mixed16" form: the twin copy of the output is fp16 (see icka_ln_fwd_h). */
int icka_embed_fwd_h(const int64_t* ids, const int64_t* token_type, const float* word, const float* pos,
                     const float* type, const float* gamma, const float* beta, void* y, void* y_f16, void* xhat,
                     float* rstd, int32_t B, int32_t S, int32_t H, int32_t vocab, int32_t n_type, float eps,
                     float p_drop, uint64_t seed, void* stream);
/* Backward.  dword / dpos are ALWAYS accumulated into with f32 atomics (the caller zeroes them for a fresh
 * gradient); dtype / dgamma / dbeta follow `accumulate` as in icka_ln_bwd.  Row `padding_idx` of the word table
 * receives no gradient (nn.Embedding(padding_idx=0), :387).  partials: icka_ln_bwd_workspace_floats(H) floats.
 * With accumulate = 0, dtype starts from zero for every n_type (n_type > 2 takes atomics onto a cleared table).
 * Ids and token types outside their table are CLAMPED, as in the forward: an id < 0 counts as row 0, an id >= vocab as
 * row vocab - 1, and padding_idx is compared with the clamped id (id -3 with padding_idx = 0 is a padding token; with
 * padding_idx = -1 no row is skipped).  dpos rows [0, S) are touched, no others.  H <= 2048 (64 KiB of dynamic LDS). */
int icka_embed_bwd(const void* dy, const int64_t* ids, const int64_t* token_type, const void* xhat,
                   const float* rstd, const float* gamma, float* dword, float* dpos, float* dtype, float* dgamma,
                   float* dbeta, float* partials, int32_t B, int32_t S, int32_t H, int32_t vocab, int32_t n_type,
                   int32_t padding_idx, float p_drop, uint64_t seed, int32_t accumulate, void* stream);
/* Row-sparse form for the data-parallel exchange of the word-embedding gradient (icka_amd/dp.py: GradReducer(sparse_embeddings=
 * True); reference: apex DDP all-reduces the dense [vocab, H] gradient, My_cross_attention.py:768-776): as icka_embed_bwd, but
 * the word-table gradient is left as per-token rows dtok f32 [B*S, H] (zero rows for padding_idx).  After an all-gather of every
 * rank's rows and ids, icka_embed_scatter_rows adds scale * rows[t] into dword[ids[t]] (f32 atomics; rows f32 or bf16; the
 * padding id and ids outside [0, vocab) are skipped; the caller zeroes dword for a fresh gradient).
 * icka_embed_bwd_rows clamps ids as icka_embed_bwd does: dtok of a token whose CLAMPED id equals padding_idx is a zero row,
 * every other row -- that of an id outside [0, vocab) included -- holds its gradient.  icka_embed_scatter_rows compares the
 * ids AS GIVEN and skips those outside the table, so the two calls add up to icka_embed_bwd for ids inside [0, vocab) only. */
int icka_embed_bwd_rows(const void* dy, const int64_t* ids, const int64_t* token_type, const void* xhat, const float* rstd,
                        const float* gamma, float* dtok, float* dpos, float* dtype, float* dgamma, float* dbeta, float* partials,
                        int32_t B, int32_t S, int32_t H, int32_t vocab, int32_t n_type, int32_t padding_idx, float p_drop,
                        uint64_t seed, int32_t accumulate, void* stream);
int icka_embed_scatter_rows(const void* rows, int32_t rows_are_bf16, const int64_t* ids, float* dword, int64_t T, int32_t H,
                            int32_t vocab, int32_t padding_idx, float scale, void* stream);
/* Embeddings of the prompt-accepting encoder stage that ends the current reference model
 * (Cross_Modal_Interaction_Module.py:1010-1012: last_encoder(input_ids=..., prompt_embeddings=prefix_emb, ...); its
 * package `local_transformers` is absent from the reference tree, so the splice rule is this build's definition, taken
 * from the reference's own offset arithmetic :1022 and the token dump at My_cross_attention.py:402-404):
 *   out[b, t] = dropout(LayerNorm(x + pos[t + pos_offset] + type[0])),   t in [0, S)
 *   x = word[ids[b, src[t]]]            if src[t] >= 0   (ids int64 [B, S_in])
 *     = prompt[b, -1 - src[t]]          otherwise        (prompt bf16 [B, P, H])
 * src is int32 [S], shared by the batch (the reference asserts equal offsets per batch, My_cross_attention.py:802). */
int icka_embed_prompt_fwd(const int64_t* ids, const int32_t* src, const void* prompt, const float* word,
                          const float* pos, const float* type, const float* gamma, const float* beta, void* y,
                          float* y_f32, void* xhat, float* rstd, int32_t B, int32_t S_in, int32_t S, int32_t P,
                          int32_t H, int32_t vocab, int32_t pos_offset, float eps, float p_drop, uint64_t seed,
                          void* stream);
/* Backward: table gradients as icka_embed_bwd (dtype = row 0 only), plus dprompt bf16 [B, P, H] (each row written
 * once: src must name every prompt vector exactly once).  dpos rows [pos_offset, pos_offset + S) are added into, no
 * others.  S <= 1024 (ICKA_E_SHAPE beyond).  partials: S * icka_ln_slab_slots() * H floats. */
int icka_embed_prompt_bwd(const void* dy, const int64_t* ids, const int32_t* src, const void* xhat, const float* rstd,
                          const float* gamma, float* dword, float* dpos, float* dtype, float* dgamma, float* dbeta,
                          void* dprompt, float* partials, int32_t B, int32_t S_in, int32_t S, int32_t P, int32_t H,
                          int32_t vocab, int32_t pos_offset, int32_t padding_idx, float p_drop, uint64_t seed,
                          int32_t accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Adversarial training on the word embeddings: FGM (Miyato et al. 2017) and FreeLB (Zhu et al. 2020) as a per-token
 * perturbation (icka_amd/adversarial.py; csrc/adversarial.hip, the forward variant in csrc/layernorm.hip).
 *
 * The perturbation is delta f32 [B, S, H], one row per token position, added to the word row before the position and
 * type rows:
 *     s[b,t] = ((word[id] + delta[b,t]) + pos[t]) + type[tt],     y = dropout(LayerNorm(s))
 * A position is valid when input_mask[b,t] != 0 (int64 [B, S]); n_b = number of valid positions of sample b.
 * Gradient: g[b,t] = dloss / ddelta[b,t] is exactly the row icka_embed_bwd_rows writes to dtok (a zero row for a token
 * whose clamped id is the padding id).
 *
 * icka_embed_fwd_adv / _h: icka_embed_fwd / _h plus a nullable `delta`; with delta == NULL the very launch of
 * icka_embed_fwd / _h (y, twin, xhat, rstd bitwise).  delta 16-byte aligned, contiguous.
 *
 * icka_adv_ascend, one ascent step, in place on delta; per sample b, Frobenius norms over the valid positions only:
 *   1. n_g = ||g_b||.
 *   2. If n_g is 0 or not finite (an inf / NaN in g_b, or a sum of squares that overflows f32), delta_b stays as it is
 *      at the valid positions and is not projected.
 *   3. Otherwise u = delta_b + (alpha / n_g) g_b.
 *   4. Projection: if ||u|| > epsilon, u <- u (epsilon / ||u||).
 *   5. Every non-valid position of delta_b is written as exact 0, whatever it held before.
 *   6. norms[b] = (n_g, ||delta_b|| after the step) f32 [B, 2]; the second entry is epsilon where step 4 shrank.
 * Deterministic (no float atomics, fixed summation order: equal inputs give equal bits), three launches, B * ceil(S / 8)
 * blocks each.  REDUCTION TREE of one sum of squares (the bounds of tests/adversarial_check.py count its depth): a sample
 * is cut into slabs of 8 token rows, one 256-thread block per slab;
 *     lane    sequential over its elements: slab rows w, w + 4 (w = wave of the block), per row the chunks lane,
 *             lane + 64, ... of 8 consecutive floats, element by element               <= 2 * ceil(H / 512) * 8 terms
 *     wave    four rotate-and-add steps inside rows of 16 lanes, then (l0 + l16) + (l32 + l48)          depth 6
 *     block   (w0 + w1) + (w2 + w3)                                                                     depth 2
 *     sample  lane l adds slab partials l and l + 64 (at most 128 slabs), then the wave tree again      depth 1 + 6
 * The per-slab partials live in `workspace` (icka_adv_workspace_floats(B, S, H) floats: 2 * B * ceil(S / 8)); each later
 * launch re-reduces them in that fixed order.  Limits: H % 8 == 0, H <= 2048, S <= 1024, B * S * H < 2^32
 * (ICKA_E_SHAPE beyond; icka_adv_workspace_floats returns 0).
 *
 * icka_adv_init_uniform, the uniform start of FreeLB: delta[b,t,h] = r * epsilon / sqrt(n_b * H) at valid positions (f32:
 * one division, one square root of the exact product, one product), 0 at all others; r in [-1, 1) is
 * (float)(hash >> 8) * 2^-23 - 1 with hash = icka_hash(s0, s1, flat element index (b S + t) H + h) of csrc/common.h (the
 * dropout hash) and (s0, s1) the low and high half of seed + counter.  counter_dev: nullable device uint64, added to
 * `seed` on the device.  icka_adv_bump: a one-thread node that advances the counter by 1 with an ordinary store; queued
 * after the init launch, every replay of a captured step draws a fresh start while equal (seed, counter) give equal bits. */
int icka_embed_fwd_adv(const int64_t* ids, const int64_t* token_type, const float* word, const float* pos,
                       const float* type, const float* gamma, const float* beta, const float* delta, void* y,
                       float* y_f32, void* xhat, float* rstd, int32_t B, int32_t S, int32_t H, int32_t vocab,
                       int32_t n_type, float eps, float p_drop, uint64_t seed, void* stream);
int icka_embed_fwd_adv_h(const int64_t* ids, const int64_t* token_type, const float* word, const float* pos,
                         const float* type, const float* gamma, const float* beta, const float* delta, void* y,
                         void* y_f16, void* xhat, float* rstd, int32_t B, int32_t S, int32_t H, int32_t vocab,
                         int32_t n_type, float eps, float p_drop, uint64_t seed, void* stream);
int64_t icka_adv_workspace_floats(int32_t B, int32_t S, int32_t H);
int icka_adv_ascend(float* delta, const float* grad, const int64_t* input_mask, float* norms, int32_t B, int32_t S,
                    int32_t H, float alpha, float epsilon, float* workspace, void* stream);
int icka_adv_init_uniform(float* delta, const int64_t* input_mask, int32_t B, int32_t S, int32_t H, float epsilon,
                          uint64_t seed, const uint64_t* counter_dev, void* stream);
int icka_adv_bump(uint64_t* counter_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Fused multi-head attention, head size 64 (bert-base 768/12, bert-large 1024/16).
 * BertSelfAttention.forward (:478-506) and BertCoAttention.forward (:590-624):
 *   scores = Q.K^T ; scores *= scale ; scores += add_mask[b, key] ; P = softmax ; P = dropout(P) ; O = P.V
 * Q/K/V/O are bf16 token-major matrices: element (b, s, head, e) at  ptr[(b*S + s)*ld + head*64 + e], so the
 * fused [M,3H] QKV projection output is consumed in place and O is written head-merged ([M,H], :503-505).
 * add_mask f32 [B,Skv] is the additive mask (1-mask)*-10000 (:364-372, :962-965).  lse f32 [B,heads,Sq] is saved
 * for the backward, which recomputes P instead of storing the [B,h,Sq,Skv] probabilities.
 */
int icka_attn_fwd(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                  const float* add_mask, void* O, int64_t ldo, float* lse, int32_t B, int32_t heads, int32_t Sq,
                  int32_t Skv, float scale, float p_drop, uint64_t seed, void* stream);
/* BASELINE config c5: the same forward with QK^T and PV on the fp8 matrix cores (OCP e4m3, fp32 accumulate; P is
 * scaled by 2^8 into e4m3's normal range, softmax statistics stay fp32).  Whole-head shapes only (Sq, Skv <= 128: the
 * text->image cross-attention); the backward is icka_attn_bwd (bf16 recomputation from the saved lse). */
int icka_attn_fwd_fp8(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                      const float* add_mask, void* O, int64_t ldo, float* lse, int32_t B, int32_t heads, int32_t Sq,
                      int32_t Skv, float scale, float p_drop, uint64_t seed, void* stream);
/* icka_attn_fwd / icka_attn_fwd_fp8 (fp8 != 0) with an additional fp16 copy O_f16 (may be NULL; same leading dimension
 * ldo) of the context: the "mixed16" mode feeds it to the out-proj GEMM as fp16 operand, O (bf16) stays the operand of
 * the bf16 weight-gradient GEMM and of icka_attn_bwd.
 * flags: ICKA_ATTN_FP8 = the fp8 QK^T / PV form (icka_attn_fwd_fp8); ICKA_ATTN_TILED = take the tiled flash-style kernels
 * also where the head would fit the whole-head kernels below (per call; the tests exercise both paths).
 * keep_bits (may be NULL; used when p_drop > 0): icka_attn_keepbits_words(B, heads, Sq, Skv) 32-bit words that receive the
 * keep decisions of the attention-probability dropout (nn.Dropout on the probabilities, :500 / :616) -- the same decisions
 * icka_attn_dropout_mask materialises -- so that icka_attn_bwd, given the same buffer, reads bits instead of hashing every
 * element again (about half of the backward's vector work).  Layout: per (batch*head, query, g = (key % 16) / 4)
 * ceil(Skv / 128) words, bit (key / 16) * 4 + key % 4.  Round 3: ABI version 4 added this parameter. */
int icka_attn_fwd_ex(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                     const float* add_mask, void* O, void* O_f16, int64_t ldo, float* lse, int32_t B, int32_t heads,
                     int32_t Sq, int32_t Skv, float scale, float p_drop, uint64_t seed, int32_t flags, void* keep_bits,
                     void* stream);
#define ICKA_ATTN_FP8 1
#define ICKA_ATTN_TILED 2
int64_t icka_attn_keepbits_words(int32_t B, int32_t heads, int32_t Sq, int32_t Skv);
/* Heads with Sq <= 128 and Skv <= 128 (the reference's max_seq_length 128 and 36/49 regions) take the whole-head
 * kernels: one block per (batch, head), forward without online-softmax rescaling, backward (dQ, dK, dV, delta) in
 * one launch (ICKA_ATTN_TILED in a call's flags takes the tiled kernels instead). */
/* delta f32 [B,heads,Sq] is workspace (rowsum(dO*O) = rowsum(P.dP)); it is written by the call.  keep_bits: NULL, or the
 * buffer the forward (icka_attn_fwd_ex) filled for the same shape, seed and replay nonce (whole-head kernels read it, the tiled
 * ones hash). */
int icka_attn_bwd(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                  const float* add_mask, const void* O, int64_t ldo, const void* dO, int64_t lddo, const float* lse,
                  float* delta, void* dQ, int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, int32_t B,
                  int32_t heads, int32_t Sq, int32_t Skv, float scale, float p_drop, uint64_t seed, const void* keep_bits,
                  int32_t flags, void* stream);
/* Attention maps (csrc/attn_probs.hip; additive, ABI version stays 6): the probabilities the fused kernels never materialise.
 * P = softmax(scale * Q.K^T + add_mask[b, key]) -- the probabilities BEFORE dropout (:492-497, :606-611).
 * Q / K: bf16 token-major as icka_attn_fwd (head size 64, element (b,s,head,e) at ptr[(b*S+s)*ld + head*64 + e]);
 * add_mask f32 [B,Skv].  P f32, contiguous: [B,heads,Sq,Skv], or with ICKA_ATTN_PROBS_HEAD_MEAN [B,Sq,Skv] = the mean
 * over heads, summed in head order 0..heads-1 inside the kernel (no atomics: the same bits on every run).
 * The sample's largest mask value is subtracted from its mask row before the add (softmax is invariant under the shift; f32 is
 * not: score - 10000 sits on a 2^-10 grid), so an all-masked sample gets the softmax of its unmasked scores at full precision.
 * Mask values are meant to be finite (the reference's 0 / -10000); a sample whose mask row is -inf for every key gets NaN, as
 * the reference's softmax gives.
 * One launch.  Any Sq >= 1, 1 <= Skv <= 512 (BERT's position limit; more is ICKA_E_SHAPE); unknown flags ICKA_E_ARG;
 * Q / K 16-byte aligned with ld % 8 == 0 and P 4-byte aligned, else ICKA_E_ALIGN.  Nothing is written past P's last element. */
int icka_attn_probs(const void* Q, int64_t ldq, const void* K, int64_t ldk, const float* add_mask, float* P,
                    int32_t B, int32_t heads, int32_t Sq, int32_t Skv, float scale, int32_t flags, void* stream);
#define ICKA_ATTN_PROBS_HEAD_MEAN 1

/* ---------------------------------------------------------------------------------------------------------------
 * Packed (padding-free) batches, csrc/packed.hip + the varlen instances of the whole-head attention kernels.  The valid
 * tokens of B samples occupy max_tokens rows: sample b the rows [cu_seqlens[b], cu_seqlens[b+1]); rows from cu_seqlens[B] on
 * are filler rows that belong to no sample.
 *
 * icka_pack_plan: ONE launch from input_mask (int64 [B,S], B <= 2048, S <= 1024; a prefix mask, pos < len, per sample) to
 *   lens [B] (int32, the prefix length of each mask), cu_seqlens [B+1] (int32), packed_to_padded [max_tokens] (b*S + s, -1
 *   for filler rows), padded_to_packed [B*S] (-1 for pads, -2 for a valid token that was not packed), cls_of [max_tokens]
 *   (b for the first row of sample b, else -1) and status (device int32[2] or NULL: total valid tokens, flags).  Samples
 *   from the first one whose rows would end past max_tokens are dropped (length 0 in cu_seqlens); flags bit 0 = overflow,
 *   bit 1 = a mask that is not a prefix mask.  On either, err_word (host-mapped uint32[2] or NULL) receives {tokens, flags}
 *   with a system-scope store; nothing clears it on the device.
 * icka_rows_gather: dst row r (r < dst_rows) = src row map[r * map_stride]; map entry -1 -> zeros, -2 -> every 32-bit word
 *   = fill (a NaN pattern marks dropped tokens), entries >= src_rows read as -1.  Rows are row_words 32-bit words (bf16:
 *   two elements a word; f32 logits: one); ld_* in words.  Packing, unpacking and both backwards are gathers through
 *   one of the two maps: every destination row is written exactly once, no atomics.
 * icka_attn_fwd_packed / icka_attn_bwd_packed: icka_attn_fwd_ex / icka_attn_bwd (bf16, whole-head, Sq <= 128 and Skv <= 128
 *   padded lengths) for packed queries: the rows of Q / O / dO / dQ are the packed rows; K / V / dK / dV are too when
 *   kv_packed (self-attention, Skv == Sq), else they stay at b*Skv + key (text -> image cross-attention).  cu_seqlens is read
 *   on the device (one graph capture serves any batch).  add_mask [B,Skv], lse / delta [B,heads,Sq], keep_bits and the
 *   dropout counters keep the PADDED coordinates, so every valid row equals the padded kernels' result bit for bit.
 *   Filler rows [cu_seqlens[B], Mrows) of O (forward) and of dQ (and dK / dV when kv_packed) are written as zeros; the
 *   backward zeroes dK / dV of the key rows of a sample with no packed query. */
int icka_pack_plan(const int64_t* mask, int32_t B, int32_t S, int32_t max_tokens, int32_t* lens, int32_t* cu_seqlens,
                   int32_t* packed_to_padded, int32_t* padded_to_packed, int32_t* cls_of, int32_t* status, void* err_word,
                   void* stream);
int icka_rows_gather(const void* src, int64_t ld_src, int64_t src_rows, void* dst, int64_t ld_dst, int64_t dst_rows,
                     int32_t row_words, const int32_t* map, int64_t map_stride, uint32_t fill, void* stream);
int icka_attn_fwd_packed(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                         const float* add_mask, void* O, int64_t ldo, float* lse, const int32_t* cu_seqlens, int32_t kv_packed,
                         int64_t Mrows, int32_t B, int32_t heads, int32_t Sq, int32_t Skv, float scale, float p_drop,
                         uint64_t seed, void* keep_bits, void* stream);
int icka_attn_bwd_packed(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                         const float* add_mask, const void* dO, int64_t lddo, const float* lse, float* delta, void* dQ,
                         int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, const int32_t* cu_seqlens,
                         int32_t kv_packed, int64_t Mrows, int32_t B, int32_t heads, int32_t Sq, int32_t Skv, float scale,
                         float p_drop, uint64_t seed, const void* keep_bits, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Element-wise / layout helpers.
 */
/* fp32 -> bf16 cast of a flat buffer (parameter shadow refresh); n elements. */
int icka_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int icka_cast_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream);
/* both 16-bit weight shadows from the f32 masters in one pass: bf16 (backward operands) and fp16 (saturating; the
 * forward operands of the "mixed16" mode).  16-byte aligned pointers. */
/* contiguous bf16 (src_is_f32 = 0) or f32 (1) -> fp16, saturating at +-65504 */
int icka_cast_to_f16(const void* src, int32_t src_is_f32, void* dst, int64_t n, void* stream);
int icka_cast_f32_to_bf16_f16(const float* src, void* dst_bf16, void* dst_f16, int64_t n, void* stream);
/* 2-D cast with zero padding: dst bf16 [M, ldd] ; dst[:, :N] = src f32 [M,N] (row stride lds), dst[:, N:ldd] = 0.
 * (logit gradients [M,C] -> a 16-byte-aligned bf16 GEMM operand.) */
int icka_cast_pad_f32_to_bf16(const float* src, int64_t lds, void* dst, int64_t ldd, int32_t M, int32_t N,
                              void* stream);
/* int64 0/1 mask [B, T] (row stride ld, first T columns used) -> additive f32 [B,T] = (1-m)*-10000  (:364-372). */
int icka_additive_mask(const int64_t* mask, int64_t ld, float* out, int32_t B, int32_t T, void* stream);
/* y = dropout(x) with the counter-hash mask; the same call with the same seed is its own backward (nn.Dropout,
 * Cross_Modal_Interaction_Module.py:953).  x,y bf16, row strides ldx/ldy; y2 optional second copy. */
int icka_dropout(const void* x, int64_t ldx, void* y, int64_t ldy, void* y2, int64_t ldy2, int32_t M, int32_t H,
                 float p_drop, uint64_t seed, void* stream);
/* Region features -> bf16 region tokens [B*R, C]:  layout 0: src f32 [B,R,C];  layout 1: src f32 [B,C,R]
 * (myResnet 'att' output [B,2048,7,7] viewed [B,2048,49] and permuted, :956). */
int icka_regions_to_tokens(const float* src, void* dst, int32_t B, int32_t R, int32_t C, int32_t layout,
                           void* stream);
/* "mixed16": the same with an fp16 twin of the tokens written in the same pass (dst_f16, same shape). */
int icka_regions_to_tokens_h(const float* src, void* dst_bf16, void* dst_f16, int32_t B, int32_t R, int32_t C, int32_t layout,
                             void* stream);
/* out[N] (+)= column sums of x[M,N] bf16 (bias gradients). */
int icka_colsum(const void* x, int64_t ldx, float* out, float* partials, int32_t M, int32_t N, int32_t accumulate,
                void* stream);
int64_t icka_colsum_workspace_floats(int32_t N);
/* Gate backward (cl_modeling.py:1363-1367): given dout = d(g*cross), g, cross:
 *   du = dout*cross*g*(1-g) ;  dcross = dout*g (+ dcross_in if not NULL).  All bf16 [M,H]. */
int icka_gate_bwd(const void* dout, int64_t lddout, const void* g, const void* cross, int64_t ldcross,
                  const void* dcross_in, int64_t lddci, void* du, void* dcross, int64_t lddc, int32_t M, int32_t H,
                  void* stream);
/* Classifier of the gated head, C <= 16 labels (cl_modeling.py:1371 `logits = self.classifier(cat(seq, Gate*cross))`),
 * as two HBM-bound kernels instead of 128x128-tile GEMMs on a 13-wide output:
 *   fwd: logits f32 [M,C] = [seq | gated] . W^T + bias      (seq, gated bf16 [M,H] contiguous; W bf16 [C,2H])
 *   bwd: dl bf16 [M, ldd >= C] -> dseq bf16 [M,H] (gradient w.r.t. seq through the classifier) and, for the gated
 *        half, the gate backward applied in place: du = dgated*cross*g*(1-g), dcross = dgated*g (as icka_gate_bwd);
 *        dW / db leave as icka_cls_head_bwd_slabs(M) slabs of icka_cls_head_slab_floats(H,C) floats each
 *        ([C*2H] weight part, then [16] bias part), to be summed by icka_gemm_grouped_ex slab reductions.
 * Needs 2H/8 <= 256 (H <= 1024), in the forward (both forms) as in the backward: anything else returns ICKA_E_SHAPE
 * and launches nothing. */
int icka_cls_head_fwd(const void* seq, const void* gated, const void* W, const float* bias, float* logits, int32_t M,
                      int32_t H, int32_t C, void* stream);
/* "mixed16" form of icka_cls_head_fwd: seq, gated and W are IEEE fp16 (the fp16 twins of the encoder outputs, the fp16
 * gate product of icka_gemm and the fp16 weight shadow). */
int icka_cls_head_fwd_h(const void* seq, const void* gated, const void* W, const float* bias, float* logits, int32_t M,
                        int32_t H, int32_t C, void* stream);
int icka_cls_head_bwd(const void* dl, int64_t ldd, const void* seq, const void* gated, const void* gate,
                      const void* cross, const void* W, void* dseq, void* du, void* dcross, float* partials, int32_t M,
                      int32_t H, int32_t C, void* stream);
int32_t icka_cls_head_bwd_slabs(int32_t M);
int64_t icka_cls_head_slab_floats(int32_t H, int32_t C);
/* Per-sample gates (fusion.hip).  a / c / out are token-major bf16 [B*S, H] with row strides.
 *  mode 0 (Cross_Modal_Interaction_Module.py:1029-1036): g_b = sigmoid(gate[b]);  out = g_b*a + (1-g_b)*c
 *  mode 1 (gate_cl_modeling.py:1369-1373): g_b = softmax(gate[b,0..1])[1];        out = g_b*a   (c = NULL)
 * Backward: da = g*dout, dc = (1-g)*dout (mode 0), and dgate (f32 [B] or [B,2], ZEROED BY THE CALLER) += its gradient. */
int icka_sample_gate_fwd(const void* a, int64_t lda, const void* c, int64_t ldc, const float* gate, int32_t mode,
                         void* out, int64_t ldo, int32_t B, int32_t S, int32_t H, void* stream);
/* "mixed16" forward of a per-sample gate without blend operand (mode 1 = gate_cl_modeling.py:1369-1373, cross = P * cross):
 * a16 fp16 [B*S, H] (row stride lda) -> out bf16 and out16 fp16 (row stride ldo), both rounded from the f32 product. */
int icka_sample_gate_fwd_h(const void* a16, int64_t lda, const float* gate, int32_t mode, void* out, void* out16, int64_t ldo,
                           int32_t B, int32_t S, int32_t H, void* stream);
int icka_sample_gate_bwd(const void* dout, int64_t lddo, const void* a, int64_t lda, const void* c, int64_t ldc,
                         const float* gate, int32_t mode, void* da, int64_t ldda, void* dc, int64_t lddc, float* dgate,
                         int32_t B, int32_t S, int32_t H, void* stream);
/* crs_classifier of gate_cl (gate_cl_modeling.py:1258,:1364-1366): crs[b,:] (f32 [B,2], ZEROED BY THE CALLER) +=
 * W[2, S*2H] . cat(seq,cross)[b].view(-1) + bias.  W bf16 (shadow), bias f32[2].  Backward: dseq / dcross (bf16
 * contiguous [B*S,H]) are the input gradients, dW f32 [2, S*2H] and dbias f32[2] follow `accumulate`. */
int icka_crs_fwd(const void* seq, int64_t lds, const void* cross, int64_t ldc, const void* W, const float* bias,
                 float* crs, int32_t B, int32_t S, int32_t H, void* stream);
int icka_crs_bwd(const float* dcrs, const void* seq, int64_t lds, const void* cross, int64_t ldc, const void* W,
                 void* dseq, void* dcross, float* dW, float* dbias, int32_t B, int32_t S, int32_t H,
                 int32_t accumulate, void* stream);
/* c = a + b (bf16, contiguous n elements; gradient fan-in). */
int icka_add_bf16(const void* a, const void* b, void* c, int64_t n, void* stream);
/* dz = dg * gelu'(z), contiguous bf16 (16-byte aligned): backward of BertIntermediate's erf-GELU (:548-551) when the
 * sub-module is called on its own; inside a layer it is the ICKA_EPI_DGELU epilogue. */
int icka_dgelu_bf16(const void* dg, const void* z, void* dz, int64_t n, void* stream);
/* dx = dy * (1 - y*y) (bf16, contiguous n elements): backward of the Tanh inside the prompt mapping networks
 * (Cross_Modal_Interaction_Module.py:914-928: Dropout, Linear, Tanh, Dropout, Linear). */
int icka_tanh_bwd(const void* dy, const void* y, void* dx, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Auxiliary training objective of the gated taggers (gate_cl_modeling.py:1276-1395, cl_modeling.py:1376-1382;
 * csrc/objective.hip).  Arithmetic in f32; fixed-order reductions, no atomics: two runs are bitwise equal.
 *
 * Contrastive (InfoNCE) loss of text rows t [B, D] against image rows v [B, D] (row strides ldt / ldv in elements;
 * dtype 0 = f32, 1 = bf16, 2 = fp16), 1 <= B <= 256, 8 <= D <= 4096, D % 8 == 0 (else ICKA_E_SHAPE):
 *   s_ij = cos(t_i, v_j) / temp (no epsilon in the norms, as the reference),
 *   stats[0] = (1/B) sum_i [temp_lamb (lse_j s_ij - s_ii) + (1 - temp_lamb)(lse_j s_ji - s_ii)].
 * With crs (f32 [B, 2], nullable) the relevance cross-entropy of gate_cl rides along:
 *   stats[1] = mean_b CE(crs_b, y_b), y_b = 0 for the last n_neg samples, 1 otherwise (0 when crs is null).
 * One launch (one workgroup).  ws: icka_contrastive_workspace_floats(B) floats, read by the backward. */
int64_t icka_contrastive_workspace_floats(int32_t B);
int icka_contrastive_fwd(const void* t, int64_t ldt, const void* v, int64_t ldv, int32_t dtype, int32_t B, int32_t D,
                         float temp, float temp_lamb, const float* crs, int32_t n_neg, float* stats, float* ws, void* stream);
/* Gradient: dt, dv contiguous f32 [B, D] (whatever the input dtype) from the upstream gradients dcl[0] (of stats[0]) and dcrs_loss[0] (of
 * stats[1]; read only with crs), both read from DEVICE memory (no host sync, capture-safe); dcrs f32 [B, 2] when crs is given.
 * One launch of 2B workgroups. */
int icka_contrastive_bwd(const void* t, int64_t ldt, const void* v, int64_t ldv, int32_t dtype, int32_t B, int32_t D,
                         float temp, float temp_lamb, const float* ws, const float* dcl, const float* dcrs_loss, void* dt,
                         void* dv, const float* crs, int32_t n_neg, float* dcrs, void* stream);
/* dx = dy * [y > 0] over n contiguous elements, bf16 (is_f32 = 0) or f32: backward of the ReLU between the two Linears of each
 * projection head (gate_cl_modeling.py:1387-1388).  dy == y == x gives the forward relu(x) of the fp32 mode. */
int icka_relu_bwd(const void* dy, const void* y, void* dx, int64_t n, int32_t is_f32, void* stream);
/* Negative-sample swap (gate_cl_modeling.py:1345-1356): y = x with samples b0 + i and b0 + h + i exchanged for i < h,
 * b0 = B - n_neg, h = n_neg / 2 (an odd last sample stays).  x, y: B samples of sample_bytes each (a multiple of 16,
 * 16-byte aligned, out of place).  The permutation is its own inverse: the backward is the same call on the gradient. */
int icka_sample_swap(const void* x, void* y, int32_t B, int64_t sample_bytes, int32_t n_neg, void* stream);
/* Token-level cross-entropy over valid tokens (benchmark loss), fused forward + backward:
 * logits f32 [M,C] (ld), labels/mask int64 [M]; loss_sum f32[1] += sum of -log p ; count f32[1] += #valid ;
 * dlogits bf16 [M, ldd] (ldd >= C, pad columns zeroed) = (softmax - onehot) * valid  (see icka_scale_by_ratio).
 * A row COUNTS ("valid") if and only if mask != 0 and 0 <= label < C, compared in 64 bits (a label of -100, C or
 * 2^32 + c does not count, as with CrossEntropyLoss(ignore_index=...)).  A row that does not count contributes nothing
 * to loss_sum / count and its gradient row is all zeros.  The same rule holds for icka_token_ce_fused and
 * icka_x_token_ce. */
int icka_token_ce(const float* logits, int64_t ld, const int64_t* labels, const int64_t* mask, float* loss_sum,
                  float* count, void* dlogits, int64_t ldd, int32_t M, int32_t C, void* stream);
/* y = x * num[0] / max(den[0], 1) for bf16 [n] with DEVICE scalars (NULL = 1): applies dloss / #valid to the
 * logit gradients without a host sync.  y may alias x. */
int icka_scale_by_ratio(const void* x, void* y, const float* num, const float* den, int64_t n, void* stream);
/* The same loss without pre-zeroed accumulators and without atomics (fixed summation order, bitwise reproducible):
 * stats f32[3] = {sum of token losses, number of valid tokens, mean loss}; dlogits [M, ldd] unscaled, bf16 or f32
 * (dl_is_f32: autograd wants the gradient of the f32 logits in f32); partials = f32 workspace of
 * icka_token_ce_workspace_floats(M).  Two launches (per-block partials, finalize).  Which rows count: as for
 * icka_token_ce (mask != 0 and 0 <= label < C in 64 bits; every other row has an all-zero gradient row). */
int64_t icka_token_ce_workspace_floats(int32_t M);
int icka_token_ce_fused(const float* logits, int64_t ld, const int64_t* labels, const int64_t* mask, float* stats,
                        float* partials, void* dlogits, int64_t ldd, int32_t dl_is_f32, int32_t M, int32_t C, void* stream);
/* p[0..n) = 0 (16-byte aligned p): clears the atomically accumulated embedding-table gradients. */
int icka_zero_f32(float* p, int64_t n, void* stream);
/* out[0] = num[0] / max(den[0], 1)   (mean loss from the two accumulators of icka_token_ce). */
int icka_scalar_ratio(float* out, const float* num, const float* den, void* stream);
/* ---------------------------------------------------------------------------------------------------------------
 * Linear-chain CRF over the per-token emissions.  The reference calls the third-party
 * `torchcrf.CRF(num_tags, batch_first=True)` (Cross_Modal_Interaction_Module.py:911, :1045-1057;
 * my_bert/cl_modeling.py:1269, :1380-1386); these entry points follow that package's algorithm (pytorch-crf 0.7.2).
 * emissions f32 [B,S,C] (row stride ld >= C), tags / mask int64 [B,S] (mask NULL = all on; step 0 is always on),
 * start/end f32 [C], trans f32 [C,C] (from, to).  C <= 64; one wave per sample.
 *   icka_crf_llh   : llh[b] = score(gold path) - log Z
 *   icka_crf_grad  : d_emissions[b,t,:] = gllh[b] * d llh / d e  (written), d_start / d_end / d_trans += (atomics)
 *   icka_crf_decode: Viterbi path per sample, best_tags [B,S] (-1 past sum(mask)), best_score [B] (nullable)
 * icka_crf_grad and icka_crf_decode keep S*C values per sample in LDS: S*C <= 12288 (else ICKA_E_SHAPE, nothing written).
 * Masks with holes follow the package rule by rule: the recursions advance at position 0 and where mask != 0 (the ON
 * positions); the gold path takes the transition into an on position t from the label at the LITERAL previous position
 * t - 1, and its end transition from the label at INDEX sum(mask[b]) - 1; back-pointers are recorded at every step and the
 * path is read back from index sum(mask[b]) - 1.
 * mask[b,0] == 0 (the package rejects it): position 0 still takes part in every recursion, but sum(mask[b]) does not count
 * it, so the end transition is read one position earlier and the decoded path is one tag shorter than there are on
 * positions: sum(mask[b]) tags, for every C.  A row whose mask is all zero decodes ONE tag and reads its end transition at
 * position 0.
 * Labels are clamped into [0, C-1] wherever they are read, so positions that are off may carry pad labels such as -100: a
 * label that no rule above reads changes nothing, one that is read counts as the clamped value.
 * d_emissions holds exact +0.0 in all C columns of every off position (every row of the sample is written; the ldd - C pad
 * columns are not touched). */
int icka_crf_llh(const float* emissions, int64_t ld, const int64_t* tags, const int64_t* mask, const float* start,
                 const float* end, const float* trans, float* llh, int32_t B, int32_t S, int32_t C, void* stream);
int icka_crf_grad(const float* emissions, int64_t ld, const int64_t* tags, const int64_t* mask, const float* start,
                  const float* end, const float* trans, const float* gllh, float* d_emissions, int64_t ldd,
                  float* d_start, float* d_end, float* d_trans, int32_t B, int32_t S, int32_t C, void* stream);
int icka_crf_decode(const float* emissions, int64_t ld, const int64_t* mask, const float* start, const float* end,
                    const float* trans, int64_t* best_tags, float* best_score, int32_t B, int32_t S, int32_t C,
                    void* stream);
/* Score and decode in one launch, with no host sync (graph-capturable decoding).  lens int32 [B]: the length of each
 * sample's Viterbi path (the entries icka_crf_decode writes before its -1 filler: sum(mask[b]), at least 1).
 * tags_flat int32 [capacity >= B*S]: the paths of all samples back to back, sample b at sum(lens[0 .. b-1]) (the kernel
 * computes the offset itself; entries past sum(lens) are left as they are).  Tags equal icka_crf_decode's.  tags and llh
 * are both NULL or both set: llh f32 [B] is then the gold-path log-likelihood, bit for bit icka_crf_llh's.
 * S*C <= 12288, B <= 2048. */
int icka_crf_score_decode(const float* emissions, int64_t ld, const int64_t* tags, const int64_t* mask,
                          const float* start, const float* end, const float* trans, float* llh, int32_t* lens,
                          int32_t* tags_flat, int64_t capacity, int32_t B, int32_t S, int32_t C, void* stream);
/* CRF posteriors (csrc/crf_posterior.hip): how sure the model is of a tag path.  One launch, one wave per sample, no host
 * sync.  Per sample the ON-POSITIONS are position 0 and every t >= 1 with mask[b,t] != 0 (mask NULL = all on), L their
 * number, x_0 .. x_{L-1} the emission rows at them.  The model is the chain over the on-positions,
 *   score(y) = start[y_0] + x_0[y_0] + sum_{i >= 1} (trans[y_{i-1}, y_i] + x_i[y_i]) + end[y_{L-1}],  Z = sum_y exp score(y).
 * A PATH is L tag ids; the paths come as icka_crf_score_decode writes them: lens int32 [B], tags_flat int32 [capacity], path
 * b at off_b = sum(lens[0 .. b-1]) (summed inside the kernel).  lens and tags_flat may both be NULL: then only log_z and
 * marginals are written (seq_logp, token_conf and the chunk arguments are ignored).  Outputs, f32 unless noted:
 *   log_z [B]          log Z
 *   seq_logp [B]       score(path) - log Z  (<= 0)
 *   token_conf         [capacity], aligned with tags_flat: P(y_i = path_i | x) at off_b + i
 *   marginals          [B,S,C] contiguous, nullable: P(y_t = j | x) at on-positions, exact 0 at off-positions; every element
 *                      of the sample is written
 *   ent int32 [capacity,3], ent_conf [capacity], n_ent int32 [B]   only with label_table (else ignored): the chunks of the
 *                      path by the rules of icka_chunk_eval below on the label_table words of its tags (nothing is skipped:
 *                      bit 2 is not read; an id >= L_ids counts as the default tag), in PATH coordinates: chunk k of sample b
 *                      at row off_b + k = (type id, start, end) with end exclusive, n_ent[b] chunks (at most lens[b], so every
 *                      sample stays inside its own segment).  ent_conf = the exact posterior that the tags at path positions
 *                      start .. end-1 equal the path's: alpha_s[y_s] prod_{i=s+1}^{e-1} psi_i(y_{i-1}, y_i) beta_{e-1}[y_{e-1}] / Z
 *                      (psi_i(u, v) = exp(trans[u,v] + x_i[v])); a chunk of one token has its token_conf, bit for bit.
 *                      Rows k >= n_ent[b] of a segment and everything past sum(lens) are not written.
 *   bad int32 [1]      += the number of REFUSED samples (the caller zeroes it): lens[b] != L, a segment outside
 *                      [0, capacity), or a tag id outside [0, C).  A refused sample gets NaN in log_z, seq_logp, its
 *                      token_conf segment and its marginals, and n_ent[b] = 0; no load or store is indexed by an unchecked
 *                      id; the other samples are unaffected.
 * Limits (else ICKA_E_SHAPE, nothing launched): C <= 64, S*C <= 12288, B <= 2048; with label_table S <= 512 and
 * 1 <= L_ids <= 64.  C <= 16 with S <= 512 runs the scaled linear-domain recursions in registers (samples whose
 * normalisers leave the f32 range, or with L*C > 4096, are redone in the log domain), otherwise the log-domain form. */
int icka_crf_posterior(const float* emissions, int64_t ld, const int64_t* mask, const float* start, const float* end,
                       const float* trans, const int32_t* lens, const int32_t* tags_flat, int64_t capacity,
                       const int32_t* label_table, int32_t L_ids, float* log_z, float* seq_logp, float* token_conf,
                       float* marginals, int32_t* ent, float* ent_conf, int32_t* n_ent, int32_t* bad, int32_t B,
                       int32_t S, int32_t C, void* stream);
/* N-best decoding (csrc/crf_nbest.hip): the nbest = K best tag paths of every sample.  One launch, one wave per sample, no
 * host sync.  The chain is icka_crf_posterior's: per sample the ON-POSITIONS are position 0 and every t >= 1 with
 * mask[b,t] != 0 (mask NULL = all on), L their number, x_0 .. x_{L-1} the emission rows at them, and
 *   score(y) = start[y_0] + x_0[y_0] + sum_{i >= 1} (trans[y_{i-1}, y_i] + x_i[y_i]) + end[y_{L-1}].
 * Sample b has n_paths[b] = min(K, C^L) results (the minimum is taken stepwise: C^L overflows): the n_paths[b] DISTINCT
 * paths of highest score, by non-increasing score.  TIE RULE: among paths of equal score the one whose REVERSED tag sequence
 * (y_{L-1}, y_{L-2}, .., y_0) is lexicographically smaller comes first.  The recurrence gives exactly this order: at every
 * position and tag equal-scoring candidates are kept in ascending (previous tag, previous rank), and the final selection
 * prefers ascending (tag, rank).  Rank 0 therefore is the path of icka_crf_score_decode (which takes the first maximum at
 * both places) whenever mask[b,0] != 0 or mask is NULL.  Emissions and parameters are assumed finite; on non-finite input
 * the paths mean nothing, but every stored tag is in [0, C) and nothing outside the sample's own segments is touched.
 * Scores are summed in f32 from left to right: ((start + x_0) + trans) + x_1 .. + end.  Outputs:
 *   lens int32 [B]           L, the length of every rank's path of the sample
 *   n_paths int32 [B]
 *   scores f32 [B, K]        score of rank r; -inf at ranks >= n_paths[b]
 *   tags_flat int32 [K, capacity], capacity >= B*S: row r holds rank r of all samples in the layout of
 *                            icka_crf_score_decode (sample b at sum(lens[0 .. b-1]), summed inside the kernel), so
 *                            (lens, row r) goes to icka_crf_posterior and icka_chunk_eval as it is; -1 at the ranks
 *                            >= n_paths[b]; entries past sum(lens) of every row are left as they are.
 * Limits (else ICKA_E_SHAPE, nothing launched): 1 <= C <= 16, 1 <= K <= 8, S <= 512, B <= 2048 and S*C*K <= 49152 (one byte
 * of back-pointer per (position, tag, rank): previous tag * 8 + previous rank).  A sample the kernel could not serve would
 * come out as n_paths = 0 with -inf scores and -1 tags; the limits above leave no such sample. */
int icka_crf_nbest(const float* emissions, int64_t ld, const int64_t* mask, const float* start, const float* end,
                   const float* trans, int32_t nbest, int32_t* lens, int32_t* n_paths, float* scores, int32_t* tags_flat,
                   int64_t capacity, int32_t B, int32_t S, int32_t C, void* stream);
/* Sampling (csrc/crf_sample.hip): num_samples = K independent EXACT draws from p(y | x) = exp(score(y) - log Z) of every
 * sample, by forward filtering and backward sampling.  One launch, one wave per sample, no host sync, capturable.  The chain
 * is icka_crf_posterior's: per sample the ON-POSITIONS p_0 < .. < p_{L-1} are position 0 and every t >= 1 with
 * mask[b,t] != 0 (mask NULL = all on), L their number, x_0 .. x_{L-1} the emission rows at them, and
 *   score(y) = start[y_0] + x_0[y_0] + sum_{i >= 1} (trans[y_{i-1}, y_i] + x_i[y_i]) + end[y_{L-1}].
 * FORWARD PASS, f32, always in the LOG domain (for every C and S: there is no scaled linear form and no fallback here), the
 * arithmetic of icka_crf_posterior's log-domain form RE-CENTRED at every position, because a draw needs alpha_i only up to a
 * constant per position and centred values keep their f32 digits on long chains:
 *   a_0 = start + x_0,  a_i(v) = (m + log sum_u exp((alpha_{i-1}(u) + trans[u,v]) - m)) + x_i[v],  m the maximum of the
 *   exponent over u;  kappa_i = max_v a_i(v),  alpha_i = a_i - kappa_i (what stays in LDS for every on-position: the true
 *   forward score minus kappa_0 + .. + kappa_i);
 *   log_z[b] = (kappa_0 + .. + kappa_{L-1}, summed in this order) + (m + log sum_j exp((alpha_{L-1}(j) + end[j]) - m)).
 * DRAW k (k = 0 .. K-1), one tag per on-position, from the last to the first:
 *   y_{L-1} from the weights w_j = exp((alpha_{L-1}(j) + end[j]) - m); then for i = L-1 .. 1
 *   y_{i-1} from the weights w_u = exp((alpha_{i-1}(u) + trans[u, y_i]) - m);  m = the maximum of the exponent over the tags.
 *   One draw is an inverse CDF in TAG ORDER: cum_j = w_0 + .. + w_j summed sequentially in f32, W = cum_{C-1}; the drawn tag
 *   is the smallest j with cum_j > r * W (the product in f32).  If rounding leaves none it is the last j with w_j > 0.  A tag
 *   whose f32 weight is exactly 0 is therefore never drawn: a transition or start of -1e4 works as a hard constraint here too.
 * UNIFORMS: the tag at on-position p_i of draw k of sample b uses r = (h >> 8) * 2^-24 with h = the counter hash of
 *   common.h (icka_hash) of (s0, s1, idx), idx = (b * K + k) * S + p_i in 32-bit arithmetic, s0 / s1 the low / high half of
 *   the by-value seed, each XORed with seed_dev[0] / seed_dev[1] when the nullable DEVICE pointer seed_dev is given.  No
 *   process-wide state takes part (the dropout nonce is not read): equal arguments give bitwise equal outputs, and a captured
 *   graph draws fresh paths on every replay when a node of the graph changes the caller's seed_dev words.
 * Outputs:
 *   lens int32 [B]           L
 *   log_z f32 [B]
 *   scores f32 [B, K]        score of draw k, summed in f32 from left to right as in icka_crf_nbest:
 *                            ((start + x_0) + trans) + x_1 .. + end; scores - log_z is the draw's log-probability
 *   tags_flat int32 [K, capacity], capacity >= B*S: row k holds draw k of all samples in the layout of icka_crf_nbest
 *                            (sample b at sum(lens[0 .. b-1]), summed inside the kernel), so (lens, row k) goes to
 *                            icka_crf_posterior, icka_chunk_eval and icka_chunk_counts as it is; entries past sum(lens) of
 *                            every row are left as they are.
 * Limits (else ICKA_E_SHAPE, nothing launched, nothing written): 1 <= C <= 64, S*C <= 12288, 1 <= K <= 64, B <= 2048.
 * C <= 16 draws four paths per pass on the four 16-lane rows of the wave, larger C one path per pass: the same arithmetic.
 * Emissions and parameters are assumed finite; on non-finite input the paths mean nothing, but every stored tag is in
 * [0, C) and nothing outside the sample's own segments is touched.
 * Not covered: sampling under allowed sets; packed batches. */
int icka_crf_sample(const float* emissions, int64_t ld, const int64_t* mask, const float* start, const float* end,
                    const float* trans, int32_t num_samples, uint64_t seed, const uint32_t* seed_dev, int32_t* lens,
                    float* log_z, float* scores, int32_t* tags_flat, int64_t capacity, int32_t B, int32_t S, int32_t C,
                    void* stream);
/* The constrained CRF (csrc/crf_constrained.hip): every on-position carries a SET of allowed tags.  Training on partially
 * labelled data maximises the marginal likelihood of all paths inside the sets; decoding returns the best path inside them.
 * One launch per entry, one wave per sample, no host sync.  The chain is icka_crf_posterior's: per sample the ON-POSITIONS
 * are position 0 and every t >= 1 with mask[b,t] != 0 (mask NULL = all on), L their number, x_0 .. x_{L-1} the emission rows
 * at them, and
 *   score(y) = start[y_0] + x_0[y_0] + sum_{i >= 1} (trans[y_{i-1}, y_i] + x_i[y_i]) + end[y_{L-1}].
 * allowed int64 [B,S] in the layout of the mask: each entry is a bit set, bit j set = tag j allowed at that position.  Only
 * on-positions are read; bits at or above C are ignored; C = 64 uses the sign bit, -1 means "every tag".  A_i is the set at
 * on-position i,
 *   Z_A = sum_{y : y_i in A_i for all i} exp score(y),   Z = sum_y exp score(y).
 * icka_crf_constrained_llh:   llh[b] = log Z_A - log Z (<= 0), log_za[b] = log Z_A, log_z[b] = log Z, all f32 [B].
 * icka_crf_constrained_grad:  gllh[b] * d llh[b] / d(.) with
 *   d llh / d x_i[j] = mu^A_i(j) - mu_i(j), the difference of the restricted and the free token marginals; for start the
 *   difference at i = 0, for end at i = L-1, for trans[u,v] the difference of the pair marginals summed over i >= 1.
 *   d_emissions [B,S,C] (row stride ldd) is WRITTEN: every row of the sample, exact +0.0 in all C columns of an off-position
 *   (the ldd - C pad columns are not touched).  d_start, d_end, d_trans are ACCUMULATED (+=) with atomics over the samples,
 *   the contract of icka_crf_grad.
 * INFEASIBLE samples: some on-position has no allowed tag below C (Z_A = 0).  llh and log_za are -inf, log_z is still
 *   written; all d_emissions rows are exact zeros and the sample adds nothing to the parameter gradients; the llh and the
 *   decode entry add 1 to infeasible (int32 [1], nullable; the caller zeroes it).  The other samples are unaffected and no
 *   NaN appears anywhere: the restricted recursions do not run on such a sample.
 * icka_crf_constrained_decode: argmax_{y in A} score(y) in the flat layout of icka_crf_score_decode: lens int32 [B] with
 *   lens[b] = L, tags_flat int32 [capacity >= B*S] with sample b at sum(lens[0 .. b-1]) (summed inside the kernel; entries
 *   past sum(lens) are left as they are), and scores f32 [B], summed in f32 from left to right as in icka_crf_nbest:
 *   ((start + x_0) + trans) + x_1 .. + end.  TIE RULE: the first maximum over the allowed tags at both places (the previous
 *   tag of every step and the final tag); with every tag allowed the path is icka_crf_score_decode's whenever mask[b,0] != 0
 *   or mask is NULL.  An infeasible sample writes -1 into its L slots, gets scores[b] = -inf and is counted in infeasible.
 * Emissions and parameters are assumed finite.  On non-finite input every stored tag is still in [0, C) or -1 and nothing
 * outside the sample's own segment is touched.
 * Limits (else ICKA_E_SHAPE, nothing launched): C <= 64, S*C <= 12288; for the decode entry B <= 2048.  Log-domain f32
 * recursions, the free and the restricted lattice one after the other in the same wave: for C <= 16 with the scores on the
 * lanes and the transitions in registers, otherwise through LDS (the same arithmetic in another summation order: neither
 * form has a range the other lacks, so there is no fallback between them).
 * Not covered: posteriors, N-best and entity confidences under constraints; transition-level constraints (write -1e4 into
 * trans); packed batches. */
int icka_crf_constrained_llh(const float* emissions, int64_t ld, const int64_t* mask, const int64_t* allowed,
                             const float* start, const float* end, const float* trans, float* llh, float* log_z,
                             float* log_za, int32_t* infeasible, int32_t B, int32_t S, int32_t C, void* stream);
int icka_crf_constrained_grad(const float* emissions, int64_t ld, const int64_t* mask, const int64_t* allowed,
                              const float* start, const float* end, const float* trans, const float* gllh,
                              float* d_emissions, int64_t ldd, float* d_start, float* d_end, float* d_trans, int32_t B,
                              int32_t S, int32_t C, void* stream);
int icka_crf_constrained_decode(const float* emissions, int64_t ld, const int64_t* mask, const int64_t* allowed,
                                const float* start, const float* end, const float* trans, int32_t* lens, int32_t* tags_flat,
                                int64_t capacity, float* scores, int32_t* infeasible, int32_t B, int32_t S, int32_t C,
                                void* stream);
/* CRF expectations (csrc/crf_expect.hip): log Z and the expectation of a path-additive payoff under the CRF distribution,
 * with gradients.  Sequence entropy, the KL divergence between two CRFs over one sentence and an expected cost reduce to it.
 * One launch per entry, one wave per sample, no host sync.  The chain is icka_crf_posterior's: per sample the ON-POSITIONS are
 * position 0 and every t >= 1 with mask[b,t] != 0 (mask NULL = all on), i = 0 .. L-1.
 * A LATTICE is (e [B,S,C] with a row stride, start [C], end [C], trans [C,C]); x_i is its e row at on-position i, its path
 * score
 *   s(y) = start[y_0] + sum_i x_i[y_i] + sum_{i >= 1} trans[y_{i-1}, y_i] + end[y_{L-1}],
 * and p(y) = exp(s_p(y) - log Z_p) for the first lattice (emissions, start, end, trans).  The PAYOFF r(y) comes from a SECOND
 * lattice (second, second_start, second_end, second_trans): every one of its four parts is nullable, a NULL part is zeros.
 *   relative == 0 (given):    r = s_second
 *   relative == 1 (relative): r = s_p - s_second, formed operand by operand as the values are loaded (never as the difference
 *                             of two accumulated sums)
 * icka_crf_expect:  log_z[b] = log Z_p and expect[b] = E_p[r(y)], f32 [B].  expect may be NULL: then only log_z is computed.
 *   H(p) = log_z - expect (relative, no second lattice);  KL(p || q) = expect - log_z_p + log_z_q (relative, q the second
 *   lattice, log_z_q from one more call on q with expect NULL);  an expected cost is expect in given mode with
 *   second[b,t,j] = cost[tags[b,t], j] and the three other parts NULL.
 * icka_crf_expect_grad:  upstream g_logz, g_expect f32 [B], each nullable (NULL = zeros).  With mu_i(j) and xi_i(k,j) the token
 *   and pair marginals of p, for the first lattice's features f (emission cells, start at i = 0, end at i = L-1, transition
 *   cells summed over i >= 1)
 *     g_logz E_p[f] + g_expect (Cov_p(f, r) + [relative] E_p[f]),
 *   and for the second lattice's features g_expect (+- E_p[f]): + given, - relative.  The contract of icka_crf_grad:
 *   d_emissions and d_second [B,S,C] (row strides ldd, ldd2) are WRITTEN, every row of the sample, exact +0.0 in all C columns of
 *   an off-position (pad columns are not touched); the three parameter gradients of each lattice are ACCUMULATED (+=) with
 *   atomics over the samples.  Each of the eight outputs is nullable: NULL = not wanted.  The covariance is computed only
 *   when g_expect and at least one of the first lattice's four outputs are given (a detached first lattice costs one plain
 *   forward-backward).
 *   Cov_p(1[y_i = j], r) = mu_i(j) (a_i(j) + b_i(j) - E_p[r]) with a_i(j) the expected payoff of the prefix through node i given
 *   y_i = j and b_i(j) that of the suffix after it (expectation semiring); the transition cells use xi_i(k,j) (a_{i-1}(k) +
 *   r_trans(k,j) + r_i(j) + b_i(j) - E_p[r]).  a + b and E_p[r] are both of size L |r|, so the kernel carries a and b minus a
 *   wave-uniform offset per position and subtracts the mu- (xi-) weighted mean instead, which is exact: nothing of that size
 *   is ever subtracted in f32.
 * Limits (else ICKA_E_SHAPE, nothing launched, nothing written): C <= 64 and S*C <= 4096 (alpha and the centred a of every
 * on-position in LDS); any B >= 1.  relative outside {0, 1}, a missing first-lattice operand or a row stride below C:
 * ICKA_E_ARG.  Log-domain f32 recursions: for C <= 16 with the scores on the lanes and the tables in registers, otherwise
 * through LDS (the same arithmetic in another summation order).  Scores are assumed finite: -inf is NOT supported (forbid a transition with -1e4,
 * which gives finite results: its probabilities underflow to exact zeros).
 * Not covered: constraints (allowed sets), packed batches. */
int icka_crf_expect(const float* emissions, int64_t ld, const int64_t* mask, const float* start, const float* end,
                    const float* trans, const float* second, int64_t ld2, const float* second_start,
                    const float* second_end, const float* second_trans, int32_t relative, float* log_z, float* expect,
                    int32_t B, int32_t S, int32_t C, void* stream);
int icka_crf_expect_grad(const float* emissions, int64_t ld, const int64_t* mask, const float* start, const float* end,
                         const float* trans, const float* second, int64_t ld2, const float* second_start,
                         const float* second_end, const float* second_trans, int32_t relative, const float* g_logz,
                         const float* g_expect, float* d_emissions, int64_t ldd, float* d_start, float* d_end,
                         float* d_trans, float* d_second, int64_t ldd2, float* d_second_start, float* d_second_end,
                         float* d_second_trans, int32_t B, int32_t S, int32_t C, void* stream);
/* ---------------------------------------------------------------------------------------------------------------
 * Chunk-level scoring of a dev / test batch (csrc/metrics.hip): the counts behind the reference's accuracy / precision /
 * recall / F1, overall and per entity type -- the per-token loop of My_cross_attention.py:882-903 followed by
 * ner_evaluate.py:4-148 (get_chunks, evaluate, evaluate_each_class).  One launch ADDS the batch's counts into
 *   counters int64 [6 + 3 * ntypes] = kept_tokens, equal_tokens, correct_preds, total_preds, total_correct, bad_ids,
 *                                     then (correct, preds, golds) per type id
 * with 64-bit atomic adds (integer sums: independent of the order, a graph replay equals an eager call).  No host sync.
 * Predictions in ONE of two forms: lens int32 [B] + tags_flat int32 [capacity], the paths back to back as
 * icka_crf_score_decode writes them (path b starts at sum(lens[0 .. b-1]), summed inside the kernel; pred NULL), or
 * pred int64 [B,S] with row stride ld_pred >= S (lens and tags_flat NULL).  labels, output_mask int64 [B,S] contiguous
 * (mask: zero / non-zero).  label_table int32 [L], one word per tag id: bit 0 = the default tag ("O"), bit 1 = class "B"
 * (name.split('-')[0] == "B"), bit 2 = skipped when it is the GOLD label (the reference's X, </s>, <s>, [CLS], [SEP]),
 * bits 8.. = type id < ntypes (name.split('-')[-1]).  1 <= S <= 512, L <= 64, ntypes <= 32, any B >= 1.
 * Per sample: the kept positions are j < n0 (n0 = index of the first zero of output_mask[b]) whose gold label has no
 * skip bit, compacted in order; the prediction at j is path_b[j] / pred[b,j].  On the compacted gold and predicted
 * sequences separately, O(i) = default tag, t(i) = type id: start(i) = !O(i) && (i == 0 || O(i-1) || t(i) != t(i-1) ||
 * B(i)), term(i) = O(i) || start(i); a chunk begins at every start, has that token's type and ends at the next term
 * (or the end).  total_preds / total_correct += predicted / gold starts (per type too); correct_preds += positions
 * where both start with one type and both chunks end at the same index (per type: under that type); kept_tokens +=
 * kept positions, equal_tokens += those with pred == gold.  A sample whose path is shorter than n0, or with a gold id
 * at j < n0 or a predicted id at a kept position outside [0, L) (never used as an index), adds 1 to bad_ids and
 * nothing else. */
int icka_chunk_eval(const int32_t* lens, const int32_t* tags_flat, int64_t capacity, const int64_t* pred, int64_t ld_pred,
                    const int64_t* labels, const int64_t* output_mask, const int32_t* label_table, int64_t* counters,
                    int32_t B, int32_t S, int32_t L, int32_t ntypes, void* stream);
/* Per-path, per-sample chunk counts (csrc/chunk_counts.hip): what turns the rows of icka_crf_nbest or icka_crf_sample into a
 * per-candidate F1 cost.  One launch, one wave per (sample, row), no atomics, no host sync.  lens int32 [B] and tags_flat
 * int32 [R, capacity] with row stride ld_tags >= capacity: row r holds one path per sample back to back (path b at
 * sum(lens[0 .. b-1]), summed inside the kernel).  labels, output_mask, label_table, L and ntypes are icka_chunk_eval's.
 *   counts int32 [R, B, 4] = (correct_preds, total_preds, total_correct, bad), WRITTEN, not accumulated.
 * The kept positions, the skip bit, start / term and the chunks are those of icka_chunk_eval, rule for rule, applied to
 * (lens, row r): for every r the sums over b of the first three columns are what icka_chunk_eval adds to correct_preds,
 * total_preds, total_correct for that row, and the sum of the fourth is what it adds to bad_ids.  A bad sample -- a path
 * shorter than n0, a segment outside [0, capacity), a gold id at j < n0 or a path id at a kept position outside [0, L),
 * such as the -1 of a rank an N-best sample does not have -- gets (0, 0, 0, 1); no id is used as an index unchecked.
 * Limits (else ICKA_E_SHAPE, nothing launched): 1 <= S <= 512, L <= 64, ntypes <= 32, 1 <= R <= 64, 1 <= B <= 2048.
 * Not covered: per-type counts. */
int icka_chunk_counts(const int32_t* lens, const int32_t* tags_flat, int64_t capacity, int64_t ld_tags, int32_t R,
                      const int64_t* labels, const int64_t* output_mask, const int32_t* label_table, int32_t* counts,
                      int32_t B, int32_t S, int32_t L, int32_t ntypes, void* stream);
/* acc[0] += (double)loss[0], acc[1] += 1 (one launch, stream-ordered): the dev loop's `dev_total_loss += loss.item();
 * index += 1` (My_cross_attention.py:877-878) without the host sync.  loss f32 [1], acc f64 [2]. */
int icka_loss_accumulate(const float* loss, double* acc, void* stream);
/* ---------------------------------------------------------------------------------------------------------------
 * Bidirectional single-layer LSTM of the tagging tail:
 * nn.LSTM(H, H, batch_first=True, bidirectional=True) at Cross_Modal_Interaction_Module.py:905-908, called :1042
 * (`x, _ = self.lstm(result)`).  Gate order i, f, g, o as torch.nn.LSTM.  The input projection (x . W_ih^T + b_ih +
 * b_hh for both directions, f32 [B*S, 8H], column = dir*4H + gate*H + unit) is an icka_gemm; these entry points run
 * the recurrence, one launch per time step (both directions per launch), B <= 64, H % 32 == 0.
 *   icka_lstm_fwd: w_hh bf16 [2][4H][H]; writes y bf16 [B,S,2H] (h_t, the LSTM output), c_all f32 [B,S,2,H],
 *                  act bf16 [B,S,2,4H] (gate activations) and optionally hprev bf16 [B,S,2H] (h_{t-1} per step: the
 *                  operand of the dW_hh GEMM).
 *   icka_lstm_bwd: dy bf16 [B,S,2H], w_hh_t = W_hh^T bf16 [2][H][4H] (icka_transpose_bf16); writes the gate
 *                  pre-activation gradients dgates bf16 [B*S, ldg >= 8H]; dW_ih, dW_hh, db and dx are GEMMs / column
 *                  sums over dgates afterwards.  dc_carry f32 [2,B,H] is workspace. */
int icka_lstm_fwd(const float* gates_x, int64_t ldg, const void* w_hh, void* y, float* c_all, void* act, void* hprev,
                  int32_t B, int32_t S, int32_t H, int32_t flags, void* stream);
int icka_lstm_bwd(const void* dy, const void* w_hh_t, const void* act, const float* c_all, void* dgates, int64_t ldg,
                  float* dc_carry, int32_t B, int32_t S, int32_t H, int32_t flags, void* stream);
/* flags of icka_lstm_fwd / icka_lstm_bwd (0 = the defaults; per call, no process-wide switch):
 *   default            for B <= 32 and H <= 1024 (and a grid of H/16 x 2 blocks that fits the device's CUs) the recurrence is ONE
 *                      persistent launch per direction pair -- W_hh slices and cell state resident in registers; the blocks hand
 *                      h_t over as flag-in-data 8-byte words polled by the consumers (forward: H % 256 == 0; backward: H % 256 ==
 *                      0 and one block per batch tile resident; other shapes use the ticket form): forward broadcasts h_t,
 *                      backward reduce-scatters bf16 partial products of dgates_t . W_hh; in the forward a batch of 17..32 rows
 *                      runs as two independent tiles of 16 rows (separate blocks) where all of them are co-resident.  Larger B
 *                      or H take one launch per time step.
 *   ICKA_LSTM_PER_STEP        one launch per time step instead of the persistent launch.
 *   ICKA_LSTM_TICKETS         persistent launch with step tickets + L1 invalidate instead of tagged words.  Forward results
 *                             agree with the tagged-word form to f32 summation order (one MFMA chain per gate here, four
 *                             per-wave partial sums there): c_all differs in its last bits and a few y / act elements by one
 *                             bf16 ulp -- not bitwise equal; backward gradients agree to bf16 rounding (the tagged-word form
 *                             rounds its partial products to bf16).  tests/test_lstm_steps_gpu.py holds both to the same
 *                             per-step bounds.
 *   ICKA_LSTM_NO_BATCH_SPLIT  one block per 16 hidden units holds all rows (bitwise the same results: a row's arithmetic does
 *                             not depend on its tile).
 * icka_lstm_barrier_error() returns 1 if a hand-off wait ever gave up (bounded spin: the kernel then finishes with NaN-poisoned
 * data instead of hanging), -1 if the query itself failed. */
#define ICKA_LSTM_PER_STEP 1
#define ICKA_LSTM_TICKETS 2
#define ICKA_LSTM_NO_BATCH_SPLIT 4
/* Variable lengths (pack_padded_sequence semantics; a departure from the reference, whose nn.LSTM call runs over the padding).
 * The *_varlen entries are icka_lstm_fwd / icka_lstm_bwd plus ``lens``: int32 [B] ON THE DEVICE, read by the kernels (each
 * reads its rows' lengths once, at its start, clamped to [0, S]); no host value derived from the lengths enters a launch, so
 * one captured graph serves every batch.  lens == NULL is icka_lstm_fwd / icka_lstm_bwd exactly (which forward here).
 *   Semantics.  Positions t >= lens[b] are pads.  The state of both directions is zero where a row's live part begins (the
 *   reverse direction starts at lens[b] - 1), and y, c_all and dgates are EXACTLY zero at every pad: the weight / input gradient
 *   GEMMs that follow may run over all B*S rows.  act there holds i = f = 0 exactly and finite g, o; hprev is, as everywhere, y
 *   of the direction's previous step: zero at pads except the forward direction's t = lens[b], which holds h of the last live
 *   step (finite, and multiplied by a zero dgates row in the dW_hh GEMM).
 *   Mechanism, bf16 mode: the FORWARD kernels replace the i and f pre-activations they load from gates_x by -1e4 at pads (a
 *   select at the load; gates_x is not written).  sigmoid gives exactly 0 there, hence c = h = 0, and the backward cell gives
 *   exactly zero gate gradients from those saved activations whatever dy holds at the pads: the backward needs no mask.
 *   fp32 mode (exact.hip) has no recurrence kernel of its own to put the select in: icka_lstm_mask_gates writes the same -1e4
 *   into its f32 gate buffer (layout of gates_x) IN PLACE, at every t >= lens[b], before its per-step loop.
 *   No step is skipped: every form walks all S positions with the mask, so a call costs what the fixed-length call costs.
 *   Persistent kernels that stop at the longest live row of the blocks that wait on each other were built and measured: half
 *   the time at a longest row of 64, but the cost did not follow the steps to within the timing spread (one extra step behind
 *   the last token and a launch that stores the unwalked positions) -- profiles/NEGATIVE_RESULTS.md, profiles/lstm_varlen.txt.
 *   icka_lstm_bwd_varlen therefore computes exactly what icka_lstm_bwd computes (``lens`` is accepted for symmetry and for a
 *   later trimmed form).  The give-up / NaN-poison path and icka_lstm_test_hooks are unchanged. */
int icka_lstm_fwd_varlen(const float* gates_x, int64_t ldg, const void* w_hh, void* y, float* c_all, void* act, void* hprev,
                         const int32_t* lens, int32_t B, int32_t S, int32_t H, int32_t flags, void* stream);
int icka_lstm_bwd_varlen(const void* dy, const void* w_hh_t, const void* act, const float* c_all, void* dgates, int64_t ldg,
                         float* dc_carry, const int32_t* lens, int32_t B, int32_t S, int32_t H, int32_t flags, void* stream);
int icka_lstm_mask_gates(float* gates_x, int64_t ldg, const int32_t* lens, int32_t B, int32_t S, int32_t H, void* stream);
/* The persistent launches wait on words written by other blocks of the same grid, with a bounded spin.  A wait that gives
 * up (a peer block that never became resident, a lost word) raises a sticky error word AND poisons the recurrence: the
 * waiting block continues with NaN operands, so every later step of every block -- y, the loss, every gradient of the
 * call -- is NaN: a failed launch never passes for a result.  icka_lstm_barrier_error() returns 1 once that has happened,
 * 0 otherwise, -1 if the query itself failed; the word lives in host memory mapped into the device, so the query costs no
 * device synchronisation and the host side (icka_amd/lstm.py, icka_amd/graph.py) polls it at every touch-point and raises.
 * icka_lstm_clear_error() resets it.  (The reference's nn.LSTM, Cross_Modal_Interaction_Module.py:905-908 / :1042, cannot
 * fail this way; this is the price of the one-launch recurrence.) */
int icka_lstm_barrier_error(void);
int icka_lstm_clear_error(void);
/* CUs to keep free of persistent LSTM blocks (default 0): the persistent forms are used only when their grid fits into the
 * device's CUs minus this reserve, else the one-launch-per-step form runs.  dp.GradReducer reserves the CUs RCCL's
 * all-reduce workgroups may occupy on the communication stream while the recurrence runs. */
int icka_lstm_set_reserved_cus(int32_t n);
/* Test hooks of the give-up path (tests/test_lstm_gpu.py): poll_limit > 0 replaces the poll budgets of all persistent
 * forms (0 restores the defaults); drop_step >= 0 makes block (0, direction 0, batch tile 0) skip publishing that step so
 * that its consumers time out (-1: off). */
int icka_lstm_test_hooks(int32_t poll_limit, int32_t drop_step);
/* y bf16 [M <= 64, N] = act(x . W^T + bias) for a handful of rows (BertPooler.forward :675-681: tanh(dense(h[:, 0])),
 * 32 rows at c2): x bf16 rows with stride ldx, W bf16 [N,K], K % 128 == 0; act 0 = none, 1 = tanh. */
int icka_linear_small_m(const void* x, int64_t ldx, const void* W, const float* bias, void* y, int64_t ldy, int32_t M,
                        int32_t N, int32_t K, int32_t act, void* stream);
/* out[b][c][r] = in[b][r][c] for bf16 matrices (batch of [R,C]). */
int icka_transpose_bf16(const void* in, void* out, int32_t batch, int32_t R, int32_t C, void* stream);
/* ---------------------------------------------------------------------------------------------------------------
 * Frozen ResNet image encoder, forward only (resnet/resnet.py:57-150 Bottleneck / ResNet,
 * resnet/resnet_utils.py:13-53 myResnet.forward).  Convolutions run as icka_gemm calls on NHWC bf16 activations with
 * eval-mode BatchNorm folded into weight / bias and ReLU / residual add in the epilogue (ICKA_EPI_RELU,
 * ICKA_EPI_ADD_RELU); these entry points build the operands.  rows_padded >= B*Ho*Wo: rows past the end are zeroed so
 * the GEMM M dimension can be a multiple of 128.
 *   stem_patches : image f32 NCHW [B,3,H,W] -> 7x7/s2/p3 patches bf16 [rows_padded, 192], k = (ky*7+kx)*3 + c, 147..191 = 0
 *   im2col3x3    : NHWC bf16 [B,H,W,C] -> [rows_padded, 9*C], k = (ky*3+kx)*C + c, pad 1, stride 1 or 2
 *   subsample    : rows (stride*y, stride*x) of an NHWC map (strided 1x1 convolution input)
 *   maxpool3x3s2 : nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
 *   features_out : x bf16 [B,P,C] -> att f32 [B,C,P] (NCHW), fc f32 [B,C] = mean over P, tokens bf16 [B*P,C] (nullable) */
int icka_conv_stem_patches(const float* image, void* patches, int32_t B, int32_t H, int32_t W, int64_t rows_padded,
                           void* stream);
int icka_conv_im2col3x3(const void* src, void* patches, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride,
                        int64_t rows_padded, void* stream);
/* The 3x3 / pad 1 convolution itself (stride 1 or 2) as an IMPLICIT GEMM: y bf16 [rows_padded, Cout] = epilogue(patches(x) .
 * w^T + bias (+ aux)), x NHWC bf16 [B,H,W,C] (C % 64 == 0), w bf16 [Cout, 9*C] with k = (ky*3+kx)*C + c (Cout % 64 == 0),
 * epilogue ICKA_EPI_NONE / RELU / ADD / ADD_RELU (aux bf16 [rows_padded, ldaux]), zeros = at least 128 B of zero bytes.
 * Same result as icka_conv_im2col3x3 + icka_gemm without the 9x patch matrix (resnet/resnet.py:63-64 conv2 + bn2 + relu). */
int icka_conv3x3_gemm(const void* x, const void* w, const float* bias, const void* aux, int64_t ldaux, void* y, int32_t B,
                      int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t stride, int64_t rows_padded, int32_t epilogue,
                      const void* zeros, void* stream);
int icka_conv_subsample(const void* src, void* dst, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride,
                        int64_t rows_padded, void* stream);
int icka_conv_maxpool3x3s2(const void* src, void* dst, int32_t B, int32_t H, int32_t W, int32_t C, int64_t rows_padded,
                           void* stream);
int icka_conv_features_out(const void* x, float* att, float* fc, void* tokens, int32_t B, int32_t P, int32_t C,
                           void* stream);
/* Train-mode BatchNorm of the ResNet encoder (nn.BatchNorm2d in training mode, track_running_stats=True; ResNet(...,
 * train_batchnorm=True)).  Each BN'd convolution runs as three launches:
 *  1. icka_gemm_bn_stats (1x1 convolutions, stem patch GEMM: y = a . w^T, a bf16 [M, lda], w bf16 [N, ldw], NT) or
 *     icka_conv3x3_gemm_stats (the implicit 3x3 convolution, arguments as icka_conv3x3_gemm): writes the RAW output bf16
 *     [M, N] (no bias, no activation) and, from the f32 accumulators, partials f32 [3][M / 128][N] = (count, mean, M2) of
 *     every (128-row tile, channel) over the rows m < rows_valid.  M % 128 == 0, N % 64 == 0, K % 64 == 0.
 *  2. icka_bn_finalize: merges the tiles' partials per channel in a fixed order (Chan's parallel variance), then
 *     scale = weight / sqrt(var + eps), shift = bias - mean * scale, running_mean / running_var <- (1 - m) * old + m * (mean,
 *     var * n / (n - 1)), m = momentum, or 1 / (num_batches_tracked + 1) when momentum < 0 (momentum=None).  In place on the
 *     device: graph-capturable, no host synchronisation.  num_batches_tracked is only read.  A partial whose count is 0 is
 *     skipped whatever its mean and M2 hold.  With a total count n == 1 the variance is 0 and so is the value blended into
 *     running_var (no n / (n - 1)); with n == 0 (every count zero) the mean is 0 too: scale = weight / sqrt(eps), shift = bias,
 *     and both running statistics become (1 - m) * old.  (The Python caller refuses rows_valid < 2.)
 *  3. icka_bn_apply: y = [relu](raw * scale + shift [+ r]) on rows < rows_valid, zeros on [rows_valid, rows_padded); r =
 *     residual (bf16), or residual * res_scale + res_shift when res_scale is given (the downsample branch); y may be raw.
 *     Adds 1 to *nbt_a and *nbt_b (int64 num_batches_tracked, each nullable): the increment of the BatchNorms it applies. */
int icka_gemm_bn_stats(const void* a, int64_t lda, const void* w, int64_t ldw, void* y, int64_t ldy, int32_t M, int32_t N, int32_t K,
                       int64_t rows_valid, float* partials, void* stream);
int icka_conv3x3_gemm_stats(const void* x, const void* w, void* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Cout,
                            int32_t stride, int64_t rows_padded, const void* zeros, float* partials, void* stream);
int icka_bn_finalize(const float* partials, int32_t tiles, int32_t C, const float* weight, const float* bias, float* running_mean,
                     float* running_var, const int64_t* num_batches_tracked, float momentum, float eps, float* scale, float* shift,
                     void* stream);
int icka_bn_apply(const void* raw, const float* scale, const float* shift, const void* residual, const float* res_scale,
                  const float* res_shift, void* y, int32_t C, int64_t rows_valid, int64_t rows_padded, int32_t relu, int64_t* nbt_a,
                  int64_t* nbt_b, void* stream);
/* Dropout nonce for hipGraph replay.  Every dropout-bearing kernel XORs two DEVICE words into its (by-value) seed at
 * entry when a nonce is registered.  A captured graph re-launches the same seed values, so the graph also captures
 * icka_bump_dropout_nonce at the start of a step: each replay then draws fresh masks, and the forward and backward
 * kernels of one replay still see the same nonce.  NULL (default) disables it.  Process-global. */
int icka_set_dropout_nonce(const uint32_t* device_words);
int icka_bump_dropout_nonce(uint32_t* device_words, void* stream);
/* Debug/test helper: materialise the dropout keep-multiplier (0 or 1/(1-p)) for element indices [0,n) as f32. */
int icka_dropout_mask(float* out, int64_t n, float p_drop, uint64_t seed, void* stream);
/* The same for the attention-probability dropout of icka_attn_fwd / icka_attn_bwd (and the fp32-mode softmax): the multiplier
 * of element (row, key) of a [rows, Skv] probability matrix, rows = (batch * heads + head) * Sq + query.  These sites draw two
 * decisions from one 32-bit hash -- hash(row * Skv + key / 2), low 16 bits for even keys, high 16 bits for odd keys -- so
 * their mask is NOT icka_dropout_mask of the flat index. */
int icka_attn_dropout_mask(float* out, int64_t rows, int32_t Skv, float p_drop, uint64_t seed, void* stream);

/* ===============================================================================================================
 * fp32 "exact" mode (icka_amd.set_precision(model, "fp32")): the same path in f32 storage and f32 arithmetic, for
 * BASELINE.json's "within 1e-3 fp32" bar -- the reference is fp32 end to end (SURVEY.md section 0;
 * Cross_Modal_Interaction_Module.py:950).  Every contraction runs on the f32-input matrix instruction
 * v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain); attention materialises its scores as the reference does
 * (:488-502).  All pointers are f32 device pointers unless stated.  Used only when selected; never a fallback.
 *
 * Batched GEMM  C[b0,b1] = alpha * op(A[b0,b1]) . op(B[b0,b1]) (+ bias[n]) (+ beta * C[b0,b1]),  nb0*nb1 <= 65535:
 *   NT: A[M,K] B[N,K]    NN: A[M,K] B[K,N]    TN: A[K,M] B[K,N]    TT: A[K,M] B[N,K]
 * any M, N, K >= 1, any leading dimension; X[b0,b1] = X + b0*x_bs0 + b1*x_bs1 (elements).  Replaces nn.Linear /
 * torch.matmul (:479-481, :488, :502, :533, :549, :562, :958; cl_modeling.py:1363, :1371) and their autograd. */
enum { ICKA_GEMM_TT = 3 };
typedef struct icka_xgemm_desc {
    int32_t op, M, N, K;
    const float* A; int64_t lda, a_bs0, a_bs1;
    const float* B; int64_t ldb, b_bs0, b_bs1;
    float* C; int64_t ldc, c_bs0, c_bs1;
    int32_t nb0, nb1;
    const float* bias;      /* f32 [N] or NULL */
    float alpha, beta;
} icka_xgemm_desc;
int icka_x_gemm(const icka_xgemm_desc* d, void* stream);
/* y = LayerNorm(dropout(x) + residual) * gamma + beta  (BertSelfOutput :561-565, BertOutput :532-536, BertLayerNorm
 * :518-522; x is the dense output WITH its bias).  xhat [M,H] / rstd [M] saved for backward (nullable). */
int icka_x_ln_fwd(const float* x, int64_t ldx, const float* residual, int64_t ldr, const float* gamma,
                  const float* beta, float* y, float* xhat, float* rstd, int32_t M, int32_t H, float eps,
                  float p_drop, uint64_t seed, void* stream);
/* dpre [M,H] = gradient of the LayerNorm input (= of the residual); ddense (nullable) = dpre * dropout mask. */
int icka_x_ln_bwd(const float* dy, int64_t lddy, const float* xhat, const float* rstd, const float* gamma,
                  float* dpre, float* ddense, int32_t M, int32_t H, float p_drop, uint64_t seed, void* stream);
/* out[c] (+)= sum_r a[r,c] * (b ? b[r,c] : 1)   (bias and LayerNorm parameter gradients; fixed summation order) */
int icka_x_colsum(const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int32_t M, int32_t N,
                  int32_t accumulate, void* stream);
/* BertEmbeddings.forward :398-410 up to the LayerNorm (dropout: icka_x_dropout); scatter = backward into the tables
 * from the LayerNorm-input gradient (f32 atomics, padding_idx row of the word table skipped). */
int icka_x_embed_fwd(const int64_t* ids, const int64_t* token_type, const float* word, const float* pos,
                     const float* typ, const float* gamma, const float* beta, float* y, float* xhat, float* rstd,
                     int32_t B, int32_t S, int32_t H, float eps, void* stream);
int icka_x_embed_scatter(const float* dpre, const int64_t* ids, const int64_t* token_type, float* dword, float* dpos,
                         float* dtyp, int32_t B, int32_t S, int32_t H, int32_t padding_idx, void* stream);
/* In place P[B,heads,Sq,Skv] = softmax(P*scale + add_mask[b,j]) (:489-494); Pd = dropout(P) (:500) when p_drop > 0.
 * Backward, in place on dS (which holds dPd on entry): dS = P * (dPd*mask - sum_j dPd*mask*P) * scale. */
int icka_x_softmax_fwd(float* P, float* Pd, const float* add_mask, int32_t B, int32_t heads, int32_t Sq, int32_t Skv,
                       float scale, float p_drop, uint64_t seed, void* stream);
int icka_x_softmax_bwd(const float* P, float* dS, int32_t B, int32_t heads, int32_t Sq, int32_t Skv, float scale,
                       float p_drop, uint64_t seed, void* stream);
/* Elementwise activations.  mode 0: y = gelu(x) (erf form, :31-37); 1: y = tanh(x) (BertPooler :675-681);
 * 2: y2 = sigmoid(x), y = y2 * aux (cl_modeling.py:1363-1367).
 * Backward: mode 0: dx = dy * gelu'(saved = x); 1: dx = dy * (1 - saved^2), saved = y; 2 (saved = gate, aux = cross):
 * dx = dy * aux * g(1-g) (gradient of the gate pre-activation), dx2 = dy * g (gradient of cross through the product). */
int icka_x_act_fwd(const float* x, const float* aux, float* y, float* y2, int64_t n, int32_t mode, void* stream);
int icka_x_act_bwd(const float* dy, const float* saved, const float* aux, float* dx, float* dx2, int64_t n,
                   int32_t mode, void* stream);
/* y = x * keep(i) / (1-p), the same counter-hash mask as the bf16 kernels (forward and backward are the same call) */
int icka_x_dropout(const float* x, float* y, int64_t n, float p_drop, uint64_t seed, void* stream);
int icka_x_add(const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t ldo, int32_t M,
               int32_t N, void* stream);
/* out [M, Ha+Hb] = [a | b]  (torch.cat((seq, cross), dim=-1), cl_modeling.py:1363-1370) */
int icka_x_concat2(const float* a, int64_t lda, int32_t Ha, const float* b, int64_t ldb, int32_t Hb, float* out,
                   int32_t M, void* stream);
/* f32 twin of icka_regions_to_tokens */
int icka_x_regions_to_tokens(const float* src, float* dst, int32_t B, int32_t R, int32_t C, int32_t layout,
                             void* stream);
/* f32 twins of icka_sample_gate_fwd / _bwd (dgate is OVERWRITTEN: one block per sample, fixed order) */
int icka_x_sample_gate_fwd(const float* a, int64_t lda, const float* c, int64_t ldc, const float* gate, int32_t mode,
                           float* out, int64_t ldo, int32_t B, int32_t S, int32_t H, void* stream);
int icka_x_sample_gate_bwd(const float* dout, int64_t lddo, const float* a, int64_t lda, const float* c, int64_t ldc,
                           const float* gate, int32_t mode, float* da, int64_t ldda, float* dc, int64_t lddc,
                           float* dgate, int32_t B, int32_t S, int32_t H, void* stream);
/* BiLSTM recurrence of the fp32 mode (nn.LSTM(H, H, batch_first=True, bidirectional=True), :905-908, call :1042).  The
 * gate pre-activations of step k are accumulated into gates [B*S, 8H] (= x.W_ih^T + b_ih + b_hh for all steps, both
 * directions: [i f g o | i f g o]) by icka_x_gemm with beta = 1 (h_{t-1} . W_hh^T, batched over the two directions);
 * cell_fwd then applies the cell update of step k for both directions (forward direction t = k, reverse t = S-1-k):
 * gates <- activations (saved), c_all / y [B*S, 2H] <- c_t / h_t, hprev <- the h_{t-1} it used (zeros at k = 0).
 * cell_bwd (k = S-1 .. 0): act <- gate pre-activation gradients in place, from dy, the gradient dh_rec [2,B,H] that
 * reached h_t through the next step's recurrent product (first != 0: none yet) and the cell-state carry dc_carry [2,B,H]. */
int icka_x_lstm_cell_fwd(float* gates, float* c_all, float* y, float* hprev, int32_t B, int32_t S, int32_t H, int32_t k,
                         void* stream);
int icka_x_lstm_cell_bwd(const float* dy, const float* dh_rec, float* dc_carry, float* act, const float* c_all, int32_t B,
                         int32_t S, int32_t H, int32_t k, int32_t first, void* stream);
/* f32 twins of icka_embed_prompt_fwd / _bwd (the LayerNorm parameter gradients come from icka_x_colsum; the scatter
 * takes the LayerNorm-input gradient; dprompt f32 [B,P,H], every row written exactly once) */
int icka_x_embed_prompt_fwd(const int64_t* ids, const int32_t* src, const float* prompt, const float* word, const float* pos,
                            const float* typ, const float* gamma, const float* beta, float* y, float* xhat, float* rstd,
                            int32_t B, int32_t S_in, int32_t S, int32_t P, int32_t H, int32_t pos_offset, float eps,
                            void* stream);
int icka_x_embed_prompt_scatter(const float* dpre, const int64_t* ids, const int32_t* src, float* dword, float* dpos,
                                float* dtyp, float* dprompt, int32_t B, int32_t S_in, int32_t S, int32_t P, int32_t H,
                                int32_t pos_offset, int32_t padding_idx, void* stream);
/* f32 twins of icka_token_ce / icka_scale_by_ratio (dlogits f32 [M,C] contiguous, unscaled).  A row counts if and only if
 * mask != 0 and 0 <= label < C in 64 bits; a row that does not count adds nothing to loss_sum / count and has an all-zero
 * gradient row. */
int icka_x_token_ce(const float* logits, int64_t ld, const int64_t* labels, const int64_t* mask, float* loss_sum,
                    float* count, float* dlogits, int32_t M, int32_t C, void* stream);
int icka_x_scale_by_ratio(const float* x, float* y, const float* num, const float* den, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Data-parallel helpers (csrc/dp.hip).  Reference: apex DistributedDataParallel all-reduces the gradients of every
 * parameter during backward (My_cross_attention.py:768-776, process group :653-657, launch line :1104); here the exchange
 * is RCCL over xGMI driven by icka_amd/dp.py, and these entry points are what runs around it on the GPU.
 *
 * Wire format: gradients travel as bf16.  Matrix gradients get their wire copy from the weight-gradient GEMM itself
 * (icka_gemm_desc.C3 beside an f32 C: the value after beta-accumulation); everything else in a bucket is cast by ONE launch
 * over a chunk table:
 *   icka_dp_cast_chunks: table_dev = n_chunks x {first element, element count} (int64 pairs in device memory; counts are
 *     multiples of 8 and at most icka_dp_chunk_elems()); dst[i] = bf16(src[i]) for every i in a chunk; src / dst are the
 *     BASES of the flat f32 gradient buffer / the bf16 wire buffer (same element offsets).
 *   icka_dp_cast_back_scaled: dst f32 [n] = src bf16 [n] * scale (the reduced bucket back into the gradient buffer, with the
 *     1 / world factor of the mean folded in: the all-reduce is a SUM).
 * Bucket-ready flags for a step captured as ONE hipGraph with eager collectives (icka_amd/graph.py: FlaggedStep):
 *   icka_dp_step_bump(step_word): step_word[0] += 1 -- first node of the graph;
 *   icka_dp_flag_set(flag_word, step_word): flag_word[0] = step_word[0] -- a node right after the kernel that finishes the
 *     bucket's last gradient;
 *   icka_dp_flag_wait(flag_word, tag, bad_word, max_polls): a one-wave kernel for the COMMUNICATION stream that returns once
 *     flag_word[0] >= tag (wrap-safe), polling with s_sleep at most max_polls times; if it gives up it raises the error word
 *     read by icka_dp_error() (host memory mapped into the device: no synchronisation) and, when bad_word (device memory,
 *     one uint32 per bucket) is given, stores tag there.  The NaN itself is written by kernels ordered AFTER everything
 *     that could overwrite it:
 *   icka_dp_poison_if(bad_word, tag, target, target_is_bf16, n): if bad_word[0] == tag, NaN into target[0 .. n) (n <= 64;
 *     bf16 or f32 elements) -- on the communication stream between the bucket's chunk cast and its all-reduce (the NaN
 *     reaches every rank through the sum) and again after the cast-back;
 *   icka_dp_poison_final(bad_words, n_buckets, tag, gflat, starts_dev, n): one launch on the COMPUTE stream after the join
 *     that ends the step (the graph's late gradient stores are over): for every bucket b with bad_words[b] == tag, NaN into
 *     gflat[starts_dev[b] .. + n).
 *   icka_dp_init() maps the error word (not inside a stream capture); icka_dp_clear_error() resets it. */
int64_t icka_dp_chunk_elems(void);
int icka_dp_cast_chunks(const float* src, void* dst_bf16, const int64_t* table_dev, int32_t n_chunks, void* stream);
int icka_dp_cast_back_scaled(const void* src_bf16, float* dst, int64_t n, float scale, void* stream);
int icka_dp_init(void);
int icka_dp_error(void);
int icka_dp_clear_error(void);
int icka_dp_step_bump(void* step_word, void* stream);
int icka_dp_flag_set(void* flag_word, const void* step_word, void* stream);
int icka_dp_flag_wait(const void* flag_word, uint32_t tag, void* bad_word, int32_t max_polls, void* stream);
int icka_dp_poison_if(const void* bad_word, uint32_t tag, void* target, int32_t target_is_bf16, int32_t n, void* stream);
int icka_dp_poison_final(const void* bad_words, int32_t n_buckets, uint32_t tag, float* gflat, const int64_t* starts_dev,
                         int32_t n, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The parameter update that follows backward in the reference's loop (My_cross_attention.py:831-844: clip_grad_norm_(1.0),
 * AdamW.step() over the two weight-decay groups of :743-751) as three launches over the flat parameter / gradient / state
 * buffers (csrc/optim.hip; icka_amd/optim.py: ArenaAdamW).  Outside the fwd+bwd metric, reported beside it.  Chunk tables as
 * for icka_dp_cast_chunks (int64 pairs {first element, count}, counts multiples of 8, at most icka_optim_chunk_elems()).
 *   icka_optim_sqnorm: partials[b] = sum of squares of grads over chunk b.
 *   icka_optim_clip:   out2[0] = sqrt(sum of the n partials) (fixed order), out2[1] = min(1, max_norm / (norm + 1e-6)) --
 *                      torch.nn.utils.clip_grad_norm_'s coefficient, left on the device (max_norm <= 0: 1).
 *   icka_optim_adamw:  torch.optim.AdamW arithmetic for the chunks of ONE weight-decay group: p *= 1 - lr * wd;
 *                      m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t)
 *                      + eps), with g = grads * clip_coef[0] (clip_coef may be NULL); also writes the bf16 (and fp16) weight
 *                      shadow of every updated element when shadow pointers are given (same element offsets). */
int64_t icka_optim_chunk_elems(void);
int icka_optim_sqnorm(const float* grads, const int64_t* table_dev, int32_t n_chunks, float* partials, void* stream);
int icka_optim_clip(const float* partials, int32_t n, float max_norm, float* out2, void* stream);
int icka_optim_adamw(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, void* shadow_f16,
                     const int64_t* table_dev, int32_t n_chunks, const float* clip_coef, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int32_t step, void* stream);

/* The same update with the step count, the learning-rate schedule and the bias corrections held on the DEVICE, so that it can be
 * captured into a graph with the step it follows (icka_amd/optim.py: ArenaAdamW(capturable=True); icka_amd/train_step.py).
 * Added under ABI version 6.  The state block is one 8-byte-aligned device buffer of this layout; "device" fields are written
 * by icka_optim_prepare only, "host" fields by the caller (uploaded outside a capture), never by a kernel:
 *   t, skipped       device  updates applied / updates refused for a non-finite gradient norm (the host writes t on resume)
 *   norm, coef       device  total gradient norm of the last prepare, and its clip coefficient
 *   skip             device  1: the update launch behind this prepare returns without touching memory
 *   kind..total      host    schedule: factor(t) = 1 (CONSTANT) or get_linear_schedule_with_warmup's lambda (LINEAR):
 *                            t / max(1, warmup) for t < warmup, else max(0, (total - t) / max(1, total - warmup))
 *   n_groups, base_lr, beta1, beta2, eps, weight_decay   host   per weight-decay group, at most ICKA_OPTIM_MAX_GROUPS
 *   lr, bc1, bc2_sqrt   device  what update number t + 1 uses: (float)(base_lr * factor(t)) with factor in double (a LambdaLR
 *                            hands the host-mode kernel the same float), 1 - beta1^(t+1), sqrt(1 - beta2^(t+1)) */
#define ICKA_OPTIM_MAX_GROUPS 8
#define ICKA_OPTIM_SCHEDULE_CONSTANT 0
#define ICKA_OPTIM_SCHEDULE_LINEAR 1
#define ICKA_OPTIM_DRY 1        /* prepare flag: set skip, change nothing else (warm-up launches ahead of a capture) */
#define ICKA_OPTIM_NO_GUARD 2   /* prepare flag: apply the update also when the norm is not finite */
typedef struct icka_optim_state {
    int64_t t;
    int64_t skipped;
    float norm;
    float coef;
    int32_t skip;
    int32_t reserved;
    int32_t kind;
    int32_t n_groups;
    int64_t warmup;
    int64_t total;
    double base_lr[ICKA_OPTIM_MAX_GROUPS];
    float beta1[ICKA_OPTIM_MAX_GROUPS];
    float beta2[ICKA_OPTIM_MAX_GROUPS];
    float eps[ICKA_OPTIM_MAX_GROUPS];
    float weight_decay[ICKA_OPTIM_MAX_GROUPS];
    float lr[ICKA_OPTIM_MAX_GROUPS];
    float bc1[ICKA_OPTIM_MAX_GROUPS];
    float bc2_sqrt[ICKA_OPTIM_MAX_GROUPS];
} icka_optim_state;
/*   icka_optim_prepare:   one block, after icka_optim_sqnorm (n = 0: no partials, norm 0).  Sums the partials in
 *                         icka_optim_clip's order (bitwise the same norm).  A finite sum: writes norm, coef (max_norm <= 0: 1),
 *                         lr / bc1 / bc2_sqrt of every group for update t + 1, advances t, clears skip.  A non-finite sum:
 *                         sets skip, skipped += 1; t and the per-step values stay.  t therefore advances exactly once per
 *                         applied update, in this launch; no launch behind the update is needed.
 *   icka_optim_adamw_dev: icka_optim_adamw's arithmetic and shadow stores for the chunks of ALL groups in one launch: the table
 *                         has three int64 per chunk {first element, count, group}; every block reads skip first. */
int icka_optim_prepare(const float* partials, int32_t n, float max_norm, int32_t flags, void* state, void* stream);
int icka_optim_adamw_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, void* shadow_f16,
                         const int64_t* table3_dev, int32_t n_chunks, const void* state, void* stream);

/* An averaged copy of the weights beside the update (icka_amd/optim.py: ArenaAdamW(average="ema" | "swa")): one more f32
 * buffer of the parameters' layout, one table-driven launch behind the update, and an in-place exchange that leaves every
 * address a captured graph holds valid.  Added under ABI version 6 (additive).  Chunk tables as for icka_optim_adamw (int64
 * pairs {first element, count}, counts multiples of 8, at most icka_optim_chunk_elems()); elements in no chunk are never read
 * or written.
 *   icka_optim_average:  avg <- avg + (1 - decay) * (params - avg) per element, in f32; decay == 0 copies params bit for bit
 *                        (the first averaged update).
 * The capturable form keeps the count of averaged updates and this update's decay in a device block of this layout (8-byte
 * aligned); "device" fields are written by icka_optim_average_prepare only, "host" fields by the caller outside a capture:
 *   n                   device  averaged updates so far (the host writes it on resume)
 *   decay_now, apply    device  what the averaging launch behind this prepare uses; apply == 0: it touches no memory
 *   kind, warmup        host    ICKA_AVERAGE_EMA / ICKA_AVERAGE_SWA; EMA: 1 = the decay is warmed up
 *   decay               host    EMA decay in [0, 1)
 *   start, every        host    update number t (1-based, icka_optim_state.t after its prepare) is averaged iff t > start and
 *                               (t - start - 1) % every == 0 */
#define ICKA_AVERAGE_EMA 0
#define ICKA_AVERAGE_SWA 1
typedef struct icka_average_state {
    int64_t n;
    float decay_now;
    int32_t apply;
    int32_t kind;
    int32_t warmup;
    double decay;
    int64_t start;
    int64_t every;
} icka_average_state;
/*   icka_optim_average_prepare: one thread, after icka_optim_prepare.  optim_state->skip set (a dry warm-up launch, a refused
 *                        non-finite update): apply = 0, nothing else changes.  Otherwise apply as above from optim_state->t;
 *                        when applying, decay_now = (float) of, in double: 0 if n == 0; n / (n + 1) for SWA; for EMA
 *                        min(decay, (1 + n) / (10 + n)) with warm-up, else decay; then n += 1.
 *   icka_optim_average_dev: icka_optim_average's arithmetic with decay_now read from the block; every block reads apply first.
 *   icka_optim_swap:     exchanges params and avg element by element and writes the bf16 (and fp16, when given) shadow of the
 *                        new params as icka_optim_adamw writes them (same rounding, same +-65504 clamp).  Applied twice it
 *                        restores every buffer bit for bit. */
int icka_optim_average(const float* params, float* avg, const int64_t* table_dev, int32_t n_chunks, float decay, void* stream);
int icka_optim_average_prepare(void* average_state, const void* optim_state, void* stream);
int icka_optim_average_dev(const float* params, float* avg, const int64_t* table_dev, int32_t n_chunks, const void* average_state,
                           void* stream);
int icka_optim_swap(float* params, float* avg, void* shadow_bf16, void* shadow_f16, const int64_t* table_dev, int32_t n_chunks,
                    void* stream);

/* Sharpness-aware minimisation on the flat parameter buffers (csrc/sam.hip; icka_amd/sam.py: SAM): the gradient at w, an ascent
 * to w + e(w), the gradient there, the way back, and the optimizer's update of w with that second gradient (SAM, Foret et al.
 * 2021; the scale-invariant ASAM, Kwon et al. 2021).  None of it is in the reference, which trains without SAM.  Added under ABI
 * version 6 (additive).  Chunk tables as for icka_optim_adamw (int64 pairs {first element, count}, counts multiples of 8, at most
 * icka_optim_chunk_elems()); elements in no chunk are never read or written.  The values of one ascent live in a device block of
 * this layout (8-byte aligned), written by thread 0 of icka_sam_prepare with ordinary stores and read by the launches behind it
 * on the stream; the host only ever reads it:
 *   norm             norm of the first-pass gradient: sqrt(sum of (t g)^2), t = 1 (plain) or |p| (adaptive)
 *   scale            step scale of this ascent: (float)(rho / ((double)norm + 1e-12)); 0 for a refused one
 *   skip             1: the ascend and restore launches behind this prepare return without touching memory
 *   ascents, skipped ascents applied / refused so far (a dry prepare counts as neither) */
#define ICKA_SAM_DRY 1          /* prepare flag: set skip, change nothing else (warm-up launches ahead of a capture) */
typedef struct icka_sam_state {
    float norm;
    float scale;
    int32_t skip;
    int32_t reserved;
    int64_t ascents;
    int64_t skipped;
} icka_sam_state;
/*   icka_sam_sqnorm:  partials[b] = sum of (t g)^2 over chunk b.  adaptive == 0: icka_optim_sqnorm itself (params is not read and
 *                     may be NULL; bitwise its partials).  adaptive != 0: the same loop and reduction tree over a = |p| * g.
 *   icka_sam_prepare: one block.  Sums the n partials in icka_optim_clip's order, in double; norm = (float)sqrt(sum).  A sum that
 *                     is not finite or is zero: skip = 1, skipped += 1, scale = 0.  Otherwise scale as above, skip = 0,
 *                     ascents += 1.  rho must be positive.
 *   icka_sam_ascend:  returns at once when skip is set.  Otherwise per element backup = p and p <- p + e, every operation an f32
 *                     rounding of its own (no fused multiply-add), in this order: plain e = scale * g (two roundings with the
 *                     sum); adaptive t = p * p, u = t * g, e = u * scale (four) -- e = p^2 g rho / || |p| g ||, over every
 *                     element of the table, biases included.  Writes the bf16 (and fp16, when given) shadow of the new p as
 *                     icka_optim_adamw writes them (same rounding, same +-65504 clamp); either shadow pointer may be NULL.
 *   icka_sam_restore: returns at once when skip is set.  Otherwise p = backup bit for bit, and the shadows of p.  (Not p - e:
 *                     the weights after a step are then bitwise what the optimizer left, and a NaN that reached the
 *                     perturbation cannot survive it.) */
int icka_sam_sqnorm(const float* params, const float* grads, const int64_t* table_dev, int32_t n_chunks, int32_t adaptive,
                    float* partials, void* stream);
int icka_sam_prepare(const float* partials, int32_t n, float rho, int32_t flags, void* state, void* stream);
int icka_sam_ascend(float* params, const float* grads, float* backup, void* shadow_bf16, void* shadow_f16, const int64_t* table_dev,
                    int32_t n_chunks, int32_t adaptive, const void* state, void* stream);
int icka_sam_restore(float* params, const float* backup, void* shadow_bf16, void* shadow_f16, const int64_t* table_dev,
                     int32_t n_chunks, const void* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICKA_HIP_H */
