// The 8-wave warp-specialised body (gemm_ws.inc) with something fused to it (DESIGN.md section 4).  Kernels in this file:
//   gemm_ln_kernel             dense -> bias + dropout + residual -> LayerNorm in one launch (icka_gemm_ln; row body: ln_row.h)
//   gemm_ws_bn_stats_kernel    raw output + the train-mode BatchNorm partials of its tile columns (icka_gemm_bn_stats)
//   gemm_ws_kernel<.., CONV>   the A tile gathered from an NHWC activation: implicit 3x3 convolution (icka_conv3x3_gemm*)
// A source fragment of gemm.hip, included once there.
#include "ln_row.h"

namespace {

// Convolution GEMM of a train-mode BatchNorm layer (icka_gemm_bn_stats, icka_conv3x3_gemm_stats): NT, bf16, 128 x BNT tiles,
// raw bf16 output + the per-(row tile, column) partials of bn_stats_tile.
struct BnStatsArgs { GemmArgs g; float* part; int rows_valid; };
template <int BNT, bool CONV>
__global__ __launch_bounds__(512) void gemm_ws_bn_stats_kernel(const BnStatsArgs p) {
    const GemmArgs g = p.g;
    __shared__ __attribute__((aligned(16))) char smem[3 * 2 * TILE_BYTES];
    gemm_ws_body<false, false, 3, 0, 2, BNT, false, CONV, false, true>(g, smem, blockIdx.x, gridDim.x, p.part, p.rows_valid);
}

// =====================================================================================================================
// dense -> bias + dropout + residual -> LayerNorm in ONE launch (BertSelfOutput.forward Cross_Modal_Interaction_Module.py:
// 561-565, BertOutput.forward :532-536): the 128 x BNT NT kernel above for shapes whose tile grid is one block per CU with
// EIGHT column tiles per 128-row stripe (N = 768 with 96-wide tiles, N = 1024 with 128-wide ones; M / 128 stripes, at most one
// block per CU).  Where M / 128 is a multiple of 8, tile_origin puts the 8 blocks of a stripe on one XCD (blocks b, b + 8, ...
// share an XCD under the observed round-robin dispatch) -- a speed property only, nothing below depends on it: with other stripe
// counts (the reference's test loop at batch 4: M = 512) a stripe spreads over two or three XCDs and the hand-off still holds.
//   phase 1  the tile's f32 output is stored write-through (sc1) into the usual GEMM -> LayerNorm intermediate;
//   seam     every wave waits for its stores (s_waitcnt vmcnt(0)), the block barrier joins them, ONE lane adds 1 to the stripe's
//            arrival counter (agent scope) and polls it (sc1 load, bounded) until all 8 blocks of the stripe have arrived;
//            measured 0.6 us (max 0.8) on an idle chip against 4.8 us first-block-start -> last-block-end for the same two
//            phases as two launches (tools/probe/xcd_seam_probe.hip, profiles/r05_xcd_seam_probe.txt);
//   phase 2  block j of the stripe finishes rows 16 j .. 16 j + 15 of it -- all 8 waves, two rows each, through the SAME row body
//            as the stand-alone kernel (ln_row.h: bitwise the same y / twin / xhat / rstd), reading the intermediate with
//            L1-bypassing (sc1) loads.
// Why the round-2 attempt at this fusion lost (profiles/r02_gemm_ln_fusion.txt: +6 - 8 us per site) and this form differs: there
// a thread kept 24 columns of a row and the 8 blocks exchanged partial (sum, M2) statistics through four dependent agent-scope
// round trips, then wrote y / twin / xhat as 48 - 96-byte pieces; here the seam is ONE counter and the LayerNorm phase moves whole
// rows, 16 bytes per lane, like the row kernel.  The counters reset themselves: the last of the 8 blocks to LEAVE the wait
// zeroes both words (by then every block of the stripe has seen the count), so a launch leaves the workspace as it found it
// and the same words serve every fused launch of a stream (launches of one stream do not overlap).
// A wait that gives up (a block of the stripe never became resident: grids of more blocks than the device's CUs minus the
// caller's reserve, icka_lstm_set_reserved_cus, are refused on the host) stores 1 into the error word -- host-mapped memory the
// host polls without a device synchronisation -- and the block turns the rows it finished into NaN: never a hang, never a
// silent wrong result.
struct GemmLnArgs {
    GemmArgs g;
    LnFwdArgs ln;
    unsigned int* sync;      // [stripes][32] words: [0] arrivals, [16] departures (one 64-byte line each)
    unsigned int* err;       // error word (host-mapped memory when the caller wants to poll it without a device sync)
    int polls;
    int test_drop;           // test hook: this block never arrives (its stripe's waits give up); -1 = off
};
template <int BNT, bool F16 = false>
__global__ __launch_bounds__(512) void gemm_ln_kernel(const GemmLnArgs p) {
    const GemmArgs g = p.g;
    __shared__ __attribute__((aligned(16))) char smem[3 * 2 * TILE_BYTES];
    __shared__ int s_gave_up;
    int m0, n0;
    tile_origin(blockIdx.x, gridDim.x, g.M / BM, g.N / BNT, m0, n0, BNT);
    const int nbn = g.N / BNT;                             // = 8 (host)
    LnFwdArgs a = p.ln;
    a.drop = drop_resolve(a.drop);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int ROWS_PER_BLOCK = BM / 8, ROWS_PER_WAVE = ROWS_PER_BLOCK / 8;
    const int r0 = m0 + (n0 / BNT) * ROWS_PER_BLOCK + wave * ROWS_PER_WAVE;
    // the residual rows this wave will finish do not depend on the GEMM: requested now, they arrive under the k-loop instead of
    // in the tail, where all 256 blocks would ask HBM for them at the same moment (32 registers per lane, held across the loop)
    float rr[ROWS_PER_WAVE][2][8];
    ln_prefetch_res<2, ROWS_PER_WAVE>(a, r0, lane, rr);
    gemm_ws_body<false, false, 3, 0, 2, BNT, F16, false, true>(g, smem, blockIdx.x, gridDim.x);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's write-through stores have left the CU
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int* arrive = p.sync + (size_t)(m0 / BM) * 32;
        unsigned int* depart = arrive + 16;
        if ((int)blockIdx.x != p.test_drop) __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool ok = false;
        for (int i = 0; i < p.polls; ++i) {
            if (__hip_atomic_load(arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= (unsigned)nbn) { ok = true; break; }
            __builtin_amdgcn_s_sleep(1);
        }
        s_gave_up = ok ? 0 : 1;
        if (!ok) __hip_atomic_store(p.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        // the last block to LEAVE the wait zeroes the stripe's words (every block of the stripe has stopped polling by then --
        // it saw the full count or gave up): the workspace is left as it was found, also after a failed launch
        if (__hip_atomic_fetch_add(depart, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(nbn - 1)) {
            __hip_atomic_store(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(depart, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    ln_fwd_rows_handoff<2, ROWS_PER_WAVE>(a, r0, lane, rr);
    if (s_gave_up) {
        // a failed launch never passes for a result: the rows this block finished from an incomplete stripe become NaN (y is the
        // operand of everything downstream: the loss and every gradient of the step are NaN), and the host raises at its next
        // touch-point (kernels.gemm_ln_check_error)
        const bf16_t qnan = f2bf(__builtin_nanf(""));
        for (int r = 0; r < ROWS_PER_WAVE; ++r)
            for (int c = lane; c < a.H; c += 64) a.y[(int64_t)(r0 + r) * a.ldy + c] = qnan;
    }
}

}  // namespace

constexpr int GEMM_LN_MAX_STRIPES = 64;
static int g_gemm_ln_polls = 0;      // icka_gemm_ln_test_hooks: 0 = the default budget (~7 ms of s_sleep polls)
static int g_gemm_ln_drop = -1;      // icka_gemm_ln_test_hooks: block that never arrives (-1: off)
extern "C" int64_t icka_gemm_ln_sync_words(void) { return (int64_t)GEMM_LN_MAX_STRIPES * 32; }
extern "C" int icka_gemm_ln_test_hooks(int32_t polls, int32_t drop_block) {
    g_gemm_ln_polls = polls > 0 ? polls : 0;
    g_gemm_ln_drop = drop_block >= 0 ? drop_block : -1;
    return 0;
}
extern "C" int icka_gemm_ln(const icka_gemm_desc* d, const float* bias, const void* residual, int64_t ldr, int32_t res_kind,
                            const float* gamma, const float* beta, void* y, int64_t ldy, void* y_twin, int32_t twin_f16,
                            void* xhat, float* rstd, float eps, float p_drop, uint64_t seed, uint32_t* sync_words,
                            uint32_t* error_word, void* stream) {
    if (!d || !gamma || !beta || !y || !sync_words || !error_word) return ICKA_E_ARG;
    if (res_kind < 0 || res_kind > 2) return ICKA_E_ARG;
    GemmArgs g;
    Tune t;
    bool aligned = false;
    const int rc = convert(d, g, aligned, t);
    if (rc) return rc;
    // eligibility (else ICKA_E_SHAPE: the caller takes icka_gemm + icka_ln_fwd): NT, bf16 operands, plain f32 output that the
    // direct epilogue stores, one reduction segment, EIGHT column tiles per stripe, whole groups of 8 stripes, and at most one
    // block per CU -- the blocks of a stripe wait for each other, so all of them must be resident at once
    if (d->op != ICKA_GEMM_NT || g.f16 || !aligned || !g.c_f32 || g.epi != ICKA_EPI_NONE || g.beta != 0.f || g.alpha != 1.f || g.bias ||
        g.bias2 || g.K1 != 0 || g.colsum || g.C3 || !t.direct || !t.ws || d->tune)
        return ICKA_E_SHAPE;
    const int bnt = (g.N % 96 == 0 && g.N / 96 == 8) ? 96 : ((g.N % 128 == 0 && g.N / 128 == 8) ? 128 : 0);
    const int stripes = g.M / BM;
    // (any number of stripes: where M / 128 is not a multiple of 8 a stripe's blocks spread over two or three XCDs -- the hand-off
    //  is write-through stores + agent-scope counter + L1-bypassing loads, correct under any placement, a little slower there)
    if (!bnt || stripes < 1 || stripes > GEMM_LN_MAX_STRIPES || stripes * 8 > icka_device_cus() - g_icka_reserved_cus) return ICKA_E_SHAPE;
    if (g.N % 8 || ldy % 8 || (residual && ldr % 8) || g.ldc % 4) return ICKA_E_ALIGN;
    if ((int64_t)g.M * g.ldc * 4 >= (1ll << 31) - 64) return ICKA_E_SHAPE;      // 32-bit byte offsets of the raw buffer accesses
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (!al16(y) || (residual && !al16(residual)) || (xhat && !al16(xhat)) || (bias && !al16(bias)) || !al16(gamma) || !al16(beta) ||
        (y_twin && !al16(y_twin)))
        return ICKA_E_ALIGN;
    GemmLnArgs p;
    p.g = g;
    p.ln = LnFwdArgs{g.C, g.ldc, 1, bias, residual, ldr, res_kind, gamma, beta, (bf16_t*)y, ldy, nullptr, 0, y_twin, (bf16_t*)xhat, rstd,
                     g.M, g.N, eps, make_drop(p_drop, seed), twin_f16};
    p.sync = sync_words;
    p.err = error_word;
    p.polls = g_gemm_ln_polls > 0 ? g_gemm_ln_polls : (1 << 18);
    p.test_drop = g_gemm_ln_drop;
    hipStream_t st = (hipStream_t)stream;
    if (bnt == 96) ICKA_LAUNCH_RETURN((gemm_ln_kernel<96>), stripes * 8, 512, st, p);
    ICKA_LAUNCH_RETURN((gemm_ln_kernel<128>), stripes * 8, 512, st, p);
}

// 3x3 / pad 1 convolution (stride 1 or 2) of an NHWC bf16 activation as an implicit GEMM on the warp-specialised kernel:
//   y[m, co] = epilogue( sum_{tap, c} x[pixel(m) + tap][c] * w[co][tap * C + c] + bias[co] (+ aux[m, co]) )
// m = output pixel (b, oy, ox) row-major, rows [rows_valid, rows_padded) of y are written from zero patches.
// Replaces icka_conv_im2col3x3 + icka_gemm: the [rows, 9 C] patch matrix (9x the activation) is never written or read.
extern "C" int icka_conv3x3_gemm(const void* x, const void* w, const float* bias, const void* aux, int64_t ldaux, void* y,
                                 int32_t B, int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t stride,
                                 int64_t rows_padded, int32_t epilogue, const void* zeros, void* stream) {
    if (!x || !w || !y || !zeros) return ICKA_E_ARG;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 64 || Cout <= 0 || Cout % 64 || (stride != 1 && stride != 2))
        return ICKA_E_SHAPE;
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    const int64_t rows = (int64_t)B * Ho * Wo;
    if (rows_padded < rows || rows_padded % BM || rows_padded > 0x7fffffff) return ICKA_E_SHAPE;
    if (epilogue != ICKA_EPI_NONE && epilogue != ICKA_EPI_RELU && epilogue != ICKA_EPI_ADD_RELU && epilogue != ICKA_EPI_ADD)
        return ICKA_E_ARG;
    if ((epilogue == ICKA_EPI_ADD_RELU || epilogue == ICKA_EPI_ADD) && !aux) return ICKA_E_ARG;
    auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (!al(x) || !al(w) || !al(y) || !al(zeros) || (aux && (!al(aux) || ldaux % 8)) || (bias && !al(bias))) return ICKA_E_ALIGN;
    GemmArgs g{};
    g.M = (int)rows_padded; g.N = Cout; g.K = 9 * C; g.K1 = 0;
    g.A = (const bf16_t*)x; g.lda = C; g.B = (const bf16_t*)w; g.ldb = 9 * (int64_t)C;
    g.C = y; g.ldc = Cout; g.aux = (const bf16_t*)aux; g.ldaux = ldaux; g.bias = bias;
    g.alpha = 1.f; g.beta = 0.f; g.epi = epilogue; g.c_f32 = 0; g.a_vec = g.b_vec = 1; g.ksplit = 1; g.direct = kTuneEnv.direct;
    g.cvH = H; g.cvW = W; g.cvC = C; g.cvS = stride; g.cvHo = Ho; g.cvWo = Wo; g.cvRows = (int)rows;
    g.cvZero = (const bf16_t*)zeros;
    hipStream_t st = (hipStream_t)stream;
    if (Cout % 128 == 0) ICKA_LAUNCH_RETURN((gemm_ws_kernel<false, false, 3, 0, 128, false, true>), (g.M / BM) * (Cout / 128), 512, st, g);
    ICKA_LAUNCH_RETURN((gemm_ws_kernel<false, false, 3, 0, 64, false, true>), (g.M / BM) * (Cout / 64), 512, st, g);
}

// Train-mode BatchNorm convolutions: the raw output (no bias, no activation) + per-(row tile, channel) partial statistics of
// the f32 accumulators over the rows m < rows_valid (see icka_hip.h).  128 x 128 tiles where N % 128 == 0, else 128 x 64.
static int launch_bn_stats(BnStatsArgs& p, hipStream_t st) {
    GemmArgs& g = p.g;
    g.K1 = 0; g.alpha = 1.f; g.beta = 0.f; g.epi = ICKA_EPI_NONE; g.c_f32 = 0; g.a_vec = g.b_vec = 1; g.ksplit = 1; g.direct = 0;
    if (g.N % 128 == 0) ICKA_LAUNCH_RETURN((gemm_ws_bn_stats_kernel<128, false>), (g.M / BM) * (g.N / 128), 512, st, p);
    ICKA_LAUNCH_RETURN((gemm_ws_bn_stats_kernel<64, false>), (g.M / BM) * (g.N / 64), 512, st, p);
}

extern "C" int icka_gemm_bn_stats(const void* a, int64_t lda, const void* w, int64_t ldw, void* y, int64_t ldy, int32_t M, int32_t N,
                                  int32_t K, int64_t rows_valid, float* partials, void* stream) {
    if (!a || !w || !y || !partials) return ICKA_E_ARG;
    if (M <= 0 || M % BM || N <= 0 || N % 64 || K <= 0 || K % BK || rows_valid < 1 || rows_valid > M) return ICKA_E_SHAPE;
    auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (!al(a) || !al(w) || !al(y) || !al(partials) || lda % 8 || ldw % 8 || ldy % 8 || lda < K || ldw < K || ldy < N)
        return ICKA_E_ALIGN;
    BnStatsArgs p{};
    p.g.M = M; p.g.N = N; p.g.K = K;
    p.g.A = (const bf16_t*)a; p.g.lda = lda; p.g.B = (const bf16_t*)w; p.g.ldb = ldw; p.g.C = y; p.g.ldc = ldy;
    p.part = partials; p.rows_valid = (int)rows_valid;
    return launch_bn_stats(p, (hipStream_t)stream);
}

extern "C" int icka_conv3x3_gemm_stats(const void* x, const void* w, void* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Cout,
                                       int32_t stride, int64_t rows_padded, const void* zeros, float* partials, void* stream) {
    if (!x || !w || !y || !zeros || !partials) return ICKA_E_ARG;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 64 || Cout <= 0 || Cout % 64 || (stride != 1 && stride != 2))
        return ICKA_E_SHAPE;
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    const int64_t rows = (int64_t)B * Ho * Wo;
    if (rows_padded < rows || rows_padded % BM || rows_padded > 0x7fffffff) return ICKA_E_SHAPE;
    auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (!al(x) || !al(w) || !al(y) || !al(zeros) || !al(partials)) return ICKA_E_ALIGN;
    BnStatsArgs p{};
    p.g.M = (int)rows_padded; p.g.N = Cout; p.g.K = 9 * C;
    p.g.A = (const bf16_t*)x; p.g.lda = C; p.g.B = (const bf16_t*)w; p.g.ldb = 9 * (int64_t)C; p.g.C = y; p.g.ldc = Cout;
    p.g.cvH = H; p.g.cvW = W; p.g.cvC = C; p.g.cvS = stride; p.g.cvHo = Ho; p.g.cvWo = Wo; p.g.cvRows = (int)rows;
    p.g.cvZero = (const bf16_t*)zeros;
    p.part = partials; p.rows_valid = (int)rows;
    GemmArgs& g = p.g;
    g.K1 = 0; g.alpha = 1.f; g.beta = 0.f; g.epi = ICKA_EPI_NONE; g.c_f32 = 0; g.a_vec = g.b_vec = 1; g.ksplit = 1; g.direct = 0;
    hipStream_t st = (hipStream_t)stream;
    if (Cout % 128 == 0) ICKA_LAUNCH_RETURN((gemm_ws_bn_stats_kernel<128, true>), (g.M / BM) * (Cout / 128), 512, st, p);
    ICKA_LAUNCH_RETURN((gemm_ws_bn_stats_kernel<64, true>), (g.M / BM) * (Cout / 64), 512, st, p);
}
