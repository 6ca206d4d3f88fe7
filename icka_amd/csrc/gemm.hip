// MFMA GEMM for the ICKA hot path (gfx950), v_mfma_f32_16x16x32_bf16, fp32 accumulation.  Three operand layouts:
//   NT: C = A[M,K] . B[N,K]^T   (both operands k-contiguous: fragments by ds_read_b128)
//   NN: C = A[M,K] . B[K,N]     (B k-major in memory: fragments by ds_read_b64_tr_b16)
//   TN: C = A[K,M]^T . B[K,N]   (both k-major: weight gradients, K = tokens)
// The MFMA is issued as D^T: a-operand = B-tile rows (n), b-operand = A-tile rows (m), so each lane ends up with
// FOUR CONSECUTIVE n of one output row m -> 8-byte (bf16) / 16-byte (f32) row-major stores and vector epilogues.
// One file per kernel family, all compiled into this translation unit (the #includes below say why):
//   gemm_core.h       what every family shares: GemmArgs, Tune, swizzles, tile loaders, fragment reads, epilogues
//   gemm.hip          this file: the host policy (convert, the tune word, the launch ladder, icka_gemm), the general path
//   gemm_ws.inc       aligned path, 128 x 128 / 96 / 64 tiles: the 256-thread DMA kernels, the 8-wave warp-specialised ones
//   gemm_w3.inc       12 waves, 256x192 / 256x128 tiles (wide short-K outputs), and the fused QKV + attention twin
//                     (gemm_w3_body.inc: the statements its plain and its live-rows kernel share)
//   gemm_fused.inc    the 8-wave kernel with a LayerNorm phase, with BatchNorm statistics, as an implicit 3x3 convolution
//   gemm_grouped.inc  several problems per launch, 256x128 tiles for the grouped weight gradients, slab reductions
// Variants of the NT kernels: F16 (IEEE fp16 operands on v_mfma_f32_16x16x32_f16, fp16 / bf16-copy outputs: the "mixed16"
// forward GEMMs) and CONV (gemm_ws_kernel only: the A tile is gathered from an NHWC activation = implicit 3x3 convolution).
// LDS images are XOR-swizzled per layout (off_kc / off_km), the swizzle applied to the DMA source address.
// Kernels in this file:
//   gemm_kernel            general path: any M, N, K / ragged / unaligned operands, register-staged, split-K
//   scale_c_kernel         C *= beta ahead of a split-K launch
#include "gemm_core.h"
#include <cstdio>
#include <cstdlib>

namespace {

// Issue the global loads of k-tile kt for both operands (second reduction segment after K1, if any).
template <bool A_KM, bool B_KM, bool ALIGNED>
__device__ __forceinline__ void fetch_tiles(const GemmArgs& g, int kt, int m0, int n0, int tid, u32x4 (&ra)[4],
                                            u32x4 (&rb)[4]) {
    int k0 = kt * BK;
    const bf16_t* Ap = g.A; int64_t la = g.lda;
    const bf16_t* Bp = g.B; int64_t lb = g.ldb;
    int klim = g.K1 > 0 ? g.K1 : g.K;
    if (g.K1 > 0 && k0 >= g.K1) {
        Ap = g.A2; la = g.lda2; Bp = g.B2; lb = g.ldb2;
        k0 -= g.K1; klim = g.K - g.K1;
    }
    g2r<A_KM, ALIGNED>(ra, Ap, la, m0, g.M, k0, klim, tid, g.a_vec);
    g2r<B_KM, ALIGNED>(rb, Bp, lb, n0, g.N, k0, klim, tid, g.b_vec);
}

template <bool A_KM, bool B_KM, bool ALIGNED, bool F16 = false>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmArgs gp) {
    const GemmArgs g = gp;  // local copy: lets SROA scalarise the descriptor instead of spilling the kernarg struct
    __shared__ __attribute__((aligned(16))) char smem[4 * TILE_BYTES];  // [2 buffers][A tile | B tile]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;

    // XCD-aware tile order: blocks b and b+8 share an XCD (round-robin dispatch), so give each XCD a contiguous
    // run of tiles (same A row panel, neighbouring B panels) -> its private L2 sees the panel re-use.
    const int nbn = (g.N + BN - 1) / BN;
    const int nb = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, qn = nb >> 3, rn = nb & 7;
    const int sw = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + (bid >> 3);
    const int m0 = (sw / nbn) * BM, n0 = (sw % nbn) * BN;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk_all = (g.K + BK - 1) / BK;
    // split-K (skinny outputs with a long reduction): blockIdx.y owns a contiguous range of k-tiles
    const int per = (nk_all + g.ksplit - 1) / g.ksplit;
    const int kt0 = blockIdx.y * per;
    const int nk = (kt0 + per < nk_all ? kt0 + per : nk_all) - kt0;
    if (nk <= 0) return;
    u32x4 ra[4], rb[4];

    fetch_tiles<A_KM, B_KM, ALIGNED>(g, kt0, m0, n0, tid, ra, rb);
    r2s<A_KM>(ra, smem, tid);
    r2s<B_KM>(rb, smem + TILE_BYTES, tid);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const char* sA = smem + (kt & 1) * 2 * TILE_BYTES;
        const char* sB = sA + TILE_BYTES;
        if (kt + 1 < nk) fetch_tiles<A_KM, B_KM, ALIGNED>(g, kt0 + kt + 1, m0, n0, tid, ra, rb);  // under the MFMAs
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 fa[4], fb[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) fa[t] = read_frag<A_KM>(sA, wr + 16 * t, ks, lane);
#pragma unroll
            for (int t = 0; t < 4; ++t) fb[t] = read_frag<B_KM>(sB, wc + 16 * t, ks, lane);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = mfma16t<F16>(fb[ni], fa[mi], acc[mi][ni]);
        }
        if (kt + 1 < nk) {
            char* dA = smem + ((kt + 1) & 1) * 2 * TILE_BYTES;
            r2s<A_KM>(ra, dA, tid);
            r2s<B_KM>(rb, dA + TILE_BYTES, tid);
        }
        __syncthreads();
    }

    // D^T layout: lane holds C[m = .. + (lane&15)][n = .. + 4*(lane>>4) + r]
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int m = m0 + wr + 16 * mi + (lane & 15);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int n = n0 + wc + 16 * ni + 4 * (lane >> 4);
            if (m < g.M && n < g.N) epilogue4(g, m, n, acc[mi][ni]);
        }
    }
}

__global__ void scale_c_kernel(float* C, int64_t ldc, int M, int N, float beta) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)M * N) return;
    const int64_t r = i / N;
    float* p = C + r * ldc + (i - r * N);
    *p = beta == 0.f ? 0.f : *p * beta;
}

#ifdef ICKA_GEMM_STAMP
static unsigned long long* g_stamp = nullptr;   // diagnostic build only: per-segment cycle sums (icka_diag_gemm_stamp_buffer)
#endif
inline bool vec_ok(const void* p, int64_t ld) { return (ld % 8 == 0) && ((reinterpret_cast<uintptr_t>(p) & 15) == 0); }

}  // namespace

static int tune_env_int(const char* name, int dflt, int lo, int hi) {
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    const int v = atoi(e);
    return v < lo || v > hi ? dflt : v;
}
static const Tune kTuneEnv = [] {
    Tune t;
    t.abl = tune_env_int("ICKA_TUNE_GEMM_ABLATION", 0, 0, 3);
    t.ws = tune_env_int("ICKA_TUNE_GEMM_WARP_SPECIALIZED", 1, 0, 3);
    t.direct = tune_env_int("ICKA_TUNE_GEMM_DIRECT_EPILOGUE", 1, 0, 1);
    t.w3 = tune_env_int("ICKA_TUNE_GEMM_WIDE_TILES", 1, 0, 1);
    t.bn = tune_env_int("ICKA_TUNE_GEMM_TILE_N", 0, 0, 128);
    if (t.bn != 0 && t.bn != 96 && t.bn != 128) t.bn = 0;
    t.nbuf = tune_env_int("ICKA_TUNE_GEMM_RING", 0, 0, 5);
    if (t.nbuf == 1) t.nbuf = 0;
    t.w3grid = tune_env_int("ICKA_TUNE_GEMM_W3_GRID", 0, 0, 8);
    if (t.w3grid != 0 && t.w3grid != 1 && t.w3grid != 2 && t.w3grid != 4 && t.w3grid != 8) t.w3grid = 0;
    t.big = tune_env_int("ICKA_TUNE_GEMM_BIG_TILES", 2, 0, 2);
    return t;
}();
// icka_gemm_desc.tune (include/icka_hip.h, ICKA_TUNE_*): 4 bits per field, 0 = keep the default, else the field's code.
// Returns false for a code outside a field's range (-> ICKA_E_ARG).
static bool tune_of(uint64_t bits, Tune& t) {
    t = kTuneEnv;
    if (!bits) return true;
    const int ring = (int)(bits & 15), tile = (int)((bits >> 4) & 15), wide = (int)((bits >> 8) & 15), dir = (int)((bits >> 12) & 15),
              ws = (int)((bits >> 16) & 15), grid = (int)((bits >> 20) & 15), big = (int)((bits >> 24) & 15), abl = (int)((bits >> 28) & 15);
    if (bits >> 32) return false;
    if (ring) { if (ring < 2 || ring > 5) return false; t.nbuf = ring; }
    if (tile) { if (tile > 2) return false; t.bn = tile == 1 ? 96 : 128; }
    if (wide) { if (wide > 2) return false; t.w3 = wide - 1; }
    if (dir) { if (dir > 2) return false; t.direct = dir - 1; }
    if (ws) { if (ws > 4) return false; t.ws = ws - 1; }
    if (grid) { if (grid != 1 && grid != 2 && grid != 4 && grid != 8) return false; t.w3grid = grid; }
    if (big) { if (big > 3) return false; t.big = big - 1; }
    if (abl) { if (abl > 3) return false; t.abl = abl; }
    return true;
}

#ifdef ICKA_GEMM_STAMP
// diagnostic builds only (tools/gemm_stamp.py): device buffer of [blocks][8] u64 receiving per-segment cycle sums
extern "C" int icka_diag_gemm_stamp_buffer(void* p) {
    g_stamp = (unsigned long long*)p;
    return 0;
}
#endif

// Diagnostic site classes of the per-site store-policy matrix (profiles/r04_store_policy_matrix.txt): which producer of a
// BERT layer a launch is, from its op / epilogue / shape ratio (N, K in units of H = min(N, K) work for bert-base and -large).
//   bit 0 QKV (NT, N = 3H)            -> attention          bit 4 d(ffn-down) dgrad (NN, N = 4H, GELU' epilogue) -> d(ffn-up), wgrad
//   bit 1 out-proj (NT, N = K)        -> LayerNorm          bit 5 d(ffn-up) dgrad   (NN, K = 4N)               -> LayerNorm bwd
//   bit 2 ffn-up + GELU (NT, N = 4K)  -> ffn-down           bit 6 d(out-proj) dgrad (NN, N = K)                -> attention bwd
//   bit 3 ffn-down (NT, K = 4N)       -> LayerNorm          bit 7 d(QKV) dgrad      (NN, K = 3N)               -> LayerNorm bwd
static int site_bit(const icka_gemm_desc* d) {
    const int64_t N = d->N, K = d->K;
    if (d->c_is_f32 == 1 || d->M < 1024) return -1;
    if (d->op == ICKA_GEMM_NT) {
        if (N == 3 * K) return 0;
        if (N == K) return 1;
        if (N == 4 * K) return 2;
        if (K == 4 * N) return 3;
    } else if (d->op == ICKA_GEMM_NN) {
        if (N == 4 * K) return 4;
        if (K == 4 * N) return 5;
        if (N == K) return 6;
        if (K == 3 * N) return 7;
    }
    return -1;
}
static int plain_mask() {
    static int m = -1;
    if (m < 0) {
        const char* e = getenv("ICKA_GEMM_PLAIN_MASK");
        m = e ? (int)strtol(e, nullptr, 0) : 0;
    }
    return m;
}

static int convert(const icka_gemm_desc* d, GemmArgs& g, bool& aligned, Tune& t) {
    if (!d || !d->A || !d->B || !d->C) return ICKA_E_ARG;
    if (!tune_of(d->tune, t)) return ICKA_E_ARG;
    if (d->M <= 0 || d->N <= 0 || d->K <= 0) return ICKA_E_SHAPE;
    if (d->op < ICKA_GEMM_NT || d->op > ICKA_GEMM_TN) return ICKA_E_ARG;
    if (d->K1 != 0 && (d->K1 < 0 || d->K1 >= d->K || d->K1 % BK != 0 || !d->A2 || !d->B2)) return ICKA_E_ARG;
    if ((d->epilogue == ICKA_EPI_GELU) && !d->C2) return ICKA_E_ARG;
    if ((d->epilogue == ICKA_EPI_DGELU || d->epilogue == ICKA_EPI_ADD || d->epilogue == ICKA_EPI_GATE ||
         d->epilogue == ICKA_EPI_ADD_RELU) && !d->aux)
        return ICKA_E_ARG;
    g.M = d->M; g.N = d->N; g.K = d->K; g.K1 = d->K1;
    g.A = (const bf16_t*)d->A; g.lda = d->lda; g.B = (const bf16_t*)d->B; g.ldb = d->ldb;
    g.A2 = (const bf16_t*)d->A2; g.lda2 = d->lda2; g.B2 = (const bf16_t*)d->B2; g.ldb2 = d->ldb2;
    g.C = d->C; g.ldc = d->ldc; g.C2 = (bf16_t*)d->C2; g.ldc2 = d->ldc2;
    g.aux = (const bf16_t*)d->aux; g.ldaux = d->ldaux; g.bias = d->bias; g.bias2 = d->bias2;
    g.alpha = d->alpha; g.beta = d->beta; g.epi = d->epilogue;
    if (d->c_is_f32 < 0 || d->c_is_f32 > 2) return ICKA_E_ARG;
    g.c_f32 = d->c_is_f32 == 1; g.c_f16 = d->c_is_f32 == 2;
    g.f16 = d->ab_f16 != 0; g.C3 = (bf16_t*)d->C3; g.ldc3 = d->ldc3; g.aux_f16 = d->aux_f16 != 0;
    if (g.f16 && d->op != ICKA_GEMM_NT) return ICKA_E_ARG;       // fp16 operands: forward (NT) GEMMs only
    if (g.c_f16 && d->beta != 0.f) return ICKA_E_ARG;              // fp16 outputs are never accumulated into
    if (g.C3 && !g.c_f16 && !g.c_f32) return ICKA_E_ARG;           // C3 = bf16 twin of an fp16 or an f32 main output
    // the wire copy of an f32 output is compiled into the weight-gradient (TN) instances of the fast paths only: any other
    // op would return 0 and leave the wire buffer stale
    if (g.C3 && g.c_f32 && d->op != ICKA_GEMM_TN) return ICKA_E_ARG;
    g.c3_only = d->c3_only != 0;
    {
        const int sb = site_bit(d);
        g.plain = (sb >= 0 && ((plain_mask() >> sb) & 1)) ? 1 : 0;
    }
    if (g.c3_only && !(g.C3 && g.c_f32 && d->beta == 0.f && d->epilogue == ICKA_EPI_NONE)) return ICKA_E_ARG;
    if (g.c_f16 && d->colsum_out) return ICKA_E_ARG;
    g.abl = t.abl;
    g.stamp = nullptr;
#ifdef ICKA_GEMM_STAMP
    g.stamp = g_stamp;
    {   // diagnostic builds: ICKA_GEMM_STAMP_FILTER="op,N,K" stamps only that shape (all GEMMs share one buffer)
        static int f_op = -2, f_n = 0, f_k = 0;
        if (f_op == -2) {
            f_op = -1;
            if (const char* e = getenv("ICKA_GEMM_STAMP_FILTER")) sscanf(e, "%d,%d,%d", &f_op, &f_n, &f_k);
        }
        if (f_op >= 0 && !(d->op == f_op && d->N == f_n && d->K == f_k)) g.stamp = nullptr;
    }
#endif
    g.colsum = d->colsum_out;
    g.colsum_acc = d->colsum_accumulate;
    g.ksplit = 1;
    g.n96ok = 0;
    g.n64ok = 0;
    g.direct = t.direct;
    g.a_vec = vec_ok(d->A, d->lda) && (d->K1 == 0 || vec_ok(d->A2, d->lda2));
    g.b_vec = vec_ok(d->B, d->ldb) && (d->K1 == 0 || vec_ok(d->B2, d->ldb2));
    auto al = [](const void* p, int64_t ld, int64_t mod) {
        return !p || (((reinterpret_cast<uintptr_t>(p) & 15) == 0) && ld % mod == 0);
    };
    if (d->colsum_out && d->op != ICKA_GEMM_TN) return ICKA_E_ARG;
    // whole tiles of 128 x (a multiple of nmod) x 64 and every operand readable / writable with 16-byte accesses
    auto tiles_ok = [&](int nmod) {
        return (d->M % BM == 0) && (d->N % nmod == 0) && (d->K % BK == 0) && g.a_vec && g.b_vec &&
               al(d->C, d->ldc, d->c_is_f32 == 1 ? 4 : 8) && al(d->C2, d->ldc2, 8) && al(d->aux, d->ldaux, 8) &&
               al(d->bias, 4, 4) && al(d->bias2, 4, 4) && al(d->C3, d->ldc3, 8);
    };
    aligned = tiles_ok(BN);
    g.n96ok = aligned && d->N % 96 == 0;
    g.n64ok = !aligned && tiles_ok(64) && d->K1 == 0 && !d->colsum_out;
    return 0;
}


// The kernel families.  They are source FRAGMENTS of this translation unit (extern "C" entry points, file-scope statics: each
// is included exactly once, here), and one unit on purpose: as five units the same sources gave other machine code for 42 of
// the 89 kernels -- other register and spill counts in 23 of them: the code hipcc makes of an inline helper depends on which
// other kernels of the unit call it -- and a 1 % slower c2 step; as one unit every kernel whose source only moved is the
// parent's, instruction for instruction (profiles/gemm_split_isa.txt, profiles/gemm_split.txt, tools/code_object_diff.py).
#include "gemm_ws.inc"
#include "gemm_w3.inc"
#include "gemm_fused.inc"
#include "gemm_grouped.inc"

namespace {

// "launch this instantiation on this grid, check, return" for the arms of the ladder
#define LAUNCH_RETURN(KERNEL, GRID, BLOCK) ICKA_LAUNCH_RETURN(KERNEL, GRID, BLOCK, st, g)

// a_live (icka_gemm_live): row-liveness bytes of A, or null.  Two arms of the ladder have a LIVE instance (NN, bf16: the 256x192
// and the 128x96 ring-of-3 kernels, the input-gradient GEMMs of the encoder backward); every other arm ignores the flags.
template <bool A_KM, bool B_KM, bool F16 = false>
int launch(GemmArgs g, bool aligned, hipStream_t st, const Tune& t, const uint8_t* a_live = nullptr) {
    constexpr bool LIVE_OK = !A_KM && B_KM && !F16;
    const int nb = ((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN);
    if constexpr (!A_KM && !B_KM) {
        if (!aligned && g.n64ok && t.ws)   // 64-channel convolutions of the ResNet stem / layer1: 128x64 tiles
            LAUNCH_RETURN((gemm_ws_kernel<false, false, 3, 0, 64, F16>), (g.M / BM) * (g.N / 64), 512);
    }
    if (aligned) {
#ifdef ICKA_GEMM_ABLATE
        if (t.abl == 1 && !t.ws) LAUNCH_RETURN((gemm_dma_kernel<A_KM, B_KM, 3, 1>), nb, 256);
        else if (t.abl == 2 && !t.ws) LAUNCH_RETURN((gemm_dma_kernel<A_KM, B_KM, 3, 2>), nb, 256);
        else
#endif
        {
            // ring depth: many tiles per CU -> two co-resident blocks (64 KiB ring of 2) overlap one block's
            // epilogue with the other's main loop; few tiles -> one block per CU with a deeper ring (measured,
            // tools/gemm_bench.py)
            if (t.ws || F16) {   // (fp16 operands exist on the warp-specialised kernels only)
#ifdef ICKA_GEMM_ABLATE
                if (t.bn == 96 && g.n96ok) {   // the 128x96-tile kernel (ICKA_TUNE_TILE_N(96))
                    const int nb96 = (g.M / BM) * (g.N / 96);
                    if (t.abl == 1) LAUNCH_RETURN((gemm_ws_kernel<A_KM, B_KM, 3, 1, 96>), nb96, 512);
                    if (t.abl == 2) LAUNCH_RETURN((gemm_ws_kernel<A_KM, B_KM, 3, 2, 96>), nb96, 512);
                    if (t.abl == 3) LAUNCH_RETURN((gemm_ws_kernel<A_KM, B_KM, 3, 3, 96>), nb96, 512);
                }
                if (t.abl == 1) LAUNCH_RETURN((gemm_ws_kernel<A_KM, B_KM, 3, 1>), nb, 512);
                if (t.abl == 2) LAUNCH_RETURN((gemm_ws_kernel<A_KM, B_KM, 3, 2>), nb, 512);
#endif
                // 256x192 tiles (12-wave kernel) where they cover the CUs in ONE round: wide outputs with a short reduction
                if constexpr (!A_KM) {
                    const int nb3 = (g.M / 256) * (g.N / 192);
                    // ... or in whole rounds: at least 3/4 of the last round of 256 must be filled
                    const int rounds3 = (nb3 + 255) / 256;
                    if (t.w3 && g.M % 256 == 0 && g.N % 192 == 0 && g.K <= 1024 && g.K1 == 0 && nb3 % 8 == 0 &&
                        nb3 >= 128 && 4 * nb3 >= 3 * 256 * rounds3 && g.ksplit == 1) {
                        w3_set_grid(g, 192, t.w3grid);
                        if constexpr (LIVE_OK) {
                            if (a_live) {
                                hipLaunchKernelGGL(gemm_w3_live_kernel, dim3(nb3), dim3(768), 0, st, g, a_live);
                                ICKA_CHECK_LAUNCH();
                                return 0;
                            }
                        }
                        LAUNCH_RETURN((gemm_w3_kernel<B_KM, F16>), nb3, 768);
                    }
                    // 256x128 tiles (the same kernel, 64-column halves) where 128x128 tiles would take exactly two rounds of
                    // the CUs with one block each (N = 1024 at bert-large / M = 8192: 256 tiles), any K
                    const int nb2 = (g.M / 256) * (g.N / 128);
                    if (t.w3 && g.M % 256 == 0 && g.K1 == 0 && g.ksplit == 1 && nb2 % 8 == 0 && nb2 >= 192 && nb2 <= 256 &&
                        !(g.n96ok && t.bn == 96) && !(g.K <= 1024 && g.direct && g.c_f32 && g.epi == ICKA_EPI_NONE && g.beta == 0.f)) {
                        // (short reductions with a plain f32 output stay on the 128-wide kernel: its direct epilogue beats
                        //  the two staged passes here, 25.9 vs 28.3 us at 8192 x 1024 x 1024)
                        w3_set_grid(g, 128, t.w3grid);
                        LAUNCH_RETURN((gemm_w3_kernel<B_KM, F16, 128>), nb2, 768);
                    }
                }
                // Tile width: 128x96 tiles when they quantise better onto the 256 CUs (N = 768: 256 tiles instead of 192).
                if (g.n96ok && t.bn != 128) {
                    // measured (profiles/README.md): a 128x96 tile costs ~0.9-1.0 of a 128x128 one (the k-loop is bound
                    // by LDS / L1 traffic of the A tile, not by MFMA count), so the narrow tile only pays where it turns
                    // an under-filled single round into a full one
                    const int nb96 = (g.M / BM) * (g.N / 96);
                    if (t.bn == 96 || (nb < 256 && nb96 <= 256 && nb96 > nb)) {
                        if ((t.ws == 2 || (t.ws == 1 && nb96 >= 448 && g.K <= 1024)) && !A_KM)
                            LAUNCH_RETURN((gemm_ws2_kernel<A_KM, B_KM, 96, F16>), nb96, 512);
                        else if (t.nbuf == 4 && !F16) LAUNCH_RETURN((gemm_ws_kernel<A_KM, B_KM, 4, 0, 96>), nb96, 512);
                        else if (t.nbuf == 5 && !F16) LAUNCH_RETURN((gemm_ws_kernel<A_KM, B_KM, 5, 0, 96>), nb96, 512);
                        else if (LIVE_OK && a_live) {
                            if constexpr (LIVE_OK) hipLaunchKernelGGL(gemm_ws_live_kernel<96>, dim3(nb96), dim3(512), 0, st, g, a_live);
                            ICKA_CHECK_LAUNCH();
                            return 0;
                        }
                        else LAUNCH_RETURN((gemm_ws_kernel<A_KM, B_KM, 3, 0, 96, F16>), nb96, 512);
                    }
                }
                // measured (tools/gemm_bench.py): two co-resident blocks win only for short reductions on grids of
                // >= ~2 tiles per CU (qkv, ffn-up, d-ffn-down); long-K shapes prefer the deeper ring of one block
                if ((t.ws == 2 || (t.ws == 1 && nb >= 448 && g.K <= 1024)) && !A_KM)
                    LAUNCH_RETURN((gemm_ws2_kernel<A_KM, B_KM, 128, F16>), nb, 512);
                else if (t.nbuf == 4 && !F16) LAUNCH_RETURN((gemm_ws_kernel<A_KM, B_KM, 4>), nb, 512);
                else if (t.nbuf == 5 && !F16) LAUNCH_RETURN((gemm_ws_kernel<A_KM, B_KM, 5>), nb, 512);
                else LAUNCH_RETURN((gemm_ws_kernel<A_KM, B_KM, 3, 0, 128, F16>), nb, 512);
            }
            const int nbuf = t.nbuf > 0 ? t.nbuf : (nb >= 448 ? 2 : 4);
            if (nbuf == 2) LAUNCH_RETURN((gemm_dma_kernel<A_KM, B_KM, 2, 0>), nb, 256);
            else if (nbuf == 3) LAUNCH_RETURN((gemm_dma_kernel<A_KM, B_KM, 3, 0>), nb, 256);
            else LAUNCH_RETURN((gemm_dma_kernel<A_KM, B_KM, 4, 0>), nb, 256);
        }
    } else {
        // skinny output + long reduction (classifier weight gradient: 13 x 768 x 4096 tokens): split K over
        // blockIdx.y and accumulate f32 partial tiles atomically (C is scaled by beta / zeroed first)
        const int nk = (g.K + BK - 1) / BK;
        int ks = 1;
        // (TN with M <= 256 only: weight-gradient shapes.  Forward outputs such as the [tokens, labels] emissions stay on one
        //  block per tile so that two identical calls give bitwise identical logits -- atomic split-K order flipped
        //  Viterbi near-ties between a 'dev' and a 'test' pass of the same batch.  M <= 256 alone is not that rule: an NT
        //  forward GEMM of a few ROWS -- [batch, 1024] x [1024, 1024] with f32 output at eval batch 2 or 3 -- met it too, and
        //  its 4 atomically added partials made the dev loss of a replayed capture differ from the eager one in the last bits.)
        if (A_KM && B_KM && g.c_f32 && g.epi == ICKA_EPI_NONE && nb < 64 && nk >= 16 && g.M <= 256 && !g.C3) {   // (a wire copy needs the final value in one epilogue)
            ks = 256 / nb;
            if (ks > nk / 4) ks = nk / 4;
            if (ks < 1) ks = 1;
        }
        if (ks > 1) {
            const int64_t n = (int64_t)g.M * g.N;
            hipLaunchKernelGGL(scale_c_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                               reinterpret_cast<float*>(g.C), g.ldc, g.M, g.N, g.beta);
            ICKA_CHECK_LAUNCH();
            g.beta = 0.f;
            g.ksplit = ks;
        }
        LAUNCH_RETURN((gemm_kernel<A_KM, B_KM, false, F16>), dim3(nb, ks), 256);
    }
}
#undef LAUNCH_RETURN

}  // namespace

extern "C" int icka_gemm(const icka_gemm_desc* d, void* stream) {
    GemmArgs g;
    Tune t;
    bool aligned = false;
    const int rc = convert(d, g, aligned, t);
    if (rc) return rc;
    if (g.colsum && !(aligned && t.ws)) return ICKA_E_ARG;   // fused column sums exist on the warp-specialised path
    hipStream_t st = (hipStream_t)stream;
    if (g.f16) return launch<false, false, true>(g, aligned, st, t);
    switch (d->op) {
        case ICKA_GEMM_NT: return launch<false, false>(g, aligned, st, t);
        case ICKA_GEMM_NN: return launch<false, true>(g, aligned, st, t);
        default: return launch<true, true>(g, aligned, st, t);
    }
}

// icka_gemm with row-liveness flags of the A operand (include/icka_hip.h).  The flags are a permission: a launch whose kernel has
// no LIVE instance, or a null pointer, is exactly icka_gemm.
extern "C" int icka_gemm_live(const icka_gemm_desc* d, const uint8_t* a_row_live, void* stream) {
    if (!a_row_live) return icka_gemm(d, stream);
    if (reinterpret_cast<uintptr_t>(a_row_live) & 15) return ICKA_E_ALIGN;
    GemmArgs g;
    Tune t;
    bool aligned = false;
    const int rc = convert(d, g, aligned, t);
    if (rc) return rc;
    if (d->op != ICKA_GEMM_NN && d->op != ICKA_GEMM_NT) return ICKA_E_ARG;   // (flags are per ROW of a row-major A)
    if (d->op != ICKA_GEMM_NN || g.f16 || g.K1 != 0 || !aligned || !t.ws || t.abl) return icka_gemm(d, stream);
    return launch<false, true>(g, aligned, (hipStream_t)stream, t, a_row_live);
}
