// The 12-wave kernels (8 compute + 4 loader waves; gemm_core.h; DESIGN.md section 4).  Kernels in this file:
//   gemm_w3_kernel         256x192 tiles (wide short-K outputs: qkv, ffn-up, d-ffn-down) or 256x128 tiles (N = 1024 / 768 at
//                          M = 8192: one round of 192..256 tiles instead of two); NT / NN, bf16 or (NT) fp16 operands
//   gemm_w3_live_kernel    the NN 256x192 instance with row-liveness flags of A (icka_gemm_live); both share gemm_w3_body.inc
//   gemm_qkv_attn_kernel   the same k-loop over one head's q | k | v columns + the whole-head attention forward in the epilogue
// A source fragment of gemm.hip, included once there.
#include "attn_core.h"

namespace {

// =====================================================================================================================
// 256 x 192 output tiles, 12 waves (8 compute waves of 64 x 96 + 4 loader waves), for the wide-output / short-K GEMMs of
// the step (qkv: 4096 x 2304, ffn-up and d(ffn-down): 4096 x 3072, K = 768): 192 / 256 tiles = ONE round of the 256 CUs
// instead of 2.25 / 3 rounds of 128 x 128 tiles, and 0.75x the operand bytes per FLOP through L2 -> LDS (the in-step
// limiter, DESIGN.md section 5).  Two compute waves per SIMD cover each other's LDS latency (fragments are read per
// 32-deep step right before their MFMAs, as in the two-blocks-per-CU kernel); LDS ring of 2 stages of
// [A rows 0..127 | A rows 128..255 | B 0..95 | B 96..191] (4 x 16 KiB images in the usual swizzled layouts); outputs go
// straight from the accumulators through the general 4-column epilogue.  A is k-contiguous (NT and NN).
constexpr int W3_A = 2 * TILE_BYTES, W3_B = 2 * TILE_BYTES;   // one k-tile of A (2 x 128 rows) / of B (2 x 96 columns)
constexpr int W3_NA = 3, W3_NB = 2;                           // ring depths: 3 x 32 KiB + 2 x 32 KiB = 160 KiB = the whole LDS
// tile of block ``bid`` of the 12-wave kernel.  Blocks b and b+8 share an XCD (and its private 4 MiB L2), and the nb / 8
// tiles an XCD works on at the same time decide what it has to fetch: a pm x pn cut of the tile grid over the XCDs makes the
// chip fetch pn * |A| + pm * |B| (every XCD needs the A row panels and the B column panels of its patch).  The host picks the
// cut (gemm_w3_grid: the dividing one with the smallest pn * M + pm * N; 8 x 1 = the row-major runs of rounds 1-2) and passes
// sn = column tiles per patch and log2(pn): ffn-up 4 x 2 (31.5 MB instead of 44 MB at c2), the M = 8192 x N = 1024 shapes of
// c4 stay 8 x 1.
__device__ __forceinline__ void w3_origin(int bid, int sn, int pnlog, int bnw, int& m0, int& n0) {
    const int xcd = bid & 7, li = bid >> 3;
    const int xi = xcd >> pnlog, xj = xcd & ((1 << pnlog) - 1);
    const int r = li / sn, c = li - r * sn;
    // sm = rows of tiles per patch = (nb / 8) / sn, implied: patch xi starts at row xi * sm
    m0 = (xi * ((int)(gridDim.x >> 3) / sn) + r) * 256;
    n0 = (xj * sn + c) * bnw;
}

// one k-tile of A / of B into ring slot SLOT (both 12-wave kernels: the loader wave's pa0 / pa1 / pb0 / pb1, strides sa / sb;
// NJB = 1-KiB pieces per B image and loader wave, a constant of the kernel)
#define ICKA_W3_A(SLOT)                                                          \
    do {                                                                         \
        dma_issue(pa0, sa, lds0 + (SLOT) * W3_A + lw * 1024);                    \
        dma_issue(pa1, sa, lds0 + (SLOT) * W3_A + TILE_BYTES + lw * 1024);       \
    } while (0)
#define ICKA_W3_B(SLOT)                                                          \
    do {                                                                         \
        dma_issue<NJB>(pb0, sb, ldsB + (SLOT) * W3_B + lw * 1024);               \
        dma_issue<NJB>(pb1, sb, ldsB + (SLOT) * W3_B + TILE_BYTES + lw * 1024);  \
    } while (0)
// The body of both kernels is the text of gemm_w3_body.inc (see there why it is not a function).
template <bool B_KM, bool F16 = false, int BNW = 192>
__global__ __launch_bounds__(768) void gemm_w3_kernel(const GemmArgs gp) {
    constexpr bool LIVE = false;
    const uint8_t* const a_live = nullptr;
#include "gemm_w3_body.inc"
}

// the NN kernel on 256 x 192 tiles with row-liveness flags of A (icka_gemm_live)
__global__ __launch_bounds__(768) void gemm_w3_live_kernel(const GemmArgs gp, const uint8_t* a_live) {
    constexpr bool B_KM = true, F16 = false, LIVE = true;
    constexpr int BNW = 192;
#include "gemm_w3_body.inc"
}

// =====================================================================================================================
// QKV projection + self-attention of a head in ONE launch (sequence length 128, head size 64 -- the reference's
// max_seq_length 128 text: BertSelfAttention.forward, Cross_Modal_Interaction_Module.py:478-506).
// The 12-wave kernel's 256 x 192 tile is laid over the problem so that its 192 columns are the 64 query, 64 key and 64 value
// columns of ONE head (B rows head*64 .. +63 of each of the three stacked weight blocks: only the loader's row pointers change)
// and its 256 rows are TWO samples: after the k-loop the block holds everything the attention of those two (sample, head) pairs
// needs.  Epilogue: accumulators + bias -> bf16 -> six [128][64] off_t images in the dead operand ring (q, k, v of either sample);
// then the four loader waves stream the images to the qkv activation (the attention backward and the weight gradient read it
// later) while the eight compute waves run the whole-head attention forward of attn_core.h straight from the images -- 32 queries
// per wave -- and store context rows and log-sum-exp.  Same bf16 q / k / v, same device function: bit for bit the result of
// icka_gemm + icka_attn_fwd, without the attention launch, its 19 MB re-read of qkv and the kernel boundary between them.
struct QkvAttnArgs { GemmArgs g; AttnArgs a; };

template <int HALF>
__device__ __forceinline__ void dma_init_qkv(const bf16_t* (&ptr)[4], const bf16_t* __restrict__ P, int64_t ld, int head, int H,
                                             int wave, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = wave + 4 * j;                 // (piece 3 of a 96-row image is never issued)
        const int row = (8 * p + (lane >> 3)) % 96;
        const int lc = (lane & 7) ^ ((row >> 1) & 7);
        const int r = 96 * HALF + row;              // tile column 0..191 = [q | k | v] of the head
        ptr[j] = P + (int64_t)((r >> 6) * H + head * 64 + (r & 63)) * ld + 8 * lc;
    }
}

// SEQ = tokens per sample: 128 (the tile's 256 rows = two samples, 32 queries per compute wave in one pass) or 256 (one sample,
// bert-large at BASELINE config c4: 32 queries per wave as two passes of 16 against the 256 keys).  F16: fp16 operands of the
// projection (the "mixed16" forward GEMMs; q / k / v stay bf16).  KB: the attention leaves its keep bits (SEQ = 256 only).
template <bool DROP, bool F16, int SEQ, bool KB>
__global__ __launch_bounds__(768) void gemm_qkv_attn_kernel(const QkvAttnArgs p) {
    static_assert(SEQ == 128 || SEQ == 256, "tokens per sample");
    const GemmArgs g = p.g;
    __shared__ __attribute__((aligned(16))) char smem[W3_NA * W3_A + W3_NB * W3_B];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)reinterpret_cast<uintptr_t>(LDS_PTR(char, smem)));
    constexpr int BH = 96, NB16 = 6;
    int m0, n0;
    w3_origin(blockIdx.x, g.w3_sn, g.w3_pnlog, 192, m0, n0);
    const int head = n0 / 192, H = g.N / 3;
    const int nk = g.K / BK;
    if (wave >= 8) {
        // loader waves: gemm_w3_kernel's ring (A two k-tiles ahead in a ring of 3, B one ahead in a ring of 2)
        const int lw = wave - 8;
        const bf16_t* pa0[4];
        const bf16_t* pa1[4];
        const bf16_t* pb0[4];
        const bf16_t* pb1[4];
        dma_init<false>(pa0, g.A, g.lda, m0, lw, lane);
        dma_init<false>(pa1, g.A, g.lda, m0 + 128, lw, lane);
        dma_init_qkv<0>(pb0, g.B, g.ldb, head, H, lw, lane);
        dma_init_qkv<1>(pb1, g.B, g.ldb, head, H, lw, lane);
        const int64_t sa = BK, sb = BK;
        constexpr int NJB = 3;   // (a B image is 96 rows)
        const uint32_t ldsB = lds0 + W3_NA * W3_A;
        ICKA_W3_A(0);
        ICKA_W3_B(0);
        if (nk > 1) ICKA_W3_A(1);
        int sa3 = 2;
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + 1 < nk) wait_vmcnt<8>(); else wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
            if (kt + 1 < nk) ICKA_W3_B((kt + 1) & 1);
            if (kt + 2 < nk) ICKA_W3_A(sa3);
            sa3 = sa3 == 2 ? 0 : sa3 + 1;
        }
    }
    const int wr = (wave >> 1) * 64, wc = (wave & 1) * BH;
    f32x4 acc[4][NB16];
    if (wave < 8) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NB16; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kt = 0; kt < nk; ++kt) {
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            const char* sA = smem + (kt % W3_NA) * W3_A + (wr >> 7) * TILE_BYTES;
            const char* sB = smem + W3_NA * W3_A + (kt & 1) * W3_B + (wave & 1) * TILE_BYTES;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 fa[4], fb[NB16];
#pragma unroll
                for (int t = 0; t < 4; ++t) fa[t] = read_frag<false>(sA, (wr & 127) + 16 * t, ks, lane);
#pragma unroll
                for (int t = 0; t < NB16; ++t) fb[t] = read_frag<false>(sB, 16 * t, ks, lane);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NB16; ++ni) acc[mi][ni] = mfma16t<F16>(fb[ni], fa[mi], acc[mi][ni]);
            }
        }
        asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");   // MFMA -> VALU read wait states
    }
    __syncthreads();   // the operand ring is dead: it becomes the bf16 images [SEQ][64] of q, k, v (of either sample): smem + (3 s + mat) * IMG
    constexpr int IMG = SEQ * 128;
    if (wave < 8) {
        const int s = SEQ == 128 ? wave >> 2 : 0;
#pragma unroll
        for (int ni = 0; ni < NB16; ++ni) {
            const int c0 = wc + 16 * ni + 4 * (lane >> 4);   // tile column of this lane's four accumulator columns
            const int mat = c0 >> 6, cc = c0 & 63;
            const f32x4 bv = *reinterpret_cast<const f32x4*>(g.bias + mat * H + head * 64 + cc);
            char* im = smem + (3 * s + mat) * IMG;
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int r = (wr & (SEQ - 1)) + 16 * mi + (lane & 15);
                const f32x4 v = acc[mi][ni] + bv;
                *reinterpret_cast<u32x2*>(im + off_t(r, cc >> 3) + 8 * ((cc >> 2) & 1)) = pack4(v[0], v[1], v[2], v[3]);
            }
        }
    }
    __syncthreads();
    if (wave >= 8) {
        // the qkv activation for the backward: 256 rows x 3 matrices x 8 chunks of 16 B, 24 per loader thread; a row's 64 columns
        // (128 B) are contiguous in global memory
        bf16_t* C = reinterpret_cast<bf16_t*>(g.C);
        const int t = tid - 512;
#pragma unroll 4
        for (int i = 0; i < 24; ++i) {
            const int id = t + 256 * i;
            const int im = id / (SEQ * 8), r = (id >> 3) & (SEQ - 1), c = id & 7;
            const int s = im >= 3 ? 1 : 0, mat = im - 3 * s;
            const u32x4 v = *reinterpret_cast<const u32x4*>(smem + im * IMG + off_t(r, c));
            st_main(reinterpret_cast<u32x4*>(C + (int64_t)(m0 + SEQ * s + r) * g.ldc + mat * H + head * 64 + 8 * c), v, g.plain);
        }
        return;
    }
    AttnArgs a = p.a;
    a.drop = drop_resolve(a.drop);
    a.Sq = a.Skv = SEQ;   // (the host checked it: as constants they fold the core's end-of-sequence clamps and selects away)
    const int s = SEQ == 128 ? wave >> 2 : 0, b = m0 / SEQ + s;
    const char* sQ = smem + 3 * s * IMG;
    if constexpr (SEQ == 128) {
        attn_fwd_whole_head<2, 8, DROP, false, KB>(a, sQ, sQ + IMG, sQ + 2 * IMG, 2 * (wave & 3), 0, b * a.h + head, b, head, lane);
    } else {
#pragma unroll 1
        for (int t = 0; t < 2; ++t) {
            asm volatile("" ::: "memory");   // (keeps the pass's LDS reads -- K fragments, mask -- inside the pass: hoisted they spill)
            attn_fwd_whole_head<1, 16, DROP, false, KB>(a, sQ, sQ + IMG, sQ + 2 * IMG, 2 * wave + t, 0, b * a.h + head, b, head, lane);
        }
    }
}

#undef ICKA_W3_A
#undef ICKA_W3_B

// rows pm of the pm x pn XCD cut of a 256 x bnw tile grid that fetches least: min pn * M + pm * N over the cuts that divide it
// (forced: Tune::w3grid, where it divides the tile grid)
static int gemm_w3_grid(int M, int N, int bnw, int forced) {
    const int nbm = M / 256, nbn = N / bnw;
    int best = 8;
    long cost = -1;
    for (int pm = 8; pm >= 1; pm >>= 1) {
        const int pn = 8 / pm;
        if (nbm % pm || nbn % pn) continue;
        if (forced && pm != forced) continue;
        const long c = (long)pn * M + (long)pm * N;
        if (cost < 0 || c < cost) { cost = c; best = pm; }
    }
    if (cost < 0) {   // forced cut does not divide: fall back to the free choice
        for (int pm = 8; pm >= 1; pm >>= 1) {
            const int pn = 8 / pm;
            if (nbm % pm || nbn % pn) continue;
            const long c = (long)pn * M + (long)pm * N;
            if (cost < 0 || c < cost) { cost = c; best = pm; }
        }
    }
    return best;
}
// sets the XCD cut of g's 256 x bnw tile grid (GemmArgs::w3_sn, w3_pnlog); false where no cut divides the grid
static bool w3_set_grid(GemmArgs& g, int bnw, int forced) {
    const int pm = gemm_w3_grid(g.M, g.N, bnw, forced), pn = 8 / pm;
    g.w3_sn = (g.N / bnw) / pn; g.w3_pnlog = pn == 1 ? 0 : (pn == 2 ? 1 : (pn == 4 ? 2 : 3));
    return (g.M / 256) % pm == 0 && (g.N / bnw) % pn == 0;
}

}  // namespace

// QKV projection + whole-head self-attention in one launch (gemm_qkv_attn_kernel).  d: the NT projection [M, 3 H] = x . Wqkv^T
// with its bias and a bf16 output (the stacked [q | k | v] activation, written as by icka_gemm); operands bf16, or both fp16
// ("mixed16").  The attention arguments as icka_attn_fwd_ex with Q / K / V = the three column blocks of that output.
// ICKA_E_SHAPE = not a shape this launch covers (the caller runs icka_gemm + icka_attn_fwd_ex, which give the same bits):
// S = 128 or 256 tokens per sample, head size 64, whole 256-row tiles, a tile grid of the 12-wave kernel.
template <bool F16, int SEQ>
static void launch_qkv_attn(const QkvAttnArgs& p, int nb3, hipStream_t st) {
    if (p.a.drop.thr && p.a.keepbits) {
        if constexpr (SEQ == 256) hipLaunchKernelGGL((gemm_qkv_attn_kernel<true, F16, 256, true>), dim3(nb3), dim3(768), 0, st, p);
    } else if (p.a.drop.thr) hipLaunchKernelGGL((gemm_qkv_attn_kernel<true, F16, SEQ, false>), dim3(nb3), dim3(768), 0, st, p);
    else hipLaunchKernelGGL((gemm_qkv_attn_kernel<false, F16, SEQ, false>), dim3(nb3), dim3(768), 0, st, p);
}
extern "C" int icka_gemm_qkv_attn(const icka_gemm_desc* d, const float* add_mask, void* ctx, void* ctx_f16, int64_t ldo, float* lse,
                                  int32_t B, int32_t heads, int32_t S, float scale, float p_drop, uint64_t seed, void* keep_bits,
                                  void* stream) {
    if (!d || !add_mask || !ctx) return ICKA_E_ARG;
    if (B <= 0 || heads <= 0 || S <= 0) return ICKA_E_SHAPE;
    GemmArgs g;
    Tune t;
    bool aligned = false;
    const int rc = convert(d, g, aligned, t);
    if (rc) return rc;
    if (d->op != ICKA_GEMM_NT || !aligned || g.c_f32 || g.c_f16 || g.epi != ICKA_EPI_NONE || g.beta != 0.f || g.alpha != 1.f ||
        !g.bias || g.bias2 || g.K1 != 0 || g.colsum || g.C3 || g.C2 || !t.w3 || !t.ws || d->tune)
        return ICKA_E_SHAPE;
    const int H = heads * 64;
    if ((S != 128 && S != 256) || g.N != 3 * H || g.M != B * S || g.M % 256 || g.K > 1024) return ICKA_E_SHAPE;
    const int nb3 = (g.M / 256) * heads;
    if (nb3 % 8 || nb3 < 128) return ICKA_E_SHAPE;   // (small grids: the two launches, whose attention spreads over more CUs)
    if ((int64_t)B * heads * S * S >= (1ll << 32)) return ICKA_E_SHAPE;
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (!al16(ctx) || (ctx_f16 && !al16(ctx_f16)) || ldo % 8 || !al16(g.bias)) return ICKA_E_ALIGN;
    const bool keep = keep_bits && p_drop > 0.f;
    if (keep && S != 256) return ICKA_E_SHAPE;       // (keep bits are left by the 256-token instance only: ops.ATTN_KEEPBITS "auto")
    if (!w3_set_grid(g, 192, t.w3grid)) return ICKA_E_SHAPE;   // (N / 192 = heads: a column tile is a head)
    QkvAttnArgs p;
    p.g = g;
    p.a = AttnArgs{};
    const bf16_t* C = reinterpret_cast<const bf16_t*>(g.C);
    p.a.Q = C; p.a.ldq = g.ldc; p.a.K = C + H; p.a.ldk = g.ldc; p.a.V = C + 2 * H; p.a.ldv = g.ldc;
    p.a.mask = add_mask; p.a.Ow = (bf16_t*)ctx; p.a.Ow16 = (_Float16*)ctx_f16; p.a.ldo = ldo; p.a.lse = lse;
    p.a.B = B; p.a.h = heads; p.a.Sq = S; p.a.Skv = S; p.a.scale = scale; p.a.drop = make_drop(p_drop, seed);
    p.a.keepbits = p.a.drop.thr ? (uint32_t*)keep_bits : nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (g.f16) { if (S == 128) launch_qkv_attn<true, 128>(p, nb3, st); else launch_qkv_attn<true, 256>(p, nb3, st); }
    else { if (S == 128) launch_qkv_attn<false, 128>(p, nb3, st); else launch_qkv_attn<false, 256>(p, nb3, st); }
    ICKA_CHECK_LAUNCH();
    return 0;
}
