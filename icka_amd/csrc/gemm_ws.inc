// The aligned GEMM path on 128 x BNT tiles (gemm_core.h; DESIGN.md section 4).  First the tile bodies, which gemm_fused.inc
// (LayerNorm, BatchNorm statistics, implicit convolution) and gemm_grouped.inc (several problems per launch) use as well:
// gemm_dma_body (256 threads), gemm_ws_body (4 loader + 4 compute waves) and bn_stats_tile.  Then the kernels of the plain launches:
//   gemm_dma_kernel        256 threads, LDS-DMA staging (predecessor of the warp-specialised kernels)
//   gemm_ws_kernel         512 threads: 4 loader waves (LDS-DMA) + 4 compute waves, ring of 3 .. 5 k-tiles, 128x128, 128x96 or
//                          128x64 output tiles, LDS-staged or direct (f32) epilogue; bf16 or (NT) fp16 operands
//   gemm_ws_live_kernel    the NN ring-of-3 instance with row-liveness flags of A (icka_gemm_live)
//   gemm_ws2_kernel        same with a ring of 2 and two co-resident blocks per CU (short-K, many-tile grids)
// Which of them a call gets is decided by the launch ladder of gemm.hip.  A source fragment of gemm.hip, included once there.
#include "gemm_core.h"

namespace {

template <bool A_KM, bool B_KM, int NBUF, int ABL>
__device__ __forceinline__ void gemm_dma_body(const GemmArgs& g, char* smem, const int bid, const int nb) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)reinterpret_cast<uintptr_t>(LDS_PTR(char, smem)));
    const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
    int m0, n0;
    tile_origin(bid, nb, g.M / BM, g.N / BN, m0, n0);

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = g.K / BK;
    const int k1t = g.K1 > 0 ? g.K1 / BK : -1;  // k-tile at which the reduction switches to (A2, B2)
    const bf16_t* pa[4];
    const bf16_t* pb[4];
    dma_init<A_KM>(pa, g.A, g.lda, m0, wave, lane);
    dma_init<B_KM>(pb, g.B, g.ldb, n0, wave, lane);
    int64_t sa = A_KM ? (int64_t)BK * g.lda : BK, sb = B_KM ? (int64_t)BK * g.ldb : BK;

#define ICKA_STAGE(KT, BUF)                                             \
    do {                                                                \
        if ((KT) == k1t) {                                              \
            dma_init<A_KM>(pa, g.A2, g.lda2, m0, wave, lane);           \
            dma_init<B_KM>(pb, g.B2, g.ldb2, n0, wave, lane);           \
            sa = A_KM ? (int64_t)BK * g.lda2 : BK;                      \
            sb = B_KM ? (int64_t)BK * g.ldb2 : BK;                      \
        }                                                               \
        dma_issue(pa, sa, lds0 + (BUF) + wave * 1024);                  \
        dma_issue(pb, sb, lds0 + (BUF) + TILE_BYTES + wave * 1024);     \
    } while (0)

    // LDS ring of NBUF stages, prefetch distance NBUF-1 k-tiles.  Each wave waits for ITS pieces of tile kt with a
    // counted vmcnt (the 8 DMA of tile kt+1 may stay in flight), then one raw s_barrier makes every wave's pieces
    // visible and also proves all waves finished reading the buffer that the next DMA overwrites.
    if (NBUF < 4) {
        // ---- v2 loop: ring of NBUF stages, fragments read right after the barrier -------------------------------
#pragma unroll
        for (int t = 0; t < NBUF - 1; ++t)
            if (t < nk) ICKA_STAGE(t, t * 2 * TILE_BYTES);
        int cur = 0;
        ICKA_STAMP(unsigned long long seg[5] = {0, 0, 0, 0, 0}, tA, tB;
                   const unsigned long long real0 = __builtin_amdgcn_s_memrealtime(), cyc0 = __builtin_amdgcn_s_memtime();)
        for (int kt = 0; kt < nk; ++kt) {
            ICKA_STAMP_NOW(tA);
            // tiles kt+1 .. min(kt+NBUF-2, nk-1) may stay in flight (8 DMA each per wave)
            int ahead = nk - 1 - kt;
            ahead = ahead > NBUF - 2 ? NBUF - 2 : ahead;
            if (ahead >= 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            ICKA_STAMP_LAP(seg[0], tA, tB);
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            ICKA_STAMP_LAP(seg[1], tA, tB);
            if (kt + NBUF - 1 < nk && ABL != 2) {
                int nx = cur + NBUF - 1;
                nx = nx >= NBUF ? nx - NBUF : nx;
                ICKA_STAGE(kt + NBUF - 1, nx * 2 * TILE_BYTES);
            }
            ICKA_STAMP_LAP(seg[2], tA, tB);
            const char* sA = smem + cur * 2 * TILE_BYTES;
            const char* sB = sA + TILE_BYTES;
            if (ABL != 1)
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
                    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = mfma16(fb[ni], fa[mi], acc[mi][ni]);
            }
            cur = cur + 1 == NBUF ? 0 : cur + 1;
            ICKA_STAMP(__builtin_amdgcn_sched_barrier(0); ICKA_STAMP_LAP(seg[3], tA, tB);)
        }
        ICKA_STAMP(if (g.stamp && (tid & 63) == 0 && wave == 0) {
            unsigned long long* o = g.stamp + (size_t)bid * 8;
            o[0] = seg[0]; o[1] = seg[1]; o[2] = seg[2]; o[3] = seg[3];
            o[4] = __builtin_amdgcn_s_memtime() - cyc0;
            o[5] = __builtin_amdgcn_s_memrealtime() - real0;
            o[6] = nk;
        })
    } else {
        // ---- v3 loop (ring of 4, one block per CU = one wave per SIMD): software-pipelined FRAGMENTS.  The barrier
        // sits between the two 16-MFMA halves of a k-tile: the second half's fragments (ks=1 of tile kt) are read
        // under the first half's MFMAs, and the NEXT tile's first fragments (ks=0 of tile kt+1, made visible by
        // this iteration's barrier) plus the DMA issue of tile kt+3 go under the second half's MFMAs, so neither
        // the LDS latency nor the DMA issue sequence is exposed at one wave per SIMD.
#pragma unroll
        for (int t = 0; t < 3; ++t)
            if (t < nk) ICKA_STAGE(t, t * 2 * TILE_BYTES);
        if (nk >= 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // tiles 0,1 landed; tile 2 may fly
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        bf16x8 fa0[4], fb0[4], fa1[4], fb1[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) fa0[t] = read_frag<A_KM>(smem, wr + 16 * t, 0, lane);
#pragma unroll
        for (int t = 0; t < 4; ++t) fb0[t] = read_frag<B_KM>(smem + TILE_BYTES, wc + 16 * t, 0, lane);
        int cur = 0;
        ICKA_STAMP(unsigned long long cseg[2] = {0, 0}, cA, cB; const unsigned long long ccyc0 = __builtin_amdgcn_s_memtime();)
        for (int kt = 0; kt < nk; ++kt) {
            ICKA_STAMP_NOW(cA);
            const char* sA = smem + cur * 2 * TILE_BYTES;
            const char* sB = sA + TILE_BYTES;
#pragma unroll
            for (int t = 0; t < 4; ++t) fa1[t] = read_frag<A_KM>(sA, wr + 16 * t, 1, lane);
#pragma unroll
            for (int t = 0; t < 4; ++t) fb1[t] = read_frag<B_KM>(sB, wc + 16 * t, 1, lane);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = mfma16(fb0[ni], fa0[mi], acc[mi][ni]);
            const int nxt = cur == 3 ? 0 : cur + 1;
            if (kt + 1 < nk) {
                // tile kt+1 must have landed (own pieces); tile kt+2 (if any) may stay in flight
                if (kt + 2 < nk) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                if (kt + 3 < nk) {
                    const int st = cur == 0 ? 3 : cur - 1;   // buffer of tile kt-1 == (kt+3) % 4
                    ICKA_STAGE(kt + 3, st * 2 * TILE_BYTES);
                }
                const char* nA = smem + nxt * 2 * TILE_BYTES;
#pragma unroll
                for (int t = 0; t < 4; ++t) fa0[t] = read_frag<A_KM>(nA, wr + 16 * t, 0, lane);
#pragma unroll
                for (int t = 0; t < 4; ++t) fb0[t] = read_frag<B_KM>(nA + TILE_BYTES, wc + 16 * t, 0, lane);
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = mfma16(fb1[ni], fa1[mi], acc[mi][ni]);
            cur = nxt;
        }
    }
#undef ICKA_STAGE
    __syncthreads();  // every wave is done with the operand ring before it is reused as the C tile

    // ---- epilogue through LDS (all waves are past the last barrier: the operand buffers are dead)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int row = wr + 16 * mi + (lane & 15);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int ch = (wc >> 2) + 4 * ni + (lane >> 4);
            *reinterpret_cast<f32x4*>(smem + off_c(row, ch)) = acc[mi][ni] * g.alpha;
        }
    }
    __syncthreads();
    epilogue_rows<16, 16, 0, A_KM>(g, smem, m0, n0, tid);
}

// Train-mode BatchNorm partials of one staged f32 output tile (off_c image at smem_c): per tile column n, (count, mean, M2)
// over the tile's rows m < rows_valid, written to part[k * (M / 128) * N + (m0 / 128) * N + n] for k = count, mean, M2.
// Thread (c, q) takes column c over the q-th 128 / NQ-row slice (two passes over LDS: mean, then squared deviations; q is
// wave-uniform); the q == 0 threads merge the NQ slices in slice order, so every partial is a fixed function of the tile.
// smem_red: 6 KiB of LDS past the C tile for the slices.
template <int BNT>
__device__ __forceinline__ void bn_stats_tile(const char* smem_c, char* smem_red, int m0, int n0, int tid, int M, int N, float* part,
                                              int rows_valid) {
    constexpr int NQ = 512 / BNT, RQ = 128 / NQ;
    const int c = tid % BNT, q = tid / BNT;
    int nv = rows_valid - m0;
    nv = nv < 0 ? 0 : (nv > BM ? BM : nv);
    const int r0 = q * RQ;
    const int r1 = r0 + RQ < nv ? r0 + RQ : nv;
    const int cnt = r1 > r0 ? r1 - r0 : 0;
    const char* col = smem_c + 4 * (c & 3);
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += *reinterpret_cast<const float*>(col + off_c(r, c >> 2));
    const float mean = cnt ? s / (float)cnt : 0.f;
    float m2 = 0.f;
    for (int r = r0; r < r1; ++r) {
        const float d = *reinterpret_cast<const float*>(col + off_c(r, c >> 2)) - mean;
        m2 += d * d;
    }
    float* red = reinterpret_cast<float*>(smem_red);
    red[tid] = (float)cnt;
    red[512 + tid] = mean;
    red[1024 + tid] = m2;
    __syncthreads();
    if (q == 0) {
        float n = 0.f, mu = 0.f, M2 = 0.f;
#pragma unroll
        for (int j = 0; j < NQ; ++j) bn_chan_merge(n, mu, M2, red[j * BNT + c], red[512 + j * BNT + c], red[1024 + j * BNT + c]);
        const int64_t plane = (int64_t)(M / BM) * N, at = (int64_t)(m0 / BM) * N + n0 + c;
        part[at] = n;
        part[plane + at] = mu;
        part[2 * plane + at] = M2;
    }
}

__device__ __forceinline__ bool g_direct_epilogue(const GemmArgs& g) {
    // f32 outputs only: 16 B per lane.  bf16 outputs (8 B per lane, 32-byte row pieces) measured 5 % slower than the
    // staged 16-byte row-contiguous stores (qkv projection, profiles/README.md)
    return g.direct && g.c_f32 && g.epi == ICKA_EPI_NONE && g.beta == 0.f;
}

// =====================================================================================================================
// Warp-specialised fast path (512 threads): waves 0-3 COMPUTE (LDS fragment reads + MFMA, 64x64 each), waves 4-7 LOAD
// (they only issue the LDS-DMA of the ring and wait for it).  In-kernel stamps of the 4-wave kernel showed a wave
// spending ~500 cycles per k-tile issuing its 8 global_load_lds (~60 cycles each) in series with its 512 cycles of
// MFMA; a loader wave co-resident on the same SIMD hides that issue time under the compute wave's matrix work.
// One s_barrier per k-tile joins both roles: loaders arrive after their counted vmcnt (tile kt landed), compute waves
// after finishing tile kt-1, so the barrier both publishes tile kt and frees the buffer of tile kt-1 for re-staging.
// LNF (gemm_ln_kernel): the tile's plain f32 output is stored WRITE-THROUGH (sc1) and the body returns instead of retiring its
// waves -- the kernel then hands the stripe's rows over to its LayerNorm phase inside the same launch.
// STATS (gemm_ws_bn_stats_kernel): the raw output tile (no bias / activation) is stored as usual, and bn_stats_tile writes
// the train-mode BatchNorm partials of its columns from the f32 tile in LDS to stats_part.
// LIVE (gemm_ws_live_kernel): a_live holds one byte per row of A, 0 = the row is all zero; the loader waves stage the 8-row
// pieces without a live row from the zero line of gemm_core.h.  Everything else, the compute waves included, is the plain body.
template <bool A_KM, bool B_KM, int NBUF, int ABL = 0, int DIST = 2, int BNT = 128, bool F16 = false, bool CONV = false, bool LNF = false,
          bool STATS = false, bool LIVE = false>
__device__ __forceinline__ void gemm_ws_body(const GemmArgs& g, char* smem, const int bid, const int nb, float* stats_part = nullptr,
                                             int stats_rows = 0, const uint8_t* a_live = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)reinterpret_cast<uintptr_t>(LDS_PTR(char, smem)));
    int m0, n0;
    // BNT = tile width: 128, or 96 when that fills the 256 CUs better (N = 768 -> 256 tiles instead of 192)
    constexpr int NTN = BNT / 32;                  // 16-column MFMA tiles per compute wave (4 or 3)
    constexpr int NJB = B_KM ? 4 : BNT / 32;       // LDS-DMA pieces of the B tile per loader wave
    constexpr int ND = 4 + NJB;                    // DMA instructions per k-tile per loader wave
    static_assert(BNT == 128 || BNT == 96 || BNT == 64, "tile width");
    tile_origin(bid, nb, g.M / BM, g.N / BNT, m0, n0, BNT);
    const int nk = g.K / BK;
    const int wr = ((wave & 3) >> 1) * 64, wc = (wave & 1) * (BNT / 2);
    ICKA_STAMP(const unsigned long long ph0 = __builtin_amdgcn_s_memtime(); unsigned long long ph1 = 0, ph2 = 0;)

    f32x4 acc[4][NTN];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NTN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Bias gradient for free: in the blocks of the first tile column the compute waves that own columns 0..63 also
    // multiply the A fragments (dY, rows = output features) by an all-ones operand: D[i][j] = sum_k A[j][k], i.e. the
    // column sums of dY over the tokens, 4 extra MFMAs per 16 (only in 1/nbn of the blocks).
    const bool do_cs = A_KM && g.colsum != nullptr && n0 == 0 && wave < 4 && wc == 0;
    f32x4 cs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) cs[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bf16x8 ones = {f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f)};

    if (wave >= 4) {
        // ------------------------------------------------------------------------------------------- loader waves
        const int lw = wave - 4;
        const int k1t = g.K1 > 0 ? g.K1 / BK : -1;
        const bf16_t* pa[4];
        const bf16_t* pb[4];
        // LIVE: the flags are requested first; the B pieces of k-tile 0 go out while they are in flight (within a k-tile the order
        // of the pieces is free: the counted waits are in whole tiles)
        uint64_t fl[4] = {0, 0, 0, 0};
        int64_t sal[4] = {0, 0, 0, 0};
        if constexpr (LIVE) {
            static_assert(!A_KM && !CONV && ABL == 0, "live A rows: a k-contiguous A operand");
            live_request(fl, a_live, m0, lw);
        }
        // CONV: the A tile is gathered from the NHWC activation.  Per piece (8 tile rows) this lane serves one output pixel:
        // the pointer to its centre input pixel (+ this lane's 16-byte chunk) and a 9-bit mask of the taps that lie inside
        // the image; a k-tile is 64 channels of ONE tap (cvC % 64 == 0), so its source is centre + a wave-uniform offset,
        // or the zero page.
        const bf16_t* ctr[4];
        uint32_t vmask[4] = {0u, 0u, 0u, 0u};
        const bf16_t* zsrc = nullptr;
        int cv_tap = 0, cv_cb = 0;
        if constexpr (CONV) {
            static_assert(!A_KM && !B_KM, "implicit convolution: NT only");
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = 8 * (lw + 4 * j) + (lane >> 3);
                const int lc = (lane & 7) ^ ((row >> 1) & 7);
                const int m = m0 + row;
                const int mm = m < g.cvRows ? m : 0;
                const int hw = g.cvHo * g.cvWo;
                const int b = mm / hw, r = mm - b * hw, oy = r / g.cvWo, ox = r - oy * g.cvWo;
                const int y0 = oy * g.cvS, x0 = ox * g.cvS;
                ctr[j] = g.A + ((int64_t)(b * g.cvH + y0) * g.cvW + x0) * g.cvC + 8 * lc;
                uint32_t vm = 0u;
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int y = y0 + t / 3 - 1, x = x0 + t % 3 - 1;
                    vm |= (m < g.cvRows && y >= 0 && y < g.cvH && x >= 0 && x < g.cvW) ? (1u << t) : 0u;
                }
                vmask[j] = vm;
                if (j == 0) zsrc = g.cvZero + 8 * (lane & 7);
            }
        } else {
            dma_init<A_KM>(pa, g.A, g.lda, m0, lw, lane);
        }
        dma_init<B_KM, BNT>(pb, g.B, g.ldb, n0, lw, lane);
        int64_t sa = CONV ? 0 : (A_KM ? (int64_t)BK * g.lda : BK), sb = B_KM ? (int64_t)BK * g.ldb : BK;
        if constexpr (LIVE) {   // (the host sends no two-segment reduction here: k1t stays -1)
            if (nk > 0) dma_issue<NJB>(pb, sb, lds0 + TILE_BYTES + lw * 1024);
            live_select(pa, sal, fl, sa, lane);
            if (nk > 0) dma_issue_live(pa, sal, lds0 + lw * 1024);
        }
#define ICKA_WS_STAGE(KT, BUF)                                          \
    do {                                                                \
        if constexpr (LIVE) {                                           \
            dma_issue_live(pa, sal, lds0 + (BUF) + lw * 1024);          \
            dma_issue<NJB>(pb, sb, lds0 + (BUF) + TILE_BYTES + lw * 1024); \
            break;                                                      \
        }                                                               \
        if ((KT) == k1t) {                                              \
            dma_init<A_KM>(pa, g.A2, g.lda2, m0, lw, lane);             \
            dma_init<B_KM, BNT>(pb, g.B2, g.ldb2, n0, lw, lane);        \
            sa = A_KM ? (int64_t)BK * g.lda2 : BK;                      \
            sb = B_KM ? (int64_t)BK * g.ldb2 : BK;                      \
        }                                                               \
        if constexpr (CONV) {   /* k-tiles are staged in order: (tap, channel block) advance as counters */ \
            const int64_t off_ = (int64_t)((cv_tap / 3 - 1) * g.cvW + (cv_tap % 3 - 1)) * g.cvC + cv_cb * 64; \
            _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)            \
                pa[j_] = ((vmask[j_] >> cv_tap) & 1u) ? ctr[j_] + off_ : zsrc; \
            if (++cv_cb == g.cvC / 64) { cv_cb = 0; ++cv_tap; }         \
        }                                                               \
        if (ABL != 2) {                                                 \
            dma_issue(pa, sa, lds0 + (BUF) + lw * 1024);                \
            dma_issue<NJB>(pb, sb, lds0 + (BUF) + TILE_BYTES + lw * 1024); \
        }                                                               \
    } while (0)
#pragma unroll
        for (int t = LIVE ? 1 : 0; t < NBUF - 1; ++t)
            if (t < nk) ICKA_WS_STAGE(t, t * 2 * TILE_BYTES);
        int cur = 0;
        ICKA_STAMP(unsigned long long seg[4] = {0, 0, 0, 0}, tA, tB;
                   const unsigned long long real0 = __builtin_amdgcn_s_memrealtime(), cyc0 = __builtin_amdgcn_s_memtime();)
        for (int kt = 0; kt < nk; ++kt) {
            ICKA_STAMP_NOW(tA);
            int ahead = nk - 1 - kt;
            ahead = ahead > NBUF - 2 ? NBUF - 2 : ahead;
            // tile kt has landed once at most `ahead` younger tiles (ND DMA instructions each) are still in flight
            static_assert(NBUF <= 5 && ND * (NBUF - 2) <= 63, "vmcnt range");
            switch (ahead) {
                case 0: wait_vmcnt<0>(); break;
                case 1: wait_vmcnt<ND>(); break;
                case 2: wait_vmcnt<2 * ND>(); break;
                default: wait_vmcnt<(NBUF > 4 ? 3 : 0) * ND>(); break;
            }
            ICKA_STAMP_LAP(seg[0], tA, tB);
            if (ABL != 3) __builtin_amdgcn_s_barrier();   // (ABL 3, diagnostic: both roles free-running, garbage results)
            ICKA_STAMP_LAP(seg[1], tA, tB);
            if (kt + NBUF - 1 < nk) {
                int nx = cur + NBUF - 1;
                nx = nx >= NBUF ? nx - NBUF : nx;
                ICKA_WS_STAGE(kt + NBUF - 1, nx * 2 * TILE_BYTES);
            }
            cur = cur + 1 == NBUF ? 0 : cur + 1;
            ICKA_STAMP_LAP(seg[2], tA, tB);
        }
        ICKA_STAMP(if (g.stamp && lane == 0 && wave == 4) {
            unsigned long long* o = g.stamp + (size_t)bid * 16;
            o[0] = seg[0]; o[1] = seg[1]; o[2] = seg[2];
            o[4] = __builtin_amdgcn_s_memtime() - cyc0;
            o[5] = __builtin_amdgcn_s_memrealtime() - real0;
            o[6] = nk;
        })
#undef ICKA_WS_STAGE
    } else {
        // ------------------------------------------------------------------------------------------ compute waves
        // Fragments are software-pipelined in registers with a prefetch distance of TWO 16-MFMA halves: while tile
        // kt is multiplied out of one register set (P), both halves of tile kt+1 are read into the other (Q).  Measured
        // (tools/probe/mfma_probe): LDS read latency at one wave per SIMD is hundreds of cycles once LDS-DMA writes
        // share the LDS pipe, far more than one half (272 cycles) covers.  Barrier kt+1 (tile kt+1 published, tile
        // kt fully in registers -> its buffer may be re-staged) is taken at the TOP of iteration kt.
        if constexpr (DIST == 1) {
            // two blocks per CU (ring of 2, <= 128 VGPRs): fragments are read per 32-deep step right before their
            // MFMAs; the co-resident block's waves cover the LDS latency and this block's epilogue/prologue
            int cur = 0;
            for (int kt = 0; kt < nk; ++kt) {
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                const char* sA = smem + cur * 2 * TILE_BYTES;
                const char* sB = sA + TILE_BYTES;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    bf16x8 fa[4], fb[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) fa[t] = read_frag<A_KM>(sA, wr + 16 * t, ks, lane);
#pragma unroll
                    for (int t = 0; t < NTN; ++t) fb[t] = read_frag<B_KM>(sB, wc + 16 * t, ks, lane);
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                        for (int ni = 0; ni < NTN; ++ni) acc[mi][ni] = mfma16t<F16>(fb[ni], fa[mi], acc[mi][ni]);
                    if (do_cs) {
#pragma unroll
                        for (int mi = 0; mi < 4; ++mi) cs[mi] = mfma16(ones, fa[mi], cs[mi]);
                    }
                }
                cur = cur + 1 == NBUF ? 0 : cur + 1;
            }
        } else {
        bf16x8 pa0[4], pb0[4], pa1[4], pb1[4], qa0[4], qb0[4], qa1[4], qb1[4];
#define ICKA_READ(FA, FB, BUFI, KS)                                                                  \
    if (ABL != 1) do {                                                                               \
        const char* b_ = smem + (BUFI) * 2 * TILE_BYTES;                                             \
        _Pragma("unroll") for (int t = 0; t < 4; ++t) FA[t] = read_frag<A_KM>(b_, wr + 16 * t, KS, lane);              \
        _Pragma("unroll") for (int t = 0; t < NTN; ++t) FB[t] = read_frag<B_KM>(b_ + TILE_BYTES, wc + 16 * t, KS, lane); \
        __builtin_amdgcn_sched_barrier(0); /* keep the reads AHEAD of the next MFMA group (hipcc sinks them) */     \
    } while (0)
#define ICKA_MMA(FA, FB)                                                                             \
    if (ABL != 1) do {                                                                               \
        _Pragma("unroll") for (int mi = 0; mi < 4; ++mi)                                             \
            _Pragma("unroll") for (int ni = 0; ni < NTN; ++ni) acc[mi][ni] = mfma16t<F16>(FB[ni], FA[mi], acc[mi][ni]); \
        if (do_cs) { _Pragma("unroll") for (int mi = 0; mi < 4; ++mi) cs[mi] = mfma16(ones, FA[mi], cs[mi]); }  \
        __builtin_amdgcn_sched_barrier(0);                                                           \
    } while (0)
// ICKA_RM: one scheduling region = fragment reads of the NEXT k-step (into the idle register set) + the MFMAs of the
// current one, with the DS reads spread between the MFMAs (sched_group_barrier: 1 MFMA, 1 DS read, ...).  Issued as a
// block in front of the MFMAs, the reads (+ their address arithmetic) left the matrix pipe idle for 150-300 cycles
// per k-step: there is one compute wave per SIMD, nothing else fills those slots (measured on the 256x128 kernel:
// 80.9 -> 64.3 us per launch).
#define ICKA_RM(RA, RB, BUFI, KS, MA, MB)                                                            \
    if (ABL != 1) do {                                                                               \
        constexpr int NR_ = 4 * (A_KM ? 2 : 1) + NTN * (B_KM ? 2 : 1), NM_ = 4 * NTN;                \
        constexpr int NP_ = NR_ < NM_ ? NR_ : NM_;                                                   \
        const char* b_ = smem + (BUFI) * 2 * TILE_BYTES;                                             \
        _Pragma("unroll") for (int t = 0; t < 4; ++t) RA[t] = read_frag<A_KM>(b_, wr + 16 * t, KS, lane);              \
        _Pragma("unroll") for (int t = 0; t < NTN; ++t) RB[t] = read_frag<B_KM>(b_ + TILE_BYTES, wc + 16 * t, KS, lane); \
        _Pragma("unroll") for (int mi = 0; mi < 4; ++mi)                                             \
            _Pragma("unroll") for (int ni = 0; ni < NTN; ++ni) acc[mi][ni] = mfma16t<F16>(MB[ni], MA[mi], acc[mi][ni]); \
        if constexpr (NR_ > NM_) __builtin_amdgcn_sched_group_barrier(0x100, NR_ - NM_, 0);          \
        _Pragma("unroll") for (int i_ = 0; i_ < NP_; ++i_) {                                         \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                       \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                       \
        }                                                                                            \
        if constexpr (NM_ > NR_) __builtin_amdgcn_sched_group_barrier(0x008, NM_ - NR_, 0);          \
        __builtin_amdgcn_sched_barrier(0);                                                           \
        if (do_cs) { _Pragma("unroll") for (int mi = 0; mi < 4; ++mi) cs[mi] = mfma16(ones, MA[mi], cs[mi]); }  \
        __builtin_amdgcn_sched_barrier(0);                                                           \
    } while (0)
#define ICKA_SYNC()                                          \
    do {                                                     \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   \
        if (ABL != 3) __builtin_amdgcn_s_barrier();          \
        asm volatile("" ::: "memory");                       \
    } while (0)
        if (ABL != 3) __builtin_amdgcn_s_barrier();   // barrier #0: tile 0 published
        asm volatile("" ::: "memory");
        ICKA_STAMP(ph1 = __builtin_amdgcn_s_memtime();)
        ICKA_READ(pa0, pb0, 0, 0);
        ICKA_READ(pa1, pb1, 0, 1);
        int nxt = NBUF > 1 ? 1 : 0;     // ring slot of tile kt+1
        int kt = 0;
        for (; kt + 2 <= nk - 1; kt += 2) {
            ICKA_SYNC();                         // barrier kt+1
            ICKA_RM(qa0, qb0, nxt, 0, pa0, pb0);
            ICKA_RM(qa1, qb1, nxt, 1, pa1, pb1);
            nxt = nxt + 1 == NBUF ? 0 : nxt + 1;
            ICKA_SYNC();                         // barrier kt+2
            ICKA_RM(pa0, pb0, nxt, 0, qa0, qb0);
            ICKA_RM(pa1, pb1, nxt, 1, qa1, qb1);
            nxt = nxt + 1 == NBUF ? 0 : nxt + 1;
        }
        // tail: kt is the next tile to multiply (in P); nk - kt is 1 or 2
        if (kt + 1 <= nk - 1) {
            ICKA_SYNC();
            ICKA_RM(qa0, qb0, nxt, 0, pa0, pb0);
            ICKA_RM(qa1, qb1, nxt, 1, pa1, pb1);
            ICKA_MMA(qa0, qb0);
            ICKA_MMA(qa1, qb1);
        } else {
            ICKA_MMA(pa0, pb0);
            ICKA_MMA(pa1, pb1);
        }
#undef ICKA_READ
#undef ICKA_MMA
#undef ICKA_RM
#undef ICKA_SYNC
        }
        // MFMA -> VALU read-after-write needs software wait states on gfx950 (8-pass MFMA: ~11).  hipcc's hazard
        // recognizer missed one across a block boundary here (<TN, 96-wide>, odd k-tile count: a v_mov of the last
        // accumulator element right behind the branch that follows the last MFMA -> one stale element per lane, found
        // by tools/gemm_tile_check.py), so the compute waves always idle 16 states before anything reads acc.
        asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
        ICKA_STAMP(ph2 = __builtin_amdgcn_s_memtime();)
    }
    // Plain f32 outputs (no activation / fan-in operand / accumulate: the GEMM -> LayerNorm intermediates) go straight
    // from the accumulators to HBM: a lane owns 4 consecutive columns of one row (16 B) and the 4 lane groups of an
    // MFMA tile cover 64 contiguous bytes per row; the stores of adjacent tiles merge in L2.  This skips two block barriers and
    // 128 KB of LDS traffic of the staged epilogue below, and the loader waves retire at once.
    if (g_direct_epilogue(g)) {
        ICKA_STAMP(if (g.stamp && lane == 0 && wave == 0) {
            unsigned long long* o = g.stamp + (size_t)bid * 16 + 11;
            o[0] = ph1 - ph0; o[1] = ph2 - ph1; o[2] = 0;
        })
        if (wave < 4) {
            __amdgpu_buffer_rsrc_t crsrc = __builtin_amdgcn_make_buffer_rsrc(g.C, 0, 0x7ffffff0, 0x00020000);   // (LNF stores)
            (void)crsrc;
            if (do_cs && lane < 16) {
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    float* p = g.colsum + m0 + wr + 16 * mi + lane;
                    *p = g.colsum_acc ? *p + cs[mi][0] : cs[mi][0];
                }
            }
#pragma unroll
            for (int ni = 0; ni < NTN; ++ni) {
                const int n = n0 + wc + 16 * ni + 4 * (lane >> 4);
                f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
                if (g.bias) b4 = *reinterpret_cast<const f32x4*>(g.bias + n);
                if (g.bias2) b4 += *reinterpret_cast<const f32x4*>(g.bias2 + n);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    const int m = m0 + wr + 16 * mi + (lane & 15);
                    const f32x4 v = acc[mi][ni] * g.alpha + b4;
                    if constexpr (LNF) {
                        // write-through (sc1 raw buffer store): the rows are read by OTHER CUs of this launch (ln_row.h).  (A first
                        // version used an inline-asm global_store ... sc1: hipcc's hazard recognizer cannot see into it, and the
                        // next tile's v_pk_fma overwrote the data registers of the store in flight -- 10 % wrong elements.)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), crsrc, (int)(((int64_t)m * g.ldc + n) * 4), 0, 16);
                    } else if (g.c_f32) {
                        if (!A_KM || !g.c3_only) st_out(reinterpret_cast<f32x4*>(reinterpret_cast<float*>(g.C) + (int64_t)m * g.ldc + n), v);
                        if constexpr (A_KM) {   // weight-gradient instances only: the data-parallel wire copy
                            if (g.C3) st_out(reinterpret_cast<u32x2*>(g.C3 + (int64_t)m * g.ldc3 + n), pack4(v[0], v[1], v[2], v[3]));
                        }
                    } else st_main(reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(g.C) + (int64_t)m * g.ldc + n),
                                pack4(v[0], v[1], v[2], v[3]), g.plain);
                }
            }
        }
        return;
    }
    __syncthreads();  // every wave is done with the operand ring before it is reused as the C tile

    if (do_cs && lane < 16) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            float* p = g.colsum + m0 + wr + 16 * mi + lane;
            *p = g.colsum_acc ? *p + cs[mi][0] : cs[mi][0];
        }
    }
    // ---- epilogue through LDS: compute waves deposit their accumulators, all 8 waves finish rows
    if (wave < 4) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int row = wr + 16 * mi + (lane & 15);
#pragma unroll
            for (int ni = 0; ni < NTN; ++ni) {
                const int ch = (wc >> 2) + 4 * ni + (lane >> 4);
                *reinterpret_cast<f32x4*>(smem + off_c(row, ch)) = acc[mi][ni] * g.alpha;
            }
        }
    }
    __syncthreads();
    if constexpr (STATS) {
        static_assert(NBUF * 2 * TILE_BYTES >= 128 * 512 + 3 * 512 * 4, "LDS room for the statistics slices");
        bn_stats_tile<BNT>(smem, smem + 128 * 512, m0, n0, tid, g.M, g.N, stats_part, stats_rows);
    }
    epilogue_rows<32, BNT / 8, 0, A_KM>(g, smem, m0, n0, tid);
    ICKA_STAMP(if (g.stamp && lane == 0 && wave == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned long long* o = g.stamp + (size_t)bid * 16 + 11;
        o[0] = ph1 - ph0; o[1] = ph2 - ph1; o[2] = __builtin_amdgcn_s_memtime() - ph2;
        o[3] = ph0; o[4] = __builtin_amdgcn_s_memtime();
    })
}

template <bool A_KM, bool B_KM, int NBUF, int ABL = 0, int BNT = 128, bool F16 = false, bool CONV = false>
__global__ __launch_bounds__(512) void gemm_ws_kernel(const GemmArgs gp) {
    const GemmArgs g = gp;
    __shared__ __attribute__((aligned(16))) char smem[NBUF * 2 * TILE_BYTES];
    gemm_ws_body<A_KM, B_KM, NBUF, ABL, 2, BNT, F16, CONV>(g, smem, blockIdx.x, gridDim.x);
}

// Two co-resident blocks per CU (64 KiB ring of 2 each, 4 waves per SIMD -> <= 128 VGPRs): for grids of several
// tiles per CU one block's prologue (first DMA latency, ~2.8k cycles) and epilogue (~5.5k) overlap the other
// block's main loop (stamps: at K = 768 they are 40 % of a tile's time).
template <bool A_KM, bool B_KM, int BNT = 128, bool F16 = false>
__global__ __launch_bounds__(512, 4) void gemm_ws2_kernel(const GemmArgs gp) {
    const GemmArgs g = gp;
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILE_BYTES];
    gemm_ws_body<A_KM, B_KM, 2, 0, 1, BNT, F16>(g, smem, blockIdx.x, gridDim.x);
}

// the NN kernel with row-liveness flags of A (icka_gemm_live; ring of 3 as the plain launch of these shapes)
template <int BNT>
__global__ __launch_bounds__(512) void gemm_ws_live_kernel(const GemmArgs gp, const uint8_t* a_live) {
    const GemmArgs g = gp;
    __shared__ __attribute__((aligned(16))) char smem[3 * 2 * TILE_BYTES];
    gemm_ws_body<false, true, 3, 0, 2, BNT, false, false, false, false, true>(g, smem, blockIdx.x, gridDim.x, nullptr, 0, a_live);
}

template <bool A_KM, bool B_KM, int NBUF, int ABL>
__global__ __launch_bounds__(256) void gemm_dma_kernel(const GemmArgs gp) {
    const GemmArgs g = gp;
    __shared__ __attribute__((aligned(16))) char smem[NBUF * 2 * TILE_BYTES];
    gemm_dma_body<A_KM, B_KM, NBUF, ABL>(g, smem, blockIdx.x, gridDim.x);
}

}  // namespace
