// Body of the 12-wave GEMM kernels of gemm_w3.inc: the statements between the braces of gemm_w3_kernel and of gemm_w3_live_kernel,
// which #include this file with B_KM, F16, BNW, LIVE (constants) and gp, a_live in scope.  Text, not a function template, on purpose:
// as an inlined function the plain instances came out with other machine code than before (tools/code_object_diff.py); included,
// each kernel compiles the very statements it always had.  LIVE: a_live holds one byte per row of A, 0 = the row is all zero; the
// loader waves stage the 8-row pieces without a live row from the zero line of gemm_core.h (as the LIVE instance of gemm_ws_body).
    const GemmArgs g = gp;
    __shared__ __attribute__((aligned(16))) char smem[W3_NA * W3_A + W3_NB * W3_B];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)reinterpret_cast<uintptr_t>(LDS_PTR(char, smem)));
    // BNW = tile width: 192 (two 96-column halves) or 128 (two 64-column halves: N = 1024 at bert-large, 256 tiles = one
    // round where 128x128 tiles take two); the B images keep their 16 KiB slots either way
    constexpr int BH = BNW / 2, NB16 = BH / 16;
    static_assert(BNW == 192 || BNW == 128, "tile width");
    int m0, n0;
    w3_origin(blockIdx.x, g.w3_sn, g.w3_pnlog, BNW, m0, n0);
    const int nk = g.K / BK;
    if (wave >= 8) {
        // ------------------------------------------------------------------------------------------- loader waves
        // The activation operand A (cold, the expensive one: tools/gemm_cold.py) runs TWO k-tiles ahead in a ring of 3,
        // the weight operand B one k-tile ahead in a ring of 2.  Issue order per iteration: B(kt+1), then A(kt+2); LDS-DMA
        // returns in order, so "A(kt), B(kt) landed" = at most the 8 instructions of A(kt+1) still in flight.
        const int lw = wave - 8;
        const bf16_t* pa0[4];
        const bf16_t* pa1[4];
        const bf16_t* pb0[4];
        const bf16_t* pb1[4];
        // LIVE: the flags are requested first, and B(0) goes out ahead of A(0) while they are in flight (the first wait only needs
        // "everything but the 8 pieces of A(1)")
        uint64_t fl0[4] = {0, 0, 0, 0}, fl1[4] = {0, 0, 0, 0};
        int64_t sl0[4] = {0, 0, 0, 0}, sl1[4] = {0, 0, 0, 0};
        if constexpr (LIVE) {
            live_request(fl0, a_live, m0, lw);
            live_request(fl1, a_live, m0 + 128, lw);
        }
        dma_init<false>(pa0, g.A, g.lda, m0, lw, lane);
        dma_init<false>(pa1, g.A, g.lda, m0 + 128, lw, lane);
        dma_init<B_KM, BH>(pb0, g.B, g.ldb, n0, lw, lane);
        dma_init<B_KM, BH>(pb1, g.B, g.ldb, n0 + BH, lw, lane);
        const int64_t sa = BK, sb = B_KM ? (int64_t)BK * g.ldb : BK;
        constexpr int NJB = B_KM ? 4 : BH / 32;
        const uint32_t ldsB = lds0 + W3_NA * W3_A;
#define ICKA_W3_A_LIVE(SLOT)                                                     \
    do {                                                                         \
        dma_issue_live(pa0, sl0, lds0 + (SLOT) * W3_A + lw * 1024);              \
        dma_issue_live(pa1, sl1, lds0 + (SLOT) * W3_A + TILE_BYTES + lw * 1024); \
    } while (0)
        if constexpr (LIVE) {
            ICKA_W3_B(0);
            live_select(pa0, sl0, fl0, sa, lane);
            live_select(pa1, sl1, fl1, sa, lane);
            ICKA_W3_A_LIVE(0);
            if (nk > 1) ICKA_W3_A_LIVE(1);
        } else {
            ICKA_W3_A(0);
            ICKA_W3_B(0);
            if (nk > 1) ICKA_W3_A(1);
        }
        int sa3 = 2;   // A slot of tile kt+2
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + 1 < nk) wait_vmcnt<8>(); else wait_vmcnt<0>();   // A(kt+1) may still be in flight (8 pieces: 2 x 4)
            __builtin_amdgcn_s_barrier();        // tile kt published; every compute wave is done with tile kt-1
            if (kt + 1 < nk) ICKA_W3_B((kt + 1) & 1);
            if constexpr (LIVE) { if (kt + 2 < nk) ICKA_W3_A_LIVE(sa3); }
            else { if (kt + 2 < nk) ICKA_W3_A(sa3); }
            sa3 = sa3 == 2 ? 0 : sa3 + 1;
        }
#undef ICKA_W3_A_LIVE
    }
    // ---------------------------------------------------------------------------------------------- compute waves
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
                for (int t = 0; t < NB16; ++t) fb[t] = read_frag<B_KM>(sB, 16 * t, ks, lane);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NB16; ++ni) acc[mi][ni] = mfma16t<F16>(fb[ni], fa[mi], acc[mi][ni]);
            }
        }
        asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");   // MFMA -> VALU read wait states (see gemm_ws_body)
    }
    // ---- epilogue through LDS in two passes of 128 x 192 (96 KiB f32): in pass p EVERY compute wave deposits the 32-row
    //      half p of its 64 x 96 accumulator tile (so only 48 accumulator registers stay alive under the row loop: with
    //      whole wave tiles per pass the other pass's 96 spilled to scratch at the 168-register cap of 3 waves / SIMD),
    //      then all 12 waves finish 8-column groups of rows with 16-byte row-contiguous accesses
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();   // operand ring dead (pass 0) / previous C tile consumed (pass 1)
        if (wave < 8) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int row = (wave >> 1) * 32 + 16 * h + (lane & 15);
#pragma unroll
                for (int ni = 0; ni < NB16; ++ni) {
                    const int ch = (wc >> 2) + 4 * ni + (lane >> 4);
                    *reinterpret_cast<f32x4*>(smem + (BNW == 192 ? off_cw(row, ch) : off_c(row, ch))) = acc[2 * pass + h][ni] * g.alpha;
                }
            }
        }
        __syncthreads();
        epilogue_rows<32, BNW / 8, BNW == 192 ? 1 : 2>(g, smem, m0 + 32 * pass, n0, tid);
    }
