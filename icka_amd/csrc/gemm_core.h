// Shared by every file of the GEMM family (gemm.hip and its fragments gemm_ws / w3 / fused / grouped .inc): the launch
// descriptor GemmArgs and the tile constants, the launch-heuristic overrides (Tune), the LDS swizzles, the register-staged and
// LDS-DMA tile loaders, the fragment reads, the output store / load helpers and both epilogues, the block -> tile map, the
// cycle-stamp macros of the diagnostic builds and the launch macro of the host side.
#pragma once
#include "common.h"

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = 128 * 64 * 2;  // one operand tile, either layout

struct GemmArgs {
    int M, N, K, K1;
    const bf16_t* A;  int64_t lda;
    const bf16_t* B;  int64_t ldb;
    const bf16_t* A2; int64_t lda2;
    const bf16_t* B2; int64_t ldb2;
    void* C;  int64_t ldc;
    bf16_t* C2; int64_t ldc2;
    const bf16_t* aux; int64_t ldaux;
    const float* bias; const float* bias2;
    float alpha, beta;
    int epi, c_f32;
    int a_vec, b_vec;  // operand rows may be read with 16-byte loads (ld % 8 == 0, base 16-B aligned)
    int abl;           // diagnostic ablation of the fast path: 1 = no MFMA/LDS reads, 2 = no DMA staging
    float* colsum; int colsum_acc;  // TN fast path: colsum[m] (+)= sum_k A[k,m] (bias gradient fused into dW = dY^T.X)
    int n96ok;                  // fast path + N % 96 == 0: the 128x96 tile is an option
    int n64ok;                  // everything aligned except N % 128: N % 64 == 0 -> the 128x64 tile (NT only)
    int direct;                 // plain outputs skip the LDS-staged epilogue (Tune::direct)
    unsigned long long* stamp;  // diagnostic: [block][8] cycle sums (ICKA_GEMM_STAMP builds)
    int ksplit;        // general path: blockIdx.y splits the k-tiles; partial sums are atomically added to f32 C
    int f16;           // operands are IEEE fp16 (v_mfma_f32_16x16x32_f16; NT only): the "mixed16" forward GEMMs
    int c_f16;         // main output C is fp16 (c_f32 == 0)
    bf16_t* C3; int64_t ldc3;   // optional bf16 copy of the main output: of an fp16 activation (the weight-gradient operand of
                                // the "mixed16" mode), or of an f32 weight gradient (the data-parallel wire copy: the value
                                // AFTER beta-accumulation, written by the same epilogue -- dp.GradReducer)
    int aux_f16;       // the epilogue operand aux is fp16 (read through load8_aux / load4_aux)
    int w3_sn, w3_pnlog;   // 12-wave kernel: column tiles per XCD patch and log2(pn) of the pm x pn XCD cut (gemm_w3_grid)
    int c3_only;       // f32 C + C3 + beta == 0: write ONLY the bf16 wire copy C3 (the f32 value is produced later, from the
                       // reduced wire buffer, by icka_dp_cast_back_scaled): the epilogue stores 2 bytes per element, not 4 + 2
    int plain;         // the MAIN 16-bit output is stored with ordinary stores instead of streaming ones (st_main): per launch,
                       // from the diagnostic site mask ICKA_GEMM_PLAIN_MASK (site_bit)
    // implicit 3x3 / pad 1 convolution (icka_conv3x3_gemm): A is an NHWC activation [B, cvH, cvW, cvC], the A "row" m is
    // output pixel m and the reduction index is k = tap * cvC + c -- the loader waves compute the patch addresses, no
    // patch matrix exists.  cvZero: at least 128 B of zeros for the taps that fall off the image / rows past cvRows.
    int cvH, cvW, cvC, cvS, cvHo, cvWo, cvRows;
    const bf16_t* cvZero;
};

// ---- launch-heuristic overrides.  NO mutable process state (launchers are re-entrant and do not rely on
// hidden state; the autograd thread and a second model see exactly what the first one does): kTuneEnv is the ICKA_TUNE_GEMM_*
// environment read ONCE when the library is loaded (same-box A/B runs: tools/ab_env.sh), and a single launch may override fields
// through icka_gemm_desc.tune (tests of the alternative kernels, tools/gemm_*.py).  Results never depend on any of it.
struct Tune {
    int abl;      // diagnostic builds (-DICKA_GEMM_ABLATE): 1 = skip MFMA + LDS reads, 2 = skip the LDS-DMA staging (wrong results)
    int ws;       // 1: warp-specialised fast path (two blocks per CU for large grids), 0: single-role kernel, 2: force two blocks, 3: never two
    int direct;   // 1: plain outputs are stored straight from the accumulators (0: always through the LDS C tile)
    int w3;       // 1: 256x192 / 256x128 tiles (12-wave kernel) for wide / short-K outputs
    int bn;       // tile width of the warp-specialised path: 0 = heuristic, 128 / 96 forced
    int nbuf;     // LDS ring depth of the fast path: 0 = per-shape heuristic, or forced 2 .. 5
    int w3grid;   // XCD cut of the 12-wave kernel's tile grid: 0 = per shape, 8 / 4 / 2 / 1 = force pm (if it divides the tile grid)
    int big;      // grouped TN launches: 2 = 256x128 tiles / 12 waves, 1 = 8 waves, 0 = 128x128 group kernel
};

// "launch this instantiation on this grid, check, RETURN the status from the enclosing host function"
#define ICKA_LAUNCH_RETURN(KERNEL, GRID, BLOCK, STREAM, ARGS)                       \
    do {                                                                            \
        hipLaunchKernelGGL(KERNEL, dim3(GRID), dim3(BLOCK), 0, STREAM, ARGS);       \
        ICKA_CHECK_LAUNCH();                                                        \
        return 0;                                                                   \
    } while (0)

// Cycle stamps of the diagnostic build (-DICKA_GEMM_STAMP, tools/gemm_stamp.py); all three expand to nothing otherwise.
//   ICKA_STAMP(code)          statements and declarations that exist in the stamp build only
//   ICKA_STAMP_NOW(v)         v = the shader clock, after this wave's outstanding scalar / LDS operations
//   ICKA_STAMP_LAP(sum, a, b) b = now; sum += b - a; a = b
#ifdef ICKA_GEMM_STAMP
#define ICKA_STAMP(...) __VA_ARGS__
#define ICKA_STAMP_NOW(v) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory")
#define ICKA_STAMP_LAP(sum, a, b) do { ICKA_STAMP_NOW(b); sum += b - a; a = b; } while (0)
#else
#define ICKA_STAMP(...)
#define ICKA_STAMP_NOW(v)
#define ICKA_STAMP_LAP(sum, a, b)
#endif

namespace {

// k-contiguous tile image [128 rows][64 k]: 128-B rows, 16-B chunk index XORed with (row>>1)&7 so that the 16 rows
// of a fragment read land on 16 distinct 16-B slots of the 256-B bank row.
__device__ __forceinline__ uint32_t off_kc(int row, int ch) { return row * 128 + (((ch ^ (row >> 1)) & 7) << 4); }
// k-major tile image [64 k][128 rows]: 256-B rows; chunk XOR per cdna guide T10 image (b), serves the transposed read.
__device__ __forceinline__ uint32_t off_km(int kr, int ch) {
    return kr * 256 + ((ch ^ (((kr & 3) << 2) | ((kr >> 2) & 3))) << 4);
}

__device__ __forceinline__ u32x4 load_partial(const bf16_t* p, int nvalid) {
    const unsigned short* ps = reinterpret_cast<const unsigned short*>(p);
    u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t x = e < nvalid ? (uint32_t)ps[e] : 0u;
        v[e >> 1] |= x << (16 * (e & 1));
    }
    return v;
}

// global -> registers: 4 x 16-byte chunks per thread cover the 128x64 (or 64x128) tile.
template <bool KM, bool ALIGNED>
__device__ __forceinline__ void g2r(u32x4 (&r)[4], const bf16_t* __restrict__ P, int64_t ld, int row0, int nrows,
                                    int k0, int K, int tid, int vec) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = tid + 256 * i;
        const bf16_t* p;
        bool ok;
        int rem;
        if (!KM) {
            const int rr = q >> 3, c = q & 7;
            const int grow = row0 + rr, gk = k0 + 8 * c;
            p = P + (int64_t)grow * ld + gk;
            ok = grow < nrows;
            rem = K - gk;
        } else {
            const int kr = q >> 4, c = q & 15;
            const int gk = k0 + kr, gcol = row0 + 8 * c;
            p = P + (int64_t)gk * ld + gcol;
            ok = gk < K;
            rem = nrows - gcol;
        }
        if (ALIGNED) {
            r[i] = *reinterpret_cast<const u32x4*>(p);
        } else {
            if (ok && rem >= 8 && vec) r[i] = *reinterpret_cast<const u32x4*>(p);
            else if (ok && rem > 0) r[i] = load_partial(p, rem < 8 ? rem : 8);
            else r[i] = u32x4{0u, 0u, 0u, 0u};
        }
    }
}

template <bool KM>
__device__ __forceinline__ void r2s(const u32x4 (&r)[4], char* tile, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = tid + 256 * i;
        const uint32_t off = KM ? off_km(q >> 4, q & 15) : off_kc(q >> 3, q & 7);
        *reinterpret_cast<u32x4*>(tile + off) = r[i];
    }
}

// MFMA operand fragment for the 16 tile-rows starting at rbase, k-step ks (32 k each) of the 64-deep tile:
// lane l gets element e = operand[row rbase + (l&15)][k = 32*ks + 8*(l>>4) + e].
template <bool KM>
__device__ __forceinline__ bf16x8 read_frag(const char* tile, int rbase, int ks, int lane) {
    if (!KM) {
        return lds_read_b128(tile, off_kc(rbase + (lane & 15), ks * 4 + (lane >> 4)));
    } else {
        const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
        const int c = (rbase >> 3) + (p >> 1);
        const int kr = ks * 32 + 8 * g + q;
        const bf16x4 lo = lds_read_tr(tile, off_km(kr, c) + 8 * (p & 1));
        const bf16x4 hi = lds_read_tr(tile, off_km(kr + 4, c) + 8 * (p & 1));
        return join8(lo, hi);
    }
}

__device__ __forceinline__ void load4(const bf16_t* base, int64_t ld, int m, int n, int nvalid, float (&o)[4]) {
    const bf16_t* p = base + (int64_t)m * ld + n;
    if (nvalid == 4 && ((reinterpret_cast<uintptr_t>(p) & 7) == 0)) {
        const bf16x4 v = as_bf16x4(*reinterpret_cast<const u32x2*>(p));
        o[0] = bf2f(v[0]); o[1] = bf2f(v[1]); o[2] = bf2f(v[2]); o[3] = bf2f(v[3]);
    } else {
        for (int r = 0; r < 4; ++r) o[r] = r < nvalid ? bf2f(p[r]) : 0.f;
    }
}
__device__ __forceinline__ void load4_aux(const bf16_t* base, int64_t ld, int m, int n, int nvalid, int f16, float (&o)[4]) {
    if (!f16) { load4(base, ld, m, n, nvalid, o); return; }
    const _Float16* p = reinterpret_cast<const _Float16*>(base) + (int64_t)m * ld + n;
    for (int r = 0; r < 4; ++r) o[r] = r < nvalid ? (float)p[r] : 0.f;
}
__device__ __forceinline__ void store4_bf16(bf16_t* base, int64_t ld, int m, int n, int nvalid, const float (&v)[4]) {
    bf16_t* p = base + (int64_t)m * ld + n;
    if (nvalid == 4 && ((reinterpret_cast<uintptr_t>(p) & 7) == 0)) {
        *reinterpret_cast<u32x2*>(p) = pack4(v[0], v[1], v[2], v[3]);
    } else {
        for (int r = 0; r < 4; ++r)
            if (r < nvalid) p[r] = f2bf(v[r]);
    }
}

__device__ __forceinline__ void epilogue4(const GemmArgs& g, int m, int n, f32x4 acc) {
    const int nvalid = (g.N - n) < 4 ? (g.N - n) : 4;
    float v[4] = {acc[0] * g.alpha, acc[1] * g.alpha, acc[2] * g.alpha, acc[3] * g.alpha};
    if (g.bias && blockIdx.y == 0) {
        for (int r = 0; r < 4; ++r)
            if (r < nvalid) v[r] += g.bias[n + r];
    }
    if (g.bias2 && blockIdx.y == 0) {
        for (int r = 0; r < 4; ++r)
            if (r < nvalid) v[r] += g.bias2[n + r];
    }
    float a[4];
    switch (g.epi) {
        case ICKA_EPI_GELU:
            store4_bf16(g.C2, g.ldc2, m, n, nvalid, v);
            for (int r = 0; r < 4; ++r) v[r] = gelu_f(v[r]);
            break;
        case ICKA_EPI_DGELU:
            load4_aux(g.aux, g.ldaux, m, n, nvalid, g.aux_f16, a);
            for (int r = 0; r < 4; ++r) v[r] *= dgelu_f(a[r]);
            break;
        case ICKA_EPI_ADD:
            load4_aux(g.aux, g.ldaux, m, n, nvalid, g.aux_f16, a);
            for (int r = 0; r < 4; ++r) v[r] += a[r];
            break;
        case ICKA_EPI_GATE:
            for (int r = 0; r < 4; ++r) v[r] = sigmoid_f(v[r]);
            if (g.C2) store4_bf16(g.C2, g.ldc2, m, n, nvalid, v);
            load4_aux(g.aux, g.ldaux, m, n, nvalid, g.aux_f16, a);
            for (int r = 0; r < 4; ++r) v[r] *= a[r];
            break;
        case ICKA_EPI_TANH:
            for (int r = 0; r < 4; ++r) v[r] = tanhf(v[r]);
            break;
        case ICKA_EPI_ADD_RELU:
            load4_aux(g.aux, g.ldaux, m, n, nvalid, g.aux_f16, a);
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r] + a[r], 0.f);
            break;
        case ICKA_EPI_RELU:
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            break;
        default: break;
    }
    if (g.ksplit > 1) {   // partial sum of one k-range (host guarantees f32 C, plain epilogue, C pre-scaled by beta)
        float* p = reinterpret_cast<float*>(g.C) + (int64_t)m * g.ldc + n;
        for (int r = 0; r < 4; ++r)
            if (r < nvalid) atomicAdd(p + r, v[r]);
        return;
    }
    if (g.c_f32 && g.c3_only) {
        store4_bf16(g.C3, g.ldc3, m, n, nvalid, v);
    } else if (g.c_f32) {
        float* p = reinterpret_cast<float*>(g.C) + (int64_t)m * g.ldc + n;
        if (nvalid == 4 && ((reinterpret_cast<uintptr_t>(p) & 15) == 0)) {
            f32x4 o = {v[0], v[1], v[2], v[3]};
            if (g.beta != 0.f) o += g.beta * *reinterpret_cast<const f32x4*>(p);
            *reinterpret_cast<f32x4*>(p) = o;
            for (int r = 0; r < 4; ++r) v[r] = o[r];
        } else {
            for (int r = 0; r < 4; ++r)
                if (r < nvalid) { v[r] += g.beta != 0.f ? g.beta * p[r] : 0.f; p[r] = v[r]; }
        }
        if (g.C3) store4_bf16(g.C3, g.ldc3, m, n, nvalid, v);
    } else if (g.c_f16) {
        _Float16* p = reinterpret_cast<_Float16*>(g.C) + (int64_t)m * g.ldc + n;
        for (int r = 0; r < 4; ++r)
            if (r < nvalid) p[r] = (_Float16)fminf(fmaxf(v[r], -65504.f), 65504.f);
        if (g.C3) store4_bf16(g.C3, g.ldc3, m, n, nvalid, v);
    } else {
        bf16_t* C = reinterpret_cast<bf16_t*>(g.C);
        if (g.beta != 0.f) {
            load4(C, g.ldc, m, n, nvalid, a);
            for (int r = 0; r < 4; ++r) v[r] += g.beta * a[r];
        }
        store4_bf16(C, g.ldc, m, n, nvalid, v);
    }
}

// =====================================================================================================================
// Fast path (M % 128 == 0, N % 128 == 0, K % 64 == 0, 16-B aligned operands): same tile / MFMA / LDS images as above,
// but (1) tiles are staged by LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave-instruction straight into LDS, no
// staging VGPRs, no ds_write pass) -- the swizzle is applied to the per-lane SOURCE address because the DMA
// destination is lane-linear -- with the next k-tile's DMA issued before the current tile's MFMAs, one barrier per
// k-tile; (2) the epilogue goes through LDS as an f32 [128][128] tile (XOR-swizzled 16-B chunks) so that every
// thread finishes 8 consecutive columns of a row: bias / activation / fan-in operands and the C stores are all
// 16-byte, row-contiguous accesses (whole 256-B rows per 16 lanes) instead of 8-byte stores scattered over 16 rows.
// Per-lane SOURCE pointers of the 4 one-KiB pieces a wave stages per operand tile (k-tile 0).  They advance by a
// wave-uniform stride per k-tile, so the k-loop carries no address arithmetic beyond 8 pointer bumps.
// NCOL = operand rows (k-contiguous) / columns (k-major) the tile really has: 128, or 96 for the narrow-N tile.  The
// LDS image keeps the 128-wide geometry; with 96 the k-contiguous image simply has no pieces 12..15 and the k-major
// image leaves chunks 12..15 of every row unused (their lanes re-fetch a valid chunk of the same row instead).
template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

template <bool KM, int NCOL = 128>
__device__ __forceinline__ void dma_init(const bf16_t* (&ptr)[4], const bf16_t* __restrict__ P, int64_t ld, int row0,
                                         int wave, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = wave + 4 * j;  // 1-KiB piece: 8 tile rows (k-contiguous image) or 4 k-rows (k-major image)
        if (!KM) {
            const int row = (8 * p + (lane >> 3)) % NCOL;   // pieces past NCOL/8 are never issued
            const int lc = (lane & 7) ^ ((row >> 1) & 7);
            ptr[j] = P + (int64_t)(row0 + row) * ld + 8 * lc;
        } else {
            const int kr = 4 * p + (lane >> 4);
            int lc = (lane & 15) ^ (((kr & 3) << 2) | ((kr >> 2) & 3));
            if (lc >= NCOL / 8) lc &= 7;
            ptr[j] = P + (int64_t)kr * ld + row0 + 8 * lc;
        }
    }
}
// Issue the 4 LDS-DMA loads of one operand tile (pieces wave, wave+4, wave+8, wave+12 -> 4 KiB apart) from INLINE
// ASM: hipcc treats a compiler-visible LDS-DMA as a pending LDS store and puts `s_waitcnt vmcnt(0)` in front of the
// next ds_read_b64_tr_b16, which serialises the whole pipeline; hidden in asm, the ring is ordered only by our own
// counted vmcnt + s_barrier (cdna guide section 5.7).  M0 (LDS destination base) is saved/restored inside.
#ifndef ICKA_DMA_POL
#define ICKA_DMA_POL ""   // cache-policy bits of the operand loads (diagnostic builds: " nt", " sc1", " sc0 sc1")
#endif
template <int NJ = 4>
__device__ __forceinline__ void dma_issue(const bf16_t* (&ptr)[4], int64_t stride, uint32_t lds_base) {
    uint32_t keep;
    if constexpr (NJ == 2) {
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %3\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %1, off" ICKA_DMA_POL "\n\t"
            "s_add_u32 m0, m0, 0x1000\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %2, off" ICKA_DMA_POL "\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(ptr[0]), "v"(ptr[1]), "s"(lds_base)
            : "memory", "scc");
#pragma unroll
        for (int j = 0; j < 2; ++j) ptr[j] += stride;
        return;
    }
    if constexpr (NJ == 3) {
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %4\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %1, off" ICKA_DMA_POL "\n\t"
            "s_add_u32 m0, m0, 0x1000\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %2, off" ICKA_DMA_POL "\n\t"
            "s_add_u32 m0, m0, 0x1000\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %3, off" ICKA_DMA_POL "\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(ptr[0]), "v"(ptr[1]), "v"(ptr[2]), "s"(lds_base)
            : "memory", "scc");
#pragma unroll
        for (int j = 0; j < 3; ++j) ptr[j] += stride;
        return;
    }
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %5\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off" ICKA_DMA_POL "\n\t"
        "s_add_u32 m0, m0, 0x1000\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %2, off" ICKA_DMA_POL "\n\t"
        "s_add_u32 m0, m0, 0x1000\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %3, off" ICKA_DMA_POL "\n\t"
        "s_add_u32 m0, m0, 0x1000\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %4, off" ICKA_DMA_POL "\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(ptr[0]), "v"(ptr[1]), "v"(ptr[2]), "v"(ptr[3]), "s"(lds_base)
        : "memory", "scc");
#pragma unroll
    for (int j = 0; j < 4; ++j) ptr[j] += stride;
}

// The same 4 loads from ptr + off, the pointers left where they are (the live-tile loader: k-tiles are not visited in
// unit steps, so the tile's operand offset replaces the running stride).
__device__ __forceinline__ void dma_issue_at(const bf16_t* const (&ptr)[4], int64_t off, uint32_t lds_base) {
    const bf16_t* q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = ptr[j] + off;
    dma_issue(q, 0, lds_base);
}

// ---- live A rows (icka_gemm_live: the LIVE instances of gemm_ws_body and of the 12-wave kernel).  a_live[t] == 0 promises that
// row t of A is all zero.  A loader wave's 1-KiB piece is 8 tile rows; a piece whose 8 bytes are all 0 is staged from this
// never-written line of zeros instead of from A (all 64 lanes read inside its 128 bytes, and the pointer does not advance with k):
// LDS receives the same zeros, the DMA sequence and every counted wait stay what they are, and the dead rows' bytes never leave L2.
__device__ __attribute__((aligned(128))) uint32_t g_zero_line[32];

// the 8 flag bytes of piece wave + 4 j of the 128-row A image at row0 (row0 % 128 == 0, a_live 16-byte aligned), j = 0 .. 3
__device__ __forceinline__ void live_request(uint64_t (&fl)[4], const uint8_t* __restrict__ a_live, int row0, int wave) {
#pragma unroll
    for (int j = 0; j < 4; ++j) fl[j] = *reinterpret_cast<const uint64_t*>(a_live + row0 + 8 * (wave + 4 * j));
}
// redirect the dead pieces of dma_init's pointers to the zero line; st[j] = the per-k-tile stride of piece j (0 when dead)
__device__ __forceinline__ void live_select(const bf16_t* (&ptr)[4], int64_t (&st)[4], const uint64_t (&fl)[4], int64_t stride, int lane) {
    const bf16_t* z = reinterpret_cast<const bf16_t*>(g_zero_line) + 8 * (lane & 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool dead = fl[j] == 0;
        ptr[j] = dead ? z : ptr[j];
        st[j] = dead ? 0 : stride;
    }
}
// dma_issue with a stride per piece
__device__ __forceinline__ void dma_issue_live(const bf16_t* (&ptr)[4], const int64_t (&st)[4], uint32_t lds_base) {
    dma_issue(ptr, 0, lds_base);
#pragma unroll
    for (int j = 0; j < 4; ++j) ptr[j] += st[j];
}

// f32 C tile in LDS: [128 rows][32 chunks of 4 floats], chunk index XORed with row&31
__device__ __forceinline__ uint32_t off_c(int row, int ch) { return row * 512 + ((ch ^ (row & 31)) << 4); }
// same for a 192-column f32 tile (48 chunks of 16 B per row; the XOR stays inside each group of 16 chunks)
__device__ __forceinline__ uint32_t off_cw(int row, int ch) { return row * 768 + ((ch ^ (row & 15)) << 4); }

// Output stores of the fast-path epilogues are NON-TEMPORAL: an FFN launch writes 25-50 MB, which as ordinary stores
// pushed the operand panels out of the XCD's 4 MiB L2 (rocprofv3: L2 hit rate 0.57-0.79, 3-6x the algorithmic bytes
// fetched over the fabric).  Measured on the c2 step: GEMM class 559 -> 593 TFLOP/s.
template <typename T>
__device__ __forceinline__ void st_out(T* p, const T v) {
#ifdef ICKA_ST_TEMPORAL
    *p = v;   // (diagnostic build: plain stores)
#else
    __builtin_nontemporal_store(v, p);
#endif
}
// epilogue operands that are read exactly once (GELU' input, residual / fan-in addend, accumulate-into output)
template <typename T>
__device__ __forceinline__ T ld_once(const T* p) {
#ifdef ICKA_NT_AUX
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
__device__ __forceinline__ void load8_bf16(const bf16_t* p, float (&o)[8]) {
    const bf16x8 v = as_bf16x8(ld_once(reinterpret_cast<const u32x4*>(p)));
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = bf2f(v[e]);
}
// epilogue operand in either 16-bit type (same element size: the pointer arithmetic is shared)
__device__ __forceinline__ void load8_aux(const bf16_t* p, int f16, float (&o)[8]) {
    if (f16) {
        const f16x8 v = __builtin_bit_cast(f16x8, ld_once(reinterpret_cast<const u32x4*>(p)));
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (float)v[e];
    } else {
        load8_bf16(p, o);
    }
}
// the same in two steps: the 16 raw bytes (issued early), converted where they are used
__device__ __forceinline__ void cvt8_aux(const u32x4 raw, int f16, float (&o)[8]) {
    if (f16) {
        const f16x8 v = __builtin_bit_cast(f16x8, raw);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (float)v[e];
    } else {
        const bf16x8 v = as_bf16x8(raw);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = bf2f(v[e]);
    }
}
__device__ __forceinline__ void store8_bf16(bf16_t* p, const float (&v)[8]) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(v[e]);
    st_out(reinterpret_cast<u32x4*>(p), as_u32x4(o));
}
// MAIN activation output with a per-launch store policy (GemmArgs.plain: the ICKA_GEMM_PLAIN_MASK diagnostic): plain = an ordinary
// store, the line stays in the L2 / Infinity Cache for the consumer kernel; else the streaming store of st_out
template <typename T>
__device__ __forceinline__ void st_main(T* p, const T v, int plain) {
    if (plain) *p = v;
    else st_out(p, v);
}
__device__ __forceinline__ void store8_bf16_main(bf16_t* p, const float (&v)[8], int plain) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(v[e]);
    st_main(reinterpret_cast<u32x4*>(p), as_u32x4(o), plain);
}

// fp16 outputs saturate at the largest finite half instead of overflowing to inf (an inf would turn the next LayerNorm
// row into NaNs); real BERT activations stay orders of magnitude below it.
__device__ __forceinline__ _Float16 f2h(float v) { return (_Float16)fminf(fmaxf(v, -65504.f), 65504.f); }
__device__ __forceinline__ void store8_f16(void* p, const float (&v)[8], int plain = 0) {
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2h(v[e]);
    st_main(reinterpret_cast<u32x4*>(p), __builtin_bit_cast(u32x4, o), plain);
}

// Block -> output tile.  Blocks b and b+8 share an XCD (round-robin dispatch); each XCD has a private 4 MiB L2.
//  * few column tiles: every XCD takes a contiguous run of row-major tiles (its A row panels + all of B stay in L2);
//  * many column tiles (N >= 1536): the 8 XCDs form a 4 x 2 grid over the tile matrix, so an XCD touches nbm/4 A
//    panels and nbn/2 B panels instead of nbm/8 and ALL nbn (B alone would overflow its L2 and be re-fetched from
//    the Infinity Cache for every tile row: rocprofv3 FETCH_SIZE was 3-4x the algorithmic bytes).
// Placement only affects speed: every tile is produced exactly once for any dispatch order.
__device__ __forceinline__ void tile_origin(int bid, int nb, int nbm, int nbn, int& m0, int& n0, int bn = BN) {
    const int xcd = bid & 7, li = bid >> 3;
    if (nbn >= 12 && (nb & 7) == 0 && (nbm & 3) == 0 && (nbn & 1) == 0) {
        const int sm = nbm >> 2, sn = nbn >> 1;
        const int xi = xcd >> 1, xj = xcd & 1;
        m0 = (xi * sm + li / sn) * BM;
        n0 = (xj * sn + li % sn) * bn;
        return;
    }
    const int qn = nb >> 3, rn = nb & 7;
    const int sw = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + li;
    if (nbn > nbm) {  // runs go along the SHORTER side, so an XCD's run is a squarish patch (fewer operand panels)
        m0 = (sw % nbm) * BM;
        n0 = (sw / nbm) * bn;
        return;
    }
    m0 = (sw / nbn) * BM;
    n0 = (sw % nbn) * bn;
}

// Second half of the LDS-staged epilogue: thread t finishes 8 consecutive columns (c8 = t & 15) of rows
// (t >> 4) + RSTEP*i; 16 lanes cover a whole 128-column row -> 16-byte row-contiguous global accesses.
// WIDE: 0 = a 128-row tile of the 8-wave kernels; 1 / 2 = one 128-row pass of gemm_w3_kernel's 192- / 128-column tile (the
// staged rows are 32-row slabs of four 64-row wave tiles; 192 columns use the off_cw image)
// WIRE: the instance may be asked for the data-parallel wire copy of an f32 output (C3 / c3_only): weight-gradient (TN)
// instances only -- compiled out everywhere else (as a run-time test in every instance it cost the 12-wave kernels, which run
// at their register cap, 5 % and showed up in kernels that never see a wire copy)
template <int RSTEP, int NC8 = 16, int WIDE = 0, bool WIRE = false>
__device__ __forceinline__ void epilogue_rows(const GemmArgs& g, const char* smem, int m0, int n0, int tid) {
    constexpr int ROWS = 128;   // rows of the staged tile
    // NC8 = 8-column groups per tile row: 16 (128-wide tile), 12 (96-wide: 384 of 512 threads) or 24 (192-wide, 768 threads)
    if (tid >= RSTEP * NC8) return;
    const int c8 = NC8 == 16 ? (tid & 15) : tid % NC8;   // 8-column group of the row
    const int rb = NC8 == 16 ? (tid >> 4) : tid / NC8;
    const int n = n0 + 8 * c8;
    float bias[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bias[e] = 0.f;
    if (g.bias) {
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(g.bias + n), b1 = *reinterpret_cast<const f32x4*>(g.bias + n + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { bias[e] = b0[e]; bias[4 + e] = b1[e]; }
    }
    if (g.bias2) {
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(g.bias2 + n), b1 = *reinterpret_cast<const f32x4*>(g.bias2 + n + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { bias[e] += b0[e]; bias[4 + e] += b1[e]; }
    }
    // The epilogue operand (fan-in gradient, GELU' input, gate factor) of ALL of this thread's rows is requested here, before
    // the first staged row is read: inside the row loop (behind the switch on the epilogue kind) every row's load waited for
    // the previous row's store to issue -- 128 / RSTEP global-load latencies in series per thread, twice that in the two
    // passes of the 12-wave kernel.
    constexpr int NROW = ROWS / RSTEP;
    const bool use_aux = g.epi == ICKA_EPI_DGELU || g.epi == ICKA_EPI_ADD || g.epi == ICKA_EPI_GATE || g.epi == ICKA_EPI_ADD_RELU;
    u32x4 araw[NROW];
#pragma unroll
    for (int i = 0; i < NROW; ++i) {
        const int row = rb + RSTEP * i;
        const int m = (WIDE == 1 || WIDE == 2) ? m0 + ((row >> 5) << 6) + (row & 31) : m0 + row;
        araw[i] = u32x4{0u, 0u, 0u, 0u};
        if (use_aux) araw[i] = ld_once(reinterpret_cast<const u32x4*>(g.aux + (int64_t)m * g.ldaux + n));
    }
    // (the 12-wave kernel runs at a 168-register cap with accumulators of the other pass alive: keep its row loop rolled)
    constexpr int UNR = (WIDE == 1 || WIDE == 2) ? 1 : ROWS / RSTEP;
#pragma unroll UNR
    for (int i = 0; i < ROWS / RSTEP; ++i) {
        const int row = rb + RSTEP * i;
        // WIDE: the staged tile holds 32-row slabs of four 64-row wave tiles (gemm_w3_kernel): slab q -> rows 64 q + 0..31
        const int m = (WIDE == 1 || WIDE == 2) ? m0 + ((row >> 5) << 6) + (row & 31) : m0 + row;
        const u32x4 acur = araw[0];   // (constant indices: the queue stays in registers when the loop is rolled)
#pragma unroll
        for (int q = 0; q + 1 < NROW; ++q) araw[q] = araw[q + 1];
        const f32x4 lo = *reinterpret_cast<const f32x4*>(smem + (WIDE == 1 ? off_cw(row, 2 * c8) : off_c(row, 2 * c8)));
        const f32x4 hi = *reinterpret_cast<const f32x4*>(smem + (WIDE == 1 ? off_cw(row, 2 * c8 + 1) : off_c(row, 2 * c8 + 1)));
        float v[8] = {lo[0] + bias[0], lo[1] + bias[1], lo[2] + bias[2], lo[3] + bias[3],
                      hi[0] + bias[4], hi[1] + bias[5], hi[2] + bias[6], hi[3] + bias[7]};
        float a[8];
        switch (g.epi) {
            case ICKA_EPI_GELU:
                store8_bf16(g.C2 + (int64_t)m * g.ldc2 + n, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = gelu_f(v[e]);
                break;
            case ICKA_EPI_DGELU:
                cvt8_aux(acur, g.aux_f16, a);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] *= dgelu_f(a[e]);
                break;
            case ICKA_EPI_ADD:
                cvt8_aux(acur, g.aux_f16, a);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += a[e];
                break;
            case ICKA_EPI_GATE:
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = sigmoid_f(v[e]);
                if (g.C2) store8_bf16(g.C2 + (int64_t)m * g.ldc2 + n, v);
                cvt8_aux(acur, g.aux_f16, a);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] *= a[e];
                break;
            case ICKA_EPI_TANH:
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = tanhf(v[e]);
                break;
            case ICKA_EPI_ADD_RELU:
                cvt8_aux(acur, g.aux_f16, a);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e] + a[e], 0.f);
                break;
            case ICKA_EPI_RELU:
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
                break;
            default: break;
        }
        if (g.c_f32) {
            float* p = reinterpret_cast<float*>(g.C) + (int64_t)m * g.ldc + n;
            f32x4 o0 = {v[0], v[1], v[2], v[3]}, o1 = {v[4], v[5], v[6], v[7]};
            if (g.beta != 0.f) {
                o0 += g.beta * ld_once(reinterpret_cast<const f32x4*>(p));
                o1 += g.beta * ld_once(reinterpret_cast<const f32x4*>(p + 4));
            }
            if (!WIRE || !g.c3_only) {
                st_out(reinterpret_cast<f32x4*>(p), o0);
                st_out(reinterpret_cast<f32x4*>(p + 4), o1);
            }
            if constexpr (WIRE) {
                if (g.C3) {
                    const float w[8] = {o0[0], o0[1], o0[2], o0[3], o1[0], o1[1], o1[2], o1[3]};
                    store8_bf16(g.C3 + (int64_t)m * g.ldc3 + n, w);
                }
            }
        } else if (g.c_f16) {   // fp16 main output (+ optional bf16 copy); beta is rejected on the host
            store8_f16(reinterpret_cast<_Float16*>(g.C) + (int64_t)m * g.ldc + n, v, g.plain);
            if (g.C3) store8_bf16(g.C3 + (int64_t)m * g.ldc3 + n, v);
        } else {
            bf16_t* p = reinterpret_cast<bf16_t*>(g.C) + (int64_t)m * g.ldc + n;
            if (g.beta != 0.f) {
                load8_bf16(p, a);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += g.beta * a[e];
            }
            store8_bf16_main(p, v, g.plain);
        }
    }
}

}  // namespace
