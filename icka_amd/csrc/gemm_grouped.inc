// Several GEMMs in one launch (gemm_core.h, gemm_ws.inc; DESIGN.md section 4).  Kernels in this file:
//   gemm_dma_group_kernel / gemm_ws_group_kernel   up to 4 problems of one layout in one launch (128x128 tiles)
//   gemm_ws_group_red_kernel   the same with slab reductions riding along as extra blocks
//   gemm_big_group_kernel      256x128 tiles for the grouped weight gradients (8 or 12 waves, optionally over the live k-tiles
//                              only) + column-sum / slab-reduction blocks
//   slab_reduce_kernel / slab_reduce_multi_kernel   the slab reductions on their own
// A source fragment of gemm.hip, included once there.

namespace {

// Several independent GEMMs of one layout in ONE launch (the four weight-gradient GEMMs of a layer: 36..144 tiles
// each, 432 together): the chip is filled once instead of four partially filled launches.
constexpr int MAX_GROUP = 4;
struct GroupArgs {
    GemmArgs p[MAX_GROUP];
    int start[MAX_GROUP + 1];  // first block of each problem; start[n..] = total
};
template <bool A_KM, bool B_KM, int NBUF>
__global__ __launch_bounds__(256) void gemm_dma_group_kernel(const GroupArgs ga) {
    __shared__ __attribute__((aligned(16))) char smem[NBUF * 2 * TILE_BYTES];
    const int bid = blockIdx.x;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < MAX_GROUP; ++i) pi += bid >= ga.start[i] ? 1 : 0;
    const GemmArgs g = ga.p[pi];
    gemm_dma_body<A_KM, B_KM, NBUF, 0>(g, smem, bid - ga.start[pi], ga.start[pi + 1] - ga.start[pi]);
}

template <bool A_KM, bool B_KM, int NBUF>
__global__ __launch_bounds__(512) void gemm_ws_group_kernel(const GroupArgs ga) {
    __shared__ __attribute__((aligned(16))) char smem[NBUF * 2 * TILE_BYTES];
    const int bid = blockIdx.x;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < MAX_GROUP; ++i) pi += bid >= ga.start[i] ? 1 : 0;
    const GemmArgs g = ga.p[pi];
    gemm_ws_body<A_KM, B_KM, NBUF>(g, smem, bid - ga.start[pi], ga.start[pi + 1] - ga.start[pi]);
}

// =====================================================================================================================
// 256x128 output tiles for the grouped weight-gradient launch (TN, K = tokens = 4096 at c2).
// The 128x128 loop is LDS-bound: four 64x64 wave tiles read 64 KB of fragments per k-tile and the LDS-DMA writes 32 KB
// (96 KB at 128 B/clk = 768 cycles against 544 cycles of MFMA).  With 128x64 wave tiles on a 256x128 block tile the
// same four compute waves issue twice the MFMAs (1024 cycles) for 96 + 48 KB of LDS traffic (1125 cycles): per FLOP
// the LDS moves 0.73x less, and the four weight-gradient problems of a BERT layer become 216 tiles = one round of
// the 256 CUs instead of 432 tiles = two.  The bias-gradient column sums do not ride on the MFMAs here (the compute
// waves have no registers to spare: 128 accumulators + two fragment sets): they are extra blocks at the END of the
// same grid, which run on the CUs the 216 tiles leave idle and stream the dY operands once.
// Outputs are written straight from the accumulators (f32, optional beta accumulate, no epilogue operand): the only
// form the weight-gradient path needs; anything else uses the 128x128 group kernel.
constexpr int BIG_STAGE = 3 * TILE_BYTES;   // A rows 0..127 | A rows 128..255 | B   (k-major images)
constexpr int BIG_NBUF = 3;
constexpr int CS_COLS = 64;                 // operand columns per column-sum block

constexpr int MAX_RED = 4;
struct SlabRed {   // out[slot][c] (+)= sum_b partials[b*slab_stride + slot*H + c]
    const float* partials; float* out[4];
    int nslab, H, nslots, slab_stride, accumulate, blocks;
};
struct BigGroupArgs {
    GemmArgs p[MAX_GROUP];
    int start[MAX_GROUP + 1];     // first GEMM tile of each problem; start[n..] = total tiles
    int cs_start[MAX_GROUP + 1];  // first column-sum block of each problem (relative to the total tiles)
    SlabRed red[MAX_RED];         // slab reductions riding on the launch (LayerNorm dgamma / dbeta of the layer)
    int red_start[MAX_RED + 1];   // first block of each reduction (relative to tiles + column-sum blocks)
    const uint8_t* k_live[MAX_GROUP];   // LIVE instances: K bytes per problem, byte t == 0 -> row t of an operand is all zero
};

// Live k-tiles of one problem (LIVE instances of the 12-wave body).  k-tile i is live if any of its 64 flag bytes is set;
// lane i ORs the 64 bytes of k-tile base + i (four 16-byte loads) and a ballot gives the wave-uniform word of 64 k-tiles.
// Every wave of the block builds the words from the same bytes (written by an earlier kernel of the stream, not during
// the launch), so loader and compute waves walk the same tiles in the same ascending order and their barrier counts
// agree by construction.  A null pointer means every row is live.
struct LiveTiles {
    const uint8_t* flags;
    int nk, base, lane;
    uint64_t word;
    __device__ __forceinline__ uint64_t load_word() const {
        uint32_t any = 0u;
        const int t = base + lane;
        if (t < nk) {
            any = 1u;
            if (flags) {
                const u32x4* q = reinterpret_cast<const u32x4*>(flags + (int64_t)t * BK);
                const u32x4 v = (q[0] | q[1]) | (q[2] | q[3]);
                any = (v[0] | v[1]) | (v[2] | v[3]);
            }
        }
        return __ballot(any != 0u);
    }
    __device__ __forceinline__ LiveTiles(const uint8_t* f, int nk_, int lane_) : flags(f), nk(nk_), base(0), lane(lane_) {
        word = load_word();
    }
    // number of live k-tiles: what next() returns before it returns -1
    static __device__ __forceinline__ int count(const uint8_t* f, int nk, int lane) {
        LiveTiles lt(f, nk, lane);
        int n = __builtin_popcountll(lt.word);
        for (lt.base = 64; lt.base < nk; lt.base += 64) n += __builtin_popcountll(lt.load_word());
        return n;
    }
    // next live k-tile in ascending order, -1 when there is none left
    __device__ __forceinline__ int next() {
        while (word == 0) {
            if (base + 64 >= nk) return -1;
            base += 64;
            word = load_word();
        }
        const int kt = base + __builtin_ctzll(word);
        word &= word - 1;
        return kt;
    }
};

// 64 output values per block (8 slab lanes x 64 columns), fixed summation order: bitwise reproducible
__device__ __forceinline__ void slab_reduce_block(const SlabRed& r, char* smem, int rb) {
    float* red = reinterpret_cast<float*>(smem);   // [8][64]
    const int tid = threadIdx.x, cx = tid & 63, sy = tid >> 6;
    const int idx = rb * 64 + cx;
    const bool ok = idx < r.nslots * r.H;
    float s = 0.f;
    if (ok) {
        const int slot = idx / r.H, c = idx - slot * r.H;
        const float* p = r.partials + (int64_t)slot * r.H + c;
        for (int b = sy; b < r.nslab; b += 8) s += p[(int64_t)b * r.slab_stride];
    }
    red[sy * 64 + cx] = s;
    __syncthreads();
    if (sy == 0 && ok) {
        const int slot = idx / r.H, c = idx - slot * r.H;
        float* out = r.out[slot];
        if (out) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) t += red[k * 64 + cx];
            out[c] = r.accumulate ? out[c] + t : t;
        }
    }
}
__global__ __launch_bounds__(512) void slab_reduce_kernel(const SlabRed r) {
    __shared__ __attribute__((aligned(16))) char smem[8 * 64 * 4];
    slab_reduce_block(r, smem, blockIdx.x);
}
// The 128x128 group kernel with slab reductions riding along as extra blocks at the end of the grid (as on the 256x128 launch):
// a group of few tiles (the two gate weight gradients of the head: 72 tiles) leaves most CUs idle, the reductions run there.
struct GroupArgsRed { GroupArgs ga; SlabRed red[MAX_RED]; int red_start[MAX_RED + 1]; };
template <bool A_KM, bool B_KM, int NBUF>
__global__ __launch_bounds__(512) void gemm_ws_group_red_kernel(const GroupArgsRed gr) {
    __shared__ __attribute__((aligned(16))) char smem[NBUF * 2 * TILE_BYTES];
    const int bid = blockIdx.x;
    const int tiles = gr.ga.start[MAX_GROUP];
    if (bid >= tiles) {
        const int rb = bid - tiles;
        int ri = 0;
#pragma unroll
        for (int i = 1; i < MAX_RED; ++i) ri += rb >= gr.red_start[i] ? 1 : 0;
        slab_reduce_block(gr.red[ri], smem, rb - gr.red_start[ri]);
        return;
    }
    int pi = 0;
#pragma unroll
    for (int i = 1; i < MAX_GROUP; ++i) pi += bid >= gr.ga.start[i] ? 1 : 0;
    const GemmArgs g = gr.ga.p[pi];
    gemm_ws_body<A_KM, B_KM, NBUF>(g, smem, bid - gr.ga.start[pi], gr.ga.start[pi + 1] - gr.ga.start[pi]);
}
// several reductions in ONE launch (the slabs no weight-gradient launch took along: each used to pay its own launch)
struct SlabRedMulti { SlabRed red[MAX_RED]; int red_start[MAX_RED + 1]; };
__global__ __launch_bounds__(512) void slab_reduce_multi_kernel(const SlabRedMulti m) {
    __shared__ __attribute__((aligned(16))) char smem[8 * 64 * 4];
    const int rb = blockIdx.x;
    int ri = 0;
#pragma unroll
    for (int i = 1; i < MAX_RED; ++i) ri += rb >= m.red_start[i] ? 1 : 0;
    slab_reduce_block(m.red[ri], smem, rb - m.red_start[ri]);
}

// one k-tile of the 256x128 tile into ring stage BUF (both bodies: the loader wave's pa0 / pa1 / pb, strides sa / sb)
#define ICKA_BIG_STAGE(BUF)                                              \
    do {                                                                 \
        dma_issue(pa0, sa, lds0 + (BUF) + lw * 1024);                    \
        dma_issue(pa1, sa, lds0 + (BUF) + TILE_BYTES + lw * 1024);       \
        dma_issue(pb, sb, lds0 + (BUF) + 2 * TILE_BYTES + lw * 1024);    \
    } while (0)
template <bool WIRE>
__device__ __forceinline__ void gemm_big_tn_body(const GemmArgs& g, char* smem, const int m0, const int n0) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)reinterpret_cast<uintptr_t>(LDS_PTR(char, smem)));
    const int nk = g.K / BK;

    if (wave >= 4) {
        // ------------------------------------------------------------------------------------------- loader waves
        const int lw = wave - 4;
        const bf16_t* pa0[4];
        const bf16_t* pa1[4];
        const bf16_t* pb[4];
        dma_init<true>(pa0, g.A, g.lda, m0, lw, lane);
        dma_init<true>(pa1, g.A, g.lda, m0 + 128, lw, lane);
        dma_init<true>(pb, g.B, g.ldb, n0, lw, lane);
        const int64_t sa = (int64_t)BK * g.lda, sb = (int64_t)BK * g.ldb;
#pragma unroll
        for (int t = 0; t < BIG_NBUF - 1; ++t)
            if (t < nk) ICKA_BIG_STAGE(t * BIG_STAGE);
        int cur = 0;
        for (int kt = 0; kt < nk; ++kt) {
            int ahead = nk - 1 - kt;
            ahead = ahead > BIG_NBUF - 2 ? BIG_NBUF - 2 : ahead;
            if (ahead >= 1) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");   // 12 DMA per k-tile per loader wave
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (kt + BIG_NBUF - 1 < nk) {
                int nx = cur + BIG_NBUF - 1;
                nx = nx >= BIG_NBUF ? nx - BIG_NBUF : nx;
                ICKA_BIG_STAGE(nx * BIG_STAGE);
            }
            cur = cur + 1 == BIG_NBUF ? 0 : cur + 1;
        }
        return;   // outputs are stored by the compute waves straight from their accumulators
    }
    // ---------------------------------------------------------------------------------------------- compute waves
    const int wsub = wave >> 1;            // which 128-row half of the A tile
    const int wc = (wave & 1) * 64;
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 fa0[8], fb0[4], fa1[8], fb1[4];   // fragment sets of the two 32-deep k-steps of a tile
#define ICKA_BIG_READ(FA, FB, BUFI, KS)                                                                     \
    do {                                                                                                    \
        const char* b_ = smem + (BUFI) * BIG_STAGE;                                                         \
        int l_ = lane;                                                                                      \
        asm volatile("" : "+v"(l_)); /* opaque: the 48 swizzled LDS addresses are recomputed per read (a few */ \
        /* VALU ops) instead of being held in registers across the loop -- held, they spilled to scratch and */ \
        /* the serialized reloads cost ~4000 cycles per k-tile */                                           \
        _Pragma("unroll") for (int t = 0; t < 8; ++t) FA[t] = read_frag<true>(b_ + wsub * TILE_BYTES, 16 * t, KS, l_); \
        _Pragma("unroll") for (int t = 0; t < 4; ++t) FB[t] = read_frag<true>(b_ + 2 * TILE_BYTES, wc + 16 * t, KS, l_); \
    } while (0)
#define ICKA_BIG_MMA(FA, FB)                                                                                \
    do {                                                                                                    \
        _Pragma("unroll") for (int mi = 0; mi < 8; ++mi)                                                    \
            _Pragma("unroll") for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = mfma16(FB[ni], FA[mi], acc[mi][ni]); \
    } while (0)
// One scheduling region = 24 fragment reads (into the idle register set) + 32 MFMAs (from the other set): the reads
// are spread between the MFMAs (1 DS read per MFMA, then the remaining MFMAs) instead of being issued as one block
// while the matrix pipe idles -- with one compute wave per SIMD nothing else would fill those cycles.
#define ICKA_BIG_INTERLEAVE()                                                                               \
    do {                                                                                                    \
        _Pragma("unroll") for (int i_ = 0; i_ < 24; ++i_) {                                                 \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                              \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                              \
        }                                                                                                   \
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
    } while (0)
    __builtin_amdgcn_s_barrier();   // barrier #0: tile 0 published
    asm volatile("" ::: "memory");
    ICKA_BIG_READ(fa0, fb0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    int cur = 0;
    for (int kt = 0; kt + 1 < nk; ++kt) {
        ICKA_BIG_READ(fa1, fb1, cur, 1);
        ICKA_BIG_MMA(fa0, fb0);
        ICKA_BIG_INTERLEAVE();
        const int nxt = cur + 1 == BIG_NBUF ? 0 : cur + 1;
        // tile kt is completely in registers: barrier kt+1 publishes tile kt+1 and frees tile kt's buffer
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        ICKA_BIG_READ(fa0, fb0, nxt, 0);
        ICKA_BIG_MMA(fa1, fb1);
        ICKA_BIG_INTERLEAVE();
        cur = nxt;
    }
    ICKA_BIG_READ(fa1, fb1, cur, 1);   // last tile
    ICKA_BIG_MMA(fa0, fb0);
    ICKA_BIG_INTERLEAVE();
    ICKA_BIG_MMA(fa1, fb1);
    __builtin_amdgcn_sched_barrier(0);
#undef ICKA_BIG_INTERLEAVE
#undef ICKA_BIG_READ
#undef ICKA_BIG_MMA
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");   // MFMA -> VALU read wait states (see gemm_ws_body)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int n = n0 + wc + 16 * ni + 4 * (lane >> 4);
#pragma unroll
        for (int mi = 0; mi < 8; ++mi) {
            const int m = m0 + wsub * 128 + 16 * mi + (lane & 15);
            f32x4* dst = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(g.C) + (int64_t)m * g.ldc + n);
            f32x4 v = acc[mi][ni] * g.alpha;
            if (g.beta != 0.f) v += g.beta * ld_once(dst);   // gradient accumulation across micro-batches
            if (!WIRE || !g.c3_only) st_out(dst, v);
            if constexpr (WIRE) {
                if (g.C3) st_out(reinterpret_cast<u32x2*>(g.C3 + (int64_t)m * g.ldc3 + n), pack4(v[0], v[1], v[2], v[3]));
            }
        }
    }
}

// column sums of a k-major operand slice: colsum[c0 .. c0+64) (+)= sum over the K rows of A[k][m].
// 8 chunk lanes (64 columns) x 64 row lanes, 8 independent 16-byte loads in flight per thread.
__device__ __forceinline__ void big_colsum_block(const GemmArgs& g, char* smem, int cb) {
    float* red = reinterpret_cast<float*>(smem);   // [64 row lanes][64 columns]
    const int tid = threadIdx.x, cx = tid & 7, ry = tid >> 3;
    const int col = cb * CS_COLS + cx * 8;
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
    if (col < g.M) {
        const bf16_t* base = g.A + col;
        int k = ry;
        for (; k + 7 * 64 < g.K; k += 8 * 64) {
            u32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const u32x4*>(base + (int64_t)(k + 64 * u) * g.lda);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bf16x8 h = as_bf16x8(v[u]);
#pragma unroll
                for (int e = 0; e < 8; ++e) s[e] += bf2f(h[e]);
            }
        }
        for (; k < g.K; k += 64) {
            const bf16x8 h = as_bf16x8(*reinterpret_cast<const u32x4*>(base + (int64_t)k * g.lda));
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += bf2f(h[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[ry * CS_COLS + cx * 8 + e] = s[e];
    __syncthreads();
    if (tid < CS_COLS) {
        const int c = cb * CS_COLS + tid;
        if (c < g.M) {
            float t = 0.f;
#pragma unroll 8
            for (int r = 0; r < 64; ++r) t += red[r * CS_COLS + tid];
            g.colsum[c] = g.colsum_acc ? g.colsum[c] + t : t;
        }
    }
}


// 12-wave form of the same tile (8 compute waves of 64 x 64, two per SIMD, + 4 loader waves): fragments are read per
// 32-deep step right before their MFMAs and the second compute wave of the SIMD covers the LDS (ds_read_b64_tr_b16)
// latency, instead of one wave per SIMD with software-pipelined register sets.
// LIVE: the reduction runs over the live k-tiles of ``k_live`` only (LiveTiles).  A skipped tile has an all-zero operand
// tile, so the full reduction would add only +-0 products to accumulators that started at +0: the result is bitwise the
// full one whenever the other operand is finite.  No live tile at all: nothing is staged and the epilogue writes beta * C.
template <bool WIRE, bool LIVE = false>
__device__ __forceinline__ void gemm_big12_tn_body(const GemmArgs& g, char* smem, const int m0, const int n0,
                                                   const uint8_t* k_live = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)reinterpret_cast<uintptr_t>(LDS_PTR(char, smem)));
    const int nk = g.K / BK;
    if (wave >= 8) {
        const int lw = wave - 8;
        const bf16_t* pa0[4];
        const bf16_t* pa1[4];
        const bf16_t* pb[4];
        dma_init<true>(pa0, g.A, g.lda, m0, lw, lane);
        dma_init<true>(pa1, g.A, g.lda, m0 + 128, lw, lane);
        dma_init<true>(pb, g.B, g.ldb, n0, lw, lane);
        const int64_t sa = (int64_t)BK * g.lda, sb = (int64_t)BK * g.ldb;
        if constexpr (LIVE) {
            // the same ring, over the live tiles: the pointers stay at k-tile 0 and every stage adds its tile's offset
            static_assert(BIG_NBUF == 3, "the live-tile loader keeps two tiles in flight");
#define ICKA_BIG_STAGE_AT(BUF, KT)                                                       \
    do {                                                                                 \
        const int64_t oa = (KT) * sa, ob = (KT) * sb;                                    \
        dma_issue_at(pa0, oa, lds0 + (BUF) + lw * 1024);                                 \
        dma_issue_at(pa1, oa, lds0 + (BUF) + TILE_BYTES + lw * 1024);                    \
        dma_issue_at(pb, ob, lds0 + (BUF) + 2 * TILE_BYTES + lw * 1024);                 \
    } while (0)
            LiveTiles lt(k_live, nk, lane);
            int t0 = lt.next();
            int t1 = t0 >= 0 ? lt.next() : -1;
            if (t0 >= 0) ICKA_BIG_STAGE_AT(0, t0);
            if (t1 >= 0) ICKA_BIG_STAGE_AT(BIG_STAGE, t1);
            int cur = 0;
            while (t0 >= 0) {   // one barrier per live tile, as in the compute waves
                const int t2 = t1 >= 0 ? lt.next() : -1;
                if (t1 >= 0) wait_vmcnt<12>();
                else wait_vmcnt<0>();
                __builtin_amdgcn_s_barrier();
                if (t2 >= 0) {
                    int nx = cur + BIG_NBUF - 1;
                    nx = nx >= BIG_NBUF ? nx - BIG_NBUF : nx;
                    ICKA_BIG_STAGE_AT(nx * BIG_STAGE, t2);
                }
                cur = cur + 1 == BIG_NBUF ? 0 : cur + 1;
                t0 = t1;
                t1 = t2;
            }
#undef ICKA_BIG_STAGE_AT
            return;
        }
#pragma unroll
        for (int t = 0; t < BIG_NBUF - 1; ++t)
            if (t < nk) ICKA_BIG_STAGE(t * BIG_STAGE);
        int cur = 0;
        for (int kt = 0; kt < nk; ++kt) {
            int ahead = nk - 1 - kt;
            ahead = ahead > BIG_NBUF - 2 ? BIG_NBUF - 2 : ahead;
            if (ahead >= 1) wait_vmcnt<12>();   // 12 DMA per k-tile per loader wave
            else wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
            if (kt + BIG_NBUF - 1 < nk) {
                int nx = cur + BIG_NBUF - 1;
                nx = nx >= BIG_NBUF ? nx - BIG_NBUF : nx;
                ICKA_BIG_STAGE(nx * BIG_STAGE);
            }
            cur = cur + 1 == BIG_NBUF ? 0 : cur + 1;
        }
        return;
    }
    const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    int cur = 0;
#define ICKA_BIG12_TILE()                                                                                    \
    do {                                                                                                     \
        __builtin_amdgcn_s_barrier();   /* next tile published; this wave is done with the one before */     \
        asm volatile("" ::: "memory");                                                                       \
        const char* st = smem + cur * BIG_STAGE;                                                             \
        const char* sA = st + (wr >> 7) * TILE_BYTES;                                                        \
        const char* sB = st + 2 * TILE_BYTES;                                                                \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                   \
            bf16x8 fa[4], fb[4];                                                                             \
            _Pragma("unroll") for (int t = 0; t < 4; ++t) fa[t] = read_frag<true>(sA, (wr & 127) + 16 * t, ks, lane); \
            _Pragma("unroll") for (int t = 0; t < 4; ++t) fb[t] = read_frag<true>(sB, wc + 16 * t, ks, lane); \
            _Pragma("unroll") for (int mi = 0; mi < 4; ++mi)                                                 \
                _Pragma("unroll") for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = mfma16(fb[ni], fa[mi], acc[mi][ni]); \
        }                                                                                                    \
        cur = cur + 1 == BIG_NBUF ? 0 : cur + 1;                                                             \
    } while (0)
    // LIVE: the compute waves need only the NUMBER of live tiles -- as many trips (and barriers) as the loader waves make
    const int ntrip = LIVE ? LiveTiles::count(k_live, nk, lane) : nk;
    for (int kt = 0; kt < ntrip; ++kt) ICKA_BIG12_TILE();
#undef ICKA_BIG12_TILE
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int n = n0 + wc + 16 * ni + 4 * (lane >> 4);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int m = m0 + wr + 16 * mi + (lane & 15);
            f32x4* dst = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(g.C) + (int64_t)m * g.ldc + n);
            f32x4 v = acc[mi][ni] * g.alpha;
            if (g.beta != 0.f) v += g.beta * ld_once(dst);
            if (!WIRE || !g.c3_only) st_out(dst, v);
            if constexpr (WIRE) {
                if (g.C3) st_out(reinterpret_cast<u32x2*>(g.C3 + (int64_t)m * g.ldc3 + n), pack4(v[0], v[1], v[2], v[3]));
            }
        }
    }
}

#undef ICKA_BIG_STAGE

// WIRE: some problem of the group writes the data-parallel wire copy (C3); LIVE (12-wave body only): some problem of the
// group carries row-liveness flags (ga.k_live) and reduces over its live k-tiles only
template <bool W12, bool WIRE = false, bool LIVE = false>
__global__ __launch_bounds__(W12 ? 768 : 512) void gemm_big_group_kernel(const BigGroupArgs ga) {
    __shared__ __attribute__((aligned(16))) char smem[BIG_NBUF * BIG_STAGE];
    const int bid = blockIdx.x;
    const int tiles = ga.start[MAX_GROUP];
    if (bid >= tiles + ga.cs_start[MAX_GROUP]) {
        const int rb = bid - tiles - ga.cs_start[MAX_GROUP];
        int ri = 0;
#pragma unroll
        for (int i = 1; i < MAX_RED; ++i) ri += rb >= ga.red_start[i] ? 1 : 0;
        if (W12 && threadIdx.x >= 512) return;   // the helper roles are written for 8 waves
        slab_reduce_block(ga.red[ri], smem, rb - ga.red_start[ri]);
        return;
    }
    if (bid >= tiles) {
        const int cb = bid - tiles;
        int pi = 0;
#pragma unroll
        for (int i = 1; i < MAX_GROUP; ++i) pi += cb >= ga.cs_start[i] ? 1 : 0;
        const GemmArgs g = ga.p[pi];
        if (W12 && threadIdx.x >= 512) return;
        big_colsum_block(g, smem, cb - ga.cs_start[pi]);
        return;
    }
    // Block -> tile across the WHOLE group (blocks b and b+8 share an XCD and its private 4 MiB L2): XCD x takes the
    // contiguous run [x*T/8, (x+1)*T/8) of the problems' concatenated tile lists, each list ordered along its shorter
    // side.  A problem then lives on ~T_p/27 XCDs instead of all 8, each of which has to fetch the operand panels its
    // tiles touch: rocprofv3 FETCH_SIZE was 340 MB per launch against ~100 MB of operands with per-problem striping.
    const int xcd = bid & 7, slot = bid >> 3;
    const int qn = tiles >> 3, rn = tiles & 7;
    const int gt = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + slot;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < MAX_GROUP; ++i) pi += gt >= ga.start[i] ? 1 : 0;
    const GemmArgs g = ga.p[pi];
    const int local = gt - ga.start[pi];
    const int nbm = g.M / 256, nbn = g.N / BN;
    int tm, tn;
    if (nbn > nbm) { tm = local % nbm; tn = local / nbm; }
    else { tm = local / nbn; tn = local % nbn; }
    if constexpr (W12 && LIVE) gemm_big12_tn_body<WIRE, true>(g, smem, tm * 256, tn * BN, ga.k_live[pi]);
    else if constexpr (W12) gemm_big12_tn_body<WIRE>(g, smem, tm * 256, tn * BN);
    else gemm_big_tn_body<WIRE>(g, smem, tm * 256, tn * BN);
}

}  // namespace

// eligible: fast-path TN, 256-row tiles, plain f32 output (overwrite or accumulate)
static bool big_ok(const GemmArgs& g, bool aligned) {
    return aligned && g.M % 256 == 0 && g.c_f32 && g.epi == ICKA_EPI_NONE && g.K1 == 0 && !g.bias && !g.bias2 && g.direct;
}

template <bool A_KM, bool B_KM>
static int launch_group(const GroupArgs& ga, int total, hipStream_t st, const Tune& t) {
    if (t.ws) ICKA_LAUNCH_RETURN((gemm_ws_group_kernel<A_KM, B_KM, 3>), total, 512, st, ga);
    const int nbuf = t.nbuf > 0 ? t.nbuf : (total >= 448 ? 2 : 4);
    if (nbuf == 2) ICKA_LAUNCH_RETURN((gemm_dma_group_kernel<A_KM, B_KM, 2>), total, 256, st, ga);
    else if (nbuf == 3) ICKA_LAUNCH_RETURN((gemm_dma_group_kernel<A_KM, B_KM, 3>), total, 256, st, ga);
    else ICKA_LAUNCH_RETURN((gemm_dma_group_kernel<A_KM, B_KM, 4>), total, 256, st, ga);
}

static int grouped_impl(const icka_gemm_desc* descs, int32_t n, const icka_slab_reduction* reds, int32_t n_red,
                        hipStream_t st, const uint8_t* const* k_live = nullptr);

extern "C" int icka_gemm_grouped(const icka_gemm_desc* descs, int32_t n, void* stream) {
    if (!descs || n <= 0) return ICKA_E_ARG;
    return grouped_impl(descs, n, nullptr, 0, (hipStream_t)stream);
}

static int grouped_args_ok(const icka_gemm_desc* descs, int32_t n, const icka_slab_reduction* reds, int32_t n_red) {
    if (n < 0 || n_red < 0 || (n > 0 && !descs) || (n_red > 0 && !reds) || n_red > MAX_RED) return ICKA_E_ARG;
    for (int r = 0; r < n_red; ++r)
        if (!reds[r].partials || reds[r].nslab <= 0 || reds[r].H <= 0 || reds[r].nslots <= 0 || reds[r].nslots > 4 ||
            reds[r].slab_stride < (int64_t)reds[r].nslots * reds[r].H)
            return ICKA_E_ARG;
    return 0;
}

extern "C" int icka_gemm_grouped_ex(const icka_gemm_desc* descs, int32_t n, const icka_slab_reduction* reds,
                                    int32_t n_red, void* stream) {
    const int rc = grouped_args_ok(descs, n, reds, n_red);
    if (rc) return rc;
    return grouped_impl(descs, n, reds, n_red, (hipStream_t)stream);
}

// icka_gemm_grouped_ex with optional row-liveness flags per problem: k_live[i] (NULL allowed) points to K bytes, 16-byte
// aligned, byte t == 0 only if row t of one of problem i's operands is all zero.  The 12-wave 256x128 launch of TN
// problems then reduces over the k-tiles that have a live row; every other path ignores the flags and reduces over all
// of K (skipping is an optimisation, never a requirement).
extern "C" int icka_gemm_grouped_live(const icka_gemm_desc* descs, int32_t n, const icka_slab_reduction* reds,
                                      int32_t n_red, const uint8_t* const* k_live, void* stream) {
    if (k_live)
        for (int i = 0; i < n; ++i)
            if (reinterpret_cast<uintptr_t>(k_live[i]) & 15) return ICKA_E_ALIGN;
    const int rc = grouped_args_ok(descs, n, reds, n_red);
    if (rc) return rc;
    return grouped_impl(descs, n, reds, n_red, (hipStream_t)stream, k_live);
}

static SlabRed to_red(const icka_slab_reduction& r) {
    SlabRed o{};
    o.partials = r.partials;
    for (int k = 0; k < 4; ++k) o.out[k] = k < r.nslots ? r.out[k] : nullptr;
    o.nslab = r.nslab; o.H = r.H; o.nslots = r.nslots; o.slab_stride = (int)r.slab_stride; o.accumulate = r.accumulate;
    o.blocks = (r.nslots * r.H + 63) / 64;
    return o;
}

static int grouped_impl(const icka_gemm_desc* descs, int32_t n, const icka_slab_reduction* reds, int32_t n_red,
                        hipStream_t st, const uint8_t* const* k_live) {
    bool reds_done = n_red == 0;
    int i = 0;
    // the group's launch heuristics: the environment default, overridden by the FIRST problem's tune word
    // (Tune::big: 256x128 tiles for runs of eligible weight-gradient problems -- 2: 12-wave blocks, +0.9 % on the c2 step)
    Tune t = kTuneEnv;
    if (n > 0 && !tune_of(descs[0].tune, t)) return ICKA_E_ARG;
    Tune tk;   // (per-problem decode: convert() validates every problem's word)
    while (i < n) {
        if (t.big && t.ws && descs[i].op == ICKA_GEMM_TN) {
            // 256x128-tile launch for runs of eligible weight-gradient problems (+ their column-sum blocks)
            BigGroupArgs ba;
            int cnt = 0, total = 0, cs_total = 0;
            while (i + cnt < n && cnt < MAX_GROUP && descs[i + cnt].op == ICKA_GEMM_TN) {
                bool aligned = false;
                GemmArgs g;
                const int rc = convert(&descs[i + cnt], g, aligned, tk);
                if (rc) return rc;
                if (!big_ok(g, aligned)) break;
                ba.p[cnt] = g;
                ba.k_live[cnt] = k_live ? k_live[i + cnt] : nullptr;
                ba.start[cnt] = total;
                ba.cs_start[cnt] = cs_total;
                total += (g.M / 256) * (g.N / BN);
                if (g.colsum) cs_total += (g.M + CS_COLS - 1) / CS_COLS;
                ++cnt;
            }
            if (cnt >= 1 && total >= 64) {
                for (int k = cnt; k <= MAX_GROUP; ++k) { ba.start[k] = total; ba.cs_start[k] = cs_total; }
                for (int k = cnt; k < MAX_GROUP; ++k) { ba.p[k] = ba.p[0]; ba.k_live[k] = nullptr; }
                int red_total = 0;
                for (int r = 0; r < MAX_RED; ++r) {
                    ba.red_start[r] = red_total;
                    if (!reds_done && r < n_red) { ba.red[r] = to_red(reds[r]); red_total += ba.red[r].blocks; }
                    else ba.red[r] = SlabRed{};
                }
                ba.red_start[MAX_RED] = red_total;
                reds_done = true;
                bool wire = false;
                bool live = false;   // (a compile-time instance: run-time switches in these bodies cost 5-9 %)
                for (int k = 0; k < cnt; ++k) {
                    wire = wire || ba.p[k].C3 != nullptr;
                    live = live || ba.k_live[k] != nullptr;
                }
                const dim3 grid(total + cs_total + red_total);
                if (t.big == 2 && live) {
                    if (wire) hipLaunchKernelGGL((gemm_big_group_kernel<true, true, true>), grid, dim3(768), 0, st, ba);
                    else hipLaunchKernelGGL((gemm_big_group_kernel<true, false, true>), grid, dim3(768), 0, st, ba);
                } else if (t.big == 2) {
                    if (wire) hipLaunchKernelGGL((gemm_big_group_kernel<true, true>), grid, dim3(768), 0, st, ba);
                    else hipLaunchKernelGGL((gemm_big_group_kernel<true, false>), grid, dim3(768), 0, st, ba);
                } else {
                    if (wire) hipLaunchKernelGGL((gemm_big_group_kernel<false, true>), grid, dim3(512), 0, st, ba);
                    else hipLaunchKernelGGL((gemm_big_group_kernel<false, false>), grid, dim3(512), 0, st, ba);
                }
                ICKA_CHECK_LAUNCH();
                i += cnt;
                continue;
            }
        }
        // greedily pack up to MAX_GROUP consecutive fast-path problems of the same layout into one launch
        GroupArgs ga;
        int cnt = 0, total = 0;
        const int op = descs[i].op;
        while (i + cnt < n && cnt < MAX_GROUP && descs[i + cnt].op == op && !descs[i + cnt].ab_f16) {   // (fp16 problems go alone)
            bool aligned = false;
            const int rc = convert(&descs[i + cnt], ga.p[cnt], aligned, tk);
            if (rc) return rc;
            if (ga.p[cnt].colsum && !(aligned && t.ws)) return ICKA_E_ARG;
            if (!aligned) break;
            ga.start[cnt] = total;
            total += (ga.p[cnt].M / BM) * (ga.p[cnt].N / BN);
            ++cnt;
        }
        if (cnt >= 2) {
            for (int k = cnt; k <= MAX_GROUP; ++k) ga.start[k] = total;
            for (int k = cnt; k < MAX_GROUP; ++k) ga.p[k] = ga.p[0];
            int rc;
            if (op == ICKA_GEMM_TN && !reds_done && t.ws) {
                // the pending slab reductions ride on this launch (extra blocks behind the tiles)
                GroupArgsRed gr;
                gr.ga = ga;
                int red_total = 0;
                for (int r = 0; r < MAX_RED; ++r) {
                    gr.red_start[r] = red_total;
                    if (r < n_red) { gr.red[r] = to_red(reds[r]); red_total += gr.red[r].blocks; }
                    else gr.red[r] = SlabRed{};
                }
                gr.red_start[MAX_RED] = red_total;
                hipLaunchKernelGGL((gemm_ws_group_red_kernel<true, true, 3>), dim3(total + red_total), dim3(512), 0, st, gr);
                ICKA_CHECK_LAUNCH();
                reds_done = true;
                rc = 0;
            } else if (op == ICKA_GEMM_NT) rc = launch_group<false, false>(ga, total, st, t);
            else if (op == ICKA_GEMM_NN) rc = launch_group<false, true>(ga, total, st, t);
            else rc = launch_group<true, true>(ga, total, st, t);
            if (rc) return rc;
            i += cnt;
        } else {
            const int rc = icka_gemm(&descs[i], (void*)st);
            if (rc) return rc;
            ++i;
        }
    }
    if (!reds_done) {   // no 256x128 launch took them along: reduce the slabs with their own small launches
        if (n_red == 1) {
            const SlabRed sr = to_red(reds[0]);
            hipLaunchKernelGGL(slab_reduce_kernel, dim3(sr.blocks), dim3(512), 0, st, sr);
        } else {
            SlabRedMulti m;
            int total = 0;
            for (int r = 0; r < MAX_RED; ++r) {
                m.red_start[r] = total;
                if (r < n_red) { m.red[r] = to_red(reds[r]); total += m.red[r].blocks; }
                else m.red[r] = SlabRed{};
            }
            m.red_start[MAX_RED] = total;
            for (int r = n_red; r < MAX_RED; ++r) m.red_start[r] = total;   // (empty ranges behind the last real one)
            hipLaunchKernelGGL(slab_reduce_multi_kernel, dim3(total), dim3(512), 0, st, m);
        }
        ICKA_CHECK_LAUNCH();
    }
    return 0;
}
