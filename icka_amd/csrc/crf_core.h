// What the CRF kernels (crf.hip, crf_posterior.hip, crf_nbest.hip, crf_constrained.hip, crf_expect.hip, crf_sample.hip) and the chunk
// passes of metrics.hip and chunk_counts.hip share: the limits of the entries, the label-table word bits with the chunk rule, the walk over a sample's on-positions and
// the 16-lane wave primitives of the register / shuffle forms.  One definition each; everything is constexpr or forced inline.
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------------------- limits
constexpr int CRF_MAX_SC = 12288;       // S * C per sample: floats of per-position scores (48 KiB) / bytes of back-pointers in LDS
constexpr int CRF_FLAT_MAX_B = 2048;    // entries that write paths back to back: each wave sums the lengths of the samples before its own
constexpr int CRF_LIN_SC = 4096;        // S * C of the scaled linear-domain form: a_t and x_t tiles of 16 KiB each
constexpr int CRF_EXPECT_SC = CRF_LIN_SC;   // S * C of icka_crf_expect / _grad: alpha and centred-payoff tiles of 16 KiB each
constexpr int CM = 16;                  // tags of the register / shuffle forms (the reference has 13 / 15 labels)
constexpr int CRF_WORDS = 8;            // 64-position words of the kernels that keep a sample's positions on the lanes
constexpr int CRF_WORDS_MAX_S = 64 * CRF_WORDS;   // S <= 512 there
constexpr float CRF_TINY = 1e-30f;      // a normaliser of the scaled form below this: the sample is redone in the log domain

// ------------------------------------------------------------------------------------------------- label words
// label_table word of a tag id: these bits, the type id from bit 8 up (defined in metrics.hip)
constexpr uint32_t LT_DEFAULT = 1u, LT_BEGIN = 2u, LT_SKIP = 4u;

// start / term of position i of a compacted sequence from its word and the word before it
__device__ __forceinline__ void chunk_flags(uint32_t w, uint32_t wp, bool first, bool in, bool& start, bool& term) {
    const bool o = (w & LT_DEFAULT) != 0;
    const bool po = (wp & LT_DEFAULT) != 0;
    start = in && !o && (first || po || (w >> 8) != (wp >> 8) || (w & LT_BEGIN) != 0);
    term = in && (o || start);
}

// ---------------------------------------------------------------------------------------------- wave primitives
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// the chain advances at position t: position 0 always, t >= 1 where mask != 0 (A: an args struct with mask [B, S] and S)
template <class A>
__device__ __forceinline__ bool on_pos(const A& a, int b, int t) {
    return t == 0 || a.mask == nullptr || a.mask[(int64_t)b * a.S + t] != 0;
}

// The on-positions of a sample as a bit set in LDS, s_on[t / 64] bit t % 64 (bits at or past S clear): a recursion finds its
// next position with a bit scan, so it can fetch that position's operands one step ahead.
typedef unsigned long long u64;
// the first on-position after t, or S (wave-uniform)
__device__ __forceinline__ int next_on(const u64* s_on, int t, int S) {
    const int q = t + 1;
    if (q >= S) return S;
    const int nw = (S + 63) >> 6;
    int k = q >> 6;
    u64 m = s_on[k] & (~0ull << (q & 63));
    while (m == 0ull) {
        if (++k >= nw) return S;
        m = s_on[k];
    }
    return __builtin_amdgcn_readfirstlane(k * 64 + __builtin_ctzll(m));
}
// the last on-position before t >= 1 (position 0 is always on; wave-uniform)
__device__ __forceinline__ int prev_on(const u64* s_on, int t) {
    const int q = t - 1;
    int k = q >> 6;
    u64 m = s_on[k] & (~0ull >> (63 - (q & 63)));
    while (m == 0ull && k > 0) m = s_on[--k];
    return __builtin_amdgcn_readfirstlane(k * 64 + 63 - __builtin_clzll(m | 1ull));
}

// 16-lane row reductions on the DPP path (row_ror: no LDS crossbar, ~4 VALU ops): every lane of the row gets the result
__device__ __forceinline__ float sum16(float v) {
    v += dpp_row<0x128>(v);   // row_ror:8
    v += dpp_row<0x124>(v);   // row_ror:4
    v += dpp_row<0x122>(v);   // row_ror:2
    v += dpp_row<0x121>(v);   // row_ror:1
    return v;
}
__device__ __forceinline__ float max16(float v) {
    v = fmaxf(v, dpp_row<0x128>(v));
    v = fmaxf(v, dpp_row<0x124>(v));
    v = fmaxf(v, dpp_row<0x122>(v));
    v = fmaxf(v, dpp_row<0x121>(v));
    return v;
}
// sum_i (value of lane i) * col[i]
__device__ __forceinline__ float dot_shfl(float x, const float (&col)[CM]) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int i = 0; i < CM; i += 4) {
        s0 = fmaf(lane_f32(x, i), col[i], s0);
        s1 = fmaf(lane_f32(x, i + 1), col[i + 1], s1);
        s2 = fmaf(lane_f32(x, i + 2), col[i + 2], s2);
        s3 = fmaf(lane_f32(x, i + 3), col[i + 3], s3);
    }
    return (s0 + s1) + (s2 + s3);
}
