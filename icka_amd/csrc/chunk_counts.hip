// Per-path, per-sample chunk counts (icka_chunk_counts): (correct_preds, total_preds, total_correct, bad) of every sample
// for each of R path rows against one set of gold labels -- what turns an N-best list or a set of sampled paths into a
// per-candidate F1 cost.  The rules are icka_chunk_eval's (metrics.hip; written out in include/icka_hip.h): the kept
// positions, the skip bit, start / term (chunk_flags, crf_core.h) and the bad-sample rule.
//
// ONE WAVE PER (sample, row): grid (B, R), position t = 64 * k + lane for k = 0 .. 7 (S <= 512), the steps of metrics.hip:
//   1. n0 = first zero of the output mask; the kept positions are compacted in order into LDS (their label-table words).
//   2. start / term on the compacted sequences; the ballots of term are wave-uniform words, so the end of a chunk is a
//      find-first-set over them.
//   3. The three counts are popcounts of ballots: no atomics, and the four words of (row, sample) are WRITTEN.
// No id is used as an index unchecked; a path id outside [0, L) -- the -1 of a rank an N-best sample does not have -- makes
// the sample bad: (0, 0, 0, 1).  No host sync, no allocation: capturable.
#include "crf_core.h"

namespace {

constexpr int CC_MAX_S = CRF_WORDS_MAX_S;
constexpr int CC_MAX_L = 64;           // tag ids
constexpr int CC_MAX_TYPES = 32;
constexpr int CC_MAX_R = 64;           // path rows

struct ChunkCountsArgs {
    const int32_t* lens; const int32_t* flat; int64_t capacity; int64_t ld_tags;
    const int64_t* labels; const int64_t* mask;
    const int32_t* table;
    int32_t* counts;
    int B, S, L;
};

__global__ __launch_bounds__(64) void chunk_counts_kernel(const ChunkCountsArgs a) {
    __shared__ uint32_t s_table[CC_MAX_L];
    __shared__ uint32_t s_g[CC_MAX_S], s_p[CC_MAX_S];   // compacted label-table words: gold, predicted
    __shared__ unsigned long long s_either[CRF_WORDS], s_both[CRF_WORDS];
    const int b = blockIdx.x, r = blockIdx.y, lane = threadIdx.x, S = a.S, L = a.L;
    s_table[lane] = lane < L ? (uint32_t)a.table[lane] : 0u;
    int32_t* out = a.counts + ((int64_t)r * a.B + b) * 4;

    long long off = 0;
    for (int q = lane; q < b; q += 64) off += a.lens[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
    const int plen = a.lens[b];
    const int64_t* lab = a.labels + (int64_t)b * S;
    const int64_t* msk = a.mask + (int64_t)b * S;
    const int32_t* path = a.flat + (int64_t)r * a.ld_tags;

    // ---- 1. the kept positions
    int64_t gold[CRF_WORDS];
    int n0 = S;
#pragma unroll
    for (int k = CRF_WORDS - 1; k >= 0; --k) {
        const int t = 64 * k + lane;
        const bool in = t < S;
        gold[k] = in ? lab[t] : 0;
        const unsigned long long z = __ballot(in && msk[t] == 0);
        if (z) n0 = 64 * k + __builtin_ctzll(z);
    }
    __syncthreads();   // block = one wave: the table is in LDS
    // a path shorter than n0 (or a length table that does not fit the buffer) is never read
    bool bad = plen < n0 || off < 0 || off + n0 > a.capacity;
    uint32_t gw[CRF_WORDS];
#pragma unroll
    for (int k = 0; k < CRF_WORDS; ++k) {
        const int t = 64 * k + lane;
        const bool in = t < n0;
        const bool g_ok = gold[k] >= 0 && gold[k] < L;
        bad = bad || (in && !g_ok);
        gw[k] = (in && g_ok) ? s_table[(int)gold[k]] : LT_SKIP;
    }
    bad = __ballot(bad) != 0ull;
    int n = 0;   // kept positions so far = the compacted index of the next one
#pragma unroll
    for (int k = 0; k < CRF_WORDS; ++k) {
        const int t = 64 * k + lane;
        const bool kept = t < n0 && !(gw[k] & LT_SKIP) && !bad;
        int p = 0;
        if (kept) p = path[off + t];
        const bool p_ok = p >= 0 && p < L;
        bad = bad || (kept && !p_ok);
        const unsigned long long km = __ballot(kept);
        if (kept) {
            const int i = n + __popcll(km & lanes_below(lane));
            s_g[i] = gw[k];
            s_p[i] = p_ok ? s_table[p] : 0u;
        }
        n += __popcll(km);
    }
    if (__ballot(bad) != 0ull) {   // wave-uniform
        if (lane < 4) out[lane] = lane == 3 ? 1 : 0;
        return;
    }
    __syncthreads();   // block = one wave: the compacted sequences are in LDS

    // ---- 2. chunk starts and ends on the compacted sequences
    uint32_t cand = 0u;   // bit k: both sides start a chunk of one type at position 64 * k + lane
    int golds = 0, preds = 0, correct = 0;
#pragma unroll
    for (int k = 0; k < CRF_WORDS; ++k) {
        const int i = 64 * k + lane;
        const bool in = i < n;
        const uint32_t g = in ? s_g[i] : 0u, p = in ? s_p[i] : 0u;
        const uint32_t gp = (in && i > 0) ? s_g[i - 1] : 0u, pp = (in && i > 0) ? s_p[i - 1] : 0u;
        bool sg, tg, sp, tp;
        chunk_flags(g, gp, i == 0, in, sg, tg);
        chunk_flags(p, pp, i == 0, in, sp, tp);
        const unsigned long long mtg = __ballot(tg), mtp = __ballot(tp);
        if (lane == 0) { s_either[k] = mtg | mtp; s_both[k] = mtg & mtp; }
        cand |= (sg && sp && (g >> 8) == (p >> 8)) ? (1u << k) : 0u;
        golds += __popcll(__ballot(sg));
        preds += __popcll(__ballot(sp));
    }
    __syncthreads();   // block = one wave: the term words are in LDS
#pragma unroll
    for (int k = 0; k < CRF_WORDS; ++k) {
        // the first term of either side after position 64 * k + lane; none: both chunks run to the end of the sequence
        bool found = false, ok = true;
#pragma unroll
        for (int q = k; q < CRF_WORDS; ++q) {
            unsigned long long w = s_either[q];
            if (q == k) w &= ~(lanes_below(lane) | (1ull << lane));
            if (!found && w) {
                found = true;
                ok = (s_both[q] >> __builtin_ctzll(w)) & 1ull;
            }
        }
        correct += __popcll(__ballot(((cand >> k) & 1u) && ok));
    }
    if (lane < 4) out[lane] = lane == 0 ? correct : lane == 1 ? preds : lane == 2 ? golds : 0;
}

}  // namespace

extern "C" int icka_chunk_counts(const int32_t* lens, const int32_t* tags_flat, int64_t capacity, int64_t ld_tags, int32_t R,
                                 const int64_t* labels, const int64_t* output_mask, const int32_t* label_table,
                                 int32_t* counts, int32_t B, int32_t S, int32_t L, int32_t ntypes, void* stream) {
    if (!lens || !tags_flat || !labels || !output_mask || !label_table || !counts) return ICKA_E_ARG;
    if (B <= 0 || B > CRF_FLAT_MAX_B || S <= 0 || S > CC_MAX_S || L <= 0 || L > CC_MAX_L || R <= 0 || R > CC_MAX_R
        || ntypes <= 0 || ntypes > CC_MAX_TYPES)
        return ICKA_E_SHAPE;
    if (capacity < 0) return ICKA_E_SHAPE;
    if (ld_tags < capacity) return ICKA_E_ARG;
    ChunkCountsArgs a{};
    a.lens = lens; a.flat = tags_flat; a.capacity = capacity; a.ld_tags = ld_tags;
    a.labels = labels; a.mask = output_mask; a.table = label_table; a.counts = counts;
    a.B = B; a.S = S; a.L = L;
    hipLaunchKernelGGL(chunk_counts_kernel, dim3(B, R), dim3(64), 0, (hipStream_t)stream, a);
    ICKA_CHECK_LAUNCH();
    return 0;
}
