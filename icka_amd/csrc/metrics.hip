// Chunk-level scoring of the dev / test passes on the device (icka_chunk_eval): the counts behind the reference's accuracy /
// precision / recall / F1, overall and per entity type -- the per-token loop of My_cross_attention.py:882-903 followed by
// ner_evaluate.py `evaluate` (:64-110) and `evaluate_each_class` (:112-148), both built on `get_chunks` (:4-48).
//
// ONE WAVE PER SAMPLE (block = 64 lanes), position t = 64 * k + lane for k = 0 .. 7 (S <= 512), every loop over k unrolled so
// that the per-word values stay in registers:
//   1. n0 = first zero of the output mask (a ballot per 64 positions); the kept positions are t < n0 whose gold label does not
//      carry the skip bit.  They are compacted in order into LDS (their label-table words): the rank of a kept position is
//      the popcount of the ballots below it.
//   2. On the compacted sequences every lane derives start / term of its positions from the words at i and i - 1; the ballots
//      of term (gold, predicted) are wave-uniform 64-bit words, so the end of a chunk is a find-first-set over them and no lane
//      ever walks the sequence.  A predicted chunk is correct when both sides start at i with one type and the first term
//      after i is a term of BOTH sides (or neither side has one: both chunks run to the end).
//   3. Per-type counts go through LDS atomics, then one 64-bit global atomic add per non-zero counter: integer sums, so the
//      table does not depend on the order of the blocks and a graph replay equals an eager call exactly.
// No host sync, no allocation: capturable.
#include "crf_core.h"

namespace {

constexpr int CE_WORDS = 8;            // 64-position words per sample: S <= 512
constexpr int CE_MAX_S = 64 * CE_WORDS;
constexpr int CE_MAX_L = 64;           // tag ids (the CRF's own cap)
constexpr int CE_MAX_TYPES = 32;
constexpr int CE_HEAD = 6;             // kept_tokens, equal_tokens, correct_preds, total_preds, total_correct, bad_ids

// label_table word of a tag id: the bits LT_DEFAULT / LT_BEGIN / LT_SKIP (crf_core.h), the type id from bit 8 up

struct ChunkEvalArgs {
    const int32_t* lens; const int32_t* flat; int64_t capacity;   // form (a): the paths back to back
    const int64_t* pred; int64_t ld_pred;                          // form (b): padded [B, S]
    const int64_t* labels; const int64_t* mask;                    // [B, S]
    const int32_t* table;                                          // [L]
    unsigned long long* counters;                                  // [CE_HEAD + 3 * ntypes]
    int B, S, L, ntypes;
};

__device__ __forceinline__ void add_counter(unsigned long long* p, unsigned long long v) {
    if (v) atomicAdd(p, v);
}

__global__ __launch_bounds__(64) void chunk_eval_kernel(const ChunkEvalArgs a) {
    __shared__ uint32_t s_table[CE_MAX_L];
    __shared__ uint32_t s_g[CE_MAX_S], s_p[CE_MAX_S];   // compacted label-table words: gold, predicted
    __shared__ int s_cnt[3 * CE_MAX_TYPES];             // per type: correct, preds, golds
    __shared__ unsigned long long s_either[CE_WORDS], s_both[CE_WORDS];   // per 64 positions: term of either / of both sides
    const int b = blockIdx.x, lane = threadIdx.x, S = a.S, L = a.L;
    s_table[lane] = lane < L ? (uint32_t)a.table[lane] : 0u;
    for (int i = lane; i < 3 * CE_MAX_TYPES; i += 64) s_cnt[i] = 0;

    // form (a): where this sample's path starts (exclusive prefix sum of the lengths) and how long it is
    long long off = 0;
    int plen = S;
    if (a.lens) {
        for (int r = lane; r < b; r += 64) off += a.lens[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
        plen = a.lens[b];
    }
    const int64_t* lab = a.labels + (int64_t)b * S;
    const int64_t* msk = a.mask + (int64_t)b * S;

    // ---- 1. the kept positions
    int64_t gold[CE_WORDS];
    int n0 = S;
#pragma unroll
    for (int k = CE_WORDS - 1; k >= 0; --k) {
        const int t = 64 * k + lane;
        const bool in = t < S;
        gold[k] = in ? lab[t] : 0;
        const unsigned long long z = __ballot(in && msk[t] == 0);
        if (z) n0 = 64 * k + __builtin_ctzll(z);
    }
    __syncthreads();   // block = one wave: the table is in LDS
    // a path shorter than n0 (or a length table that does not fit the buffer) is never read
    bool bad = a.lens != nullptr && (plen < n0 || off < 0 || off + n0 > a.capacity);
    uint32_t gw[CE_WORDS];
    int equal = 0;
#pragma unroll
    for (int k = 0; k < CE_WORDS; ++k) {
        const int t = 64 * k + lane;
        const bool in = t < n0;
        const bool g_ok = gold[k] >= 0 && gold[k] < L;
        bad = bad || (in && !g_ok);
        gw[k] = (in && g_ok) ? s_table[(int)gold[k]] : LT_SKIP;
    }
    bad = __ballot(bad) != 0ull;
    int n = 0;   // kept positions so far = the compacted index of the next one
#pragma unroll
    for (int k = 0; k < CE_WORDS; ++k) {
        const int t = 64 * k + lane;
        const bool kept = t < n0 && !(gw[k] & LT_SKIP) && !bad;
        int64_t p = 0;
        if (kept) p = a.lens ? (int64_t)a.flat[off + t] : a.pred[(int64_t)b * a.ld_pred + t];
        const bool p_ok = p >= 0 && p < L;
        bad = bad || (kept && !p_ok);
        const unsigned long long km = __ballot(kept);
        if (kept) {
            const int i = n + __popcll(km & lanes_below(lane));
            s_g[i] = gw[k];
            s_p[i] = p_ok ? s_table[(int)p] : 0u;
        }
        n += __popcll(km);
        equal += __popcll(__ballot(kept && p == gold[k]));
    }
    if (__ballot(bad) != 0ull) {   // wave-uniform: the sample counts one bad_ids and nothing else
        if (lane == 0) atomicAdd(a.counters + 5, 1ull);
        return;
    }
    __syncthreads();   // block = one wave: the compacted sequences are in LDS

    // ---- 2. chunk starts and ends on the compacted sequences
    const int tmax = a.ntypes - 1;
    uint32_t cand = 0u;   // bit k: both sides start a chunk of one type at position 64 * k + lane (a VGPR, not 8 lane masks)
    int gtype[CE_WORDS];
#pragma unroll
    for (int k = 0; k < CE_WORDS; ++k) {
        const int i = 64 * k + lane;
        const bool in = i < n;
        const uint32_t g = in ? s_g[i] : 0u, p = in ? s_p[i] : 0u;
        const uint32_t gp = (in && i > 0) ? s_g[i - 1] : 0u, pp = (in && i > 0) ? s_p[i - 1] : 0u;
        bool sg, tg, sp, tp;
        chunk_flags(g, gp, i == 0, in, sg, tg);
        chunk_flags(p, pp, i == 0, in, sp, tp);
        const unsigned long long mtg = __ballot(tg), mtp = __ballot(tp);
        if (lane == 0) { s_either[k] = mtg | mtp; s_both[k] = mtg & mtp; }
        const int ty_g = min((int)(g >> 8), tmax), ty_p = min((int)(p >> 8), tmax);
        gtype[k] = ty_g;
        cand |= (sg && sp && (g >> 8) == (p >> 8)) ? (1u << k) : 0u;
        if (sg) atomicAdd(&s_cnt[3 * ty_g + 2], 1);
        if (sp) atomicAdd(&s_cnt[3 * ty_p + 1], 1);
    }
    __syncthreads();   // block = one wave: the term words are in LDS
#pragma unroll
    for (int k = 0; k < CE_WORDS; ++k) {
        // the first term of either side after position 64 * k + lane; none: both chunks run to the end of the sequence
        bool found = false, ok = true;
#pragma unroll
        for (int q = k; q < CE_WORDS; ++q) {
            unsigned long long w = s_either[q];
            if (q == k) w &= ~(lanes_below(lane) | (1ull << lane));
            if (!found && w) {
                found = true;
                ok = (s_both[q] >> __builtin_ctzll(w)) & 1ull;
            }
        }
        const bool correct = ((cand >> k) & 1u) && ok;
        if (correct) atomicAdd(&s_cnt[3 * gtype[k]], 1);
    }
    __syncthreads();   // block = one wave: the per-type counts are complete

    // ---- 3. one 64-bit atomic add per non-zero counter
    if (lane < 3) {   // the overall counts = the sums over the types (lane 0: correct, 1: preds, 2: golds)
        int tot = 0;
        for (int t = 0; t < a.ntypes; ++t) tot += s_cnt[3 * t + lane];
        add_counter(a.counters + 2 + lane, (unsigned long long)tot);
    }
    if (lane == 0) {
        add_counter(a.counters + 0, (unsigned long long)n);
        add_counter(a.counters + 1, (unsigned long long)equal);
    }
    for (int i = lane; i < 3 * a.ntypes; i += 64) add_counter(a.counters + CE_HEAD + i, (unsigned long long)s_cnt[i]);
}

// acc[0] += loss (the f32 converts exactly), acc[1] += 1: the dev loop's `dev_total_loss += loss.item(); index += 1`
__global__ __launch_bounds__(64) void loss_accumulate_kernel(const float* loss, double* acc) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        acc[0] += (double)loss[0];
        acc[1] += 1.0;
    }
}

}  // namespace

extern "C" int icka_chunk_eval(const int32_t* lens, const int32_t* tags_flat, int64_t capacity, const int64_t* pred,
                               int64_t ld_pred, const int64_t* labels, const int64_t* output_mask,
                               const int32_t* label_table, int64_t* counters, int32_t B, int32_t S, int32_t L,
                               int32_t ntypes, void* stream) {
    if (!labels || !output_mask || !label_table || !counters) return ICKA_E_ARG;
    if ((lens == nullptr) != (tags_flat == nullptr)) return ICKA_E_ARG;
    if ((lens != nullptr) == (pred != nullptr)) return ICKA_E_ARG;   // exactly one form of the predictions
    if (B <= 0 || S <= 0 || S > CE_MAX_S || L <= 0 || L > CE_MAX_L || ntypes <= 0 || ntypes > CE_MAX_TYPES)
        return ICKA_E_SHAPE;
    if (lens && capacity < 0) return ICKA_E_SHAPE;
    if (pred && ld_pred < S) return ICKA_E_ARG;
    ChunkEvalArgs a{};
    a.lens = lens; a.flat = tags_flat; a.capacity = capacity; a.pred = pred; a.ld_pred = ld_pred;
    a.labels = labels; a.mask = output_mask; a.table = label_table;
    a.counters = reinterpret_cast<unsigned long long*>(counters);
    a.B = B; a.S = S; a.L = L; a.ntypes = ntypes;
    hipLaunchKernelGGL(chunk_eval_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_loss_accumulate(const float* loss, double* acc, void* stream) {
    if (!loss || !acc) return ICKA_E_ARG;
    hipLaunchKernelGGL(loss_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss, acc);
    ICKA_CHECK_LAUNCH();
    return 0;
}
