// N-best decoding of the linear-chain CRF (icka_crf_nbest): per sample the K distinct tag paths of highest score, by
// non-increasing score, with the tie rule pinned in include/icka_hip.h (equal scores: the path whose REVERSED tag sequence is
// lexicographically smaller comes first; rank 0 is icka_crf_score_decode's path).
//
// ONE WAVE PER SAMPLE over the on-positions (position 0 and every t >= 1 with mask != 0), compacted with the ballots of
// crf_posterior.hip.  K-list Viterbi: every (position, tag) keeps its K best prefix scores, sorted.  Adding trans[p][c] keeps
// the list of predecessor p sorted, so the K best candidates of tag c are a K-WAY MERGE of the C sorted lists, not a sort:
//   lane = 4 * c + q: tag c (16 tags), quarter q; the lane holds the heads of the lists of the predecessors p = q, q + 4,
//     q + 8, q + 12 (value and rank) and, prefetched from LDS, the entry behind each head;
//   one round = the lane's best head (ties: the smaller p), a maximum over the 4 lanes of the tag on the DPP quad_perm path
//     carrying (score, 8 p + r) (ties: the smaller index, i.e. ascending (previous tag, previous rank)), and the one lane that
//     owns the winning list moves that head on; min(K, candidates) rounds per position.
//   The running lists ping-pong between two [16][8] f32 tiles in LDS (1 KiB); one byte of back-pointer 8 p + r per
//   (position, tag, rank): S * C * K <= 49152 bytes of static LDS.
// Every tag of a position has the same number of valid ranks, min(K, C^i): kept as one wave-uniform counter that is
// multiplied stepwise and clipped at K (C^L overflows).  The final selection is the same merge with end[] in place of a
// transition column (ties: ascending (tag, rank)); then lane r walks the back-pointers of rank r.
// Tags and ranks read back from the back-pointers are clamped into range before they index anything: on non-finite input the
// paths are meaningless but no access leaves the sample's own segment.  All global stores are ordinary vector stores.
#include <math.h>

#include "crf_core.h"

namespace {

constexpr int NB_MAX_C = 16;
constexpr int NB_MAX_K = 8;
constexpr int NB_BP_BYTES = 49152;      // S * C * K

struct NbestArgs {
    const float* e; int64_t ld;
    const int64_t* mask;
    const float* start; const float* end; const float* trans;
    int32_t* lens; int32_t* n_paths; float* scores; int32_t* flat; int64_t cap;
    int B, S, C, K;
};

template <int CTRL>
__device__ __forceinline__ int nb_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }

// (bs, bi) <- the better of it and the pair of the lane that the quad permutation CTRL names: higher score, then lower index
template <int CTRL>
__device__ __forceinline__ void nb_quad_best(float& bs, int& bi) {
    const float os = __builtin_bit_cast(float, nb_dpp<CTRL>(__builtin_bit_cast(int, bs)));
    const int oi = nb_dpp<CTRL>(bi);
    const bool take = (os > bs) | ((os == bs) & (oi < bi));   // (no short circuit: it compiles to branches)
    bs = take ? os : bs;
    bi = take ? oi : bi;
}

// The K-way merge of one target: `rounds` best of prev[p][r] + T[p] over p < C, r < cnt, in order; sink(k, score, 8 p + r)
// is called by every lane with the result of its own quad.  prev: [16][K] f32 in LDS.  T[m] belongs to predecessor q + 4 m
// (-inf for p >= C).
template <class SINK>
__device__ __forceinline__ void nb_merge(const float* prev, int K, int C, int cnt, int rounds, int q, const float (&T)[4],
                                         const SINK& sink) {
    // Every LDS read below is UNCONDITIONAL at an index clamped into the [16][8] tile and its value is dropped by a select
    // where it does not count: a guarded read compiles to a branch with its own wait, one after the other on the chain.
    constexpr int LAST = NB_MAX_C * NB_MAX_K - 1;
    float v[4], n[4];
    int h[4];
    float x0[4], x1[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int p = q + 4 * m;            // p * K + 1 <= 15 * 8 + 1
        x0[m] = prev[p * K];
        x1[m] = prev[p * K + 1];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const bool ok = q + 4 * m < C;
        h[m] = 0;
        v[m] = ok ? x0[m] + T[m] : -INFINITY;                    // cnt >= 1
        n[m] = (ok && 1 < cnt) ? x1[m] + T[m] : -INFINITY;
    }
    // the word fetched in one round is consumed in the next, after that round's reduction: its LDS latency is off the chain
    float xp = 0.f;      // prev[..] fetched for list pm of this lane (pm < 0: none pending); pmore: it is a valid rank
    int pm = -1;
    bool pmore = false;
    for (int k = 0; k < rounds; ++k) {
        float bs = v[0];
        int bi = 8 * q + h[0];
#pragma unroll
        for (int m = 1; m < 4; ++m)
            if (v[m] > bs) { bs = v[m]; bi = 8 * (q + 4 * m) + h[m]; }
        nb_quad_best<0xB1>(bs, bi);   // quad_perm [1, 0, 3, 2]
        nb_quad_best<0x4E>(bs, bi);   // quad_perm [2, 3, 0, 1]
        sink(k, bs, bi);
#pragma unroll
        for (int m = 0; m < 4; ++m)        // (xp + T[m] per m, not T[pm]: a selected T becomes an indexed array in scratch)
            n[m] = pm == m ? (pmore ? xp + T[m] : -INFINITY) : n[m];
        // the winner is rank r of list wp: the lane that owns the list moves its head on to r + 1 (in n) and fetches
        // r + 2; the other lanes fetch the same word and drop it
        const int wp = bi >> 3, r = bi & 7;
        const bool own = (wp & 3) == q;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const bool adv = own & ((wp >> 2) == m);
            h[m] += adv ? 1 : 0;
            v[m] = adv ? n[m] : v[m];
        }
        xp = prev[min(wp * K + r + 2, LAST)];
        pm = own ? (wp >> 2) : -1;
        pmore = (wp < C) & (r + 2 < cnt);
    }
}

__global__ __launch_bounds__(64) void crf_nbest_kernel(const NbestArgs a) {
    __shared__ unsigned char s_bp[NB_BP_BYTES];
    __shared__ float s_sc[2][NB_MAX_C * NB_MAX_K];
    __shared__ unsigned short s_pos[CRF_WORDS_MAX_S];
    __shared__ int s_fin[NB_MAX_K];
    const int b = blockIdx.x, lane = threadIdx.x, S = a.S, C = a.C, K = a.K;
    const int c = lane >> 2, q = lane & 3;

    // the on-positions, compacted in order (crf_posterior.hip)
    // (mask loads go out unconditionally at clamped indices, eight in flight, and are dropped by a select: a guarded load
    // compiles to a branch that waits for it)
    int64_t mw[CRF_WORDS];
#pragma unroll
    for (int w = 0; w < CRF_WORDS; ++w) mw[w] = a.mask ? a.mask[(int64_t)b * S + min(64 * w + lane, S - 1)] : 1;
    int L = 0;
#pragma unroll
    for (int w = 0; w < CRF_WORDS; ++w) {
        const int t = 64 * w + lane;
        const bool on = t < S && (t == 0 || mw[w] != 0);
        const unsigned long long km = __ballot(on);
        if (on) s_pos[L + __popcll(km & lanes_below(lane))] = (unsigned short)t;
        L += __popcll(km);
    }
    // sum of the path lengths of the samples before this one: b + the non-zero mask entries at their positions >= 1
    long long off = (long long)b * S;
    if (a.mask != nullptr) {
        const int n = b * S;   // <= 2^20
        int nz = 0;
        for (int base = 0; base < n; base += 64 * CRF_WORDS) {
#pragma unroll
            for (int u = 0; u < CRF_WORDS; ++u) mw[u] = a.mask[min(base + 64 * u + lane, n - 1)];
#pragma unroll
            for (int u = 0; u < CRF_WORDS; ++u) nz += (base + 64 * u + lane < n && mw[u] != 0) ? 1 : 0;
        }
        for (int r = lane; r < b; r += 64) nz -= a.mask[(int64_t)r * S] != 0 ? 1 : 0;   // position 0 counts whatever its mask says
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nz += __shfl_xor(nz, o, 64);
        off = (long long)b + nz;
    }
    __syncthreads();   // block = one wave: the positions are in LDS

    if (lane == 0) a.lens[b] = L;
    // a sample this kernel cannot serve (the entry's checks exclude both): no paths
    if (off + L > a.cap || (long long)L * C * K > NB_BP_BYTES) {
        if (lane == 0) a.n_paths[b] = 0;
        if (lane < K) a.scores[(int64_t)b * K + lane] = -INFINITY;
        for (int r = 0; r < K; ++r)
            for (int i = lane; i < L; i += 64)
                if (off + i < a.cap) a.flat[(int64_t)r * a.cap + off + i] = -1;
        return;
    }

    const bool tag_on = c < C;
    const int cc = min(c, C - 1);
    const float* eb = a.e + (int64_t)b * S * a.ld;
    float T[4], Tend[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {          // (loaded at clamped indices, then selected: ten loads in flight)
        const int pc = min(q + 4 * m, C - 1);
        T[m] = a.trans[pc * C + cc];
        Tend[m] = a.end[pc];
    }
    const float s0 = a.start[cc] + eb[cc];   // position 0 is on-position 0
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const bool ok = q + 4 * m < C;
        T[m] = (tag_on && ok) ? T[m] : -INFINITY;
        Tend[m] = ok ? Tend[m] : -INFINITY;
    }
    const bool writer = tag_on && q == 0;
    if (writer) s_sc[0][c * K] = s0;
    // emissions one step ahead of the chain, their positions two steps ahead; every lane loads (clamped: no branch, no wait)
    float en = eb[(int64_t)s_pos[min(1, L - 1)] * a.ld + cc];
    int pn = s_pos[min(2, L - 1)];
    int cnt = 1, cur = 0;
    for (int i = 1; i < L; ++i) {
        const float et = en;
        en = eb[(int64_t)pn * a.ld + cc];          // the row of on-position min(i + 1, L - 1)
        pn = s_pos[min(i + 2, L - 1)];
        const int cnt_new = min(K, cnt * C);
        __syncthreads();   // block = one wave: the lists of position i - 1 are in LDS
        float* nxt = s_sc[cur ^ 1];
        unsigned char* bp = s_bp + (i * C + c) * K;
        nb_merge(s_sc[cur], K, C, cnt, cnt_new, q, T, [&](int k, float bs, int bi) {
            if (writer) {
                nxt[c * K + k] = bs + et;
                bp[k] = (unsigned char)bi;
            }
        });
        cnt = cnt_new;
        cur ^= 1;
    }
    const int np = min(K, cnt * C);
    __syncthreads();   // block = one wave: the lists of the last position are in LDS
    nb_merge(s_sc[cur], K, C, cnt, np, q, Tend, [&](int k, float bs, int bi) {
        if (lane == 0) {
            a.scores[(int64_t)b * K + k] = bs;
            s_fin[k] = bi;
        }
    });
    if (lane == 0) a.n_paths[b] = np;
    if (lane >= np && lane < K) a.scores[(int64_t)b * K + lane] = -INFINITY;
    __syncthreads();   // block = one wave: the final (tag, rank) pairs are in LDS
    // lane r < np walks the back-pointers of rank r
    if (lane < np) {
        int32_t* out = a.flat + (int64_t)lane * a.cap + off;
        int bi = s_fin[lane];
        for (int i = L - 1; i >= 0; --i) {
            const int tag = min(bi >> 3, C - 1), r = min(bi & 7, K - 1);
            out[i] = tag;
            if (i > 0) bi = s_bp[(i * C + tag) * K + r];
        }
    }
    // the missing ranks
    for (int r = np; r < K; ++r) {
        int32_t* out = a.flat + (int64_t)r * a.cap + off;
        for (int i = lane; i < L; i += 64) out[i] = -1;
    }
}

}  // namespace

extern "C" int icka_crf_nbest(const float* emissions, int64_t ld, const int64_t* mask, const float* start, const float* end,
                              const float* trans, int32_t nbest, int32_t* lens, int32_t* n_paths, float* scores,
                              int32_t* tags_flat, int64_t capacity, int32_t B, int32_t S, int32_t C, void* stream) {
    if (!emissions || !start || !end || !trans || !lens || !n_paths || !scores || !tags_flat || ld < C) return ICKA_E_ARG;
    if (B <= 0 || S <= 0 || C <= 0 || nbest <= 0) return ICKA_E_SHAPE;
    if (C > NB_MAX_C || nbest > NB_MAX_K || S > CRF_WORDS_MAX_S || B > CRF_FLAT_MAX_B) return ICKA_E_SHAPE;
    if ((int64_t)S * C * nbest > NB_BP_BYTES || capacity < (int64_t)B * S) return ICKA_E_SHAPE;
    NbestArgs a{};
    a.e = emissions; a.ld = ld; a.mask = mask; a.start = start; a.end = end; a.trans = trans;
    a.lens = lens; a.n_paths = n_paths; a.scores = scores; a.flat = tags_flat; a.cap = capacity;
    a.B = B; a.S = S; a.C = C; a.K = nbest;
    hipLaunchKernelGGL(crf_nbest_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    ICKA_CHECK_LAUNCH();
    return 0;
}
