// Posteriors of the linear-chain CRF (icka_crf_posterior): log Z, the token marginals P(y_t = j | x), and for a given tag path
// (what icka_crf_score_decode writes: lens + tags_flat) its log-probability, the marginal of every path tag, and the chunks
// of the path by the rules of metrics.hip with the exact posterior of each chunk's tag span.  The definitions are written out
// in include/icka_hip.h.
//
// ONE WAVE PER SAMPLE, tag j on lane j, like every kernel of crf.hip; no cross-block communication.  The chain runs over the
// ON-positions only (position 0 and every t >= 1 with mask != 0), i = 0 .. L-1; a path has one tag per on-position.
//   C <= 16, S <= 512, L * C <= 4096: the scaled linear-domain forward-backward of crf_grad_small_kernel (crf.hip) on the
//     COMPACTED sample (the on-positions' emission rows staged back to back in LDS), no transcendental on either S-step chain.
//     Per path position only three scalars leave the chains: a_i[y_i] bhat_i[y_i] (the token marginal), bhat_i[y_i] and the
//     scaled step factor E[y_{i-1}][y_i] x_i[y_i] / c_i; their logs are taken afterwards, lanes over i.
//   otherwise, and for a sample whose normalisers leave the safe range: the log-domain recursions through LDS.
// Both bodies hand the chunk pass the same two arrays: tc_i = P(y_i = path_i | x) and
//   r_i = log P(y_i = path_i | y_{i-1} = path_{i-1}, x) = log(psi_i(path_{i-1}, path_i) beta_i[path_i] / beta_{i-1}[path_{i-1}]) <= 0,
// so the posterior of a span s .. e-1 is tc_s exp(R_{e-1} - R_s) with R the prefix sums of r: alpha_s psi .. psi beta_{e-1} / Z
// with the inner betas telescoped away.  Every r_i is of the size of one step's log-probability, never of the size of the
// accumulated scores, so the difference of two prefix sums keeps its digits on long spans.
// The limits, the label-word bits, chunk_flags, on_pos and the 16-lane primitives (sum16 / max16 / dot_shfl) are crf_core.h's.
#include <math.h>

#include "crf_core.h"

namespace {

constexpr int P_MAX_L = 64;             // label-table words
constexpr float R_FLOOR = -128.f;       // log of a conditional probability that underflowed: exp(R_FLOOR) == 0 in f32

struct PostArgs {
    const float* e; int64_t ld;
    const int64_t* mask;
    const float* start; const float* end; const float* trans;
    const int32_t* lens; const int32_t* flat; int64_t cap;    // the paths (both NULL: no path outputs)
    const int32_t* table; int L_ids;                          // NULL: no chunk outputs
    float* log_z; float* seq_logp; float* token_conf; float* marg;
    int32_t* ent; float* ent_conf; int32_t* n_ent; int32_t* bad;
    int B, S, C;
};

// per-sample LDS of the path and the chunk pass
struct PostLds {
    unsigned char* y;      // [L] path tags (checked)
    float* tc;             // [<= 512] token marginal of the path tag
    float* bh;             // [<= 512] bhat_i[y_i] (scaled) / beta_i[y_i] (log)
    float* g;              // [<= 512] scaled step factor (scaled) / emission of the path tag (log); then r_i, then R_i
    uint32_t* w;           // [<= 512] label-table words of the path
    uint32_t* table;       // [64]
    unsigned long long* term;   // [CRF_WORDS]
};

// ------------------------------------------------------------------------------------------------------ the path
// Exclusive prefix of lens, the number of on-positions L, the checks of the contract, and the path tags into LDS.
// Returns false (wave-uniform) when the sample is refused.  No load or store is indexed by an unchecked id or length.
__device__ __forceinline__ bool post_path(const PostArgs& a, int b, int lane, int L, long long& off, int& plen, unsigned char* s_y) {
    off = 0;
    plen = L;
    if (a.lens == nullptr) return true;
    bool neg = false;
    for (int r = lane; r < b; r += 64) {
        const int n = a.lens[r];
        neg = neg || n < 0;
        off += n;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
    plen = a.lens[b];
    bool bad = neg || plen != L || off < 0 || off + L > a.cap;
    bad = __ballot(bad) != 0ull;
    if (bad) return false;
    for (int i = lane; i < L; i += 64) {
        const int y = a.flat[off + i];
        const bool ok = y >= 0 && y < a.C;
        bad = bad || !ok;
        s_y[i] = (unsigned char)(ok ? y : 0);
    }
    return __ballot(bad) == 0ull;
}

// a refused sample: NaN in its float outputs, no chunks, one more in `bad`
__device__ __forceinline__ void post_refuse(const PostArgs& a, int b, int lane, long long off, int plen) {
    const float nan = __builtin_nanf("");
    if (lane == 0) {
        a.log_z[b] = nan;
        if (a.seq_logp) a.seq_logp[b] = nan;
        if (a.n_ent) a.n_ent[b] = 0;
        atomicAdd(a.bad, 1);
    }
    if (a.token_conf && off >= 0) {   // its own segment [off, off + lens[b]), as far as it lies inside the buffer
        const int n = plen < a.S ? plen : a.S;
        for (int i = lane; i < n; i += 64)
            if (off + i < a.cap) a.token_conf[off + i] = nan;
    }
    if (a.marg) {
        float* mg = a.marg + (int64_t)b * a.S * a.C;
        for (int i = lane; i < a.S * a.C; i += 64) mg[i] = nan;
    }
}

// exact zeros at the off-positions of the marginals
__device__ __forceinline__ void post_zero_off(const PostArgs& a, int b, int lane) {
    if (!a.marg || !a.mask) return;
    float* mg = a.marg + (int64_t)b * a.S * a.C;
    for (int t = 1 + lane; t < a.S; t += 64) {   // lanes over t: one mask load per position, off the chains
        if (a.mask[(int64_t)b * a.S + t] != 0) continue;
        for (int j = 0; j < a.C; ++j) mg[t * a.C + j] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------------------ chunks
// (start / term of a position: chunk_flags, crf_core.h)
// The chunks of the path and their posteriors.  In: p.y, p.tc, p.g = r_i (i >= 1), p.table.  L <= 512.
__device__ __forceinline__ void post_chunks(const PostArgs& a, const PostLds& p, int b, int lane, long long off, int L) {
    // label words; prefix sums R of r (in place), one 64-lane scan per word with the carry of the words before
    float carry = 0.f;
#pragma unroll
    for (int k = 0; k < CRF_WORDS; ++k) {
        const int i = 64 * k + lane;
        const bool in = i < L;
        if (in) {
            const int y = p.y[i];
            p.w[i] = y < a.L_ids ? p.table[y] : LT_DEFAULT;   // an id the table does not name lies outside every chunk
        }
        float v = (in && i >= 1) ? p.g[i] : 0.f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float u = __shfl_up(v, o, 64);
            if (lane >= o) v += u;
        }
        v += carry;
        if (in) p.g[i] = v;
        carry = __shfl(v, 63, 64);
    }
    __syncthreads();   // block = one wave: words and prefix sums are in LDS
    int rank[CRF_WORDS];
    uint32_t starts = 0u;
    int n = 0;
#pragma unroll
    for (int k = 0; k < CRF_WORDS; ++k) {
        const int i = 64 * k + lane;
        const bool in = i < L;
        const uint32_t w = in ? p.w[i] : 0u, wp = (in && i > 0) ? p.w[i - 1] : 0u;
        bool st, tm;
        chunk_flags(w, wp, i == 0, in, st, tm);
        const unsigned long long ms = __ballot(st), mt = __ballot(tm);
        if (lane == 0) p.term[k] = mt;
        rank[k] = n + __popcll(ms & lanes_below(lane));
        starts |= st ? (1u << k) : 0u;
        n += __popcll(ms);
    }
    __syncthreads();   // block = one wave: the term words are in LDS
#pragma unroll
    for (int k = 0; k < CRF_WORDS; ++k) {
        if (!((starts >> k) & 1u)) continue;
        const int i = 64 * k + lane;
        int e = L;   // no term after i: the chunk runs to the end of the path
        bool found = false;
#pragma unroll
        for (int q = k; q < CRF_WORDS; ++q) {
            unsigned long long w = p.term[q];
            if (q == k) w &= ~(lanes_below(lane) | (1ull << lane));
            if (!found && w) { found = true; e = 64 * q + __builtin_ctzll(w); }
        }
        const long long row = off + rank[k];   // rank < L: inside the sample's own segment
        a.ent[row * 3] = (int32_t)(p.w[i] >> 8);
        a.ent[row * 3 + 1] = i;
        a.ent[row * 3 + 2] = e;
        a.ent_conf[row] = p.tc[i] * __expf(fminf(p.g[e - 1] - p.g[i], 0.f));   // a chunk of one token: exp(0) = 1
    }
    if (lane == 0) a.n_ent[b] = n;
}

__device__ __forceinline__ float clamp_r(float r) {   // a log conditional probability: <= 0; NaN / -inf (0 / 0 paths) -> floor
    return r >= R_FLOOR ? fminf(r, 0.f) : R_FLOOR;
}

// ------------------------------------------------------------------------------------------------------ log domain
// The recursions of crf_grad_kernel without the gradient: alpha of every on-position in LDS (compacted), beta on the lanes.
__device__ __forceinline__ void post_log_body(const PostArgs& a, const PostLds p, int L, long long off, float* s_T, float* s_al,
                                              float* s_vec) {
    const int b = blockIdx.x, j = threadIdx.x, C = a.C, S = a.S;
    const bool lane_on = j < C, path = a.lens != nullptr, ent = a.table != nullptr;
    for (int i = j; i < C * C; i += 64) s_T[i] = a.trans[i];
    const float* eb = a.e + (int64_t)b * S * a.ld;
    float* mg = a.marg ? a.marg + (int64_t)b * S * C : nullptr;
    float alpha = lane_on ? a.start[j] + eb[j] : -INFINITY;
    if (lane_on) s_al[j] = alpha;
    int i = 0;
    for (int t = 1; t < S; ++t) {
        if (!on_pos(a, b, t)) continue;   // wave-uniform
        __syncthreads();   // block = one wave: orders the LDS exchange
        if (lane_on) {
            const float* prev = s_al + i * C;
            float m = -INFINITY;
            for (int k = 0; k < C; ++k) m = fmaxf(m, prev[k] + s_T[k * C + j]);
            float s = 0.f;
            for (int k = 0; k < C; ++k) s += __expf(prev[k] + s_T[k * C + j] - m);
            alpha = m + __logf(s) + eb[(int64_t)t * a.ld + j];
            s_al[(i + 1) * C + j] = alpha;
        }
        ++i;
    }
    __syncthreads();   // block = one wave: orders the LDS exchange
    const float v = lane_on ? alpha + a.end[j] : -INFINITY;
    const float m = wave_max(v);
    const float logz = m + __logf(wave_sum(lane_on ? __expf(v - m) : 0.f));

    float beta = lane_on ? a.end[j] : -INFINITY;
    float num = 0.f;   // the path's score, summed on the lanes of its tags
    i = L - 1;
    for (int t = S - 1; t >= 0; --t) {
        if (!on_pos(a, b, t)) {
            if (mg && lane_on) mg[t * C + j] = 0.f;
            continue;
        }
        const float et = lane_on ? eb[(int64_t)t * a.ld + j] : 0.f;
        const float pm = lane_on ? __expf(s_al[i * C + j] + beta - logz) : 0.f;
        if (mg && lane_on) mg[t * C + j] = pm;
        if (path && j == p.y[i]) {
            a.token_conf[off + i] = pm;
            num += et + (i == 0 ? a.start[j] : s_T[p.y[i - 1] * C + j]) + (i == L - 1 ? a.end[j] : 0.f);
            if (ent) { p.tc[i] = pm; p.bh[i] = beta; p.g[i] = et; }
        }
        if (t == 0) break;
        const float u = et + beta;   // e_t[j] + beta_t[j]
        __syncthreads();   // block = one wave: orders the LDS exchange
        if (lane_on) s_vec[j] = u;
        __syncthreads();   // block = one wave: orders the LDS exchange
        if (lane_on) {
            float mx = -INFINITY;
            for (int k = 0; k < C; ++k) mx = fmaxf(mx, s_T[j * C + k] + s_vec[k]);
            float s = 0.f;
            for (int k = 0; k < C; ++k) s += __expf(s_T[j * C + k] + s_vec[k] - mx);
            beta = mx + __logf(s);
        }
        --i;
    }
    num = wave_sum(num);
    if (j == 0) {
        a.log_z[b] = logz;
        if (path) a.seq_logp[b] = num - logz;
    }
    if (ent) {
        __syncthreads();   // block = one wave: the per-position scalars are in LDS
        float r[CRF_WORDS];
#pragma unroll
        for (int k = 0; k < CRF_WORDS; ++k) {
            const int q = 64 * k + j;
            r[k] = 0.f;
            if (q >= 1 && q < L) r[k] = clamp_r(s_T[p.y[q - 1] * C + p.y[q]] + p.g[q] + p.bh[q] - p.bh[q - 1]);
        }
        __syncthreads();   // block = one wave: every g is read before it is overwritten
#pragma unroll
        for (int k = 0; k < CRF_WORDS; ++k) {
            const int q = 64 * k + j;
            if (q < L) p.g[q] = r[k];
        }
        __syncthreads();
        post_chunks(a, p, b, j, off, L);
    }
}

// out of line for the register / shuffle kernel: its rare second pass stays out of the scaled body's register budget.  The
// arguments go BY VALUE: a reference would make the kernel keep its whole argument struct in scratch and read every pointer of
// the scaled body from there; by value only this call copies them (the kernel's scratch is this call frame)
__device__ __noinline__ void post_log_fallback(const PostArgs a, const PostLds p, int L, long long off, float* s_T, float* s_al,
                                               float* s_vec) {
    post_log_body(a, p, L, off, s_T, s_al, s_vec);
}

// ------------------------------------------------------------------------------------------------------ scaled form
// a_i[j] = (sum_k a_{i-1}[k] E[k][j]) x_i[j] / c_i with E = exp(trans - max trans), x_i = exp(e_i - max_j e_i) and c_i =
// sum_k a_{i-1}[k]; bhat_{i-1}[k] = sum_j E[k][j] x_i[j] bhat_i[j] / c_i; marginal_i = a_i . bhat_i (crf.hip, the comment
// above crf_forward_lin).  False (wave-uniform) when a normaliser left the safe range or a marginal is not finite: the caller
// redoes the sample in the log domain, which overwrites whatever this body stored.
__device__ __forceinline__ bool post_lin_body(const PostArgs& a, const PostLds p, int L, long long off, float* s_al, float* s_x,
                                              float* s_c, const unsigned short* s_pos) {
    const int b = blockIdx.x, j = threadIdx.x, C = a.C, S = a.S;
    const bool lane_on = j < C, path = a.lens != nullptr, ent = a.table != nullptr;
    const float* eb = a.e + (int64_t)b * S * a.ld;
    float* mg = a.marg ? a.marg + (int64_t)b * S * C : nullptr;
    // E: column j (into tag j) and row j (out of tag j)
    float mT = -INFINITY;
    for (int k = j; k < C * C; k += 64) mT = fmaxf(mT, a.trans[k]);
    mT = wave_max(mT);
    float Ec[CM], Er[CM];
#pragma unroll
    for (int k = 0; k < CM; ++k) {
        Ec[k] = (lane_on && k < C) ? __expf(a.trans[k * C + j] - mT) : 0.f;
        Er[k] = (lane_on && k < C) ? __expf(a.trans[j * C + k] - mT) : 0.f;
    }
    // stage the on-positions' emission rows back to back, then (lanes over i) x_i in place, the static part of log Z and
    // the path's score from the raw values
    for (int idx = j; idx < L * C; idx += 64) {
        const int i = idx / C, k = idx - i * C;
        s_x[idx] = eb[(int64_t)s_pos[i] * a.ld + k];
    }
    __syncthreads();
    float lzs = 0.f, num = 0.f;
    for (int i = j; i < L; i += 64) {
        float m = -INFINITY;
        for (int k = 0; k < C; ++k) m = fmaxf(m, s_x[i * C + k]);
        if (path) {
            const int y = p.y[i];
            num += s_x[i * C + y] + (i == 0 ? a.start[y] : a.trans[p.y[i - 1] * C + y]) + (i == L - 1 ? a.end[y] : 0.f);
        }
        for (int k = 0; k < C; ++k) s_x[i * C + k] = __expf(s_x[i * C + k] - m);
        lzs += i == 0 ? m : m + mT;
    }
    __syncthreads();
    lzs = wave_sum(lzs);
    num = wave_sum(num);

    // forward: every a_i kept, the normaliser of step i in s_c[i]
    bool ok = true;
    const float sv = lane_on ? a.start[j] : -INFINITY;
    const float mS = max16(sv);
    float al = lane_on ? __expf(sv - mS) * s_x[j] : 0.f;
    float lz = mS + lzs;
    if (lane_on) s_al[j] = al;
    float xn = (lane_on && L > 1) ? s_x[C + j] : 0.f;
    for (int i = 1; i < L; ++i) {
        const float x = xn;
        if (i + 1 < L) xn = lane_on ? s_x[(i + 1) * C + j] : 0.f;
        const float sm = sum16(al);   // beside the 16-term dot product
        ok = ok && sm > CRF_TINY && sm < 1e30f;
        al = dot_shfl(al, Ec) * (x * (1.f / sm));
        lz += __logf(sm);
        if (j == 0) s_c[i] = sm;
        if (lane_on) s_al[i * C + j] = al;
    }
    const float ev = lane_on ? a.end[j] : -INFINITY;
    const float mEnd = max16(ev);
    const float zend = sum16(lane_on ? al * __expf(ev - mEnd) : 0.f);
    ok = ok && zend > CRF_TINY && zend < 1e30f;
    const float logz = lz + mEnd + __logf(zend);
    ok = ok && isfinite(logz);
    // (lanes 16 .. 63 carry the zeros / NaNs of their own empty rows: only the first 16 lanes vote)
    if ((__ballot(!ok) & 0xffffull) != 0ull) return false;
    __syncthreads();

    // x_i / c_i for every step, all rows at once (lanes over i): no division on the backward chain
    for (int i = 1 + j; i < L; i += 64) {
        const float r = 1.f / s_c[i];
        for (int k = 0; k < C; ++k) s_x[i * C + k] *= r;
    }
    __syncthreads();
    // backward; operands fetched from LDS one step ahead
    float bh = lane_on ? __expf(ev - mEnd) / zend : 0.f;
    float al_n = lane_on ? s_al[(L - 1) * C + j] : 0.f, xc_n = lane_on ? s_x[(L - 1) * C + j] : 0.f;
    int y_n = path ? p.y[L - 1] : -1, t_n = s_pos[L - 1];
    for (int i = L - 1; i >= 0; --i) {
        const float alt = al_n, xc = xc_n;
        const int y = y_n, t = t_n;
        if (i > 0) {
            al_n = lane_on ? s_al[(i - 1) * C + j] : 0.f;
            xc_n = lane_on ? s_x[(i - 1) * C + j] : 0.f;
            y_n = path ? p.y[i - 1] : -1;
            t_n = s_pos[i - 1];
        }
        const float pm = alt * bh;
        ok = ok && isfinite(pm);
        if (mg && lane_on) mg[t * C + j] = pm;
        if (j == y) {
            a.token_conf[off + i] = pm;
            if (ent) { p.tc[i] = pm; p.bh[i] = bh; p.g[i] = xc; }   // xc = x_i[y_i] / c_i (i >= 1)
        }
        if (i == 0) break;
        const float u = xc * bh;
        bh = lane_on ? dot_shfl(u, Er) : 0.f;   // bhat_{i-1}[j] = sum_k E[j][k] u[k]
    }
    if ((__ballot(!ok) & 0xffffull) != 0ull) return false;
    if (j == 0) {
        a.log_z[b] = lane_f32(logz, 0);
        if (path) a.seq_logp[b] = num - lane_f32(logz, 0);
    }
    post_zero_off(a, b, j);
    if (ent) {
        __syncthreads();   // block = one wave: the per-position scalars are in LDS
        // r_i = log(E[y_{i-1}][y_i] (x_i[y_i] / c_i) bhat_i[y_i] / bhat_{i-1}[y_{i-1}]): the logs beside the chains, lanes over i
        float r[CRF_WORDS];
#pragma unroll
        for (int k = 0; k < CRF_WORDS; ++k) {
            const int q = 64 * k + j;
            r[k] = 0.f;
            if (q >= 1 && q < L)
                r[k] = clamp_r((a.trans[p.y[q - 1] * C + p.y[q]] - mT) + __logf(p.g[q]) + __logf(p.bh[q]) - __logf(p.bh[q - 1]));
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CRF_WORDS; ++k) {
            const int q = 64 * k + j;
            if (q < L) p.g[q] = r[k];
        }
        __syncthreads();
        post_chunks(a, p, b, j, off, L);
    }
    return true;
}

// ------------------------------------------------------------------------------------------------------ kernels
// C <= 16 and S <= 512
__global__ __launch_bounds__(64) void crf_posterior_small_kernel(const PostArgs a) {
    __shared__ float s_buf[CRF_MAX_SC];   // scaled form: a_i[j] | x_i[j] (L * C <= 4096 each); log form: alpha_i[j]
    __shared__ float s_T[CM * CM], s_vec[64];
    __shared__ float s_c[CRF_WORDS_MAX_S], s_tc[CRF_WORDS_MAX_S], s_bh[CRF_WORDS_MAX_S], s_g[CRF_WORDS_MAX_S];
    __shared__ uint32_t s_w[CRF_WORDS_MAX_S], s_table[P_MAX_L];
    __shared__ unsigned long long s_term[CRF_WORDS];
    __shared__ unsigned short s_pos[CRF_WORDS_MAX_S];
    __shared__ unsigned char s_y[CRF_WORDS_MAX_S];
    const int b = blockIdx.x, lane = threadIdx.x, S = a.S;
    if (a.table) s_table[lane] = lane < a.L_ids ? (uint32_t)a.table[lane] : LT_DEFAULT;
    // the on-positions, compacted in order: the rank of a position is the popcount of the ballots below it
    int L = 0;
#pragma unroll
    for (int k = 0; k < CRF_WORDS; ++k) {
        const int t = 64 * k + lane;
        const bool on = t < S && on_pos(a, b, t);
        const unsigned long long km = __ballot(on);
        if (on) s_pos[L + __popcll(km & lanes_below(lane))] = (unsigned short)t;
        L += __popcll(km);
    }
    long long off;
    int plen;
    const bool good = post_path(a, b, lane, L, off, plen, s_y);
    __syncthreads();   // block = one wave: positions, tags and table are in LDS
    if (!good) { post_refuse(a, b, lane, off, plen); return; }
    PostLds p;
    p.y = s_y; p.tc = s_tc; p.bh = s_bh; p.g = s_g; p.w = s_w; p.table = s_table; p.term = s_term;
    if (L * a.C <= CRF_LIN_SC && post_lin_body(a, p, L, off, s_buf, s_buf + CRF_LIN_SC, s_c, s_pos)) return;
    __syncthreads();
    post_log_fallback(a, p, L, off, s_T, s_buf, s_vec);
}

// C <= 64, S * C <= CRF_MAX_SC (the chunk outputs: S <= 512)
__global__ __launch_bounds__(64) void crf_posterior_kernel(const PostArgs a) {
    __shared__ float s_buf[CRF_MAX_SC];
    __shared__ float s_T[64 * 64], s_vec[64];
    __shared__ float s_tc[CRF_WORDS_MAX_S], s_bh[CRF_WORDS_MAX_S], s_g[CRF_WORDS_MAX_S];
    __shared__ uint32_t s_w[CRF_WORDS_MAX_S], s_table[P_MAX_L];
    __shared__ unsigned long long s_term[CRF_WORDS];
    __shared__ unsigned char s_y[CRF_MAX_SC];
    const int b = blockIdx.x, lane = threadIdx.x, S = a.S;
    if (a.table) s_table[lane] = lane < a.L_ids ? (uint32_t)a.table[lane] : LT_DEFAULT;
    int L = 0;
    for (int t0 = 0; t0 < S; t0 += 64) {
        const int t = t0 + lane;
        L += __popcll(__ballot(t < S && on_pos(a, b, t)));
    }
    long long off;
    int plen;
    const bool good = post_path(a, b, lane, L, off, plen, s_y);
    __syncthreads();   // block = one wave: tags and table are in LDS
    if (!good) { post_refuse(a, b, lane, off, plen); return; }
    PostLds p;
    p.y = s_y; p.tc = s_tc; p.bh = s_bh; p.g = s_g; p.w = s_w; p.table = s_table; p.term = s_term;
    post_log_body(a, p, L, off, s_T, s_buf, s_vec);
}

}  // namespace

extern "C" int icka_crf_posterior(const float* emissions, int64_t ld, const int64_t* mask, const float* start,
                                  const float* end, const float* trans, const int32_t* lens, const int32_t* tags_flat,
                                  int64_t capacity, const int32_t* label_table, int32_t L_ids, float* log_z,
                                  float* seq_logp, float* token_conf, float* marginals, int32_t* ent, float* ent_conf,
                                  int32_t* n_ent, int32_t* bad, int32_t B, int32_t S, int32_t C, void* stream) {
    if (!emissions || !start || !end || !trans || !log_z || !bad || ld < C) return ICKA_E_ARG;
    if ((lens == nullptr) != (tags_flat == nullptr)) return ICKA_E_ARG;
    if (lens && (!seq_logp || !token_conf || capacity < 0)) return ICKA_E_ARG;
    if (label_table && (!lens || !ent || !ent_conf || !n_ent)) return ICKA_E_ARG;
    if (B <= 0 || S <= 0 || C <= 0 || C > 64) return ICKA_E_SHAPE;
    if ((int64_t)S * C > CRF_MAX_SC || B > CRF_FLAT_MAX_B) return ICKA_E_SHAPE;
    if (label_table && (S > CRF_WORDS_MAX_S || L_ids <= 0 || L_ids > P_MAX_L)) return ICKA_E_SHAPE;
    PostArgs a{};
    a.e = emissions; a.ld = ld; a.mask = mask; a.start = start; a.end = end; a.trans = trans;
    a.lens = lens; a.flat = tags_flat; a.cap = capacity; a.table = label_table; a.L_ids = L_ids;
    a.log_z = log_z; a.seq_logp = lens ? seq_logp : nullptr; a.token_conf = lens ? token_conf : nullptr; a.marg = marginals;
    a.ent = ent; a.ent_conf = ent_conf; a.n_ent = label_table ? n_ent : nullptr; a.bad = bad;
    a.B = B; a.S = S; a.C = C;
    if (C <= CM && S <= CRF_WORDS_MAX_S) hipLaunchKernelGGL(crf_posterior_small_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(crf_posterior_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    ICKA_CHECK_LAUNCH();
    return 0;
}
