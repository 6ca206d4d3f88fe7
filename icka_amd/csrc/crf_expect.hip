// CRF expectations (icka_crf_expect / icka_crf_expect_grad): log Z and E_p[r(y)] of a path-additive payoff r under the CRF
// distribution p, with the gradient of both -- the gradient of an expectation is a covariance, Cov_p(f, r), a second-order
// quantity.  Sequence entropy, the KL divergence between two CRFs and an expected cost all reduce to it.  The definitions are
// written out in include/icka_hip.h.
//
// ONE WAVE PER SAMPLE, tag j on lane j, like every kernel of crf.hip; no cross-block communication.  The chain is
// icka_crf_posterior's: it runs over the ON-positions only (position 0 and every t >= 1 with mask != 0), i = 0 .. L-1, found
// with the bit-set walk of crf_core.h; a position's rows are fetched ONE STEP AHEAD of the recursion.
//   The payoff is the path score of a second lattice (given mode) or p's own score minus it (relative mode, formed operand by
//   operand as the values are loaded).  Its node part rn_i(j) takes the start payoff at i = 0 and the end payoff at i = L-1;
//   its edge part is the [C,C] table s_R.
//   EXPECTATION SEMIRING, CENTRED.  Beside the log-domain alpha the forward sweep carries the expected payoff of the prefix
//   through node i given y_i = j,
//     a_i(j) = rn_i(j) + sum_k P(y_{i-1} = k | y_i = j, prefix) (a_{i-1}(k) + R(k, j)),
//   and the backward sweep, beside beta, the expected payoff b_i(j) of the suffix after node i.  Cov(1[y_i = j], r) =
//   mu_i(j) (a_i(j) + b_i(j) - E[r]) subtracts quantities of size L |r|: in f32 the digits are gone (measured 1e-2 .. 1.5e-1
//   on d_emissions at S 128).  So a and b are carried MINUS A WAVE-UNIFORM OFFSET per position: after every forward step the
//   filtering mean m_i = sum_j P(y_i = j | prefix) a_i(j) is taken off (the offsets add up to E[r] - the last, mu-weighted,
//   mean), and at every backward position b is shifted so that sum_j mu_i(j) (a_i(j) + b_i(j)) = 0, which is what the exact
//   quantities satisfy after E[r] is subtracted.  The pair cells use xi_i(k, j) (a_{i-1}(k) + R(k, j) + rn_i(j) + b_i(j) - m_i):
//   summing the first two terms over k gives mu_i(j) (a_i(j) + m_i - rn_i(j)), so this too has mean zero under xi_i.
//   Nothing of size L |r| is ever subtracted.
//   C > 16: the LDS form (scores, transitions, the payoff edge table and the two [C,C] accumulators -- sum_i xi_i and the
//   covariance cells -- in LDS).  C <= 16 (the reference has 13 / 15 labels): the REGISTER form of the same recursions, in the
//   manner of crf_constrained.hip -- column and row of a lane's tag of both tables and its two accumulator columns in
//   registers, the running scores and payoffs exchanged with lane reads: no LDS read across lanes and no barrier on either
//   chain.  The same arithmetic in another summation order: neither form has a range the other lacks.
//   LDS of the gradient kernels: alpha and the centred a of every on-position (two S*C f32 tiles, 16 KiB each at the limit
//   S*C <= 4096) and m_i (S floats, 16 KiB at C = 1): 48.5 KiB in the register form; plus four 16 KiB tables in the LDS form,
//   113 KiB, one block per 160 KiB gfx950 CU.  The value kernels keep two rows of alpha and a in turn (none in registers).
//   -inf scores are not supported (a - b of two -inf payoffs); -1e4 is the documented way to forbid a transition: its
//   probabilities underflow to exact zeros and every product with them is zero.
#include <math.h>

#include "crf_core.h"

namespace {

constexpr int EX_WORDS = CRF_EXPECT_SC / 64;   // S <= 4096 (C = 1): 64 positions per word

struct ExArgs {
    const float* e; int64_t ld;
    const int64_t* mask;
    const float* start; const float* end; const float* trans;
    const float* g; int64_t ldg;                                  // the second lattice: every part nullable (= zeros)
    const float* gstart; const float* gend; const float* gtrans;
    int relative;                                                 // r = s_p - s_second (else r = s_second)
    float* log_z; float* expect;
    const float* glz; const float* gex;                           // upstream [B], nullable (= zeros)
    float* de; int64_t ldd; float* dstart; float* dend; float* dtrans;
    float* dg; int64_t lddg; float* dgstart; float* dgend; float* dgtrans;
    int B, S, C;
};

// the on-positions as bits of s_on[t / 64] (bits at or past S stay clear) and their number L (wave-uniform).  The caller
// orders the LDS writes before its reads (__syncthreads).
__device__ __forceinline__ int ex_scan(const ExArgs& a, int b, int lane, u64* s_on) {
    int L = 0;
    for (int t0 = 0; t0 < a.S; t0 += 64) {
        const int t = t0 + lane;
        const u64 w = __ballot(t < a.S && on_pos(a, b, t));
        if (lane == 0) s_on[t0 >> 6] = w;
        L += __popcll(w);
    }
    return L;
}

// one operand of the payoff from p's value x and the second lattice's value g
__device__ __forceinline__ float pay(bool rel, float x, float g) { return rel ? x - g : g; }

// the payoff edge table beside the transitions
__device__ __forceinline__ void ex_load_tables(const ExArgs& a, int lane, float* s_T, float* s_R) {
    const bool rel = a.relative != 0;
    for (int i = lane; i < a.C * a.C; i += 64) {
        const float t = a.trans[i];
        s_T[i] = t;
        if (s_R) s_R[i] = pay(rel, t, a.gtrans ? a.gtrans[i] : 0.f);
    }
}

// The register form (C <= CM): column j (into tag j) and row j (out of tag j) of the transitions (-inf past C) and of the
// payoff edge table (0 past C), and the columns of the two [C,C] accumulators of tag j
struct ExRegs {
    float Tc[CM], Tr[CM], Rc[CM], Rr[CM], dX[CM], dV[CM];
};
__device__ __forceinline__ void ex_load_regs(const ExArgs& a, int j, ExRegs& r) {
    const bool rel = a.relative != 0;
#pragma unroll
    for (int k = 0; k < CM; ++k) {
        const bool in = j < a.C && k < a.C;
        const float tc = in ? a.trans[k * a.C + j] : -INFINITY, tr = in ? a.trans[j * a.C + k] : -INFINITY;
        r.Tc[k] = tc;
        r.Tr[k] = tr;
        r.Rc[k] = in ? pay(rel, tc, a.gtrans ? a.gtrans[k * a.C + j] : 0.f) : 0.f;
        r.Rr[k] = in ? pay(rel, tr, a.gtrans ? a.gtrans[j * a.C + k] : 0.f) : 0.f;
        r.dX[k] = 0.f;
        r.dV[k] = 0.f;
    }
}

// Forward sweep -> log Z and, with PAY, E_p[r] (both wave-uniform).  KEEP: alpha and the centred a of on-position i at
// s_al / s_at[i * C + j] and the offset m_i at s_m[i]; else two rows of each in turn.  REG (C <= CM): the scores stay on the
// lanes and the tables in registers -- no LDS read and no barrier on the chain, no rows unless KEEP.
template <bool PAY, bool KEEP, bool REG>
__device__ __forceinline__ float ex_forward(const ExArgs& a, int b, int j, const u64* s_on, const float* s_T, const float* s_R,
                                            const ExRegs& r, float* s_al, float* s_at, float* s_m, float& expect) {
    const int C = a.C, S = a.S;
    const bool lane_on = j < C, rel = a.relative != 0;
    const float* eb = a.e + (int64_t)b * S * a.ld;
    const float* gb = a.g ? a.g + (int64_t)b * S * a.ldg : nullptr;
    const float st = lane_on ? a.start[j] : 0.f, en = lane_on ? a.end[j] : 0.f;
    float p_st = 0.f, p_en = 0.f;   // start / end payoff of tag j
    if (PAY && lane_on) {
        p_st = pay(rel, st, a.gstart ? a.gstart[j] : 0.f);
        p_en = pay(rel, en, a.gend ? a.gend[j] : 0.f);
    }
    int t = next_on(s_on, 0, S);
    const float e0 = lane_on ? eb[j] : 0.f;
    float alpha = lane_on ? st + e0 : -INFINITY;
    float at = 0.f, csum = 0.f;
    if (PAY) {
        at = lane_on ? p_st + pay(rel, e0, gb ? gb[j] : 0.f) + (t >= S ? p_en : 0.f) : 0.f;
        const float mx = wave_max(alpha);
        const float p = lane_on ? __expf(alpha - mx) : 0.f;
        const float mi = wave_sum(p * at) / wave_sum(p);
        at = lane_on ? at - mi : 0.f;
        csum = mi;
        if (KEEP && j == 0) s_m[0] = mi;
    }
    if (lane_on && (KEEP || !REG)) {
        s_al[j] = alpha;
        if (PAY) s_at[j] = at;
    }
    float e_n = 0.f, g_n = 0.f;
    if (lane_on && t < S) {
        e_n = eb[(int64_t)t * a.ld + j];
        if (PAY && gb) g_n = gb[(int64_t)t * a.ldg + j];
    }
    int i = 0;
    while (t < S) {   // wave-uniform
        const float et = e_n, gt = g_n;
        t = next_on(s_on, t, S);
        if (lane_on && t < S) {   // the next step's operands: in flight during this step's arithmetic
            e_n = eb[(int64_t)t * a.ld + j];
            if (PAY && gb) g_n = gb[(int64_t)t * a.ldg + j];
        }
        if (REG) {   // (every lane takes part in the lane reads)
            float v[CM];
            float m = -INFINITY;
#pragma unroll
            for (int k = 0; k < CM; ++k) { v[k] = lane_f32(alpha, k) + r.Tc[k]; m = fmaxf(m, v[k]); }
            float s = 0.f, n = 0.f;
#pragma unroll
            for (int k = 0; k < CM; ++k) {
                const float w = __expf(v[k] - m);   // Tc = -inf past C: 0
                s += w;
                if (PAY) n = fmaf(w, lane_f32(at, k) + r.Rc[k], n);
            }
            alpha = lane_on ? m + __logf(s) + et : -INFINITY;
            if (PAY) at = lane_on ? pay(rel, et, gt) + (t >= S ? p_en : 0.f) + n / s : 0.f;
        } else {
            __syncthreads();   // block = one wave: orders the LDS exchange
            if (lane_on) {
                const float* pa = s_al + (KEEP ? i : (i & 1)) * C;
                const float* pt = s_at + (KEEP ? i : (i & 1)) * C;
                float m = -INFINITY;
                for (int k = 0; k < C; ++k) m = fmaxf(m, pa[k] + s_T[k * C + j]);
                float s = 0.f, n = 0.f;
                for (int k = 0; k < C; ++k) {
                    const float w = __expf(pa[k] + s_T[k * C + j] - m);
                    s += w;
                    if (PAY) n = fmaf(w, pt[k] + s_R[k * C + j], n);
                }
                alpha = m + __logf(s) + et;
                if (PAY) at = pay(rel, et, gt) + (t >= S ? p_en : 0.f) + n / s;
            }
        }
        ++i;
        if (PAY) {   // take the filtering mean off: the offsets add up in csum
            const float mx = wave_max(alpha);
            const float p = lane_on ? __expf(alpha - mx) : 0.f;
            const float mi = wave_sum(p * at) / wave_sum(p);
            at = lane_on ? at - mi : 0.f;
            csum += mi;
            if (KEEP && j == 0) s_m[i] = mi;
        }
        if (lane_on && (KEEP || !REG)) {
            s_al[(KEEP ? i : (i & 1)) * C + j] = alpha;
            if (PAY) s_at[(KEEP ? i : (i & 1)) * C + j] = at;
        }
    }
    __syncthreads();   // block = one wave: orders the LDS exchange
    const float v = lane_on ? alpha + en : -INFINITY;
    const float m = wave_max(v);
    const float logz = m + __logf(wave_sum(lane_on ? __expf(v - m) : 0.f));
    if (PAY) {
        const float mu = lane_on ? __expf(v - logz) : 0.f;
        expect = csum + wave_sum(mu * at) / wave_sum(mu);
    }
    return logz;
}

// exact +0.0 in the C columns of every off-position row of the sample in d (lanes over the positions)
__device__ __forceinline__ void ex_zero_off_rows(const ExArgs& a, int b, int lane, const u64* s_on, float* d, int64_t ldd) {
    if (a.mask == nullptr || d == nullptr) return;
    float* db = d + (int64_t)b * a.S * ldd;
    for (int t = lane; t < a.S; t += 64) {
        if ((s_on[t >> 6] >> (t & 63)) & 1ull) continue;
        for (int k = 0; k < a.C; ++k) db[(int64_t)t * ldd + k] = 0.f;
    }
}

// Backward sweep over the tiles ex_forward<COV, true> left.  Writes the on-position rows of d_emissions (glz mu + gex (cov +
// [relative] mu)) and of the second lattice's (+- gex mu); s_X collects the pair marginals sum_i xi_i and, with COV, s_V the
// covariance cells; mu0 / cov0 and muL / covL are the node quantities at the first / last on-position (start, end).
// REG (C <= CM): beta and b stay on the lanes, the tables and the accumulator columns (r.dX, r.dV) in registers; a lane reads
// only its own tag's entries of the tiles.
template <bool COV, bool REG>
__device__ __forceinline__ void ex_backward(const ExArgs& a, int b, int j, int L, float glz, float gex,
                                            const u64* s_on, const float* s_T, const float* s_R, float* s_X, float* s_V,
                                            ExRegs& r, const float* s_al, const float* s_at, const float* s_m, float* s_vec,
                                            float* s_vec2, float& mu0, float& cov0, float& muL, float& covL) {
    const int C = a.C, S = a.S;
    const bool lane_on = j < C, rel = a.relative != 0;
    const float* eb = a.e + (int64_t)b * S * a.ld;
    const float* gb = (COV && a.g) ? a.g + (int64_t)b * S * a.ldg : nullptr;
    float* deb = a.de ? a.de + (int64_t)b * S * a.ldd : nullptr;
    float* dgb = a.dg ? a.dg + (int64_t)b * S * a.lddg : nullptr;
    const float c_mu = glz + (rel ? gex : 0.f);   // d_emissions = c_mu mu + gex cov
    const float c_g = rel ? -gex : gex;           // the second lattice's = c_g mu
    float p_en = 0.f;
    if (COV && lane_on) p_en = pay(rel, a.end[j], a.gend ? a.gend[j] : 0.f);
    float beta = lane_on ? a.end[j] : -INFINITY;
    float braw = 0.f;
    int t = L > 1 ? prev_on(s_on, S) : 0;   // the last on-position
    float e_n = lane_on ? eb[(int64_t)t * a.ld + j] : 0.f;
    float g_n = (gb && lane_on) ? gb[(int64_t)t * a.ldg + j] : 0.f;
    for (int i = L - 1; i >= 0; --i) {
        const float et = e_n, gt = g_n;
        const int tc = t;
        if (i > 0) {   // the next step's operands: in flight during this step's arithmetic
            t = prev_on(s_on, t);
            if (lane_on) {
                e_n = eb[(int64_t)t * a.ld + j];
                if (gb) g_n = gb[(int64_t)t * a.ldg + j];
            }
        }
        // mu_i = softmax_j (alpha_i + beta_i): normalised by log Z AS THIS POSITION SEES IT (lzi), so the rounding its alphas have
        // in common after i steps drops out (measured 5x on d_emissions at S 128 against exp(alpha + beta - log Z))
        const float ab = lane_on ? s_al[i * C + j] + beta : -INFINITY;
        const float abm = wave_max(ab);
        const float pe = lane_on ? __expf(ab - abm) : 0.f;
        const float pes = wave_sum(pe);
        const float mu = pe / pes;
        const float lzi = abm + __logf(pes);
        float bt = 0.f, cov = 0.f;
        if (COV) {   // shift b so that a + b has mean zero under mu
            const float sab = lane_on ? s_at[i * C + j] + braw : 0.f;
            const float mean = wave_sum(mu * sab);
            bt = braw - mean;
            cov = mu * (sab - mean);
        }
        if (lane_on) {
            if (deb) deb[(int64_t)tc * a.ldd + j] = COV ? fmaf(gex, cov, c_mu * mu) : c_mu * mu;
            if (dgb) dgb[(int64_t)tc * a.lddg + j] = c_g * mu;
        }
        if (i == L - 1) { muL = mu; covL = cov; }
        if (i == 0) { mu0 = mu; cov0 = cov; break; }
        const float u = lane_on ? et + beta : -INFINITY;   // x_i[j] + beta_i[j]
        float rb = 0.f;                                      // rn_i(j) + b_i(j)
        if (COV) rb = lane_on ? pay(rel, et, gt) + (i == L - 1 ? p_en : 0.f) + bt : 0.f;
        if (REG) {   // (every lane takes part in the lane reads)
            const float c = u - lzi, w = COV ? rb - s_m[i] : 0.f;
            const float al_p = lane_on ? s_al[(i - 1) * C + j] : -INFINITY;
            const float at_p = (COV && lane_on) ? s_at[(i - 1) * C + j] : 0.f;
#pragma unroll
            for (int k = 0; k < CM; ++k) {
                const float xi = __expf(lane_f32(al_p, k) + r.Tc[k] + c);   // Tc = -inf past C: + 0
                r.dX[k] += xi;
                if (COV) r.dV[k] = fmaf(xi, lane_f32(at_p, k) + r.Rc[k] + w, r.dV[k]);
            }
            // beta_{i-1}[j] = logsumexp_k (T[j][k] + u[k]) and b_{i-1}(j), its weights' mean of R(j, k) + rn_i(k) + b_i(k)
            float v[CM];
            float mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < CM; ++k) { v[k] = r.Tr[k] + lane_f32(u, k); mx = fmaxf(mx, v[k]); }
            float s = 0.f, n = 0.f;
#pragma unroll
            for (int k = 0; k < CM; ++k) {
                const float wk = __expf(v[k] - mx);
                s += wk;
                if (COV) n = fmaf(wk, r.Rr[k] + lane_f32(rb, k), n);
            }
            beta = lane_on ? mx + __logf(s) : -INFINITY;
            if (COV) braw = lane_on ? n / s : 0.f;
            continue;
        }
        if (lane_on) {
            const float c = u - lzi, w = COV ? rb - s_m[i] : 0.f;
            const float* pa = s_al + (i - 1) * C;
            const float* pt = s_at + (i - 1) * C;
            for (int k = 0; k < C; ++k) {
                const float xi = __expf(pa[k] + s_T[k * C + j] + c);
                s_X[k * C + j] += xi;
                if (COV) s_V[k * C + j] = fmaf(xi, pt[k] + s_R[k * C + j] + w, s_V[k * C + j]);
            }
        }
        // beta_{i-1}[k] = logsumexp_j (T[k][j] + u[j]) and b_{i-1}(k), its weights' mean of R(k, j) + rn_i(j) + b_i(j): lane k
        // loops over j
        __syncthreads();   // block = one wave: orders the LDS exchange
        if (lane_on) {
            s_vec[j] = u;
            if (COV) s_vec2[j] = rb;
        }
        __syncthreads();   // block = one wave: orders the LDS exchange
        if (lane_on) {
            float mx = -INFINITY;
            for (int k = 0; k < C; ++k) mx = fmaxf(mx, s_T[j * C + k] + s_vec[k]);
            float s = 0.f, n = 0.f;
            for (int k = 0; k < C; ++k) {
                const float w = __expf(s_T[j * C + k] + s_vec[k] - mx);
                s += w;
                if (COV) n = fmaf(w, s_R[j * C + k] + s_vec2[k], n);
            }
            beta = mx + __logf(s);
            if (COV) braw = n / s;
        }
        __syncthreads();   // block = one wave: orders the LDS exchange
    }
}

// ---------------------------------------------------------------------------------------------------------- values
template <bool PAY>
__global__ __launch_bounds__(64) void crf_expect_kernel(const ExArgs a) {
    __shared__ float s_T[64 * 64];
    __shared__ float s_R[PAY ? 64 * 64 : 1];
    __shared__ float s_al[2 * 64];
    __shared__ float s_at[2 * 64];
    __shared__ u64 s_on[EX_WORDS];
    const int b = blockIdx.x, j = threadIdx.x;
    ex_scan(a, b, j, s_on);
    ex_load_tables(a, j, s_T, PAY ? s_R : nullptr);
    __syncthreads();
    float expect = 0.f;
    ExRegs r;   // (not used by this form)
    const float logz = ex_forward<PAY, false, false>(a, b, j, s_on, s_T, s_R, r, s_al, s_at, nullptr, expect);
    if (j == 0) {
        a.log_z[b] = logz;
        if (PAY) a.expect[b] = expect;
    }
}

template <bool PAY>
__global__ __launch_bounds__(64) void crf_expect_small_kernel(const ExArgs a) {   // C <= 16
    __shared__ u64 s_on[EX_WORDS];
    const int b = blockIdx.x, j = threadIdx.x;
    ex_scan(a, b, j, s_on);
    ExRegs r;
    ex_load_regs(a, j, r);
    __syncthreads();
    float expect = 0.f;
    const float logz = ex_forward<PAY, false, true>(a, b, j, s_on, nullptr, nullptr, r, nullptr, nullptr, nullptr, expect);
    if (j == 0) {
        a.log_z[b] = logz;
        if (PAY) a.expect[b] = expect;
    }
}

// -------------------------------------------------------------------------------------------------------- gradient
template <bool COV>
__global__ __launch_bounds__(64) void crf_expect_grad_kernel(const ExArgs a) {
    __shared__ float s_T[64 * 64];
    __shared__ float s_X[64 * 64];                      // sum_i xi_i(k, j)
    __shared__ float s_R[COV ? 64 * 64 : 1];
    __shared__ float s_V[COV ? 64 * 64 : 1];            // sum_i xi_i(k, j) (centred payoff through the edge)
    __shared__ float s_al[CRF_EXPECT_SC];               // alpha of on-position i at [i * C + j]
    __shared__ float s_at[COV ? CRF_EXPECT_SC : 1];     // the centred prefix payoff likewise
    __shared__ float s_m[COV ? CRF_EXPECT_SC : 1];      // the offset taken off at on-position i
    __shared__ float s_vec[64], s_vec2[64];
    __shared__ u64 s_on[EX_WORDS];
    const int b = blockIdx.x, j = threadIdx.x, C = a.C;
    const bool rel = a.relative != 0;
    const int L = ex_scan(a, b, j, s_on);
    ex_load_tables(a, j, s_T, COV ? s_R : nullptr);
    for (int i = j; i < C * C; i += 64) {
        s_X[i] = 0.f;
        if (COV) s_V[i] = 0.f;
    }
    __syncthreads();
    ex_zero_off_rows(a, b, j, s_on, a.de, a.ldd);
    ex_zero_off_rows(a, b, j, s_on, a.dg, a.lddg);
    const float glz = a.glz ? a.glz[b] : 0.f, gex = a.gex ? a.gex[b] : 0.f;
    float expect = 0.f, mu0 = 0.f, cov0 = 0.f, muL = 0.f, covL = 0.f;
    ExRegs r;   // (not used by this form)
    ex_forward<COV, true, false>(a, b, j, s_on, s_T, s_R, r, s_al, s_at, s_m, expect);
    ex_backward<COV, false>(a, b, j, L, glz, gex, s_on, s_T, s_R, s_X, s_V, r, s_al, s_at, s_m, s_vec, s_vec2, mu0, cov0, muL,
                            covL);
    const float c_mu = glz + (rel ? gex : 0.f), c_g = rel ? -gex : gex;
    if (j < C) {
        if (a.dstart) atomicAdd(a.dstart + j, fmaf(gex, cov0, c_mu * mu0));
        if (a.dend) atomicAdd(a.dend + j, fmaf(gex, covL, c_mu * muL));
        if (a.dgstart) atomicAdd(a.dgstart + j, c_g * mu0);
        if (a.dgend) atomicAdd(a.dgend + j, c_g * muL);
    }
    __syncthreads();   // block = one wave: orders the LDS exchange
    for (int i = j; i < C * C; i += 64) {
        if (a.dtrans) atomicAdd(a.dtrans + i, COV ? fmaf(gex, s_V[i], c_mu * s_X[i]) : c_mu * s_X[i]);
        if (a.dgtrans) atomicAdd(a.dgtrans + i, c_g * s_X[i]);
    }
}

template <bool COV>
__global__ __launch_bounds__(64) void crf_expect_grad_small_kernel(const ExArgs a) {   // C <= 16
    __shared__ float s_al[CRF_EXPECT_SC];               // alpha of on-position i at [i * C + j]
    __shared__ float s_at[COV ? CRF_EXPECT_SC : 1];     // the centred prefix payoff likewise
    __shared__ float s_m[COV ? CRF_EXPECT_SC : 1];      // the offset taken off at on-position i
    __shared__ u64 s_on[EX_WORDS];
    const int b = blockIdx.x, j = threadIdx.x, C = a.C;
    const bool rel = a.relative != 0;
    const int L = ex_scan(a, b, j, s_on);
    ExRegs r;
    ex_load_regs(a, j, r);
    __syncthreads();
    ex_zero_off_rows(a, b, j, s_on, a.de, a.ldd);
    ex_zero_off_rows(a, b, j, s_on, a.dg, a.lddg);
    const float glz = a.glz ? a.glz[b] : 0.f, gex = a.gex ? a.gex[b] : 0.f;
    float expect = 0.f, mu0 = 0.f, cov0 = 0.f, muL = 0.f, covL = 0.f;
    ex_forward<COV, true, true>(a, b, j, s_on, nullptr, nullptr, r, s_al, s_at, s_m, expect);   // (ends with a barrier: s_m)
    ex_backward<COV, true>(a, b, j, L, glz, gex, s_on, nullptr, nullptr, nullptr, nullptr, r, s_al, s_at, s_m, nullptr, nullptr,
                           mu0, cov0, muL, covL);
    const float c_mu = glz + (rel ? gex : 0.f), c_g = rel ? -gex : gex;
    if (j < C) {
        if (a.dstart) atomicAdd(a.dstart + j, fmaf(gex, cov0, c_mu * mu0));
        if (a.dend) atomicAdd(a.dend + j, fmaf(gex, covL, c_mu * muL));
        if (a.dgstart) atomicAdd(a.dgstart + j, c_g * mu0);
        if (a.dgend) atomicAdd(a.dgend + j, c_g * muL);
#pragma unroll
        for (int k = 0; k < CM; ++k) {
            if (k >= C) continue;
            if (a.dtrans) atomicAdd(a.dtrans + k * C + j, COV ? fmaf(gex, r.dV[k], c_mu * r.dX[k]) : c_mu * r.dX[k]);
            if (a.dgtrans) atomicAdd(a.dgtrans + k * C + j, c_g * r.dX[k]);
        }
    }
}

inline int ex_check(const void* e, const void* start, const void* end, const void* trans, int64_t ld, const void* g,
                    int64_t ldg, int relative, int B, int S, int C) {
    if (!e || !start || !end || !trans || ld < C || (g && ldg < C) || (relative != 0 && relative != 1)) return ICKA_E_ARG;
    if (B <= 0 || S <= 0 || C <= 0 || C > 64 || (int64_t)S * C > CRF_EXPECT_SC) return ICKA_E_SHAPE;
    return 0;
}

}  // namespace

extern "C" int icka_crf_expect(const float* emissions, int64_t ld, const int64_t* mask, const float* start, const float* end,
                               const float* trans, const float* second, int64_t ld2, const float* second_start,
                               const float* second_end, const float* second_trans, int32_t relative, float* log_z,
                               float* expect, int32_t B, int32_t S, int32_t C, void* stream) {
    if (int rc = ex_check(emissions, start, end, trans, ld, second, ld2, relative, B, S, C)) return rc;
    if (!log_z) return ICKA_E_ARG;
    ExArgs a{};
    a.e = emissions; a.ld = ld; a.mask = mask; a.start = start; a.end = end; a.trans = trans;
    a.g = second; a.ldg = ld2; a.gstart = second_start; a.gend = second_end; a.gtrans = second_trans; a.relative = relative;
    a.log_z = log_z; a.expect = expect; a.B = B; a.S = S; a.C = C;
    const dim3 grid(B), block(64);
    hipStream_t st = (hipStream_t)stream;
    if (C <= CM) {
        if (expect) hipLaunchKernelGGL(crf_expect_small_kernel<true>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(crf_expect_small_kernel<false>, grid, block, 0, st, a);
    } else {
        if (expect) hipLaunchKernelGGL(crf_expect_kernel<true>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(crf_expect_kernel<false>, grid, block, 0, st, a);
    }
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_crf_expect_grad(const float* emissions, int64_t ld, const int64_t* mask, const float* start,
                                    const float* end, const float* trans, const float* second, int64_t ld2,
                                    const float* second_start, const float* second_end, const float* second_trans,
                                    int32_t relative, const float* g_logz, const float* g_expect, float* d_emissions,
                                    int64_t ldd, float* d_start, float* d_end, float* d_trans, float* d_second, int64_t ldd2,
                                    float* d_second_start, float* d_second_end, float* d_second_trans, int32_t B, int32_t S,
                                    int32_t C, void* stream) {
    if (int rc = ex_check(emissions, start, end, trans, ld, second, ld2, relative, B, S, C)) return rc;
    if ((d_emissions && ldd < C) || (d_second && ldd2 < C)) return ICKA_E_ARG;
    ExArgs a{};
    a.e = emissions; a.ld = ld; a.mask = mask; a.start = start; a.end = end; a.trans = trans;
    a.g = second; a.ldg = ld2; a.gstart = second_start; a.gend = second_end; a.gtrans = second_trans; a.relative = relative;
    a.glz = g_logz; a.gex = g_expect;
    a.de = d_emissions; a.ldd = ldd; a.dstart = d_start; a.dend = d_end; a.dtrans = d_trans;
    a.dg = d_second; a.lddg = ldd2; a.dgstart = d_second_start; a.dgend = d_second_end; a.dgtrans = d_second_trans;
    a.B = B; a.S = S; a.C = C;
    // the covariance is what the first lattice's gradient of `expect` needs: skipped when nothing asks for it
    const bool cov = g_expect && (d_emissions || d_start || d_end || d_trans);
    const dim3 grid(B), block(64);
    hipStream_t st = (hipStream_t)stream;
    if (C <= CM) {
        if (cov) hipLaunchKernelGGL(crf_expect_grad_small_kernel<true>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(crf_expect_grad_small_kernel<false>, grid, block, 0, st, a);
    } else {
        if (cov) hipLaunchKernelGGL(crf_expect_grad_kernel<true>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(crf_expect_grad_kernel<false>, grid, block, 0, st, a);
    }
    ICKA_CHECK_LAUNCH();
    return 0;
}
