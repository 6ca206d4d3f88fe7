// The constrained linear-chain CRF (icka_crf_constrained_llh / _grad / _decode): every on-position carries a SET of allowed
// tags (a 64-bit word, bit j = tag j).  Training on partially labelled data maximises the marginal likelihood of all paths
// that stay inside the sets, llh = log Z_A - log Z; decoding returns the best path inside the sets.  The definitions are
// written out in include/icka_hip.h.
//
// ONE WAVE PER SAMPLE, tag j on lane j, like every kernel of crf.hip; no cross-block communication.  The chain is
// icka_crf_posterior's: it runs over the ON-positions only (position 0 and every t >= 1 with mask != 0), i = 0 .. L-1.
// The allowed test is bit j of a wave-uniform 64-bit word.  Log-domain recursions in f32.  The two lattices run ONE AFTER THE
// OTHER in the same wave and share the alpha tile: first the free one (log Z, - marginals), then the restricted one (log Z_A,
// + marginals), in which a tag outside A_i has alpha_i = -inf and drops out of the beta sums.  An infeasible sample (an empty
// set at an on-position) is found by a scan of the words before either lattice: the restricted recursions never run on it, so
// no (-inf) - (-inf) is ever formed.
//   The same scan leaves the on-positions as a bit set in LDS (one ballot per 64 positions), so a recursion finds its next
//   position with a bit scan and fetches that position's emissions, allowed word and (restricted backward) d_emissions row
//   ONE STEP AHEAD: no global load is waited for on the chain.
//   C > 16: the LDS form, the bodies of crf_grad_kernel / post_log_body (scores and transitions in LDS; measured 1.8 us per
//   step and lattice at C = 17, where the fetch-ahead changed nothing: its 4 C LDS reads per step dominate).
//   C <= 16 (the reference has 13 / 15 labels): the REGISTER form of the same recursions -- the transition column (and row,
//   and the gradient column) of a lane's tag in registers, the running scores exchanged with lane reads: no LDS read and no
//   barrier on either chain (0.4 us per step and lattice at C = 13 against 1.5 us in the LDS form).  It is the same arithmetic
//   in another summation order, not a scaled form: it has no range the LDS form lacks, so there is no fallback between them.
//   LDS of the gradient kernels: alpha 48 KiB, plus transitions 16 KiB and their gradient 16 KiB in the LDS form (80 KiB, what
//   crf_grad_kernel takes: two blocks per 160 KiB gfx950 CU; both lattices side by side would take 128 KiB).
#include <math.h>

#include "crf_core.h"

namespace {

constexpr int ON_WORDS = CRF_MAX_SC / 64;   // S <= 12288 (C = 1): 64 positions per word

struct ConArgs {
    const float* e; int64_t ld;
    const int64_t* mask; const int64_t* allowed;
    const float* start; const float* end; const float* trans;
    float* llh; float* log_z; float* log_za; int32_t* infeasible;
    const float* gllh; float* de; int64_t ldd; float* dstart; float* dend; float* dtrans;
    int32_t* lens; int32_t* flat; float* scores;
    int B, S, C;
};

__device__ __forceinline__ unsigned long long tag_bits(int C) { return C >= 64 ? ~0ull : (1ull << C) - 1ull; }
__device__ __forceinline__ unsigned long long allowed_at(const ConArgs& a, int b, int t) {
    return (unsigned long long)a.allowed[(int64_t)b * a.S + t];
}

// The on-positions as bits of s_on[t / 64] (bits at or past S stay clear), their number L, and whether every one of them has
// an allowed tag below C (all wave-uniform).  The caller orders the LDS writes before its reads (__syncthreads).
__device__ __forceinline__ int scan_sample(const ConArgs& a, int b, int lane, u64* s_on, bool& feasible) {
    const u64 cm = tag_bits(a.C);
    int L = 0;
    bool bad = false;
    for (int t0 = 0; t0 < a.S; t0 += 64) {
        const int t = t0 + lane;
        const bool on = t < a.S && on_pos(a, b, t);
        bad = bad || (on && (allowed_at(a, b, t) & cm) == 0ull);
        const u64 w = __ballot(on);
        if (lane == 0) s_on[t0 >> 6] = w;
        L += __popcll(w);
    }
    feasible = __ballot(bad) == 0ull;
    return L;
}
// Forward recursion of the free (R = false) or the restricted lattice -> log Z (wave-uniform).  KEEP: alpha of on-position i
// at s_al[i * C + j] (L * C floats); else two rows in turn.
template <bool R, bool KEEP>
__device__ __forceinline__ float con_forward(const ConArgs& a, int b, int j, const u64* s_on, const float* s_T, float* s_al) {
    const int C = a.C, S = a.S;
    const bool lane_on = j < C;
    const float* eb = a.e + (int64_t)b * S * a.ld;
    float alpha = (lane_on && (!R || ((allowed_at(a, b, 0) >> j) & 1ull))) ? a.start[j] + eb[j] : -INFINITY;
    if (lane_on) s_al[j] = alpha;
    int t = next_on(s_on, 0, S);
    float e_n = (lane_on && t < S) ? eb[(int64_t)t * a.ld + j] : 0.f;
    u64 w_n = (R && t < S) ? allowed_at(a, b, t) : 0ull;
    int i = 0;
    while (t < S) {   // wave-uniform
        const float et = e_n;
        const bool ok = lane_on && (!R || ((w_n >> j) & 1ull));
        t = next_on(s_on, t, S);
        if (t < S) {   // the next step's operands: in flight during this step's arithmetic
            if (lane_on) e_n = eb[(int64_t)t * a.ld + j];
            if (R) w_n = allowed_at(a, b, t);
        }
        __syncthreads();   // block = one wave: orders the LDS exchange
        if (lane_on) {
            const float* prev = s_al + (KEEP ? i : (i & 1)) * C;
            float m = -INFINITY;
            for (int k = 0; k < C; ++k) m = fmaxf(m, prev[k] + s_T[k * C + j]);
            float s = 0.f;
            for (int k = 0; k < C; ++k) s += __expf(prev[k] + s_T[k * C + j] - m);
            alpha = ok ? m + __logf(s) + et : -INFINITY;
            s_al[(KEEP ? i + 1 : ((i + 1) & 1)) * C + j] = alpha;
        }
        ++i;
    }
    __syncthreads();   // block = one wave: orders the LDS exchange
    const float v = lane_on ? alpha + a.end[j] : -INFINITY;
    const float m = wave_max(v);
    return m + __logf(wave_sum(lane_on ? __expf(v - m) : 0.f));
}

// exact +0.0 in the C columns of every off-position row of the sample's d_emissions (lanes over the positions)
__device__ __forceinline__ void zero_off_rows(const ConArgs& a, int b, int lane, const u64* s_on) {
    if (a.mask == nullptr) return;
    float* deb = a.de + (int64_t)b * a.S * a.ldd;
    for (int t = lane; t < a.S; t += 64) {
        if ((s_on[t >> 6] >> (t & 63)) & 1ull) continue;
        for (int k = 0; k < a.C; ++k) deb[(int64_t)t * a.ldd + k] = 0.f;
    }
}

// exact +0.0 in the C columns of every row of the sample's d_emissions (an infeasible sample)
__device__ __forceinline__ void zero_all_rows(const ConArgs& a, int b, int lane) {
    float* deb = a.de + (int64_t)b * a.S * a.ldd;
    for (int idx = lane; idx < a.S * a.C; idx += 64) {
        const int t = idx / a.C, k = idx - t * a.C;
        deb[(int64_t)t * a.ldd + k] = 0.f;
    }
}

// Backward recursion of one lattice over the alphas con_forward<R, true> left in s_al.  The free lattice runs first and WRITES
// the on-position rows of d_emissions (- g * marginal); the restricted one then ADDS g * marginal to them (the old value is
// fetched one step ahead).  s_dT, dstart and dend collect (restricted - free) pair / first / last marginals, not yet times g.
template <bool R>
__device__ __forceinline__ void con_backward(const ConArgs& a, int b, int j, int L, float g, float logz, const u64* s_on,
                                             const float* s_T, float* s_dT, const float* s_al, float* s_vec, float& dstart,
                                             float& dend) {
    const int C = a.C, S = a.S;
    const bool lane_on = j < C;
    const float sg = R ? 1.f : -1.f;
    const float* eb = a.e + (int64_t)b * S * a.ld;
    float* deb = a.de + (int64_t)b * S * a.ldd;
    float beta = lane_on ? a.end[j] : -INFINITY;
    int t = L > 1 ? prev_on(s_on, S) : 0;   // the last on-position
    float e_n = lane_on ? eb[(int64_t)t * a.ld + j] : 0.f;
    float d_n = (R && lane_on) ? deb[(int64_t)t * a.ldd + j] : 0.f;
    u64 w_n = R ? allowed_at(a, b, t) : 0ull;
    for (int i = L - 1; i >= 0; --i) {
        const float et = e_n, d_old = d_n;
        const bool ok = lane_on && (!R || ((w_n >> j) & 1ull));
        const int tc = t;
        if (i > 0) {   // the next step's operands: in flight during this step's arithmetic
            t = prev_on(s_on, t);
            if (lane_on) e_n = eb[(int64_t)t * a.ld + j];
            if (R && lane_on) d_n = deb[(int64_t)t * a.ldd + j];
            if (R) w_n = allowed_at(a, b, t);
        }
        const float pm = lane_on ? __expf(s_al[i * C + j] + beta - logz) : 0.f;   // alpha = -inf outside A_i: exactly 0
        if (lane_on) deb[(int64_t)tc * a.ldd + j] = R ? d_old + g * pm : -(g * pm);
        if (i == L - 1) dend += sg * pm;
        if (i == 0) { dstart += sg * pm; break; }
        const float u = ok ? et + beta : -INFINITY;   // x_i[j] + beta_i[j], tags outside A_i drop out
        if (lane_on)
            for (int k = 0; k < C; ++k) s_dT[k * C + j] += sg * __expf(s_al[(i - 1) * C + k] + s_T[k * C + j] + u - logz);
        // beta_{i-1}[k] = logsumexp_j (T[k][j] + u[j]): lane k loops over j (a feasible sample has a finite u at every step)
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
        __syncthreads();   // block = one wave: orders the LDS exchange
    }
}

// ------------------------------------------------------------------------------------------------ register form (C <= CM)
// lse_k (value of lane k + col[k]) over the CM lanes of the tags; col[k] = -inf for k >= C
__device__ __forceinline__ float lse_lanes(float x, const float (&col)[CM]) {
    float v[CM];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < CM; ++k) { v[k] = lane_f32(x, k) + col[k]; m = fmaxf(m, v[k]); }
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int k = 0; k < CM; k += 2) { s0 += __expf(v[k] - m); s1 += __expf(v[k + 1] - m); }
    return m + __logf(s0 + s1);
}
// column j (into tag j) and row j (out of tag j) of the transitions, -inf past C
__device__ __forceinline__ void load_T(const ConArgs& a, int j, float (&Tc)[CM], float (&Tr)[CM]) {
#pragma unroll
    for (int k = 0; k < CM; ++k) {
        Tc[k] = (j < a.C && k < a.C) ? a.trans[k * a.C + j] : -INFINITY;
        Tr[k] = (j < a.C && k < a.C) ? a.trans[j * a.C + k] : -INFINITY;
    }
}

// con_forward with the scores on the lanes.  KEEP: alpha of on-position i at s_al[i * C + j]; else s_al is not touched.
template <bool R, bool KEEP>
__device__ __forceinline__ float con_forward_reg(const ConArgs& a, int b, int j, const u64* s_on, const float (&Tc)[CM],
                                                 float* s_al) {
    const int C = a.C, S = a.S;
    const bool lane_on = j < C;
    const float* eb = a.e + (int64_t)b * S * a.ld;
    float alpha = (lane_on && (!R || ((allowed_at(a, b, 0) >> j) & 1ull))) ? a.start[j] + eb[j] : -INFINITY;
    if (KEEP && lane_on) s_al[j] = alpha;
    int t = next_on(s_on, 0, S);
    float e_n = (lane_on && t < S) ? eb[(int64_t)t * a.ld + j] : 0.f;
    u64 w_n = (R && t < S) ? allowed_at(a, b, t) : 0ull;
    int i = 0;
    while (t < S) {   // wave-uniform
        const float et = e_n;
        const bool ok = lane_on && (!R || ((w_n >> j) & 1ull));
        t = next_on(s_on, t, S);
        if (t < S) {   // the next step's operands: in flight during this step's arithmetic
            if (lane_on) e_n = eb[(int64_t)t * a.ld + j];
            if (R) w_n = allowed_at(a, b, t);
        }
        const float nx = lse_lanes(alpha, Tc) + et;   // (every lane takes part in the lane reads)
        alpha = ok ? nx : -INFINITY;
        ++i;
        if (KEEP && lane_on) s_al[i * C + j] = alpha;
    }
    const float v = lane_on ? alpha + a.end[j] : -INFINITY;
    const float m = wave_max(v);
    return m + __logf(wave_sum(lane_on ? __expf(v - m) : 0.f));
}

// con_backward with beta on the lanes and the gradient column of tag j in dT
template <bool R>
__device__ __forceinline__ void con_backward_reg(const ConArgs& a, int b, int j, int L, float g, float logz, const u64* s_on,
                                                 const float (&Tc)[CM], const float (&Tr)[CM], float (&dT)[CM],
                                                 const float* s_al, float& dstart, float& dend) {
    const int C = a.C, S = a.S;
    const bool lane_on = j < C;
    const float sg = R ? 1.f : -1.f;
    const float* eb = a.e + (int64_t)b * S * a.ld;
    float* deb = a.de + (int64_t)b * S * a.ldd;
    float beta = lane_on ? a.end[j] : -INFINITY;
    int t = L > 1 ? prev_on(s_on, S) : 0;   // the last on-position
    float e_n = lane_on ? eb[(int64_t)t * a.ld + j] : 0.f;
    float d_n = (R && lane_on) ? deb[(int64_t)t * a.ldd + j] : 0.f;
    u64 w_n = R ? allowed_at(a, b, t) : 0ull;
    float al = lane_on ? s_al[(L - 1) * C + j] : -INFINITY;
    for (int i = L - 1; i >= 0; --i) {
        const float et = e_n, d_old = d_n;
        const bool ok = lane_on && (!R || ((w_n >> j) & 1ull));
        const int tc = t;
        float al_p = -INFINITY;   // alpha_{i-1}[j]
        if (i > 0) {   // the next step's operands: in flight during this step's arithmetic
            t = prev_on(s_on, t);
            if (lane_on) { e_n = eb[(int64_t)t * a.ld + j]; al_p = s_al[(i - 1) * C + j]; }
            if (R && lane_on) d_n = deb[(int64_t)t * a.ldd + j];
            if (R) w_n = allowed_at(a, b, t);
        }
        const float pm = lane_on ? __expf(al + beta - logz) : 0.f;   // alpha = -inf outside A_i: exactly 0
        if (lane_on) deb[(int64_t)tc * a.ldd + j] = R ? d_old + g * pm : -(g * pm);
        if (i == L - 1) dend += sg * pm;
        if (i == 0) { dstart += sg * pm; break; }
        const float u = ok ? et + beta : -INFINITY;   // x_i[j] + beta_i[j], tags outside A_i drop out
        const float c = u - logz;
#pragma unroll
        for (int k = 0; k < CM; ++k) dT[k] += sg * __expf(lane_f32(al_p, k) + Tc[k] + c);   // Tc = -inf past C: + 0
        const float nb = lse_lanes(u, Tr);   // beta_{i-1}[j] = lse_k (T[j][k] + u[k])
        beta = lane_on ? nb : -INFINITY;
        al = al_p;
    }
}

// ------------------------------------------------------------------------------------------------ log-likelihood
__global__ __launch_bounds__(64) void crf_constrained_llh_kernel(const ConArgs a) {
    __shared__ float s_T[64 * 64];
    __shared__ float s_al[2 * 64];
    __shared__ u64 s_on[ON_WORDS];
    const int b = blockIdx.x, j = threadIdx.x, C = a.C;
    bool feasible;
    scan_sample(a, b, j, s_on, feasible);
    for (int i = j; i < C * C; i += 64) s_T[i] = a.trans[i];
    __syncthreads();
    const float logz = con_forward<false, false>(a, b, j, s_on, s_T, s_al);
    float logza = -INFINITY, llh = -INFINITY;
    if (feasible) {
        __syncthreads();
        logza = con_forward<true, false>(a, b, j, s_on, s_T, s_al);
        llh = logza - logz;
    }
    if (j == 0) {
        a.log_z[b] = logz;
        a.log_za[b] = logza;
        a.llh[b] = llh;
        if (!feasible && a.infeasible) atomicAdd(a.infeasible, 1);
    }
}

__global__ __launch_bounds__(64) void crf_constrained_llh_small_kernel(const ConArgs a) {   // C <= 16
    __shared__ u64 s_on[ON_WORDS];
    const int b = blockIdx.x, j = threadIdx.x;
    bool feasible;
    scan_sample(a, b, j, s_on, feasible);
    float Tc[CM], Tr[CM];
    load_T(a, j, Tc, Tr);
    __syncthreads();
    const float logz = con_forward_reg<false, false>(a, b, j, s_on, Tc, nullptr);
    float logza = -INFINITY, llh = -INFINITY;
    if (feasible) {
        logza = con_forward_reg<true, false>(a, b, j, s_on, Tc, nullptr);
        llh = logza - logz;
    }
    if (j == 0) {
        a.log_z[b] = logz;
        a.log_za[b] = logza;
        a.llh[b] = llh;
        if (!feasible && a.infeasible) atomicAdd(a.infeasible, 1);
    }
}

// ------------------------------------------------------------------------------------------------------ gradient
__global__ __launch_bounds__(64) void crf_constrained_grad_kernel(const ConArgs a) {
    __shared__ float s_T[64 * 64];
    __shared__ float s_dT[64 * 64];
    __shared__ float s_vec[64];
    __shared__ float s_al[CRF_MAX_SC];   // alpha of on-position i at [i * C + j], one lattice at a time
    __shared__ u64 s_on[ON_WORDS];
    const int b = blockIdx.x, j = threadIdx.x, C = a.C;
    bool feasible;
    const int L = scan_sample(a, b, j, s_on, feasible);
    if (!feasible) { zero_all_rows(a, b, j); return; }   // wave-uniform: nothing for the parameters
    for (int i = j; i < C * C; i += 64) { s_T[i] = a.trans[i]; s_dT[i] = 0.f; }
    __syncthreads();
    zero_off_rows(a, b, j, s_on);
    const float g = a.gllh[b];
    float dstart = 0.f, dend = 0.f;
    const float logz = con_forward<false, true>(a, b, j, s_on, s_T, s_al);
    con_backward<false>(a, b, j, L, g, logz, s_on, s_T, s_dT, s_al, s_vec, dstart, dend);
    __syncthreads();   // the free lattice has read its last alpha
    const float logza = con_forward<true, true>(a, b, j, s_on, s_T, s_al);
    con_backward<true>(a, b, j, L, g, logza, s_on, s_T, s_dT, s_al, s_vec, dstart, dend);
    if (j < C) {
        atomicAdd(a.dstart + j, g * dstart);
        atomicAdd(a.dend + j, g * dend);
    }
    __syncthreads();   // block = one wave: orders the LDS exchange
    for (int i = j; i < C * C; i += 64) atomicAdd(a.dtrans + i, g * s_dT[i]);
}

__global__ __launch_bounds__(64) void crf_constrained_grad_small_kernel(const ConArgs a) {   // C <= 16
    __shared__ float s_al[CRF_MAX_SC];   // alpha of on-position i at [i * C + j], one lattice at a time
    __shared__ u64 s_on[ON_WORDS];
    const int b = blockIdx.x, j = threadIdx.x, C = a.C;
    bool feasible;
    const int L = scan_sample(a, b, j, s_on, feasible);
    if (!feasible) { zero_all_rows(a, b, j); return; }   // wave-uniform: nothing for the parameters
    float Tc[CM], Tr[CM], dT[CM];
    load_T(a, j, Tc, Tr);
#pragma unroll
    for (int k = 0; k < CM; ++k) dT[k] = 0.f;
    __syncthreads();
    zero_off_rows(a, b, j, s_on);
    const float g = a.gllh[b];
    float dstart = 0.f, dend = 0.f;
    const float logz = con_forward_reg<false, true>(a, b, j, s_on, Tc, s_al);
    __syncthreads();   // block = one wave: the alphas are in LDS
    con_backward_reg<false>(a, b, j, L, g, logz, s_on, Tc, Tr, dT, s_al, dstart, dend);
    __syncthreads();   // the free lattice has read its last alpha
    const float logza = con_forward_reg<true, true>(a, b, j, s_on, Tc, s_al);
    __syncthreads();   // block = one wave: the alphas are in LDS
    con_backward_reg<true>(a, b, j, L, g, logza, s_on, Tc, Tr, dT, s_al, dstart, dend);
    if (j < C) {
        atomicAdd(a.dstart + j, g * dstart);
        atomicAdd(a.dend + j, g * dend);
#pragma unroll
        for (int k = 0; k < CM; ++k)
            if (k < C) atomicAdd(a.dtrans + k * C + j, g * dT[k]);
    }
}

// ------------------------------------------------------------------------------------------------------- Viterbi
// sum over the samples r < b of their numbers of on-positions (wave-uniform)
__device__ __forceinline__ int64_t con_flat_offset(const ConArgs& a, int b, int lane) {
    if (a.mask == nullptr) return (int64_t)b * a.S;
    int64_t off = 0;
    for (int r = 0; r < b; ++r) {
        const int64_t* mr = a.mask + (int64_t)r * a.S;
        int n = 0;
        for (int t0 = 0; t0 < a.S; t0 += 64) {
            const int t = t0 + lane;
            n += __popcll(__ballot(t < a.S && (t == 0 || mr[t] != 0)));
        }
        off += n;
    }
    return off;
}

// lens[b], this sample's offset, and for an infeasible sample its -1 / -inf outputs -> false (wave-uniform)
__device__ __forceinline__ bool decode_prologue(const ConArgs& a, int b, int j, u64* s_on, int& L, int64_t& off) {
    bool feasible;
    L = scan_sample(a, b, j, s_on, feasible);   // 1 <= L <= S
    off = con_flat_offset(a, b, j);             // off + L <= B * S <= capacity
    if (j == 0) a.lens[b] = L;
    if (feasible) return true;
    for (int i = j; i < L; i += 64) a.flat[off + i] = -1;
    if (j == 0) {
        a.scores[b] = -INFINITY;
        if (a.infeasible) atomicAdd(a.infeasible, 1);
    }
    return false;
}
// (one lane) the best final tag -- the first maximum -- and the path along the back-pointers
__device__ __forceinline__ void decode_backtrace(const ConArgs& a, int b, int L, int64_t off, const float* s_fin,
                                                 const unsigned char* s_bp) {
    const int C = a.C;
    int bt = 0;
    float bs = s_fin[0];
    for (int k = 1; k < C; ++k)
        if (s_fin[k] > bs) { bs = s_fin[k]; bt = k; }
    a.scores[b] = bs;
    int32_t* out = a.flat + off;
    out[L - 1] = bt;
    for (int q = L - 1; q >= 1; --q) {
        bt = s_bp[q * C + bt];
        out[q - 1] = bt;
    }
}

// REG: the scores on the lanes and the transition column in registers (C <= 16); else both through LDS.
// A tag outside A_i scores -inf: `>` against a running maximum that starts at -inf never selects it.
template <bool REG>
__device__ __forceinline__ void decode_body(const ConArgs& a, float* s_T, float* s_alpha, unsigned char* s_bp, u64* s_on) {
    const int b = blockIdx.x, j = threadIdx.x, C = a.C, S = a.S;
    const bool lane_on = j < C;
    int L;
    int64_t off;
    if (!decode_prologue(a, b, j, s_on, L, off)) return;
    float Tc[CM];
    if (REG) {
#pragma unroll
        for (int k = 0; k < CM; ++k) Tc[k] = (lane_on && k < C) ? a.trans[k * C + j] : -INFINITY;
    } else {
        for (int i = j; i < C * C; i += 64) s_T[i] = a.trans[i];
    }
    __syncthreads();
    const float* eb = a.e + (int64_t)b * S * a.ld;
    float score = (lane_on && ((allowed_at(a, b, 0) >> j) & 1ull)) ? a.start[j] + eb[j] : -INFINITY;
    int t = next_on(s_on, 0, S);
    float e_n = (lane_on && t < S) ? eb[(int64_t)t * a.ld + j] : 0.f;
    u64 w_n = t < S ? allowed_at(a, b, t) : 0ull;
    int i = 0;
    while (t < S) {   // wave-uniform
        const float et = e_n;
        const bool ok = lane_on && ((w_n >> j) & 1ull);
        t = next_on(s_on, t, S);
        if (t < S) {   // the next step's operands: in flight during this step's arithmetic
            if (lane_on) e_n = eb[(int64_t)t * a.ld + j];
            w_n = allowed_at(a, b, t);
        }
        ++i;
        float m = -INFINITY;
        int am = 0;
        if (REG) {
#pragma unroll
            for (int k = 0; k < CM; ++k) {   // (every lane takes part in the lane reads; Tc = -inf past C)
                const float v = lane_f32(score, k) + Tc[k];
                if (v > m) { m = v; am = k; }
            }
        } else {
            __syncthreads();   // block = one wave: orders the LDS exchange
            if (lane_on) s_alpha[j] = score;
            __syncthreads();   // block = one wave: orders the LDS exchange
            if (lane_on)
                for (int k = 0; k < C; ++k) {
                    const float v = s_alpha[k] + s_T[k * C + j];
                    if (v > m) { m = v; am = k; }
                }
        }
        if (lane_on) s_bp[i * C + j] = (unsigned char)am;
        score = ok ? m + et : -INFINITY;
    }
    __syncthreads();   // block = one wave: orders the LDS exchange
    if (lane_on) s_alpha[j] = score + a.end[j];
    __syncthreads();   // block = one wave: orders the LDS exchange
    if (j == 0) decode_backtrace(a, b, L, off, s_alpha, s_bp);
}

__global__ __launch_bounds__(64) void crf_constrained_decode_kernel(const ConArgs a) {
    __shared__ float s_T[64 * 64];
    __shared__ float s_alpha[64];
    __shared__ unsigned char s_bp[CRF_MAX_SC];   // back-pointers [i][j] of the on-positions
    __shared__ u64 s_on[ON_WORDS];
    decode_body<false>(a, s_T, s_alpha, s_bp, s_on);
}

__global__ __launch_bounds__(64) void crf_constrained_decode_small_kernel(const ConArgs a) {   // C <= 16
    __shared__ float s_alpha[64];
    __shared__ unsigned char s_bp[CRF_MAX_SC];
    __shared__ u64 s_on[ON_WORDS];
    decode_body<true>(a, nullptr, s_alpha, s_bp, s_on);
}

inline int con_check(const void* e, const void* allowed, const void* start, const void* end, const void* trans, int64_t ld,
                     int B, int S, int C) {
    if (!e || !allowed || !start || !end || !trans || ld < C) return ICKA_E_ARG;
    if (B <= 0 || S <= 0 || C <= 0 || C > 64 || (int64_t)S * C > CRF_MAX_SC) return ICKA_E_SHAPE;
    return 0;
}

}  // namespace

extern "C" int icka_crf_constrained_llh(const float* emissions, int64_t ld, const int64_t* mask, const int64_t* allowed,
                                        const float* start, const float* end, const float* trans, float* llh, float* log_z,
                                        float* log_za, int32_t* infeasible, int32_t B, int32_t S, int32_t C, void* stream) {
    if (int rc = con_check(emissions, allowed, start, end, trans, ld, B, S, C)) return rc;
    if (!llh || !log_z || !log_za) return ICKA_E_ARG;
    ConArgs a{};
    a.e = emissions; a.ld = ld; a.mask = mask; a.allowed = allowed; a.start = start; a.end = end; a.trans = trans;
    a.llh = llh; a.log_z = log_z; a.log_za = log_za; a.infeasible = infeasible; a.B = B; a.S = S; a.C = C;
    if (C <= CM) hipLaunchKernelGGL(crf_constrained_llh_small_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(crf_constrained_llh_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_crf_constrained_grad(const float* emissions, int64_t ld, const int64_t* mask, const int64_t* allowed,
                                         const float* start, const float* end, const float* trans, const float* gllh,
                                         float* d_emissions, int64_t ldd, float* d_start, float* d_end, float* d_trans,
                                         int32_t B, int32_t S, int32_t C, void* stream) {
    if (int rc = con_check(emissions, allowed, start, end, trans, ld, B, S, C)) return rc;
    if (!gllh || !d_emissions || !d_start || !d_end || !d_trans || ldd < C) return ICKA_E_ARG;
    ConArgs a{};
    a.e = emissions; a.ld = ld; a.mask = mask; a.allowed = allowed; a.start = start; a.end = end; a.trans = trans;
    a.gllh = gllh; a.de = d_emissions; a.ldd = ldd; a.dstart = d_start; a.dend = d_end; a.dtrans = d_trans;
    a.B = B; a.S = S; a.C = C;
    if (C <= CM) hipLaunchKernelGGL(crf_constrained_grad_small_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(crf_constrained_grad_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_crf_constrained_decode(const float* emissions, int64_t ld, const int64_t* mask, const int64_t* allowed,
                                           const float* start, const float* end, const float* trans, int32_t* lens,
                                           int32_t* tags_flat, int64_t capacity, float* scores, int32_t* infeasible,
                                           int32_t B, int32_t S, int32_t C, void* stream) {
    if (int rc = con_check(emissions, allowed, start, end, trans, ld, B, S, C)) return rc;
    if (!lens || !tags_flat || !scores) return ICKA_E_ARG;
    if (B > CRF_FLAT_MAX_B || capacity < (int64_t)B * S) return ICKA_E_SHAPE;
    ConArgs a{};
    a.e = emissions; a.ld = ld; a.mask = mask; a.allowed = allowed; a.start = start; a.end = end; a.trans = trans;
    a.lens = lens; a.flat = tags_flat; a.scores = scores; a.infeasible = infeasible; a.B = B; a.S = S; a.C = C;
    if (C <= CM) hipLaunchKernelGGL(crf_constrained_decode_small_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(crf_constrained_decode_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    ICKA_CHECK_LAUNCH();
    return 0;
}
