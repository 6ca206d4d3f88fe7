// Exact sampling from the linear-chain CRF (icka_crf_sample): K independent tag paths per sample drawn from p(y | x) by
// forward filtering, backward sampling.  The normative definition (the weights of every step, the inverse CDF, the uniforms)
// is written out in include/icka_hip.h; the tests replay it.
//
// ONE WAVE PER SAMPLE over the on-positions (position 0 and every t >= 1 with mask != 0), compacted with the ballots of
// crf_posterior.hip.  Lanes are cut into ROWS of RW lanes, tag j on lane j of its row:
//   C <= 16: RW = 16, four rows.  The forward pass runs once (every row computes the same alpha, row 0 stores it); then the
//            four rows draw four paths per pass, each with the DPP row reductions of crf_core.h.
//   C  > 16: RW = 64, one row, one draw per pass, wave reductions.
// Forward: the log-domain recursion of crf_posterior.hip's post_log_body, re-centred at every position; the centred alpha
// of every on-position is kept in LDS, in the slot its staged emission row was read from.
// One backward step of one draw: v_u = alpha_{i-1}(u) + trans[u, y_i] on the lanes, m = row maximum, w_u = exp(v_u - m), the
// weights through LDS, and every lane sums w_0 .. w_j in TAG ORDER (its own prefix; the additions of 0 for q > j are exact),
// so cum_j is the sequential sum of the definition and non-decreasing in j.  The drawn tag is the first set bit of the ballot
// of (w_j > 0 && cum_j > r W), else the last set bit of (w_j > 0), else 0 (non-finite input only).
// The tags of a pass stay in LDS; afterwards they are stored lanes-over-positions and the score is summed from left to right
// over 64 positions at a time (the terms are loaded lanes-over-positions, the sum runs over lane reads).
// Tags are in [0, C) by construction (a bit index below C, or 0).  All global stores are ordinary vector stores.
#include <math.h>

#include "crf_core.h"

namespace {

constexpr int SM_MAX_K = 64;

struct SampleArgs {
    const float* e; int64_t ld;
    const int64_t* mask;
    const float* start; const float* end; const float* trans;
    const uint32_t* seed_dev; uint32_t s0, s1;
    int32_t* lens; float* log_z; float* scores; int32_t* flat; int64_t cap;
    int B, S, C, K;
};

template <int RW>
__device__ __forceinline__ float row_max(float v) {
    if constexpr (RW == 16) return max16(v);
    else return wave_max(v);
}
template <int RW>
__device__ __forceinline__ float row_sum(float v) {
    if constexpr (RW == 16) return sum16(v);
    else return wave_sum(v);
}

template <int RW>
__global__ __launch_bounds__(64) void crf_sample_kernel(const SampleArgs a) {
    constexpr int G = 64 / RW;                            // draws per pass
    __shared__ float s_al[CRF_MAX_SC];                    // alpha_i[j] of the compacted sample
    __shared__ float s_T[RW * RW];
    __shared__ unsigned short s_pos[CRF_MAX_SC];          // S <= 12288 (C = 1)
    __shared__ unsigned char s_y[G * CRF_MAX_SC];         // the tags of the pass, row g at g * S
    __shared__ float s_w[2][64];                          // the weights of a step; two buffers: one barrier per step
    const int b = blockIdx.x, lane = threadIdx.x, S = a.S, C = a.C, K = a.K;
    const int g = lane / RW, j = lane % RW;
    const bool lane_on = j < C;
    const int jc = min(j, C - 1);

    // the on-positions, compacted in order
    int L = 0;
    for (int t0 = 0; t0 < S; t0 += 64) {
        const int t = t0 + lane;
        const bool on = t < S && on_pos(a, b, t);
        const unsigned long long km = __ballot(on);
        if (on) s_pos[L + __popcll(km & lanes_below(lane))] = (unsigned short)t;
        L += __popcll(km);
    }
    // sum of the path lengths of the samples before this one (crf_nbest.hip): b + the non-zero mask entries at their
    // positions >= 1
    long long off = (long long)b * S;
    if (a.mask != nullptr) {
        const int n = b * S;   // <= 2048 * 12288
        int nz = 0;
        for (int base = lane; base < n; base += 64) nz += a.mask[base] != 0 ? 1 : 0;
        for (int r = lane; r < b; r += 64) nz -= a.mask[(int64_t)r * S] != 0 ? 1 : 0;   // position 0 counts whatever its mask says
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nz += __shfl_xor(nz, o, 64);
        off = (long long)b + nz;
    }
    for (int i = lane; i < C * C; i += 64) s_T[i] = a.trans[i];
    __syncthreads();   // block = one wave: positions and transitions are in LDS
    if (off + L > a.cap) return;   // (the entry's checks leave no such sample)

    // ---- the on-positions' emission rows, staged back to back into the slots that alpha_i will take: the chain below reads
    // no global memory (x_i[j] is read from slot (i, j) before alpha_i[j] is stored there)
    const float* eb = a.e + (int64_t)b * S * a.ld;
    for (int idx = lane; idx < L * C; idx += 64) {
        const int i = idx / C, k = idx - i * C;
        s_al[idx] = eb[(int64_t)s_pos[i] * a.ld + k];
    }
    __syncthreads();   // block = one wave: the emissions are in LDS

    // ---- forward, log domain, re-centred at every position (alpha_i - kappa_i, kappa_i the row maximum: the draws need alpha_i
    // only up to a constant per position, and centred values keep their f32 digits on long chains); log Z collects the kappa_i
    float alpha = lane_on ? a.start[j] + s_al[j] : -INFINITY;
    float kappa = row_max<RW>(alpha);
    float lz = kappa;
    alpha -= kappa;
    if (lane_on && g == 0) s_al[j] = alpha;
    if constexpr (RW == 16) {
        // alpha_{i-1} sits on the lanes of every row: lane reads of row 0 in place of LDS, the transition column in registers,
        // x_i fetched from LDS one step ahead; nothing on the chain waits for memory.  The terms k >= C are exp(-inf) = +0.
        float Tc[CM];
#pragma unroll
        for (int k = 0; k < CM; ++k) Tc[k] = (lane_on && k < C) ? a.trans[k * C + j] : -INFINITY;
        float xn = s_al[min(1, L - 1) * C + jc];
        for (int i = 1; i < L; ++i) {
            const float x = xn;
            xn = s_al[min(i + 1, L - 1) * C + jc];
            float v[CM];
            float m = -INFINITY;
#pragma unroll
            for (int k = 0; k < CM; ++k) {
                v[k] = lane_f32(alpha, k) + Tc[k];
                m = fmaxf(m, v[k]);
            }
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < CM; ++k) s += __expf(v[k] - m);
            const float al = lane_on ? m + __logf(s) + x : -INFINITY;
            kappa = max16(al);
            lz += kappa;
            alpha = al - kappa;
            if (lane_on && g == 0) s_al[i * C + j] = alpha;
        }
    } else {
        for (int i = 1; i < L; ++i) {
            __syncthreads();   // block = one wave: alpha of on-position i - 1 is in LDS
            float al = -INFINITY;
            if (lane_on) {
                const float x = s_al[i * C + j];
                const float* prev = s_al + (i - 1) * C;
                float m = -INFINITY;
#pragma unroll 8
                for (int k = 0; k < C; ++k) m = fmaxf(m, prev[k] + s_T[k * C + j]);
                float s = 0.f;
#pragma unroll 8
                for (int k = 0; k < C; ++k) s += __expf(prev[k] + s_T[k * C + j] - m);
                al = m + __logf(s) + x;
            }
            kappa = wave_max(al);
            lz += kappa;
            alpha = al - kappa;
            if (lane_on) s_al[i * C + j] = alpha;
        }
    }
    __syncthreads();   // block = one wave: every alpha is in LDS
    const float endv = lane_on ? a.end[j] : 0.f;
    {
        const float v = lane_on ? alpha + endv : -INFINITY;
        const float m = row_max<RW>(v);
        const float logz = lz + (m + __logf(row_sum<RW>(lane_on ? __expf(v - m) : 0.f)));
        if (lane == 0) {
            a.lens[b] = L;
            a.log_z[b] = logz;
        }
    }

    // ---- the draws, G per pass
    uint32_t s0 = a.s0, s1 = a.s1;
    if (a.seed_dev != nullptr) { s0 ^= a.seed_dev[0]; s1 ^= a.seed_dev[1]; }
    const unsigned long long row_bits = RW == 64 ? ~0ull : ((1ull << (RW & 63)) - 1ull);
    const int row_shift = g * RW;
    for (int k0 = 0; k0 < K; k0 += G) {
        const int k = min(k0 + g, K - 1);   // a row past K repeats draw K - 1 and stores nothing
        const uint32_t ibase = (uint32_t)(b * K + k) * (uint32_t)S;
        int ynext = 0;
        for (int i = L - 1; i >= 0; --i) {
            const float t = i == L - 1 ? endv : s_T[jc * C + ynext];
            const float v = lane_on ? s_al[i * C + jc] + t : -INFINITY;
            const float m = row_max<RW>(v);
            const float w = lane_on ? __expf(v - m) : 0.f;
            float* sw = s_w[i & 1];   // (the step before read the other buffer)
            sw[lane] = w;
            __syncthreads();   // block = one wave: the weights are in LDS
            float cum = 0.f, tot = 0.f;
            if constexpr (RW == 16) {   // all 16 reads go out together; the weights of the lanes j >= C are +0
#pragma unroll
                for (int q = 0; q < CM; ++q) {
                    const float x = sw[row_shift + q];
                    tot += x;
                    cum += q <= j ? x : 0.f;
                }
            } else {
#pragma unroll 8
                for (int q = 0; q < C; ++q) {
                    const float x = sw[q];
                    tot += x;
                    cum += q <= j ? x : 0.f;
                }
            }
            const uint32_t h = icka_hash(s0, s1, ibase + (uint32_t)s_pos[i]);
            const float r = (float)(h >> 8) * 0x1p-24f;
            const float thr = r * tot;
            const bool pos = lane_on && w > 0.f;
            const unsigned long long hb = (__ballot(pos && cum > thr) >> row_shift) & row_bits;
            const unsigned long long pb = (__ballot(pos) >> row_shift) & row_bits;
            const int y = hb ? __builtin_ctzll(hb) : (pb ? 63 - __builtin_clzll(pb) : 0);
            ynext = y;
            if (j == 0) s_y[g * S + i] = (unsigned char)y;
        }
        __syncthreads();   // block = one wave: the tags of the pass are in LDS
        for (int gg = 0; gg < G && k0 + gg < K; ++gg) {
            const unsigned char* yy = s_y + gg * S;
            int32_t* out = a.flat + (int64_t)(k0 + gg) * a.cap + off;
            for (int i = lane; i < L; i += 64) out[i] = yy[i];
            // the score, summed left to right as icka_crf_nbest sums it: ((start + x_0) + trans) + x_1 .. + end
            float sc = 0.f;
            for (int base = 0; base < L; base += 64) {
                const int i = min(base + lane, L - 1);
                const int y = yy[i], yp = yy[max(i - 1, 0)];
                const float tr = i == 0 ? a.start[y] : s_T[yp * C + y];
                const float x = eb[(int64_t)s_pos[i] * a.ld + y];
                const int n = min(64, L - base);
                for (int u = 0; u < n; ++u) sc = (sc + lane_f32(tr, u)) + lane_f32(x, u);   // (u is wave-uniform)
            }
            sc += a.end[yy[L - 1]];
            if (lane == 0) a.scores[(int64_t)b * K + k0 + gg] = sc;
        }
        __syncthreads();   // block = one wave: the tags are read before the next pass overwrites them
    }
}

}  // namespace

extern "C" int icka_crf_sample(const float* emissions, int64_t ld, const int64_t* mask, const float* start, const float* end,
                               const float* trans, int32_t num_samples, uint64_t seed, const uint32_t* seed_dev,
                               int32_t* lens, float* log_z, float* scores, int32_t* tags_flat, int64_t capacity, int32_t B,
                               int32_t S, int32_t C, void* stream) {
    if (!emissions || !start || !end || !trans || !lens || !log_z || !scores || !tags_flat || ld < C) return ICKA_E_ARG;
    if (B <= 0 || S <= 0 || C <= 0 || num_samples <= 0) return ICKA_E_SHAPE;
    if (C > 64 || num_samples > SM_MAX_K || B > CRF_FLAT_MAX_B) return ICKA_E_SHAPE;
    if ((int64_t)S * C > CRF_MAX_SC || capacity < (int64_t)B * S) return ICKA_E_SHAPE;
    SampleArgs a{};
    a.e = emissions; a.ld = ld; a.mask = mask; a.start = start; a.end = end; a.trans = trans;
    a.seed_dev = seed_dev; a.s0 = (uint32_t)seed; a.s1 = (uint32_t)(seed >> 32);
    a.lens = lens; a.log_z = log_z; a.scores = scores; a.flat = tags_flat; a.cap = capacity;
    a.B = B; a.S = S; a.C = C; a.K = num_samples;
    if (C <= CM) hipLaunchKernelGGL(crf_sample_kernel<16>, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(crf_sample_kernel<64>, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    ICKA_CHECK_LAUNCH();
    return 0;
}
