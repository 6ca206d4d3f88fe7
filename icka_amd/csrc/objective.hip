// Auxiliary training objective of the gated taggers (my_bert/gate_cl_modeling.py:1276-1395, cl_modeling.py:1376-1382):
//   * the text <-> image contrastive (InfoNCE) loss over the two projection heads, forward and gradient;
//   * the two-class relevance cross-entropy of gate_cl (crs_loss, :1385), folded into the same two launches;
//   * the ReLU backward of the heads' hidden activations;
//   * the negative-sample pair swap of the cross-modal stream (:1345-1356).
// The problems are tiny (B <= 256 samples, D <= 4096): the structure is chosen for latency, not for MFMA rate.  Every reduction
// runs in a fixed order (no float atomics), so two runs are bitwise equal.
#include "common.h"

namespace {

constexpr int kMaxB = 256;
constexpr int kMaxD = 4096;
constexpr int kFwdThreads = 1024;        // 32 x 32 threads, thread (ty, tx) owns the (ty + 32a, tx + 32b) cosine entries
constexpr int kStageFloats = 6144;       // LDS staging of one K chunk of t and of v (f32, transposed)
constexpr int kBwdThreads = 256;         // one block per output row, 8-element chunks c = tid, tid + 256 (D / 8 <= 512)

template <typename T> __device__ __forceinline__ float ld1(const T* p) { return (float)*p; }

template <typename T> __device__ __forceinline__ void ld8f(const T* p, float (&o)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (float)p[e];
}

__device__ __forceinline__ float block_sum256(float v, float* red) {   // 256 threads = 4 waves, fixed combination order
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ws layout (f32): S [B*B] = cos(t_i, v_j) / temp, then per row (text -> image) and per column (image -> text) the max m and
// L = log(sum exp(s - m)) = log1p(sum over all but one maximal entry): [m_row B][m_col B][L_row B][L_col B], |t_i| [B], |v_j| [B].
// Keeping m and L apart (and log1p / expm1 where the softmax is close to one-hot) holds the loss and the gradient to f32
// relative precision when the matching pair dominates (loss ~ exp(-10) at temp 0.05) instead of the 1e-7 of lse's rounding.
// NB = ceil(B / 32) rounded up to a power of two: the (ty + 32a, tx + 32b) tile loops are compile-time (a guarded 8 x 8 tile
// executes ~100 instructions per k for the single entry a thread owns at B <= 32)
template <typename T, int NB>
__global__ __launch_bounds__(kFwdThreads) void contrastive_fwd_kernel(const T* __restrict__ t, int64_t ldt, const T* __restrict__ v,
                                                                      int64_t ldv, int B, int D, float temp, float temp_lamb,
                                                                      const float* __restrict__ crs, int n_neg,
                                                                      float* __restrict__ stats, float* __restrict__ ws) {
    __shared__ float stage[2 * kStageFloats];
    __shared__ float nrm[2 * kMaxB];
    __shared__ float term[2 * kMaxB];
    __shared__ float part[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* S = ws;
    // ---- row norms of t and v (no epsilon, as the reference's torch.norm)
    for (int r = wave; r < 2 * B; r += kFwdThreads / 64) {
        const T* x = r < B ? t + (int64_t)r * ldt : v + (int64_t)(r - B) * ldv;
        float s = 0.f;
        for (int d = lane * 8; d < D; d += 512) {
            float o[8];
            ld8f(x + d, o);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += o[e] * o[e];
        }
        s = wave_sum(s);
        if (lane == 0) nrm[r] = sqrtf(s);
    }
    // ---- dot products t_i . v_j, K chunks staged transposed in LDS ([k][i], row stride ldp)
    const int ldp = NB * 32 + 1;
    const int kc = (kStageFloats / ldp) & ~7;           // >= 16 for B <= 256
    const int ty = tid >> 5, tx = tid & 31;
    float acc[NB][NB];
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = 0.f;
    for (int k0 = 0; k0 < D; k0 += kc) {
        // 8 consecutive elements per thread and pass (kc and D are multiples of 8): the loads of a pass are independent
        const int gpr = kc >> 3, n = B * gpr;
        for (int idx = tid; idx < 2 * n; idx += kFwdThreads) {
            const int which = idx >= n;
            const int rem = idx - which * n;
            const int i = rem / gpr, kg = rem - i * gpr, k = k0 + kg * 8;
            float o[8];
            if (k < D) {
                ld8f(which ? v + (int64_t)i * ldv + k : t + (int64_t)i * ldt + k, o);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = 0.f;
            }
            float* dst = stage + which * kStageFloats + kg * 8 * ldp + i;
#pragma unroll
            for (int e = 0; e < 8; ++e) dst[e * ldp] = o[e];
        }
        __syncthreads();
        const int kn = min(kc, D - k0);
        for (int kk = 0; kk < kn; ++kk) {
            const float* st = stage + kk * ldp;
            const float* sv = stage + kStageFloats + kk * ldp;
            float bv[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) bv[b] = sv[tx + 32 * b];
#pragma unroll
            for (int a = 0; a < NB; ++a) {
                const float av = st[ty + 32 * a];
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[a][b] += av * bv[b];
            }
        }
        __syncthreads();
    }
    const float* nt = nrm;
    const float* nv = nrm + B;
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int i = ty + 32 * a, j = tx + 32 * b;
            if (i < B && j < B) S[(int64_t)i * B + j] = (acc[a][b] / (nt[i] * nv[j])) / temp;
        }
    __threadfence_block();
    __syncthreads();
    // ---- log-sum-exp of every row (text -> image) and every column (image -> text), max-shifted
    for (int r = wave; r < 2 * B; r += kFwdThreads / 64) {
        const bool row = r < B;
        const int q = row ? r : r - B;
        float m = -INFINITY;
        for (int j = lane; j < B; j += 64) m = fmaxf(m, row ? S[(int64_t)q * B + j] : S[(int64_t)j * B + q]);
        m = wave_max(m);
        int jm = B;                                       // first maximal entry: left out of the log1p sum
        for (int j = lane; j < B; j += 64)
            if ((row ? S[(int64_t)q * B + j] : S[(int64_t)j * B + q]) == m) jm = min(jm, j);
        jm = -(int)wave_max(-(float)jm);
        float s = 0.f;
        for (int j = lane; j < B; j += 64)
            if (j != jm) s += expf((row ? S[(int64_t)q * B + j] : S[(int64_t)j * B + q]) - m);
        s = wave_sum(s);
        if (lane == 0) {
            const float L = log1pf(s);
            term[r] = (m - S[(int64_t)q * B + q]) + L;    // lse - s_qq
            ws[(int64_t)B * B + r] = m;
            ws[(int64_t)B * B + 2 * B + r] = L;
        }
    }
    __syncthreads();
    if (wave == 0) {
        float s = 0.f;
        for (int i = lane; i < B; i += 64) {
            s += temp_lamb * term[i] + (1.f - temp_lamb) * term[B + i];
        }
        s = wave_sum(s);
        if (lane == 0) part[0] = s / (float)B;
    } else if (wave == 1) {
        float s = 0.f;
        if (crs != nullptr) {
            for (int b = lane; b < B; b += 64) {
                const float c0 = crs[2 * b], c1 = crs[2 * b + 1];
                const float m = fmaxf(c0, c1);
                const float l = m + log1pf(expf(fminf(c0, c1) - m));
                s += l - (b >= B - n_neg ? c0 : c1);
            }
        }
        s = wave_sum(s);
        if (lane == 0) part[1] = s / (float)B;
    }
    __syncthreads();
    if (tid < 2 * B) ws[(int64_t)B * B + 4 * B + tid] = nrm[tid];
    if (tid < 2) stats[tid] = part[tid];
}

// Block r < B: dt_r; block B + r: dv_r.
//   G_ij = (1/B) [tl (softmax_row_i(j) - d_ij) + (1 - tl)(softmax_col_j(i) - d_ij)] / temp     (times dloss_cl)
//   dt^_i = sum_j G_ij v^_j,  dv^_j = sum_i G_ij t^_i,  dx = (dx^ - x^ (x^ . dx^)) / |x|
template <typename T>
__global__ __launch_bounds__(kBwdThreads) void contrastive_bwd_kernel(const T* __restrict__ t, int64_t ldt, const T* __restrict__ v,
                                                                      int64_t ldv, int B, int D, float temp, float temp_lamb,
                                                                      const float* __restrict__ ws, const float* __restrict__ dcl,
                                                                      const float* __restrict__ dcrs_loss,
                                                                      float* __restrict__ dt, float* __restrict__ dv,
                                                                      const float* __restrict__ crs, int n_neg,
                                                                      float* __restrict__ dcrs) {
    __shared__ float g[kMaxB];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const bool text = blockIdx.x < (unsigned)B;
    const int r = text ? blockIdx.x : blockIdx.x - B;
    const float* S = ws;
    const float* m_row = ws + (int64_t)B * B;
    const float* m_col = m_row + B;
    const float* L_row = m_col + B;
    const float* L_col = L_row + B;
    const float* nt = L_col + B;
    const float* nv = nt + B;
    const float coef = *dcl / ((float)B * temp);
    for (int j = tid; j < B; j += kBwdThreads) {
        const int i = text ? r : j, c = text ? j : r;     // entry (i, c) of G
        const float s = S[(int64_t)i * B + c];
        const float xr = (s - m_row[i]) - L_row[i], xc = (s - m_col[c]) - L_col[c];
        // softmax - delta; expm1 on the diagonal, where the softmax may be within an ulp of one
        const float pr = i == c ? expm1f(xr) : expf(xr), pc = i == c ? expm1f(xc) : expf(xc);
        const float G = temp_lamb * pr + (1.f - temp_lamb) * pc;
        g[j] = G * coef / (text ? nv[j] : nt[j]);
    }
    __syncthreads();
    const T* other = text ? v : t;
    const int64_t ldo = text ? ldv : ldt;
    const T* own = text ? t + (int64_t)r * ldt : v + (int64_t)r * ldv;
    const float n = text ? nt[r] : nv[r];
    const int nch = D >> 3;
    float acc[2][8], x[2][8];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[c][e] = x[c][e] = 0.f;
    for (int j = 0; j < B; ++j) {
        const float gj = g[j];
        const T* row = other + (int64_t)j * ldo;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int ch = tid + c * kBwdThreads;
            if (ch < nch) {
                float o[8];
                ld8f(row + ch * 8, o);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[c][e] += gj * o[e];
            }
        }
    }
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int ch = tid + c * kBwdThreads;
        if (ch < nch) {
            ld8f(own + ch * 8, x[c]);
#pragma unroll
            for (int e = 0; e < 8; ++e) dot += x[c][e] * acc[c][e];
        }
    }
    const float proj = block_sum256(dot, red) / (n * n);     // (x^ . dx^) / |x|
    float* out = (text ? dt : dv) + (int64_t)r * D;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int ch = tid + c * kBwdThreads;
        if (ch < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) out[ch * 8 + e] = (acc[c][e] - x[c][e] * proj) / n;
        }
    }
    if (blockIdx.x == 0 && crs != nullptr) {
        const float dc = *dcrs_loss / (float)B;
        for (int b = tid; b < B; b += kBwdThreads) {
            const float c0 = crs[2 * b], c1 = crs[2 * b + 1];
            const float m = fmaxf(c0, c1);
            const float e0 = expf(c0 - m), e1 = expf(c1 - m);
            const float p0 = e0 / (e0 + e1), p1 = e1 / (e0 + e1);
            const bool neg = b >= B - n_neg;
            dcrs[2 * b] = (p0 - (neg ? 1.f : 0.f)) * dc;
            dcrs[2 * b + 1] = (p1 - (neg ? 0.f : 1.f)) * dc;
        }
    }
}

template <typename T>
__global__ void relu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y, T* __restrict__ dx, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dx[i] = ld1(y + i) > 0.f ? dy[i] : (T)0.f;
}

// y[b] = x[perm(b)]: samples b0 + i and b0 + h + i (i < h = n / 2, b0 = B - n) trade places; 16-byte words
__global__ void sample_swap_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ y, int B, int64_t words, int n_neg) {
    const int b0 = B - n_neg, h = n_neg >> 1;
    const int64_t total = (int64_t)B * words;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(w / words);
        const int64_t off = w - (int64_t)b * words;
        int src = b;
        if (b >= b0 && b < b0 + 2 * h) src = b < b0 + h ? b + h : b - h;
        y[w] = x[(int64_t)src * words + off];
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int grid_for(int64_t n, int per_block = 256, int cap = 4096) {
    const int64_t g = (n + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

template <typename T>
int launch_fwd(const void* t, int64_t ldt, const void* v, int64_t ldv, int B, int D, float temp, float tl, const float* crs,
               int n_neg, float* stats, float* ws, hipStream_t s) {
    const int nb = (B + 31) >> 5;
    auto k = nb == 1 ? contrastive_fwd_kernel<T, 1> : nb == 2 ? contrastive_fwd_kernel<T, 2>
           : nb <= 4 ? contrastive_fwd_kernel<T, 4> : contrastive_fwd_kernel<T, 8>;
    hipLaunchKernelGGL(k, dim3(1), dim3(kFwdThreads), 0, s, (const T*)t, ldt, (const T*)v, ldv, B, D, temp, tl, crs, n_neg, stats,
                       ws);
    ICKA_CHECK_LAUNCH();
    return 0;
}

template <typename T>
int launch_bwd(const void* t, int64_t ldt, const void* v, int64_t ldv, int B, int D, float temp, float tl, const float* ws,
               const float* dcl, const float* dcrs_loss, void* dt, void* dv, const float* crs, int n_neg, float* dcrs, hipStream_t s) {
    hipLaunchKernelGGL(contrastive_bwd_kernel<T>, dim3(2 * B), dim3(kBwdThreads), 0, s, (const T*)t, ldt, (const T*)v, ldv, B, D,
                       temp, tl, ws, dcl, dcrs_loss, (float*)dt, (float*)dv, crs, n_neg, dcrs);
    ICKA_CHECK_LAUNCH();
    return 0;
}

int check_shape(const void* t, int64_t ldt, const void* v, int64_t ldv, int32_t dtype, int32_t B, int32_t D, int32_t n_neg) {
    if (!t || !v) return ICKA_E_ARG;
    if (dtype < 0 || dtype > 2) return ICKA_E_ARG;
    if (B < 1 || B > kMaxB || D < 8 || D > kMaxD || (D & 7) || ldt < D || ldv < D || n_neg < 0 || n_neg > B) return ICKA_E_SHAPE;
    return 0;
}

}  // namespace

extern "C" int64_t icka_contrastive_workspace_floats(int32_t B) { return (int64_t)B * B + 6 * (int64_t)B; }

extern "C" int icka_contrastive_fwd(const void* t, int64_t ldt, const void* v, int64_t ldv, int32_t dtype, int32_t B, int32_t D,
                                    float temp, float temp_lamb, const float* crs, int32_t n_neg, float* stats, float* ws,
                                    void* stream) {
    const int rc = check_shape(t, ldt, v, ldv, dtype, B, D, n_neg);
    if (rc) return rc;
    if (!stats || !ws) return ICKA_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0) return launch_fwd<float>(t, ldt, v, ldv, B, D, temp, temp_lamb, crs, n_neg, stats, ws, s);
    if (dtype == 1) return launch_fwd<bf16_t>(t, ldt, v, ldv, B, D, temp, temp_lamb, crs, n_neg, stats, ws, s);
    return launch_fwd<_Float16>(t, ldt, v, ldv, B, D, temp, temp_lamb, crs, n_neg, stats, ws, s);
}

extern "C" int icka_contrastive_bwd(const void* t, int64_t ldt, const void* v, int64_t ldv, int32_t dtype, int32_t B, int32_t D,
                                    float temp, float temp_lamb, const float* ws, const float* dcl, const float* dcrs_loss,
                                    void* dt, void* dv, const float* crs, int32_t n_neg, float* dcrs, void* stream) {
    const int rc = check_shape(t, ldt, v, ldv, dtype, B, D, n_neg);
    if (rc) return rc;
    if (!ws || !dcl || !dt || !dv || (crs && (!dcrs || !dcrs_loss))) return ICKA_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0) return launch_bwd<float>(t, ldt, v, ldv, B, D, temp, temp_lamb, ws, dcl, dcrs_loss, dt, dv, crs, n_neg, dcrs, s);
    if (dtype == 1) return launch_bwd<bf16_t>(t, ldt, v, ldv, B, D, temp, temp_lamb, ws, dcl, dcrs_loss, dt, dv, crs, n_neg, dcrs, s);
    return launch_bwd<_Float16>(t, ldt, v, ldv, B, D, temp, temp_lamb, ws, dcl, dcrs_loss, dt, dv, crs, n_neg, dcrs, s);
}

extern "C" int icka_relu_bwd(const void* dy, const void* y, void* dx, int64_t n, int32_t is_f32, void* stream) {
    if (!dy || !y || !dx) return ICKA_E_ARG;
    if (n <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (is_f32)
        hipLaunchKernelGGL(relu_bwd_kernel<float>, dim3(grid_for(n)), dim3(256), 0, s, (const float*)dy, (const float*)y,
                           (float*)dx, n);
    else
        hipLaunchKernelGGL(relu_bwd_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, s, (const bf16_t*)dy, (const bf16_t*)y,
                           (bf16_t*)dx, n);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_sample_swap(const void* x, void* y, int32_t B, int64_t sample_bytes, int32_t n_neg, void* stream) {
    if (!x || !y || x == y) return ICKA_E_ARG;
    if (B < 1 || sample_bytes <= 0 || n_neg < 0 || n_neg > B) return ICKA_E_SHAPE;
    if ((sample_bytes & 15) || !al16(x) || !al16(y)) return ICKA_E_ALIGN;
    const int64_t words = sample_bytes >> 4;
    hipLaunchKernelGGL(sample_swap_kernel, dim3(grid_for((int64_t)B * words)), dim3(256), 0, (hipStream_t)stream,
                       (const u32x4*)x, (u32x4*)y, B, words, n_neg);
    ICKA_CHECK_LAUNCH();
    return 0;
}
