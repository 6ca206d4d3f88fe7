// exact.hip -- the fp32 "exact" arithmetic mode of the ICKA MNER hot path (include/icka_hip.h, icka_x_*).
//
// The reference is fp32 end to end (Cross_Modal_Interaction_Module.py:950 `.float()`), and
// BASELINE.json's north_star asks for logits within 1e-3 of it in fp32 (2e-2 in bf16).  The bf16-MFMA product kernels
// cannot meet 1e-3 by construction, so this file carries the same path in f32 storage and f32 arithmetic:
//   * every contraction (nn.Linear, QK^T, PV and all their gradients) is ONE batched GEMM kernel on the f32-input
//     matrix instruction v_mfma_f32_16x16x4_f32 (bit-for-bit a k-ordered fmaf chain, 1/16 of the bf16 MFMA rate);
//   * attention materialises its score tensor exactly like the reference (:488-502) -- a validation mode buys
//     exactness, not speed -- softmax / dropout / GELU / LayerNorm are straightforward f32 kernels (libm erff, expf).
// Nothing here is used by the bf16 product path, and nothing here falls back to anything: it is selected explicitly
// with icka_amd.set_precision(model, "fp32").
#include "common.h"

#include <math.h>

namespace {

// =====================================================================================================================
// Batched f32 GEMM.  C[M,N] = alpha * op(A) . op(B) (+ bias[n]) (+ beta * C) for nb0*nb1 independent problems whose
// operands differ by two batch strides (attention: batch, head).  Each operand is either "k-contiguous"
// ([rows, K], nn.Linear x and W) or "k-major" ([K, rows], the transposed uses in the gradients):
//   NT: A[M,K] B[N,K]   NN: A[M,K] B[K,N]   TN: A[K,M] B[K,N]   TT: A[K,M] B[N,K]
// 128x128x16 block tile, 4 waves of 64x64 (4x4 MFMA tiles of 16x16, 64 accumulator registers), operands staged
// global -> registers -> LDS with the next k-tile's global loads issued before the current tile's MFMAs.
constexpr int XBM = 128, XBN = 128, XBK = 16;
constexpr int XKC_LD = 20;   // k-contiguous image [128][20]: 16-byte aligned rows, fragment reads conflict-free
constexpr int XKM_LD = 144;  // k-major image [16][144]: the 4 k-rows of a fragment read land 16 banks apart
constexpr int XIMG = XBM * XKC_LD;   // floats per operand image (>= 16 * 144)

struct XGemmArgs {
    const float* A; int64_t lda, a_bs0, a_bs1;
    const float* B; int64_t ldb, b_bs0, b_bs1;
    float* C; int64_t ldc, c_bs0, c_bs1;
    const float* bias;
    int M, N, K, nb1;
    float alpha, beta;
    int a_vec, b_vec;   // 16-byte vector loads allowed (pointer, leading dimension and batch strides aligned)
};

// One k-tile of one operand: 128 rows x 16 k = 512 float4, two per thread, held in registers until the LDS store.
template <bool KM>
__device__ __forceinline__ void xload(const float* __restrict__ P, int64_t ld, int rows, int K, int row0, int k0, int vec,
                                      f32x4 (&r)[2]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int f = tid + i * 256;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (!KM) {
            const int row = row0 + (f >> 2), k = k0 + ((f & 3) << 2);
            if (row < rows && k < K) {
                const float* p = P + (int64_t)row * ld + k;
                if (vec && k + 3 < K) v = *reinterpret_cast<const f32x4*>(p);
                else {
                    v[0] = p[0];
                    if (k + 1 < K) v[1] = p[1];
                    if (k + 2 < K) v[2] = p[2];
                    if (k + 3 < K) v[3] = p[3];
                }
            }
        } else {
            const int k = k0 + (f >> 5), col = row0 + ((f & 31) << 2);
            if (k < K && col < rows) {
                const float* p = P + (int64_t)k * ld + col;
                if (vec && col + 3 < rows) v = *reinterpret_cast<const f32x4*>(p);
                else {
                    v[0] = p[0];
                    if (col + 1 < rows) v[1] = p[1];
                    if (col + 2 < rows) v[2] = p[2];
                    if (col + 3 < rows) v[3] = p[3];
                }
            }
        }
        r[i] = v;
    }
}
template <bool KM>
__device__ __forceinline__ void xstore(float* img, const f32x4 (&r)[2]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int f = tid + i * 256;
        const int off = KM ? (f >> 5) * XKM_LD + ((f & 31) << 2) : (f >> 2) * XKC_LD + ((f & 3) << 2);
        *reinterpret_cast<f32x4*>(img + off) = r[i];
    }
}
// fragment element of the 16x16x4 f32 MFMA: lane l holds op[row = l & 15][k = l >> 4]
template <bool KM>
__device__ __forceinline__ float xfrag(const float* img, int row, int k) {
    return KM ? img[k * XKM_LD + row] : img[row * XKC_LD + k];
}

template <bool A_KM, bool B_KM>
__global__ __launch_bounds__(256) void xgemm_kernel(XGemmArgs g) {
    __shared__ __attribute__((aligned(16))) float As[XIMG];
    __shared__ __attribute__((aligned(16))) float Bs[XIMG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * XBM, n0 = blockIdx.x * XBN;
    const int b0 = blockIdx.z / g.nb1, b1 = blockIdx.z - b0 * g.nb1;
    const float* A = g.A + b0 * g.a_bs0 + b1 * g.a_bs1;
    const float* B = g.B + b0 * g.b_bs0 + b1 * g.b_bs1;
    float* C = g.C + b0 * g.c_bs0 + b1 * g.c_bs1;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    f32x4 ra[2], rb[2];
    xload<A_KM>(A, g.lda, g.M, g.K, m0, 0, g.a_vec, ra);
    xload<B_KM>(B, g.ldb, g.N, g.K, n0, 0, g.b_vec, rb);
    const int nk = (g.K + XBK - 1) / XBK;
    const int fr = lane & 15, fk = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();                      // every wave is done reading the previous tile
        xstore<A_KM>(As, ra);
        xstore<B_KM>(Bs, rb);
        __syncthreads();
        if (kt + 1 < nk) {                    // next tile's global loads fly under this tile's MFMAs
            xload<A_KM>(A, g.lda, g.M, g.K, m0, (kt + 1) * XBK, g.a_vec, ra);
            xload<B_KM>(B, g.ldb, g.N, g.K, n0, (kt + 1) * XBK, g.b_vec, rb);
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            float a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                a[t] = xfrag<A_KM>(As, wm * 64 + t * 16 + fr, kk * 4 + fk);
                b[t] = xfrag<B_KM>(Bs, wn * 64 + t * 16 + fr, kk * 4 + fk);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    // D[row = 4*(lane>>4) + r][col = lane & 15]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + wn * 64 + j * 16 + fr;
            if (col >= g.N) continue;
            const float bv = g.bias ? g.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * 64 + i * 16 + fk * 4 + r;
                if (row >= g.M) continue;
                float* p = C + (int64_t)row * g.ldc + col;
                float v = g.alpha * acc[i][j][r] + bv;
                if (g.beta != 0.f) v += g.beta * *p;
                *p = v;
            }
        }
    }
}

// =====================================================================================================================
// LayerNorm (BertLayerNorm.forward :518-522: biased variance, eps inside the sqrt), f32, one wave per row.
//   y = LN(dropout(x) + residual) * gamma + beta      (x already carries the dense bias: it is the GEMM's output)
__global__ __launch_bounds__(256) void xln_fwd_kernel(const float* __restrict__ x, int64_t ldx,
                                                      const float* __restrict__ res, int64_t ldr,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float* __restrict__ y, float* __restrict__ xhat,
                                                      float* __restrict__ rstd, int M, int H, float eps, DropCfg d_) {
    const DropCfg d = drop_resolve(d_);
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* xr = x + (int64_t)row * ldx;
    const float* rr = res ? res + (int64_t)row * ldr : nullptr;
    auto val = [&](int c) {
        float v = xr[c] * drop_mul(d, (uint32_t)row * (uint32_t)H + (uint32_t)c);
        if (rr) v += rr[c];
        return v;
    };
    float s = 0.f;
    for (int c = lane; c < H; c += 64) s += val(c);
    const float mean = wave_sum(s) / (float)H;
    float q = 0.f;
    for (int c = lane; c < H; c += 64) { const float t = val(c) - mean; q += t * t; }
    const float rs = 1.f / sqrtf(wave_sum(q) / (float)H + eps);
    for (int c = lane; c < H; c += 64) {
        const float xh = (val(c) - mean) * rs;
        if (xhat) xhat[(int64_t)row * H + c] = xh;
        y[(int64_t)row * H + c] = xh * gamma[c] + beta[c];
    }
    if (rstd && lane == 0) rstd[row] = rs;
}
// dpre = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma : gradient of the LayerNorm input (= gradient of
// the residual); ddense = dpre * dropout mask (gradient of the dense branch), optional.
__global__ __launch_bounds__(256) void xln_bwd_kernel(const float* __restrict__ dy, int64_t lddy,
                                                      const float* __restrict__ xhat, const float* __restrict__ rstd,
                                                      const float* __restrict__ gamma, float* __restrict__ dpre,
                                                      float* __restrict__ ddense, int M, int H, DropCfg d_) {
    const DropCfg d = drop_resolve(d_);
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* dr = dy + (int64_t)row * lddy;
    const float* xh = xhat + (int64_t)row * H;
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < H; c += 64) {
        const float gv = dr[c] * gamma[c];
        s1 += gv;
        s2 += gv * xh[c];
    }
    s1 = wave_sum(s1) / (float)H;
    s2 = wave_sum(s2) / (float)H;
    const float rs = rstd[row];
    for (int c = lane; c < H; c += 64) {
        const float v = rs * (dr[c] * gamma[c] - s1 - xh[c] * s2);
        dpre[(int64_t)row * H + c] = v;
        if (ddense) ddense[(int64_t)row * H + c] = v * drop_mul(d, (uint32_t)row * (uint32_t)H + (uint32_t)c);
    }
}

// out[c] (+)= sum_r a[r,c] * (b ? b[r,c] : 1): bias / LayerNorm parameter gradients.  A block owns 64 columns; fixed
// summation order (4 row phases, then an LDS tree): bitwise reproducible.
__global__ __launch_bounds__(256) void xcolsum_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ b,
                                                      int64_t ldb, float* __restrict__ out, int M, int N, int accumulate) {
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + tx;
    float s = 0.f;
    if (c < N) {
        for (int r = ty; r < M; r += 4) {
            const float v = a[(int64_t)r * lda + c];
            s += b ? v * b[(int64_t)r * ldb + c] : v;
        }
    }
    red[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && c < N) {
        const float t = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
        out[c] = accumulate ? out[c] + t : t;
    }
}

// =====================================================================================================================
// Embeddings (BertEmbeddings.forward :398-412): word[ids] + position[arange(S)] + token_type[tt] -> LayerNorm.
// (the dropout after it is icka_x_dropout.)
__global__ __launch_bounds__(256) void xembed_fwd_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ tt,
                                                         const float* __restrict__ word, const float* __restrict__ pos,
                                                         const float* __restrict__ typ, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ y,
                                                         float* __restrict__ xhat, float* __restrict__ rstd, int M, int S,
                                                         int H, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* w = word + ids[row] * (int64_t)H;
    const float* p = pos + (int64_t)(row % S) * H;
    const float* t = typ + (tt ? tt[row] : 0) * (int64_t)H;
    float s = 0.f;
    for (int c = lane; c < H; c += 64) s += (w[c] + p[c]) + t[c];
    const float mean = wave_sum(s) / (float)H;
    float q = 0.f;
    for (int c = lane; c < H; c += 64) { const float v = (w[c] + p[c]) + t[c] - mean; q += v * v; }
    const float rs = 1.f / sqrtf(wave_sum(q) / (float)H + eps);
    for (int c = lane; c < H; c += 64) {
        const float xh = ((w[c] + p[c]) + t[c] - mean) * rs;
        if (xhat) xhat[(int64_t)row * H + c] = xh;
        y[(int64_t)row * H + c] = xh * gamma[c] + beta[c];
    }
    if (rstd && lane == 0) rstd[row] = rs;
}
// scatter of the LayerNorm-input gradient into the three tables (f32 atomics; nn.Embedding padding_idx row skipped)
__global__ __launch_bounds__(256) void xembed_scatter_kernel(const float* __restrict__ dpre, const int64_t* __restrict__ ids,
                                                             const int64_t* __restrict__ tt, float* __restrict__ dword,
                                                             float* __restrict__ dpos, float* __restrict__ dtyp, int M, int S,
                                                             int H, int padding_idx) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const int64_t id = ids[row];
    float* w = dword + id * (int64_t)H;
    float* p = dpos + (int64_t)(row % S) * H;
    float* t = dtyp + (tt ? tt[row] : 0) * (int64_t)H;
    const float* g = dpre + (int64_t)row * H;
    for (int c = lane; c < H; c += 64) {
        const float v = g[c];
        if (id != padding_idx) atomicAdd(w + c, v);
        atomicAdd(p + c, v);
        atomicAdd(t + c, v);
    }
}

// =====================================================================================================================
// Attention probabilities (BertSelfAttention.forward :488-500): in place  P = softmax(S * scale + mask[b, j]) over the
// key axis; Pd = dropout(P) to a second buffer when dropout is active.  One wave per (batch, head, query) row.
__global__ __launch_bounds__(256) void xsoftmax_fwd_kernel(float* __restrict__ P, float* __restrict__ Pd,
                                                           const float* __restrict__ mask, int rows, int rows_per_batch,
                                                           int Skv, float scale, DropCfg d_) {
    const DropCfg d = drop_resolve(d_);
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float* p = P + (int64_t)row * Skv;
    const float* mk = mask + (int64_t)(row / rows_per_batch) * Skv;
    float mx = -INFINITY;
    for (int j = lane; j < Skv; j += 64) mx = fmaxf(mx, p[j] * scale + mk[j]);
    mx = wave_max(mx);
    float se = 0.f;
    for (int j = lane; j < Skv; j += 64) se += expf(p[j] * scale + mk[j] - mx);
    se = wave_sum(se);
    for (int j = lane; j < Skv; j += 64) {
        const float v = expf(p[j] * scale + mk[j] - mx) / se;
        p[j] = v;
        if (Pd) Pd[(int64_t)row * Skv + j] = v * (d.thr ? drop_mul_key(d, (uint32_t)row * (uint32_t)Skv, (uint32_t)j) : d.scale);
    }
}
// in place on dPd:  dP = dPd * mask ;  dS = P * (dP - sum_j dP*P) * scale
__global__ __launch_bounds__(256) void xsoftmax_bwd_kernel(const float* __restrict__ P, float* __restrict__ dS, int rows,
                                                           int Skv, float scale, DropCfg d_) {
    const DropCfg d = drop_resolve(d_);
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* p = P + (int64_t)row * Skv;
    float* g = dS + (int64_t)row * Skv;
    float dot = 0.f;
    for (int j = lane; j < Skv; j += 64)
        dot += g[j] * (d.thr ? drop_mul_key(d, (uint32_t)row * (uint32_t)Skv, (uint32_t)j) : d.scale) * p[j];
    dot = wave_sum(dot);
    for (int j = lane; j < Skv; j += 64) {
        const float dp = g[j] * (d.thr ? drop_mul_key(d, (uint32_t)row * (uint32_t)Skv, (uint32_t)j) : d.scale);
        g[j] = p[j] * (dp - dot) * scale;
    }
}

// =====================================================================================================================
// Elementwise f32.
enum { XACT_GELU = 0, XACT_TANH = 1, XACT_SIGMOID_GATE = 2 };
__device__ __forceinline__ float xgelu(float x) { return x * 0.5f * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float xdgelu(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * expf(-0.5f * x * x);
}
// mode GELU: y = gelu(x) (gelu :31-37);  TANH: y = tanh(x) (BertPooler :675-681);
// SIGMOID_GATE: y2 = sigmoid(x), y = y2 * aux (cl_modeling.py:1363-1367)
__global__ void xact_fwd_kernel(const float* __restrict__ x, const float* __restrict__ aux, float* __restrict__ y,
                                float* __restrict__ y2, int64_t n, int mode) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = x[i];
        if (mode == XACT_GELU) y[i] = xgelu(v);
        else if (mode == XACT_TANH) y[i] = tanhf(v);
        else {
            const float s = 1.f / (1.f + expf(-v));
            y2[i] = s;
            y[i] = s * aux[i];
        }
    }
}
// GELU: dx = dy * gelu'(x_saved);  TANH: dx = dy * (1 - y_saved^2);
// SIGMOID_GATE (saved = gate g, aux = cross): dx = dy * aux * g * (1 - g), dx2 = dy * g
__global__ void xact_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ saved, const float* __restrict__ aux,
                                float* __restrict__ dx, float* __restrict__ dx2, int64_t n, int mode) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float gy = dy[i], s = saved[i];
        if (mode == XACT_GELU) dx[i] = gy * xdgelu(s);
        else if (mode == XACT_TANH) dx[i] = gy * (1.f - s * s);
        else {
            dx[i] = gy * aux[i] * s * (1.f - s);
            dx2[i] = gy * s;
        }
    }
}
__global__ void xdropout_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, DropCfg d_) {
    const DropCfg d = drop_resolve(d_);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = x[i] * drop_mul(d, (uint32_t)i);
}
// out[r, c] = a[r, c] + b[r, c] on strided 2-D views (gradient fan-in)
__global__ void xadd_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb,
                            float* __restrict__ out, int64_t ldo, int M, int N) {
    const int64_t n = (int64_t)M * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / N, c = i - r * N;
        out[r * ldo + c] = a[r * lda + c] + b[r * ldb + c];
    }
}
// out[M, Ha+Hb] = [a | b]   (cat(seq, cross) / cat(seq, gate*cross), cl_modeling.py:1363-1370)
__global__ void xconcat_kernel(const float* __restrict__ a, int64_t lda, int Ha, const float* __restrict__ b, int64_t ldb,
                               int Hb, float* __restrict__ out, int M) {
    const int W = Ha + Hb;
    const int64_t n = (int64_t)M * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / W;
        const int c = (int)(i - r * W);
        out[i] = c < Ha ? a[r * lda + c] : b[r * ldb + (c - Ha)];
    }
}
// region features -> token-major f32 [B*R, C]; layout 1: [B, C, R] (myResnet 'att' viewed (-1, 2048, 49), :956),
// layout 0: already [B, R, C]
__global__ void xregions_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int R, int Cc, int layout) {
    const int64_t n = (int64_t)B * R * Cc;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / ((int64_t)R * Cc);
        const int64_t rem = i - b * (int64_t)R * Cc;
        const int r = (int)(rem / Cc), c = (int)(rem - (int64_t)r * Cc);
        dst[i] = layout ? src[(b * Cc + c) * R + r] : src[i];
    }
}

// per-sample gates (f32 twins of fusion.hip's gate_fwd / gate_bwd kernels)
__device__ __forceinline__ float xsample_gate(const float* gate, int b, int mode) {
    if (mode == 0) return 1.f / (1.f + expf(-gate[b]));
    return 1.f / (1.f + expf(gate[2 * b] - gate[2 * b + 1]));
}
__global__ __launch_bounds__(256) void xsgate_fwd_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ c,
                                                         int64_t ldc, const float* __restrict__ gate, int mode,
                                                         float* __restrict__ out, int64_t ldo, int S, int H) {
    const int b = blockIdx.y;
    const float g = xsample_gate(gate, b, mode);
    const int total = S * H;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int s = i / H, ch = i - s * H;
        const int64_t row = (int64_t)b * S + s;
        const float x = a[row * lda + ch];
        out[row * ldo + ch] = c ? g * x + (1.f - g) * c[row * ldc + ch] : g * x;
    }
}
// one block per sample: fixed summation order
__global__ __launch_bounds__(256) void xsgate_bwd_kernel(const float* __restrict__ dout, int64_t lddo,
                                                         const float* __restrict__ a, int64_t lda,
                                                         const float* __restrict__ c, int64_t ldc,
                                                         const float* __restrict__ gate, int mode, float* __restrict__ da,
                                                         int64_t ldda, float* __restrict__ dc, int64_t lddc,
                                                         float* __restrict__ dgate, int S, int H) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    const float g = xsample_gate(gate, b, mode);
    const int total = S * H;
    float acc = 0.f;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int s = i / H, ch = i - s * H;
        const int64_t row = (int64_t)b * S + s;
        const float d = dout[row * lddo + ch];
        const float x = a[row * lda + ch];
        acc += c ? d * (x - c[row * ldc + ch]) : d * x;
        da[row * ldda + ch] = g * d;
        if (c && dc) dc[row * lddc + ch] = (1.f - g) * d;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float t = ((red[0] + red[1]) + (red[2] + red[3])) * g * (1.f - g);
        if (mode == 0) dgate[b] = t;
        else { dgate[2 * b + 1] = t; dgate[2 * b] = -t; }
    }
}

// token-level cross-entropy, mean over valid tokens; dlogits unscaled in f32
__global__ __launch_bounds__(256) void xtoken_ce_kernel(const float* __restrict__ logits, int64_t ld,
                                                        const int64_t* __restrict__ labels, const int64_t* __restrict__ mask,
                                                        float* loss_sum, float* count, float* __restrict__ dl, int M, int C) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    float loss = 0.f, cnt = 0.f;
    if (row < M) {
        const float* p = logits + (int64_t)row * ld;
        const int64_t y = labels[row];
        const bool valid = mask[row] != 0 && y >= 0 && y < C;   // the row counts (64-bit compare): loss, count AND gradient
        float mx = -INFINITY;
        for (int c = 0; c < C; ++c) mx = fmaxf(mx, p[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(p[c] - mx);
        const float lse = mx + logf(se);
        for (int c = 0; c < C; ++c)
            dl[(int64_t)row * C + c] = valid ? expf(p[c] - lse) - (c == (int)y ? 1.f : 0.f) : 0.f;
        if (valid) { loss = lse - p[y]; cnt = 1.f; }
    }
    loss = wave_sum(loss);
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt > 0.f) { atomicAdd(loss_sum, loss); atomicAdd(count, cnt); }
}
// y = x * num[0] / max(den[0], 1)
__global__ void xscale_ratio_kernel(const float* __restrict__ x, float* __restrict__ y, const float* num, const float* den,
                                    int64_t n) {
    const float s = (num ? num[0] : 1.f) / (den ? fmaxf(den[0], 1.f) : 1.f);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = x[i] * s;
}


// =====================================================================================================================
// BiLSTM recurrence in f32 (nn.LSTM(H, H, batch_first=True, bidirectional=True), Cross_Modal_Interaction_Module.py
// :905-908): the per-step gate pre-activations are gx[t] + h_{t-1} . W_hh^T, accumulated into the gate buffer by
// icka_x_gemm (batched over the two directions); these kernels are the pointwise cell update of step k for both
// directions (forward direction at t = k, reverse direction at t = S-1-k).  Gate order i, f, g, o as in PyTorch.
__global__ void xlstm_cell_fwd_kernel(float* __restrict__ gates, float* __restrict__ c_all, float* __restrict__ y,
                                      float* __restrict__ hprev, int B, int S, int H, int k) {
    const int n = 2 * B * H;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int dir = i / (B * H), r = i - dir * B * H, b = r / H, j = r - b * H;
        const int t = dir ? S - 1 - k : k, tp = dir ? t + 1 : t - 1;
        const int64_t row = (int64_t)b * S + t, rowp = (int64_t)b * S + tp;
        float* gr = gates + row * 8 * H + dir * 4 * H;
        const float ig = 1.f / (1.f + expf(-gr[j])), fg = 1.f / (1.f + expf(-gr[H + j]));
        const float gg = tanhf(gr[2 * H + j]), og = 1.f / (1.f + expf(-gr[3 * H + j]));
        const float cp = k ? c_all[rowp * 2 * H + dir * H + j] : 0.f;
        const float c = fg * cp + ig * gg;
        gr[j] = ig; gr[H + j] = fg; gr[2 * H + j] = gg; gr[3 * H + j] = og;      // activations, saved for backward
        c_all[row * 2 * H + dir * H + j] = c;
        y[row * 2 * H + dir * H + j] = og * tanhf(c);
        hprev[row * 2 * H + dir * H + j] = k ? y[rowp * 2 * H + dir * H + j] : 0.f;
    }
}
// backward of step k (run for k = S-1 .. 0): act -> dgates (pre-activation gradients) in place; dh_rec [2,B,H] is the
// gradient that reached h_t through the NEXT step's recurrent product (ignored at k = S-1); dc_carry [2,B,H] in/out.
__global__ void xlstm_cell_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ dh_rec,
                                      float* __restrict__ dc_carry, float* __restrict__ act, const float* __restrict__ c_all,
                                      int B, int S, int H, int k, int first) {
    const int n = 2 * B * H;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int dir = i / (B * H), r = i - dir * B * H, b = r / H, j = r - b * H;
        const int t = dir ? S - 1 - k : k, tp = dir ? t + 1 : t - 1;
        const int64_t row = (int64_t)b * S + t, rowp = (int64_t)b * S + tp;
        float* gr = act + row * 8 * H + dir * 4 * H;
        const float ig = gr[j], fg = gr[H + j], gg = gr[2 * H + j], og = gr[3 * H + j];
        const float c = c_all[row * 2 * H + dir * H + j], cp = k ? c_all[rowp * 2 * H + dir * H + j] : 0.f;
        const float tc = tanhf(c);
        const float dh = dy[row * 2 * H + dir * H + j] + (first ? 0.f : dh_rec[i]);
        const float dc = (first ? 0.f : dc_carry[i]) + dh * og * (1.f - tc * tc);
        gr[j] = dc * gg * ig * (1.f - ig);
        gr[H + j] = dc * cp * fg * (1.f - fg);
        gr[2 * H + j] = dc * ig * (1.f - gg * gg);
        gr[3 * H + j] = dh * tc * og * (1.f - og);
        dc_carry[i] = dc * fg;
    }
}

// =====================================================================================================================
// Embeddings of the prompt-accepting encoder stage (f32 twin of icka_embed_prompt_fwd): out[b, t] = LN(x + pos[t +
// pos_offset] + type[0]),  x = word[ids[b, src[t]]] for src[t] >= 0, prompt[b, -1-src[t]] otherwise.
__global__ __launch_bounds__(256) void xembed_prompt_fwd_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ src,
                                                                const float* __restrict__ prompt, const float* __restrict__ word,
                                                                const float* __restrict__ pos, const float* __restrict__ typ,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float* __restrict__ y, float* __restrict__ xhat,
                                                                float* __restrict__ rstd, int M, int S_in, int S, int P, int H,
                                                                int pos_offset, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const int b = row / S, sp = row - b * S, sidx = src[sp];
    const float* w = sidx < 0 ? prompt + ((int64_t)b * P + (-1 - sidx)) * H : word + ids[(int64_t)b * S_in + sidx] * (int64_t)H;
    const float* p = pos + (int64_t)(sp + pos_offset) * H;
    float s = 0.f;
    for (int c = lane; c < H; c += 64) s += (w[c] + p[c]) + typ[c];
    const float mean = wave_sum(s) / (float)H;
    float q = 0.f;
    for (int c = lane; c < H; c += 64) { const float v = (w[c] + p[c]) + typ[c] - mean; q += v * v; }
    const float rs = 1.f / sqrtf(wave_sum(q) / (float)H + eps);
    for (int c = lane; c < H; c += 64) {
        const float xh = ((w[c] + p[c]) + typ[c] - mean) * rs;
        if (xhat) xhat[(int64_t)row * H + c] = xh;
        y[(int64_t)row * H + c] = xh * gamma[c] + beta[c];
    }
    if (rstd && lane == 0) rstd[row] = rs;
}
// backward scatter of the LayerNorm-input gradient: word rows (atomics, padding row skipped), position rows, type row 0,
// and the prompt block gradient (every [b, p] row has exactly one source position: plain stores)
__global__ __launch_bounds__(256) void xembed_prompt_scatter_kernel(const float* __restrict__ dpre, const int64_t* __restrict__ ids,
                                                                    const int32_t* __restrict__ src, float* __restrict__ dword,
                                                                    float* __restrict__ dpos, float* __restrict__ dtyp,
                                                                    float* __restrict__ dprompt, int M, int S_in, int S, int P,
                                                                    int H, int pos_offset, int padding_idx) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const int b = row / S, sp = row - b * S, sidx = src[sp];
    const float* g = dpre + (int64_t)row * H;
    float* p = dpos + (int64_t)(sp + pos_offset) * H;
    if (sidx < 0) {
        float* dp = dprompt + ((int64_t)b * P + (-1 - sidx)) * H;
        for (int c = lane; c < H; c += 64) { dp[c] = g[c]; atomicAdd(p + c, g[c]); atomicAdd(dtyp + c, g[c]); }
    } else {
        const int64_t id = ids[(int64_t)b * S_in + sidx];
        float* w = dword + id * (int64_t)H;
        for (int c = lane; c < H; c += 64) {
            if (id != padding_idx) atomicAdd(w + c, g[c]);
            atomicAdd(p + c, g[c]);
            atomicAdd(dtyp + c, g[c]);
        }
    }
}

inline int xgrid(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// =====================================================================================================================
extern "C" int icka_x_gemm(const icka_xgemm_desc* d, void* stream) {
    if (!d || !d->A || !d->B || !d->C) return ICKA_E_ARG;
    if (d->M <= 0 || d->N <= 0 || d->K <= 0 || d->nb0 <= 0 || d->nb1 <= 0) return ICKA_E_SHAPE;
    if ((int64_t)d->nb0 * d->nb1 > 65535) return ICKA_E_SHAPE;
    XGemmArgs g;
    g.A = d->A; g.lda = d->lda; g.a_bs0 = d->a_bs0; g.a_bs1 = d->a_bs1;
    g.B = d->B; g.ldb = d->ldb; g.b_bs0 = d->b_bs0; g.b_bs1 = d->b_bs1;
    g.C = d->C; g.ldc = d->ldc; g.c_bs0 = d->c_bs0; g.c_bs1 = d->c_bs1;
    g.bias = d->bias;
    g.M = d->M; g.N = d->N; g.K = d->K; g.nb1 = d->nb1;
    g.alpha = d->alpha; g.beta = d->beta;
    g.a_vec = al16(d->A) && d->lda % 4 == 0 && d->a_bs0 % 4 == 0 && d->a_bs1 % 4 == 0;
    g.b_vec = al16(d->B) && d->ldb % 4 == 0 && d->b_bs0 % 4 == 0 && d->b_bs1 % 4 == 0;
    const dim3 grid((d->N + XBN - 1) / XBN, (d->M + XBM - 1) / XBM, d->nb0 * d->nb1);
    hipStream_t s = (hipStream_t)stream;
    switch (d->op) {
        case ICKA_GEMM_NT: hipLaunchKernelGGL((xgemm_kernel<false, false>), grid, dim3(256), 0, s, g); break;
        case ICKA_GEMM_NN: hipLaunchKernelGGL((xgemm_kernel<false, true>), grid, dim3(256), 0, s, g); break;
        case ICKA_GEMM_TN: hipLaunchKernelGGL((xgemm_kernel<true, true>), grid, dim3(256), 0, s, g); break;
        case ICKA_GEMM_TT: hipLaunchKernelGGL((xgemm_kernel<true, false>), grid, dim3(256), 0, s, g); break;
        default: return ICKA_E_ARG;
    }
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_x_ln_fwd(const float* x, int64_t ldx, const float* residual, int64_t ldr, const float* gamma,
                             const float* beta, float* y, float* xhat, float* rstd, int32_t M, int32_t H, float eps,
                             float p_drop, uint64_t seed, void* stream) {
    if (!x || !gamma || !beta || !y) return ICKA_E_ARG;
    if (M <= 0 || H <= 0 || (int64_t)M * H > 0xFFFFFFFFll) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(xln_fwd_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, ldx, residual, ldr, gamma,
                       beta, y, xhat, rstd, M, H, eps, make_drop(p_drop, seed));
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_ln_bwd(const float* dy, int64_t lddy, const float* xhat, const float* rstd, const float* gamma,
                             float* dpre, float* ddense, int32_t M, int32_t H, float p_drop, uint64_t seed, void* stream) {
    if (!dy || !xhat || !rstd || !gamma || !dpre) return ICKA_E_ARG;
    if (M <= 0 || H <= 0 || (int64_t)M * H > 0xFFFFFFFFll) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(xln_bwd_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, dy, lddy, xhat, rstd, gamma,
                       dpre, ddense, M, H, make_drop(p_drop, seed));
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_colsum(const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int32_t M, int32_t N,
                             int32_t accumulate, void* stream) {
    if (!a || !out) return ICKA_E_ARG;
    if (M <= 0 || N <= 0) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(xcolsum_kernel, dim3((N + 63) / 64), dim3(256), 0, (hipStream_t)stream, a, lda, b, ldb, out, M, N,
                       accumulate);
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_embed_fwd(const int64_t* ids, const int64_t* token_type, const float* word, const float* pos,
                                const float* typ, const float* gamma, const float* beta, float* y, float* xhat,
                                float* rstd, int32_t B, int32_t S, int32_t H, float eps, void* stream) {
    if (!ids || !word || !pos || !typ || !gamma || !beta || !y) return ICKA_E_ARG;
    if (B <= 0 || S <= 0 || H <= 0) return ICKA_E_SHAPE;
    const int M = B * S;
    hipLaunchKernelGGL(xembed_fwd_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, ids, token_type, word, pos,
                       typ, gamma, beta, y, xhat, rstd, M, S, H, eps);
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_embed_scatter(const float* dpre, const int64_t* ids, const int64_t* token_type, float* dword,
                                    float* dpos, float* dtyp, int32_t B, int32_t S, int32_t H, int32_t padding_idx,
                                    void* stream) {
    if (!dpre || !ids || !dword || !dpos || !dtyp) return ICKA_E_ARG;
    if (B <= 0 || S <= 0 || H <= 0) return ICKA_E_SHAPE;
    const int M = B * S;
    hipLaunchKernelGGL(xembed_scatter_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, dpre, ids, token_type,
                       dword, dpos, dtyp, M, S, H, padding_idx);
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_softmax_fwd(float* P, float* Pd, const float* add_mask, int32_t B, int32_t heads, int32_t Sq,
                                  int32_t Skv, float scale, float p_drop, uint64_t seed, void* stream) {
    if (!P || !add_mask) return ICKA_E_ARG;
    const int64_t rows = (int64_t)B * heads * Sq;
    if (rows <= 0 || Skv <= 0 || rows * Skv > 0xFFFFFFFFll) return ICKA_E_SHAPE;
    if (p_drop > 0.f && !Pd) return ICKA_E_ARG;
    hipLaunchKernelGGL(xsoftmax_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, P,
                       p_drop > 0.f ? Pd : nullptr, add_mask, (int)rows, heads * Sq, Skv, scale, make_drop(p_drop, seed));
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_softmax_bwd(const float* P, float* dS, int32_t B, int32_t heads, int32_t Sq, int32_t Skv, float scale,
                                  float p_drop, uint64_t seed, void* stream) {
    if (!P || !dS) return ICKA_E_ARG;
    const int64_t rows = (int64_t)B * heads * Sq;
    if (rows <= 0 || Skv <= 0 || rows * Skv > 0xFFFFFFFFll) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(xsoftmax_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, P, dS,
                       (int)rows, Skv, scale, make_drop(p_drop, seed));
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_act_fwd(const float* x, const float* aux, float* y, float* y2, int64_t n, int32_t mode, void* stream) {
    if (!x || !y || mode < 0 || mode > 2 || (mode == XACT_SIGMOID_GATE && (!aux || !y2))) return ICKA_E_ARG;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(xact_fwd_kernel, dim3(xgrid(n)), dim3(256), 0, (hipStream_t)stream, x, aux, y, y2, n, mode);
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_act_bwd(const float* dy, const float* saved, const float* aux, float* dx, float* dx2, int64_t n,
                              int32_t mode, void* stream) {
    if (!dy || !saved || !dx || mode < 0 || mode > 2 || (mode == XACT_SIGMOID_GATE && (!aux || !dx2))) return ICKA_E_ARG;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(xact_bwd_kernel, dim3(xgrid(n)), dim3(256), 0, (hipStream_t)stream, dy, saved, aux, dx, dx2, n, mode);
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_dropout(const float* x, float* y, int64_t n, float p_drop, uint64_t seed, void* stream) {
    if (!x || !y) return ICKA_E_ARG;
    if (n <= 0) return 0;
    if (n > 0xFFFFFFFFll) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(xdropout_kernel, dim3(xgrid(n)), dim3(256), 0, (hipStream_t)stream, x, y, n, make_drop(p_drop, seed));
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_add(const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t ldo, int32_t M,
                          int32_t N, void* stream) {
    if (!a || !b || !out) return ICKA_E_ARG;
    if (M <= 0 || N <= 0) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(xadd_kernel, dim3(xgrid((int64_t)M * N)), dim3(256), 0, (hipStream_t)stream, a, lda, b, ldb, out, ldo,
                       M, N);
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_concat2(const float* a, int64_t lda, int32_t Ha, const float* b, int64_t ldb, int32_t Hb, float* out,
                              int32_t M, void* stream) {
    if (!a || !b || !out) return ICKA_E_ARG;
    if (M <= 0 || Ha <= 0 || Hb <= 0) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(xconcat_kernel, dim3(xgrid((int64_t)M * (Ha + Hb))), dim3(256), 0, (hipStream_t)stream, a, lda, Ha, b,
                       ldb, Hb, out, M);
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_regions_to_tokens(const float* src, float* dst, int32_t B, int32_t R, int32_t C, int32_t layout,
                                        void* stream) {
    if (!src || !dst) return ICKA_E_ARG;
    if (B <= 0 || R <= 0 || C <= 0) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(xregions_kernel, dim3(xgrid((int64_t)B * R * C)), dim3(256), 0, (hipStream_t)stream, src, dst, B, R, C,
                       layout);
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_sample_gate_fwd(const float* a, int64_t lda, const float* c, int64_t ldc, const float* gate,
                                      int32_t mode, float* out, int64_t ldo, int32_t B, int32_t S, int32_t H, void* stream) {
    if (!a || !gate || !out || (mode != 0 && mode != 1)) return ICKA_E_ARG;
    if (B <= 0 || S <= 0 || H <= 0 || B > 65535) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(xsgate_fwd_kernel, dim3(xgrid((int64_t)S * H) > 64 ? 64 : xgrid((int64_t)S * H), B), dim3(256), 0,
                       (hipStream_t)stream, a, lda, c, ldc, gate, mode, out, ldo, S, H);
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_sample_gate_bwd(const float* dout, int64_t lddo, const float* a, int64_t lda, const float* c,
                                      int64_t ldc, const float* gate, int32_t mode, float* da, int64_t ldda, float* dc,
                                      int64_t lddc, float* dgate, int32_t B, int32_t S, int32_t H, void* stream) {
    if (!dout || !a || !gate || !da || !dgate || (mode != 0 && mode != 1)) return ICKA_E_ARG;
    if (B <= 0 || S <= 0 || H <= 0) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(xsgate_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, dout, lddo, a, lda, c, ldc, gate, mode,
                       da, ldda, dc, lddc, dgate, S, H);
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_token_ce(const float* logits, int64_t ld, const int64_t* labels, const int64_t* mask, float* loss_sum,
                               float* count, float* dlogits, int32_t M, int32_t C, void* stream) {
    if (!logits || !labels || !mask || !loss_sum || !count || !dlogits) return ICKA_E_ARG;
    if (M <= 0 || C <= 0 || ld < C) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(xtoken_ce_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, logits, ld, labels, mask,
                       loss_sum, count, dlogits, M, C);
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_scale_by_ratio(const float* x, float* y, const float* num, const float* den, int64_t n, void* stream) {
    if (!x || !y) return ICKA_E_ARG;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(xscale_ratio_kernel, dim3(xgrid(n)), dim3(256), 0, (hipStream_t)stream, x, y, num, den, n);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_x_lstm_cell_fwd(float* gates, float* c_all, float* y, float* hprev, int32_t B, int32_t S, int32_t H,
                                    int32_t k, void* stream) {
    if (!gates || !c_all || !y || !hprev) return ICKA_E_ARG;
    if (B <= 0 || S <= 0 || H <= 0 || k < 0 || k >= S) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(xlstm_cell_fwd_kernel, dim3(xgrid(2ll * B * H)), dim3(256), 0, (hipStream_t)stream, gates, c_all, y, hprev,
                       B, S, H, k);
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_lstm_cell_bwd(const float* dy, const float* dh_rec, float* dc_carry, float* act, const float* c_all,
                                    int32_t B, int32_t S, int32_t H, int32_t k, int32_t first, void* stream) {
    if (!dy || !dh_rec || !dc_carry || !act || !c_all) return ICKA_E_ARG;
    if (B <= 0 || S <= 0 || H <= 0 || k < 0 || k >= S) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(xlstm_cell_bwd_kernel, dim3(xgrid(2ll * B * H)), dim3(256), 0, (hipStream_t)stream, dy, dh_rec, dc_carry,
                       act, c_all, B, S, H, k, first);
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_embed_prompt_fwd(const int64_t* ids, const int32_t* src, const float* prompt, const float* word,
                                       const float* pos, const float* typ, const float* gamma, const float* beta, float* y,
                                       float* xhat, float* rstd, int32_t B, int32_t S_in, int32_t S, int32_t P, int32_t H,
                                       int32_t pos_offset, float eps, void* stream) {
    if (!ids || !src || !prompt || !word || !pos || !typ || !gamma || !beta || !y) return ICKA_E_ARG;
    if (B <= 0 || S_in <= 0 || S <= 0 || P <= 0 || H <= 0 || pos_offset < 0) return ICKA_E_SHAPE;
    const int M = B * S;
    hipLaunchKernelGGL(xembed_prompt_fwd_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, ids, src, prompt, word,
                       pos, typ, gamma, beta, y, xhat, rstd, M, S_in, S, P, H, pos_offset, eps);
    ICKA_CHECK_LAUNCH();
    return 0;
}
extern "C" int icka_x_embed_prompt_scatter(const float* dpre, const int64_t* ids, const int32_t* src, float* dword, float* dpos,
                                           float* dtyp, float* dprompt, int32_t B, int32_t S_in, int32_t S, int32_t P,
                                           int32_t H, int32_t pos_offset, int32_t padding_idx, void* stream) {
    if (!dpre || !ids || !src || !dword || !dpos || !dtyp || !dprompt) return ICKA_E_ARG;
    if (B <= 0 || S_in <= 0 || S <= 0 || P <= 0 || H <= 0 || pos_offset < 0) return ICKA_E_SHAPE;
    const int M = B * S;
    hipLaunchKernelGGL(xembed_prompt_scatter_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, dpre, ids, src, dword,
                       dpos, dtyp, dprompt, M, S_in, S, P, H, pos_offset, padding_idx);
    ICKA_CHECK_LAUNCH();
    return 0;
}
