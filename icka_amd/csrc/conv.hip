// Data-movement kernels of the frozen ResNet-152 image encoder (resnet/resnet.py:57-150,
// resnet/resnet_utils.py:13-53), forward only.  Every convolution is a GEMM of the GEMM kernels on NHWC bf16
// activations ([B*H*W, C] matrices, eval-mode BatchNorm folded into the weights / bias, ReLU and the residual add in
// the GEMM epilogue: ICKA_EPI_RELU / ICKA_EPI_ADD_RELU); this file only builds the GEMM operands:
//   stem_patches : [B,3,H,W] f32 NCHW image  -> 7x7 / stride 2 / pad 3 patches, bf16 [B*Ho*Wo, 192] (147 taps + zero pad)
//   im2col3x3    : NHWC bf16 -> 3x3 / pad 1 patches, stride 1 or 2, [B*Ho*Wo, 9*C]
//   subsample    : NHWC rows at (s*y, s*x) for the strided 1x1 downsample convolutions
//   maxpool3x3s2 : nn.MaxPool2d(3, 2, 1)
//   features_out : last NHWC map -> att f32 [B,C,7,7] (F.adaptive_avg_pool2d(x,[7,7]) of a 7x7 map = identity),
//                  fc = mean over the 49 positions, and the region-token matrix bf16 [B*49, C] the MNER trunk reads.
// Train-mode BatchNorm (ResNet.train_batchnorm) replaces the fold by three steps per BatchNorm: the convolution GEMM writes
// the raw output and per-tile partial statistics (gemm_fused.inc, icka_gemm_bn_stats / icka_conv3x3_gemm_stats), then
//   bn_finalize  : partials -> batch mean / variance -> scale, shift + the running-statistics update, on the device
//   bn_apply     : relu(raw * scale + shift [+ residual]), the residual optionally through the downsample's scale / shift
// Rows past the last valid row of a padded (multiple-of-128) GEMM operand are written as zeros.
#include "common.h"

namespace {

__global__ void stem_patches_kernel(const float* __restrict__ img, bf16_t* __restrict__ out, int B, int H, int W, int Ho,
                                    int Wo, int64_t rows_padded) {
    // one thread per (row, 8-element chunk of the 192-wide patch): k = (ky*7 + kx)*3 + c
    const int64_t total = rows_padded * 24;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / 24;
        const int ch = (int)(i - row * 24);
        bf16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = f2bf(0.f);
        if (row < (int64_t)B * Ho * Wo) {
            const int b = (int)(row / (Ho * Wo)), r = (int)(row - (int64_t)b * Ho * Wo), oy = r / Wo, ox = r - oy * Wo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = ch * 8 + e;
                if (k < 147) {
                    const int tap = k / 3, c = k - tap * 3, ky = tap / 7, kx = tap - ky * 7;
                    const int y = oy * 2 - 3 + ky, x = ox * 2 - 3 + kx;
                    if (y >= 0 && y < H && x >= 0 && x < W) v[e] = f2bf(img[(((int64_t)b * 3 + c) * H + y) * W + x]);
                }
            }
        }
        *reinterpret_cast<u32x4*>(out + row * 192 + ch * 8) = as_u32x4(v);
    }
}

__global__ void im2col3x3_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ out, int B, int H, int W, int C,
                                 int stride, int Ho, int Wo, int64_t rows_padded) {
    const int cpr = C >> 3;                       // 16-byte chunks per tap
    const int64_t total = rows_padded * 9 * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / (9 * cpr);
        const int rem = (int)(i - row * 9 * cpr), tap = rem / cpr, ch = rem - tap * cpr;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (row < (int64_t)B * Ho * Wo) {
            const int b = (int)(row / (Ho * Wo)), r = (int)(row - (int64_t)b * Ho * Wo), oy = r / Wo, ox = r - oy * Wo;
            const int y = oy * stride - 1 + tap / 3, x = ox * stride - 1 + tap % 3;
            if (y >= 0 && y < H && x >= 0 && x < W)
                v = *reinterpret_cast<const u32x4*>(src + (((int64_t)b * H + y) * W + x) * C + ch * 8);
        }
        *reinterpret_cast<u32x4*>(out + row * 9 * C + (int64_t)tap * C + ch * 8) = v;
    }
}

__global__ void subsample_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ out, int B, int H, int W, int C,
                                 int stride, int Ho, int Wo, int64_t rows_padded) {
    const int cpr = C >> 3;
    const int64_t total = rows_padded * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cpr;
        const int ch = (int)(i - row * cpr);
        u32x4 v = {0u, 0u, 0u, 0u};
        if (row < (int64_t)B * Ho * Wo) {
            const int b = (int)(row / (Ho * Wo)), r = (int)(row - (int64_t)b * Ho * Wo), oy = r / Wo, ox = r - oy * Wo;
            v = *reinterpret_cast<const u32x4*>(src + (((int64_t)b * H + oy * stride) * W + ox * stride) * C + ch * 8);
        }
        *reinterpret_cast<u32x4*>(out + row * C + ch * 8) = v;
    }
}

__global__ void maxpool3x3s2_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ out, int B, int H, int W, int C,
                                    int Ho, int Wo, int64_t rows_padded) {
    const int cpr = C >> 3;
    const int64_t total = rows_padded * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cpr;
        const int ch = (int)(i - row * cpr);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = f2bf(0.f);
        if (row < (int64_t)B * Ho * Wo) {
            const int b = (int)(row / (Ho * Wo)), r = (int)(row - (int64_t)b * Ho * Wo), oy = r / Wo, ox = r - oy * Wo;
            float m[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) {
                    const int y = oy * 2 - 1 + ky, x = ox * 2 - 1 + kx;
                    if (y < 0 || y >= H || x < 0 || x >= W) continue;   // padding never wins (nn.MaxPool2d pads with -inf)
                    const bf16x8 v = as_bf16x8(*reinterpret_cast<const u32x4*>(src + (((int64_t)b * H + y) * W + x) * C + ch * 8));
#pragma unroll
                    for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], bf2f(v[e]));
                }
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f2bf(m[e]);
        }
        *reinterpret_cast<u32x4*>(out + row * C + ch * 8) = as_u32x4(o);
    }
}

// x: NHWC bf16 [B, P, C] (P = 49 positions).  att f32 [B, C, P]; fc f32 [B, C]; tokens bf16 [B*P, C] (optional copy)
__global__ void features_out_kernel(const bf16_t* __restrict__ x, float* __restrict__ att, float* __restrict__ fc,
                                    bf16_t* __restrict__ tokens, int B, int P, int C) {
    const int64_t total = (int64_t)B * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / C), c = (int)(i - (int64_t)b * C);
        float s = 0.f;
        for (int p = 0; p < P; ++p) {
            const bf16_t v = x[((int64_t)b * P + p) * C + c];
            const float f = bf2f(v);
            s += f;
            att[((int64_t)b * C + c) * P + p] = f;
            if (tokens) tokens[((int64_t)b * P + p) * C + c] = v;
        }
        fc[i] = s / (float)P;
    }
}

// Train-mode BatchNorm, per channel c: merge the [tiles] partials of icka_gemm_bn_stats / icka_conv3x3_gemm_stats in a fixed
// order (thread (c, j) takes tiles j, j+16, ... in turn, then the 16 slices are merged in slice order), so an eager call and a
// graph replay give the same bits.  Block = 16 channels x 16 slices.
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ part, int tiles, int C, const float* __restrict__ weight,
                                                          const float* __restrict__ bias, float* __restrict__ running_mean,
                                                          float* __restrict__ running_var, const int64_t* __restrict__ nbt, float momentum,
                                                          float eps, float* __restrict__ scale, float* __restrict__ shift) {
    __shared__ float red[3][256];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + tx;
    const int64_t plane = (int64_t)tiles * C;
    float n = 0.f, mu = 0.f, m2 = 0.f;
    if (c < C)
        for (int t = ty; t < tiles; t += 16) {
            const int64_t at = (int64_t)t * C + c;
            bn_chan_merge(n, mu, m2, part[at], part[plane + at], part[2 * plane + at]);
        }
    red[0][threadIdx.x] = n;
    red[1][threadIdx.x] = mu;
    red[2][threadIdx.x] = m2;
    __syncthreads();
    if (ty != 0 || c >= C) return;
    for (int j = 1; j < 16; ++j) bn_chan_merge(n, mu, m2, red[0][j * 16 + tx], red[1][j * 16 + tx], red[2][j * 16 + tx]);
    const float var = n > 0.f ? m2 / n : 0.f;                 // biased: the normalisation
    const float sc = weight[c] * (1.f / sqrtf(var + eps));
    scale[c] = sc;
    shift[c] = bias[c] - mu * sc;
    // momentum < 0: cumulative average, 1 / num_batches_tracked after this call's increment (icka_bn_apply adds the 1)
    const float m = momentum >= 0.f ? momentum : 1.f / (float)(nbt[0] + 1);
    const float unbiased = n > 1.f ? var * (n / (n - 1.f)) : var;
    running_mean[c] = m * mu + (1.f - m) * running_mean[c];
    running_var[c] = m * unbiased + (1.f - m) * running_var[c];
}

__device__ __forceinline__ void load8_f32(const float* p, float (&o)[8]) {   // p 32-byte aligned
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = a[e]; o[4 + e] = b[e]; }
}

// y = [relu](raw * scale + shift [+ residual]) on rows < rows_valid, zeros on [rows_valid, rows_padded).  residual: bf16 as is, or
// (res_scale) residual * res_scale + res_shift (the downsample branch's BatchNorm).  raw / y / residual: [rows_padded, C], y may be
// raw.  The first thread also adds 1 to the num_batches_tracked counters of the BatchNorms it applies.
__global__ void bn_apply_kernel(const bf16_t* raw, const float* __restrict__ scale, const float* __restrict__ shift, const bf16_t* res,
                                const float* __restrict__ res_scale, const float* __restrict__ res_shift, bf16_t* y, int C,
                                int64_t rows_valid, int64_t rows_padded, int relu, int64_t* nbt_a, int64_t* nbt_b) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (nbt_a) nbt_a[0] = nbt_a[0] + 1;
        if (nbt_b) nbt_b[0] = nbt_b[0] + 1;
    }
    const int cpr = C >> 3;
    const int64_t total = rows_padded * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cpr;
        const int c0 = (int)(i - row * cpr) * 8;
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = f2bf(0.f);
        if (row < rows_valid) {
            const bf16x8 v = as_bf16x8(*reinterpret_cast<const u32x4*>(raw + row * C + c0));
            float r[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = 0.f;
            float sc[8], sh[8];
            load8_f32(scale + c0, sc);
            load8_f32(shift + c0, sh);
            if (res) {
                const bf16x8 rv = as_bf16x8(*reinterpret_cast<const u32x4*>(res + row * C + c0));
#pragma unroll
                for (int e = 0; e < 8; ++e) r[e] = bf2f(rv[e]);
                if (res_scale) {
                    float rs[8], rb[8];
                    load8_f32(res_scale + c0, rs);
                    load8_f32(res_shift + c0, rb);
#pragma unroll
                    for (int e = 0; e < 8; ++e) r[e] = r[e] * rs[e] + rb[e];
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float t = bf2f(v[e]) * sc[e] + sh[e] + r[e];
                o[e] = f2bf(relu ? fmaxf(t, 0.f) : t);
            }
        }
        *reinterpret_cast<u32x4*>(y + row * C + c0) = as_u32x4(o);
    }
}

inline int grid_for(int64_t n) {
    int64_t g = (n + 255) / 256;
    return (int)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int icka_conv_stem_patches(const float* image, void* patches, int32_t B, int32_t H, int32_t W,
                                      int64_t rows_padded, void* stream) {
    if (!image || !patches) return ICKA_E_ARG;
    const int Ho = (H + 6 - 7) / 2 + 1, Wo = (W + 6 - 7) / 2 + 1;
    if (B <= 0 || H < 7 || W < 7 || rows_padded < (int64_t)B * Ho * Wo) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(stem_patches_kernel, dim3(grid_for(rows_padded * 24)), dim3(256), 0, (hipStream_t)stream, image,
                       (bf16_t*)patches, B, H, W, Ho, Wo, rows_padded);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_conv_im2col3x3(const void* src, void* patches, int32_t B, int32_t H, int32_t W, int32_t C,
                                   int32_t stride, int64_t rows_padded, void* stream) {
    if (!src || !patches) return ICKA_E_ARG;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || (stride != 1 && stride != 2)) return ICKA_E_SHAPE;
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    if (rows_padded < (int64_t)B * Ho * Wo) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(im2col3x3_kernel, dim3(grid_for(rows_padded * 9 * (C / 8))), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)src, (bf16_t*)patches, B, H, W, C, stride, Ho, Wo, rows_padded);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_conv_subsample(const void* src, void* dst, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride,
                                   int64_t rows_padded, void* stream) {
    if (!src || !dst) return ICKA_E_ARG;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || stride < 1) return ICKA_E_SHAPE;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if (rows_padded < (int64_t)B * Ho * Wo) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(subsample_kernel, dim3(grid_for(rows_padded * (C / 8))), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)src, (bf16_t*)dst, B, H, W, C, stride, Ho, Wo, rows_padded);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_conv_maxpool3x3s2(const void* src, void* dst, int32_t B, int32_t H, int32_t W, int32_t C,
                                      int64_t rows_padded, void* stream) {
    if (!src || !dst) return ICKA_E_ARG;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) return ICKA_E_SHAPE;
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    if (rows_padded < (int64_t)B * Ho * Wo) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3(grid_for(rows_padded * (C / 8))), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)src, (bf16_t*)dst, B, H, W, C, Ho, Wo, rows_padded);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_bn_finalize(const float* partials, int32_t tiles, int32_t C, const float* weight, const float* bias,
                                float* running_mean, float* running_var, const int64_t* num_batches_tracked, float momentum, float eps,
                                float* scale, float* shift, void* stream) {
    if (!partials || !weight || !bias || !running_mean || !running_var || !num_batches_tracked || !scale || !shift) return ICKA_E_ARG;
    if (tiles <= 0 || C <= 0 || !(eps >= 0.f)) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 15) / 16), dim3(256), 0, (hipStream_t)stream, partials, tiles, C, weight, bias,
                       running_mean, running_var, num_batches_tracked, momentum, eps, scale, shift);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_bn_apply(const void* raw, const float* scale, const float* shift, const void* residual, const float* res_scale,
                             const float* res_shift, void* y, int32_t C, int64_t rows_valid, int64_t rows_padded, int32_t relu,
                             int64_t* nbt_a, int64_t* nbt_b, void* stream) {
    if (!raw || !scale || !shift || !y || (res_scale && (!residual || !res_shift))) return ICKA_E_ARG;
    if (C <= 0 || C % 8 || rows_valid < 0 || rows_padded < rows_valid) return ICKA_E_SHAPE;
    auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (!al(raw) || !al(y) || (residual && !al(residual)) || !al(scale) || !al(shift) || (res_scale && (!al(res_scale) || !al(res_shift))))
        return ICKA_E_ALIGN;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for(rows_padded * (C / 8))), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)raw,
                       scale, shift, (const bf16_t*)residual, res_scale, res_shift, (bf16_t*)y, C, rows_valid, rows_padded, relu,
                       nbt_a, nbt_b);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_conv_features_out(const void* x, float* att, float* fc, void* tokens, int32_t B, int32_t P, int32_t C,
                                      void* stream) {
    if (!x || !att || !fc) return ICKA_E_ARG;
    if (B <= 0 || P <= 0 || C <= 0) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(features_out_kernel, dim3(grid_for((int64_t)B * C)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)x, att, fc, (bf16_t*)tokens, B, P, C);
    ICKA_CHECK_LAUNCH();
    return 0;
}
