// Sharpness-aware minimisation (SAM, Foret et al. 2021; ASAM, Kwon et al. 2021) on the flat ParamArena buffers.  Outside the
// reference, which trains without it; off unless icka_amd.SAM is used.  A step takes the gradient at w, climbs to w + e(w),
// takes the gradient there and updates w with that second gradient.  As a stock wrapper that is two walks over ~220 parameter
// tensors with host-side norms; here parameters, gradients and the 16-bit shadows share ONE flat layout, so the ascent is
//   icka_sam_sqnorm    per-chunk sums of (t g)^2, t = 1 (plain) or |p| (adaptive)       (reads 4 / 8 B per parameter)
//   icka_sam_prepare   one block: fixed-order sum of the partials -> norm, the step scale rho / (norm + 1e-12), or the skip word
//   icka_sam_ascend    backup <- p; p <- p + e; the 16-bit shadows of the new p         (18 B per parameter, + 2 with fp16)
// and the way back, behind the second backward, is
//   icka_sam_restore   p <- backup; the 16-bit shadows of p                              (10 B per parameter, + 2 with fp16)
// The per-ascent values live in a device block (icka_sam_state, include/icka_hip.h) written by thread 0 of the prepare launch
// and read by the launches behind it on the stream: no host read, so the whole sequence can sit inside a captured step.
// Access pattern = optim_adamw_kernel's (csrc/optim.hip): 256 threads per chunk of at most 8192 elements, 16-byte accesses,
// {first element, count} tables, no atomics, LDS only for the block reduction, fixed summation order.
#include "common.h"

namespace {

using SamState = icka_sam_state;

__device__ __forceinline__ bool finite_f64(double x) {
    return ((unsigned long long)__double_as_longlong(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// partials[b] = sum over chunk b of (|p| g)^2: optim_sqnorm_kernel's loop and reduction tree with one more product per element
__global__ __launch_bounds__(256) void sam_sqnorm_adaptive_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                                  const int64_t* __restrict__ table, float* __restrict__ partials) {
    __shared__ float red[4];
    const int64_t lo = table[2 * blockIdx.x], len = table[2 * blockIdx.x + 1];
    float s = 0.f;
    for (int64_t c = threadIdx.x * 4; c < len; c += 256 * 4) {
        const f32x4 pv = *reinterpret_cast<const f32x4*>(p + lo + c);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + lo + c);
        const float a0 = fabsf(pv[0]) * gv[0], a1 = fabsf(pv[1]) * gv[1], a2 = fabsf(pv[2]) * gv[2], a3 = fabsf(pv[3]) * gv[3];
        s += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One block, after the norm launch: the sum of optim_clip_kernel (same order, in double), and what the ascent behind it uses.
// Thread 0 writes the block with ordinary stores.
__global__ __launch_bounds__(1024) void sam_prepare_kernel(const float* __restrict__ partials, int n, float rho, int flags,
                                                           SamState* __restrict__ st) {
    __shared__ double red[16];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) s += (double)partials[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int i = 0; i < 16; ++i) sum += red[i];
    if (flags & ICKA_SAM_DRY) {              // warm-up launches: nothing is applied, nothing is counted
        st->skip = 1;
        return;
    }
    const float norm = (float)sqrt(sum);
    st->norm = norm;
    if (!finite_f64(sum) || sum == 0.0) {    // inf / NaN gradient, or no gradient at all: there is no direction to climb in
        st->scale = 0.f;
        st->skip = 1;
        st->skipped += 1;
        return;
    }
    st->scale = (float)((double)rho / ((double)norm + 1e-12));
    st->skip = 0;
    st->ascents += 1;
}

template <bool ADAPTIVE>
__global__ __launch_bounds__(256) void sam_ascend_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ backup, bf16_t* __restrict__ shadow,
                                                         _Float16* __restrict__ shadow16, const int64_t* __restrict__ table,
                                                         const SamState* __restrict__ st) {
#pragma clang fp contract(off)               // every product and sum below is an f32 rounding of its own (icka_hip.h)
    if (st->skip) return;
    const float scale = st->scale;
    const int64_t lo = table[2 * blockIdx.x], len = table[2 * blockIdx.x + 1];
    for (int64_t c = threadIdx.x * 8; c < len; c += 256 * 8) {
        const int64_t i = lo + c;
        float np[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i + 4 * h);
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i + 4 * h);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float step;
                if (ADAPTIVE) {
                    const float t = pv[e] * pv[e];
                    const float u = t * gv[e];
                    step = u * scale;
                } else {
                    step = scale * gv[e];
                }
                o[e] = pv[e] + step;
                np[4 * h + e] = o[e];
            }
            *reinterpret_cast<f32x4*>(backup + i + 4 * h) = pv;
            *reinterpret_cast<f32x4*>(p + i + 4 * h) = o;
        }
        if (shadow) {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f2bf(np[e]);
            *reinterpret_cast<u32x4*>(shadow + i) = as_u32x4(o);
        }
        if (shadow16) {
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (_Float16)fminf(fmaxf(np[e], -65504.f), 65504.f);
            *reinterpret_cast<f16x8*>(shadow16 + i) = o;
        }
    }
}

// p <- backup over the chunks of the table, and the 16-bit shadows of p as optim_adamw_kernel stores them
__global__ __launch_bounds__(256) void sam_restore_kernel(float* __restrict__ p, const float* __restrict__ backup,
                                                          bf16_t* __restrict__ shadow, _Float16* __restrict__ shadow16,
                                                          const int64_t* __restrict__ table, const SamState* __restrict__ st) {
    if (st->skip) return;
    const int64_t lo = table[2 * blockIdx.x], len = table[2 * blockIdx.x + 1];
    for (int64_t c = threadIdx.x * 8; c < len; c += 256 * 8) {
        const int64_t i = lo + c;
        float np[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(backup + i + 4 * h);
            *reinterpret_cast<f32x4*>(p + i + 4 * h) = b;
#pragma unroll
            for (int e = 0; e < 4; ++e) np[4 * h + e] = b[e];
        }
        if (shadow) {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f2bf(np[e]);
            *reinterpret_cast<u32x4*>(shadow + i) = as_u32x4(o);
        }
        if (shadow16) {
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (_Float16)fminf(fmaxf(np[e], -65504.f), 65504.f);
            *reinterpret_cast<f16x8*>(shadow16 + i) = o;
        }
    }
}

}  // namespace

extern "C" int icka_sam_sqnorm(const float* params, const float* grads, const int64_t* table_dev, int32_t n_chunks,
                               int32_t adaptive, float* partials, void* stream) {
    if (!adaptive) return icka_optim_sqnorm(grads, table_dev, n_chunks, partials, stream);   // the same kernel: the same bits
    if (!params || !grads || !table_dev || !partials) return ICKA_E_ARG;
    if (n_chunks <= 0) return ICKA_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads)) & 15) return ICKA_E_ALIGN;
    hipLaunchKernelGGL(sam_sqnorm_adaptive_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, params, grads, table_dev,
                       partials);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_sam_prepare(const float* partials, int32_t n, float rho, int32_t flags, void* state, void* stream) {
    if (!state || (n > 0 && !partials)) return ICKA_E_ARG;
    if (n < 0 || !(rho > 0.f) || (flags & ~ICKA_SAM_DRY)) return ICKA_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(state) & 7) return ICKA_E_ALIGN;
    hipLaunchKernelGGL(sam_prepare_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, partials, n, rho, flags, (SamState*)state);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_sam_ascend(float* params, const float* grads, float* backup, void* shadow_bf16, void* shadow_f16,
                               const int64_t* table_dev, int32_t n_chunks, int32_t adaptive, const void* state, void* stream) {
    if (!params || !grads || !backup || !table_dev || !state || params == backup || grads == backup) return ICKA_E_ARG;
    if (n_chunks <= 0) return ICKA_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(backup) |
         reinterpret_cast<uintptr_t>(shadow_bf16) | reinterpret_cast<uintptr_t>(shadow_f16)) & 15)
        return ICKA_E_ALIGN;
    if (reinterpret_cast<uintptr_t>(state) & 7) return ICKA_E_ALIGN;
    if (adaptive)
        hipLaunchKernelGGL(sam_ascend_kernel<true>, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, params, grads, backup,
                           (bf16_t*)shadow_bf16, (_Float16*)shadow_f16, table_dev, (const SamState*)state);
    else
        hipLaunchKernelGGL(sam_ascend_kernel<false>, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, params, grads, backup,
                           (bf16_t*)shadow_bf16, (_Float16*)shadow_f16, table_dev, (const SamState*)state);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_sam_restore(float* params, const float* backup, void* shadow_bf16, void* shadow_f16, const int64_t* table_dev,
                                int32_t n_chunks, const void* state, void* stream) {
    if (!params || !backup || !table_dev || !state || params == backup) return ICKA_E_ARG;
    if (n_chunks <= 0) return ICKA_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(backup) | reinterpret_cast<uintptr_t>(shadow_bf16) |
         reinterpret_cast<uintptr_t>(shadow_f16)) & 15)
        return ICKA_E_ALIGN;
    if (reinterpret_cast<uintptr_t>(state) & 7) return ICKA_E_ALIGN;
    hipLaunchKernelGGL(sam_restore_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, params, backup, (bf16_t*)shadow_bf16,
                       (_Float16*)shadow_f16, table_dev, (const SamState*)state);
    ICKA_CHECK_LAUNCH();
    return 0;
}
