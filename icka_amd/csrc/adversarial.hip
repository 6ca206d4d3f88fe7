// Adversarial training on the word embeddings (icka_hip.h, "adversarial training"): the kernels that turn the per-token
// gradient rows g [B, S, H] into the next perturbation delta [B, S, H] without a host round trip -- per-sample norm, step,
// projection onto the epsilon-ball, zeroing of the non-valid positions -- and the uniform start of FreeLB.
//
// Pure f32 memory sweeps.  A sample is cut into slabs of ADV_SLAB_ROWS token rows, one 256-thread block per (sample, slab):
// B * ceil(S / 8) blocks (512 at 32 x 128) instead of one block per sample.  A norm is never accumulated with atomics: every
// block leaves ONE partial sum of squares in the workspace and the next launch re-reduces the partials of its sample in a
// fixed order, so equal inputs give equal bits.  Three launches per ascent step:
//   1. adv_gnorm_kernel    ws_g[b][slab] = sum of g^2 over the slab's valid rows
//   2. adv_step_kernel     n_g = sqrt(sum_slab ws_g); u = delta + (alpha / n_g) g at valid rows (delta itself when n_g is 0
//                          or not finite), exact 0 at the others; ws_u[b][slab] = sum of u^2; norms[b][0] = n_g
//   3. adv_project_kernel  n_u = sqrt(sum_slab ws_u); if the sample stepped and n_u > epsilon: delta *= epsilon / n_u at
//                          valid rows; norms[b][1] = min(n_u, epsilon) resp. n_u
// The reduction tree of one sum of squares (stated in the header, the test bounds count its depth):
//   lane     sequential over its elements of the slab: rows wave, wave + 4 of the slab, chunks lane, lane + 64, .. of 8
//            consecutive floats each                                                          <= 2 * 4 * 8 = 64 terms
//   wave     wave_sum: four row_ror steps, then (l0 + l16) + (l32 + l48)                      depth 6
//   block    (w0 + w1) + (w2 + w3) through LDS                                                depth 2
//   sample   lane l adds partials l and l + 64 (at most 128 slabs), then wave_sum             depth 1 + 6
#include "common.h"

namespace {

constexpr int ADV_SLAB_ROWS = 8;     // token rows per block: 4 waves x 2 rows
constexpr int ADV_MAX_H = 2048;
constexpr int ADV_MAX_S = 1024;      // -> at most 128 slabs per sample: two partials per lane in the re-reduction

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// (w0 + w1) + (w2 + w3) of the four waves' sums; every thread returns the block's value
__device__ __forceinline__ float block_sum4(float wave_value, float* lds4) {
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds4[w] = wave_value;
    __syncthreads();
    const float r = (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
    __syncthreads();
    return r;
}

// sum of the nslab (<= 128) partials of one sample, the same bits in every wave of every block that asks
__device__ __forceinline__ float sample_sum(const float* part, int nslab) {
    const int lane = threadIdx.x & 63;
    const float a = lane < nslab ? part[lane] : 0.f;
    const float b = lane + 64 < nslab ? part[lane + 64] : 0.f;
    return wave_sum(a + b);
}

__device__ __forceinline__ bool steps(float n_g) { return n_g > 0.f && n_g < __builtin_inff(); }

struct AdvArgs {
    float* delta; const float* grad; const int64_t* mask; float* norms; float* ws_g; float* ws_u;
    int B, S, H, nslab; float alpha, epsilon;
};

__global__ __launch_bounds__(256) void adv_gnorm_kernel(const AdvArgs a) {
    __shared__ float lds4[4];
    const int b = blockIdx.x / a.nslab, slab = blockIdx.x % a.nslab;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nchunk = a.H >> 3;
    float acc = 0.f;
    for (int r = w; r < ADV_SLAB_ROWS; r += 4) {
        const int t = slab * ADV_SLAB_ROWS + r;
        if (t >= a.S || a.mask[(int64_t)b * a.S + t] == 0) continue;      // (wave-uniform)
        const float* g = a.grad + ((int64_t)b * a.S + t) * a.H;
        for (int c = lane; c < nchunk; c += 64) {
            const f32x4 x = ld4(g + c * 8), y = ld4(g + c * 8 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += x[e] * x[e];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += y[e] * y[e];
        }
    }
    const float s = block_sum4(wave_sum(acc), lds4);
    if (threadIdx.x == 0) a.ws_g[(int64_t)b * a.nslab + slab] = s;
}

__global__ __launch_bounds__(256) void adv_step_kernel(const AdvArgs a) {
    __shared__ float lds4[4];
    const int b = blockIdx.x / a.nslab, slab = blockIdx.x % a.nslab;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nchunk = a.H >> 3;
    const float n_g = sqrtf(sample_sum(a.ws_g + (int64_t)b * a.nslab, a.nslab));
    const bool go = steps(n_g);
    const float sc = go ? a.alpha / n_g : 0.f;
    float acc = 0.f;
    for (int r = w; r < ADV_SLAB_ROWS; r += 4) {
        const int t = slab * ADV_SLAB_ROWS + r;
        if (t >= a.S) continue;
        float* d = a.delta + ((int64_t)b * a.S + t) * a.H;
        if (a.mask[(int64_t)b * a.S + t] == 0) {      // a non-valid position: exact zeros, whatever it held
            for (int c = lane; c < nchunk; c += 64) { st4(d + c * 8, f32x4{0.f, 0.f, 0.f, 0.f}); st4(d + c * 8 + 4, f32x4{0.f, 0.f, 0.f, 0.f}); }
            continue;
        }
        const float* g = a.grad + ((int64_t)b * a.S + t) * a.H;
        for (int c = lane; c < nchunk; c += 64) {
            f32x4 x = ld4(d + c * 8), y = ld4(d + c * 8 + 4);
            if (go) {       // (a sample that does not step never reads g's values into delta: an inf or NaN there stays out)
                const f32x4 gx = ld4(g + c * 8), gy = ld4(g + c * 8 + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { x[e] = x[e] + sc * gx[e]; y[e] = y[e] + sc * gy[e]; }
                st4(d + c * 8, x);
                st4(d + c * 8 + 4, y);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += x[e] * x[e];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += y[e] * y[e];
        }
    }
    const float s = block_sum4(wave_sum(acc), lds4);
    if (threadIdx.x == 0) {
        a.ws_u[(int64_t)b * a.nslab + slab] = s;
        if (slab == 0) a.norms[2 * b] = n_g;
    }
}

__global__ __launch_bounds__(256) void adv_project_kernel(const AdvArgs a) {
    const int b = blockIdx.x / a.nslab, slab = blockIdx.x % a.nslab;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nchunk = a.H >> 3;
    const float n_u = sqrtf(sample_sum(a.ws_u + (int64_t)b * a.nslab, a.nslab));
    const bool shrink = steps(a.norms[2 * b]) && n_u > a.epsilon;       // (norms[b][0]: written by the launch before this one)
    if (threadIdx.x == 0 && slab == 0) a.norms[2 * b + 1] = shrink ? a.epsilon : n_u;
    if (!shrink) return;
    const float sc = a.epsilon / n_u;
    for (int r = w; r < ADV_SLAB_ROWS; r += 4) {
        const int t = slab * ADV_SLAB_ROWS + r;
        if (t >= a.S || a.mask[(int64_t)b * a.S + t] == 0) continue;
        float* d = a.delta + ((int64_t)b * a.S + t) * a.H;
        for (int c = lane; c < nchunk; c += 64) {
            f32x4 x = ld4(d + c * 8), y = ld4(d + c * 8 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { x[e] *= sc; y[e] *= sc; }
            st4(d + c * 8, x);
            st4(d + c * 8 + 4, y);
        }
    }
}

// delta[b, t, h] = r * epsilon / sqrt(n_b * H) at valid positions, 0 elsewhere; one block per token row, the sample's valid
// count n_b summed by each block itself (integers: exact in any order).
__global__ __launch_bounds__(256) void adv_init_uniform_kernel(float* delta, const int64_t* mask, int B, int S, int H, float epsilon,
                                                               uint64_t seed, const uint64_t* counter) {
    __shared__ int cnt[4];
    const int row = blockIdx.x, b = row / S;
    const int64_t* m = mask + (int64_t)b * S;
    int n = 0;
    for (int t = threadIdx.x; t < S; t += 256) n += m[t] != 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = n;
    __syncthreads();
    const int n_b = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    const uint64_t sd = seed + (counter ? counter[0] : 0ull);
    const uint32_t s0 = (uint32_t)sd, s1 = (uint32_t)(sd >> 32);
    const bool valid = mask[row] != 0;
    const float sc = valid ? epsilon / sqrtf((float)n_b * (float)H) : 0.f;
    float* d = delta + (int64_t)row * H;
    const uint32_t base = (uint32_t)row * (uint32_t)H;
    for (int c = threadIdx.x; c < (H >> 2); c += 256) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (valid) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float r = (float)(icka_hash(s0, s1, base + c * 4 + e) >> 8) * 0x1p-23f - 1.f;
                v[e] = r * sc;
            }
        }
        st4(d + c * 4, v);
    }
}

__global__ void adv_bump_kernel(uint64_t* counter) {
    if (threadIdx.x == 0 && blockIdx.x == 0) counter[0] = counter[0] + 1ull;
}

inline bool adv_shape_ok(int B, int S, int H) {
    return B > 0 && S > 0 && S <= ADV_MAX_S && H > 0 && H % 8 == 0 && H <= ADV_MAX_H && (int64_t)B * S * H < (1ll << 32) &&
           (int64_t)B * ((S + ADV_SLAB_ROWS - 1) / ADV_SLAB_ROWS) < (1ll << 31);
}
inline bool adv_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int64_t icka_adv_workspace_floats(int32_t B, int32_t S, int32_t H) {
    if (!adv_shape_ok(B, S, H)) return 0;
    return 2 * (int64_t)B * ((S + ADV_SLAB_ROWS - 1) / ADV_SLAB_ROWS);
}

extern "C" int icka_adv_ascend(float* delta, const float* grad, const int64_t* input_mask, float* norms, int32_t B, int32_t S,
                               int32_t H, float alpha, float epsilon, float* workspace, void* stream) {
    if (!delta || !grad || !input_mask || !norms || !workspace) return ICKA_E_ARG;
    if (!adv_shape_ok(B, S, H)) return ICKA_E_SHAPE;
    if (!adv_al16(delta) || !adv_al16(grad)) return ICKA_E_ALIGN;
    const int nslab = (S + ADV_SLAB_ROWS - 1) / ADV_SLAB_ROWS;
    AdvArgs a{delta, grad, input_mask, norms, workspace, workspace + (int64_t)B * nslab, B, S, H, nslab, alpha, epsilon};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * nslab));
    hipLaunchKernelGGL(adv_gnorm_kernel, grid, dim3(256), 0, st, a);
    ICKA_CHECK_LAUNCH();
    hipLaunchKernelGGL(adv_step_kernel, grid, dim3(256), 0, st, a);
    ICKA_CHECK_LAUNCH();
    hipLaunchKernelGGL(adv_project_kernel, grid, dim3(256), 0, st, a);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_adv_init_uniform(float* delta, const int64_t* input_mask, int32_t B, int32_t S, int32_t H, float epsilon,
                                     uint64_t seed, const uint64_t* counter_dev, void* stream) {
    if (!delta || !input_mask) return ICKA_E_ARG;
    if (!adv_shape_ok(B, S, H)) return ICKA_E_SHAPE;
    if (!adv_al16(delta)) return ICKA_E_ALIGN;
    hipLaunchKernelGGL(adv_init_uniform_kernel, dim3((unsigned)(B * S)), dim3(256), 0, (hipStream_t)stream, delta, input_mask, B, S, H,
                       epsilon, seed, counter_dev);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_adv_bump(uint64_t* counter_dev, void* stream) {
    if (!counter_dev) return ICKA_E_ARG;
    hipLaunchKernelGGL(adv_bump_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counter_dev);
    ICKA_CHECK_LAUNCH();
    return 0;
}
