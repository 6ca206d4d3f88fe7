// The reference's parameter update after backward (My_cross_attention.py:831-844): clip_grad_norm_(model.parameters(), 1.0),
// AdamW.step() with the two weight-decay groups of :743-751, scheduler.step(), zero_grad.  Outside the fwd+bwd metric
//  but reported beside it; as ~220 per-tensor launches of the stock optimizer it costs 2.9 ms on a
// 4.5 ms step.  Parameters, gradients and optimizer state live in flat buffers of ONE layout (ParamArena), so the whole
// update is three launches over chunk tables:
//   icka_optim_sqnorm   per-chunk sums of squares of the gradients                      (reads 4 B per gradient)
//   icka_optim_clip     fixed-order sum of the partials -> total norm and the clip coefficient, on the device (no host sync)
//   icka_optim_adamw    p, m, v <- AdamW(p, g * coef, m, v) for one weight-decay group, and in the same pass the 16-bit
//                       weight shadows the next forward's GEMMs read (bf16, and fp16 in the "mixed16" mode): the separate
//                       per-forward re-cast of the arena (98 us at bert-base) has nothing left to do
// Arithmetic = torch.optim.AdamW (decoupled decay first, bias-corrected moments, eps added to sqrt(v_hat)); all f32.
// The capturable form of the same update keeps the step count, the learning-rate schedule and the bias corrections in a
// device block (icka_optim_state), so that it can sit inside a captured training step:
//   icka_optim_prepare    (in place of icka_optim_clip) norm, non-finite test, clip coefficient, this update's lr / bias
//                         corrections per group, t += 1 -- or, for a non-finite norm, the skip word
//   icka_optim_adamw_dev  all groups in one launch, values from the block; returns at once when the skip word is set
// An averaged copy of the weights (EMA / SWA; outside the reference, off by default) is one more f32 buffer of the same layout:
//   icka_optim_average          avg <- avg + (1 - d) (p - avg) over a chunk table of every parameter  (12 B per parameter)
//   icka_optim_average_prepare  (capturable form) one thread behind icka_optim_prepare: is this update averaged, its decay,
//                               n += 1, in a second device block (icka_average_state); icka_optim_average_dev reads it
//   icka_optim_swap             p <-> avg in place, with the 16-bit shadows of the new p: evaluating the averaged weights keeps
//                               every address a captured graph holds
#include "common.h"

namespace {

constexpr int OPT_CHUNK = 8192;

// table[2 b] = first element, table[2 b + 1] = count (multiple of 8, <= OPT_CHUNK)
__global__ __launch_bounds__(256) void optim_sqnorm_kernel(const float* __restrict__ g, const int64_t* __restrict__ table,
                                                           float* __restrict__ partials) {
    __shared__ float red[4];
    const int64_t lo = table[2 * blockIdx.x], len = table[2 * blockIdx.x + 1];
    float s = 0.f;
    for (int64_t c = threadIdx.x * 4; c < len; c += 256 * 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(g + lo + c);
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[0] = total gradient norm, out[1] = clip coefficient min(1, max_norm / (norm + 1e-6)) (clip_grad_norm_'s formula);
// one block, fixed summation order: bitwise repeatable
__global__ __launch_bounds__(1024) void optim_clip_kernel(const float* __restrict__ partials, int n, float max_norm,
                                                          float* __restrict__ out) {
    __shared__ double red[16];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) s += (double)partials[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 16; ++i) t += red[i];
        const float norm = (float)sqrt(t);
        out[0] = norm;
        const float c = max_norm / (norm + 1e-6f);
        out[1] = max_norm > 0.f ? (c < 1.f ? c : 1.f) : 1.f;
    }
}

struct AdamArgs {
    float* p; const float* g; float* m; float* v;
    bf16_t* shadow; _Float16* shadow16;      // may be NULL
    const int64_t* table;
    const float* coef;                       // device scalar (out[1] of the clip kernel) or NULL
    float lr, beta1, beta2, eps, wd, bc1, bc2_sqrt;   // bc1 = 1 - beta1^t, bc2_sqrt = sqrt(1 - beta2^t)
};

__global__ __launch_bounds__(256) void optim_adamw_kernel(const AdamArgs a) {
    const int64_t lo = a.table[2 * blockIdx.x], len = a.table[2 * blockIdx.x + 1];
    const float coef = a.coef ? a.coef[0] : 1.f;
    const float step = a.lr / a.bc1, decay = 1.f - a.lr * a.wd;
    for (int64_t c = threadIdx.x * 8; c < len; c += 256 * 8) {
        const int64_t i = lo + c;
        float p[8], g[8], m[8], v[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(a.p + i + 4 * h), gv = *reinterpret_cast<const f32x4*>(a.g + i + 4 * h);
            const f32x4 mv = *reinterpret_cast<const f32x4*>(a.m + i + 4 * h), vv = *reinterpret_cast<const f32x4*>(a.v + i + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) { p[4 * h + e] = pv[e]; g[4 * h + e] = gv[e] * coef; m[4 * h + e] = mv[e]; v[4 * h + e] = vv[e]; }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            p[e] *= decay;                                               // decoupled weight decay (torch.optim.AdamW)
            m[e] = a.beta1 * m[e] + (1.f - a.beta1) * g[e];              // exp_avg.lerp_(grad, 1 - beta1)
            v[e] = a.beta2 * v[e] + (1.f - a.beta2) * g[e] * g[e];
            const float denom = sqrtf(v[e]) / a.bc2_sqrt + a.eps;
            p[e] -= step * (m[e] / denom);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<f32x4*>(a.p + i + 4 * h) = f32x4{p[4 * h], p[4 * h + 1], p[4 * h + 2], p[4 * h + 3]};
            *reinterpret_cast<f32x4*>(a.m + i + 4 * h) = f32x4{m[4 * h], m[4 * h + 1], m[4 * h + 2], m[4 * h + 3]};
            *reinterpret_cast<f32x4*>(a.v + i + 4 * h) = f32x4{v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]};
        }
        if (a.shadow) {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f2bf(p[e]);
            *reinterpret_cast<u32x4*>(a.shadow + i) = as_u32x4(o);
        }
        if (a.shadow16) {
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (_Float16)fminf(fmaxf(p[e], -65504.f), 65504.f);
            *reinterpret_cast<f16x8*>(a.shadow16 + i) = o;
        }
    }
}

// ---- device-held schedule (icka_optim_state, include/icka_hip.h): the update as graph nodes, no per-step host value
using OptState = icka_optim_state;

__device__ __forceinline__ bool finite_f64(double x) {
    return ((unsigned long long)__double_as_longlong(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// One block, after optim_sqnorm_kernel: the sum of optim_clip_kernel (same order: bitwise the same norm), the non-finite
// test, and -- for an update that is applied -- the clip coefficient, the per-group rate and bias corrections of update
// number t + 1, and t itself.  Thread 0 writes the block with ordinary stores; the update kernel of the same stream reads it.
__global__ __launch_bounds__(1024) void optim_prepare_kernel(const float* __restrict__ partials, int n, float max_norm, int flags,
                                                             OptState* __restrict__ st) {
    __shared__ double red[16];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) s += (double)partials[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int i = 0; i < 16; ++i) sum += red[i];
    if (flags & ICKA_OPTIM_DRY) {            // warm-up launches: nothing is applied, nothing is counted
        st->skip = 1;
        return;
    }
    const float norm = (float)sqrt(sum);
    st->norm = norm;
    if (!(flags & ICKA_OPTIM_NO_GUARD) && !finite_f64(sum)) {
        st->skip = 1;
        st->skipped += 1;
        return;
    }
    const float c = max_norm / (norm + 1e-6f);
    st->coef = max_norm > 0.f ? (c < 1.f ? c : 1.f) : 1.f;
    const int64_t t = st->t, warm = st->warmup, total = st->total;
    double factor = 1.0;
    if (st->kind == ICKA_OPTIM_SCHEDULE_LINEAR) {
        if (t < warm) {
            factor = (double)t / (double)(warm > 1 ? warm : 1);
        } else {
            const int64_t span = total - warm;
            factor = (double)(total - t) / (double)(span > 1 ? span : 1);
            factor = factor > 0.0 ? factor : 0.0;
        }
    }
    const int ng = st->n_groups < ICKA_OPTIM_MAX_GROUPS ? st->n_groups : ICKA_OPTIM_MAX_GROUPS;
    for (int g = 0; g < ng; ++g) {
        st->lr[g] = (float)(st->base_lr[g] * factor);
        st->bc1[g] = (float)(1.0 - pow((double)st->beta1[g], (double)(t + 1)));
        st->bc2_sqrt[g] = (float)sqrt(1.0 - pow((double)st->beta2[g], (double)(t + 1)));
    }
    st->t = t + 1;
    st->skip = 0;
}

struct AdamDevArgs {
    float* p; const float* g; float* m; float* v;
    bf16_t* shadow; _Float16* shadow16;      // may be NULL
    const int64_t* table;                    // table[3 b] = first element, [3 b + 1] = count, [3 b + 2] = group
    const OptState* st;
};

// optim_adamw_kernel's arithmetic for the chunks of ALL groups, the group's values read from the state block the prepare
// launch in front of it wrote; a refused update (skip) touches no memory
__global__ __launch_bounds__(256) void optim_adamw_dev_kernel(const AdamDevArgs a) {
    if (a.st->skip) return;
    const int64_t lo = a.table[3 * blockIdx.x], len = a.table[3 * blockIdx.x + 1];
    const int grp = (int)a.table[3 * blockIdx.x + 2] & (ICKA_OPTIM_MAX_GROUPS - 1);   // (never past the block)
    const float coef = a.st->coef;
    const float lr = a.st->lr[grp], beta1 = a.st->beta1[grp], beta2 = a.st->beta2[grp], eps = a.st->eps[grp];
    const float wd = a.st->weight_decay[grp], bc1 = a.st->bc1[grp], bc2_sqrt = a.st->bc2_sqrt[grp];
    const float step = lr / bc1, decay = 1.f - lr * wd;
    for (int64_t c = threadIdx.x * 8; c < len; c += 256 * 8) {
        const int64_t i = lo + c;
        float p[8], g[8], m[8], v[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(a.p + i + 4 * h), gv = *reinterpret_cast<const f32x4*>(a.g + i + 4 * h);
            const f32x4 mv = *reinterpret_cast<const f32x4*>(a.m + i + 4 * h), vv = *reinterpret_cast<const f32x4*>(a.v + i + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) { p[4 * h + e] = pv[e]; g[4 * h + e] = gv[e] * coef; m[4 * h + e] = mv[e]; v[4 * h + e] = vv[e]; }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            p[e] *= decay;
            m[e] = beta1 * m[e] + (1.f - beta1) * g[e];
            v[e] = beta2 * v[e] + (1.f - beta2) * g[e] * g[e];
            const float denom = sqrtf(v[e]) / bc2_sqrt + eps;
            p[e] -= step * (m[e] / denom);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<f32x4*>(a.p + i + 4 * h) = f32x4{p[4 * h], p[4 * h + 1], p[4 * h + 2], p[4 * h + 3]};
            *reinterpret_cast<f32x4*>(a.m + i + 4 * h) = f32x4{m[4 * h], m[4 * h + 1], m[4 * h + 2], m[4 * h + 3]};
            *reinterpret_cast<f32x4*>(a.v + i + 4 * h) = f32x4{v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]};
        }
        if (a.shadow) {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f2bf(p[e]);
            *reinterpret_cast<u32x4*>(a.shadow + i) = as_u32x4(o);
        }
        if (a.shadow16) {
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (_Float16)fminf(fmaxf(p[e], -65504.f), 65504.f);
            *reinterpret_cast<f16x8*>(a.shadow16 + i) = o;
        }
    }
}

// ---- averaged weights (icka_average_state, include/icka_hip.h): an EMA / SWA copy of the parameters kept beside the update
using AvgState = icka_average_state;

// One thread, behind optim_prepare_kernel: whether the update that prepare just admitted (number st->t) is averaged, and with
// which decay.  A refused or dry update (skip) is never averaged and never counted.
__global__ void optim_average_prepare_kernel(AvgState* __restrict__ av, const OptState* __restrict__ st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st->skip) {
        av->apply = 0;
        return;
    }
    const int64_t t = st->t, start = av->start, every = av->every > 0 ? av->every : 1;
    if (!(t > start && (t - start - 1) % every == 0)) {
        av->apply = 0;
        return;
    }
    const int64_t n = av->n;
    double d;
    if (n == 0) {
        d = 0.0;
    } else if (av->kind == ICKA_AVERAGE_SWA) {
        d = (double)n / (double)(n + 1);
    } else {
        d = av->decay;
        if (av->warmup) {
            const double w = (double)(1 + n) / (double)(10 + n);
            d = w < d ? w : d;
        }
    }
    av->decay_now = (float)d;
    av->n = n + 1;
    av->apply = 1;
}

// avg <- avg + (1 - decay) * (p - avg) over the chunks of the table (pairs, as optim_adamw_kernel's).  av != NULL: the decay
// and the apply word come from the block the prepare launch in front wrote (one compilation serves both forms: they agree
// bit for bit).  decay == 0 stores p itself: avg + (p - avg) is not p in floating point.
__global__ __launch_bounds__(256) void optim_average_kernel(const float* __restrict__ p, float* __restrict__ avg,
                                                            const int64_t* __restrict__ table, const AvgState* __restrict__ av,
                                                            float decay) {
    if (av) {
        if (!av->apply) return;
        decay = av->decay_now;
    }
    const int64_t lo = table[2 * blockIdx.x], len = table[2 * blockIdx.x + 1];
    const float w = 1.f - decay;
    const bool copy = decay == 0.f;
    for (int64_t c = threadIdx.x * 8; c < len; c += 256 * 8) {
        const int64_t i = lo + c;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i + 4 * h);
            f32x4 o = pv;
            if (!copy) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(avg + i + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = a[e] + w * (pv[e] - a[e]);
            }
            *reinterpret_cast<f32x4*>(avg + i + 4 * h) = o;
        }
    }
}

// p <-> avg over the chunks of the table, and the 16-bit shadows of the new p as optim_adamw_kernel stores them
__global__ __launch_bounds__(256) void optim_swap_kernel(float* __restrict__ p, float* __restrict__ avg, bf16_t* __restrict__ shadow,
                                                         _Float16* __restrict__ shadow16, const int64_t* __restrict__ table) {
    const int64_t lo = table[2 * blockIdx.x], len = table[2 * blockIdx.x + 1];
    for (int64_t c = threadIdx.x * 8; c < len; c += 256 * 8) {
        const int64_t i = lo + c;
        float np[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i + 4 * h);
            const f32x4 a = *reinterpret_cast<const f32x4*>(avg + i + 4 * h);
            *reinterpret_cast<f32x4*>(p + i + 4 * h) = a;
            *reinterpret_cast<f32x4*>(avg + i + 4 * h) = pv;
#pragma unroll
            for (int e = 0; e < 4; ++e) np[4 * h + e] = a[e];
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

extern "C" int64_t icka_optim_chunk_elems(void) { return OPT_CHUNK; }

extern "C" int icka_optim_sqnorm(const float* grads, const int64_t* table_dev, int32_t n_chunks, float* partials, void* stream) {
    if (!grads || !table_dev || !partials) return ICKA_E_ARG;
    if (n_chunks <= 0) return ICKA_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(grads) & 15) return ICKA_E_ALIGN;
    hipLaunchKernelGGL(optim_sqnorm_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, grads, table_dev, partials);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_optim_clip(const float* partials, int32_t n, float max_norm, float* out2, void* stream) {
    if (!partials || !out2) return ICKA_E_ARG;
    if (n <= 0) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(optim_clip_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, partials, n, max_norm, out2);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_optim_adamw(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                void* shadow_f16, const int64_t* table_dev, int32_t n_chunks, const float* clip_coef, float lr,
                                float beta1, float beta2, float eps, float weight_decay, int32_t step, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !table_dev) return ICKA_E_ARG;
    if (n_chunks <= 0 || step <= 0) return ICKA_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(exp_avg) |
         reinterpret_cast<uintptr_t>(exp_avg_sq) | reinterpret_cast<uintptr_t>(shadow_bf16) | reinterpret_cast<uintptr_t>(shadow_f16)) & 15)
        return ICKA_E_ALIGN;
    AdamArgs a;
    a.p = params; a.g = grads; a.m = exp_avg; a.v = exp_avg_sq; a.shadow = (bf16_t*)shadow_bf16; a.shadow16 = (_Float16*)shadow_f16;
    a.table = table_dev; a.coef = clip_coef; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay;
    a.bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    a.bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    hipLaunchKernelGGL(optim_adamw_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, a);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_optim_prepare(const float* partials, int32_t n, float max_norm, int32_t flags, void* state, void* stream) {
    if (!state || (n > 0 && !partials)) return ICKA_E_ARG;
    if (n < 0 || (flags & ~(ICKA_OPTIM_DRY | ICKA_OPTIM_NO_GUARD))) return ICKA_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(state) & 7) return ICKA_E_ALIGN;
    hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, partials, n, max_norm, flags,
                       (OptState*)state);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_optim_adamw_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                    void* shadow_f16, const int64_t* table3_dev, int32_t n_chunks, const void* state, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !table3_dev || !state) return ICKA_E_ARG;
    if (n_chunks <= 0) return ICKA_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(exp_avg) |
         reinterpret_cast<uintptr_t>(exp_avg_sq) | reinterpret_cast<uintptr_t>(shadow_bf16) | reinterpret_cast<uintptr_t>(shadow_f16)) & 15)
        return ICKA_E_ALIGN;
    if (reinterpret_cast<uintptr_t>(state) & 7) return ICKA_E_ALIGN;
    AdamDevArgs a;
    a.p = params; a.g = grads; a.m = exp_avg; a.v = exp_avg_sq; a.shadow = (bf16_t*)shadow_bf16; a.shadow16 = (_Float16*)shadow_f16;
    a.table = table3_dev; a.st = (const OptState*)state;
    hipLaunchKernelGGL(optim_adamw_dev_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, a);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_optim_average(const float* params, float* avg, const int64_t* table_dev, int32_t n_chunks, float decay,
                                  void* stream) {
    if (!params || !avg || !table_dev || params == avg) return ICKA_E_ARG;
    if (n_chunks <= 0 || !(decay >= 0.f && decay < 1.f)) return ICKA_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(avg)) & 15) return ICKA_E_ALIGN;
    hipLaunchKernelGGL(optim_average_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, params, avg, table_dev,
                       (const AvgState*)nullptr, decay);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_optim_average_prepare(void* average_state, const void* optim_state, void* stream) {
    if (!average_state || !optim_state) return ICKA_E_ARG;
    if ((reinterpret_cast<uintptr_t>(average_state) | reinterpret_cast<uintptr_t>(optim_state)) & 7) return ICKA_E_ALIGN;
    hipLaunchKernelGGL(optim_average_prepare_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (AvgState*)average_state,
                       (const OptState*)optim_state);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_optim_average_dev(const float* params, float* avg, const int64_t* table_dev, int32_t n_chunks,
                                      const void* average_state, void* stream) {
    if (!params || !avg || !table_dev || !average_state || params == avg) return ICKA_E_ARG;
    if (n_chunks <= 0) return ICKA_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(avg)) & 15) return ICKA_E_ALIGN;
    if (reinterpret_cast<uintptr_t>(average_state) & 7) return ICKA_E_ALIGN;
    hipLaunchKernelGGL(optim_average_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, params, avg, table_dev,
                       (const AvgState*)average_state, 0.f);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_optim_swap(float* params, float* avg, void* shadow_bf16, void* shadow_f16, const int64_t* table_dev,
                               int32_t n_chunks, void* stream) {
    if (!params || !avg || !table_dev || params == avg) return ICKA_E_ARG;
    if (n_chunks <= 0) return ICKA_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(avg) | reinterpret_cast<uintptr_t>(shadow_bf16) |
         reinterpret_cast<uintptr_t>(shadow_f16)) & 15)
        return ICKA_E_ALIGN;
    hipLaunchKernelGGL(optim_swap_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, params, avg, (bf16_t*)shadow_bf16,
                       (_Float16*)shadow_f16, table_dev);
    ICKA_CHECK_LAUNCH();
    return 0;
}
