// Padding-free ("packed") batches of the MNER tagger: the valid tokens of B samples live in a fixed number of rows
// (max_tokens), sample b in rows [cu[b], cu[b+1]).  This file holds the pack plan (one launch that turns input_mask into the
// row maps) and the row gather that moves activations, logits and their gradients between the padded [B*S] and the packed
// [max_tokens] layouts.  The varlen attention kernels are the VL instances of the whole-head kernels in attention.hip.
#include "common.h"

namespace {

constexpr int PLAN_THREADS = 1024;
constexpr int PLAN_MAX_B = 2048;

// One block.  Phase 1: the prefix length of every sample (and whether its mask is a prefix mask at all).  Phase 2: the packed
// offsets; samples from the first one that would end past max_tokens are dropped (length 0 in cu).  Phase 3: both row maps.
__global__ __launch_bounds__(PLAN_THREADS) void pack_plan_kernel(const int64_t* __restrict__ mask, int B, int S,
                                                                 int max_tokens, int32_t* __restrict__ lens,
                                                                 int32_t* __restrict__ cu, int32_t* __restrict__ p2p,
                                                                 int32_t* __restrict__ pad2pack, int32_t* __restrict__ cls_of,
                                                                 int32_t* __restrict__ status, uint32_t* err) {
    __shared__ int s_len[PLAN_MAX_B];
    __shared__ int s_cu[PLAN_MAX_B + 1];
    __shared__ int s_nonprefix;
    const int tid = threadIdx.x;
    if (tid == 0) s_nonprefix = 0;
    __syncthreads();
    for (int b = tid; b < B; b += PLAN_THREADS) {
        const int64_t* m = mask + (int64_t)b * S;
        int first_zero = S, count = 0;
        for (int s = 0; s < S; ++s) {
            const bool v = m[s] != 0;
            count += v ? 1 : 0;
            if (!v && first_zero == S) first_zero = s;
        }
        s_len[b] = first_zero;
        lens[b] = first_zero;
        if (count != first_zero) s_nonprefix = 1;
    }
    __syncthreads();
    if (tid == 0) {
        int kept = 0, total = 0;
        bool dropping = false;
        for (int b = 0; b < B; ++b) {
            const int len = s_len[b];
            total += len;
            s_cu[b] = kept;
            if (!dropping && kept + len <= max_tokens) kept += len;
            else dropping = true;
        }
        s_cu[B] = kept;
        const int flags = (total > max_tokens ? 1 : 0) | (s_nonprefix ? 2 : 0);
        if (status) { status[0] = total; status[1] = flags; }
        if (err && flags) {   // host-mapped error word: [0] = token count, [1] = flags (1 overflow, 2 not a prefix mask)
            __hip_atomic_store(err, (uint32_t)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(err + 1, (uint32_t)flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    __syncthreads();
    for (int b = tid; b <= B; b += PLAN_THREADS) cu[b] = s_cu[b];
    const int n = B * S;
    for (int i = tid; i < n; i += PLAN_THREADS) {
        const int b = i / S, s = i - b * S;
        const int c0 = s_cu[b], plen = s_cu[b + 1] - c0;
        if (s < plen) {
            const int t = c0 + s;
            pad2pack[i] = t;
            p2p[t] = i;
            cls_of[t] = s == 0 ? b : -1;
        } else {
            pad2pack[i] = mask[i] != 0 ? -2 : -1;   // -2: a valid token that is not packed (dropped / not a prefix mask)
        }
    }
    for (int t = s_cu[B] + tid; t < max_tokens; t += PLAN_THREADS) {   // filler rows
        p2p[t] = -1;
        cls_of[t] = -1;
    }
}

// dst row r = src row map[r * map_stride]; map < 0 -> zeros (-2: the fill word instead); a map entry >= src_rows (a corrupt map)
// is read as -1.  VEC: 16-byte chunks.
template <bool VEC>
__global__ __launch_bounds__(256) void rows_gather_kernel(const uint32_t* __restrict__ src, int64_t ld_src,
                                                          uint32_t* __restrict__ dst, int64_t ld_dst, int row_words,
                                                          const int32_t* __restrict__ map, int64_t map_stride,
                                                          int64_t dst_rows, int64_t src_rows, uint32_t fill) {
    constexpr int W = VEC ? 4 : 1;
    const int cpr = row_words / W;
    const int64_t n = dst_rows * cpr;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cpr;
        const int c = (int)(i - r * cpr);
        int64_t m = map[r * map_stride];
        if (m >= src_rows) m = -1;
        if constexpr (VEC) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (m >= 0) v = *reinterpret_cast<const u32x4*>(src + m * ld_src + 4 * c);
            else if (m == -2) v = u32x4{fill, fill, fill, fill};
            *reinterpret_cast<u32x4*>(dst + r * ld_dst + 4 * c) = v;
        } else {
            uint32_t v = 0u;
            if (m >= 0) v = src[m * ld_src + c];
            else if (m == -2) v = fill;
            dst[r * ld_dst + c] = v;
        }
    }
}

}  // namespace

extern "C" int icka_pack_plan(const int64_t* mask, int32_t B, int32_t S, int32_t max_tokens, int32_t* lens, int32_t* cu_seqlens,
                              int32_t* packed_to_padded, int32_t* padded_to_packed, int32_t* cls_of, int32_t* status,
                              void* err_word, void* stream) {
    if (!mask || !lens || !cu_seqlens || !packed_to_padded || !padded_to_packed || !cls_of) return ICKA_E_ARG;
    if (B <= 0 || B > PLAN_MAX_B || S <= 0 || S > 1024 || max_tokens <= 0) return ICKA_E_SHAPE;
    hipLaunchKernelGGL(pack_plan_kernel, dim3(1), dim3(PLAN_THREADS), 0, (hipStream_t)stream, mask, B, S, max_tokens, lens,
                       cu_seqlens, packed_to_padded, padded_to_packed, cls_of, status, (uint32_t*)err_word);
    ICKA_CHECK_LAUNCH();
    return 0;
}

extern "C" int icka_rows_gather(const void* src, int64_t ld_src, int64_t src_rows, void* dst, int64_t ld_dst, int64_t dst_rows,
                                int32_t row_words, const int32_t* map, int64_t map_stride, uint32_t fill, void* stream) {
    if (!src || !dst || !map) return ICKA_E_ARG;
    if (row_words <= 0 || dst_rows < 0 || src_rows < 0 || ld_src < row_words || ld_dst < row_words || map_stride <= 0)
        return ICKA_E_SHAPE;
    if (dst_rows == 0) return 0;
    const bool vec = row_words % 4 == 0 && ld_src % 4 == 0 && ld_dst % 4 == 0 &&
                     (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const int64_t n = dst_rows * (vec ? row_words / 4 : row_words);
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (vec)
        hipLaunchKernelGGL(rows_gather_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                           (const uint32_t*)src, ld_src, (uint32_t*)dst, ld_dst, row_words, map, map_stride, dst_rows, src_rows, fill);
    else
        hipLaunchKernelGGL(rows_gather_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                           (const uint32_t*)src, ld_src, (uint32_t*)dst, ld_dst, row_words, map, map_stride, dst_rows, src_rows, fill);
    ICKA_CHECK_LAUNCH();
    return 0;
}
