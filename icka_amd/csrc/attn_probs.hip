// Attention maps (icka_attn_probs): the probabilities the fused attention kernels never materialise,
//     P = softmax(scale * Q.K^T + additive mask)          -- BEFORE dropout (BertSelfAttention.forward :492-497, BertCoAttention :606-611)
// from the bf16 Q / K the forward already wrote.  A diagnostic output: f32, [B,heads,Sq,Skv] or the mean over heads [B,Sq,Skv].
// Score stage = attn_core.h's whole-head forward: one block owns 64 queries (4 waves x 16), K goes through LDS once per block (and
// head) in chunks of up to 256 keys, S^T = K.Q^T on v_mfma_f32_16x16x32_bf16 puts the query on the lane (l & 15) and keys
// 16 kt + 4 (l >> 4) .. + 3 in the accumulator, so all 16 x Skv scores of a wave stay in registers (KT x 4 floats a lane, KT <= 32
// for BERT's 512 positions) and the row max / sum are in-lane plus two cross-lane steps.  Softmax in f32 with the forward's exp.
// Keys past Skv carry -inf (exactly 0 after exp, never stored); the mask itself is the reference's finite -10000, so a sample whose
// keys are all masked gets the softmax of its unmasked scores as the reference does (here without the reference's f32 rounding of
// score - 10000: the sample's largest mask value is subtracted from the mask first).
// Head-mean form: the block of a (sample, query tile) walks the heads 0 .. heads-1 and adds each head's probabilities to a register
// accumulator: one launch, no atomics, the same bits on every run.
#include "attn_core.h"

namespace {

struct ProbsArgs {
    const bf16_t* Q; int64_t ldq; const bf16_t* K; int64_t ldk; const float* mask; float* P;
    int B, h, Sq, Skv; float scale; int vec;   // vec: rows of P are whole 16-byte groups (Skv % 4 == 0 and P 16-byte aligned)
};

// rows [0, ROWS) of a token-major matrix (one head's 64 columns) -> off_t image; rows >= nrows (nrows >= 1) re-read the last
// valid row and are zeroed by a select: no address past the matrix, no divergent branch
template <int ROWS>
__device__ __forceinline__ void probs_stage(char* lds, const bf16_t* base, int64_t ld, int nrows, int tid) {
#pragma unroll
    for (int i = 0; i < ROWS * 8 / 256; ++i) {
        const int q = tid + 256 * i, r = q >> 3, c = q & 7;
        const int rr = r < nrows ? r : nrows - 1;
        const u32x4 v = *reinterpret_cast<const u32x4*>(base + (int64_t)rr * ld + c * 8);
        const uint32_t keep = r < nrows ? 0xffffffffu : 0u;
        *reinterpret_cast<u32x4*>(lds + off_t(r, c)) = v & keep;
    }
}

// this lane's 4 values of key tile kt -> row `prow` of P (keys past Skv are not written)
__device__ __forceinline__ void probs_store(float* prow, const f32x4& v, int kt, int g, int Skv, int vec) {
    const int key0 = 16 * kt + 4 * g;
    if (vec) {
        if (key0 < Skv) *reinterpret_cast<f32x4*>(prow + key0) = v;   // Skv % 4 == 0: key0 + 3 < Skv
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (key0 + r < Skv) prow[key0 + r] = v[r];
    }
}

// KT = 16-key tiles held per query (16 KT >= Skv; the launcher picks the smallest instance, so that every staged chunk of KC
// tiles starts below Skv).  MEAN: grid.x = B and the block walks the heads; else grid.x = B * heads.  grid.y = 64-query tiles.
template <int KT, bool MEAN>
__global__ __launch_bounds__(256) void attn_probs_kernel(const ProbsArgs a) {
    constexpr int KC = KT < 16 ? KT : 16, NCH = KT / KC;
    static_assert(KT % KC == 0, "whole chunks");
    __shared__ __attribute__((aligned(16))) char smem[(64 + 16 * KC) * 128 + 16 * KT * 4];
    char* sQ = smem; char* sK = smem + 64 * 128;
    float* s_mask = reinterpret_cast<float*>(sK + 16 * KC * 128);   // additive mask of the sample's keys; -inf past Skv
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i15 = lane & 15;
    const int b = MEAN ? blockIdx.x : blockIdx.x / a.h;
    const int head0 = MEAN ? 0 : blockIdx.x % a.h, nh = MEAN ? a.h : 1;
    const int q0 = blockIdx.y * 64, q = q0 + 16 * wave + i15;
    const bool live = q0 + 16 * wave < a.Sq;   // wave-uniform: a wave wholly past Sq only stages and waits at the barriers
    const float* mb = a.mask + (int64_t)b * a.Skv;
    // The mask goes to LDS (it is the same for every head: held in registers across the head loop it costs KT x 4 of them next
    // to the scores and the head-mean accumulator) with the sample's LARGEST mask value taken off -- softmax does not see a
    // shift of the whole row, but f32 does: -10000 added to a score of unit order leaves it on a 2^-10 grid, and a sample whose
    // keys are all masked would get its "softmax of the unmasked scores" from scores rounded to 1e-3 (1.2e-4 in P).
    __shared__ float s_red[4];
    float mtop = -INFINITY;
    for (int key = tid; key < a.Skv; key += 256) mtop = fmaxf(mtop, mb[key]);
    mtop = wave_max(mtop);
    if (lane == 0) s_red[wave] = mtop;
    __syncthreads();
    mtop = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    mtop = fminf(fmaxf(mtop, -3.0e38f), 3.0e38f);   // (a row of infinities must not turn into NaN by the subtraction itself)
    for (int key = tid; key < 16 * KT; key += 256) s_mask[key] = key < a.Skv ? mb[key] - mtop : -INFINITY;

    f32x4 macc[MEAN ? KT : 1];
    if constexpr (MEAN) {
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) macc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int hh = 0; hh < nh; ++hh) {
        const int head = head0 + hh;
        if (hh) __syncthreads();   // every wave is done with the previous head's tiles
        probs_stage<64>(sQ, a.Q + ((int64_t)b * a.Sq + q0) * a.ldq + head * HD, a.ldq, a.Sq - q0, tid);
        f32x4 s[KT];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (c) __syncthreads();   // ... with the previous chunk of keys
            probs_stage<16 * KC>(sK, a.K + ((int64_t)b * a.Skv + 16 * KC * c) * a.ldk + head * HD, a.ldk, a.Skv - 16 * KC * c, tid);
            __syncthreads();
            if (live) {
                const bf16x8 qf0 = frag_row(sQ, 16 * wave, 0, lane), qf1 = frag_row(sQ, 16 * wave, 1, lane);
#pragma unroll
                for (int kc = 0; kc < KC; ++kc) {
                    const int kt = KC * c + kc;
                    const f32x4 mk = *reinterpret_cast<const f32x4*>(s_mask + 16 * kt + 4 * g);
                    f32x4 t = mfma16(frag_row(sK, 16 * kc, 0, lane), qf0, f32x4{0.f, 0.f, 0.f, 0.f});
                    t = mfma16(frag_row(sK, 16 * kc, 1, lane), qf1, t);
#pragma unroll
                    for (int r = 0; r < 4; ++r) t[r] = t[r] * a.scale + mk[r];
                    s[kt] = t;
                }
            }
        }
        if (!live) continue;
        float mx = -INFINITY;   // (finite after the loop: key 0 exists and the mask is finite)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float psum = 0.f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = __expf(s[kt][r] - mx);
                psum += pv;
                s[kt][r] = pv;
            }
        psum += __shfl_xor(psum, 16, 64);
        psum += __shfl_xor(psum, 32, 64);
        const float inv = 1.f / psum;
        if constexpr (MEAN) {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) macc[kt] += s[kt] * inv;
        } else if (q < a.Sq) {
            float* prow = a.P + (((int64_t)b * a.h + head) * a.Sq + q) * a.Skv;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) probs_store(prow, s[kt] * inv, kt, g, a.Skv, a.vec);
        }
    }
    if constexpr (MEAN) {
        if (live && q < a.Sq) {
            const float hinv = 1.f / (float)a.h;
            float* prow = a.P + ((int64_t)b * a.Sq + q) * a.Skv;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) probs_store(prow, macc[kt] * hinv, kt, g, a.Skv, a.vec);
        }
    }
}

template <int KT>
void launch_probs(const ProbsArgs& a, bool mean, hipStream_t st) {
    const dim3 grid(mean ? a.B : a.B * a.h, (a.Sq + 63) / 64);
    if (mean) hipLaunchKernelGGL((attn_probs_kernel<KT, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((attn_probs_kernel<KT, false>), grid, dim3(256), 0, st, a);
}

}  // namespace

extern "C" int icka_attn_probs(const void* Q, int64_t ldq, const void* K, int64_t ldk, const float* add_mask, float* P,
                               int32_t B, int32_t heads, int32_t Sq, int32_t Skv, float scale, int32_t flags, void* stream) {
    if (!Q || !K || !add_mask || !P) return ICKA_E_ARG;
    if (flags & ~ICKA_ATTN_PROBS_HEAD_MEAN) return ICKA_E_ARG;
    if (B <= 0 || heads <= 0 || Sq <= 0 || Skv <= 0 || Skv > 512) return ICKA_E_SHAPE;
    if ((int64_t)B * heads >= (1ll << 31) || (Sq + 63) / 64 > 65535) return ICKA_E_SHAPE;   // grid limits
    const auto ok16 = [](const void* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 8 == 0; };
    if (!ok16(Q, ldq) || !ok16(K, ldk) || (reinterpret_cast<uintptr_t>(P) & 3)) return ICKA_E_ALIGN;
    ProbsArgs a{};
    a.Q = (const bf16_t*)Q; a.ldq = ldq; a.K = (const bf16_t*)K; a.ldk = ldk; a.mask = add_mask; a.P = P;
    a.B = B; a.h = heads; a.Sq = Sq; a.Skv = Skv; a.scale = scale;
    a.vec = (Skv % 4 == 0 && (reinterpret_cast<uintptr_t>(P) & 15) == 0) ? 1 : 0;
    const bool mean = (flags & ICKA_ATTN_PROBS_HEAD_MEAN) != 0;
    hipStream_t st = (hipStream_t)stream;
    if (Skv > 256) launch_probs<32>(a, mean, st);
    else if (Skv > 128) launch_probs<16>(a, mean, st);
    else if (Skv > 64) launch_probs<8>(a, mean, st);
    else launch_probs<4>(a, mean, st);
    ICKA_CHECK_LAUNCH();
    return 0;
}
