// What the LSTM recurrence kernels of lstm.hip share, ONE definition each: the argument block, the hand-off primitives
// of the persistent forms, the cell update of each direction, the tile helpers.
// The compiler simplifies a __forceinline__ helper on its own BEFORE it inlines it: its parameters then rank below every
// instruction when sums and products are ordered, and a reference parameter becomes a value loaded ahead of the call.  So a
// helper takes what a kernel loaded late as a callable or a pointer and returns what stayed in a register.  Where even that
// changed the machine code the kernels keep their own spelling: index arithmetic, operand prefetch, the tagged-word waits,
// the accumulator store of the ticket kernels, the cell of lstm_fwd_ll_kernel and of lstm_bwd_step_kernel.
#pragma once
#include <math.h>

#include "common.h"

namespace {

struct LstmArgs {
    const float* gx; int64_t ldg;      // input projection + both biases, f32 [B*S, 8H]: col = dir*4H + gate*H + unit
    const bf16_t* whh;                 // forward: [2][4H][H] (gate-row, k contiguous); backward: W_hh^T [2][H][4H]
    bf16_t* y;                         // [B, S, 2H] hidden states (= LSTM output), col = dir*H + unit
    float* c_all;                      // [B, S, 2, H] cell states
    bf16_t* act;                       // [B, S, 2, 4H] gate activations i, f, g, o
    bf16_t* hprev;                     // [B, S, 2H] h_{t-1} of every step (operand of the dW_hh GEMM), may be NULL
    const bf16_t* dy;                  // [B, S, 2H] gradient of the output
    bf16_t* dgates;                    // [B*S, 8H] gate pre-activation gradients
    float* dc_carry;                   // [2, B, H] dc_{t+1} * f_{t+1}
    int B, S, H, step;
    int poll_limit;                    // persistent forms: polls before a hand-off wait gives up (error word + NaN poison)
    int test_drop;                     // test hook (icka_lstm_test_hooks): block (0, 0, 0) does not publish this step; -1 = off
    const int32_t* lens;               // [B] sequence lengths on the device (icka_lstm_*_varlen), NULL = every row has S steps
};

// ---- sequence lengths (icka_lstm_fwd_varlen / icka_lstm_bwd_varlen; include/icka_hip.h states the contract)
// A kernel reads the lengths of its rows ONCE, at its start, clamped to [0, S]; no host value derived from them enters a
// launch.  Positions t >= len[b] are pads: the forward kernels replace the i and f pre-activations they load from gates_x
// by LSTM_PAD_GATE there (a select at the load, the cell code is untouched): sigmoid_f gives exactly 0, so c = 0 and h = 0
// exactly, and the backward's gate gradients are exactly 0 without knowing about lengths at all.
constexpr float LSTM_PAD_GATE = -1e4f;
__device__ __forceinline__ int lstm_len(const int32_t* lens, int b, int S) {
    if (!lens) return S;
    const int v = lens[b];
    return v < 0 ? 0 : (v > S ? S : v);
}
// 16-byte fragment of a k-contiguous row (8 bf16); zero when the row is invalid
__device__ __forceinline__ bf16x8 frag16(const bf16_t* row, bool ok) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (ok) v = *reinterpret_cast<const u32x4*>(row);
    return as_bf16x8(v);
}

constexpr int MAX_RT = 4;   // batch row tiles of 16 (B <= 64 per launch)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    return (uint32_t)__builtin_bit_cast(unsigned short, f2bf(lo)) | ((uint32_t)__builtin_bit_cast(unsigned short, f2bf(hi)) << 16);
}

// Forward: i, f, o = sigmoid, g = tanh of the pre-activations z(0 .. 3); c = f c' + i g; returns h = o tanh(c).  z is a
// callable, evaluated where its value is used: each kernel adds its partial sums in its own order and its LDS loads stay
// between the activations.  c' comes through a pointer and is read after the gates, where the kernels read it.
template <class Z>
__device__ __forceinline__ float lstm_cell_fwd(Z z, const float* c_prev, float& gi_, float& gf_, float& gg_, float& go_, float& c_) {
    const float gi = sigmoid_f(z(0)), gf = sigmoid_f(z(1)), gg = tanhf(z(2)), go = sigmoid_f(z(3));
    const float cp = *c_prev, c = gf * cp + gi * gg;
    gi_ = gi; gf_ = gf; gg_ = gg; go_ = go; c_ = c;
    return go * tanhf(c);
}
// Backward: dh = dy + the recurrent part (summed by the caller), g = the saved activations, c / cp = c_t / c_{t-1},
// carry = dc_{t+1} f_{t+1}.  The gate pre-activation gradients di, df, dg, do go where the caller binds them (LDS);
// returns the next carry dc_t f_t.
__device__ __forceinline__ float lstm_cell_bwd(float dh, const float (&g)[4], float c, float cp, float carry, bf16_t& di, bf16_t& df,
                                               bf16_t& dg, bf16_t& dout) {
    const float gi = g[0], gf = g[1], gg = g[2], go = g[3];
    const float tc = tanhf(c);
    const float dc = dh * go * (1.f - tc * tc) + carry;
    const float next = dc * gf;
    di = f2bf(dc * gg * gi * (1.f - gi));
    df = f2bf(dc * cp * gf * (1.f - gf));
    dg = f2bf(dc * gi * (1.f - gg * gg));
    dout = f2bf(dh * tc * go * (1.f - go));
    return next;
}
// MFMA accumulator tiles D[i = unit 4 g4 + q][j = batch i15] of this wave to its LDS plane [batch row][unit]
template <int NRT, int ROWS>
__device__ __forceinline__ void lstm_acc_to_lds(float (&s)[ROWS][17], const f32x4 (&acc)[NRT], int i15, int g4) {
#pragma unroll
    for (int r = 0; r < NRT; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[16 * r + i15][4 * g4 + q] = acc[r][q];
}

// ---- hand-offs of the persistent forms (lstm.hip describes the forms themselves)
struct LstmPersist {
    unsigned int* tickets;   // [2] per-direction step counters, zeroed by the host before the launch
    unsigned int* err;       // [1] set to 1 if a barrier wait gave up
};

// Hand-off form (cdna_hip_programming.md Guideline 16): the payload another block reads (h_t / dgates_t) is stored
// WRITE-THROUGH with 8-byte agent-scope atomic stores (sc1), every storing wave drains its stores (s_waitcnt vmcnt(0)),
// the block barrier joins them and ONE lane adds the ticket; the consumer polls with one lane, that lane issues ONE
// agent-scope acquire (invalidates this CU's L1) and drains it, the block barrier releases the other waves to plain
// loads.  No release fence (buffer_wbl2) and no per-thread __threadfence(): those made a step ~26 us.
__device__ __forceinline__ void lstm_store_wt(void* p, unsigned long long v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// A wait that gives up (a peer block that is not resident, a lost word) must not pass for a result: it raises the error
// word -- host-visible memory when the library could map it (lstm_err_word), so the host reads it without a device
// synchronisation -- and POISONS the recurrence: the waiting block continues with NaN operands, which reach every later
// step of every block through h / dgates, so y, the loss and the gradients of the call are NaN.  Once poisoned a block no
// longer spins (a failed launch costs one time-out, not one per step).
__device__ __forceinline__ void lstm_raise(unsigned int* err) {
    __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ float lstm_nan() { return __uint_as_float(0x7fc00000u); }
template <int N>
__device__ __forceinline__ void lstm_poison(f32x4 (&acc)[N]) {
#pragma unroll
    for (int r = 0; r < N; ++r) acc[r] = f32x4{lstm_nan(), lstm_nan(), lstm_nan(), lstm_nan()};
}
// returns true (to every thread of the block) when the block is poisoned; ``s_poison`` is a __shared__ word zeroed at kernel start
__device__ __forceinline__ bool lstm_grid_wait(unsigned int* ctr, unsigned int target, unsigned int* err, int limit,
                                               int* s_poison) {
    if (threadIdx.x == 0) {
        int polls = 0;
        if (*s_poison == 0)
            while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
                __builtin_amdgcn_s_sleep(2);
                if (++polls > limit) { lstm_raise(err); *s_poison = 1; break; }
            }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    return *s_poison != 0;
}
__device__ __forceinline__ void lstm_grid_signal(unsigned int* ctr) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains its write-through stores
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Tagged words ({payload, u32 tag} in 8 bytes, two per 16-byte load) are read past this CU's L1.
__device__ __forceinline__ u32x4 ll_load16(const unsigned long long* p) {
    u32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(v) : "v"(p) : "memory");
    return v;
}

}  // namespace
