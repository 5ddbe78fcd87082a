// xq_nstep.hip.h — n-step TD returns from the replay ring (xq_replay_set_n_step, DESIGN.md §4 "n-step returns"): the gather that
// assembles a minibatch of n-step transitions into the handle's staging buffers, on which the TD step then runs unchanged, and the
// priority write-back of a prioritized draw behind that step.
// (kernel half of xq_dqn.hip; included by xq_dqn.hip only, behind xq_l0.hip.h for SlotSrc / slot_of)
#pragma once

namespace xq {

enum { kNStepMax = 8 };        // == XQ_MAX_N_STEP

struct NStepArgs {
    // the ring (read)
    const uint32_t* boards; const uint32_t* next_boards; const int32_t* action_to; const float* reward; const uint8_t* done;
    int cap, first, count, stride, n;        // readable range: `count` slots in age order from slot `first`; chain of n, `stride` apart
    float disc[kNStepMax];                   // disc[k] = gamma^k in fp32, one rounding per factor (host)
    // the staging batch (written), row b
    uint32_t* s_boards; uint32_t* s_next; int32_t* s_action; float* s_reward; uint8_t* s_done;
    int32_t* s_m; int32_t* s_first; int32_t* s_last;
};

// One thread per row.  The chain's slots are arithmetic on the sampled slot, so every action / reward / done load of the chain and the
// three 16-byte pieces of boards[s] are issued before anything is used; the scan runs in registers; the one dependent round trip is
// next_boards[slot_{m-1}], three 16-byte loads.  A slot is 48 B and the arrays come from hipMalloc, so every board is 16-byte aligned.
__global__ __launch_bounds__(64) void nstep_assemble_kernel(NStepArgs A, SlotSrc src, int batch) {
    // One rounding per operation.  Not __fmul_rn / __fadd_rn: to the compiler they are a plain product and a plain sum compiled under the
    // default -ffp-contract=fast, and a product that feeds a sum (as here, unlike per_sample_kernel's sum that feeds a product) is
    // contracted into one fma.  The pragma covers the operators written in this function.
#pragma clang fp contract(off)
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= batch) return;
    const int s = slot_of(src, b);
    long long off0 = (long long)s - A.first;
    if (off0 < 0) off0 += A.cap;
    int slot[kNStepMax]; bool exists[kNStepMax];
    int a[kNStepMax]; float r[kNStepMax]; uint8_t dn[kNStepMax];
#pragma unroll
    for (int k = 0; k < kNStepMax; ++k) {
        const long long off = off0 + (long long)k * A.stride;             // (< 2 cap: (n - 1) stride < cap)
        exists[k] = k < A.n && off < (long long)A.count;
        slot[k] = k == 0 ? s : (int)(((long long)A.first + off) % A.cap);
    }
#pragma unroll
    for (int k = 0; k < kNStepMax; ++k) {
        // only what exists is read (the sampled slot always): beside an overlapped collect the slots past the readable range are being written
        const bool ld = k == 0 || exists[k];
        a[k] = ld ? A.action_to[slot[k]] : -1;
        r[k] = ld ? A.reward[slot[k]] : 0.f;
        dn[k] = ld ? A.done[slot[k]] : (uint8_t)0;
    }
    const uint4* own = reinterpret_cast<const uint4*>(A.boards + (long long)s * kBoardWords);
    const uint4 b0 = own[0], b1 = own[1], b2 = own[2];
    float R = r[0];
    bool D = dn[0] != 0;
    bool dead = a[0] < 0, stop = dead || D;
    int m = 1;
#pragma unroll
    for (int k = 1; k < kNStepMax; ++k) {
        if (k < A.n && !stop) {
            if (!exists[k] || a[k] < 0) { dead = true; stop = true; }
            else {
                const float term = A.disc[k] * r[k];
                R = R + term;
                D = dn[k] != 0;
                m = k + 1;
                stop = D;
            }
        }
    }
    int last = s;
#pragma unroll
    for (int k = 1; k < kNStepMax; ++k) if (k == m - 1) last = slot[k];
    const uint4* nx = reinterpret_cast<const uint4*>(A.next_boards + (long long)(dead ? s : last) * kBoardWords);
    const uint4 n0 = nx[0], n1 = nx[1], n2 = nx[2];
    uint4* ob = reinterpret_cast<uint4*>(A.s_boards + (long long)b * kBoardWords);
    uint4* on = reinterpret_cast<uint4*>(A.s_next + (long long)b * kBoardWords);
    ob[0] = b0; ob[1] = b1; ob[2] = b2;
    on[0] = n0; on[1] = n1; on[2] = n2;
    A.s_action[b] = dead ? -1 : a[0];
    A.s_reward[b] = R;
    A.s_done[b] = D ? (uint8_t)1 : (uint8_t)0;
    A.s_m[b] = m; A.s_first[b] = s; A.s_last[b] = last;
}

// Behind the TD step of a prioritized n-step draw: prio[first_slot[b]] = (|q - y| + eps)^alpha for the live rows, and the running maximum
// by td_delta_kernel's test-then-atomicMax (per_priority_store, xq_td.hip.h)
__global__ __launch_bounds__(256) void per_writeback_kernel(int n, const float* __restrict__ qsa, const float* __restrict__ yv,
                                                            const int32_t* __restrict__ act, const int32_t* __restrict__ first_slot,
                                                            float* __restrict__ prio, unsigned* pmax_live, float eps, float alpha) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= n) return;
    if (act[b] < 0) return;
    per_priority_store(prio, pmax_live, first_slot[b], qsa[b], yv[b], eps, alpha);
}

}  // namespace xq
