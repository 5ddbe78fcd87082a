// xq_legal.hip.h — the legal-move TD bootstrap (xq_dqn_set_td_bootstrap, DESIGN.md §4 "Legal-move bootstrap"): per minibatch row the
// largest pre-activation z(s')[to_k] over the moves (from_k, to_k) of getAllValidActions(s', side) in the canonical order, by the env
// kernel's greedy pick (first maximum, a NaN never wins, nothing wins: entry 0), in place of the maximum over all 8100 outputs.
// (kernel half of xq_dqn.hip; included by xq_dqn.hip only, behind xq_l0.hip.h for SlotSrc / slot_of; the rules engine is xq_rules.hip.h)
#pragma once

#include "xq_rules.hip.h"

namespace xq {

enum { kLegalMaxSlabs = 8 };

struct LegalArgs {
    // the transitions, by slot (slot_of): the next board, the action (< 0: a dead row), done and the side to move in the next board
    const uint32_t* next_boards; const int32_t* action_to; const uint8_t* done; const uint8_t* side;
    // the 96-row head product of s' by minibatch row: nslabs k-slabs [nslabs][n][96] without the bias (q_head_finish_kernel's layout and
    // association) and the output bias — of the net that selects, and (Double DQN) of the net that evaluates, else nullptr
    const float* sel_slabs; const float* sel_bias;
    const float* ev_slabs; const float* ev_bias;
    long long slab_stride; int nslabs;
    // out, by minibatch row: z96 [n][96] the selecting net's pre-activations, zmax the bootstrap's pre-activation (0 where y = r: done,
    // dead; no move: no_move_zmax), zidx the winning `to` (-1 there), n_moves the list length (-1 on done and dead rows)
    float* z96; float* zmax; int* zidx; int* n_moves;
    // what zmax gets where the side to move in s' has no move: 0 (y = r), or -inf under the zero-sum target (tanh: -1, y = r + g)
    float no_move_zmax;
};

// k-slabs summed in groups of four, (p0 + p1) + (p2 + p3), the groups in order, plus the bias — q_head_finish_kernel's association where
// the count is even, and right for every count 1..kLegalMaxSlabs (launch_gemm may leave fewer slabs than asked: 7 for K = 640 or 896):
// slabs past nslabs were loaded as 0, and a group is skipped only when it holds none
__device__ __forceinline__ float legal_head_sum(const float (&p)[kLegalMaxSlabs], int nslabs, float bias) {
    float sum = 0.f;
#pragma unroll
    for (int z = 0; z < kLegalMaxSlabs; z += 4) {
        if (z < nslabs) {
            float t = p[z] + p[z + 1];
            if (z + 2 < nslabs) t += p[z + 2] + p[z + 3];
            sum = z == 0 ? t : sum + t;
        }
    }
    return bias + sum;
}

// One wavefront per minibatch row, four rows per block (env_kernel's arrangement).  Every load of the row — the 12 board words, done,
// the action, the side byte, the slabs and biases of the row's two outputs per lane (lane, 64 + lane < 96) — is issued before the first
// use.  A done or dead row leaves wave-uniformly behind its z96 row; every other row generates the side's moves and picks with
// env_kernel's two-register pick on z96[to] (the raw pre-activations: no tanh, so the pick is the one xq_env_selfplay_step makes on
// the same values).
__global__ __launch_bounds__(256) void legal_qmax_kernel(LegalArgs A, SlotSrc src, int n) {
    __shared__ WaveSlab slabs[4];
    __shared__ float qev[4][96];
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = lane_id();
    const int b = (int)blockIdx.x * 4 + wid;
    if (b >= n) return;                                      // (wave-uniform; no block-wide barrier below)
    WaveSlab& S = slabs[wid];
    const int s = __builtin_amdgcn_readfirstlane(slot_of(src, b));
    const int j1 = 64 + (lane < 32 ? lane : 0);
    const bool dbl = A.ev_slabs != nullptr;
    uint32_t word = 0;
    if (lane < kBoardWords) word = A.next_boards[(size_t)s * kBoardWords + lane];
    const int a = A.action_to[s];
    const uint8_t dn = A.done[s], sd = A.side[s];
    float p0[kLegalMaxSlabs], p1[kLegalMaxSlabs], e0[kLegalMaxSlabs], e1[kLegalMaxSlabs];
    const size_t row = (size_t)b * 96;
#pragma unroll
    for (int z = 0; z < kLegalMaxSlabs; ++z) {
        const bool in = z < A.nslabs;
        p0[z] = in ? A.sel_slabs[z * A.slab_stride + row + lane] : 0.f;
        p1[z] = in ? A.sel_slabs[z * A.slab_stride + row + j1] : 0.f;
        e0[z] = in && dbl ? A.ev_slabs[z * A.slab_stride + row + lane] : 0.f;
        e1[z] = in && dbl ? A.ev_slabs[z * A.slab_stride + row + j1] : 0.f;
    }
    const float pb0 = A.sel_bias[lane], pb1 = A.sel_bias[j1];
    const float eb0 = dbl ? A.ev_bias[lane] : 0.f, eb1 = dbl ? A.ev_bias[j1] : 0.f;

    const float z0 = legal_head_sum(p0, A.nslabs, pb0), z1 = legal_head_sum(p1, A.nslabs, pb1);
    A.z96[row + lane] = z0;
    if (lane < 32) A.z96[row + 64 + lane] = z1;
    if (dn != 0 || a < 0) {                                  // y = r (done) or no sample at all (dead): no move generation
        if (lane == 0) { A.zmax[b] = 0.f; A.zidx[b] = -1; A.n_moves[b] = -1; }
        return;
    }
    unpack_to_slab(word, S.sq);
    wave_sync();
    const int n_moves = gen_all_actions(S, sd != 0 ? C_BLACK : C_RED);
    S.q[lane] = z0;
    if (lane < 32) S.q[64 + lane] = z1;
    if (dbl) {
        qev[wid][lane] = legal_head_sum(e0, A.nslabs, eb0);
        if (lane < 32) qev[wid][64 + lane] = legal_head_sum(e1, A.nslabs, eb1);
    }
    wave_sync();
    if (n_moves <= 0) {                                      // the side has no move in s': y = r (zero-sum: it has lost, y = r + g)
        if (lane == 0) { A.zmax[b] = A.no_move_zmax; A.zidx[b] = -1; A.n_moves[b] = 0; }
        return;
    }
    const float NEG = -__builtin_inff();
    float v0 = NEG, v1 = NEG;
    if (lane < n_moves) v0 = S.q[S.moves[lane] % 90];
    if (n_moves > 64) {                                      // (wave-uniform)
        if (lane + 64 < n_moves) v1 = S.q[S.moves[lane + 64] % 90];
    }
    if (!(v0 == v0)) v0 = NEG;                               // a NaN never wins
    if (!(v1 == v1)) v1 = NEG;
    const float ma = wave_max(v0), mb = wave_max(v1);
    int idx;
    if (mb > ma) {                                           // strict >: the first maximum wins
        const unsigned long long m = __ballot(lane + 64 < n_moves && v1 == mb);
        idx = m ? 64 + (__ffsll((long long)m) - 1) : 0;
    } else {
        const unsigned long long m = __ballot(lane < n_moves && v0 == ma);
        idx = m ? (__ffsll((long long)m) - 1) : 0;           // nothing wins (all -inf or NaN): entry 0 of the list
    }
    const int to = __builtin_amdgcn_readfirstlane((int)S.moves[idx]) % 90;
    if (lane == 0) {
        A.zmax[b] = dbl ? qev[wid][to] : S.q[to];
        A.zidx[b] = to;
        A.n_moves[b] = n_moves;
    }
}

// The side bytes of a staged batch (n-step: of the slot whose next board was staged; mirror: of the sampled slot — a reflection does not
// change the side): out[b] = ring_side[row_slot[b]]
__global__ __launch_bounds__(256) void legal_side_stage_kernel(const uint8_t* __restrict__ ring_side, const int32_t* __restrict__ row_slot,
                                                               uint8_t* __restrict__ out, int n, int cap) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= n) return;
    const int s = row_slot[b];
    out[b] = (unsigned)s < (unsigned)cap ? ring_side[s] : (uint8_t)0;
}

}  // namespace xq
