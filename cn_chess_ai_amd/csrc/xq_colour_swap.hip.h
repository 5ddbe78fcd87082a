// xq_colour_swap.hip.h — colour-swap augmentation of replay batches (xq_replay_set_colour_swap, DESIGN.md §4 "Colour-swap
// augmentation"): the staging transform that exchanges the colours of a Philox-chosen part of a minibatch while turning the board top to
// bottom (row -> 9 - row, Red <-> Black: both boards, the action's square and, under the legal-move bootstrap, the side to move in s')
// in the handle's staging buffers, on which the TD step then runs unchanged.  The ring is never written.
// (kernel half of xq_dqn.hip; included by xq_dqn.hip only, behind xq_mirror.hip.h, whose mirror_unpack and layout notes it shares)
#pragma once

namespace xq {

struct ColourSwapArgs {
    // what is read: the ring by slot (gather form), or the staging batch itself by row (in place, behind nstep_assemble_kernel and / or
    // mirror_stage_kernel)
    const uint32_t* boards; const uint32_t* next_boards; const int32_t* action_to; const float* reward; const uint8_t* done;
    // the staging batch (written), row b; s_reward / s_done / s_first: gather form only
    uint32_t* s_boards; uint32_t* s_next; int32_t* s_action; float* s_reward; uint8_t* s_done; int32_t* s_first; uint8_t* s_flag;
    // legal-move bootstrap only (ring_side == nullptr: no side is staged): s_side[b] = flag_b ? 1 - ring_side[slot] : ring_side[slot], the slot from
    // row_slot[b] (in place: the slot whose side the staged row takes) or, with row_slot == nullptr, the gathered slot itself
    const uint8_t* ring_side; const int32_t* row_slot; uint8_t* s_side;
    int cap;
    uint32_t thresh, all;                    // flag_b = all || philox(b, 0, call, 4).v[0] < thresh
    uint32_t gather;                         // 1: from the ring by slot_of; 0: the staging batch in place
    uint32_t call, seed_lo, seed_hi;
};

// sigma on the eight nibbles of a word at once: 0 stays, 1..7 (Red) + 7, 8..14 (Black) - 7.  `hi` holds a 1 at the bottom of every nibble
// whose high bit is set, `nz` at every non-zero nibble; neither step carries across a nibble (7 + 7 = 14, 8 - 7 = 1).
__device__ __forceinline__ uint32_t colour_swap_codes(uint32_t x) {
    const uint32_t hi = (x >> 3) & 0x11111111u;
    const uint32_t nz = (x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x11111111u;
    return x + 7u * (nz & ~hi) - 7u * hi;
}

// Board row r is the 36 bits from bit 36 r (xq_mirror.hip.h), so row r of the image is row 9 - r of sigma(board): the 36-bit field is
// cut out of the 64-bit window of its two words at nibble phase r mod 8 and ORed into zeroed words at the phase of 9 - r, so nibbles
// 90..95 come out 0.  Fully unrolled: every word index and shift is a compile-time constant.
__device__ __forceinline__ void colour_swap_board(const uint32_t (&w)[kBoardWords], uint32_t (&o)[kBoardWords]) {
    uint32_t c[kBoardWords];
#pragma unroll
    for (int i = 0; i < kBoardWords; ++i) { c[i] = colour_swap_codes(w[i]); o[i] = 0u; }
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const int wi = (36 * r) >> 5, sh = (36 * r) & 31;
        const int wo = (36 * (9 - r)) >> 5, so = (36 * (9 - r)) & 31;
        const uint64_t win = (uint64_t)c[wi] | ((uint64_t)c[wi + 1] << 32);
        const uint64_t y = ((win >> sh) & 0xFFFFFFFFFull) << so;       // (so <= 28: the 36 bits stay inside the window)
        o[wo] |= (uint32_t)y;
        o[wo + 1] |= (uint32_t)(y >> 32);
    }
}

// mirror_stage_kernel's sibling, in its two forms.  One thread per row, the slot from slot_of.  Every load of the row — six 16-byte board
// loads, the action, in the gather form reward and done, under the legal bootstrap the side's slot — is issued before the first use, so a
// thread has read its whole row before it writes any of it (in place the rows it reads are the rows it writes); only the side byte, whose
// address is the loaded slot, follows.  Both boards are transformed unconditionally and selected by the flag: no wave diverges on it.
// A.gather (uniform over the launch): from the ring at the sampled slot into the staging batch, with the slot and the flag; otherwise the
// staging batch in place (boards, action and the flag; reward, done, the slot and the n-step row fields are left alone).
__global__ __launch_bounds__(64) void colour_swap_stage_kernel(ColourSwapArgs A, SlotSrc src, int batch) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= batch) return;
    const bool gather = A.gather != 0u;
    const bool sided = A.ring_side != nullptr;
    const int s = gather ? slot_of(src, b) : b;
    int ss = s;
    if (sided && A.row_slot) ss = A.row_slot[b];
    const uint4* pb = reinterpret_cast<const uint4*>(A.boards + (long long)s * kBoardWords);
    const uint4* pn = reinterpret_cast<const uint4*>(A.next_boards + (long long)s * kBoardWords);
    const uint4 b0 = pb[0], b1 = pb[1], b2 = pb[2];
    const uint4 n0 = pn[0], n1 = pn[1], n2 = pn[2];
    const int a = A.action_to[s];
    float rw = 0.f; uint8_t dn = 0, sd = 0;
    if (gather) { rw = A.reward[s]; dn = A.done[s]; }
    if (sided && (unsigned)ss < (unsigned)A.cap) sd = A.ring_side[ss];
    const bool flag = A.all != 0u || philox4x32_10((uint32_t)b, 0u, A.call, 4u, A.seed_lo, A.seed_hi).v[0] < A.thresh;
    const uint32_t keep = flag ? 0u : 0xFFFFFFFFu;
    uint32_t w[kBoardWords], o[kBoardWords], wn[kBoardWords], on[kBoardWords];
    mirror_unpack(b0, b1, b2, w);
    mirror_unpack(n0, n1, n2, wn);
    colour_swap_board(w, o);
    colour_swap_board(wn, on);
#pragma unroll
    for (int i = 0; i < kBoardWords; ++i) {
        o[i] = (w[i] & keep) | (o[i] & ~keep);
        on[i] = (wn[i] & keep) | (on[i] & ~keep);
    }
    const int as = a + 81 - 18 * (a / 9);    // (9 - row, col) of a square 0..89; anything else (-1: dead or empty, 90..95) stays
    const int ao = (flag && a >= 0 && a < 90) ? as : a;
    uint4* ob = reinterpret_cast<uint4*>(A.s_boards + (long long)b * kBoardWords);
    uint4* onx = reinterpret_cast<uint4*>(A.s_next + (long long)b * kBoardWords);
    ob[0] = make_uint4(o[0], o[1], o[2], o[3]); ob[1] = make_uint4(o[4], o[5], o[6], o[7]); ob[2] = make_uint4(o[8], o[9], o[10], o[11]);
    onx[0] = make_uint4(on[0], on[1], on[2], on[3]); onx[1] = make_uint4(on[4], on[5], on[6], on[7]);
    onx[2] = make_uint4(on[8], on[9], on[10], on[11]);
    A.s_action[b] = ao;
    A.s_flag[b] = flag ? (uint8_t)1 : (uint8_t)0;
    if (gather) { A.s_reward[b] = rw; A.s_done[b] = dn; A.s_first[b] = s; }
    if (sided) A.s_side[b] = flag ? (uint8_t)(1 - sd) : sd;
}

}  // namespace xq
