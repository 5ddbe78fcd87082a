// xq_mirror.hip.h — mirror augmentation of replay batches (xq_replay_set_mirror, DESIGN.md §4 "Mirror augmentation"): the staging
// transform that reflects a Philox-chosen part of a minibatch left-right (col -> 8 - col: both boards and the action's square) in the
// handle's staging buffers, on which the TD step then runs unchanged.  The ring is never written.
// (kernel half of xq_dqn.hip; included by xq_dqn.hip only, behind xq_l0.hip.h for SlotSrc / slot_of and beside xq_nstep.hip.h)
#pragma once

namespace xq {

struct MirrorArgs {
    // what is read: the ring by slot (gather form), or the staging batch itself by row (in place, behind nstep_assemble_kernel)
    const uint32_t* boards; const uint32_t* next_boards; const int32_t* action_to; const float* reward; const uint8_t* done;
    // the staging batch (written), row b; s_reward / s_done / s_first: gather form only
    uint32_t* s_boards; uint32_t* s_next; int32_t* s_action; float* s_reward; uint8_t* s_done; int32_t* s_first; uint8_t* s_flag;
    uint32_t thresh, all;                    // flag_b = all || philox(b, 0, call, 3).v[0] < thresh
    uint32_t gather;                         // 1: from the ring by slot_of; 0: the staging batch in place
    uint32_t call, seed_lo, seed_hi;
};

// A board is 96 nibbles in 12 words, square s = nibble s & 7 of word s >> 3, so board row r is the 36 bits from bit 36 r: it starts at
// nibble phase r mod 8 and straddles two words (rows 0-7: words r, r + 1; row 8: 9, 10; row 9: 10, 11).  Per row: the 64-bit window of
// its two words, shifted and masked to 36 bits; its nine nibbles reversed (byte swap, the nibbles of each byte swapped: sixteen nibbles
// reversed, nibble i -> 15 - i; down by 7 nibbles: i -> 8 - i); shifted back and ORed into zeroed words, so nibbles 90..95 come out 0.
// Fully unrolled: every word index is a compile-time constant (a register array indexed at run time would go to scratch).
__device__ __forceinline__ void mirror_board(const uint32_t (&w)[kBoardWords], uint32_t (&o)[kBoardWords]) {
#pragma unroll
    for (int i = 0; i < kBoardWords; ++i) o[i] = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const int wi = (36 * r) >> 5, sh = (36 * r) & 31;
        const uint64_t win = (uint64_t)w[wi] | ((uint64_t)w[wi + 1] << 32);
        const uint64_t x = (win >> sh) & 0xFFFFFFFFFull;
        uint64_t y = __builtin_bswap64(x);
        y = ((y & 0x0F0F0F0F0F0F0F0Full) << 4) | ((y >> 4) & 0x0F0F0F0F0F0F0F0Full);
        y = (y >> 28) << sh;                 // (sh <= 28: the 36 bits stay inside the window)
        o[wi] |= (uint32_t)y;
        o[wi + 1] |= (uint32_t)(y >> 32);
    }
}

__device__ __forceinline__ void mirror_unpack(const uint4& a, const uint4& b, const uint4& c, uint32_t (&w)[kBoardWords]) {
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    w[8] = c.x; w[9] = c.y; w[10] = c.z; w[11] = c.w;
}

// One thread per row, the slot from slot_of (nstep_assemble_kernel's layout).  Every load of the row — six 16-byte board loads, the
// action and, in the gather form, reward and done — is issued before the first use, so a thread has read its whole row before it writes
// any of it (in place the rows it reads are the rows it writes).  Both boards are mirrored unconditionally and selected by the flag:
// no wave diverges on it.  A.gather (uniform over the launch): from the ring at the sampled slot into the staging batch, with the slot and
// the flag; otherwise the staging batch in place (boards, action and the flag; reward, done and the n-step row fields are left alone).
__global__ __launch_bounds__(64) void mirror_stage_kernel(MirrorArgs A, SlotSrc src, int batch) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= batch) return;
    const bool gather = A.gather != 0u;
    const int s = gather ? slot_of(src, b) : b;
    const uint4* pb = reinterpret_cast<const uint4*>(A.boards + (long long)s * kBoardWords);
    const uint4* pn = reinterpret_cast<const uint4*>(A.next_boards + (long long)s * kBoardWords);
    const uint4 b0 = pb[0], b1 = pb[1], b2 = pb[2];
    const uint4 n0 = pn[0], n1 = pn[1], n2 = pn[2];
    const int a = A.action_to[s];
    float rw = 0.f; uint8_t dn = 0;
    if (gather) { rw = A.reward[s]; dn = A.done[s]; }
    const bool flag = A.all != 0u || philox4x32_10((uint32_t)b, 0u, A.call, 3u, A.seed_lo, A.seed_hi).v[0] < A.thresh;
    const uint32_t keep = flag ? 0u : 0xFFFFFFFFu;
    uint32_t w[kBoardWords], o[kBoardWords], wn[kBoardWords], on[kBoardWords];
    mirror_unpack(b0, b1, b2, w);
    mirror_unpack(n0, n1, n2, wn);
    mirror_board(w, o);
    mirror_board(wn, on);
#pragma unroll
    for (int i = 0; i < kBoardWords; ++i) {
        o[i] = (w[i] & keep) | (o[i] & ~keep);
        on[i] = (wn[i] & keep) | (on[i] & ~keep);
    }
    const int am = a - 2 * (a % 9) + 8;      // (row, 8 - col) of a square 0..89; anything else (-1: dead or empty, 90..95) stays
    const int ao = (flag && a >= 0 && a < 90) ? am : a;
    uint4* ob = reinterpret_cast<uint4*>(A.s_boards + (long long)b * kBoardWords);
    uint4* onx = reinterpret_cast<uint4*>(A.s_next + (long long)b * kBoardWords);
    ob[0] = make_uint4(o[0], o[1], o[2], o[3]); ob[1] = make_uint4(o[4], o[5], o[6], o[7]); ob[2] = make_uint4(o[8], o[9], o[10], o[11]);
    onx[0] = make_uint4(on[0], on[1], on[2], on[3]); onx[1] = make_uint4(on[4], on[5], on[6], on[7]);
    onx[2] = make_uint4(on[8], on[9], on[10], on[11]);
    A.s_action[b] = ao;
    A.s_flag[b] = flag ? (uint8_t)1 : (uint8_t)0;
    if (gather) { A.s_reward[b] = rw; A.s_done[b] = dn; A.s_first[b] = s; }
}

}  // namespace xq
