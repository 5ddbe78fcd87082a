// xq_view.hip.h — mover-relative board view (xq_dqn_set_view, DESIGN.md §4 "Mover view"): view(board, side) is the board when Red is to
// move and its colour swap (xq_colour_swap.hip.h: row -> 9 - row, Red <-> Black) when Black is.  view_boards_kernel maps packed boards
// with a side each; mover_view_stage_kernel is the last staging transform of a TD step from a ring: s by who moved, s' by who moves
// next, the action with s.  The ring is never written.
// (kernel half of xq_dqn.hip; included by xq_dqn.hip only, behind xq_colour_swap.hip.h, whose colour_swap_board and whose layout notes
// — with xq_mirror.hip.h's mirror_unpack — it shares)
#pragma once

namespace xq {

// One thread per board.  The three 16-byte loads and the side are issued before the first use; the board is transformed unconditionally
// and selected by the side: no wave diverges on it.  The side of board b is side[b] != 0 or, with meta != nullptr (uniform over the
// launch: the boards are an env's), bit 16 of meta[b].x.  Nibbles 90..95 come out 0 on the swapped boards and as they were on the others.
__global__ __launch_bounds__(64) void view_boards_kernel(const uint32_t* __restrict__ boards, const uint8_t* __restrict__ side,
                                                         const uint4* __restrict__ meta, int n, uint32_t* __restrict__ out) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= n) return;
    const uint4* pb = reinterpret_cast<const uint4*>(boards + (long long)b * kBoardWords);
    const uint4 b0 = pb[0], b1 = pb[1], b2 = pb[2];
    const bool black = meta != nullptr ? ((meta[b].x >> 16) & 1u) != 0u : side[b] != 0;
    const uint32_t keep = black ? 0u : 0xFFFFFFFFu;
    uint32_t w[kBoardWords], o[kBoardWords];
    mirror_unpack(b0, b1, b2, w);
    colour_swap_board(w, o);
#pragma unroll
    for (int i = 0; i < kBoardWords; ++i) o[i] = (w[i] & keep) | (o[i] & ~keep);
    uint4* ob = reinterpret_cast<uint4*>(out + (long long)b * kBoardWords);
    ob[0] = make_uint4(o[0], o[1], o[2], o[3]); ob[1] = make_uint4(o[4], o[5], o[6], o[7]); ob[2] = make_uint4(o[8], o[9], o[10], o[11]);
}

struct MoverViewArgs {
    // what is read: the ring by slot (gather form), or the staging batch itself by row (in place, behind nstep_assemble_kernel and / or
    // mirror_stage_kernel)
    const uint32_t* boards; const uint32_t* next_boards; const int32_t* action_to; const float* reward; const uint8_t* done;
    // the staging batch (written), row b; s_reward / s_done / s_first: gather form only
    uint32_t* s_boards; uint32_t* s_next; int32_t* s_action; float* s_reward; uint8_t* s_done; int32_t* s_first;
    // the ring's two side columns, by slot: flag_s = mover[first slot], flag_s' = next_player[the slot whose s' was staged].  In place
    // the two slots are row_first[b] and row_last[b] (behind the n-step assembly its first and last slot; behind the mirror alone both are
    // the sampled slot); the gather form takes the gathered slot for both and reads neither array
    const uint8_t* mover; const uint8_t* next_player; const int32_t* row_first; const int32_t* row_last;
    uint8_t* s_flag; uint8_t* s_flag_next;   // the two flags, per row
    uint8_t* s_side;                         // legal-move bootstrap only (else nullptr): the staged side to move in s' — 0, Red, on every row
    int cap;
    uint32_t gather;                         // 1: from the ring by slot_of; 0: the staging batch in place
};

// colour_swap_stage_kernel's sibling, in its two forms.  One thread per row, the slot from slot_of.  Every load of the row — six 16-byte
// board loads, the action, in the gather form reward and done, in place the two slots — is issued before the first use, so a thread has
// read its whole row before it writes any of it (in place the rows it reads are the rows it writes); only the two side bytes, whose
// addresses are the slots, follow.  Both boards are transformed unconditionally and selected each by its own flag: no wave diverges.
__global__ __launch_bounds__(64) void mover_view_stage_kernel(MoverViewArgs A, SlotSrc src, int batch) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= batch) return;
    const bool gather = A.gather != 0u;
    const int s = gather ? slot_of(src, b) : b;
    int sf = s, sl = s;
    if (!gather) { sf = A.row_first[b]; sl = A.row_last[b]; }
    const uint4* pb = reinterpret_cast<const uint4*>(A.boards + (long long)s * kBoardWords);
    const uint4* pn = reinterpret_cast<const uint4*>(A.next_boards + (long long)s * kBoardWords);
    const uint4 b0 = pb[0], b1 = pb[1], b2 = pb[2];
    const uint4 n0 = pn[0], n1 = pn[1], n2 = pn[2];
    const int a = A.action_to[s];
    float rw = 0.f; uint8_t dn = 0, mv = 0, np = 0;
    if (gather) { rw = A.reward[s]; dn = A.done[s]; }
    if ((unsigned)sf < (unsigned)A.cap) mv = A.mover[sf];
    if ((unsigned)sl < (unsigned)A.cap) np = A.next_player[sl];
    const bool flag = mv != 0, flag_next = np != 0;
    const uint32_t keep = flag ? 0u : 0xFFFFFFFFu, keep_next = flag_next ? 0u : 0xFFFFFFFFu;
    uint32_t w[kBoardWords], o[kBoardWords], wn[kBoardWords], on[kBoardWords];
    mirror_unpack(b0, b1, b2, w);
    mirror_unpack(n0, n1, n2, wn);
    colour_swap_board(w, o);
    colour_swap_board(wn, on);
#pragma unroll
    for (int i = 0; i < kBoardWords; ++i) {
        o[i] = (w[i] & keep) | (o[i] & ~keep);
        on[i] = (wn[i] & keep_next) | (on[i] & ~keep_next);
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
    A.s_flag_next[b] = flag_next ? (uint8_t)1 : (uint8_t)0;
    if (gather) { A.s_reward[b] = rw; A.s_done[b] = dn; A.s_first[b] = s; }
    if (A.s_side != nullptr) A.s_side[b] = 0;
}

}  // namespace xq
