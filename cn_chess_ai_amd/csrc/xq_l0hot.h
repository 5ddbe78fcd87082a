// xq_l0hot.h — which rows of gW0^T the matrix pipe works on (xq_l0grad.hip.h): the "hot" rows, a superset of every (square, piece) that
// the move rules can produce from the start position; every other row is "cold" and gets its exact sum from an occurrence list
// (l0_cold_block).  No result depends on this table — it only decides which of the two routes a row takes.  Plain C++, no HIP: built on the
// host once per process, copied to the device as it stands, walked on the CPU by tests/cpp/l0hot_probe.cpp.
//
// The hot set is the closure of each piece kind's start squares under its move rule on an EMPTY board (blockers only take moves away,
// so ignoring them only enlarges the set), with the rules as xq_rules.hip.h::piece_rule states them, quirks included: the general and
// the advisor test "any palace", the advisor's FROM square is not tested at all, the soldier's direction follows its colour.  692 rows:
// chariot, horse, cannon 90 squares each, soldier 55, general 9, elephant 7, advisor 5, per colour.
// Packing: the squares in board order are cut into kL0HotGroups runs of at most kL0HotSqB squares and kL0HotGroupRows hot rows; a run's
// hot rows, in row order, are the packed rows of one row group of the kernel, the rest of the group is padding (kL0NoRow).
#pragma once

#include <cstdint>
#include <cstring>

namespace xq {

constexpr int kL0HotGroups = 3;            // row groups of the kernel's grid
constexpr int kL0HotGroupRows = 256;       // packed rows per group: 4 waves x 4 tiles x 16
constexpr int kL0HotSqB = 32;              // squares whose selector words a group's blocks stage
constexpr uint16_t kL0NoRow = 0xFFFF;
constexpr uint16_t kL0ColdBit = 0x8000;

struct L0HotTable {
    uint16_t row[kL0HotGroups * kL0HotGroupRows];   // packed hot index -> row of gW0^T (square * 14 + piece - 1), kL0NoRow = padding
    uint16_t index[1260];                           // row -> packed hot index, or kL0ColdBit | cold index
    uint16_t cold_row[1260];                        // cold index -> row (ascending), kL0NoRow behind n_cold
    uint16_t hot_mask[96];                          // per square: bit (piece - 1) set = hot
    uint16_t cold_base[96];                         // per square: cold index of its first cold row
    uint16_t sq0[kL0HotGroups + 1];                 // first square of every group; [kL0HotGroups] = 90
    uint16_t n_hot, n_cold, ok, pad_;               // ok = 0: the board does not fit the groups (a bug: nothing may run on the table)
};

namespace l0hot_detail {
inline bool any_palace(int r, int c) { return c >= 3 && c <= 5 && ((r >= 0 && r <= 2) || (r >= 7 && r <= 9)); }
// piece_rule (xq_rules.hip.h) on an empty board; code = 1..14
inline bool rule(int code, int fr, int fc, int tr, int tc) {
    if ((unsigned)tr >= 10u || (unsigned)tc >= 9u) return false;
    const int type = code > 7 ? code - 7 : code;
    const int dr = tr - fr, dc = tc - fc, adr = dr < 0 ? -dr : dr, adc = dc < 0 ? -dc : dc;
    switch (type) {
        case 1: return any_palace(fr, fc) && any_palace(tr, tc) && adr + adc == 1;
        case 2: return any_palace(tr, tc) && adr == 1 && adc == 1;
        case 3: return adr == 2 && adc == 2 && ((fr < 5 && tr < 5) || (fr >= 5 && tr >= 5));
        case 4: return (adr == 2 && adc == 1) || (adr == 1 && adc == 2);
        case 5: case 6: return (fr == tr) != (fc == tc);
        case 7:
            if (code <= 7) return fr < 5 ? (dr == 1 && adc == 0) : ((dr == 1 && adc == 0) || (dr == 0 && adc == 1));
            return fr >= 5 ? (dr == -1 && adc == 0) : ((dr == -1 && adc == 0) || (dr == 0 && adc == 1));
        default: return false;
    }
}
}  // namespace l0hot_detail

inline void l0_hot_build(L0HotTable* t) {
    using namespace l0hot_detail;
    memset(t, 0, sizeof *t);
    // the start position (chessboard.cpp:8-29; xq_common.h::start_position)
    static const uint8_t back[9] = {5, 4, 3, 2, 1, 2, 3, 4, 5};
    uint8_t start[90] = {0};
    for (int c = 0; c < 9; ++c) { start[c] = back[c]; start[81 + c] = (uint8_t)(back[c] + 7); }
    start[19] = start[25] = 6; start[64] = start[70] = 13;
    for (int c = 0; c < 9; c += 2) { start[27 + c] = 7; start[54 + c] = 14; }
    bool hot[1260] = {false};
    for (int s = 0; s < 90; ++s) if (start[s]) hot[s * 14 + start[s] - 1] = true;
    for (bool grew = true; grew;) {
        grew = false;
        for (int code = 1; code <= 14; ++code)
            for (int s = 0; s < 90; ++s) {
                if (!hot[s * 14 + code - 1]) continue;
                for (int d = 0; d < 90; ++d)
                    if (d != s && !hot[d * 14 + code - 1] && rule(code, s / 9, s % 9, d / 9, d % 9)) hot[d * 14 + code - 1] = grew = true;
            }
    }
    for (int i = 0; i < kL0HotGroups * kL0HotGroupRows; ++i) t->row[i] = kL0NoRow;
    for (int i = 0; i < 1260; ++i) t->cold_row[i] = kL0NoRow;
    int g = 0, in_rows = 0, in_sq = 0, n_hot = 0, n_cold = 0;
    bool fits = true;
    t->sq0[0] = 0;
    for (int s = 0; s < 90; ++s) {
        int h = 0;
        for (int p = 0; p < 14; ++p) h += hot[s * 14 + p];
        if (in_rows + h > kL0HotGroupRows || in_sq == kL0HotSqB) {
            if (++g >= kL0HotGroups) { fits = false; break; }
            t->sq0[g] = (uint16_t)s; in_rows = in_sq = 0;
        }
        t->cold_base[s] = (uint16_t)n_cold;
        for (int p = 0; p < 14; ++p) {
            const int r = s * 14 + p;
            if (hot[r]) {
                t->hot_mask[s] |= (uint16_t)(1u << p);
                t->index[r] = (uint16_t)(g * kL0HotGroupRows + in_rows);
                t->row[g * kL0HotGroupRows + in_rows++] = (uint16_t)r;
                ++n_hot;
            } else {
                t->index[r] = (uint16_t)(kL0ColdBit | n_cold);
                t->cold_row[n_cold++] = (uint16_t)r;
            }
        }
        ++in_sq;
    }
    for (int k = g + 1; k <= kL0HotGroups; ++k) t->sq0[k] = 90;
    for (int s = 90; s < 96; ++s) t->cold_base[s] = (uint16_t)n_cold;
    t->n_hot = (uint16_t)n_hot; t->n_cold = (uint16_t)n_cold; t->ok = fits ? 1 : 0;
}

// the process's table
inline const L0HotTable& l0_hot_table() {
    static const L0HotTable* t = [] { L0HotTable* p = new L0HotTable; l0_hot_build(p); return p; }();
    return *t;
}

}  // namespace xq
