// l0hot_probe — prints the hot-row table of cn_chess_ai_amd/csrc/xq_l0hot.h as the library builds it; tests/test_l0_hot_table_cpu.py reads
// the lines.  Plain C++17, links against nothing.  One line per array: its name, then its values.
#include "../../cn_chess_ai_amd/csrc/xq_l0hot.h"

#include <cstdio>

using namespace xq;

static void line(const char* name, const uint16_t* v, int n) {
    std::printf("%s", name);
    for (int i = 0; i < n; ++i) std::printf(" %u", (unsigned)v[i]);
    std::printf("\n");
}

int main() {
    const L0HotTable& t = l0_hot_table();
    const uint16_t head[6] = {t.ok, t.n_hot, t.n_cold, (uint16_t)kL0HotGroups, (uint16_t)kL0HotGroupRows, (uint16_t)kL0HotSqB};
    line("head", head, 6);
    line("row", t.row, kL0HotGroups * kL0HotGroupRows);
    line("index", t.index, 1260);
    line("cold_row", t.cold_row, 1260);
    line("hot_mask", t.hot_mask, 96);
    line("cold_base", t.cold_base, 96);
    line("sq0", t.sq0, kL0HotGroups + 1);
    return 0;
}
