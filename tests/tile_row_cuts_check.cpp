// tile_row_cuts_check.cpp — par_tile_row_cuts (csrc/par_hostcall.h), the cut of a call's rows into launches that
// par_outline_device and par_finish_device share: for each case the launches partition [row_begin, row_end) in order
// without gap or overlap, every launch but the last covers whole tile rows, no launch has more than 65535 tile rows, and
// a launch of more than one tile row has at most 0x7FFFFFF0 pixels. Built without HIP and run by
// tests/test_finish_cpu.py; prints "<checks> checks, <failures> failures".
#include <cstdint>
#include <cstdio>

#include "par_hostcall.h"

namespace {

constexpr uint32_t TILE_H = 16;
long checks = 0, failures = 0;

void check(bool ok, const char* what, const char* tag, int ra, int rb) {
    checks++;
    if (ok) return;
    failures++;
    if (failures <= 20) std::printf("FAILED %s: %s at launch [%d, %d)\n", tag, what, ra, rb);
}

// the number of launches, or -1 after the walk was ended from within
int run(const char* tag, int row_begin, int row_end, uint32_t W, int stop_after = 0) {
    int next = row_begin, launches = 0;
    const int status = par_tile_row_cuts(row_begin, row_end, W, TILE_H, [&](int ra, int rb, uint32_t tile_rows) {
        launches++;
        check(ra == next, "a gap or an overlap", tag, ra, rb);
        check(ra < rb && rb <= row_end, "an empty launch or one past the end", tag, ra, rb);
        check(tile_rows == ((uint32_t)(rb - ra) + TILE_H - 1) / TILE_H, "tile_rows is not the launch's", tag, ra, rb);
        check(rb == row_end || (uint32_t)(rb - ra) % TILE_H == 0, "a cut inside a tile row", tag, ra, rb);
        check(tile_rows >= 1 && tile_rows <= 65535u, "the grid's y extent", tag, ra, rb);
        check(tile_rows == 1 || (uint64_t)tile_rows * TILE_H * W <= 0x7FFFFFF0ull, "the pixels of a launch", tag, ra, rb);
        next = rb;
        return launches == stop_after ? 7 : 0;
    });
    if (stop_after) {
        check(status == 7 && launches == stop_after, "the first status that is not 0 ends the walk", tag, row_begin, next);
        return -1;
    }
    check(status == 0 && next == row_end, "the launches do not end at row_end", tag, row_begin, row_end);
    return launches;
}

}  // namespace

int main() {
    // cut by the grid's y extent
    check(run("W 1, 65535 * 16 + 1 rows", 0, 65535 * 16 + 1, 1u) == 2, "launches", "W 1", 0, 0);
    // one tile row alone exceeds the pixel cap and is still not cut further
    check(run("W 2^27, 40 rows", 0, 40, 1u << 27) == 3, "launches", "W 2^27", 0, 0);
    // cut by pixels: 2^31 / 2^20 / 16 = 128 tile rows would be 2^31 pixels, so 127 a launch
    check(run("W 2^20, 4096 rows", 0, 4096, 1u << 20) == 3, "launches", "W 2^20", 0, 0);
    check(run("rows [5, 6)", 5, 6, 640u) == 1, "launches", "rows [5, 6)", 5, 6);
    // a range that ends exactly on a cut, from a row_begin that is no multiple of the tile height
    check(run("ends on a cut", 3, 3 + 2 * 127 * 16, 1u << 20) == 2, "launches", "ends on a cut", 0, 0);
    check(run("ends on a cut by y", 0, 65535 * 16, 1u) == 1, "launches", "ends on a cut by y", 0, 0);
    check(run("no rows", 9, 9, 640u) == 0, "launches", "no rows", 9, 9);
    // a launch's status that is not 0 ends the walk and is what the walk returns
    run("stopped", 0, 4096, 1u << 20, 2);
    std::printf("%ld checks, %ld failures\n", checks, failures);
    return failures ? 1 : 0;
}
