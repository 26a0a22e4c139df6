// delta_check.cpp — par_tiles_apply_host (csrc/par_scene.cpp) over seeded random shapes, bin sizes, row blocks and tile
// lists, against a plain per-pixel loop, on heap buffers of exactly the size the contract names (so a sanitiser sees any
// access beyond them). Built and run by tests/test_delta_cpu.py with par_scene.cpp alone; prints
// "<checks> checks, <failures> failures".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "par_raytracer.h"

namespace {

uint64_t state = 0x243F6A8885A308D3ull;
uint64_t next() {  // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
int below(int n) { return (int)(next() % (uint64_t)n); }

long checks = 0, failures = 0;
void check(bool ok, const char* what, int w, int h, int b, int r0, int r1, int n) {
    checks++;
    if (ok) return;
    failures++;
    if (failures <= 20) std::printf("FAILED %s: %d x %d bin %d rows [%d, %d) n %d\n", what, w, h, b, r0, r1, n);
}

}  // namespace

int main() {
    const int bins[] = {8, 9, 10, 12, 16, 31, 40, 64, 160};
    for (int round = 0; round < 600; round++) {
        par_params p;
        par_default_params(&p);
        const int B = bins[below(9)];
        const int W = 1 + below(3 * B + 7), H = 1 + below(3 * B + 7);
        p.width = W;
        p.height = H;
        p.length = H;
        p.bin_size = B;
        const int gx = (W + B - 1) / B, gy = (H + B - 1) / B;
        int r0 = 0, r1 = H;
        if (round % 3 != 0) {
            r0 = below(H);
            r1 = r0 + 1 + below(H - r0);
        }
        // a list in any order, with repeats (a later slot wins), of up to twice the grid
        const int n = round % 7 == 0 ? 0 : below(2 * gx * gy + 1);
        int32_t* tiles = new int32_t[n];
        for (int i = 0; i < n; i++) tiles[i] = below(gx) | (below(gy) << 16);
        const size_t slot = (size_t)B * B;
        par_color* packed = new par_color[(size_t)n * slot];
        for (size_t i = 0; i < (size_t)n * slot; i++) {
            const uint32_t v = (uint32_t)next();
            std::memcpy(&packed[i], &v, 4);
        }
        par_color* frame = new par_color[(size_t)W * H];
        for (size_t i = 0; i < (size_t)W * H; i++) {
            const uint32_t v = (uint32_t)next();
            std::memcpy(&frame[i], &v, 4);
        }
        std::vector<par_color> expect(frame, frame + (size_t)W * H);
        for (int i = 0; i < n; i++) {
            const int bx = tiles[i] & 0xFFFF, by = tiles[i] >> 16;
            for (int y = 0; y < B; y++) {
                for (int x = 0; x < B; x++) {
                    const int col = bx * B + x, row = by * B + y;
                    if (col >= W || row >= H || row < r0 || row >= r1) continue;
                    expect[(size_t)row * W + col] = packed[(size_t)i * slot + (size_t)y * B + x];
                }
            }
        }
        const int rc = par_tiles_apply_host(&p, tiles, n, packed, r0, r1, frame);
        check(rc == PAR_OK, "status", W, H, B, r0, r1, n);
        check(std::memcmp(frame, expect.data(), (size_t)W * H * sizeof(par_color)) == 0, "frame", W, H, B, r0, r1, n);
        // one bad entry anywhere: refused, and the frame stays as it is
        if (n > 0) {
            const int at = below(n);
            const int32_t kept = tiles[at];
            tiles[at] = round % 2 ? (gx | (below(gy) << 16)) : (below(gx) | (gy << 16));
            const int rc_bad = par_tiles_apply_host(&p, tiles, n, packed, r0, r1, frame);
            check(rc_bad == PAR_ERR_INVALID_ARG, "bad entry status", W, H, B, r0, r1, n);
            check(std::memcmp(frame, expect.data(), (size_t)W * H * sizeof(par_color)) == 0, "bad entry frame", W, H, B, r0,
                  r1, n);
            tiles[at] = kept;
        }
        delete[] tiles;
        delete[] packed;
        delete[] frame;
    }
    std::printf("%ld checks, %ld failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
