// plane_tiles_check.cpp — par_plane_tiles_apply_host (csrc/par_scene.cpp) over seeded random shapes, bin sizes, row
// blocks, tile lists and the three element sizes, against a plain per-byte loop, on heap buffers of exactly the size the
// contract names (so a sanitiser sees any access beyond them) and, for 1-byte elements, at odd addresses. Built and run
// by tests/test_plane_tiles_cpu.py with par_scene.cpp alone; prints "<checks> checks, <failures> failures".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "par_raytracer.h"

namespace {

uint64_t state = 0x13198A2E03707344ull;
uint64_t next() {  // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
int below(int n) { return (int)(next() % (uint64_t)n); }

long checks = 0, failures = 0;
void check(bool ok, const char* what, int e, int w, int h, int b, int r0, int r1, int n) {
    checks++;
    if (ok) return;
    failures++;
    if (failures <= 20) std::printf("FAILED %s: E %d, %d x %d bin %d rows [%d, %d) n %d\n", what, e, w, h, b, r0, r1, n);
}

}  // namespace

int main() {
    const int bins[] = {8, 9, 10, 12, 16, 31, 40, 64, 160};
    const int sizes[] = {1, 4, 28};
    for (int round = 0; round < 900; round++) {
        par_params p;
        par_default_params(&p);
        const int E = sizes[round % 3];
        const int B = bins[below(9)];
        const int W = 1 + below(3 * B + 7), H = 1 + below(3 * B + 7);
        p.width = W;
        p.height = H;
        p.length = H;
        p.bin_size = B;
        const int gx = (W + B - 1) / B, gy = (H + B - 1) / B;
        int r0 = 0, r1 = H;
        if (round % 4 != 0) {
            r0 = below(H);
            r1 = r0 + 1 + below(H - r0);
        }
        // a list in any order, with repeats (a later slot wins), of up to twice the grid
        const int n = round % 7 == 0 ? 0 : below(2 * gx * gy + 1);
        int32_t* tiles = new int32_t[n];
        for (int i = 0; i < n; i++) tiles[i] = below(gx) | (below(gy) << 16);
        const size_t slot = (size_t)B * B * E, plane = (size_t)W * H * E;
        // 1-byte planes and slots may start on any byte: one byte into their allocation on odd rounds
        const size_t skew = E == 1 ? (size_t)((round / 3) % 2) : 0;
        unsigned char* packed_buf = new unsigned char[(size_t)n * slot + skew];
        unsigned char* frame_buf = new unsigned char[plane + skew];
        unsigned char* packed = packed_buf + skew;
        unsigned char* frame = frame_buf + skew;
        for (size_t i = 0; i < (size_t)n * slot; i++) packed[i] = (unsigned char)next();
        for (size_t i = 0; i < plane; i++) frame[i] = (unsigned char)next();
        std::vector<unsigned char> expect(frame, frame + plane);
        for (int i = 0; i < n; i++) {
            const int bx = tiles[i] & 0xFFFF, by = tiles[i] >> 16;
            for (int y = 0; y < B; y++) {
                for (int x = 0; x < B; x++) {
                    const int col = bx * B + x, row = by * B + y;
                    if (col >= W || row >= H || row < r0 || row >= r1) continue;
                    for (int k = 0; k < E; k++) {
                        expect[((size_t)row * W + col) * E + k] = packed[(size_t)i * slot + ((size_t)y * B + x) * E + k];
                    }
                }
            }
        }
        const int rc = par_plane_tiles_apply_host(&p, E, tiles, n, packed, r0, r1, frame);
        check(rc == PAR_OK, "status", E, W, H, B, r0, r1, n);
        check(std::memcmp(frame, expect.data(), plane) == 0, "frame", E, W, H, B, r0, r1, n);
        // one bad entry anywhere: refused, and the frame stays as it is
        if (n > 0) {
            const int at = below(n);
            const int32_t kept = tiles[at];
            const int kind = (round / 3) % 3;
            tiles[at] = kind == 0 ? (gx | (below(gy) << 16)) : kind == 1 ? (below(gx) | (gy << 16)) : (int32_t)(below(gx) | 0x80000000u);
            const int rc_bad = par_plane_tiles_apply_host(&p, E, tiles, n, packed, r0, r1, frame);
            check(rc_bad == PAR_ERR_INVALID_ARG, "bad entry status", E, W, H, B, r0, r1, n);
            check(std::memcmp(frame, expect.data(), plane) == 0, "bad entry frame", E, W, H, B, r0, r1, n);
            tiles[at] = kept;
            // an element size the library does not have: refused as early
            const int rc_size = par_plane_tiles_apply_host(&p, E == 1 ? 2 : E + 4, tiles, n, packed, r0, r1, frame);
            check(rc_size == PAR_ERR_INVALID_ARG, "bad size status", E, W, H, B, r0, r1, n);
            check(std::memcmp(frame, expect.data(), plane) == 0, "bad size frame", E, W, H, B, r0, r1, n);
        }
        delete[] tiles;
        delete[] packed_buf;
        delete[] frame_buf;
    }
    std::printf("%ld checks, %ld failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
