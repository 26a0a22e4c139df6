// The range cull's slab (csrc/par_lightbox.h, the functions the light kernel runs) on the host. For every case on the
// command line -- B H bx by bz lx ly lz px py pz ex ey ez dmin dmax -- one output line: the bin's slab and its L1
// distance to the light, then the piece of it the slot record can show (or six zeros and -1 when it is empty) and that
// piece's distance. Without arguments the cases are read from standard input instead, the same sixteen integers each,
// separated by white space. tests/test_light_range_cpu.py holds the answers to a brute-force enumeration of pixel
// positions.
#include <cstdio>
#include <cstdlib>

#include "par_lightbox.h"

namespace {

constexpr int N = 16;

void answer(const int* v) {
    const par_light_slab b = par_light_slab_of(v[0], v[1], v[2], v[3], v[4]);
    std::printf("%d %d %d %d %d %d %d ", b.x0, b.x1, b.s0, b.s1, b.z0, b.z1, par_light_slab_l1(b, v[5], v[6], v[7]));
    par_light_slab c;
    if (par_light_slab_clip(b, v[8], v[9], v[10], v[11], v[12], v[13], v[14], v[15], &c)) {
        std::printf("%d %d %d %d %d %d %d\n", c.x0, c.x1, c.s0, c.s1, c.z0, c.z1, par_light_slab_l1(c, v[5], v[6], v[7]));
    } else {
        std::printf("0 0 0 0 0 0 -1\n");
    }
}

}  // namespace

int main(int argc, char** argv) {
    int v[N];
    if (argc > 1) {
        if ((argc - 1) % N != 0) return 2;
        for (int i = 1; i + N - 1 < argc; i += N) {
            for (int k = 0; k < N; k++) v[k] = std::atoi(argv[i + k]);
            answer(v);
        }
        return 0;
    }
    int k = 0;
    while (std::scanf("%d", &v[k]) == 1) {
        if (++k == N) {
            answer(v);
            k = 0;
        }
    }
    return k == 0 && std::feof(stdin) ? 0 : 2;  // (a case cut short, or something that is no integer)
}
