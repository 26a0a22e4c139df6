// par_post.h — the per-pixel arithmetic of the passes over finished planes, one implementation per contract: the
// outline pass's (par_outline.hip), the palette pass's (par_quantize.hip) and the present pass's (par_present.hip), shared
// with the kernel that runs the three in one launch (par_finish.hip), and the scalers' rules (par_upscale.hip, which takes
// the present pass's exchange from here too). Everything here is __forceinline__ device code in
// an unnamed namespace: each unit gets its own copy, inlined where it is called.
#ifndef PAR_POST_H
#define PAR_POST_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace {

// ---- outlines ------------------------------------------------------------------------------------------------------

// What a pixel's class needs of a texel.
struct Texel {
    bool covered;
    uint32_t key, entity, n0, n1, n2;
};

__device__ __forceinline__ Texel texel_at(const uint32_t* w, uint32_t background) {
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4], w5 = w[5], w6 = w[6];
    Texel t;
    t.covered = (w0 | w1 | w2 | (w3 ^ background) | w4 | w5 | w6) != 0;
    t.key = w4 - w5;
    t.entity = w6;
    t.n0 = w0; t.n1 = w1; t.n2 = w2;
    return t;
}

// (bitwise operators on purpose in these two: nothing here is worth a branch)
// `t` (covered) meets the silhouette condition against its present neighbour `n`
__device__ __forceinline__ int silhouette_against(const Texel& t, const Texel& n, int depth_step) {
    return (int)!n.covered | ((int)(n.entity != t.entity) & (int)((int32_t)(t.key - n.key) >= depth_step));
}

// the right or down neighbour `n` of `t` (covered) makes `t` a crease
__device__ __forceinline__ int crease_with(const Texel& t, const Texel& n, int present, int depth_step) {
    return present & (int)n.covered & (1 ^ silhouette_against(n, t, depth_step)) &
           (int)(((n.n0 ^ t.n0) | (n.n1 ^ t.n1) | (n.n2 ^ t.n2)) != 0u);
}

__device__ __forceinline__ uint32_t scaled(uint32_t px, int s) {
    const uint32_t r = std::min(255u, ((px & 0xFFu) * (uint32_t)s) >> 8);
    const uint32_t g = std::min(255u, (((px >> 8) & 0xFFu) * (uint32_t)s) >> 8);
    const uint32_t b = std::min(255u, (((px >> 16) & 0xFFu) * (uint32_t)s) >> 8);
    return r | (g << 8) | (b << 16) | (px & 0xFF000000u);
}

// ---- palette output ------------------------------------------------------------------------------------------------

constexpr uint32_t QUANT_RGB = 0x00FFFFFFu;  // red, green, blue of a par_color read as one little-endian word

// The 4x4 Bayer matrix of the contract, B4[y & 3][x & 3], as sixteen nibbles: entry (y, x) at bit 4 * (4 * y + x).
constexpr int BAYER4[4][4] = {{0, 8, 2, 10}, {12, 4, 14, 6}, {3, 11, 1, 9}, {15, 7, 13, 5}};
constexpr uint64_t bayer_nibbles() {
    uint64_t v = 0;
    for (int y = 0; y < 4; y++) {
        for (int x = 0; x < 4; x++) v |= (uint64_t)BAYER4[y][x] << (4 * (4 * y + x));
    }
    return v;
}
constexpr uint64_t BAYER_NIBBLES = bayer_nibbles();

// c' = min(255, max(0, c + off)) on the three colour channels; the alpha byte of the result is 0.
__device__ __forceinline__ uint32_t dithered(uint32_t px, uint32_t x, uint32_t y, int spread) {
    const int t = (int)((BAYER_NIBBLES >> (((y & 3u) << 4) | ((x & 3u) << 2))) & 15u);
    const int off = ((2 * t - 15) * spread) >> 5;  // floor: an arithmetic shift rounds towards minus infinity
    const int r = std::min(255, std::max(0, (int)(px & 0xFFu) + off));
    const int g = std::min(255, std::max(0, (int)((px >> 8) & 0xFFu) + off));
    const int b = std::min(255, std::max(0, (int)((px >> 16) & 0xFFu) + off));
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}

__device__ __forceinline__ uint32_t min3u(uint32_t a, uint32_t b, uint32_t c) { return std::min(std::min(a, b), c); }

// ---- present -------------------------------------------------------------------------------------------------------

// red and blue of a par_color read as one little-endian word exchanged
__device__ __forceinline__ uint32_t exchanged(uint32_t c) {
    return (c & 0xFF00FF00u) | ((c & 0xFFu) << 16) | ((c >> 16) & 0xFFu);
}

// ---- upscale -------------------------------------------------------------------------------------------------------

// The neighbourhood of E is A B C / D E F / G H I, every element one word; two elements are equal iff their words are.
// (bitwise operators on purpose, as above: a rule is a handful of compares and one select)

// Scale2x: the 2 x 2 block of E, row by row
__device__ __forceinline__ void scale2x_block(uint32_t B, uint32_t D, uint32_t E, uint32_t F, uint32_t H, uint32_t o[4]) {
    const bool g = (B != H) & (D != F);
    o[0] = (g & (D == B)) ? D : E;
    o[1] = (g & (B == F)) ? F : E;
    o[2] = (g & (D == H)) ? D : E;
    o[3] = (g & (H == F)) ? F : E;
}

// Scale3x: the 3 x 3 block of E, row by row
__device__ __forceinline__ void scale3x_block(uint32_t A, uint32_t B, uint32_t C, uint32_t D, uint32_t E, uint32_t F,
                                              uint32_t G, uint32_t H, uint32_t I, uint32_t o[9]) {
    const bool g = (B != H) & (D != F);
    const bool db = g & (D == B), bf = g & (B == F), dh = g & (D == H), hf = g & (H == F);
    o[0] = db ? D : E;
    o[1] = ((db & (E != C)) | (bf & (E != A))) ? B : E;
    o[2] = bf ? F : E;
    o[3] = ((db & (E != G)) | (dh & (E != A))) ? D : E;
    o[4] = E;
    o[5] = ((bf & (E != I)) | (hf & (E != C))) ? F : E;
    o[6] = dh ? D : E;
    o[7] = ((dh & (E != I)) | (hf & (E != G))) ? H : E;
    o[8] = hf ? F : E;
}

}  // namespace

#endif
