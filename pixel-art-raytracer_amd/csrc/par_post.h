// par_post.h — what the passes over finished planes share, one implementation per contract: the outline pass's texel
// arithmetic and its tile geometry (par_outline.hip), the palette pass's dither (par_quantize.hip) and the present
// pass's exchange, palette entry and group expand (par_present.hip), shared with the kernel that runs the three in one
// launch (par_finish.hip), the scalers' rules (par_upscale.hip, which takes the present pass's exchange and palette
// entry from here too), and the tally of a palette refine round (par_palette.hip and the fitted-cells add-on,
// par_cells_fit.hip). Everything here is __forceinline__ device code in an unnamed namespace: each unit gets its own
// copy, inlined where it is called. (The staged tile's loads, stores and classification and the palette search are NOT
// here: as functions they are simplified on their own before they are inlined and came out as other, slower code in
// outline_kernel, finish_kernel and quantize_kernel; those kernels keep them in their bodies.)
#ifndef PAR_POST_H
#define PAR_POST_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_fastdiv.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

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

// The tile of outline_kernel and finish_kernel: a workgroup of OUTLINE_THREADS takes OUTLINE_TILE_W x OUTLINE_TILE_H
// pixels and stages the tile's texels plus a one-texel halo into LDS as they lie in memory, seven dwords a texel; a
// wavefront then classifies four consecutive tile rows (outline_kernel's description in par_outline.hip).
constexpr int OUTLINE_TILE_W = 64;   // one wavefront's lanes
constexpr int OUTLINE_TILE_H = 16;   // four wavefronts x four rows
constexpr int OUTLINE_THREADS = 256;
constexpr int OUTLINE_WAVES = OUTLINE_THREADS / 64;
constexpr int OUTLINE_ROWS_PER_WAVE = OUTLINE_TILE_H / OUTLINE_WAVES;
constexpr int TEXEL_DWORDS = 7;
constexpr int STAGED_W = OUTLINE_TILE_W + 2, STAGED_H = OUTLINE_TILE_H + 2;
// dwords between staged rows: a row's 462 dwords, its phase shift of at most 3, rounded up to whole 16-byte units
constexpr int STAGED_PITCH = (STAGED_W * TEXEL_DWORDS + 3 + 3) / 4 * 4;
constexpr int UNITS_PER_ROW = (STAGED_W * TEXEL_DWORDS + 3 + 3) / 4;  // 16-byte units a row's run can touch
constexpr int UNIT_ROUNDS = (UNITS_PER_ROW + 63) / 64;
constexpr int STAGE_ROUNDS = (STAGED_H + OUTLINE_WAVES - 1) / OUTLINE_WAVES;
static_assert(OUTLINE_TILE_W == 64 && OUTLINE_ROWS_PER_WAVE == 4,
              "a wavefront classifies 4 rows x 64 columns; outline_kernel's vector outputs deal 4 rows x 16 lanes");
static_assert(STAGED_PITCH % 4 == 0 && UNITS_PER_ROW * 4 <= STAGED_PITCH, "a staged row stays inside its pitch");

// The shift (0..3 dwords) of the staged row of the tile at column tx0 that holds absolute row r: with it the LDS index
// of a texel's dword is congruent, modulo 4, to its dword address in memory (7 = -1 modulo 4). `a` is the kernel's
// argument struct (its g0 and width), `galign` the plane's first dword within its 16-byte line.
template <class Args>
__device__ __forceinline__ uint32_t row_shift(const Args& a, uint32_t galign, int r, uint32_t tx0) {
    return (galign - (uint32_t)(r - a.g0) * a.width - tx0 + 1u) & 3u;
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

// ---- palette refine ------------------------------------------------------------------------------------------------

constexpr uint32_t HIGH_NIBBLES = 0x00F0F0F0u;  // of red, green and blue in a par_color's word

// `n` pixels of entry k and colour rgb into the tallies t of a stage, 3 x 16 dwords an entry: every channel's high
// nibble, or (LO) the low nibble of the channels whose high nibble is the one chosen for (k, channel), high[k].
// (par_palette.hip's refine rounds and par_cells_fit.hip's, whose medians are the same by contract)
template <bool LO>
__device__ __forceinline__ void tally_add(uint32_t* t, const uint32_t* high, uint32_t k, uint32_t rgb, uint32_t n) {
    uint32_t* const row = t + k * 48u;
    if (LO) {
        const uint32_t other = (rgb ^ high[k]) & HIGH_NIBBLES;
        for (int c = 0; c < 3; c++) {
            if (((other >> (8 * c)) & 0xFFu) == 0u) atomicAdd(&row[16 * c + ((rgb >> (8 * c)) & 15u)], n);
        }
    } else {
        for (int c = 0; c < 3; c++) atomicAdd(&row[16 * c + ((rgb >> (8 * c + 4)) & 15u)], n);
    }
}

// ---- present -------------------------------------------------------------------------------------------------------

// red and blue of a par_color read as one little-endian word exchanged
__device__ __forceinline__ uint32_t exchanged(uint32_t c) {
    return (c & 0xFF00FF00u) | ((c & 0xFFu) << 16) | ((c >> 16) & 0xFFu);
}

// This thread's entry of a palette a workgroup of PAR_MAX_PALETTE threads holds in LDS: entry i is
// palette[min(i, n_colors - 1)] (an index never exceeds n_colors - 1: the clamp only keeps the load inside the palette)
// in the surface's byte order, so the clamp and the exchange are paid once per workgroup. (The load alone is for the
// kernel that issues it behind other loads and wants the exchange, which waits for it, behind them too.)
__device__ __forceinline__ uint32_t palette_entry_load(const uint32_t* palette, int n_colors) {
    return palette[std::min<uint32_t>(threadIdx.x, (uint32_t)n_colors - 1u)];
}
__device__ __forceinline__ uint32_t palette_entry(const uint32_t* palette, int n_colors, bool swap) {
    const uint32_t e = palette_entry_load(palette, n_colors);
    return swap ? exchanged(e) : e;
}

// The source columns of a group of four output pixels of one source row, the first at output column `first`: of pixel 0
// by division by the scale sx, of the others by stepping. A column never exceeds `last`: a pixel past the row's end
// takes the last column, so that every load stays inside the row, and is not stored.
__device__ __forceinline__ void group_columns(uint32_t first, uint32_t sx, par_udiv31 by_sx, uint32_t last,
                                              uint32_t at[4]) {
    at[0] = par_udiv31_quotient(first, by_sx);
    uint32_t rem = first - at[0] * sx;
    for (int i = 1; i < 4; i++) {
        const bool step = ++rem == sx;
        rem = step ? 0u : rem;
        at[i] = std::min(at[i - 1] + (step ? 1u : 0u), last);
    }
}

// The group's four words c[] to the sy output rows of its source row, `pitch` bytes apart from `dst` on: 16 bytes a row
// where `dst` and the pitch are on 16-byte boundaries (VEC) and the group lies inside the row's out_width pixels (`full`,
// base + 4 <= out_width), else pixel by pixel. `base` is the group's first output column.
template <bool VEC>
__device__ __forceinline__ void store_group(char* dst, const uint32_t c[4], bool full, uint32_t base, uint32_t out_width,
                                            uint32_t sy, size_t pitch) {
    if (VEC && full) {
        const u32x4 v = {c[0], c[1], c[2], c[3]};
        for (uint32_t y = 0; y < sy; y++) *reinterpret_cast<u32x4*>(dst + y * pitch) = v;
    } else {
        for (uint32_t y = 0; y < sy; y++) {
            uint32_t* const o = reinterpret_cast<uint32_t*>(dst + y * pitch);
            for (int i = 0; i < 4; i++) {
                if (base + i < out_width) o[i] = c[i];
            }
        }
    }
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
