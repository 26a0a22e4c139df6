// par_tilehw.h — what the add-ons over tile hardware's bytes share, the encoder (par_vram.hip) and the decoders
// (par_screen.hip, par_objects.hip): the tile formats, a tile's bytes, the check of a map layout, the count of a launch's
// bad cells, and for the decoders the spread of a row's bits and nibbles to a byte a pixel and the widened colour word.
// It includes neither add-on's public header: the formats are its own constants, to which each unit pins its public
// enumeration with static_asserts, and the layout check is a template over the unit's own layout struct. Everything is
// in an unnamed namespace, device code __forceinline__: each unit gets its own copy and nothing is linked between the
// libraries.
#ifndef PAR_TILEHW_H
#define PAR_TILEHW_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace {

// the values of par_vram_tile_format and of par_screen_tile_format
constexpr int TILEHW_1BPP = 0, TILEHW_2BPP_PLANAR = 1, TILEHW_2BPP_ROWS = 2, TILEHW_4BPP_ROWS = 3, TILEHW_4BPP_PACKED_HI = 4,
              TILEHW_4BPP_PACKED_LO = 5, TILEHW_4BPP_ROW_PLANES = 6;

__host__ __device__ inline uint32_t bpp_of(uint32_t format) {
    return format == TILEHW_1BPP ? 1u : (format <= TILEHW_2BPP_ROWS ? 2u : 4u);
}

__host__ __device__ inline bool packed(uint32_t format) {
    return format == TILEHW_4BPP_PACKED_HI || format == TILEHW_4BPP_PACKED_LO;
}

// the byte of a sub-tile that holds bit plane b of row y (the planar formats)
__device__ __forceinline__ uint32_t plane_byte(uint32_t format, uint32_t b, uint32_t y) {
    switch (format) {
        case TILEHW_2BPP_PLANAR: return 8 * b + y;
        case TILEHW_2BPP_ROWS: return 2 * y + b;
        case TILEHW_4BPP_ROWS: return 16 * (b >> 1) + 2 * y + (b & 1);
        case TILEHW_4BPP_ROW_PLANES: return 4 * y + b;
        default: return y;
    }
}

// the values of par_screen_palette_format and of par_objects_palette_format
constexpr uint32_t TILEHW_BGR555 = 0, TILEHW_BGR333_MD = 1, TILEHW_BGR222 = 2, TILEHW_RGBA8 = 3;

// bit 7 - k of `byte` as byte k of the result, 0 or 1
__device__ __forceinline__ uint64_t spread_bits(uint32_t byte) {
    const uint64_t picked = ((uint64_t)byte * 0x0101010101010101ull) & 0x0102040810204080ull;
    return ((picked + 0x7F7F7F7F7F7F7F7Full) >> 7) & 0x0101010101010101ull;
}

// byte m of `x` as byte 2 m of the result
__device__ __forceinline__ uint64_t spread_bytes(uint32_t x) {
    uint64_t v = x;
    v = (v | v << 16) & 0x0000FFFF0000FFFFull;
    return (v | v << 8) & 0x00FF00FF00FF00FFull;
}

// an entry of `pal_words` widened: red | green << 8 | blue << 16 | 255 << 24 (the kernels' and par_screen_palette_rgba's)
__host__ __device__ __forceinline__ uint32_t widen(const uint8_t* pal_words, uint32_t format, uint32_t i) {
    uint32_t r, g, b;
    if (format == TILEHW_RGBA8) {
        r = pal_words[4 * i], g = pal_words[4 * i + 1], b = pal_words[4 * i + 2];
    } else if (format == TILEHW_BGR555) {
        const uint32_t w = pal_words[2 * i] | (uint32_t)pal_words[2 * i + 1] << 8;
        const uint32_t qr = w & 31u, qg = (w >> 5) & 31u, qb = (w >> 10) & 31u;
        r = qr << 3 | qr >> 2, g = qg << 3 | qg >> 2, b = qb << 3 | qb >> 2;
    } else if (format == TILEHW_BGR333_MD) {
        const uint32_t w = (uint32_t)pal_words[2 * i] << 8 | pal_words[2 * i + 1];
        const uint32_t qr = (w >> 1) & 7u, qg = (w >> 5) & 7u, qb = (w >> 9) & 7u;
        r = qr << 5 | qr << 2 | qr >> 1, g = qg << 5 | qg << 2 | qg >> 1, b = qb << 5 | qb << 2 | qb >> 1;
    } else {
        const uint32_t w = pal_words[i];
        r = (w & 3u) * 0x55u, g = ((w >> 2) & 3u) * 0x55u, b = ((w >> 4) & 3u) * 0x55u;
    }
    return r | g << 8 | b << 16 | 0xFF000000u;
}

// The workgroup's bad cells in one atomic; every thread of a workgroup of WAVES wavefronts calls it.
template <uint32_t WAVES>
__device__ __forceinline__ void add_bad(bool bad, uint32_t* bad_out) {
    __shared__ uint32_t bad_of[WAVES];
    const uint32_t in_wave = (uint32_t)__popcll(__ballot(bad));
    if ((threadIdx.x & 63u) == 0) bad_of[threadIdx.x >> 6] = in_wave;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (uint32_t w = 0; w < WAVES; w++) total += bad_of[w];
        if (total) atomicAdd(bad_out, total);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

inline bool tile_dim_ok(int d) { return d == 8 || d == 16; }
inline bool format_ok(int format) { return format >= TILEHW_1BPP && format <= TILEHW_4BPP_ROW_PLANES; }
inline bool pal_format_ok(int format) { return format >= (int)TILEHW_BGR555 && format <= (int)TILEHW_RGBA8; }
inline size_t pal_entry_bytes(int format) { return format == (int)TILEHW_RGBA8 ? 4 : (format == (int)TILEHW_BGR222 ? 1 : 2); }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline uint32_t log2_of(int d) { return d == 8 ? 3u : (d == 16 ? 4u : (d == 2 ? 1u : 0u)); }

// the bytes of a tile, 0 for a format or a size that does not exist
inline size_t tile_bytes_of(int format, int tile_w, int tile_h) {
    if (!format_ok(format) || !tile_dim_ok(tile_w) || !tile_dim_ok(tile_h)) return 0;
    return (size_t)(8 * bpp_of((uint32_t)format)) * (size_t)(tile_w / 8) * (size_t)(tile_h / 8);
}

// Layout: par_vram_map_layout or par_screen_map_layout, field for field the same
template <class Layout>
bool layout_ok(const Layout* L) {
    if (L->word_bytes != 1 && L->word_bytes != 2 && L->word_bytes != 4) return false;
    const int bits = 8 * L->word_bytes;
    if (L->big_endian != 0 && L->big_endian != 1) return false;
    if (L->tile_bits < 1 || L->tile_shift < 0 || L->tile_bits > bits || L->tile_shift > bits - L->tile_bits) return false;
    if (L->pal_bits < 0 || L->pal_shift < 0 || L->pal_bits > bits || L->pal_shift > bits - L->pal_bits) return false;
    if (L->flip_x_bit < -1 || L->flip_x_bit >= bits || L->flip_y_bit < -1 || L->flip_y_bit >= bits) return false;
    if (L->tile_step < 1 || L->tile_step > 16 || L->tile_base < 0 || L->tile_base > 65535) return false;
    return bits == 32 || ((uint32_t)L->set_bits >> bits) == 0;
}

// the four-byte fill behind which a call counts into bad_out
inline hipError_t zero_bad(hipStream_t stream, uint32_t* bad_out) {
    return bad_out ? hipMemsetAsync(bad_out, 0, sizeof(uint32_t), stream) : hipSuccess;
}

}  // namespace

#endif
