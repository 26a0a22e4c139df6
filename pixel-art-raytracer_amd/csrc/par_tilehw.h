// par_tilehw.h — what the two add-ons over tile hardware's bytes share, the encoder (par_vram.hip) and the decoder
// (par_screen.hip): the tile formats, a tile's bytes, the check of a map layout and the count of a launch's bad cells.
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
