// par_screen.hip — the screen add-on (libpar_screen.so): one background layer drawn from VRAM bytes, and map words read
// back into the project's tile map. The contract is beside the declarations in addons/include/par_screen.h; nothing here
// knows a par_context or a par_params, and nothing here is linked into libpar_raytracer.so or libpar_vram.so.
//
// Every device call is one launch, behind one four-byte fill where it counts into a bad_out:
//   draw    a thread takes one eight-pixel segment of a tile row IN MAP SPACE on one screen row: the map's width in pixels
//           is a multiple of eight, so a segment never crosses a cell, a sub-tile or the wrap seam, and one map word and
//           bpp row bytes (four for the packed formats) give its eight values at once: a planar byte is spread to a bit a
//           byte by one multiplication, a packed word to a nibble a byte by two shifts, an x flip is a byte swap. The row's
//           first segment starts (scroll phase) pixels left of the screen; a row has (width + 14) / 8 segment slots, the
//           most a phase needs, and a slot beyond the row's last does nothing. A segment wholly on the screen is stored as
//           two 16-byte words of fb_out and one 8-byte word of index_out where the addresses allow, else in dwords and
//           bytes; a clipped one pixel by pixel. The palette is widened to RGBA8 once a workgroup, into LDS. The first
//           map_w * map_h threads of the launch also judge one cell each, and a workgroup adds its bad cells in one atomic.
//   decode  a thread a cell; the bad cells of a workgroup in one atomic
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_hostcall.h"
#include "par_screen.h"
#include "par_tilehw.h"

namespace {

constexpr uint32_t SC_THREADS = 256;
constexpr uint32_t SC_WAVES = SC_THREADS / 64;
constexpr uint32_t SC_ID_LIMIT = 1u << 30;

// par_tilehw.h's formats are par_screen_tile_format's
static_assert(PAR_SCREEN_1BPP == TILEHW_1BPP);
static_assert(PAR_SCREEN_2BPP_PLANAR == TILEHW_2BPP_PLANAR);
static_assert(PAR_SCREEN_2BPP_ROWS == TILEHW_2BPP_ROWS);
static_assert(PAR_SCREEN_4BPP_ROWS == TILEHW_4BPP_ROWS);
static_assert(PAR_SCREEN_4BPP_PACKED_HI == TILEHW_4BPP_PACKED_HI);
static_assert(PAR_SCREEN_4BPP_PACKED_LO == TILEHW_4BPP_PACKED_LO);
static_assert(PAR_SCREEN_4BPP_ROW_PLANES == TILEHW_4BPP_ROW_PLANES);
// and its colour words (spread_bits, spread_bytes and widen live there, one copy with par_objects.hip) par_screen_palette_format's
static_assert(PAR_SCREEN_BGR555 == TILEHW_BGR555 && PAR_SCREEN_BGR333_MD == TILEHW_BGR333_MD);
static_assert(PAR_SCREEN_BGR222 == TILEHW_BGR222 && PAR_SCREEN_RGBA8 == TILEHW_RGBA8);

// what the kernels need of a layout, as unsigned fields
struct word_layout {
    uint32_t word_bytes, big_endian, tile_shift, tile_mask, pal_shift, pal_mask, tile_step, tile_base;
    int32_t flip_x_bit, flip_y_bit;
};

struct map_cell {
    uint32_t id, p, fx, fy;
    bool bad;
};

// cell c's word taken apart; `limit` is the first id that is bad
__device__ __forceinline__ map_cell read_cell(const word_layout& L, const uint8_t* map_words, uint32_t c, uint32_t limit) {
    const uint8_t* at = map_words + (size_t)c * L.word_bytes;
    uint32_t w = 0;
    for (uint32_t k = 0; k < L.word_bytes; k++) w |= (uint32_t)at[k] << (8 * (L.big_endian ? L.word_bytes - 1 - k : k));
    const uint32_t t = (w >> L.tile_shift) & L.tile_mask;
    map_cell cell;
    cell.p = (w >> L.pal_shift) & L.pal_mask;
    cell.fx = L.flip_x_bit >= 0 ? (w >> L.flip_x_bit) & 1u : 0u;
    cell.fy = L.flip_y_bit >= 0 ? (w >> L.flip_y_bit) & 1u : 0u;
    const uint32_t above = t - L.tile_base;  // (meaningless when t < tile_base, which is bad)
    cell.id = L.tile_step == 1 ? above : above / L.tile_step;
    cell.bad = t < L.tile_base || cell.id * L.tile_step != above || cell.id >= limit;
    return cell;
}

struct draw_args {
    word_layout L;
    uint32_t lw, lh;          // the binary logarithms of the tile's width and height (3 or 4)
    uint32_t format, n_tiles, tile_bytes;
    uint32_t map_w, n_cells;
    uint32_t period_x, period_y;  // the map in pixels
    uint32_t rxs, rys, ccx;   // the logarithms of the ratios, the colour cells a row of `attr`
    uint32_t pal_format, n_colors, sub_size, backdrop;
    uint32_t width, height, slots;  // slots: the segment slots a row
    uint32_t scroll_x, scroll_y;    // reduced into [0, period)
};

// floor(v mod period) for any int32 v and a period below 2^25
__device__ __forceinline__ uint32_t floor_mod(int32_t v, uint32_t period) {
    const int32_t r = v % (int32_t)period;
    return (uint32_t)(r < 0 ? r + (int32_t)period : r);
}

__global__ __launch_bounds__(SC_THREADS) void draw_kernel(draw_args A, const uint8_t* chr, const uint8_t* map_words,
                                                          const uint8_t* attr, const uint8_t* pal_words, const int32_t* line_scroll,
                                                          uint8_t* fb_out, uint8_t* index_out, uint32_t* bad_out) {
    __shared__ uint32_t colours[256];
    const uint32_t gid = blockIdx.x * SC_THREADS + threadIdx.x;
    if (fb_out) {  // (the same for every thread of the launch)
        if (threadIdx.x < A.n_colors) colours[threadIdx.x] = widen(pal_words, A.pal_format, threadIdx.x);
        __syncthreads();
    }
    if (bad_out) add_bad<SC_WAVES>(gid < A.n_cells && read_cell(A.L, map_words, gid, A.n_tiles).bad, bad_out);

    const uint32_t y = gid / A.slots, slot = gid - y * A.slots;
    if (y >= A.height) return;
    uint32_t sx = A.scroll_x, sy = A.scroll_y + y;  // (y < 4096 and a scroll below its period, which is at most 2^24)
    if (line_scroll) {
        sx += floor_mod(line_scroll[2 * y], A.period_x);
        sy += floor_mod(line_scroll[2 * y + 1], A.period_y);
    }
    // the row's first segment starts `phase` pixels left of the screen
    const uint32_t phase = sx & 7u;
    const int32_t x0 = (int32_t)(8 * slot) - (int32_t)phase;
    if (x0 >= (int32_t)A.width) return;
    const uint32_t mx = (sx - phase + 8 * slot) % A.period_x, my = sy % A.period_y;  // (sums below 2^26)
    const uint32_t cx = mx >> A.lw, cy = my >> A.lh;
    map_cell cell = read_cell(A.L, map_words, cx + cy * A.map_w, A.n_tiles);
    if (attr) cell.p = attr[(cx >> A.rxs) + (cy >> A.rys) * A.ccx];

    uint64_t values = 0;  // byte k: the value of the segment's pixel k, left to right on the screen
    if (!cell.bad) {
        const uint32_t tw = 1u << A.lw, th = 1u << A.lh;
        const uint32_t in_x = mx & (tw - 1u), in_y = my & (th - 1u);      // the segment's left end in the tile, and the row
        const uint32_t px = cell.fx ? tw - 8u - in_x : in_x, py = cell.fy ? th - 1u - in_y : in_y;  // as stored
        const uint32_t sub = (py >> 3) * (tw >> 3) + (px >> 3), row = py & 7u, bpp = bpp_of(A.format);
        const uint8_t* d = chr + (size_t)cell.id * A.tile_bytes + (size_t)sub * (8 * bpp);
        if (packed(A.format)) {
            const uint8_t* q = d + 4 * row;
            const uint32_t w = q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
            const uint32_t high = (w >> 4) & 0x0F0F0F0Fu, low = w & 0x0F0F0F0Fu;
            values = A.format == PAR_SCREEN_4BPP_PACKED_HI ? spread_bytes(high) | spread_bytes(low) << 8
                                                           : spread_bytes(low) | spread_bytes(high) << 8;
        } else {
            for (uint32_t b = 0; b < bpp; b++) values |= spread_bits(d[plane_byte(A.format, b, row)]) << b;
        }
        if (cell.fx) values = __builtin_bswap64(values);
    }

    // (p is up to 32 bits wide: p * K is cut at 255, which n_colors - 1 never exceeds, so the clamp below sees no difference)
    const uint32_t base = (uint32_t)std::min<uint64_t>((uint64_t)cell.p * A.sub_size, 255u), last = A.n_colors - 1u;
    uint64_t indices = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
        const uint32_t v = (uint32_t)(values >> (8 * k)) & 0xFFu;
        uint32_t i = std::min(base + v, last);
        if (cell.bad || (A.backdrop && v == 0)) i = 0;
        indices |= (uint64_t)i << (8 * k);
    }

    const size_t row_at = (size_t)y * A.width;
    if (x0 >= 0 && x0 + 8 <= (int32_t)A.width) {
        const size_t at = row_at + (size_t)x0;
        if (index_out) {
            uint8_t* o = index_out + at;
            if ((reinterpret_cast<uintptr_t>(o) & 7u) == 0) {
                *reinterpret_cast<uint64_t*>(o) = indices;
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) o[k] = (uint8_t)(indices >> (8 * k));
            }
        }
        if (fb_out) {
            uint32_t c[8];
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) c[k] = colours[(uint32_t)(indices >> (8 * k)) & 0xFFu];
            uint32_t* o = reinterpret_cast<uint32_t*>(fb_out) + at;
            if ((reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
                reinterpret_cast<uint4*>(o)[0] = make_uint4(c[0], c[1], c[2], c[3]);
                reinterpret_cast<uint4*>(o)[1] = make_uint4(c[4], c[5], c[6], c[7]);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) o[k] = c[k];
            }
        }
        return;
    }
    for (uint32_t k = 0; k < 8; k++) {
        const int32_t x = x0 + (int32_t)k;
        if (x < 0 || x >= (int32_t)A.width) continue;
        const uint32_t i = (uint32_t)(indices >> (8 * k)) & 0xFFu;
        if (index_out) index_out[row_at + (size_t)x] = (uint8_t)i;
        if (fb_out) reinterpret_cast<uint32_t*>(fb_out)[row_at + (size_t)x] = colours[i];
    }
}

__global__ __launch_bounds__(SC_THREADS) void decode_map_kernel(word_layout L, const uint8_t* map_words, uint32_t n,
                                                                uint32_t* map_out, uint8_t* pal_out, uint32_t* bad_out) {
    const uint32_t c = blockIdx.x * SC_THREADS + threadIdx.x;
    bool bad = false;
    if (c < n) {
        const map_cell cell = read_cell(L, map_words, c, SC_ID_LIMIT);
        bad = cell.bad;
        map_out[c] = (bad ? 0u : cell.id) | cell.fx << 30 | cell.fy << 31;
        if (pal_out) pal_out[c] = (uint8_t)cell.p;
    }
    if (bad_out) add_bad<SC_WAVES>(bad, bad_out);  // (the same for every lane of the launch)
}

// ---- host side ---------------------------------------------------------------------------------------------------------

word_layout words_of(const par_screen_map_layout* L) {
    word_layout W;
    W.word_bytes = (uint32_t)L->word_bytes, W.big_endian = (uint32_t)L->big_endian;
    // a shift of the whole word leaves nothing (pal_bits 0 at pal_shift 32): shift 0 under mask 0 says the same
    W.tile_shift = (uint32_t)L->tile_shift, W.tile_mask = (uint32_t)((1ull << L->tile_bits) - 1u);
    W.pal_mask = (uint32_t)((1ull << L->pal_bits) - 1u), W.pal_shift = W.pal_mask ? (uint32_t)L->pal_shift : 0u;
    W.tile_step = (uint32_t)L->tile_step, W.tile_base = (uint32_t)L->tile_base;
    W.flip_x_bit = L->flip_x_bit, W.flip_y_bit = L->flip_y_bit;
    return W;
}

bool draw_args_ok(const par_screen_desc* d, const uint8_t* chr, const uint8_t* map_words, const uint8_t* pal_words,
                  const int32_t* line_scroll, const uint8_t* fb_out, const uint8_t* index_out) {
    if (!d || !chr || !map_words || (!fb_out && !index_out) || (fb_out && !pal_words)) return false;
    if (!aligned4(line_scroll) || !aligned4(fb_out)) return false;
    if (!layout_ok(&d->layout) || !tile_dim_ok(d->tile_w) || !tile_dim_ok(d->tile_h) || !format_ok(d->tile_format)) return false;
    if (d->n_tiles < 1 || d->n_tiles > PAR_SCREEN_MAX_TILES || d->map_w < 1 || d->map_h < 1) return false;
    if ((int64_t)d->map_w * (int64_t)d->map_h > PAR_SCREEN_MAX_CELLS) return false;
    if ((d->ratio_x != 1 && d->ratio_x != 2) || (d->ratio_y != 1 && d->ratio_y != 2)) return false;
    if (!pal_format_ok(d->pal_format) || d->n_colors < 1 || d->n_colors > 256 || d->sub_size < 1 || d->sub_size > 256) return false;
    if (d->backdrop != 0 && d->backdrop != 1) return false;
    return d->width >= 1 && d->width <= PAR_SCREEN_MAX_SIDE && d->height >= 1 && d->height <= PAR_SCREEN_MAX_SIDE;
}

bool decode_args_ok(const par_screen_map_layout* layout, const uint8_t* map_words, int n_cells, const uint32_t* map_out) {
    return layout && map_words && map_out && aligned4(map_out) && n_cells >= 1 && n_cells <= PAR_SCREEN_MAX_CELLS && layout_ok(layout);
}

uint32_t floor_mod_host(int32_t v, uint32_t period) {
    const int64_t r = (int64_t)v % (int64_t)period;
    return (uint32_t)(r < 0 ? r + (int64_t)period : r);
}

hipError_t launch_draw(hipStream_t stream, const par_screen_desc* d, const uint8_t* chr, const uint8_t* map_words, const uint8_t* attr,
                       const uint8_t* pal_words, const int32_t* line_scroll, uint8_t* fb_out, uint8_t* index_out, uint32_t* bad_out) {
    const hipError_t e = zero_bad(stream, bad_out);
    if (e != hipSuccess) return e;
    draw_args A;
    A.L = words_of(&d->layout);
    A.lw = log2_of(d->tile_w), A.lh = log2_of(d->tile_h);
    A.format = (uint32_t)d->tile_format, A.n_tiles = (uint32_t)d->n_tiles;
    A.tile_bytes = (uint32_t)par_screen_tile_bytes(d->tile_format, d->tile_w, d->tile_h);
    A.map_w = (uint32_t)d->map_w, A.n_cells = (uint32_t)d->map_w * (uint32_t)d->map_h;
    A.period_x = (uint32_t)d->map_w << A.lw, A.period_y = (uint32_t)d->map_h << A.lh;
    A.rxs = log2_of(d->ratio_x), A.rys = log2_of(d->ratio_y), A.ccx = (uint32_t)((d->map_w + d->ratio_x - 1) / d->ratio_x);
    A.pal_format = (uint32_t)d->pal_format, A.n_colors = (uint32_t)d->n_colors, A.sub_size = (uint32_t)d->sub_size;
    A.backdrop = (uint32_t)d->backdrop;
    A.width = (uint32_t)d->width, A.height = (uint32_t)d->height, A.slots = ((uint32_t)d->width + 14u) / 8u;
    A.scroll_x = floor_mod_host(d->scroll_x, A.period_x), A.scroll_y = floor_mod_host(d->scroll_y, A.period_y);
    const uint32_t threads = std::max(A.height * A.slots, bad_out ? A.n_cells : 0u);  // (at most 4096 * 513, or 2^20)
    hipLaunchKernelGGL(draw_kernel, dim3((threads + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS), 0, stream, A, chr, map_words, attr,
                       pal_words, line_scroll, fb_out, index_out, bad_out);
    return hipGetLastError();
}

hipError_t launch_decode_map(hipStream_t stream, const par_screen_map_layout* layout, const uint8_t* map_words, int n_cells,
                             uint32_t* map_out, uint8_t* pal_out, uint32_t* bad_out) {
    const hipError_t e = zero_bad(stream, bad_out);
    if (e != hipSuccess) return e;
    const uint32_t n = (uint32_t)n_cells;
    hipLaunchKernelGGL(decode_map_kernel, dim3((n + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS), 0, stream, words_of(layout),
                       map_words, n, map_out, pal_out, bad_out);
    return hipGetLastError();
}

}  // namespace

extern "C" {

size_t par_screen_tile_bytes(int format, int tile_w, int tile_h) { return tile_bytes_of(format, tile_w, tile_h); }

size_t par_screen_palette_rgba(const uint8_t* words, int n, int format, uint8_t* rgba_out) {
    if (!words || !rgba_out || n < 1 || n > 256 || !pal_format_ok(format)) return 0;
    for (int i = 0; i < n; i++) {
        const uint32_t c = widen(words, (uint32_t)format, (uint32_t)i);
        for (int k = 0; k < 4; k++) rgba_out[4 * i + k] = (uint8_t)(c >> (8 * k));
    }
    return (size_t)n * 4;
}

int par_screen_draw_device(void* stream, const par_screen_desc* desc, const uint8_t* chr, const uint8_t* map_words,
                           const uint8_t* attr, const uint8_t* pal_words, const int32_t* line_scroll, uint8_t* fb_out,
                           uint8_t* index_out, uint32_t* bad_out) {
    if (!draw_args_ok(desc, chr, map_words, pal_words, line_scroll, fb_out, index_out) || !aligned4(bad_out)) return PAR_ERR_INVALID_ARG;
    return launch_draw((hipStream_t)stream, desc, chr, map_words, attr, pal_words, line_scroll, fb_out, index_out, bad_out) == hipSuccess
               ? PAR_OK
               : PAR_ERR_HIP;
}

int par_screen_decode_map_device(void* stream, const par_screen_map_layout* layout, const uint8_t* map_words, int n_cells,
                                 uint32_t* map_out, uint8_t* pal_out, uint32_t* bad_out) {
    if (!decode_args_ok(layout, map_words, n_cells, map_out) || !aligned4(bad_out)) return PAR_ERR_INVALID_ARG;
    return launch_decode_map((hipStream_t)stream, layout, map_words, n_cells, map_out, pal_out, bad_out) == hipSuccess ? PAR_OK
                                                                                                                        : PAR_ERR_HIP;
}

int par_screen_draw_host(int device, const par_screen_desc* desc, const uint8_t* chr, const uint8_t* map_words,
                         const uint8_t* attr, const uint8_t* pal_words, const int32_t* line_scroll, uint8_t* fb_out,
                         uint8_t* index_out, int* bad) {
    if (!draw_args_ok(desc, chr, map_words, pal_words, line_scroll, fb_out, index_out) || !bad) return PAR_ERR_INVALID_ARG;
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    const size_t cells = (size_t)desc->map_w * (size_t)desc->map_h, pixels = (size_t)desc->width * (size_t)desc->height;
    const size_t colour_cells = (size_t)((desc->map_w + desc->ratio_x - 1) / desc->ratio_x) *
                                (size_t)((desc->map_h + desc->ratio_y - 1) / desc->ratio_y);
    uint32_t n_bad = 0;
    par_device_buffer d_chr(e, chr, (size_t)desc->n_tiles * par_screen_tile_bytes(desc->tile_format, desc->tile_w, desc->tile_h), true);
    par_device_buffer d_map(e, map_words, cells * (size_t)desc->layout.word_bytes, true);
    par_device_buffer d_attr(e, attr, colour_cells, true);
    // (colour words that are not shown are not copied: the device call does not read them either)
    par_device_buffer d_pal(e, fb_out ? pal_words : nullptr, (size_t)desc->n_colors * pal_entry_bytes(desc->pal_format), true);
    par_device_buffer d_lines(e, line_scroll, 2 * (size_t)desc->height * sizeof(int32_t), true);
    par_device_buffer d_fb(e, fb_out, 4 * pixels, false);
    par_device_buffer d_index(e, index_out, pixels, false);
    par_device_buffer d_bad(e, &n_bad, sizeof(n_bad), false);
    if (e == hipSuccess) {
        e = launch_draw(nullptr, desc, d_chr.as<uint8_t>(), d_map.as<uint8_t>(), d_attr.as<uint8_t>(), d_pal.as<uint8_t>(),
                        d_lines.as<int32_t>(), d_fb.as<uint8_t>(), d_index.as<uint8_t>(), d_bad.as<uint32_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    d_fb.download(fb_out);
    d_index.download(index_out);
    d_bad.download(&n_bad);
    if (e == hipSuccess) *bad = (int)n_bad;
    return par_status_of(e);
}

int par_screen_decode_map_host(int device, const par_screen_map_layout* layout, const uint8_t* map_words, int n_cells,
                               uint32_t* map_out, uint8_t* pal_out, int* bad) {
    if (!decode_args_ok(layout, map_words, n_cells, map_out) || !bad) return PAR_ERR_INVALID_ARG;
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    uint32_t n_bad = 0;
    par_device_buffer d_words(e, map_words, (size_t)n_cells * (size_t)layout->word_bytes, true);
    par_device_buffer d_map(e, map_out, (size_t)n_cells * sizeof(uint32_t), false);
    par_device_buffer d_pal(e, pal_out, (size_t)n_cells, false);
    par_device_buffer d_bad(e, &n_bad, sizeof(n_bad), false);
    if (e == hipSuccess) {
        e = launch_decode_map(nullptr, layout, d_words.as<uint8_t>(), n_cells, d_map.as<uint32_t>(), d_pal.as<uint8_t>(), d_bad.as<uint32_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    d_map.download(map_out);
    d_pal.download(pal_out);
    d_bad.download(&n_bad);
    if (e == hipSuccess) *bad = (int)n_bad;
    return par_status_of(e);
}

}  // extern "C"
