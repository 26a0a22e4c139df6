// par_objects.hip — the objects add-on (libpar_objects.so): a tile machine's sprite layer drawn over its background, the
// object table a frame needs over a kept background, and the OAM bytes of two machines. The contract is beside the
// declarations in addons/include/par_objects.h; nothing here knows a par_context or a par_params, and nothing here is
// linked into libpar_raytracer.so or another add-on's library.
//
//   draw       two launches behind the four-byte fills of bad_out and over_out:
//     lines    a wavefront takes a scanline and walks the table 64 records at a time: the ballot of "live and covers this
//              line" and the popcount below a lane give every covering object its slot in table order, with no atomic; slots
//              below line_limit go to the line's list in `work`, and the line's count is written, so the block needs no
//              preparation. The wavefront of scanline 0 also counts the bad objects (once a call); a workgroup adds its
//              dropped and its bad objects in one atomic each.
//     draw     a thread takes eight consecutive pixels of a row, at a multiple of eight on the screen. A workgroup all of
//              whose rows have empty lists returns before it touches a plane or the colour words. Otherwise the thread
//              walks the row's list; of an object that overlaps its pixels it fetches the one or two eight-pixel segments
//              of the tile row it needs (a planar byte spread to a bit a byte by one multiplication, a packed word to a
//              nibble a byte by two shifts, an x flip as a byte swap), shifts them under its pixels and merges them into
//              the pixels without a winner; it stops when all eight have one. Then the behind test, the clamp and the
//              palette from LDS. The planes are read-modify-write: only written pixels are stored, and the wide stores (two
//              16-byte words of fb_io, one 8-byte word of index_io) are taken only when all eight are written and the
//              address allows.
//   from_maps  three launches over workgroups of 1024 cells, ordered by the kernel boundaries alone: the differing cells of
//              a workgroup counted, the counts scanned to bases by one workgroup (which writes D), and the records
//              scattered at base + the ballot rank; no atomic places anything.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_hostcall.h"
#include "par_objects.h"
#include "par_tilehw.h"

namespace {

constexpr uint32_t OB_THREADS = 256;
constexpr uint32_t OB_WAVES = OB_THREADS / 64;
constexpr uint32_t MAP_THREADS = 1024;
constexpr uint32_t MAP_WAVES = MAP_THREADS / 64;
constexpr uint64_t EACH_BYTE = 0x0101010101010101ull;

// par_tilehw.h's formats are par_objects_tile_format's and par_objects_palette_format's
static_assert(PAR_OBJECTS_1BPP == TILEHW_1BPP && PAR_OBJECTS_2BPP_PLANAR == TILEHW_2BPP_PLANAR);
static_assert(PAR_OBJECTS_2BPP_ROWS == TILEHW_2BPP_ROWS && PAR_OBJECTS_4BPP_ROWS == TILEHW_4BPP_ROWS);
static_assert(PAR_OBJECTS_4BPP_PACKED_HI == TILEHW_4BPP_PACKED_HI && PAR_OBJECTS_4BPP_PACKED_LO == TILEHW_4BPP_PACKED_LO);
static_assert(PAR_OBJECTS_4BPP_ROW_PLANES == TILEHW_4BPP_ROW_PLANES);
static_assert(PAR_OBJECTS_BGR555 == TILEHW_BGR555 && PAR_OBJECTS_BGR333_MD == TILEHW_BGR333_MD);
static_assert(PAR_OBJECTS_BGR222 == TILEHW_BGR222 && PAR_OBJECTS_RGBA8 == TILEHW_RGBA8);
static_assert(sizeof(par_object) == 16 && sizeof(par_objects_desc) == 56);

// ---- draw ------------------------------------------------------------------------------------------------------------------

// work: `height` counts, then `limit` table indices a line
__global__ __launch_bounds__(OB_THREADS) void lines_kernel(const par_object* objects, const uint32_t* count, uint32_t n_objects,
                                                           uint32_t n_tiles, uint32_t tile_h, uint32_t height, uint32_t limit,
                                                           uint32_t* work, uint32_t* bad_out, uint32_t* over_out) {
    __shared__ uint32_t over_of[OB_WAVES], bad_of[OB_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t y = blockIdx.x * OB_WAVES + wave;  // (the same for every lane of a wavefront)
    const uint32_t n = count ? std::min(*count, n_objects) : n_objects;
    uint32_t slots = 0, bad = 0;
    if (y < height) {
        uint32_t* list = work + height + (size_t)y * limit;
        for (uint32_t start = 0; start < n; start += 64) {
            const uint32_t j = start + lane;
            bool is_bad = false, covers = false;
            if (j < n) {
                const par_object o = objects[j];
                const bool hidden = (o.attr & PAR_OBJECTS_HIDDEN) != 0;
                is_bad = !hidden && (o.tile < 0 || (uint32_t)o.tile >= n_tiles || o.x < -32768 || o.x > 32767 || o.y < -32768 || o.y > 32767);
                // (y - y_j in unsigned arithmetic: below tile_h exactly when y_j <= y < y_j + tile_h)
                covers = !hidden && !is_bad && y - (uint32_t)o.y < tile_h;
            }
            const unsigned long long m = __ballot(covers);
            const uint32_t slot = slots + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (covers && slot < limit) list[slot] = j;
            slots += (uint32_t)__popcll(m);
            if (y == 0) bad += (uint32_t)__popcll(__ballot(is_bad));
        }
        if (lane == 0) work[y] = std::min(slots, limit);
    }
    if (lane == 0) over_of[wave] = slots > limit ? slots - limit : 0u, bad_of[wave] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t over = 0, bads = 0;
        for (uint32_t w = 0; w < OB_WAVES; w++) over += over_of[w], bads += bad_of[w];
        if (over_out && over) atomicAdd(over_out, over);
        if (bad_out && bads) atomicAdd(bad_out, bads);
    }
}

struct draw_args {
    uint32_t lw, lh;  // the binary logarithms of the tile's width and height (3 or 4)
    uint32_t format, tile_bytes, limit;
    uint32_t pal_format, n_colors, sub_size, pal_base, bg_sub_size, opaque;
    uint32_t width, height, slots;  // slots: the eight-pixel segments a row
};

// byte k: the value of pixel k of row `row` of the 8 x 8 sub-tile at d, as stored
__device__ __forceinline__ uint64_t segment_values(uint32_t format, const uint8_t* d, uint32_t row) {
    if (packed(format)) {
        const uint8_t* q = d + 4 * row;
        const uint32_t w = q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
        const uint32_t high = (w >> 4) & 0x0F0F0F0Fu, low = w & 0x0F0F0F0Fu;
        return format == TILEHW_4BPP_PACKED_HI ? spread_bytes(high) | spread_bytes(low) << 8 : spread_bytes(low) | spread_bytes(high) << 8;
    }
    uint64_t values = 0;
    const uint32_t bpp = bpp_of(format);
    for (uint32_t b = 0; b < bpp; b++) values |= spread_bits(d[plane_byte(format, b, row)]) << b;
    return values;
}

__global__ __launch_bounds__(OB_THREADS) void draw_kernel(draw_args A, const uint8_t* chr, const par_object* objects,
                                                          const uint8_t* pal_words, const uint8_t* bg_index, const uint32_t* work,
                                                          uint8_t* fb_io, uint8_t* index_io) {
    __shared__ uint32_t colours[256];
    const uint32_t gid = blockIdx.x * OB_THREADS + threadIdx.x;
    const uint32_t y = gid / A.slots, slot = gid - y * A.slots;
    const uint32_t count = y < A.height ? work[y] : 0u;
    if (!__syncthreads_or(count != 0)) return;  // the common case: nothing on the workgroup's rows
    if (fb_io) {                                // (the same for every thread of the launch)
        if (threadIdx.x < A.n_colors) colours[threadIdx.x] = widen(pal_words, A.pal_format, threadIdx.x);
        __syncthreads();
    }
    if (count == 0) return;

    const uint32_t x0 = 8 * slot, tw = 1u << A.lw, th = 1u << A.lh, nseg = tw >> 3, seg_bytes = 8 * bpp_of(A.format);
    const uint32_t in_row = std::min(8u, A.width - x0);  // (x0 < width: a row has ceil(width / 8) segments)
    const uint64_t off = in_row == 8 ? 0ull : ~0ull << (8 * in_row);  // the pixels past the row's end count as taken
    uint64_t have = off, values = 0, bases = 0, behinds = 0;          // a byte a pixel, left to right
    const uint32_t* list = work + A.height + (size_t)y * A.limit;
    for (uint32_t k = 0; k < count && have != ~0ull; k++) {
        const par_object o = objects[list[k]];
        const int32_t d = (int32_t)x0 - o.x;  // the segment's left end in the object (|x| < 2^15, x0 < 2^12)
        if (d <= -8 || d >= (int32_t)tw) continue;
        const uint32_t fx = ((uint32_t)o.attr >> 8) & 1u, fy = ((uint32_t)o.attr >> 9) & 1u;
        const uint32_t ty = y - (uint32_t)o.y, py = fy ? th - 1u - ty : ty;  // (the lines kernel saw ty < th)
        const uint8_t* tile_row = chr + (size_t)(uint32_t)o.tile * A.tile_bytes + (size_t)((py >> 3) * nseg) * seg_bytes;
        const int32_t s0 = d >> 3;             // the tile segment under the thread's first pixel, -1: left of the object
        const uint32_t r = (uint32_t)d & 7u;   // and where in it
        uint64_t vals = 0, cover = 0;
        if (s0 >= 0) {  // (s0 < nseg, as d < tw)
            const uint32_t col = fx ? nseg - 1u - (uint32_t)s0 : (uint32_t)s0;
            uint64_t v = segment_values(A.format, tile_row + (size_t)col * seg_bytes, py & 7u);
            if (fx) v = __builtin_bswap64(v);
            vals = v >> (8 * r), cover = ~0ull >> (8 * r);
        }
        if (r != 0 && s0 + 1 < (int32_t)nseg) {
            const uint32_t s1 = (uint32_t)(s0 + 1), col = fx ? nseg - 1u - s1 : s1;
            uint64_t v = segment_values(A.format, tile_row + (size_t)col * seg_bytes, py & 7u);
            if (fx) v = __builtin_bswap64(v);
            vals |= v << (64 - 8 * r), cover |= ~0ull << (64 - 8 * r);
        }
        if (!A.opaque) cover &= (((vals + 0x7F7F7F7F7F7F7F7Full) >> 7) & EACH_BYTE) * 0xFFull;  // (a value is below 16)
        const uint64_t win = cover & ~have;
        if (win == 0) continue;
        // (p * K is cut at 255, which n_colors - 1 never exceeds, so the clamp below sees no difference)
        const uint64_t base = std::min(A.pal_base + ((uint32_t)o.attr & 0xFFu) * A.sub_size, 255u);
        values |= vals & win, bases |= (base * EACH_BYTE) & win, have |= win;
        if (o.attr & PAR_OBJECTS_BEHIND) behinds |= win;
    }

    uint64_t written = have & ~off;
    const size_t at = (size_t)y * A.width + x0;
    if (bg_index && behinds != 0) {
        for (uint32_t k = 0; k < 8; k++) {
            const uint64_t pixel = 0xFFull << (8 * k);
            if ((behinds & pixel) != 0 && bg_index[at + k] % A.bg_sub_size != 0) written &= ~pixel;
        }
    }
    if (written == 0) return;
    const uint32_t last = A.n_colors - 1u;
    uint64_t indices = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
        const uint32_t i = std::min(((uint32_t)(bases >> (8 * k)) & 0xFFu) + ((uint32_t)(values >> (8 * k)) & 0xFFu), last);
        indices |= (uint64_t)i << (8 * k);
    }
    if (written == ~0ull) {  // all eight, hence a whole segment within the row
        if (index_io) {
            uint8_t* o = index_io + at;
            if ((reinterpret_cast<uintptr_t>(o) & 7u) == 0) {
                *reinterpret_cast<uint64_t*>(o) = indices;
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) o[k] = (uint8_t)(indices >> (8 * k));
            }
        }
        if (fb_io) {
            uint32_t c[8];
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) c[k] = colours[(uint32_t)(indices >> (8 * k)) & 0xFFu];
            uint32_t* o = reinterpret_cast<uint32_t*>(fb_io) + at;
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
        if (((written >> (8 * k)) & 0xFFu) == 0) continue;
        const uint32_t i = (uint32_t)(indices >> (8 * k)) & 0xFFu;
        if (index_io) index_io[at + k] = (uint8_t)i;
        if (fb_io) reinterpret_cast<uint32_t*>(fb_io)[at + k] = colours[i];
    }
}

// ---- from_maps -------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool differs(const uint32_t* map_bg, const uint8_t* cells_bg, const uint32_t* map, const uint8_t* cells,
                                        uint32_t c, uint32_t n) {
    return c < n && (map_bg[c] != map[c] || (cells && cells_bg[c] != cells[c]));
}

// work[b]: the differing cells of workgroup b's 1024 cells
__global__ __launch_bounds__(MAP_THREADS) void maps_count_kernel(const uint32_t* map_bg, const uint8_t* cells_bg, const uint32_t* map,
                                                                 const uint8_t* cells, uint32_t n, uint32_t* work) {
    __shared__ uint32_t wave_count[MAP_WAVES];
    const uint32_t c = blockIdx.x * MAP_THREADS + threadIdx.x;
    const unsigned long long m = __ballot(differs(map_bg, cells_bg, map, cells, c, n));
    if ((threadIdx.x & 63u) == 0) wave_count[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (uint32_t w = 0; w < MAP_WAVES; w++) total += wave_count[w];
        work[blockIdx.x] = total;
    }
}

// ONE workgroup: work[b] becomes the differing cells before workgroup b, and *count_out their sum (blocks <= 1024)
__global__ __launch_bounds__(MAP_THREADS) void maps_scan_kernel(uint32_t* work, uint32_t blocks, uint32_t* count_out) {
    __shared__ uint32_t wave_total[MAP_WAVES];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t own = t < blocks ? work[t] : 0u;
    uint32_t incl = own;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < MAP_WAVES; w++) {
        if (w < wave) before += wave_total[w];
        total += wave_total[w];
    }
    if (t < blocks) work[t] = before + incl - own;
    if (t == 0) *count_out = total;
}

__global__ __launch_bounds__(MAP_THREADS) void maps_scatter_kernel(const uint32_t* map_bg, const uint8_t* cells_bg, const uint32_t* map,
                                                                   const uint8_t* cells, uint32_t n, uint32_t gcx, int32_t tile_w,
                                                                   int32_t tile_h, int32_t x0, int32_t y0, uint32_t capacity,
                                                                   const uint32_t* work, par_object* objects_out) {
    __shared__ uint32_t wave_count[MAP_WAVES];
    const uint32_t c = blockIdx.x * MAP_THREADS + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool differing = differs(map_bg, cells_bg, map, cells, c, n);
    const unsigned long long m = __ballot(differing);
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!differing) return;
    uint32_t rank = work[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; w++) rank += wave_count[w];
    if (rank >= capacity) return;
    const uint32_t word = map[c], cy = c / gcx, cx = c - cy * gcx;
    par_object o;
    o.x = x0 + (int32_t)cx * tile_w, o.y = y0 + (int32_t)cy * tile_h;
    o.tile = (int32_t)(word & 0x3FFFFFFFu);
    o.attr = (int32_t)((cells ? (uint32_t)cells[c] : 0u) | ((word >> 30) & 1u) << 8 | (word >> 31) << 9);
    objects_out[rank] = o;
}

// ---- host side ---------------------------------------------------------------------------------------------------------

bool draw_args_ok(const par_objects_desc* d, const uint8_t* chr, const par_object* objects, const uint8_t* pal_words,
                  const uint8_t* fb_io, const uint8_t* index_io) {
    if (!d || !chr || !objects || (!fb_io && !index_io) || (fb_io && !pal_words)) return false;
    if (!aligned4(objects) || !aligned4(fb_io)) return false;
    if (!tile_dim_ok(d->tile_w) || !tile_dim_ok(d->tile_h) || !format_ok(d->tile_format)) return false;
    if (d->n_tiles < 1 || d->n_tiles > PAR_OBJECTS_MAX_TILES || d->n_objects < 1 || d->n_objects > PAR_OBJECTS_MAX) return false;
    if (d->line_limit < 1 || d->line_limit > PAR_OBJECTS_MAX_LINE) return false;
    if (!pal_format_ok(d->pal_format) || d->n_colors < 1 || d->n_colors > 256 || d->sub_size < 1 || d->sub_size > 256) return false;
    if (d->pal_base < 0 || d->pal_base > 255 || d->bg_sub_size < 1 || d->bg_sub_size > 256) return false;
    if (d->opaque != 0 && d->opaque != 1) return false;
    return d->width >= 1 && d->width <= PAR_OBJECTS_MAX_SIDE && d->height >= 1 && d->height <= PAR_OBJECTS_MAX_SIDE;
}

bool in_int16(int64_t v) { return v >= -32768 && v <= 32767; }

bool maps_args_ok(const uint32_t* map_bg, const uint8_t* cells_bg, const uint32_t* map, const uint8_t* cells, int gcx, int gcy,
                  int tile_w, int tile_h, int x0, int y0, int capacity, const par_object* objects_out) {
    if (!map_bg || !map || !objects_out || (cells_bg == nullptr) != (cells == nullptr)) return false;
    if (!aligned4(map_bg) || !aligned4(map) || !aligned4(objects_out)) return false;
    if (gcx < 1 || gcy < 1 || (int64_t)gcx * (int64_t)gcy > PAR_OBJECTS_MAX_CELLS) return false;
    if (!tile_dim_ok(tile_w) || !tile_dim_ok(tile_h) || capacity < 1 || capacity > PAR_OBJECTS_MAX) return false;
    return in_int16(x0) && in_int16(y0) && in_int16((int64_t)x0 + (int64_t)(gcx - 1) * tile_w) &&
           in_int16((int64_t)y0 + (int64_t)(gcy - 1) * tile_h);
}

hipError_t launch_draw(hipStream_t stream, const par_objects_desc* d, const uint8_t* chr, const par_object* objects, const uint32_t* count,
                       const uint8_t* pal_words, const uint8_t* bg_index, void* work, uint8_t* fb_io, uint8_t* index_io,
                       uint32_t* bad_out, uint32_t* over_out) {
    hipError_t e = zero_bad(stream, bad_out);
    if (e == hipSuccess) e = zero_bad(stream, over_out);
    if (e != hipSuccess) return e;
    const uint32_t height = (uint32_t)d->height;
    hipLaunchKernelGGL(lines_kernel, dim3((height + OB_WAVES - 1) / OB_WAVES), dim3(OB_THREADS), 0, stream, objects, count,
                       (uint32_t)d->n_objects, (uint32_t)d->n_tiles, (uint32_t)d->tile_h, height, (uint32_t)d->line_limit,
                       static_cast<uint32_t*>(work), bad_out, over_out);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    draw_args A;
    A.lw = log2_of(d->tile_w), A.lh = log2_of(d->tile_h);
    A.format = (uint32_t)d->tile_format, A.tile_bytes = (uint32_t)tile_bytes_of(d->tile_format, d->tile_w, d->tile_h);
    A.limit = (uint32_t)d->line_limit;
    A.pal_format = (uint32_t)d->pal_format, A.n_colors = (uint32_t)d->n_colors, A.sub_size = (uint32_t)d->sub_size;
    A.pal_base = (uint32_t)d->pal_base, A.bg_sub_size = (uint32_t)d->bg_sub_size, A.opaque = (uint32_t)d->opaque;
    A.width = (uint32_t)d->width, A.height = height, A.slots = ((uint32_t)d->width + 7u) / 8u;
    const uint32_t threads = A.height * A.slots;  // (at most 4096 * 512)
    hipLaunchKernelGGL(draw_kernel, dim3((threads + OB_THREADS - 1) / OB_THREADS), dim3(OB_THREADS), 0, stream, A, chr, objects, pal_words,
                       bg_index, static_cast<const uint32_t*>(work), fb_io, index_io);
    return hipGetLastError();
}

hipError_t launch_from_maps(hipStream_t stream, const uint32_t* map_bg, const uint8_t* cells_bg, const uint32_t* map, const uint8_t* cells,
                            int gcx, int gcy, int tile_w, int tile_h, int x0, int y0, int capacity, void* work, par_object* objects_out,
                            uint32_t* count_out) {
    const uint32_t n = (uint32_t)gcx * (uint32_t)gcy, blocks = (n + MAP_THREADS - 1) / MAP_THREADS;  // (at most 1024)
    uint32_t* bases = static_cast<uint32_t*>(work);
    hipLaunchKernelGGL(maps_count_kernel, dim3(blocks), dim3(MAP_THREADS), 0, stream, map_bg, cells_bg, map, cells, n, bases);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(maps_scan_kernel, dim3(1), dim3(MAP_THREADS), 0, stream, bases, blocks, count_out);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(maps_scatter_kernel, dim3(blocks), dim3(MAP_THREADS), 0, stream, map_bg, cells_bg, map, cells, n, (uint32_t)gcx,
                       tile_w, tile_h, x0, y0, (uint32_t)capacity, bases, objects_out);
    return hipGetLastError();
}

struct oam_format {
    int y_add, x_add, y_lo, y_hi, x_lo, x_hi, p_mask, fx_bit, fy_bit, behind_bit, hidden_y;
    int at_y, at_x, at_tile, at_attr;  // where each byte goes
};
constexpr oam_format OAM[2] = {{-1, 0, 1, 256, 0, 255, 3, 6, 7, 5, 0xFF, 0, 3, 1, 2}, {16, 8, -16, 239, -8, 247, 7, 5, 6, 7, 0, 0, 1, 2, 3}};

}  // namespace

extern "C" {

size_t par_objects_work_bytes(int height, int line_limit) {
    if (height < 1 || height > PAR_OBJECTS_MAX_SIDE || line_limit < 1 || line_limit > PAR_OBJECTS_MAX_LINE) return 0;
    return 4 * (size_t)height * (1 + (size_t)line_limit);
}

size_t par_objects_from_maps_work_bytes(int n_cells) {
    if (n_cells < 1 || n_cells > PAR_OBJECTS_MAX_CELLS) return 0;
    return 4 * (((size_t)n_cells + MAP_THREADS - 1) / MAP_THREADS);
}

int par_objects_machine_limits(int machine, int* line_limit, int* max_objects) {
    static const int limits[6][2] = {{8, 64}, {10, 40}, {8, 64}, {20, 80}, {32, 128}, {128, 128}};
    if (machine < PAR_OBJECTS_NES || machine > PAR_OBJECTS_GBA || !line_limit || !max_objects) return PAR_ERR_INVALID_ARG;
    *line_limit = limits[machine][0], *max_objects = limits[machine][1];
    return PAR_OK;
}

int par_objects_pack(int format, const par_object* objects, int n, uint8_t* out, int* bad) {
    if ((format != PAR_OBJECTS_OAM_NES && format != PAR_OBJECTS_OAM_GB) || !objects || !out || !bad || n < 1 || n > PAR_OBJECTS_MAX)
        return PAR_ERR_INVALID_ARG;
    const oam_format& F = OAM[format];
    int n_bad = 0;
    for (int j = 0; j < n; j++) {
        const par_object& o = objects[j];
        const uint32_t attr = (uint32_t)o.attr, p = attr & 0xFFu;
        const bool hidden = (attr & PAR_OBJECTS_HIDDEN) != 0;
        const bool fits = o.y >= F.y_lo && o.y <= F.y_hi && o.x >= F.x_lo && o.x <= F.x_hi && o.tile >= 0 && o.tile <= 255 && p <= (uint32_t)F.p_mask;
        n_bad += !hidden && !fits;
        uint8_t* b = out + 4 * (size_t)j;
        b[F.at_y] = hidden ? (uint8_t)F.hidden_y : (uint8_t)((uint32_t)o.y + (uint32_t)F.y_add);
        b[F.at_x] = (uint8_t)((uint32_t)o.x + (uint32_t)F.x_add);
        b[F.at_tile] = (uint8_t)o.tile;
        b[F.at_attr] = (uint8_t)((p & (uint32_t)F.p_mask) | ((attr >> 8) & 1u) << F.fx_bit | ((attr >> 9) & 1u) << F.fy_bit |
                                 ((attr >> 10) & 1u) << F.behind_bit);
    }
    *bad = n_bad;
    return PAR_OK;
}

int par_objects_unpack(int format, const uint8_t* data, int n, par_object* objects_out) {
    if ((format != PAR_OBJECTS_OAM_NES && format != PAR_OBJECTS_OAM_GB) || !data || !objects_out || n < 1 || n > PAR_OBJECTS_MAX)
        return PAR_ERR_INVALID_ARG;
    const oam_format& F = OAM[format];
    for (int j = 0; j < n; j++) {
        const uint8_t* b = data + 4 * (size_t)j;
        par_object& o = objects_out[j];
        const uint32_t a = b[F.at_attr];
        o.y = (int32_t)b[F.at_y] - F.y_add, o.x = (int32_t)b[F.at_x] - F.x_add, o.tile = b[F.at_tile];
        o.attr = (int32_t)((a & (uint32_t)F.p_mask) | ((a >> F.fx_bit) & 1u) << 8 | ((a >> F.fy_bit) & 1u) << 9 | ((a >> F.behind_bit) & 1u) << 10);
    }
    return PAR_OK;
}

int par_objects_draw_device(void* stream, const par_objects_desc* desc, const uint8_t* chr, const par_object* objects,
                            const uint32_t* count, const uint8_t* pal_words, const uint8_t* bg_index, void* work,
                            uint8_t* fb_io, uint8_t* index_io, uint32_t* bad_out, uint32_t* over_out) {
    if (!draw_args_ok(desc, chr, objects, pal_words, fb_io, index_io) || !work || !aligned4(work) || !aligned4(count) ||
        !aligned4(bad_out) || !aligned4(over_out))
        return PAR_ERR_INVALID_ARG;
    return launch_draw((hipStream_t)stream, desc, chr, objects, count, pal_words, bg_index, work, fb_io, index_io, bad_out, over_out) == hipSuccess
               ? PAR_OK
               : PAR_ERR_HIP;
}

int par_objects_from_maps_device(void* stream, const uint32_t* map_bg, const uint8_t* cells_bg, const uint32_t* map,
                                 const uint8_t* cells, int gcx, int gcy, int tile_w, int tile_h, int x0, int y0, int capacity,
                                 void* work, par_object* objects_out, uint32_t* count_out) {
    if (!maps_args_ok(map_bg, cells_bg, map, cells, gcx, gcy, tile_w, tile_h, x0, y0, capacity, objects_out) || !work || !aligned4(work) ||
        !count_out || !aligned4(count_out))
        return PAR_ERR_INVALID_ARG;
    return launch_from_maps((hipStream_t)stream, map_bg, cells_bg, map, cells, gcx, gcy, tile_w, tile_h, x0, y0, capacity, work, objects_out,
                            count_out) == hipSuccess
               ? PAR_OK
               : PAR_ERR_HIP;
}

int par_objects_draw_host(int device, const par_objects_desc* desc, const uint8_t* chr, const par_object* objects, int count,
                          const uint8_t* pal_words, const uint8_t* bg_index, uint8_t* fb_io, uint8_t* index_io, int* bad,
                          int* over) {
    if (!draw_args_ok(desc, chr, objects, pal_words, fb_io, index_io) || count < 0 || !bad || !over) return PAR_ERR_INVALID_ARG;
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    const size_t pixels = (size_t)desc->width * (size_t)desc->height;
    const uint32_t n = (uint32_t)count;
    uint32_t n_bad = 0, n_over = 0;
    const bool bg_is_index = bg_index && bg_index == index_io;
    par_device_buffer d_chr(e, chr, (size_t)desc->n_tiles * tile_bytes_of(desc->tile_format, desc->tile_w, desc->tile_h), true);
    par_device_buffer d_objects(e, objects, (size_t)desc->n_objects * sizeof(par_object), true);
    par_device_buffer d_count(e, &n, sizeof(n), true);
    // (colour words that are not shown are not copied: the device call does not read them either)
    par_device_buffer d_pal(e, fb_io ? pal_words : nullptr, (size_t)desc->n_colors * pal_entry_bytes(desc->pal_format), true);
    par_device_buffer d_bg(e, bg_is_index ? nullptr : bg_index, pixels, true);
    par_device_buffer d_work(e, chr, par_objects_work_bytes(desc->height, desc->line_limit), false);  // (device memory only)
    par_device_buffer d_fb(e, fb_io, 4 * pixels, true);
    par_device_buffer d_index(e, index_io, pixels, true);
    par_device_buffer d_bad(e, &n_bad, sizeof(n_bad), false);
    par_device_buffer d_over(e, &n_over, sizeof(n_over), false);
    if (e == hipSuccess) {
        e = launch_draw(nullptr, desc, d_chr.as<uint8_t>(), d_objects.as<par_object>(), d_count.as<uint32_t>(), d_pal.as<uint8_t>(),
                        bg_is_index ? d_index.as<uint8_t>() : d_bg.as<uint8_t>(), d_work.as<void>(), d_fb.as<uint8_t>(),
                        d_index.as<uint8_t>(), d_bad.as<uint32_t>(), d_over.as<uint32_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    d_fb.download(fb_io);
    d_index.download(index_io);
    d_bad.download(&n_bad);
    d_over.download(&n_over);
    if (e == hipSuccess) *bad = (int)n_bad, *over = (int)n_over;
    return par_status_of(e);
}

int par_objects_from_maps_host(int device, const uint32_t* map_bg, const uint8_t* cells_bg, const uint32_t* map,
                               const uint8_t* cells, int gcx, int gcy, int tile_w, int tile_h, int x0, int y0, int capacity,
                               par_object* objects_out, int* count) {
    if (!maps_args_ok(map_bg, cells_bg, map, cells, gcx, gcy, tile_w, tile_h, x0, y0, capacity, objects_out) || !count) return PAR_ERR_INVALID_ARG;
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    const size_t n = (size_t)gcx * (size_t)gcy;
    uint32_t found = 0;
    par_device_buffer d_map_bg(e, map_bg, n * sizeof(uint32_t), true);
    par_device_buffer d_cells_bg(e, cells_bg, n, true);
    par_device_buffer d_map(e, map, n * sizeof(uint32_t), true);
    par_device_buffer d_cells(e, cells, n, true);
    par_device_buffer d_work(e, map, par_objects_from_maps_work_bytes((int)n), false);  // (device memory only)
    par_device_buffer d_objects(e, objects_out, (size_t)capacity * sizeof(par_object), false);
    par_device_buffer d_count(e, &found, sizeof(found), false);
    if (e == hipSuccess) {
        e = launch_from_maps(nullptr, d_map_bg.as<uint32_t>(), d_cells_bg.as<uint8_t>(), d_map.as<uint32_t>(), d_cells.as<uint8_t>(), gcx, gcy,
                             tile_w, tile_h, x0, y0, capacity, d_work.as<void>(), d_objects.as<par_object>(), d_count.as<uint32_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    d_count.download(&found);
    // the records that were written, and no byte of the caller's beyond them
    const size_t made = std::min<size_t>(found, (size_t)capacity);
    if (e == hipSuccess && made) e = hipMemcpy(objects_out, d_objects.as<par_object>(), made * sizeof(par_object), hipMemcpyDeviceToHost);
    if (e == hipSuccess) *count = (int)found;
    return par_status_of(e);
}

}  // extern "C"
