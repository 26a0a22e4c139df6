// par_vram.hip — the VRAM-export add-on (libpar_vram.so): the local plane, tiles packed into and out of the bit planes and
// nibbles of tile hardware, map words under a machine's layout, palette words. The contract is beside the declarations in
// addons/include/par_vram.h; nothing here knows a par_context or a par_params, and nothing here is linked into
// libpar_raytracer.so.
//
// Every device call is one launch, behind one four-byte fill where it counts into a bad_out:
//   local   a thread takes eight bytes: v % K as v - K * ((v * ceil(65536 / K)) >> 16), exact for v < 256 and K <= 256
//           (the magic's excess over 65536 / K is below K / 65536 a unit, times 255 below one)
//   encode  a wavefront takes an 8 x 8 sub-tile, lane l its pixel (7 - (l & 7), l >> 3): the ballot of bit b of the
//           pixels is plane b's eight row bytes, most significant bit leftmost, byte y in bits [8 y, 8 y + 8). Lane j
//           then stores byte j of the sub-tile: a byte of one ballot, or for the packed formats two pixels fetched
//           across the lanes. The launch is sized by `capacity`; a wavefront past min(*count, capacity) tiles stores
//           nothing. A workgroup is four wavefronts and a tile is one, two or four sub-tiles, so a tile's sub-tiles share
//           a workgroup, which ORs their "a byte too large" marks in LDS and adds its tiles to bad_out in one atomic.
//   decode  a wavefront a sub-tile, lane l the pixel (l & 7, l >> 3): bpp byte loads, or one and a nibble
//   map     a thread a cell; the bad cells of a workgroup in one atomic
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_hostcall.h"
#include "par_tilehw.h"
#include "par_vram.h"

namespace {

constexpr uint32_t VR_THREADS = 256;
constexpr uint32_t VR_WAVES = VR_THREADS / 64;   // sub-tiles a workgroup
constexpr uint32_t VR_LOCAL_BYTES = 8;           // bytes a thread of the local plane
constexpr uint32_t VR_ID_MASK = 0x3FFFFFFFu;
static_assert(VR_WAVES == 4, "a tile's one, two or four sub-tiles share a workgroup");

// par_tilehw.h's formats are par_vram_tile_format's
static_assert(PAR_VRAM_1BPP == TILEHW_1BPP);
static_assert(PAR_VRAM_2BPP_PLANAR == TILEHW_2BPP_PLANAR);
static_assert(PAR_VRAM_2BPP_ROWS == TILEHW_2BPP_ROWS);
static_assert(PAR_VRAM_4BPP_ROWS == TILEHW_4BPP_ROWS);
static_assert(PAR_VRAM_4BPP_PACKED_HI == TILEHW_4BPP_PACKED_HI);
static_assert(PAR_VRAM_4BPP_PACKED_LO == TILEHW_4BPP_PACKED_LO);
static_assert(PAR_VRAM_4BPP_ROW_PLANES == TILEHW_4BPP_ROW_PLANES);

// plane_byte's inverse: the plane (low two bits) and the row (from bit 2 on) of byte j
__device__ __forceinline__ uint32_t plane_and_row(uint32_t format, uint32_t j) {
    switch (format) {
        case PAR_VRAM_2BPP_PLANAR: return ((j >> 3) & 1) | ((j & 7) << 2);
        case PAR_VRAM_2BPP_ROWS: return (j & 1) | (((j >> 1) & 7) << 2);
        case PAR_VRAM_4BPP_ROWS: return (((j >> 4) & 1) << 1) | (j & 1) | (((j >> 1) & 7) << 2);
        case PAR_VRAM_4BPP_ROW_PLANES: return (j & 3) | (((j >> 2) & 7) << 2);
        default: return (j & 7) << 2;
    }
}

__global__ __launch_bounds__(VR_THREADS) void local_kernel(const uint8_t* index, uint32_t n, uint32_t K, uint32_t magic,
                                                           uint8_t* local_out) {
    const uint32_t at = (blockIdx.x * VR_THREADS + threadIdx.x) * VR_LOCAL_BYTES;  // (n < 2^31: below 2^31 + 2048)
    if (at >= n) return;
    if (n - at >= VR_LOCAL_BYTES) {
        uint64_t v, r = 0;
        __builtin_memcpy(&v, index + at, VR_LOCAL_BYTES);
#pragma unroll
        for (uint32_t k = 0; k < VR_LOCAL_BYTES; k++) {
            const uint32_t b = (uint32_t)(v >> (8 * k)) & 0xFFu;
            r |= (uint64_t)(b - K * ((b * magic) >> 16)) << (8 * k);
        }
        __builtin_memcpy(local_out + at, &r, VR_LOCAL_BYTES);
        return;
    }
    for (uint32_t i = at; i < n; i++) {
        const uint32_t b = index[i];
        local_out[i] = (uint8_t)(b - K * ((b * magic) >> 16));
    }
}

// lw, lh: the binary logarithms of the tile's width and height (3 or 4)
__global__ __launch_bounds__(VR_THREADS) void encode_tiles_kernel(const uint8_t* tiles, uint32_t capacity, const uint32_t* count,
                                                                  uint32_t lw, uint32_t lh, uint32_t format, uint8_t* out,
                                                                  uint32_t* bad_out) {
    __shared__ uint32_t over_of[VR_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n = count ? std::min(*count, capacity) : capacity;
    const uint32_t ls = lw + lh - 6;               // the logarithm of the sub-tiles a tile
    const uint32_t g = blockIdx.x * VR_WAVES + wave;  // the sub-tile, below 2^22
    const uint32_t tile = g >> ls, sub = g & ((1u << ls) - 1u);
    const bool live = tile < n;
    const uint32_t bpp = bpp_of(format), sub_bytes = 8 * bpp;
    uint32_t v = 0;
    if (live) {
        const uint32_t sx = sub & ((1u << (lw - 3)) - 1u), sy = sub >> (lw - 3);
        const uint32_t x = 7u - (lane & 7u), y = lane >> 3;
        v = tiles[((size_t)tile << (lw + lh)) + (((sy << 3) + y) << lw) + (sx << 3) + x];
    }
    const bool over = __ballot((v >> bpp) != 0) != 0;
    uint32_t byte;
    if (packed(format)) {
        // byte j = 4 y + (x >> 1) holds the pixels (2 (j & 3), j >> 2) and the one to its right, a lane lower
        const uint32_t even = 8 * ((lane >> 2) & 7u) + 7u - 2 * (lane & 3u);
        const uint32_t a = (uint32_t)__shfl((int)v, (int)even) & 15u, b = (uint32_t)__shfl((int)v, (int)even - 1) & 15u;
        byte = format == PAR_VRAM_4BPP_PACKED_HI ? (a << 4 | b) : (b << 4 | a);
    } else {
        const uint64_t m0 = __ballot(v & 1u), m1 = __ballot(v & 2u), m2 = __ballot(v & 4u), m3 = __ballot(v & 8u);
        const uint32_t by = plane_and_row(format, lane), b = by & 3u, y = by >> 2;
        const uint64_t m = b == 0 ? m0 : (b == 1 ? m1 : (b == 2 ? m2 : m3));
        byte = (uint32_t)(m >> (8 * y)) & 0xFFu;
    }
    if (live && lane < sub_bytes) out[(size_t)g * sub_bytes + lane] = (uint8_t)byte;
    if (!bad_out) return;  // (the same for every lane of the launch)
    if (lane == 0) over_of[wave] = live && over ? 1u : 0u;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t bad = 0;
        for (uint32_t w = 0; w < VR_WAVES; w += 1u << ls) {
            uint32_t any = 0;
            for (uint32_t k = 0; k < (1u << ls); k++) any |= over_of[w + k];
            bad += any;
        }
        if (bad) atomicAdd(bad_out, bad);
    }
}

__global__ __launch_bounds__(VR_THREADS) void decode_tiles_kernel(const uint8_t* data, uint32_t n_tiles, uint32_t lw, uint32_t lh,
                                                                  uint32_t format, uint8_t* tiles_out) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t ls = lw + lh - 6;
    const uint32_t g = blockIdx.x * VR_WAVES + wave;
    const uint32_t tile = g >> ls, sub = g & ((1u << ls) - 1u);
    if (tile >= n_tiles) return;
    const uint32_t bpp = bpp_of(format);
    const uint32_t sx = sub & ((1u << (lw - 3)) - 1u), sy = sub >> (lw - 3);
    const uint32_t x = lane & 7u, y = lane >> 3;
    const uint8_t* d = data + (size_t)g * (8 * bpp);
    uint32_t v = 0;
    if (packed(format)) {
        const uint32_t byte = d[4 * y + (x >> 1)];
        const bool high = ((x & 1u) != 0) == (format == PAR_VRAM_4BPP_PACKED_LO);
        v = high ? byte >> 4 : byte & 15u;
    } else {
        for (uint32_t b = 0; b < bpp; b++) v |= ((d[plane_byte(format, b, y)] >> (7u - x)) & 1u) << b;
    }
    tiles_out[((size_t)tile << (lw + lh)) + (((sy << 3) + y) << lw) + (sx << 3) + x] = (uint8_t)v;
}

// rxs, rys: the binary logarithms of the ratios; ccx: the colour cells a row
__global__ __launch_bounds__(VR_THREADS) void encode_map_kernel(par_vram_map_layout L, const uint32_t* map, uint32_t gcx,
                                                                uint32_t n, const uint8_t* cells, uint32_t rxs, uint32_t rys,
                                                                uint32_t ccx, uint8_t* out, uint32_t* bad_out) {
    const uint32_t c = blockIdx.x * VR_THREADS + threadIdx.x;
    bool bad = false;
    if (c < n) {
        const uint32_t entry = map[c], id = entry & VR_ID_MASK, fx = (entry >> 30) & 1u, fy = entry >> 31;
        const uint32_t ty = c / gcx, tx = c - ty * gcx;
        const uint64_t p = cells ? cells[(tx >> rxs) + (ty >> rys) * ccx] : 0u;
        const uint64_t t = (uint64_t)id * (uint32_t)L.tile_step + (uint32_t)L.tile_base;
        const uint64_t tile_mask = (1ull << L.tile_bits) - 1u, pal_mask = (1ull << L.pal_bits) - 1u;
        uint32_t w = (uint32_t)((t & tile_mask) << L.tile_shift) | (uint32_t)((p & pal_mask) << L.pal_shift) | (uint32_t)L.set_bits;
        bad = t > tile_mask || p > pal_mask;
        if (L.flip_x_bit >= 0) w |= fx << L.flip_x_bit;
        else bad = bad || fx != 0;
        if (L.flip_y_bit >= 0) w |= fy << L.flip_y_bit;
        else bad = bad || fy != 0;
        const uint32_t wb = (uint32_t)L.word_bytes;
        uint8_t* o = out + (size_t)c * wb;
        for (uint32_t k = 0; k < wb; k++) o[k] = (uint8_t)(w >> (8 * (L.big_endian ? wb - 1 - k : k)));
    }
    if (bad_out) add_bad<VR_WAVES>(bad, bad_out);  // (the same for every lane of the launch)
}

// ---- host side ---------------------------------------------------------------------------------------------------------

bool tiles_args_ok(const uint8_t* in, int n_tiles, int tile_w, int tile_h, int format, const uint8_t* out) {
    return in && out && n_tiles >= 1 && n_tiles <= PAR_VRAM_MAX_TILES && tile_dim_ok(tile_w) && tile_dim_ok(tile_h) && format_ok(format);
}

bool map_args_ok(const par_vram_map_layout* layout, const uint32_t* map, int gcx, int gcy, int ratio_x, int ratio_y,
                 const uint8_t* out) {
    if (!layout || !map || !out || !aligned4(map) || gcx < 1 || gcy < 1) return false;
    if ((int64_t)gcx * (int64_t)gcy > PAR_VRAM_MAX_CELLS) return false;
    if ((ratio_x != 1 && ratio_x != 2) || (ratio_y != 1 && ratio_y != 2)) return false;
    return layout_ok(layout);
}

hipError_t launch_encode_tiles(hipStream_t stream, const uint8_t* tiles, int capacity, const uint32_t* count, int tile_w, int tile_h,
                               int format, uint8_t* out, uint32_t* bad_out) {
    const hipError_t e = zero_bad(stream, bad_out);
    if (e != hipSuccess) return e;
    const uint32_t lw = log2_of(tile_w), lh = log2_of(tile_h);
    const uint32_t subs = (uint32_t)capacity << (lw + lh - 6);
    hipLaunchKernelGGL(encode_tiles_kernel, dim3((subs + VR_WAVES - 1) / VR_WAVES), dim3(VR_THREADS), 0, stream, tiles,
                       (uint32_t)capacity, count, lw, lh, (uint32_t)format, out, bad_out);
    return hipGetLastError();
}

hipError_t launch_decode_tiles(hipStream_t stream, const uint8_t* data, int n_tiles, int tile_w, int tile_h, int format,
                               uint8_t* tiles_out) {
    const uint32_t lw = log2_of(tile_w), lh = log2_of(tile_h);
    const uint32_t subs = (uint32_t)n_tiles << (lw + lh - 6);
    hipLaunchKernelGGL(decode_tiles_kernel, dim3((subs + VR_WAVES - 1) / VR_WAVES), dim3(VR_THREADS), 0, stream, data,
                       (uint32_t)n_tiles, lw, lh, (uint32_t)format, tiles_out);
    return hipGetLastError();
}

hipError_t launch_encode_map(hipStream_t stream, const par_vram_map_layout* layout, const uint32_t* map, int gcx, int gcy,
                             const uint8_t* cells, int ratio_x, int ratio_y, uint8_t* out, uint32_t* bad_out) {
    const hipError_t e = zero_bad(stream, bad_out);
    if (e != hipSuccess) return e;
    const uint32_t n = (uint32_t)gcx * (uint32_t)gcy;
    hipLaunchKernelGGL(encode_map_kernel, dim3((n + VR_THREADS - 1) / VR_THREADS), dim3(VR_THREADS), 0, stream, *layout, map,
                       (uint32_t)gcx, n, cells, log2_of(ratio_x), log2_of(ratio_y), (uint32_t)((gcx + ratio_x - 1) / ratio_x), out,
                       bad_out);
    return hipGetLastError();
}

}  // namespace

extern "C" {

size_t par_vram_tile_bytes(int format, int tile_w, int tile_h) { return tile_bytes_of(format, tile_w, tile_h); }

int par_vram_local_device(void* stream, const uint8_t* index, int n_bytes, int sub_size, uint8_t* local_out) {
    if (!index || !local_out || n_bytes < 1 || sub_size < 1 || sub_size > 256) return PAR_ERR_INVALID_ARG;
    const uint32_t n = (uint32_t)n_bytes, K = (uint32_t)sub_size, per_group = VR_THREADS * VR_LOCAL_BYTES;
    hipLaunchKernelGGL(local_kernel, dim3((n + per_group - 1) / per_group), dim3(VR_THREADS), 0, (hipStream_t)stream, index, n, K,
                       (65536u + K - 1) / K, local_out);
    return hipGetLastError() == hipSuccess ? PAR_OK : PAR_ERR_HIP;
}

int par_vram_encode_tiles_device(void* stream, const uint8_t* tiles, int capacity, const uint32_t* count, int tile_w,
                                 int tile_h, int format, uint8_t* out, uint32_t* bad_out) {
    if (!tiles_args_ok(tiles, capacity, tile_w, tile_h, format, out) || !aligned4(count) || !aligned4(bad_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    return launch_encode_tiles((hipStream_t)stream, tiles, capacity, count, tile_w, tile_h, format, out, bad_out) == hipSuccess
               ? PAR_OK
               : PAR_ERR_HIP;
}

int par_vram_decode_tiles_device(void* stream, const uint8_t* data, int n_tiles, int tile_w, int tile_h, int format,
                                 uint8_t* tiles_out) {
    if (!tiles_args_ok(data, n_tiles, tile_w, tile_h, format, tiles_out)) return PAR_ERR_INVALID_ARG;
    return launch_decode_tiles((hipStream_t)stream, data, n_tiles, tile_w, tile_h, format, tiles_out) == hipSuccess ? PAR_OK
                                                                                                                    : PAR_ERR_HIP;
}

int par_vram_map_layout_preset(int machine, par_vram_map_layout* layout) {
    // word_bytes, big_endian, tile shift / bits, palette shift / bits, x flip, y flip, step, base, set bits
    static const par_vram_map_layout presets[] = {
        {1, 0, 0, 8, 0, 0, -1, -1, 1, 0, 0},    // NES: the name table's byte; the palette lives in the attribute table
        {2, 0, 0, 8, 8, 3, 13, 14, 1, 0, 0},    // GBC: the tile map below the attribute map
        {2, 0, 0, 9, 11, 1, 9, 10, 1, 0, 0},    // SMS
        {2, 1, 0, 11, 13, 2, 11, 12, 1, 0, 0},  // Mega Drive
        {2, 0, 0, 10, 10, 3, 14, 15, 1, 0, 0},  // SNES
        {2, 0, 0, 10, 12, 4, 10, 11, 1, 0, 0},  // GBA, text backgrounds
    };
    if (!layout || machine < PAR_VRAM_NES || machine > PAR_VRAM_GBA) return PAR_ERR_INVALID_ARG;
    *layout = presets[machine];
    return PAR_OK;
}

int par_vram_encode_map_device(void* stream, const par_vram_map_layout* layout, const uint32_t* map, int gcx, int gcy,
                               const uint8_t* cells, int ratio_x, int ratio_y, uint8_t* out, uint32_t* bad_out) {
    if (!map_args_ok(layout, map, gcx, gcy, ratio_x, ratio_y, out) || !aligned4(bad_out)) return PAR_ERR_INVALID_ARG;
    return launch_encode_map((hipStream_t)stream, layout, map, gcx, gcy, cells, ratio_x, ratio_y, out, bad_out) == hipSuccess
               ? PAR_OK
               : PAR_ERR_HIP;
}

size_t par_vram_palette_words(const uint8_t* palette, int n, int format, uint8_t* out) {
    if (!palette || !out || n < 1 || n > 256 || format < PAR_VRAM_BGR555 || format > PAR_VRAM_BGR222) return 0;
    uint8_t* o = out;
    for (int i = 0; i < n; i++) {
        const uint32_t r = palette[4 * i], g = palette[4 * i + 1], b = palette[4 * i + 2];
        if (format == PAR_VRAM_BGR555) {
            const uint32_t w = (r >> 3) | (g >> 3) << 5 | (b >> 3) << 10;
            *o++ = (uint8_t)w;
            *o++ = (uint8_t)(w >> 8);
        } else if (format == PAR_VRAM_BGR333_MD) {
            const uint32_t w = (r >> 5) << 1 | (g >> 5) << 5 | (b >> 5) << 9;
            *o++ = (uint8_t)(w >> 8);
            *o++ = (uint8_t)w;
        } else {
            *o++ = (uint8_t)((r >> 6) | (g >> 6) << 2 | (b >> 6) << 4);
        }
    }
    return (size_t)(o - out);
}

int par_vram_encode_tiles_host(int device, const uint8_t* tiles, int capacity, int count, int tile_w, int tile_h,
                               int format, uint8_t* out, int* bad) {
    if (!tiles_args_ok(tiles, capacity, tile_w, tile_h, format, out) || count < 0 || !bad) return PAR_ERR_INVALID_ARG;
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    const int n = std::min(count, capacity);
    if (n == 0) {
        *bad = 0;
        return PAR_OK;
    }
    hipError_t e = hipSetDevice(device);
    uint32_t n_bad = 0;
    par_device_buffer d_tiles(e, tiles, (size_t)n * (size_t)(tile_w * tile_h), true);
    par_device_buffer d_out(e, out, (size_t)n * par_vram_tile_bytes(format, tile_w, tile_h), false);
    par_device_buffer d_bad(e, &n_bad, sizeof(n_bad), false);
    // (the n tiles are the whole device set: no device count)
    if (e == hipSuccess) {
        e = launch_encode_tiles(nullptr, d_tiles.as<uint8_t>(), n, nullptr, tile_w, tile_h, format, d_out.as<uint8_t>(),
                                d_bad.as<uint32_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    d_out.download(out);
    d_bad.download(&n_bad);
    if (e == hipSuccess) *bad = (int)n_bad;
    return par_status_of(e);
}

int par_vram_decode_tiles_host(int device, const uint8_t* data, int n_tiles, int tile_w, int tile_h, int format,
                               uint8_t* tiles_out) {
    if (!tiles_args_ok(data, n_tiles, tile_w, tile_h, format, tiles_out)) return PAR_ERR_INVALID_ARG;
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    par_device_buffer d_data(e, data, (size_t)n_tiles * par_vram_tile_bytes(format, tile_w, tile_h), true);
    par_device_buffer d_tiles(e, tiles_out, (size_t)n_tiles * (size_t)(tile_w * tile_h), false);
    if (e == hipSuccess) e = launch_decode_tiles(nullptr, d_data.as<uint8_t>(), n_tiles, tile_w, tile_h, format, d_tiles.as<uint8_t>());
    if (e == hipSuccess) e = hipDeviceSynchronize();
    d_tiles.download(tiles_out);
    return par_status_of(e);
}

int par_vram_encode_map_host(int device, const par_vram_map_layout* layout, const uint32_t* map, int gcx, int gcy,
                             const uint8_t* cells, int ratio_x, int ratio_y, uint8_t* out, int* bad) {
    if (!map_args_ok(layout, map, gcx, gcy, ratio_x, ratio_y, out) || !bad) return PAR_ERR_INVALID_ARG;
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    const size_t n = (size_t)gcx * (size_t)gcy;
    const size_t colour_cells = (size_t)((gcx + ratio_x - 1) / ratio_x) * (size_t)((gcy + ratio_y - 1) / ratio_y);
    uint32_t n_bad = 0;
    par_device_buffer d_map(e, map, n * sizeof(uint32_t), true);
    par_device_buffer d_cells(e, cells, colour_cells, true);
    par_device_buffer d_out(e, out, n * (size_t)layout->word_bytes, false);
    par_device_buffer d_bad(e, &n_bad, sizeof(n_bad), false);
    if (e == hipSuccess) {
        e = launch_encode_map(nullptr, layout, d_map.as<uint32_t>(), gcx, gcy, d_cells.as<uint8_t>(), ratio_x, ratio_y,
                              d_out.as<uint8_t>(), d_bad.as<uint32_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    d_out.download(out);
    d_bad.download(&n_bad);
    if (e == hipSuccess) *bad = (int)n_bad;
    return par_status_of(e);
}

}  // extern "C"
