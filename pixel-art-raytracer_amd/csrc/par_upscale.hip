// par_upscale.hip — the pixel-art scalers: a frame or an index plane magnified 2, 3 or 4 times by Scale2x, Scale3x or
// Scale4x onto a surface, an index plane or both (par_upscale_device, par_upscale_host). The contract is beside the
// declarations in par_raytracer.h and the rules themselves are in par_post.h; nothing here knows a par_context, and the
// render kernels (par_kernels.hip) know nothing of this.
//
// The kernel. Like present the pass writes k * k times what it reads, so it is laid out by its stores; unlike present
// an output pixel depends on a 3 x 3 neighbourhood, so a workgroup first stages a tile of UP_TW x UP_TH source
// elements with its halo in LDS, one word an element (an index byte widened, a frame's word already exchanged for a
// BGRA surface: an exchange keeps words apart that were apart). The clamps at the frame's and the block's edges are
// applied there, once per staged element, and no rule clamps again. For Scale4x the workgroup then computes the tile
// of the intermediate 2x plane T, with a halo of one element and T's own clamps, from the staged source into LDS, and
// the last pass is Scale2x on that tile: T is never in memory. With an index source and a surface the palette sits in
// 1 KiB of LDS, entry i being palette[min(i, n_colors - 1)] in the surface's byte order, as in present_kernel.
// The last pass: a lane takes a GROUP of 4 consecutive output pixels of the kk output rows of one row of the plane it
// reads (kk = 3 for Scale3x, else 2): 16 bytes a row, on a 16-byte boundary when `out` and the pitch are. A group lies
// over exactly two elements of that row, so the lane reads a 3 x 4 window from LDS once, computes both blocks and
// stores kk times 16 bytes; neighbouring lanes store neighbouring 16 bytes of one output row. The group that hangs
// over a row's end, and every group when `out` or the pitch is off the 16-byte phase, goes pixel by pixel. The index
// output of a group is one word where index_out and the scaled width allow, else bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_hostcall.h"
#include "par_post.h"
#include "par_raytracer.h"

namespace {

constexpr int UP_THREADS = 256;
constexpr int UP_TW = 128;  // source columns of a workgroup's tile
constexpr int UP_TH = 4;    // source rows of it
// Tiles of one launch: the grid's y stays below 2^16 and its thread count below 2^32 (a frame wider than 2^24 tiles'
// worth of columns aside, which no pitch can name).
constexpr uint32_t UP_MAX_TILES = 1u << 24, UP_MAX_TILE_ROWS = 65535;

struct UpscaleArgs {
    const void* src;          // (s0, column 0)
    const uint32_t* palette;  // null without a surface from an index source
    int n_colors;
    char* out;           // (k * r0, byte 0), nullable
    uint8_t* index_out;  // (k * r0, column 0), nullable
    int width, s0, s1, r0, r1;
    size_t pitch;
    bool swap;         // BGRA
    bool index_words;  // index_out on a 4-byte boundary and k * width a multiple of 4
    uint32_t first_tile_row;  // of this launch
};

// one element of a Scale2x block picked by its position in the block
__device__ __forceinline__ uint32_t scale2x_at(const uint32_t* p, int stride, int sx, int sy) {
    uint32_t o[4];
    scale2x_block(p[-stride], p[-1], p[0], p[1], p[stride], o);
    const uint32_t top = sx ? o[1] : o[0], bottom = sx ? o[3] : o[2];
    return sy ? bottom : top;
}

// INDEXED: `src` is an index plane (bytes); else a frame (words). K: the factor. VEC: `out` and `pitch` are multiples
// of 16 (without a surface VEC is false).
template <bool INDEXED, int K, bool VEC>
__global__ __launch_bounds__(UP_THREADS) void upscale_kernel(const UpscaleArgs a) {
    constexpr int HALO = K == 4 ? 2 : 1;  // source elements round the tile
    constexpr int SW = UP_TW + 2 * HALO, SH = UP_TH + 2 * HALO;
    constexpr int M = K == 4 ? 2 : 1;     // the plane of the last pass is M times the source: T for Scale4x
    constexpr int KK = K == 4 ? 2 : K;    // the factor of the last pass
    constexpr int PW = M * UP_TW + 2, PH = M * UP_TH + 2;  // that plane's tile with its halo of one
    constexpr int GROUPS = KK * M * UP_TW / 4, ITEMS = GROUPS * M * UP_TH;
    static_assert((KK * M * UP_TW) % 4 == 0, "a tile's output row is whole groups");

    __shared__ uint32_t pal[PAR_MAX_PALETTE];
    __shared__ uint32_t staged[SH * SW + 1];  // and a word that takes what no one reads
    __shared__ uint32_t mid[K == 4 ? PH * PW : 1];

    const uint32_t tx = blockIdx.x, ty = a.first_tile_row + blockIdx.y;
    const int64_t x0 = (int64_t)tx * UP_TW, y0 = (int64_t)a.r0 + (int64_t)ty * UP_TH;  // the tile's first source element
    const int64_t width = a.width;

    // The source tile with its halo: the clamps of the contract, once per element. A thread keeps its column (the first
    // 2 * HALO threads of a row the halo's columns past the tile's UP_TW as well) and the two halves of the workgroup
    // take alternate rows: a column's clamp is computed once, a row's once per row. Every load of a thread is issued
    // before the first is waited for (a workgroup lives as long as its dependent trips to memory take): no load sits
    // behind a branch, so every thread loads a far column too, clamped like any other; only the first 2 * HALO keep it,
    // the others write theirs to the word past the tile.
    static_assert(UP_THREADS == 2 * UP_TW && SH % 2 == 0, "two rows of the tile per pass of the workgroup");
    {
        const int lane = threadIdx.x % UP_TW, half = threadIdx.x / UP_TW;
        const uint32_t last = (uint32_t)a.width - 1u, first = (uint32_t)x0 + (uint32_t)lane;  // (below 2^31 + SW)
        const uint32_t col = std::min(std::max(first, (uint32_t)HALO) - HALO, last);
        const uint32_t far_col = std::min(first + UP_TW - HALO, last);  // column UP_TW + lane of the tile
        uint32_t v[SH / 2], far[SH / 2];
#pragma unroll
        for (int pass = 0; pass < SH / 2; pass++) {
            const int64_t row = std::min(std::max<int64_t>(y0 - HALO + 2 * pass + half, a.s0), (int64_t)a.s1 - 1);
            const size_t at = (size_t)(row - a.s0) * (size_t)width;
            if (INDEXED) {
                const uint8_t* const s = static_cast<const uint8_t*>(a.src) + at;
                v[pass] = s[col];
                far[pass] = s[far_col];
            } else {
                const uint32_t* const s = static_cast<const uint32_t*>(a.src) + at;
                v[pass] = s[col];
                far[pass] = s[far_col];
            }
        }
        // (the palette's entry is loaded behind the tile's loads and before their waits: one trip to memory, not two)
        static_assert(UP_THREADS == PAR_MAX_PALETTE, "one palette entry per thread");
        uint32_t entry = 0;
        if (INDEXED && a.out) entry = palette_entry_load(a.palette, a.n_colors);
#pragma unroll
        for (int pass = 0; pass < SH / 2; pass++) {
            const int j = 2 * pass + half;
            const bool swap = !INDEXED && a.swap;
            staged[j * SW + lane] = swap ? exchanged(v[pass]) : v[pass];
            staged[lane < 2 * HALO ? j * SW + UP_TW + lane : SH * SW] = swap ? exchanged(far[pass]) : far[pass];
        }
        if (INDEXED) pal[threadIdx.x] = a.swap ? exchanged(entry) : entry;
    }
    __syncthreads();

    if constexpr (K == 4) {
        // T's tile with a halo of one: T's own clamps, then the element of the Scale2x block of the source element
        // under it. Column X / 2 lies in [x0 - 1, x0 + UP_TW] and its neighbours in the staged tile (HALO 2); rows
        // alike. A thread keeps its column of T, so X's clamp is computed once and Y's is the same for the whole
        // workgroup; the two columns past the workgroup's 256 are one element each for 2 * PH threads of the second
        // wavefront (on one thread they would double the time every other thread waits for at the barrier).
        static_assert(PW == UP_THREADS + 2 || K != 4, "a column of T's tile per thread, and two more");
        const auto t_element = [&](int i, int j) {
            const int64_t X = std::min(std::max<int64_t>(2 * x0 - 1 + i, 0), 2 * width - 1);
            const int64_t Y = std::min(std::max<int64_t>(2 * y0 - 1 + j, 2 * (int64_t)a.s0), 2 * (int64_t)a.s1 - 1);
            const int c = (int)((X >> 1) - (x0 - HALO)), r = (int)((Y >> 1) - (y0 - HALO));
            mid[j * PW + i] = scale2x_at(&staged[r * SW + c], SW, (int)(X & 1), (int)(Y & 1));
        };
        {
            const int i = threadIdx.x;
            const int64_t X = std::min(std::max<int64_t>(2 * x0 - 1 + i, 0), 2 * width - 1);
            const int c = (int)((X >> 1) - (x0 - HALO)), sx = (int)(X & 1);
            for (int j = 0; j < PH; j++) {
                const int64_t Y = std::min(std::max<int64_t>(2 * y0 - 1 + j, 2 * (int64_t)a.s0), 2 * (int64_t)a.s1 - 1);
                const int r = (int)((Y >> 1) - (y0 - HALO));
                mid[j * PW + i] = scale2x_at(&staged[r * SW + c], SW, sx, (int)(Y & 1));
            }
            const int extra = (int)threadIdx.x - 64;
            if (extra >= 0 && extra < 2 * PH) t_element(UP_THREADS + extra / PH, extra % PH);
        }
        __syncthreads();
    }
    const uint32_t* const plane = K == 4 ? mid : staged;
    constexpr int STRIDE = K == 4 ? PW : SW;
    constexpr int EDGE = K == 4 ? 1 : HALO;  // the halo of `plane`

    const uint64_t out_width = (uint64_t)K * (uint64_t)width;
    const int64_t plane_rows_end = (int64_t)M * a.r1;
    for (int it = threadIdx.x; it < ITEMS; it += UP_THREADS) {
        const int prow = it / GROUPS, g = it - prow * GROUPS;
        const int64_t py = M * y0 + prow;  // the row of the plane, absolute
        const uint64_t X0 = (uint64_t)(KK * M) * (uint64_t)x0 + 4u * (uint32_t)g;  // the group's first output pixel
        if (py >= plane_rows_end || X0 >= out_width) continue;
        const int c0 = 4 * g / KK, phase = 4 * g - KK * c0;  // the group's first element of the row, and where in it
        const uint32_t* const w = &plane[(prow + EDGE - 1) * STRIDE + c0 + EDGE - 1];
        uint32_t n[3][4];
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 4; c++) n[r][c] = w[r * STRIDE + c];
        }
        uint32_t e[KK][4];  // the group's elements, output row by output row
        if (KK == 2) {
            uint32_t b0[4], b1[4];
            scale2x_block(n[0][1], n[1][0], n[1][1], n[1][2], n[2][1], b0);
            scale2x_block(n[0][2], n[1][1], n[1][2], n[1][3], n[2][2], b1);
            for (int sy = 0; sy < 2; sy++) {
                e[sy][0] = b0[2 * sy]; e[sy][1] = b0[2 * sy + 1]; e[sy][2] = b1[2 * sy]; e[sy][3] = b1[2 * sy + 1];
            }
        } else {
            uint32_t b0[9], b1[9];
            scale3x_block(n[0][0], n[0][1], n[0][2], n[1][0], n[1][1], n[1][2], n[2][0], n[2][1], n[2][2], b0);
            scale3x_block(n[0][1], n[0][2], n[0][3], n[1][1], n[1][2], n[1][3], n[2][1], n[2][2], n[2][3], b1);
            // the six elements of the two blocks' row, of which the group takes four from `phase` on (selects: a
            // run-time index would put the array in scratch)
            for (int sy = 0; sy < KK; sy++) {
                const uint32_t q0 = b0[3 * sy], q1 = b0[3 * sy + 1], q2 = b0[3 * sy + 2];
                const uint32_t q3 = b1[3 * sy], q4 = b1[3 * sy + 1], q5 = b1[3 * sy + 2];
                e[sy][0] = phase == 0 ? q0 : (phase == 1 ? q1 : q2);
                e[sy][1] = phase == 0 ? q1 : (phase == 1 ? q2 : q3);
                e[sy][2] = phase == 0 ? q2 : (phase == 1 ? q3 : q4);
                e[sy][3] = phase == 0 ? q3 : (phase == 1 ? q4 : q5);
            }
        }
        const bool full = X0 + 4u <= out_width;
        const size_t out_row = (size_t)(KK * py - (int64_t)K * a.r0);  // from the first output row of the call
        if (a.out) {
            char* const dst = a.out + out_row * a.pitch + 4u * (size_t)X0;
            for (int sy = 0; sy < KK; sy++) {
                uint32_t c[4];
                for (int i = 0; i < 4; i++) c[i] = INDEXED ? pal[e[sy][i]] : e[sy][i];
                if (VEC && full) {
                    const u32x4 v = {c[0], c[1], c[2], c[3]};
                    *reinterpret_cast<u32x4*>(dst + sy * a.pitch) = v;
                } else {
                    uint32_t* const o = reinterpret_cast<uint32_t*>(dst + sy * a.pitch);
                    for (int i = 0; i < 4; i++) {
                        if (X0 + i < out_width) o[i] = c[i];
                    }
                }
            }
        }
        if (INDEXED && a.index_out) {
            uint8_t* const dst = a.index_out + out_row * (size_t)out_width + (size_t)X0;
            for (int sy = 0; sy < KK; sy++) {
                uint8_t* const o = dst + sy * (size_t)out_width;
                if (a.index_words) {  // (then every group is full)
                    *reinterpret_cast<uint32_t*>(o) = e[sy][0] | (e[sy][1] << 8) | (e[sy][2] << 16) | (e[sy][3] << 24);
                } else {
                    for (int i = 0; i < 4; i++) {
                        if (X0 + i < out_width) o[i] = (uint8_t)e[sy][i];
                    }
                }
            }
        }
    }
}

// One launch per run of whole tile rows: a workgroup finds its tile in blockIdx, with no division.
template <bool INDEXED, int K, bool VEC>
hipError_t launch_tiles(hipStream_t stream, UpscaleArgs a, uint32_t tiles_x, uint32_t tile_rows) {
    const uint32_t rows_per_launch = std::max(1u, std::min(UP_MAX_TILE_ROWS, (UP_MAX_TILES - 1u) / tiles_x));
    for (uint32_t first = 0; first < tile_rows; first += rows_per_launch) {
        a.first_tile_row = first;
        const uint32_t rows = std::min(rows_per_launch, tile_rows - first);
        hipLaunchKernelGGL((upscale_kernel<INDEXED, K, VEC>), dim3(tiles_x, rows), dim3(UP_THREADS), 0, stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <bool INDEXED, bool VEC>
hipError_t launch_factor(hipStream_t stream, int k, const UpscaleArgs& a, uint32_t tiles_x, uint32_t tile_rows) {
    if (k == PAR_UPSCALE_SCALE2X) return launch_tiles<INDEXED, 2, VEC>(stream, a, tiles_x, tile_rows);
    if (k == PAR_UPSCALE_SCALE3X) return launch_tiles<INDEXED, 3, VEC>(stream, a, tiles_x, tile_rows);
    return launch_tiles<INDEXED, 4, VEC>(stream, a, tiles_x, tile_rows);
}

hipError_t launch_upscale(hipStream_t stream, const par_upscale_desc& d, int width, const par_color* fb,
                          const uint8_t* index, const par_color* d_palette, int n_colors, int s0, int s1, int r0, int r1,
                          void* out, uint8_t* index_out) {
    UpscaleArgs a;
    a.src = index ? static_cast<const void*>(index) : static_cast<const void*>(fb);
    a.palette = reinterpret_cast<const uint32_t*>(d_palette);
    a.n_colors = n_colors;
    a.out = static_cast<char*>(out);
    a.index_out = index_out;
    a.width = width; a.s0 = s0; a.s1 = s1; a.r0 = r0; a.r1 = r1;
    a.pitch = out ? (size_t)d.pitch : 0;
    a.swap = out && d.order == PAR_PRESENT_BGRA;
    a.index_words = index_out && (reinterpret_cast<uintptr_t>(index_out) & 3u) == 0 &&
                    (((uint64_t)d.scaler * (uint64_t)width) & 3u) == 0;
    a.first_tile_row = 0;
    const uint32_t tiles_x = ((uint32_t)width + UP_TW - 1) / UP_TW, tile_rows = ((uint32_t)(r1 - r0) + UP_TH - 1) / UP_TH;
    const bool vec = out && (reinterpret_cast<uintptr_t>(out) & 15u) == 0 && (d.pitch & 15) == 0;
    if (index) {
        return vec ? launch_factor<true, true>(stream, d.scaler, a, tiles_x, tile_rows)
                   : launch_factor<true, false>(stream, d.scaler, a, tiles_x, tile_rows);
    }
    return vec ? launch_factor<false, true>(stream, d.scaler, a, tiles_x, tile_rows)
               : launch_factor<false, false>(stream, d.scaler, a, tiles_x, tile_rows);
}

bool upscale_args_ok(const par_params* p, const par_upscale_desc* d, const par_color* fb, const uint8_t* index,
                     const par_color* palette, int n_colors, int s0, int s1, int r0, int r1, const void* out,
                     const uint8_t* index_out) {
    if (!p || !d || (fb != nullptr) == (index != nullptr)) return false;
    if ((!out && !index_out) || (fb && index_out)) return false;
    if (index && out) {
        if (!palette || n_colors < 1 || n_colors > PAR_MAX_PALETTE) return false;
    } else if (palette || n_colors != 0) {
        return false;
    }
    if (d->scaler != PAR_UPSCALE_SCALE2X && d->scaler != PAR_UPSCALE_SCALE3X && d->scaler != PAR_UPSCALE_SCALE4X) return false;
    if (p->width <= 0 || s0 < 0 || s0 > r0 || r0 >= r1 || r1 > s1 || s1 > p->height) return false;
    if (!out) return true;  // the pitch and the order are a surface's
    if (d->order != PAR_PRESENT_RGBA && d->order != PAR_PRESENT_BGRA) return false;
    // (a pitch is an int32: a row of more bytes than that has no valid pitch)
    return (d->pitch & 3) == 0 && (int64_t)d->pitch >= 4 * (int64_t)p->width * (int64_t)d->scaler;
}

}  // namespace

extern "C" {

int par_upscale_device(const par_params* params, void* stream, const par_upscale_desc* desc, const par_color* fb,
                       const uint8_t* index, const par_color* d_palette, int n_colors, int src_row_begin, int src_row_end,
                       int row_begin, int row_end, void* out, uint8_t* index_out) {
    if (!upscale_args_ok(params, desc, fb, index, d_palette, n_colors, src_row_begin, src_row_end, row_begin, row_end, out, index_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    const hipError_t e = launch_upscale((hipStream_t)stream, *desc, params->width, fb, index, d_palette, n_colors,
                                        src_row_begin, src_row_end, row_begin, row_end, out, index_out);
    return e == hipSuccess ? PAR_OK : PAR_ERR_HIP;
}

int par_upscale_host(const par_params* params, int device, const par_upscale_desc* desc, const par_color* fb,
                     const uint8_t* index, const par_color* palette, int n_colors, int src_row_begin, int src_row_end,
                     int row_begin, int row_end, void* out, uint8_t* index_out) {
    if (!upscale_args_ok(params, desc, fb, index, palette, n_colors, src_row_begin, src_row_end, row_begin, row_end, out, index_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    const size_t k = (size_t)desc->scaler;
    const size_t n = (size_t)(src_row_end - src_row_begin) * (size_t)params->width;
    const size_t out_rows = (size_t)(row_end - row_begin) * k;
    const size_t row_px = (size_t)params->width * k;
    par_device_buffer d_palette(e, palette, (size_t)n_colors * sizeof(par_color), true), d_index(e, index, n, true);
    par_device_buffer d_fb(e, fb, n * sizeof(par_color), true), d_out(e, out, out_rows * (size_t)desc->pitch, false);
    par_device_buffer d_index_out(e, index_out, out_rows * row_px, false);
    if (e == hipSuccess) {
        e = launch_upscale(nullptr, *desc, params->width, d_fb.as<par_color>(), d_index.as<uint8_t>(),
                           d_palette.as<par_color>(), n_colors, src_row_begin, src_row_end, row_begin, row_end,
                           d_out.as<void>(), d_index_out.as<uint8_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    // a pitched copy: the caller's gap bytes stay as they are
    if (e == hipSuccess && out) e = hipMemcpy2D(out, (size_t)desc->pitch, d_out.as<void>(), (size_t)desc->pitch, 4 * row_px, out_rows, hipMemcpyDeviceToHost);
    d_index_out.download(index_out);
    return par_status_of(e);
}

}  // extern "C"
