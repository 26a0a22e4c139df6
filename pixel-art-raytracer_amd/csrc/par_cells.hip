// par_cells.hip — colour cells: a frame quantised under per-cell sub-palettes (par_quantize_cells_device,
// par_quantize_cells_host), and the sub-palettes of the any-two-colours mode (par_cells_pairs). The contract is beside
// the declarations in par_cells.h; nothing here knows a par_context, and the statuses are par_raytracer.h's.
//
// The kernel. A lane takes FOUR consecutive pixels of one row of a cell, as quantize_kernel's lanes do, so that the scalar
// side of the search (the entries' loads and masks, the loop) is paid once for four pixels. A cell is then 16, 32 or 64
// lanes: an 8 x 8 cell is exactly one ROW of 16 lanes, the unit of the DPP row operations, 8 x 16 and 16 x 8 cells are two
// rows and a 16 x 16 cell is the wavefront. A workgroup of 256 threads takes the 16, 8 or 4 cells that lie side by side in
// one cell row. Nothing is divided: the cell sizes are template arguments and powers of two. There is no LDS, no barrier,
// no atomic and no flag: a cell's output is a function of its input alone, computed by the cell's own lanes.
//   Pass 1: the sub-palette index is wave-uniform, so the entries come through the scalar cache, eight at a time. Only
//           distances are wanted: one v_sad_u8 an entry and pixel, v_min3_u32 takes two. For a PAIR of sub-palettes
//           (2q, 2q + 1) a lane adds its four pixels' two distances in the halves of one word (64 pixels x 765 = 48 960
//           fits 16 bits; a pixel that does not exist adds 0), and four DPP steps (two quad permutes, the half-row and
//           the row mirror) leave every lane of a row with the row's sum: for an 8 x 8 cell that is E(2q) and E(2q + 1).
//           The larger cells add their two or four rows through ds_bpermute, half by half (a 16 x 16 cell's E needs 18
//           bits). Every lane of a cell then holds the same sums and keeps the minimum of (E(s) << 8) | s: s*.
//   Pass 2: the K-entry search once more, for s* alone, with v_sad_hi_u8's (L1 distance << 16) + k as in quantize_kernel.
//           Where every cell of the wavefront chose the same sub-palette (always, for a 16 x 16 cell or with S = 1) its
//           entries come through the scalar cache again; else every lane reads its own cell's entries.
//   A lane loads its own pixels before the passes and stores nothing but those pixels, so fb_out == fb holds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_cells.h"
#include "par_cells_lanes.h"
#include "par_hostcall.h"
#include "par_post.h"
#include "par_raytracer.h"

namespace {

constexpr int CELLS_THREADS = 256;

// The planes address the launch's first row, `row_begin` is that row's absolute number and `rows` the launch's rows;
// blockIdx.y is the cell row within the launch, blockIdx.x the group of CELLS cells within it.
template <int CW, int CH, bool DITHER>
__global__ __launch_bounds__(CELLS_THREADS) void cells_kernel(const uint32_t* fb, uint32_t* fb_out, uint8_t* index_out,
                                                              uint8_t* cell_out, const uint32_t* __restrict__ palette,
                                                              int n_sub, int sub_size, uint32_t width, uint32_t rows,
                                                              uint32_t gcx, uint32_t row_begin, int spread) {
    static_assert((CW == 8 || CW == 16) && (CH == 8 || CH == 16), "a cell is 1, 2 or 4 rows of 16 lanes");
    constexpr int LANES = CW * CH / 4, QUADS = CW / 4, CELLS = CELLS_THREADS / LANES;

    const uint32_t t = threadIdx.x, j = t % LANES;
    const uint32_t cx = blockIdx.x * (uint32_t)CELLS + t / LANES;
    const uint32_t x0 = cx * CW + (j % QUADS) * 4u, y = blockIdx.y * (uint32_t)CH + j / QUADS;  // (y: within the launch)
    const size_t at = (size_t)y * width + x0;
    bool live[4];
    uint32_t src[4], rgb[4];
    for (int i = 0; i < 4; i++) {
        live[i] = y < rows && x0 + i < width;
        src[i] = live[i] ? fb[at + i] : 0u;
        rgb[i] = DITHER ? dithered(src[i], x0 + i, row_begin + y, spread) : src[i] & QUANT_RGB;
    }

    // pass 1: E(s) of the cell a pair of sub-palettes at a time, and the minimum of (E(s) << 8) | s (every branch here
    // is on kernel arguments: all 64 lanes reach the cross-lane steps)
    uint32_t best = ~0u;
    for (int s = 0; s < n_sub; s += 2) {
        const bool two = s + 1 < n_sub;
        uint32_t d0[4], d1[4] = {0u, 0u, 0u, 0u};
        nearest_distances(rgb, palette + s * sub_size, sub_size, d0);
        if (two) nearest_distances(rgb, palette + (s + 1) * sub_size, sub_size, d1);
        uint32_t w = 0;
        for (int i = 0; i < 4; i++) w += live[i] ? d0[i] | (d1[i] << 16) : 0u;
        uint32_t even, odd;
        cell_sums<LANES>(row_sum(w), even, odd);
        best = std::min(best, (even << 8) | (uint32_t)s);
        if (two) best = std::min(best, (odd << 8) | (uint32_t)(s + 1));
    }
    const uint32_t chosen = best & 0xFFu;

    // pass 2: quantize_kernel's search over the chosen sub-palette
    uint32_t key[4] = {~0u, ~0u, ~0u, ~0u};
    const uint32_t shared = (uint32_t)__builtin_amdgcn_readfirstlane((int)chosen);
    if (LANES == 64 || __ballot(chosen != shared) == 0) {
        const uint32_t* __restrict__ sub = palette + shared * (uint32_t)sub_size;
        int k = 0;
        for (; k + 8 <= sub_size; k += 8) {
            uint32_t e[8];
            for (int n = 0; n < 8; n++) e[n] = sub[k + n] & QUANT_RGB;
            for (int n = 0; n < 8; n += 2) {
                for (int i = 0; i < 4; i++) {
                    key[i] = min3u(key[i], __builtin_amdgcn_sad_hi_u8(rgb[i], e[n], (uint32_t)(k + n)),
                                   __builtin_amdgcn_sad_hi_u8(rgb[i], e[n + 1], (uint32_t)(k + n + 1)));
                }
            }
        }
        for (; k < sub_size; k++) {
            const uint32_t e = sub[k] & QUANT_RGB;
            for (int i = 0; i < 4; i++) key[i] = std::min(key[i], __builtin_amdgcn_sad_hi_u8(rgb[i], e, (uint32_t)k));
        }
    } else {
        const uint32_t* __restrict__ sub = palette + chosen * (uint32_t)sub_size;  // this lane's cell's
        for (int k = 0; k < sub_size; k++) {
            const uint32_t e = sub[k] & QUANT_RGB;
            for (int i = 0; i < 4; i++) key[i] = std::min(key[i], __builtin_amdgcn_sad_hi_u8(rgb[i], e, (uint32_t)k));
        }
    }

    for (int i = 0; i < 4; i++) {
        if (!live[i]) continue;
        const uint32_t index = chosen * (uint32_t)sub_size + (key[i] & 0xFFFFu);
        if (index_out) index_out[at + i] = (uint8_t)index;
        if (fb_out) fb_out[at + i] = (palette[index] & QUANT_RGB) | (src[i] & ~QUANT_RGB);
    }
    if (cell_out && j == 0 && cx < gcx) cell_out[(size_t)blockIdx.y * gcx + cx] = (uint8_t)chosen;
}

struct CellsCall {
    const par_color* palette;
    int n_sub, sub_size, spread, width;
    const par_color* fb;
    int row_begin, row_end;
    par_color* fb_out;
    uint8_t* index_out;
    uint8_t* cell_out;
};

// Rows [row_begin, row_end) in launches of whole cell rows (par_tile_row_cuts: one launch for any frame below 2^31
// pixels and 65535 cell rows).
template <int CW, int CH, bool DITHER>
hipError_t launch_cells(hipStream_t stream, const CellsCall& c) {
    const uint32_t W = (uint32_t)c.width, gcx = (W + CW - 1) / CW;
    constexpr uint32_t CELLS = CELLS_THREADS / (CW * CH / 4);  // four pixels a lane
    return (hipError_t)par_tile_row_cuts(c.row_begin, c.row_end, W, CH, [&](int ra, int rb, uint32_t cell_rows) {
        const size_t at = (size_t)(ra - c.row_begin) * W;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(c.fb) + at;
        uint32_t* dst = c.fb_out ? reinterpret_cast<uint32_t*>(c.fb_out) + at : nullptr;
        uint8_t* idx = c.index_out ? c.index_out + at : nullptr;
        uint8_t* cells = c.cell_out ? c.cell_out + (size_t)((ra - c.row_begin) / CH) * gcx : nullptr;
        hipLaunchKernelGGL((cells_kernel<CW, CH, DITHER>), dim3((gcx + CELLS - 1) / CELLS, cell_rows), dim3(CELLS_THREADS),
                           0, stream, src, dst, idx, cells, reinterpret_cast<const uint32_t*>(c.palette), c.n_sub,
                           c.sub_size, W, (uint32_t)(rb - ra), gcx, (uint32_t)ra, c.spread);
        return (int)hipGetLastError();
    });
}

template <int CW, int CH>
hipError_t launch_cells(hipStream_t stream, const CellsCall& c) {
    return c.spread != 0 ? launch_cells<CW, CH, true>(stream, c) : launch_cells<CW, CH, false>(stream, c);
}

hipError_t launch_cells(hipStream_t stream, int cell_w, int cell_h, const CellsCall& c) {
    if (cell_w == 8) return cell_h == 8 ? launch_cells<8, 8>(stream, c) : launch_cells<8, 16>(stream, c);
    return cell_h == 8 ? launch_cells<16, 8>(stream, c) : launch_cells<16, 16>(stream, c);
}

bool cells_args_ok(const par_params* p, const par_color* palette, int n_sub, int sub_size, int cell_w, int cell_h,
                   int spread, const par_color* fb, int row_begin, int row_end, const par_color* fb_out,
                   const uint8_t* index_out) {
    if (!p || !palette || !fb || (!fb_out && !index_out)) return false;
    if (n_sub < 1 || sub_size < 1 || (int64_t)n_sub * sub_size > PAR_MAX_PALETTE) return false;
    if ((cell_w != 8 && cell_w != 16) || (cell_h != 8 && cell_h != 16) || spread < 0 || spread > 255) return false;
    if (p->width <= 0 || row_begin < 0 || row_begin >= row_end || row_end > p->height) return false;
    return row_begin % cell_h == 0 && (row_end % cell_h == 0 || row_end == p->height);
}

}  // namespace

extern "C" {

int par_quantize_cells_device(const par_params* params, void* stream, const par_color* d_palette, int n_sub,
                              int sub_size, int cell_w, int cell_h, int spread, const par_color* fb, int row_begin,
                              int row_end, par_color* fb_out, uint8_t* index_out, uint8_t* cell_out) {
    if (!cells_args_ok(params, d_palette, n_sub, sub_size, cell_w, cell_h, spread, fb, row_begin, row_end, fb_out,
                       index_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    const CellsCall c{d_palette, n_sub, sub_size, spread, params->width, fb, row_begin, row_end, fb_out, index_out, cell_out};
    return launch_cells((hipStream_t)stream, cell_w, cell_h, c) == hipSuccess ? PAR_OK : PAR_ERR_HIP;
}

int par_quantize_cells_host(const par_params* params, int device, const par_color* palette, int n_sub, int sub_size,
                            int cell_w, int cell_h, int spread, const par_color* fb, int row_begin, int row_end,
                            par_color* fb_out, uint8_t* index_out, uint8_t* cell_out) {
    if (!cells_args_ok(params, palette, n_sub, sub_size, cell_w, cell_h, spread, fb, row_begin, row_end, fb_out,
                       index_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    const size_t n = (size_t)(row_end - row_begin) * (size_t)params->width;
    const size_t n_cells = (size_t)((params->width + cell_w - 1) / cell_w) * (size_t)((row_end - row_begin + cell_h - 1) / cell_h);
    // the device copy of fb is quantised in place when fb_out is asked for
    par_device_buffer d_palette(e, palette, (size_t)n_sub * (size_t)sub_size * sizeof(par_color), true);
    par_device_buffer d_fb(e, fb, n * sizeof(par_color), true), d_index(e, index_out, n, false);
    par_device_buffer d_cells(e, cell_out, n_cells, false);
    if (e == hipSuccess) {
        const CellsCall c{d_palette.as<par_color>(), n_sub, sub_size, spread, params->width, d_fb.as<par_color>(), row_begin,
                          row_end, fb_out ? d_fb.as<par_color>() : nullptr, d_index.as<uint8_t>(), d_cells.as<uint8_t>()};
        e = launch_cells(nullptr, cell_w, cell_h, c);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (fb_out) d_fb.download(fb_out);
    d_index.download(index_out);
    d_cells.download(cell_out);
    return par_status_of(e);
}

int par_cells_pairs(const par_color* palette, int n_colors, par_color* out, int capacity) {
    if (!palette || !out || capacity < 0 || n_colors < 2 || n_colors > 16) return -PAR_ERR_INVALID_ARG;
    int at = 0;
    for (int i = 0; i < n_colors; i++) {
        for (int j = i + 1; j < n_colors; j++, at += 2) {
            if (at < capacity) out[at] = palette[i];
            if (at + 1 < capacity) out[at + 1] = palette[j];
        }
    }
    return at / 2;
}

}  // extern "C"
