// par_finish.hip — finish: outline, quantise and present a frame in one launch (par_finish_device, par_finish_host). The
// contract is beside the declarations in par_raytracer.h and is the composition of the three passes' contracts, byte for
// byte; nothing here knows a par_context, and the three passes (par_outline.hip, par_quantize.hip, par_present.hip) know
// nothing of this. The per-pixel arithmetic, the tile's geometry and the group expand are the three passes' own, shared
// through par_post.h; the stage and the search are restated here (as functions of that header they compiled to other,
// slower code in both kernels: DESIGN, "Post passes").
//
// The kernel. A workgroup of 256 threads takes the outline pass's tile of 64 x 16 source pixels (par_post.h).
// OUTLINE: the tile's texels plus the one-texel halo are staged into LDS exactly as outline_kernel stages them (16-byte
// units aligned in memory, the LDS phase equal to the memory phase, one barrier), and a wavefront classifies four tile
// rows, lane = column. The lane's four fb pixels are scaled by class.
// QUANT: the four pixels are dithered on their absolute row and column and searched as quantize_kernel searches: the
// palette index is wave-uniform, the entries come through the scalar cache eight at a time, v_sad_hi_u8 keys go under
// v_min3_u32. The index goes to index_out from registers (four lanes' bytes as one dword where the plane's placement
// allows). The pixel's final word is an entry of the palette as the workgroup holds it in 1 KiB of LDS, exchanged under
// BGRA once per workgroup as present_kernel does; without QUANT it is the scaled pixel, exchanged under BGRA.
// The final words go into a 64 x 16 colour tile in LDS (4 KiB, beside the staged texels). Second barrier.
// Expand: the tile's surface region is 64 * sx x 16 * sy pixels. A wavefront expands the four tile rows it classified:
// 64 * sx groups of four output pixels in sx rounds, a lane's group lying in one source row. It reads the group's at
// most four colour words from LDS and stores them as present_kernel does (group_columns, store_group). A tile starts
// at byte 256 * sx * (tile column) of a row, so every full group is 16-byte aligned when `out` and the pitch are (VEC);
// the group that hangs over W', and every group otherwise, goes pixel by pixel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_fastdiv.h"
#include "par_hostcall.h"
#include "par_post.h"
#include "par_raytracer.h"

namespace {

constexpr int TILE_W = OUTLINE_TILE_W, TILE_H = OUTLINE_TILE_H, THREADS = OUTLINE_THREADS;
constexpr int ROWS_PER_WAVE = OUTLINE_ROWS_PER_WAVE, WAVES = OUTLINE_WAVES;
static_assert(THREADS == PAR_MAX_PALETTE, "one palette entry per thread");

struct FinishArgs {
    const uint32_t* gbuf;  // dwords of the G-buffer plane, row g0 at index 0 (OUTLINE)
    const uint32_t* fb;    // fb and index_out address (ra, 0)
    uint8_t* index_out;
    char* out;             // output row ra * sy, byte 0
    uint32_t width;
    int g0, g1;   // G-buffer rows: neighbours outside are absent
    int ra, rb;   // rows of this launch
    uint32_t background;  // w3 of the background texel
    int depth_step, silhouette_scale, crease_scale;
    int n_colors, spread;
    uint32_t sx, sy;
    par_udiv31 by_sx;
    size_t pitch;
    bool swap;
    bool index_wide;  // index_out on a 4-byte boundary and the width a multiple of 4
};

// OUTLINE: stage 1 runs (else no G-buffer is staged). QUANT: stage 2 runs (else no search). VEC: `out` and `pitch` are
// multiples of 16. (spread == 0 needs no variant: dithered() then leaves the three channels as they are.)
template <bool OUTLINE, bool QUANT, bool VEC>
__global__ __launch_bounds__(THREADS) void finish_kernel(FinishArgs a, const uint32_t* __restrict__ palette) {
    __shared__ u32x4 staged4[OUTLINE ? STAGED_H * STAGED_PITCH / 4 : 1];
    __shared__ uint32_t pal[QUANT ? PAR_MAX_PALETTE : 1];
    __shared__ uint32_t colour[TILE_H * TILE_W];
    uint32_t* staged = reinterpret_cast<uint32_t*>(staged4);

    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t W = a.width;
    const uint32_t tx0 = blockIdx.x * (uint32_t)TILE_W;
    const int ty0 = a.ra + (int)blockIdx.y * TILE_H;
    const int ly0 = wave * ROWS_PER_WAVE;
    const uint32_t px = tx0 + (uint32_t)lane;
    const bool in_cols = px < W;

    if (QUANT) {
        const uint32_t e = palette_entry_load(palette, a.n_colors);
        pal[threadIdx.x] = a.swap ? exchanged(e) : e;
    }

    uint32_t cls[ROWS_PER_WAVE] = {0u, 0u, 0u, 0u};
    uint32_t src[ROWS_PER_WAVE] = {0u, 0u, 0u, 0u};
    if (OUTLINE) {
        u32x4 v[STAGE_ROUNDS][UNIT_ROUNDS];
        const uint32_t galign = (uint32_t)(reinterpret_cast<uintptr_t>(a.gbuf) >> 2) & 3u;
        // ---- stage: staged row j holds absolute row ty0 - 1 + j, staged column c holds column tx0 - 1 + c ---------
        const uint32_t cx0 = tx0 == 0 ? 0u : tx0 - 1u;                    // the columns that exist
        const uint32_t cx1 = std::min(tx0 + (uint32_t)TILE_W + 1u, W);
        const int c0 = (int)(cx0 - (tx0 - 1u));                           // staged column of cx0: 0 or 1
        const int len = (int)(cx1 - cx0) * TEXEL_DWORDS;                  // dwords of a row's run
        // (a unit that hangs over an end of its run is loaded whole all the same, where its 16 bytes lie inside the
        // plane: what it brings along lands in LDS dwords of the row's own pitch that hold no texel of the tile. Only
        // the first and the last unit of the whole plane can go dword by dword.)
        const int64_t plane = (int64_t)(a.g1 - a.g0) * W * TEXEL_DWORDS;
        #pragma unroll
        for (int jj = 0; jj < STAGE_ROUNDS; jj++) {
            const int j = wave + WAVES * jj;
            const int r = ty0 - 1 + j;
            if (j >= STAGED_H || r < a.g0 || r >= a.g1) continue;  // (wave-uniform)
            const int64_t run = ((int64_t)(r - a.g0) * W + cx0) * TEXEL_DWORDS;  // the run's first dword
            const int ph = (int)((galign + (uint32_t)run) & 3u);                 // its phase in a 16-byte line of memory
            #pragma unroll
            for (int it = 0; it < UNIT_ROUNDS; it++) {
                const int n0 = 4 * (lane + 64 * it) - ph;  // unit: run dwords [n0, n0 + 4), 16-byte aligned in memory
                v[jj][it] = u32x4{0u, 0u, 0u, 0u};
                if (n0 > -4 && n0 < len) {
                    const int64_t g = run + n0;
                    if (g >= 0 && g + 4 <= plane) {
                        v[jj][it] = *reinterpret_cast<const u32x4*>(a.gbuf + g);
                    } else {
                        #pragma unroll
                        for (int i = 0; i < 4; i++) {
                            if (g + i >= 0 && g + i < plane) v[jj][it][i] = a.gbuf[g + i];
                        }
                    }
                }
            }
        }
        // this lane's pixels of fb, asked for before the tile is waited for
        #pragma unroll
        for (int k = 0; k < ROWS_PER_WAVE; k++) {
            const int y = ty0 + ly0 + k;
            if (y < a.rb && in_cols) src[k] = a.fb[(size_t)(y - a.ra) * W + px];
        }
        #pragma unroll
        for (int jj = 0; jj < STAGE_ROUNDS; jj++) {
            const int j = wave + WAVES * jj;
            const int r = ty0 - 1 + j;
            if (j >= STAGED_H || r < a.g0 || r >= a.g1) continue;
            const int64_t run = ((int64_t)(r - a.g0) * W + cx0) * TEXEL_DWORDS;
            const int ph = (int)((galign + (uint32_t)run) & 3u);
            const int at = j * STAGED_PITCH + (int)row_shift(a, galign, r, tx0) + c0 * TEXEL_DWORDS;  // of run dword 0
            #pragma unroll
            for (int it = 0; it < UNIT_ROUNDS; it++) {
                const int n0 = 4 * (lane + 64 * it) - ph;
                // (at + n0) is a multiple of 4, and [at + n0, at + n0 + 4) lies inside staged row j's pitch
                if (n0 > -4 && n0 < len) *reinterpret_cast<u32x4*>(staged + at + n0) = v[jj][it];
            }
        }
        __syncthreads();
        // ---- classify: this wavefront's rows ly0 .. ly0 + 3 of the tile, lane = column ---------------------------
        // Every read below stays inside `staged` and none is skipped: a texel of a row or column that was not staged
        // holds whatever LDS held, and its neighbour's `has_` flag keeps it out of the class.
        const int has_left = px >= 1u, has_right = px + 1u < W;
        Texel centre[ROWS_PER_WAVE + 2];
        #pragma unroll
        for (int k = 0; k < ROWS_PER_WAVE + 2; k++) {
            const uint32_t* row = staged + (ly0 + k) * STAGED_PITCH + row_shift(a, galign, ty0 - 1 + ly0 + k, tx0);
            centre[k] = texel_at(row + (lane + 1) * TEXEL_DWORDS, a.background);
        }
        #pragma unroll
        for (int k = 0; k < ROWS_PER_WAVE; k++) {
            const int y = ty0 + ly0 + k;
            const uint32_t* row = staged + (ly0 + k + 1) * STAGED_PITCH + row_shift(a, galign, y, tx0);
            const Texel left = texel_at(row + lane * TEXEL_DWORDS, a.background);
            const Texel right = texel_at(row + (lane + 2) * TEXEL_DWORDS, a.background);
            const Texel &t = centre[k + 1], &up = centre[k], &down = centre[k + 2];
            const int has_up = y - 1 >= a.g0, has_down = y + 1 < a.g1;
            const int sil = (has_left & silhouette_against(t, left, a.depth_step)) |
                             (has_right & silhouette_against(t, right, a.depth_step)) |
                             (has_up & silhouette_against(t, up, a.depth_step)) |
                             (has_down & silhouette_against(t, down, a.depth_step));
            const int crease = crease_with(t, right, has_right, a.depth_step) | crease_with(t, down, has_down, a.depth_step);
            cls[k] = (in_cols && y < a.rb && t.covered) ? (sil ? 2u : (uint32_t)crease) : 0u;
        }
        #pragma unroll
        for (int k = 0; k < ROWS_PER_WAVE; k++) {
            const int s = cls[k] == 2u ? a.silhouette_scale : (cls[k] == 1u ? a.crease_scale : 256);
            src[k] = scaled(src[k], s);
        }
    } else {
        #pragma unroll
        for (int k = 0; k < ROWS_PER_WAVE; k++) {
            const int y = ty0 + ly0 + k;
            if (y < a.rb && in_cols) src[k] = a.fb[(size_t)(y - a.ra) * W + px];
        }
        if (QUANT) __syncthreads();  // the palette in LDS
    }

    // ---- quantise and the colour tile: a pixel that does not exist gets the word of a zero pixel, and is not stored --
    uint32_t word[ROWS_PER_WAVE];
    if (QUANT) {
        uint32_t rgb[ROWS_PER_WAVE];
        #pragma unroll
        for (int k = 0; k < ROWS_PER_WAVE; k++) rgb[k] = dithered(src[k], px, (uint32_t)(ty0 + ly0 + k), a.spread);
        uint32_t key[ROWS_PER_WAVE] = {~0u, ~0u, ~0u, ~0u};
        const int n_colors = a.n_colors;
        int p = 0;
        for (; p + 8 <= n_colors; p += 8) {
            uint32_t e[8];
            for (int k = 0; k < 8; k++) e[k] = palette[p + k] & QUANT_RGB;
            for (int k = 0; k < 8; k += 2) {
                for (int i = 0; i < ROWS_PER_WAVE; i++) {
                    key[i] = min3u(key[i], __builtin_amdgcn_sad_hi_u8(rgb[i], e[k], (uint32_t)(p + k)),
                                   __builtin_amdgcn_sad_hi_u8(rgb[i], e[k + 1], (uint32_t)(p + k + 1)));
                }
            }
        }
        for (; p < n_colors; p++) {
            const uint32_t e = palette[p] & QUANT_RGB;
            for (int i = 0; i < ROWS_PER_WAVE; i++) key[i] = std::min(key[i], __builtin_amdgcn_sad_hi_u8(rgb[i], e, (uint32_t)p));
        }
        #pragma unroll
        for (int k = 0; k < ROWS_PER_WAVE; k++) {
            const uint32_t idx = key[k] & 0xFFu;  // < n_colors
            word[k] = pal[idx];
            if (a.index_out) {
                const int y = ty0 + ly0 + k;
                const size_t at = (size_t)(y - a.ra) * W + px;
                // (the shuffles are outside every branch: all 64 lanes take part)
                const uint32_t four = idx | ((uint32_t)__shfl_down((int)idx, 1) << 8) |
                                      ((uint32_t)__shfl_down((int)idx, 2) << 16) | ((uint32_t)__shfl_down((int)idx, 3) << 24);
                if (a.index_wide) {  // W is a multiple of 4: the four columns exist or none does
                    if (y < a.rb && in_cols && (lane & 3) == 0) *reinterpret_cast<uint32_t*>(a.index_out + at) = four;
                } else if (y < a.rb && in_cols) {
                    a.index_out[at] = (uint8_t)idx;
                }
            }
        }
    } else {
        #pragma unroll
        for (int k = 0; k < ROWS_PER_WAVE; k++) word[k] = a.swap ? exchanged(src[k]) : src[k];
    }
    #pragma unroll
    for (int k = 0; k < ROWS_PER_WAVE; k++) colour[(ly0 + k) * TILE_W + lane] = word[k];
    // (a wavefront reads back only the four rows it wrote, so a wave-level wait for its LDS writes would do; the
    // workgroup's barrier is kept because it is what the language guarantees, and it is not what bounds the kernel)
    __syncthreads();

    // ---- expand: this wavefront's four tile rows, 64 * sx groups of four output pixels in sx rounds ----------------
    const uint32_t sx = a.sx, sy = a.sy;
    const uint32_t groups_per_row = 16u * sx;                 // of the tile
    const uint32_t out_width = W * sx;                        // W'
    const uint32_t tile_x0 = tx0 * sx;                        // the tile's first output pixel of a row
    for (uint32_t round = 0; round < sx; round++) {
        const uint32_t g = (uint32_t)lane + 64u * round;      // < 64 * sx
        const uint32_t k = (g >= groups_per_row ? 1u : 0u) + (g >= 2u * groups_per_row ? 1u : 0u) +
                           (g >= 3u * groups_per_row ? 1u : 0u);  // tile row of the wavefront's four
        const uint32_t local = 4u * (g - k * groups_per_row);  // the group's first output pixel within the tile's row
        const uint32_t base = tile_x0 + local;                 // and within the surface's
        const int y = ty0 + ly0 + (int)k;
        if (y >= a.rb || base >= out_width) continue;
        uint32_t at[4];  // tile columns: every one stays below 64
        group_columns(local, sx, a.by_sx, (uint32_t)TILE_W - 1u, at);
        const uint32_t* row = colour + (ly0 + (int)k) * TILE_W;
        uint32_t c[4];
        for (int i = 0; i < 4; i++) c[i] = row[at[i]];
        char* const dst = a.out + (size_t)(y - a.ra) * sy * a.pitch + 4u * (size_t)base;
        store_group<VEC>(dst, c, base + 4u <= out_width, base, out_width, sy, a.pitch);
    }
}

template <bool OUTLINE, bool QUANT>
void launch_one(hipStream_t stream, const dim3& grid, bool vec, const FinishArgs& a, const uint32_t* palette) {
    if (vec) hipLaunchKernelGGL((finish_kernel<OUTLINE, QUANT, true>), grid, dim3(THREADS), 0, stream, a, palette);
    else hipLaunchKernelGGL((finish_kernel<OUTLINE, QUANT, false>), grid, dim3(THREADS), 0, stream, a, palette);
}

// Rows [row_begin, row_end) in launches of whole tile rows, cut by par_tile_row_cuts as launch_outline's are. Every
// launch reads the one G-buffer plane: the rows beside a cut are its halo.
hipError_t launch_finish(hipStream_t stream, const par_params* p, const par_outline_style* style, const par_pixel* gbuf,
                         int g0, int g1, const par_color* d_palette, int n_colors, int spread, const par_present_desc& d,
                         const par_color* fb, int row_begin, int row_end, void* out, uint8_t* index_out) {
    const uint32_t W = (uint32_t)p->width;
    const uint32_t gray = p->background;
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15u) == 0 && (d.pitch & 15) == 0;
    return (hipError_t)par_tile_row_cuts(row_begin, row_end, W, TILE_H, [&](int ra, int rb, uint32_t tile_rows) {
        const size_t at = (size_t)(ra - row_begin) * W;
        FinishArgs a;
        a.gbuf = reinterpret_cast<const uint32_t*>(gbuf);
        a.fb = reinterpret_cast<const uint32_t*>(fb) + at;
        a.index_out = index_out ? index_out + at : nullptr;
        a.out = static_cast<char*>(out) + (size_t)(ra - row_begin) * (size_t)d.scale_y * (size_t)d.pitch;
        a.width = W;
        a.g0 = g0; a.g1 = g1; a.ra = ra; a.rb = rb;
        a.background = gray | (gray << 8) | (gray << 16);
        a.depth_step = style ? style->depth_step : 1;
        a.silhouette_scale = style ? style->silhouette_scale : 256;
        a.crease_scale = style ? style->crease_scale : 256;
        a.n_colors = n_colors;
        a.spread = spread;
        a.sx = (uint32_t)d.scale_x;
        a.sy = (uint32_t)d.scale_y;
        a.by_sx = par_udiv31_make(a.sx);
        a.pitch = (size_t)d.pitch;
        a.swap = d.order == PAR_PRESENT_BGRA;
        // (a multiple of 4 pixels a row keeps every row of every launch at the phase of the plane's first byte)
        a.index_wide = W % 4u == 0 && (reinterpret_cast<uintptr_t>(a.index_out) & 3u) == 0;
        const uint32_t* palette = reinterpret_cast<const uint32_t*>(d_palette);
        const dim3 grid((W + TILE_W - 1) / TILE_W, tile_rows);
        if (style && d_palette) launch_one<true, true>(stream, grid, vec, a, palette);
        else if (style) launch_one<true, false>(stream, grid, vec, a, palette);
        else launch_one<false, true>(stream, grid, vec, a, palette);
        return (int)hipGetLastError();
    });
}

bool finish_args_ok(const par_params* p, const par_outline_style* s, const par_pixel* gbuf, int g0, int g1,
                    const par_color* palette, int n_colors, int spread, const par_present_desc* d, const par_color* fb,
                    int r0, int r1, const void* out, const uint8_t* index_out) {
    if (!p || !d || !fb || !out) return false;
    if ((s != nullptr) != (gbuf != nullptr)) return false;
    if (!s && !palette) return false;  // neither stage: that call is par_present_device
    if (p->width <= 0) return false;
    if (s) {
        if (s->depth_step < 1 || s->silhouette_scale < 0 || s->silhouette_scale > 1024 || s->crease_scale < 0 ||
            s->crease_scale > 1024) return false;
        if (!(0 <= g0 && g0 <= r0 && r0 < r1 && r1 <= g1 && g1 <= p->height)) return false;
    } else if (!(0 <= r0 && r0 < r1 && r1 <= p->height)) {
        return false;
    }
    if (palette) {
        if (n_colors < 1 || n_colors > PAR_MAX_PALETTE || spread < 0 || spread > 255) return false;
    } else if (n_colors != 0 || spread != 0 || index_out) {
        return false;
    }
    return present_desc_ok(d, p->width);
}

}  // namespace

extern "C" {

int par_finish_device(const par_params* params, void* stream, const par_outline_style* style, const par_pixel* gbuf,
                      int gbuf_row_begin, int gbuf_row_end, const par_color* d_palette, int n_colors, int spread,
                      const par_present_desc* desc, const par_color* fb, int row_begin, int row_end, void* out,
                      uint8_t* index_out) {
    if (!finish_args_ok(params, style, gbuf, gbuf_row_begin, gbuf_row_end, d_palette, n_colors, spread, desc, fb,
                        row_begin, row_end, out, index_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    const hipError_t e = launch_finish((hipStream_t)stream, params, style, gbuf, gbuf_row_begin, gbuf_row_end, d_palette,
                                       n_colors, spread, *desc, fb, row_begin, row_end, out, index_out);
    return e == hipSuccess ? PAR_OK : PAR_ERR_HIP;
}

int par_finish_host(const par_params* params, int device, const par_outline_style* style, const par_pixel* gbuf,
                    int gbuf_row_begin, int gbuf_row_end, const par_color* palette, int n_colors, int spread,
                    const par_present_desc* desc, const par_color* fb, int row_begin, int row_end, void* out,
                    uint8_t* index_out) {
    if (!finish_args_ok(params, style, gbuf, gbuf_row_begin, gbuf_row_end, palette, n_colors, spread, desc, fb, row_begin,
                        row_end, out, index_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    const size_t n = (size_t)(row_end - row_begin) * (size_t)params->width;
    const size_t n_g = style ? (size_t)(gbuf_row_end - gbuf_row_begin) * (size_t)params->width : 0;
    const size_t out_rows = (size_t)(row_end - row_begin) * (size_t)desc->scale_y;
    const size_t row_bytes = 4 * (size_t)params->width * (size_t)desc->scale_x;
    par_device_buffer d_gbuf(e, gbuf, n_g * sizeof(par_pixel), true);
    par_device_buffer d_palette(e, palette, (size_t)n_colors * sizeof(par_color), true);
    par_device_buffer d_fb(e, fb, n * sizeof(par_color), true), d_index(e, index_out, n, false);
    par_device_buffer d_out(e, out, out_rows * (size_t)desc->pitch, false);
    if (e == hipSuccess) {
        e = launch_finish(nullptr, params, style, d_gbuf.as<par_pixel>(), gbuf_row_begin, gbuf_row_end,
                          d_palette.as<par_color>(), n_colors, spread, *desc, d_fb.as<par_color>(), row_begin, row_end,
                          d_out.as<void>(), d_index.as<uint8_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    // a pitched copy: the caller's gap bytes stay as they are
    if (e == hipSuccess) e = hipMemcpy2D(out, (size_t)desc->pitch, d_out.as<void>(), (size_t)desc->pitch, row_bytes, out_rows, hipMemcpyDeviceToHost);
    d_index.download(index_out);
    return par_status_of(e);
}

}  // extern "C"
