// par_outline.hip — outlines: silhouettes and creases drawn from a frame's G-buffer (par_outline_device,
// par_outline_host). The contract is beside the declarations in par_raytracer.h; nothing here knows a par_context, and
// the render kernels (par_kernels.hip) and the palette pass (par_quantize.hip) know nothing of this.
//
// The kernel. A workgroup of 256 threads takes a tile of OUTLINE_TILE_W x OUTLINE_TILE_H = 64 x 16 pixels and stages
// the tile's texels plus a one-texel halo (66 x 18, clipped to the frame's columns and to the G-buffer rows the caller
// passed) into LDS as they lie in memory, seven dwords a texel: the halo makes 66 * 18 / (64 * 16) = 1.16 texels
// fetched per pixel. A staged row is one contiguous run of at most 462 dwords whose first byte sits at any 4-byte phase
// (28-byte texels, any width); a wavefront takes a row and loads it in 16-byte units that are aligned in MEMORY, so
// every unit whose 16 bytes lie inside the plane is one global_load_dwordx4, the two that hang over the run's ends
// included. A row's place in LDS is shifted by 0..3 dwords so that its LDS phase equals its memory phase: a unit is one
// ds_write_b128 too. One barrier. Then a wavefront classifies four consecutive tile rows, lane = column, in straight-
// line code: a texel's dwords are 7 apart between lanes, and 7 is coprime with the 32 banks a ds_read_b32 sees, so the
// reads are conflict-free without padding or a compacted record (which would need a second pass over the staged bytes
// to build). The six centre texels of a lane's column are read once and shared by the four pixels as centre, upper and
// lower neighbour.
// Outputs. VEC (the host's choice: width a multiple of 4 and every plane in use on its natural 16 / 4 byte boundary):
// the wavefront's 4 x 64 classes go through two ballots per row into scalar masks, and lane L takes the four pixels
// 4 * (L & 15) .. + 3 of row L >> 4: one global_load_dwordx4 of fb, one global_store_dwordx4 of fb_out, one dword of
// four classes. Otherwise lane = column: one dword of fb, one of fb_out and one byte per pixel, still contiguous over
// the wavefront.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_hostcall.h"
#include "par_post.h"
#include "par_raytracer.h"

namespace {

// (OUTLINE_TILE_W .. STAGE_ROUNDS, the tile's geometry, and row_shift are par_post.h's: finish_kernel stages the same
// tile, in its own copy of the stage below)
struct OutlineArgs {
    const uint32_t* gbuf;  // dwords of the G-buffer plane, row g0 at index 0
    const uint32_t* fb;    // the three planes address (ra, 0)
    uint32_t* fb_out;
    uint8_t* edge_out;
    uint32_t width;
    int g0, g1;   // G-buffer rows: neighbours outside are absent
    int ra, rb;   // rows of this launch
    uint32_t background;  // w3 of the background texel
    int depth_step, silhouette_scale, crease_scale;
};

template <bool VEC>
__global__ __launch_bounds__(OUTLINE_THREADS) void outline_kernel(OutlineArgs a) {
    __shared__ u32x4 staged4[STAGED_H * STAGED_PITCH / 4];
    uint32_t* staged = reinterpret_cast<uint32_t*>(staged4);

    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t W = a.width;
    const uint32_t tx0 = blockIdx.x * (uint32_t)OUTLINE_TILE_W;
    const int ty0 = a.ra + (int)blockIdx.y * OUTLINE_TILE_H;
    u32x4 v[STAGE_ROUNDS][UNIT_ROUNDS];
    const uint32_t galign = (uint32_t)(reinterpret_cast<uintptr_t>(a.gbuf) >> 2) & 3u;

    // ---- stage: staged row j holds absolute row ty0 - 1 + j, staged column c holds column tx0 - 1 + c -------------
    const uint32_t cx0 = tx0 == 0 ? 0u : tx0 - 1u;                    // the columns that exist
    const uint32_t cx1 = std::min(tx0 + (uint32_t)OUTLINE_TILE_W + 1u, W);
    const int c0 = (int)(cx0 - (tx0 - 1u));                           // staged column of cx0: 0 or 1
    const int len = (int)(cx1 - cx0) * TEXEL_DWORDS;                  // dwords of a row's run
    // (a unit that hangs over an end of its run is loaded whole all the same, where its 16 bytes lie inside the plane:
    // what it brings along lands in LDS dwords of the row's own pitch that hold no texel of the tile. Only the first
    // and the last unit of the whole plane can go dword by dword.)
    const int64_t plane = (int64_t)(a.g1 - a.g0) * W * TEXEL_DWORDS;
    #pragma unroll
    for (int jj = 0; jj < STAGE_ROUNDS; jj++) {
        const int j = wave + OUTLINE_WAVES * jj;
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
    // this thread's pixels of fb, asked for before the tile is waited for
    const int ly0 = wave * OUTLINE_ROWS_PER_WAVE;
    const uint32_t px = tx0 + (uint32_t)lane;
    const bool in_cols = px < W;
    // VEC: lane L takes pixels 4 * (L & 15) .. + 3 of row L >> 4 (the width is a multiple of 4: all four exist or none)
    const int kk = lane >> 4, xx = 4 * (lane & 15);
    const int y4 = ty0 + ly0 + kk;
    const bool live4 = y4 < a.rb && tx0 + (uint32_t)xx < W;
    const size_t at4 = (size_t)(y4 - a.ra) * W + tx0 + (uint32_t)xx;
    u32x4 src{0u, 0u, 0u, 0u};
    if (a.fb_out) {
        if (VEC) {
            if (live4) src = *reinterpret_cast<const u32x4*>(a.fb + at4);
        } else {
            #pragma unroll
            for (int k = 0; k < OUTLINE_ROWS_PER_WAVE; k++) {
                const int y = ty0 + ly0 + k;
                if (y < a.rb && in_cols) src[k] = a.fb[(size_t)(y - a.ra) * W + px];
            }
        }
    }
    #pragma unroll
    for (int jj = 0; jj < STAGE_ROUNDS; jj++) {
        const int j = wave + OUTLINE_WAVES * jj;
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

    uint32_t cls[OUTLINE_ROWS_PER_WAVE];
    // ---- classify: this wavefront's rows ly0 .. ly0 + 3 of the tile, lane = column -------------------------------
    // Every read below stays inside `staged` and none is skipped: a texel of a row or column that was not staged holds
    // whatever LDS held, and its neighbour's `has_` flag keeps it out of the class.
    const int has_left = px >= 1u, has_right = px + 1u < W;
    Texel centre[OUTLINE_ROWS_PER_WAVE + 2];
    #pragma unroll
    for (int k = 0; k < OUTLINE_ROWS_PER_WAVE + 2; k++) {
        const uint32_t* row = staged + (ly0 + k) * STAGED_PITCH + row_shift(a, galign, ty0 - 1 + ly0 + k, tx0);
        centre[k] = texel_at(row + (lane + 1) * TEXEL_DWORDS, a.background);
    }
    #pragma unroll
    for (int k = 0; k < OUTLINE_ROWS_PER_WAVE; k++) {
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

    // ---- outputs ---------------------------------------------------------------------------------------------------
    if (VEC) {
        uint64_t crease_bits = 0, sil_bits = 0;
        #pragma unroll
        for (int k = 0; k < OUTLINE_ROWS_PER_WAVE; k++) {
            const uint64_t m1 = __ballot(cls[k] == 1u), m2 = __ballot(cls[k] == 2u);
            if (kk == k) { crease_bits = m1; sil_bits = m2; }
        }
        const uint32_t c4 = (uint32_t)(crease_bits >> xx) & 15u, s4 = (uint32_t)(sil_bits >> xx) & 15u;
        if (live4) {
            if (a.edge_out) {
                uint32_t packed = 0;
                #pragma unroll
                for (int i = 0; i < 4; i++) packed |= ((((s4 >> i) & 1u) << 1) | ((c4 >> i) & 1u)) << (8 * i);
                *reinterpret_cast<uint32_t*>(a.edge_out + at4) = packed;
            }
            if (a.fb_out) {
                u32x4 dst;
                #pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int s = ((s4 >> i) & 1u) ? a.silhouette_scale : (((c4 >> i) & 1u) ? a.crease_scale : 256);
                    dst[i] = scaled(src[i], s);
                }
                *reinterpret_cast<u32x4*>(a.fb_out + at4) = dst;
            }
        }
    } else {
        #pragma unroll
        for (int k = 0; k < OUTLINE_ROWS_PER_WAVE; k++) {
            const int y = ty0 + ly0 + k;
            if (y >= a.rb || !in_cols) continue;
            const size_t at = (size_t)(y - a.ra) * W + px;
            if (a.edge_out) a.edge_out[at] = (uint8_t)cls[k];
            if (a.fb_out) {
                const int s = cls[k] == 2u ? a.silhouette_scale : (cls[k] == 1u ? a.crease_scale : 256);
                a.fb_out[at] = scaled(src[k], s);
            }
        }
    }
}

// Rows [row_begin, row_end) in launches of whole tile rows, cut by par_tile_row_cuts. Every launch reads the one
// G-buffer plane: the rows beside a cut are its halo.
hipError_t launch_outline(hipStream_t stream, const par_params* p, const par_outline_style* style, const par_pixel* gbuf,
                          int g0, int g1, const par_color* fb, int row_begin, int row_end, par_color* fb_out,
                          uint8_t* edge_out) {
    const uint32_t W = (uint32_t)p->width;
    const uint32_t gray = p->background;
    const uintptr_t in = reinterpret_cast<uintptr_t>(fb), out = reinterpret_cast<uintptr_t>(fb_out),
                    edge = reinterpret_cast<uintptr_t>(edge_out);
    // (a multiple of 4 pixels a row keeps every row of every launch at the phase of the plane's first byte)
    const bool vec = W % 4u == 0 && (!fb_out || ((in | out) & 15u) == 0) && (edge & 3u) == 0;
    return (hipError_t)par_tile_row_cuts(row_begin, row_end, W, OUTLINE_TILE_H, [&](int ra, int rb, uint32_t tile_rows) {
        const size_t at = (size_t)(ra - row_begin) * W;
        OutlineArgs a;
        a.gbuf = reinterpret_cast<const uint32_t*>(gbuf);
        a.fb = fb ? reinterpret_cast<const uint32_t*>(fb) + at : nullptr;
        a.fb_out = fb_out ? reinterpret_cast<uint32_t*>(fb_out) + at : nullptr;
        a.edge_out = edge_out ? edge_out + at : nullptr;
        a.width = W;
        a.g0 = g0; a.g1 = g1; a.ra = ra; a.rb = rb;
        a.background = gray | (gray << 8) | (gray << 16);
        a.depth_step = style->depth_step;
        a.silhouette_scale = style->silhouette_scale;
        a.crease_scale = style->crease_scale;
        const dim3 grid((W + OUTLINE_TILE_W - 1) / OUTLINE_TILE_W, tile_rows);
        if (vec) hipLaunchKernelGGL(outline_kernel<true>, grid, dim3(OUTLINE_THREADS), 0, stream, a);
        else hipLaunchKernelGGL(outline_kernel<false>, grid, dim3(OUTLINE_THREADS), 0, stream, a);
        return (int)hipGetLastError();
    });
}

bool outline_args_ok(const par_params* p, const par_outline_style* s, const par_pixel* gbuf, int g0, int g1,
                     const par_color* fb, int r0, int r1, const par_color* fb_out, const uint8_t* edge_out) {
    return p && s && gbuf && (fb_out || edge_out) && (fb || !fb_out) && p->width > 0 && s->depth_step >= 1 &&
           s->silhouette_scale >= 0 && s->silhouette_scale <= 1024 && s->crease_scale >= 0 && s->crease_scale <= 1024 &&
           0 <= g0 && g0 <= r0 && r0 < r1 && r1 <= g1 && g1 <= p->height;
}

}  // namespace

extern "C" {

int par_outline_device(const par_params* params, void* stream, const par_outline_style* style, const par_pixel* gbuf,
                       int gbuf_row_begin, int gbuf_row_end, const par_color* fb, int row_begin, int row_end,
                       par_color* fb_out, uint8_t* edge_out) {
    if (!outline_args_ok(params, style, gbuf, gbuf_row_begin, gbuf_row_end, fb, row_begin, row_end, fb_out, edge_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    const hipError_t e = launch_outline((hipStream_t)stream, params, style, gbuf, gbuf_row_begin, gbuf_row_end, fb,
                                        row_begin, row_end, fb_out, edge_out);
    return e == hipSuccess ? PAR_OK : PAR_ERR_HIP;
}

int par_outline_host(const par_params* params, int device, const par_outline_style* style, const par_pixel* gbuf,
                     int gbuf_row_begin, int gbuf_row_end, const par_color* fb, int row_begin, int row_end,
                     par_color* fb_out, uint8_t* edge_out) {
    if (!outline_args_ok(params, style, gbuf, gbuf_row_begin, gbuf_row_end, fb, row_begin, row_end, fb_out, edge_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    const size_t n = (size_t)(row_end - row_begin) * (size_t)params->width;
    const size_t n_g = (size_t)(gbuf_row_end - gbuf_row_begin) * (size_t)params->width;
    // the device copy of fb is outlined in place when fb_out is asked for
    par_device_buffer d_gbuf(e, gbuf, n_g * sizeof(par_pixel), true);
    par_device_buffer d_fb(e, fb_out ? fb : nullptr, n * sizeof(par_color), true), d_edge(e, edge_out, n, false);
    if (e == hipSuccess) {
        e = launch_outline(nullptr, params, style, d_gbuf.as<par_pixel>(), gbuf_row_begin, gbuf_row_end,
                           d_fb.as<par_color>(), row_begin, row_end, d_fb.as<par_color>(), d_edge.as<uint8_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    d_fb.download(fb_out);
    d_edge.download(edge_out);
    return par_status_of(e);
}

}  // extern "C"
