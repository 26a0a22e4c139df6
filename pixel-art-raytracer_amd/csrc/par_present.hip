// par_present.hip — present: a frame or an index plane scaled onto a surface at an integer scale, nearest neighbour, in
// the surface's byte order and row pitch (par_present_device, par_present_host). The contract is beside the declarations
// in par_raytracer.h; nothing here knows a par_context, and the render kernels (par_kernels.hip) know nothing of this.
//
// The kernel. The pass writes sx * sy times the bytes it reads, so it is laid out by its stores. A lane takes a GROUP
// of 4 consecutive output pixels of one SOURCE row: 16 bytes, on a 16-byte boundary when `out` and the pitch are. It
// finds the group's source columns with one division by sx (then steps), loads its at most four source elements once,
// all four loads in flight together, and stores the same 16-byte value to the sy output rows of its source row:
// neighbouring lanes store neighbouring 16 bytes, 1 KiB per wavefront and store instruction. The group that hangs over
// a row's end, and every group when `out` or the pitch is off the 16-byte phase, goes pixel by pixel. With an index
// source a workgroup first loads the palette into 1 KiB of LDS, entry i being palette[min(i, n_colors - 1)] in the
// surface's byte order: the clamp and the exchange are paid once per workgroup, and a lane's gather is an LDS read per
// pixel at the address the index byte gives.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_fastdiv.h"
#include "par_hostcall.h"
#include "par_post.h"
#include "par_raytracer.h"

namespace {

constexpr int PRESENT_THREADS = 256;
// Output pixels of one row of one launch, summed over its source rows (the groups' padding included): flat group
// indices and both divisions stay below 2^31 (par_udiv31).
constexpr uint32_t PRESENT_MAX_PX = 0x7FFFFFF0u;

// INDEXED: `src` is an index plane (bytes) and `palette` its palette; else `src` is a frame (words). VEC: `out` and
// `pitch` are multiples of 16. `wide_src` (VEC, a frame, sx == 1, `src` on a 16-byte boundary, width a multiple of 4):
// a full group's four source pixels are one 16-byte load.
template <bool INDEXED, bool VEC>
__global__ __launch_bounds__(PRESENT_THREADS) void present_kernel(const void* __restrict__ src,
                                                                   const uint32_t* __restrict__ palette, int n_colors,
                                                                   char* __restrict__ out, uint32_t n_groups,
                                                                   uint32_t groups_per_row, par_udiv31 by_groups_per_row,
                                                                   uint32_t width, uint32_t out_width, uint32_t sx,
                                                                   par_udiv31 by_sx, uint32_t sy, size_t pitch, bool swap,
                                                                   bool wide_src) {
    __shared__ uint32_t pal[PAR_MAX_PALETTE];
    if (INDEXED) {
        static_assert(PRESENT_THREADS == PAR_MAX_PALETTE, "one palette entry per thread");
        pal[threadIdx.x] = palette_entry(palette, n_colors, swap);
        __syncthreads();
    }
    const uint32_t t = blockIdx.x * (uint32_t)PRESENT_THREADS + threadIdx.x;
    if (t >= n_groups) return;
    const uint32_t row = par_udiv31_quotient(t, by_groups_per_row);  // source row within the launch
    const uint32_t base = 4u * (t - row * groups_per_row);           // the group's first output pixel, < out_width
    const bool full = base + 4u <= out_width;
    const size_t src_row = (size_t)row * width;
    char* const dst = out + (size_t)row * sy * pitch + 4u * (size_t)base;

    uint32_t c[4];
    if (VEC && wide_src && full) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(static_cast<const uint32_t*>(src) + src_row + base);
        for (int i = 0; i < 4; i++) c[i] = v[i];
    } else {
        // the source columns (group_columns): a pixel past the row's end takes the last column and is not stored. No
        // load waits for a decision: the four are issued together, and those of one source element are one address
        uint32_t at[4];
        group_columns(base, sx, by_sx, width - 1u, at);
        if (INDEXED) {
            uint32_t k[4];
            for (int i = 0; i < 4; i++) k[i] = static_cast<const uint8_t*>(src)[src_row + at[i]];
            for (int i = 0; i < 4; i++) c[i] = pal[k[i]];
        } else {
            for (int i = 0; i < 4; i++) c[i] = static_cast<const uint32_t*>(src)[src_row + at[i]];
        }
    }
    if (!INDEXED && swap) {
        for (int i = 0; i < 4; i++) c[i] = exchanged(c[i]);
    }

    store_group<VEC>(dst, c, full, base, out_width, sy, pitch);
}

template <bool INDEXED, bool VEC>
void launch_one(hipStream_t stream, const void* src, const uint32_t* palette, int n_colors, char* out, uint32_t rows,
                uint32_t groups_per_row, uint32_t width, const par_present_desc& d, bool wide_src) {
    const uint32_t n_groups = rows * groups_per_row;
    const uint32_t blocks = (n_groups + PRESENT_THREADS - 1) / PRESENT_THREADS;
    hipLaunchKernelGGL((present_kernel<INDEXED, VEC>), dim3(blocks), dim3(PRESENT_THREADS), 0, stream, src, palette,
                       n_colors, out, n_groups, groups_per_row, par_udiv31_make(groups_per_row), width,
                       width * (uint32_t)d.scale_x, (uint32_t)d.scale_x, par_udiv31_make((uint32_t)d.scale_x),
                       (uint32_t)d.scale_y, (size_t)d.pitch, d.order == PAR_PRESENT_BGRA, wide_src);
}

// Source rows [row_begin, row_end) in launches of whole source rows, at most PRESENT_MAX_PX output pixels a row of
// groups each (a single row is never cut: 4 * width * sx fits an int32, so its groups stay far below 2^31).
hipError_t launch_present(hipStream_t stream, const par_present_desc& d, int width, const par_color* fb,
                          const uint8_t* index, const par_color* d_palette, int n_colors, int row_begin, int row_end,
                          void* out) {
    const uint32_t groups_per_row = ((uint32_t)width * (uint32_t)d.scale_x + 3u) / 4u;
    const uint32_t rows_per_launch = std::max<uint32_t>(1u, PRESENT_MAX_PX / (4u * groups_per_row));
    const uint32_t* palette = reinterpret_cast<const uint32_t*>(d_palette);
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15u) == 0 && (d.pitch & 15) == 0;
    for (int r0 = row_begin; r0 < row_end;) {
        const uint32_t rows = std::min<uint32_t>(rows_per_launch, (uint32_t)(row_end - r0));
        const size_t at = (size_t)(r0 - row_begin) * (size_t)width;
        char* dst = static_cast<char*>(out) + (size_t)(r0 - row_begin) * (size_t)d.scale_y * (size_t)d.pitch;
        if (index) {
            if (vec) launch_one<true, true>(stream, index + at, palette, n_colors, dst, rows, groups_per_row, (uint32_t)width, d, false);
            else launch_one<true, false>(stream, index + at, palette, n_colors, dst, rows, groups_per_row, (uint32_t)width, d, false);
        } else {
            const par_color* src = fb + at;
            const bool wide = vec && d.scale_x == 1 && (width & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15u) == 0;
            if (vec) launch_one<false, true>(stream, src, nullptr, 0, dst, rows, groups_per_row, (uint32_t)width, d, wide);
            else launch_one<false, false>(stream, src, nullptr, 0, dst, rows, groups_per_row, (uint32_t)width, d, false);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        r0 += (int)rows;
    }
    return hipSuccess;
}

bool present_args_ok(const par_params* p, const par_present_desc* d, const par_color* fb, const uint8_t* index,
                     const par_color* palette, int n_colors, int row_begin, int row_end, const void* out) {
    if (!p || !d || !out || (fb != nullptr) == (index != nullptr)) return false;
    if (index && (!palette || n_colors < 1 || n_colors > PAR_MAX_PALETTE)) return false;
    if (fb && (palette || n_colors != 0)) return false;
    if (p->width <= 0 || row_begin < 0 || row_begin >= row_end || row_end > p->height) return false;
    return present_desc_ok(d, p->width);
}

}  // namespace

extern "C" {

int par_present_device(const par_params* params, void* stream, const par_present_desc* desc, const par_color* fb,
                       const uint8_t* index, const par_color* d_palette, int n_colors, int row_begin, int row_end,
                       void* out) {
    if (!present_args_ok(params, desc, fb, index, d_palette, n_colors, row_begin, row_end, out)) return PAR_ERR_INVALID_ARG;
    const hipError_t e = launch_present((hipStream_t)stream, *desc, params->width, fb, index, d_palette, n_colors,
                                        row_begin, row_end, out);
    return e == hipSuccess ? PAR_OK : PAR_ERR_HIP;
}

int par_present_host(const par_params* params, int device, const par_present_desc* desc, const par_color* fb,
                     const uint8_t* index, const par_color* palette, int n_colors, int row_begin, int row_end, void* out) {
    if (!present_args_ok(params, desc, fb, index, palette, n_colors, row_begin, row_end, out)) return PAR_ERR_INVALID_ARG;
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    const size_t n = (size_t)(row_end - row_begin) * (size_t)params->width;
    const size_t out_rows = (size_t)(row_end - row_begin) * (size_t)desc->scale_y;
    const size_t row_bytes = 4 * (size_t)params->width * (size_t)desc->scale_x;
    par_device_buffer d_palette(e, palette, (size_t)n_colors * sizeof(par_color), true), d_index(e, index, n, true);
    par_device_buffer d_fb(e, fb, n * sizeof(par_color), true), d_out(e, out, out_rows * (size_t)desc->pitch, false);
    if (e == hipSuccess) {
        e = launch_present(nullptr, *desc, params->width, d_fb.as<par_color>(), d_index.as<uint8_t>(),
                           d_palette.as<par_color>(), n_colors, row_begin, row_end, d_out.as<void>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    // a pitched copy: the caller's gap bytes stay as they are
    if (e == hipSuccess) e = hipMemcpy2D(out, (size_t)desc->pitch, d_out.as<void>(), (size_t)desc->pitch, row_bytes, out_rows, hipMemcpyDeviceToHost);
    return par_status_of(e);
}

}  // extern "C"
