// par_quantize.hip — palette output: a frame quantised to a fixed palette on the device (par_quantize_device,
// par_quantize_host), and the natural palette of a scene (par_palette_ramp). The contract is beside the declarations in
// par_raytracer.h; nothing here knows a par_context, and the render kernels (par_kernels.hip) know nothing of this.
//
// The kernel. The rows of a call are one dense array of n pixels. A lane takes a GROUP of 4 consecutive pixels; the
// groups are laid so that their first pixels sit on 16-byte boundaries of the source (`lead` pixels that do not exist
// come before pixel 0), and a group that lies wholly inside the array is one global_load_dwordx4, one dword store of
// four indices and one dwordx4 store of fb_out. The (at most two) groups that hang over an end, and every group when
// the caller's pointers do not share a 16-byte phase, go pixel by pixel. The palette index of the search loop is
// wave-uniform: the entries are read through the scalar cache, eight at a time, and cost no vector register. One
// v_sad_hi_u8 gives (L1 distance << 16) + index, the distance (<= 765) above bit 16 and the index (<= 255) below it,
// so the minimum of the keys is the nearest entry and the lowest index among equals; v_min3_u32 takes two entries.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_fastdiv.h"
#include "par_hostcall.h"
#include "par_post.h"
#include "par_raytracer.h"

namespace {

constexpr int QUANT_THREADS = 256;
// Pixels of one launch: flat indices and the division by the width stay below 2^31 (par_udiv31).
constexpr uint32_t QUANT_MAX_PX = 0x7FFFFFF0u;

template <bool DITHER, bool VEC>
__global__ __launch_bounds__(QUANT_THREADS) void quantize_kernel(const uint32_t* fb, uint32_t* fb_out, uint8_t* index_out,
                                                                 const uint32_t* __restrict__ palette, int n_colors,
                                                                 uint32_t n_px, uint32_t lead, uint32_t width,
                                                                 par_udiv31 by_width, uint32_t row_begin, int spread) {
    // pixel i of the group is u + i - lead; it exists when that is in [0, n_px)
    const uint32_t u = 4u * (blockIdx.x * (uint32_t)QUANT_THREADS + threadIdx.x);
    if (u >= n_px + lead) return;
    const uint32_t base = u - lead;  // (wraps for the first group of a launch with lead > 0: then `full` is false)
    const bool full = u >= lead && base + 4u <= n_px;
    bool live[4];
    uint32_t src[4];
    if (VEC && full) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(fb + base);
        for (int i = 0; i < 4; i++) { live[i] = true; src[i] = v[i]; }
    } else {
        for (int i = 0; i < 4; i++) {
            live[i] = u + i >= lead && base + i < n_px;
            src[i] = live[i] ? fb[base + i] : 0u;
        }
    }

    uint32_t rgb[4];
    if (DITHER) {
        // column and absolute row of the group's first pixel that exists, then one step per pixel
        const uint32_t first = u >= lead ? base : 0u;
        const uint32_t q = par_udiv31_quotient(first, by_width);
        uint32_t x = first - q * width, y = row_begin + q;
        for (int i = 0; i < 4; i++) {
            if (i > 0 && u + i > lead) {
                x++;
                if (x == width) { x = 0; y++; }
            }
            rgb[i] = dithered(src[i], x, y, spread);
        }
    } else {
        for (int i = 0; i < 4; i++) rgb[i] = src[i] & QUANT_RGB;
    }

    uint32_t key[4] = {~0u, ~0u, ~0u, ~0u};
    int p = 0;
    for (; p + 8 <= n_colors; p += 8) {
        uint32_t e[8];
        for (int k = 0; k < 8; k++) e[k] = palette[p + k] & QUANT_RGB;
        for (int k = 0; k < 8; k += 2) {
            for (int i = 0; i < 4; i++) {
                key[i] = min3u(key[i], __builtin_amdgcn_sad_hi_u8(rgb[i], e[k], (uint32_t)(p + k)),
                               __builtin_amdgcn_sad_hi_u8(rgb[i], e[k + 1], (uint32_t)(p + k + 1)));
            }
        }
    }
    for (; p < n_colors; p++) {
        const uint32_t e = palette[p] & QUANT_RGB;
        for (int i = 0; i < 4; i++) key[i] = std::min(key[i], __builtin_amdgcn_sad_hi_u8(rgb[i], e, (uint32_t)p));
    }

    uint32_t k[4];
    for (int i = 0; i < 4; i++) k[i] = key[i] & 0xFFu;
    if (index_out) {
        if (VEC && full) {
            *reinterpret_cast<uint32_t*>(index_out + base) = k[0] | (k[1] << 8) | (k[2] << 16) | (k[3] << 24);
        } else {
            for (int i = 0; i < 4; i++) {
                if (live[i]) index_out[base + i] = (uint8_t)k[i];
            }
        }
    }
    if (fb_out) {
        uint32_t o[4];
        for (int i = 0; i < 4; i++) o[i] = (palette[k[i]] & QUANT_RGB) | (src[i] & ~QUANT_RGB);
        if (VEC && full) {
            const u32x4 v = {o[0], o[1], o[2], o[3]};
            *reinterpret_cast<u32x4*>(fb_out + base) = v;
        } else {
            for (int i = 0; i < 4; i++) {
                if (live[i]) fb_out[base + i] = o[i];
            }
        }
    }
}

template <bool DITHER, bool VEC>
void launch_one(hipStream_t stream, const uint32_t* fb, uint32_t* fb_out, uint8_t* index_out, const uint32_t* palette,
                int n_colors, uint32_t n_px, uint32_t lead, uint32_t width, uint32_t row_begin, int spread) {
    const uint32_t groups = (n_px + lead + 3u) / 4u;
    const uint32_t blocks = (groups + QUANT_THREADS - 1) / QUANT_THREADS;
    hipLaunchKernelGGL((quantize_kernel<DITHER, VEC>), dim3(blocks), dim3(QUANT_THREADS), 0, stream, fb, fb_out, index_out,
                       palette, n_colors, n_px, lead, width, par_udiv31_make(width), row_begin, spread);
}

// Rows [row_begin, row_end) in launches of whole rows, at most QUANT_MAX_PX pixels each (one launch for any frame
// below 8 GiB; a single row is never cut, and width < 2^31 keeps it inside par_udiv31's range).
hipError_t launch_quantize(hipStream_t stream, const par_color* d_palette, int n_colors, int spread, int width,
                           const par_color* fb, int row_begin, int row_end, par_color* fb_out, uint8_t* index_out) {
    const uint32_t rows_per_launch = std::max<uint32_t>(1u, QUANT_MAX_PX / (uint32_t)width);
    const uint32_t* palette = reinterpret_cast<const uint32_t*>(d_palette);
    for (int r0 = row_begin; r0 < row_end;) {
        const uint32_t rows = std::min<uint32_t>(rows_per_launch, (uint32_t)(row_end - r0));
        const size_t at = (size_t)(r0 - row_begin) * (size_t)width;
        const uint32_t n_px = rows * (uint32_t)width;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(fb) + at;
        uint32_t* dst = fb_out ? reinterpret_cast<uint32_t*>(fb_out) + at : nullptr;
        uint8_t* idx = index_out ? index_out + at : nullptr;
        // pixels before the first 16-byte boundary of the source; the vector forms need every pointer in use to sit
        // at that same phase (fb_out: 16 bytes, index_out: its 4 bytes)
        const uintptr_t a = reinterpret_cast<uintptr_t>(src);
        const uint32_t head = (uint32_t)(((16u - (a & 15u)) & 15u) / 4u);
        const bool vec = (a & 3u) == 0 && (!dst || ((reinterpret_cast<uintptr_t>(dst) - a) & 15u) == 0) &&
                         (!idx || ((reinterpret_cast<uintptr_t>(idx) + head) & 3u) == 0);
        const uint32_t lead = vec ? (4u - head) & 3u : 0u;
        if (spread != 0) {
            if (vec) launch_one<true, true>(stream, src, dst, idx, palette, n_colors, n_px, lead, (uint32_t)width, (uint32_t)r0, spread);
            else launch_one<true, false>(stream, src, dst, idx, palette, n_colors, n_px, lead, (uint32_t)width, (uint32_t)r0, spread);
        } else {
            if (vec) launch_one<false, true>(stream, src, dst, idx, palette, n_colors, n_px, lead, (uint32_t)width, (uint32_t)r0, spread);
            else launch_one<false, false>(stream, src, dst, idx, palette, n_colors, n_px, lead, (uint32_t)width, (uint32_t)r0, spread);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        r0 += (int)rows;
    }
    return hipSuccess;
}

bool quantize_args_ok(const par_params* p, const par_color* palette, int n_colors, int spread, const par_color* fb,
                      int row_begin, int row_end, const par_color* fb_out, const uint8_t* index_out) {
    return p && palette && fb && (fb_out || index_out) && n_colors >= 1 && n_colors <= PAR_MAX_PALETTE && spread >= 0 &&
           spread <= 255 && p->width > 0 && row_begin >= 0 && row_begin < row_end && row_end <= p->height;
}

}  // namespace

extern "C" {

int par_quantize_device(const par_params* params, void* stream, const par_color* d_palette, int n_colors, int spread,
                        const par_color* fb, int row_begin, int row_end, par_color* fb_out, uint8_t* index_out) {
    if (!quantize_args_ok(params, d_palette, n_colors, spread, fb, row_begin, row_end, fb_out, index_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    const hipError_t e = launch_quantize((hipStream_t)stream, d_palette, n_colors, spread, params->width, fb, row_begin,
                                         row_end, fb_out, index_out);
    return e == hipSuccess ? PAR_OK : PAR_ERR_HIP;
}

int par_quantize_host(const par_params* params, int device, const par_color* palette, int n_colors, int spread,
                      const par_color* fb, int row_begin, int row_end, par_color* fb_out, uint8_t* index_out) {
    if (!quantize_args_ok(params, palette, n_colors, spread, fb, row_begin, row_end, fb_out, index_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    const size_t n = (size_t)(row_end - row_begin) * (size_t)params->width;
    // the device copy of fb is quantised in place when fb_out is asked for
    par_device_buffer d_palette(e, palette, (size_t)n_colors * sizeof(par_color), true);
    par_device_buffer d_fb(e, fb, n * sizeof(par_color), true), d_index(e, index_out, n, false);
    if (e == hipSuccess) {
        e = launch_quantize(nullptr, d_palette.as<par_color>(), n_colors, spread, params->width, d_fb.as<par_color>(),
                            row_begin, row_end, fb_out ? d_fb.as<par_color>() : nullptr, d_index.as<uint8_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (fb_out) d_fb.download(fb_out);
    d_index.download(index_out);
    return par_status_of(e);
}

int par_palette_ramp(const par_params* params, int levels, par_color* out, int capacity) {
    if (!params || !out || capacity < 0 || levels < 2 || levels > 255 || params->palette_size < 1 ||
        params->palette_size > PAR_MAX_PALETTE || !(params->ambient >= 0.f && params->ambient <= 1.f)) {
        return -PAR_ERR_INVALID_ARG;
    }
    const int count = params->palette_size * levels + 1;
    if (count > PAR_MAX_PALETTE) return -PAR_ERR_INVALID_ARG;
    const int a = (int)(params->ambient * 255.f);
    for (int i = 0; i < count - 1 && i < capacity; i++) {
        const par_color c = params->palette[i / levels];
        const int s = a + ((255 - a) * (i % levels)) / (levels - 1);
        out[i] = par_color{(uint8_t)((c.red * s) / 255), (uint8_t)((c.green * s) / 255), (uint8_t)((c.blue * s) / 255),
                           c.alpha};
    }
    if (count - 1 < capacity) {
        const uint8_t ch = (uint8_t)((float)params->background * params->ambient);  // par_background_fill's colour
        out[count - 1] = par_color{ch, ch, ch, 0};
    }
    return count;
}

}  // extern "C"
