// par_pattern.hip — pattern dither: a frame quantised to a palette by Thomas Knoll's pattern dithering on the device
// (par_quantize_pattern_device, par_quantize_pattern_host). The contract is beside the declarations in par_raytracer.h;
// nothing here knows a par_context, and par_quantize.hip knows nothing of this.
//
// The kernel follows quantize_kernel (par_quantize.hip). The rows of a call are one dense array of n pixels. A lane
// takes a GROUP of 2 consecutive pixels (two, not quantise's four: a pixel carries 16 sort keys, and two pixels' keys
// with the error terms stay within 64 vector registers); the groups are laid so that their first pixels sit on 8-byte
// boundaries of the source (`lead` pixels that do not exist come before pixel 0), and a group that lies wholly inside
// the array is one global_load_dwordx2, one 16-bit store of two indices and one dwordx2 store of fb_out. The (at most
// two) groups that hang over an end, and every group when the caller's pointers do not share an 8-byte phase, go pixel
// by pixel.
// A candidate is one search of quantise's: the entries come through the scalar cache, eight at a time, v_sad_hi_u8
// gives (L1 distance << 16) + index on the clamped bytes of t, v_min3_u32 takes two entries. What a candidate needs
// of the entry it found, its colour for the error term and its sort key, comes from a table the workgroup builds in LDS
// once (one ds_read_b64 a candidate and pixel). `depth` is a kernel argument and the same in every lane: the loop over
// the candidates is unrolled, each key has a register of its own, and a candidate j >= depth is a branch over its code.
// The keys not reached stay 0xFFFFFFFF, above every real key (24 bits), so a sorting network over 4, 8 or 16 registers,
// the smallest that holds `depth`, leaves the real keys in front in ascending order; the rank is then taken by a tree of
// selects on its bits. No scratch memory is used.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_fastdiv.h"
#include "par_hostcall.h"
#include "par_post.h"
#include "par_raytracer.h"

namespace {

constexpr int PATTERN_THREADS = 256;
constexpr int PATTERN_PX = 2;  // pixels of a lane
constexpr int PATTERN_MAX_DEPTH = 16;
static_assert(PATTERN_THREADS == PAR_MAX_PALETTE, "thread i of a workgroup writes entry i of the table in LDS");

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// Batcher's odd-even merge sort over k[0..N), N a power of two: 5, 19 and 63 compare-exchanges for N = 4, 8 and 16.
// Every index is a constant once the loops are unrolled.
template <int N>
__device__ __forceinline__ void sort_keys(uint32_t (&k)[PATTERN_MAX_DEPTH]) {
#pragma unroll
    for (int p = 1; p < N; p *= 2) {
#pragma unroll
        for (int s = p; s >= 1; s /= 2) {
#pragma unroll
            for (int j = s % p; j + s < N; j += 2 * s) {
#pragma unroll
                for (int i = 0; i < s && i + j + s < N; i++) {
                    if ((i + j) / (2 * p) == (i + j + s) / (2 * p)) {
                        const uint32_t lo = std::min(k[i + j], k[i + j + s]), hi = std::max(k[i + j], k[i + j + s]);
                        k[i + j] = lo;
                        k[i + j + s] = hi;
                    }
                }
            }
        }
    }
}

// k[rank], rank < N, by a tree of selects on the bits of rank: N - 1 v_cndmask_b32. (Written with a mask on purpose.
// As `up ? v[i + s] : v[i]` the selects are folded into an index while the keys are still an array in memory, and come
// out as a chain of sixteen compares and selects for every node of the tree.)
template <int N>
__device__ __forceinline__ uint32_t key_at(const uint32_t (&k)[PATTERN_MAX_DEPTH], uint32_t rank) {
    uint32_t v[N];
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = k[i];
#pragma unroll
    for (int s = 1; s < N; s *= 2) {
        const uint32_t up = 0u - ((rank / (uint32_t)s) & 1u);  // all ones or none
#pragma unroll
        for (int i = 0; i + s < N; i += 2 * s) v[i] ^= (v[i] ^ v[i + s]) & up;
    }
    return v[0];
}

template <int N>
__device__ __forceinline__ uint32_t ranked(uint32_t (&k)[PATTERN_MAX_DEPTH], uint32_t rank) {
    sort_keys<N>(k);
    return key_at<N>(k, rank);
}

template <bool VEC>
__global__ __launch_bounds__(PATTERN_THREADS) void pattern_kernel(const uint32_t* fb, uint32_t* fb_out, uint8_t* index_out,
                                                                  const uint32_t* __restrict__ palette, int n_colors,
                                                                  int depth, int strength, uint32_t n_px, uint32_t lead,
                                                                  uint32_t width, par_udiv31 by_width, uint32_t row_begin) {
    // entry i as a candidate needs it: {its colour, its sort key (luma << 8) | i}; the entries past n_colors - 1 are
    // never read (an index never exceeds n_colors - 1: the clamp only keeps the load inside the palette)
    __shared__ u32x2 table[PAR_MAX_PALETTE];
    {
        const uint32_t i = std::min<uint32_t>(threadIdx.x, (uint32_t)n_colors - 1u);
        const uint32_t c = palette[i] & QUANT_RGB;
        const uint32_t luma = 77u * (c & 0xFFu) + 150u * ((c >> 8) & 0xFFu) + 29u * (c >> 16);
        const u32x2 v = {c, (luma << 8) | i};
        table[threadIdx.x] = v;
    }
    __syncthreads();

    // pixel i of the group is u + i - lead; it exists when that is in [0, n_px)
    const uint32_t u = (uint32_t)PATTERN_PX * (blockIdx.x * (uint32_t)PATTERN_THREADS + threadIdx.x);
    if (u >= n_px + lead) return;
    const uint32_t base = u - lead;  // (wraps for the first group of a launch with lead > 0: then `full` is false)
    const bool full = u >= lead && base + (uint32_t)PATTERN_PX <= n_px;
    bool live[PATTERN_PX];
    uint32_t src[PATTERN_PX];
    if (VEC && full) {
        const u32x2 v = *reinterpret_cast<const u32x2*>(fb + base);
        for (int i = 0; i < PATTERN_PX; i++) { live[i] = true; src[i] = v[i]; }
    } else {
        for (int i = 0; i < PATTERN_PX; i++) {
            live[i] = u + i >= lead && base + i < n_px;
            src[i] = live[i] ? fb[base + i] : 0u;
        }
    }

    // the rank of each pixel, from its column and absolute row: those of the group's first pixel that exists, then one
    // step per pixel
    uint32_t rank[PATTERN_PX];
    {
        const uint32_t first = u >= lead ? base : 0u;
        const uint32_t q = par_udiv31_quotient(first, by_width);
        uint32_t x = first - q * width, y = row_begin + q;
        for (int i = 0; i < PATTERN_PX; i++) {
            if (i > 0 && u + i > lead) {
                x++;
                if (x == width) { x = 0; y++; }
            }
            const uint32_t t = (uint32_t)(BAYER_NIBBLES >> (((y & 3u) << 4) | ((x & 3u) << 2))) & 15u;
            rank[i] = (t * (uint32_t)depth) >> 4;
        }
    }

    int c[PATTERN_PX][3], e[PATTERN_PX][3];
    uint32_t keys[PATTERN_PX][PATTERN_MAX_DEPTH];
    for (int i = 0; i < PATTERN_PX; i++) {
        for (int ch = 0; ch < 3; ch++) {
            c[i][ch] = (int)((src[i] >> (8 * ch)) & 0xFFu);
            e[i][ch] = 0;
        }
#pragma unroll
        for (int j = 0; j < PATTERN_MAX_DEPTH; j++) keys[i][j] = ~0u;
    }

#pragma unroll
    for (int j = 0; j < PATTERN_MAX_DEPTH; j++) {
        // (not `break`: with it the compiler keeps the loop rolled and indexes the keys' registers through M0; a skipped
        // candidate is one scalar compare and branch)
        if (j >= depth) continue;
        // t = min(255, max(0, c + floor(e * strength / 256))): an arithmetic shift rounds towards minus infinity, and
        // |e * strength| <= 255 * 16 * 256 < 2^23 is a 24-bit product
        uint32_t rgb[PATTERN_PX];
        for (int i = 0; i < PATTERN_PX; i++) {
            uint32_t t = 0;
            for (int ch = 0; ch < 3; ch++) {
                const int v = std::min(255, std::max(0, c[i][ch] + (__mul24(e[i][ch], strength) >> 8)));
                t |= (uint32_t)v << (8 * ch);
            }
            rgb[i] = t;
        }

        uint32_t key[PATTERN_PX] = {~0u, ~0u};
        int p = 0;
        for (; p + 8 <= n_colors; p += 8) {
            uint32_t en[8];
            for (int k = 0; k < 8; k++) en[k] = palette[p + k] & QUANT_RGB;
            for (int k = 0; k < 8; k += 2) {
                for (int i = 0; i < PATTERN_PX; i++) {
                    key[i] = min3u(key[i], __builtin_amdgcn_sad_hi_u8(rgb[i], en[k], (uint32_t)(p + k)),
                                   __builtin_amdgcn_sad_hi_u8(rgb[i], en[k + 1], (uint32_t)(p + k + 1)));
                }
            }
        }
        for (; p < n_colors; p++) {
            const uint32_t en = palette[p] & QUANT_RGB;
            for (int i = 0; i < PATTERN_PX; i++) key[i] = std::min(key[i], __builtin_amdgcn_sad_hi_u8(rgb[i], en, (uint32_t)p));
        }

        for (int i = 0; i < PATTERN_PX; i++) {
            const u32x2 found = table[key[i] & 0xFFu];
            keys[i][j] = found[1];
            for (int ch = 0; ch < 3; ch++) e[i][ch] += c[i][ch] - (int)((found[0] >> (8 * ch)) & 0xFFu);
        }
    }

    uint32_t k[PATTERN_PX];
    if (depth <= 4) {
        for (int i = 0; i < PATTERN_PX; i++) k[i] = ranked<4>(keys[i], rank[i]) & 0xFFu;
    } else if (depth <= 8) {
        for (int i = 0; i < PATTERN_PX; i++) k[i] = ranked<8>(keys[i], rank[i]) & 0xFFu;
    } else {
        for (int i = 0; i < PATTERN_PX; i++) k[i] = ranked<16>(keys[i], rank[i]) & 0xFFu;
    }

    if (index_out) {
        if (VEC && full) {
            *reinterpret_cast<uint16_t*>(index_out + base) = (uint16_t)(k[0] | (k[1] << 8));
        } else {
            for (int i = 0; i < PATTERN_PX; i++) {
                if (live[i]) index_out[base + i] = (uint8_t)k[i];
            }
        }
    }
    if (fb_out) {
        uint32_t o[PATTERN_PX];
        for (int i = 0; i < PATTERN_PX; i++) o[i] = table[k[i]][0] | (src[i] & ~QUANT_RGB);
        if (VEC && full) {
            const u32x2 v = {o[0], o[1]};
            *reinterpret_cast<u32x2*>(fb_out + base) = v;
        } else {
            for (int i = 0; i < PATTERN_PX; i++) {
                if (live[i]) fb_out[base + i] = o[i];
            }
        }
    }
}

template <bool VEC>
void launch_one(hipStream_t stream, const uint32_t* fb, uint32_t* fb_out, uint8_t* index_out, const uint32_t* palette,
                int n_colors, int depth, int strength, uint32_t n_px, uint32_t lead, uint32_t width, uint32_t row_begin) {
    const uint32_t groups = (n_px + lead + PATTERN_PX - 1u) / PATTERN_PX;
    const uint32_t blocks = (groups + PATTERN_THREADS - 1) / PATTERN_THREADS;
    hipLaunchKernelGGL((pattern_kernel<VEC>), dim3(blocks), dim3(PATTERN_THREADS), 0, stream, fb, fb_out, index_out, palette,
                       n_colors, depth, strength, n_px, lead, width, par_udiv31_make(width), row_begin);
}

// Rows [row_begin, row_end) in launches of whole rows, at most PAR_MAX_LAUNCH_PX pixels each, as quantise cuts them (one
// launch for any frame below 8 GiB; a single row is never cut, and width < 2^31 keeps it inside par_udiv31's range).
hipError_t launch_pattern(hipStream_t stream, const par_color* d_palette, int n_colors, int depth, int strength, int width,
                          const par_color* fb, int row_begin, int row_end, par_color* fb_out, uint8_t* index_out) {
    // strength 0 leaves every t at the pixel: all candidates are the first, whatever the depth
    if (strength == 0) depth = 1;
    const uint32_t rows_per_launch = std::max<uint32_t>(1u, PAR_MAX_LAUNCH_PX / (uint32_t)width);
    const uint32_t* palette = reinterpret_cast<const uint32_t*>(d_palette);
    for (int r0 = row_begin; r0 < row_end;) {
        const uint32_t rows = std::min<uint32_t>(rows_per_launch, (uint32_t)(row_end - r0));
        const size_t at = (size_t)(r0 - row_begin) * (size_t)width;
        const uint32_t n_px = rows * (uint32_t)width;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(fb) + at;
        uint32_t* dst = fb_out ? reinterpret_cast<uint32_t*>(fb_out) + at : nullptr;
        uint8_t* idx = index_out ? index_out + at : nullptr;
        // pixels before the first 8-byte boundary of the source; the vector forms need every pointer in use to sit at
        // that same phase (fb_out: 8 bytes, index_out: its 2 bytes)
        const uintptr_t a = reinterpret_cast<uintptr_t>(src);
        const uint32_t head = (uint32_t)(((8u - (a & 7u)) & 7u) / 4u);
        const bool vec = (a & 3u) == 0 && (!dst || ((reinterpret_cast<uintptr_t>(dst) - a) & 7u) == 0) &&
                         (!idx || ((reinterpret_cast<uintptr_t>(idx) + head) & 1u) == 0);
        const uint32_t lead = vec ? (PATTERN_PX - head) % PATTERN_PX : 0u;
        if (vec) launch_one<true>(stream, src, dst, idx, palette, n_colors, depth, strength, n_px, lead, (uint32_t)width, (uint32_t)r0);
        else launch_one<false>(stream, src, dst, idx, palette, n_colors, depth, strength, n_px, lead, (uint32_t)width, (uint32_t)r0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        r0 += (int)rows;
    }
    return hipSuccess;
}

bool pattern_args_ok(const par_params* p, const par_color* palette, int n_colors, int depth, int strength,
                     const par_color* fb, int row_begin, int row_end, const par_color* fb_out, const uint8_t* index_out) {
    return p && palette && fb && (fb_out || index_out) && n_colors >= 1 && n_colors <= PAR_MAX_PALETTE && depth >= 1 &&
           depth <= PATTERN_MAX_DEPTH && strength >= 0 && strength <= 256 && p->width > 0 && row_begin >= 0 &&
           row_begin < row_end && row_end <= p->height;
}

}  // namespace

extern "C" {

int par_quantize_pattern_device(const par_params* params, void* stream, const par_color* d_palette, int n_colors,
                                int depth, int strength, const par_color* fb, int row_begin, int row_end,
                                par_color* fb_out, uint8_t* index_out) {
    if (!pattern_args_ok(params, d_palette, n_colors, depth, strength, fb, row_begin, row_end, fb_out, index_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    const hipError_t e = launch_pattern((hipStream_t)stream, d_palette, n_colors, depth, strength, params->width, fb,
                                        row_begin, row_end, fb_out, index_out);
    return e == hipSuccess ? PAR_OK : PAR_ERR_HIP;
}

int par_quantize_pattern_host(const par_params* params, int device, const par_color* palette, int n_colors, int depth,
                              int strength, const par_color* fb, int row_begin, int row_end, par_color* fb_out,
                              uint8_t* index_out) {
    if (!pattern_args_ok(params, palette, n_colors, depth, strength, fb, row_begin, row_end, fb_out, index_out)) {
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
        e = launch_pattern(nullptr, d_palette.as<par_color>(), n_colors, depth, strength, params->width,
                           d_fb.as<par_color>(), row_begin, row_end, fb_out ? d_fb.as<par_color>() : nullptr,
                           d_index.as<uint8_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (fb_out) d_fb.download(fb_out);
    d_index.download(index_out);
    return par_status_of(e);
}

}  // extern "C"
