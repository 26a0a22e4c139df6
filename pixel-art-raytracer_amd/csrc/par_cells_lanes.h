// par_cells_lanes.h — the cross-lane arithmetic of the colour-cell kernels, shared by par_cells.hip (cells_kernel) and the
// fitted-cells add-on (par_cells_fit.hip): a lane takes four consecutive pixels of one row of a cell, so a row of an
// 8-pixel-wide cell is two lanes, an 8 x 8 cell one DPP row of 16 lanes, and the larger cells two or four such rows. One
// implementation per step: __forceinline__ device code in an unnamed namespace, every unit gets its own copy.
#ifndef PAR_CELLS_LANES_H
#define PAR_CELLS_LANES_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_post.h"

namespace {

// The source lane of a DPP step within a row of 16 lanes; every lane of a wavefront is active where these are used.
constexpr int DPP_QUAD_1032 = 0xB1, DPP_QUAD_2301 = 0x4E, DPP_ROW_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140;

template <int CTRL>
__device__ __forceinline__ uint32_t from_lane(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}

// The sum of a word over each row of 16 lanes, in every lane of the row.
__device__ __forceinline__ uint32_t row_sum(uint32_t v) {
    v += from_lane<DPP_QUAD_1032>(v);
    v += from_lane<DPP_QUAD_2301>(v);
    v += from_lane<DPP_ROW_HALF_MIRROR>(v);
    v += from_lane<DPP_ROW_MIRROR>(v);
    return v;
}

// The two halves of the row sums `w` added over the LANES / 16 rows of a cell, in every lane of the cell.
template <int LANES>
__device__ __forceinline__ void cell_sums(uint32_t w, uint32_t& even, uint32_t& odd) {
    even = w & 0xFFFFu;
    odd = w >> 16;
    if (LANES >= 32) {
        const uint32_t other = (uint32_t)__shfl_xor((int)w, 16);
        even += other & 0xFFFFu;
        odd += other >> 16;
    }
    if (LANES == 64) {
        even += (uint32_t)__shfl_xor((int)even, 32);
        odd += (uint32_t)__shfl_xor((int)odd, 32);
    }
}

// The L1 distances of four pixels (alpha byte 0) to the nearest of the K entries at `sub` (a wave-uniform address).
__device__ __forceinline__ void nearest_distances(const uint32_t rgb[4], const uint32_t* __restrict__ sub, int K,
                                                  uint32_t d[4]) {
    for (int i = 0; i < 4; i++) d[i] = ~0u;
    int k = 0;
    for (; k + 8 <= K; k += 8) {
        uint32_t e[8];
        for (int n = 0; n < 8; n++) e[n] = sub[k + n] & QUANT_RGB;
        for (int n = 0; n < 8; n += 2) {
            for (int i = 0; i < 4; i++) {
                d[i] = min3u(d[i], __builtin_amdgcn_sad_u8(rgb[i], e[n], 0u), __builtin_amdgcn_sad_u8(rgb[i], e[n + 1], 0u));
            }
        }
    }
    for (; k < K; k++) {
        const uint32_t e = sub[k] & QUANT_RGB;
        for (int i = 0; i < 4; i++) d[i] = std::min(d[i], __builtin_amdgcn_sad_u8(rgb[i], e, 0u));
    }
}

}  // namespace

#endif
