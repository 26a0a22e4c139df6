// par_palette.hip — fitted palettes: a frame's palette made on the device by median cut over a 15-bit colour histogram
// (par_palette_reset_device, _count_device, _cut_device, _sum_device, _emit_device, par_palette_fit_host), and a palette
// refined by k-medians rounds (par_palette_refine_device, par_palette_refine_host). The contracts
// are beside the declarations in par_raytracer.h; nothing here knows a par_context, and everything is integer arithmetic
// whose result does not depend on the order in which the device runs it.
//
// Count and sum. The rows of a call are one dense array of n pixels, cut into slices, one per workgroup of 1024 lanes. A
// lane takes `rounds` groups of 4 consecutive pixels laid on the source's 16-byte boundaries as quantize_kernel lays
// them (`lead`): a whole group is one global_load_dwordx4, the groups over the ends go pixel by pixel. One round
// (PALETTE_PX_PER_ROUND = 4096 pixels a workgroup) up to PALETTE_TARGET_WGS workgroups, so that a small plane spreads
// over the CUs instead of walking its pixels on three of them; beyond that the rounds grow, up to PALETTE_MAX_ROUNDS,
// so that a large plane does not pay for zeroing and flushing thousands of histograms. The workgroup adds into a
// private histogram in LDS (count: all 32 768 cells, 128 KiB; sum: 256 x 4 dwords beside the 32 KiB table) and flushes
// the non-zero entries with device-scope global adds.
// Pixel art is mostly one colour: a lane merges equal neighbours before it adds, and a wavefront whose 256 pixels are
// all one cell (count) or one colour (sum) adds once; a wavefront of one entry but several colours (sum) reduces in
// registers first. A slice is at most 65 536 pixels, so no LDS dword overflows (65 536 x 255 < 2^32).
//
// Cut. One workgroup holds the histogram in LDS. A step visits the chosen region's tight box only: every lane adds its
// occupied cells into the region's 32 marginal bins on the split axis and ORs the cells' other two coordinates into a
// bit mask per bin; from those 32 bins the first wavefront finds the split, both halves' populations and tight bounds
// (prefix sum, ballots, OR reductions) and chooses the next region among the at most 256 (four a lane, then a butterfly).
// Two barriers a step. The table is written at the end, a region's box per wavefront.
//
// Refine (par_palette_refine_device, par_palette_refine_host). A round is par_quantize_device's index plane and then
// every entry's per-channel lower median over its pixels. An exact median wants 256 bins per entry and channel, 768 KiB,
// which no workgroup can hold; it is selected by radix instead, four bits a stage. tally_kernel<., false> counts the
// high nibble of every channel value per (entry, channel), select_kernel<false> finds per (entry, channel) the nibble
// the rank (n - 1) / 2 falls into and the rank within it, tally_kernel<., true> counts the low nibble of the values that
// have that high nibble, and select_kernel<true> finds the low nibble and writes the entry. The tally is laid as count
// and sum are (load_group, launch_over_rows) with 256 x 3 x 16 private dwords in LDS, 48 KiB, and keeps their two
// remedies: a wavefront of one index and one colour adds once, a lane merges equal neighbours. The stages are ordered by
// kernel boundaries alone, and a select leaves the bins zero for the next tally.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "par_hostcall.h"
#include "par_post.h"
#include "par_raytracer.h"

static_assert(sizeof(par_palette_work) == 172048 && offsetof(par_palette_work, hist) == 0 &&
                  offsetof(par_palette_work, sums) == 131072 && offsetof(par_palette_work, lut) == 139264 &&
                  offsetof(par_palette_work, n_entries) == 172032 && offsetof(par_palette_work, reserved) == 172036,
              "par_palette_work is a public layout");
static_assert(sizeof(par_palette_refine_work) == 54272 && offsetof(par_palette_refine_work, bins) == 0 &&
                  offsetof(par_palette_refine_work, rank) == 49152 && offsetof(par_palette_refine_work, high) == 53248 &&
                  alignof(par_palette_refine_work) <= 8,
              "par_palette_refine_work is a public layout");

namespace {

constexpr int PALETTE_THREADS = 1024;
constexpr int PALETTE_WAVES = PALETTE_THREADS / 64;
// Pixels of one workgroup of count_kernel and sum_kernel per round, the workgroups up to which a launch stays at one
// round, and the most rounds (tests/test_gpu_palette.py sizes its two largest frames by these).
constexpr uint32_t PALETTE_PX_PER_ROUND = 4u * PALETTE_THREADS;
constexpr uint32_t PALETTE_TARGET_WGS = 256;
constexpr uint32_t PALETTE_MAX_ROUNDS = 16;
constexpr uint32_t PALETTE_MAX_PX = 0x7FFFFFF0u;  // pixels of one launch: flat indices stay below 2^31
constexpr int CELLS = PAR_PALETTE_CELLS;
static_assert(PALETTE_MAX_ROUNDS * PALETTE_PX_PER_ROUND * 255ull < (1ull << 32), "a slice's channel sums fit an LDS dword");

__device__ __forceinline__ uint32_t cell_of(uint32_t px) {
    return ((px >> 3) & 31u) | (((px >> 11) & 31u) << 5) | (((px >> 19) & 31u) << 10);
}

// The group `g` of a launch: its four words (0 where a pixel does not exist), whether each exists, and whether all do.
template <bool VEC>
__device__ __forceinline__ bool load_group(const uint32_t* fb, uint32_t g, uint32_t n_px, uint32_t lead, uint32_t src[4],
                                           uint32_t live[4]) {
    // pixel i of the group is u + i - lead; it exists when that is in [0, n_px)
    const uint32_t u = 4u * g;
    const uint32_t base = u - lead;  // (wraps for the first group of a launch with lead > 0: then `full` is false)
    const bool inside = u < n_px + lead;
    const bool full = inside && u >= lead && base + 4u <= n_px;
    if (VEC && full) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(fb + base);
        for (int i = 0; i < 4; i++) { live[i] = 1u; src[i] = v[i]; }
    } else {
        for (int i = 0; i < 4; i++) {
            live[i] = (inside && u + i >= lead && base + i < n_px) ? 1u : 0u;
            src[i] = live[i] ? fb[base + i] : 0u;
        }
    }
    return full;
}

// ---- zeroing a work block ----------------------------------------------------------------------------------------

// Zeroes the n 8-byte words from dst on. A kernel and not hipMemsetAsync: the calls here are promised to be capturable as
// any stream-ordered launch is, and a memset node does not keep that promise everywhere. In a graph that torch.cuda.graph
// captured on the HIP 7.0 runtime that PyTorch-ROCm bundles, the memset of par_palette_reset_device zeroed the block in
// the graph's first launch and filled it with other bytes in every later one (tests/test_gpu_post_graph.py). A kernel
// node carries its arguments by value.
__global__ __launch_bounds__(256) void zero_kernel(unsigned long long* dst, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) dst[i] = 0ull;
}

// `bytes` bytes from the 8-byte aligned `dst` on, a multiple of 8
hipError_t launch_zero(hipStream_t stream, void* dst, size_t bytes) {
    const uint32_t n = (uint32_t)(bytes / 8);
    hipLaunchKernelGGL(zero_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, static_cast<unsigned long long*>(dst), n);
    return hipGetLastError();
}
static_assert(sizeof(par_palette_work) % 8 == 0 && sizeof(par_palette_refine_work::bins) % 8 == 0 &&
                  offsetof(par_palette_refine_work, bins) % 8 == 0,
              "launch_zero stores 8-byte words; the work blocks are 8-byte aligned");

// ---- count -------------------------------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(PALETTE_THREADS) void count_kernel(const uint32_t* fb, uint32_t* hist, uint32_t n_px,
                                                                uint32_t lead, uint32_t rounds) {
    __shared__ __attribute__((aligned(16))) uint32_t h[CELLS];
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int i = threadIdx.x; i < CELLS / 4; i += PALETTE_THREADS) reinterpret_cast<u32x4*>(h)[i] = zero;
    __syncthreads();

    const uint32_t g0 = blockIdx.x * rounds * PALETTE_THREADS + threadIdx.x;
    for (uint32_t it = 0; it < rounds; it++) {
        uint32_t src[4], n[4], c[4];
        const bool full = load_group<VEC>(fb, g0 + it * PALETTE_THREADS, n_px, lead, src, n);
        for (int i = 0; i < 4; i++) c[i] = cell_of(src[i]);
        // a wavefront whose 256 pixels are one cell adds once
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)c[0]);
        const bool one = full && c[0] == first && c[1] == first && c[2] == first && c[3] == first;
        if (__ballot(one) == ~0ull) {
            if ((threadIdx.x & 63) == 0) atomicAdd(&h[first], 256u);
            continue;
        }
        // equal neighbours merge to the right (a pixel that does not exist counts 0 wherever it lands)
        for (int i = 1; i < 4; i++) {
            if (c[i] == c[i - 1]) { n[i] += n[i - 1]; n[i - 1] = 0u; }
        }
        for (int i = 0; i < 4; i++) {
            if (n[i]) atomicAdd(&h[c[i]], n[i]);
        }
    }
    __syncthreads();

    for (int i = threadIdx.x; i < CELLS / 4; i += PALETTE_THREADS) {
        const u32x4 v = reinterpret_cast<const u32x4*>(h)[i];
        for (int k = 0; k < 4; k++) {
            if (v[k]) atomicAdd(&hist[4 * i + k], v[k]);
        }
    }
}

// ---- sum ---------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(PALETTE_THREADS) void sum_kernel(const uint32_t* fb, const uint8_t* lut,
                                                              unsigned long long* sums, uint32_t n_px, uint32_t lead,
                                                              uint32_t rounds) {
    __shared__ __attribute__((aligned(8))) uint8_t table[CELLS];
    __shared__ uint32_t s[PAR_MAX_PALETTE * 4];
    // (the block is 8-byte aligned and so is the table in it)
    for (int i = threadIdx.x; i < CELLS / 8; i += PALETTE_THREADS) {
        reinterpret_cast<uint64_t*>(table)[i] = reinterpret_cast<const uint64_t*>(lut)[i];
    }
    s[threadIdx.x] = 0u;
    static_assert(PAR_MAX_PALETTE * 4 == PALETTE_THREADS, "a lane per sum");
    __syncthreads();

    const uint32_t g0 = blockIdx.x * rounds * PALETTE_THREADS + threadIdx.x;
    for (uint32_t it = 0; it < rounds; it++) {
        uint32_t src[4], n[4], e[4], r[4], g[4], b[4];
        const bool full = load_group<VEC>(fb, g0 + it * PALETTE_THREADS, n_px, lead, src, n);
        for (int i = 0; i < 4; i++) {
            e[i] = table[cell_of(src[i])];
            r[i] = n[i] ? src[i] & 0xFFu : 0u;
            g[i] = n[i] ? (src[i] >> 8) & 0xFFu : 0u;
            b[i] = n[i] ? (src[i] >> 16) & 0xFFu : 0u;
        }
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)e[0]);
        const bool one_entry = full && e[0] == e0 && e[1] == e0 && e[2] == e0 && e[3] == e0;
        if (__ballot(one_entry) == ~0ull) {
            // a wavefront of one entry adds once: of one colour at that from lane 0's pixel, else reduced in registers
            const uint32_t c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(src[0] & QUANT_RGB));
            const bool one_colour = (src[0] & QUANT_RGB) == c0 && (src[1] & QUANT_RGB) == c0 &&
                                    (src[2] & QUANT_RGB) == c0 && (src[3] & QUANT_RGB) == c0;
            uint32_t R, G, B;
            if (__ballot(one_colour) == ~0ull) {
                R = 256u * (c0 & 0xFFu); G = 256u * ((c0 >> 8) & 0xFFu); B = 256u * ((c0 >> 16) & 0xFFu);
            } else {
                R = wave_sum(r[0] + r[1] + r[2] + r[3]);
                G = wave_sum(g[0] + g[1] + g[2] + g[3]);
                B = wave_sum(b[0] + b[1] + b[2] + b[3]);
            }
            if ((threadIdx.x & 63) == 0) {
                atomicAdd(&s[4 * e0 + 0], R);
                atomicAdd(&s[4 * e0 + 1], G);
                atomicAdd(&s[4 * e0 + 2], B);
                atomicAdd(&s[4 * e0 + 3], 256u);
            }
            continue;
        }
        // neighbours of one entry merge to the right
        for (int i = 1; i < 4; i++) {
            if (e[i] == e[i - 1]) {
                n[i] += n[i - 1]; r[i] += r[i - 1]; g[i] += g[i - 1]; b[i] += b[i - 1];
                n[i - 1] = 0u;
            }
        }
        for (int i = 0; i < 4; i++) {
            if (n[i]) {
                atomicAdd(&s[4 * e[i] + 0], r[i]);
                atomicAdd(&s[4 * e[i] + 1], g[i]);
                atomicAdd(&s[4 * e[i] + 2], b[i]);
                atomicAdd(&s[4 * e[i] + 3], n[i]);
            }
        }
    }
    __syncthreads();
    const uint32_t v = s[threadIdx.x];
    if (v) atomicAdd(&sums[threadIdx.x], (unsigned long long)v);
}

// Rows [row_begin, row_end) in launches of whole rows, at most PALETTE_MAX_PX pixels each, as launch_quantize cuts them.
template <class Launch>
hipError_t launch_over_rows(const par_color* fb, int width, int row_begin, int row_end, Launch launch) {
    const uint32_t rows_per_launch = std::max<uint32_t>(1u, PALETTE_MAX_PX / (uint32_t)width);
    for (int r0 = row_begin; r0 < row_end;) {
        const uint32_t rows = std::min<uint32_t>(rows_per_launch, (uint32_t)(row_end - r0));
        const uint32_t n_px = rows * (uint32_t)width;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(fb) + (size_t)(r0 - row_begin) * (size_t)width;
        // pixels before the first 16-byte boundary of the source
        const uintptr_t a = reinterpret_cast<uintptr_t>(src);
        const bool vec = (a & 3u) == 0;
        const uint32_t lead = vec ? (4u - (uint32_t)(((16u - (a & 15u)) & 15u) / 4u)) & 3u : 0u;
        const uint32_t groups = (n_px + lead + 3u) / 4u;
        const uint32_t rounds = std::min(PALETTE_MAX_ROUNDS, std::max(1u, (groups + PALETTE_THREADS * PALETTE_TARGET_WGS - 1) /
                                                                             (PALETTE_THREADS * PALETTE_TARGET_WGS)));
        launch(src, n_px, lead, vec, rounds, (groups + rounds * PALETTE_THREADS - 1) / (rounds * PALETTE_THREADS));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        r0 += (int)rows;
    }
    return hipSuccess;
}

hipError_t launch_count(hipStream_t stream, int width, const par_color* fb, int row_begin, int row_end,
                        par_palette_work* work) {
    uint32_t* hist = work->hist;
    return launch_over_rows(
        fb, width, row_begin, row_end,
        [&](const uint32_t* src, uint32_t n_px, uint32_t lead, bool vec, uint32_t rounds, uint32_t blocks) {
            const dim3 grid(blocks), block(PALETTE_THREADS);
            if (vec) hipLaunchKernelGGL(count_kernel<true>, grid, block, 0, stream, src, hist, n_px, lead, rounds);
            else hipLaunchKernelGGL(count_kernel<false>, grid, block, 0, stream, src, hist, n_px, lead, rounds);
        });
}

hipError_t launch_sum(hipStream_t stream, int width, const par_color* fb, int row_begin, int row_end,
                      par_palette_work* work) {
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(&work->sums[0][0]);
    const uint8_t* lut = work->lut;
    return launch_over_rows(
        fb, width, row_begin, row_end,
        [&](const uint32_t* src, uint32_t n_px, uint32_t lead, bool vec, uint32_t rounds, uint32_t blocks) {
            const dim3 grid(blocks), block(PALETTE_THREADS);
            if (vec) hipLaunchKernelGGL(sum_kernel<true>, grid, block, 0, stream, src, lut, sums, n_px, lead, rounds);
            else hipLaunchKernelGGL(sum_kernel<false>, grid, block, 0, stream, src, lut, sums, n_px, lead, rounds);
        });
}

// ---- cut ---------------------------------------------------------------------------------------------------------

// A corner of a box of cells is packed as a cell is: red | green << 5 | blue << 10.
__device__ __forceinline__ uint32_t coord(uint32_t packed, int axis) { return (packed >> (5 * axis)) & 31u; }
__device__ __forceinline__ uint32_t with_coord(uint32_t packed, int axis, uint32_t v) {
    return (packed & ~(31u << (5 * axis))) | (v << (5 * axis));
}
// the two axes beside `axis`, in the order red, green, blue
__device__ __forceinline__ int other1(int axis) { return axis == 0 ? 1 : 0; }
__device__ __forceinline__ int other2(int axis) { return axis == 2 ? 1 : 2; }

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o);
    return v;
}
__device__ __forceinline__ uint32_t lowest(uint32_t mask) { return (uint32_t)__builtin_ctz(mask); }
__device__ __forceinline__ uint32_t highest(uint32_t mask) { return 31u - (uint32_t)__builtin_clz(mask); }

struct CutState {
    unsigned long long m[32];  // the chosen region's population per coordinate on the split axis
    uint32_t occ1[32], occ2[32];  // per coordinate on the split axis: the occupied coordinates on the other two axes
    uint32_t box_lo[PAR_MAX_PALETTE], box_hi[PAR_MAX_PALETTE];      // a region's box
    uint32_t tight_lo[PAR_MAX_PALETTE], tight_hi[PAR_MAX_PALETTE];  // and its tight bounds
    unsigned long long pop[PAR_MAX_PALETTE];
    int chosen;     // region | axis << 8 of the next step, or -1: the cut is over
    int n_regions;
};

// a region's extent and the first axis that has it
__device__ __forceinline__ uint32_t extent_of(uint32_t lo, uint32_t hi, int* axis) {
    const uint32_t d0 = coord(hi, 0) - coord(lo, 0), d1 = coord(hi, 1) - coord(lo, 1), d2 = coord(hi, 2) - coord(lo, 2);
    const uint32_t e = std::max(d0, std::max(d1, d2));
    *axis = d0 == e ? 0 : (d1 == e ? 1 : 2);
    return e;
}

// The first wavefront chooses among regions [0, K): the largest extent >= 1, then the larger population, then the lower
// index. Leaves region | axis << 8 or -1 in st.chosen.
__device__ void choose_region(CutState& st, int K, int n_colors, int lane) {
    uint32_t be = 0u, bi = 0u;
    unsigned long long bn = 0ull;
    if (K < n_colors) {
        for (int k = lane; k < K; k += 64) {  // ascending: a later region wins only when it is strictly better
            int axis;
            const uint32_t e = extent_of(st.tight_lo[k], st.tight_hi[k], &axis);
            const unsigned long long n = st.pop[k];
            if (e > be || (e == be && e > 0u && n > bn)) { be = e; bn = n; bi = (uint32_t)k; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t oe = (uint32_t)__shfl_xor((int)be, o), oi = (uint32_t)__shfl_xor((int)bi, o);
            const unsigned long long on = __shfl_xor(bn, o);
            if (oe > be || (oe == be && (on > bn || (on == bn && oi < bi)))) { be = oe; bn = on; bi = oi; }
        }
    }
    if (lane == 0) {
        int axis = 0;
        if (be > 0u) (void)extent_of(st.tight_lo[bi], st.tight_hi[bi], &axis);
        st.chosen = be > 0u ? (int)(bi | ((uint32_t)axis << 8)) : -1;
    }
}

// Every lane of the workgroup: the occupied cells of the box [lo, hi] into the marginal bins on `axis`.
__device__ __forceinline__ void measure(CutState& st, const uint32_t* h, uint32_t lo, uint32_t hi, int axis) {
    const uint32_t l0 = coord(lo, 0), l1 = coord(lo, 1), l2 = coord(lo, 2);
    const uint32_t d0 = coord(hi, 0) - l0 + 1u, d1 = coord(hi, 1) - l1 + 1u, d2 = coord(hi, 2) - l2 + 1u;
    const uint32_t total = d0 * d1 * d2;
    for (uint32_t i = threadIdx.x; i < total; i += PALETTE_THREADS) {
        const uint32_t q = i / d0;
        const uint32_t c[3] = {l0 + (i - q * d0), l1 + q % d1, l2 + q / d1};
        const uint32_t v = h[c[0] | (c[1] << 5) | (c[2] << 10)];
        if (v) {
            const uint32_t a = c[axis];
            atomicAdd(&st.m[a], (unsigned long long)v);
            atomicOr(&st.occ1[a], 1u << c[other1(axis)]);
            atomicOr(&st.occ2[a], 1u << c[other2(axis)]);
        }
    }
}

__global__ __launch_bounds__(PALETTE_THREADS) void cut_kernel(par_palette_work* work, int n_colors) {
    __shared__ __attribute__((aligned(16))) uint32_t h[CELLS];
    __shared__ CutState st;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // (the block is 8-byte aligned, and so is its histogram)
    for (int i = threadIdx.x; i < CELLS / 2; i += PALETTE_THREADS) {
        reinterpret_cast<uint2*>(h)[i] = reinterpret_cast<const uint2*>(work->hist)[i];
    }
    reinterpret_cast<unsigned long long*>(&work->sums[0][0])[threadIdx.x] = 0ull;
    if (threadIdx.x < 32) { st.m[threadIdx.x] = 0ull; st.occ1[threadIdx.x] = 0u; st.occ2[threadIdx.x] = 0u; }
    __syncthreads();
    measure(st, h, 0u, (uint32_t)CELLS - 1u, 0);
    __syncthreads();

    int K = 0;  // (the first wavefront's count of regions)
    if (wave == 0) {
        // region 0: the whole cube
        const unsigned long long mv = lane < 32 ? st.m[lane] : 0ull;
        const uint32_t o1 = lane < 32 ? st.occ1[lane] : 0u, o2 = lane < 32 ? st.occ2[lane] : 0u;
        unsigned long long n = mv;
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
        const uint32_t on_axis = (uint32_t)__ballot(mv > 0ull), all1 = wave_or(o1), all2 = wave_or(o2);
        if (lane < 32) { st.m[lane] = 0ull; st.occ1[lane] = 0u; st.occ2[lane] = 0u; }
        if (n > 0ull) {
            K = 1;
            if (lane == 0) {
                st.box_lo[0] = 0u;
                st.box_hi[0] = (uint32_t)CELLS - 1u;
                st.tight_lo[0] = lowest(on_axis) | (lowest(all1) << 5) | (lowest(all2) << 10);
                st.tight_hi[0] = highest(on_axis) | (highest(all1) << 5) | (highest(all2) << 10);
                st.pop[0] = n;
            }
        }
        __threadfence_block();
        choose_region(st, K, n_colors, lane);
        if (lane == 0) st.n_regions = K;
    }
    __syncthreads();

    while (true) {
        const int chosen = st.chosen;
        if (chosen < 0) break;
        const int R = chosen & 0xFF, axis = chosen >> 8;
        measure(st, h, st.tight_lo[R], st.tight_hi[R], axis);
        __syncthreads();
        if (wave == 0) {
            const unsigned long long mv = lane < 32 ? st.m[lane] : 0ull;
            const uint32_t o1 = lane < 32 ? st.occ1[lane] : 0u, o2 = lane < 32 ? st.occ2[lane] : 0u;
            if (lane < 32) { st.m[lane] = 0ull; st.occ1[lane] = 0u; st.occ2[lane] = 0u; }
            const uint32_t t_lo = st.tight_lo[R], t_hi = st.tight_hi[R];
            const uint32_t lo = coord(t_lo, axis), hi = coord(t_hi, axis);
            const unsigned long long n = st.pop[R];
            // the split point: the smallest v in [lo, hi - 1] with 2 * (m[lo] + ... + m[v]) >= n, else hi - 1
            unsigned long long cum = mv;
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long below = __shfl_up(cum, o);
                if (lane >= o) cum += below;
            }
            const unsigned long long at = __ballot((uint32_t)lane >= lo && (uint32_t)lane < hi && 2ull * cum >= n);
            const uint32_t s = at ? (uint32_t)__builtin_ctzll(at) : hi - 1u;
            const unsigned long long n_left = __shfl(cum, (int)s);
            const bool left = (uint32_t)lane <= s;
            const uint32_t on_axis = (uint32_t)__ballot(mv > 0ull), upto = (2u << s) - 1u;
            const uint32_t a_l = on_axis & upto, a_r = on_axis & ~upto;
            const uint32_t l1 = wave_or(left ? o1 : 0u), r1 = wave_or(left ? 0u : o1);
            const uint32_t l2 = wave_or(left ? o2 : 0u), r2 = wave_or(left ? 0u : o2);
            if (lane == 0) {
                const int x1 = other1(axis), x2 = other2(axis);
                st.tight_lo[R] = with_coord(with_coord(with_coord(0u, axis, lowest(a_l)), x1, lowest(l1)), x2, lowest(l2));
                st.tight_hi[R] = with_coord(with_coord(with_coord(0u, axis, highest(a_l)), x1, highest(l1)), x2, highest(l2));
                st.tight_lo[K] = with_coord(with_coord(with_coord(0u, axis, lowest(a_r)), x1, lowest(r1)), x2, lowest(r2));
                st.tight_hi[K] = with_coord(with_coord(with_coord(0u, axis, highest(a_r)), x1, highest(r1)), x2, highest(r2));
                st.box_lo[K] = with_coord(st.box_lo[R], axis, s + 1u);
                st.box_hi[K] = st.box_hi[R];
                st.box_hi[R] = with_coord(st.box_hi[R], axis, s);
                st.pop[R] = n_left;
                st.pop[K] = n - n_left;
                st.n_regions = K + 1;
            }
            K++;
            __threadfence_block();
            choose_region(st, K, n_colors, lane);
        }
        __syncthreads();
    }

    // the table: a region's box per wavefront; without a region every cell maps to 0
    const int regions = st.n_regions;
    if (threadIdx.x == 0) work->n_entries = regions;
    if (regions == 0) {
        for (int i = threadIdx.x; i < CELLS / 8; i += PALETTE_THREADS) reinterpret_cast<uint64_t*>(work->lut)[i] = 0ull;
        return;
    }
    for (int k = wave; k < regions; k += PALETTE_WAVES) {
        const uint32_t lo = st.box_lo[k], hi = st.box_hi[k];
        const uint32_t l0 = coord(lo, 0), l1 = coord(lo, 1), l2 = coord(lo, 2);
        const uint32_t d0 = coord(hi, 0) - l0 + 1u, d1 = coord(hi, 1) - l1 + 1u, d2 = coord(hi, 2) - l2 + 1u;
        const uint32_t total = std::min(d0 * d1 * d2, (uint32_t)CELLS);
        for (uint32_t i = (uint32_t)lane; i < total; i += 64u) {
            const uint32_t q = i / d0;
            // (the mask cannot act on a box inside the cube: it is what keeps this store inside the table regardless)
            const uint32_t cell = (l0 + (i - q * d0)) | ((l1 + q % d1) << 5) | ((l2 + q / d1) << 10);
            work->lut[cell & (uint32_t)(CELLS - 1)] = (uint8_t)k;
        }
    }
}

// ---- emit --------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(PAR_MAX_PALETTE) void emit_kernel(const par_palette_work* work, int n_colors,
                                                               uint32_t* palette) {
    const int k = threadIdx.x;
    if (k >= n_colors) return;
    const int m = std::min(work->n_entries, n_colors);
    uint32_t out = 0u;
    if (m > 0) {
        const uint64_t* s = work->sums[k < m ? k : 0];
        const uint64_t n = s[3];
        if (n > 0) {
            out = 0xFF000000u;
            for (int c = 0; c < 3; c++) out |= (uint32_t)(((2ull * s[c] + n) / (2ull * n)) & 0xFFull) << (8 * c);
        }
    }
    palette[k] = out;
}

// ---- refine ------------------------------------------------------------------------------------------------------

constexpr int REFINE_BINS = PAR_MAX_PALETTE * 3 * 16;  // dwords of par_palette_refine_work::bins
constexpr int REFINE_MAX_ITERATIONS = 16;
static_assert(REFINE_BINS % (4 * PALETTE_THREADS) == 0, "a workgroup zeroes and flushes its tallies in whole rounds");

// `index` holds the launch's index bytes; index_words: index + (a whole group's first pixel) is on a 4-byte boundary.
template <bool VEC, bool LO>
__global__ __launch_bounds__(PALETTE_THREADS) void tally_kernel(const uint32_t* fb, const uint8_t* index, bool index_words,
                                                                par_palette_refine_work* work, uint32_t n_px,
                                                                uint32_t lead, uint32_t rounds) {
    __shared__ __attribute__((aligned(16))) uint32_t t[REFINE_BINS];
    __shared__ uint32_t high[PAR_MAX_PALETTE];
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int i = threadIdx.x; i < REFINE_BINS / 4; i += PALETTE_THREADS) reinterpret_cast<u32x4*>(t)[i] = zero;
    if (LO && threadIdx.x < PAR_MAX_PALETTE) high[threadIdx.x] = work->high[threadIdx.x];
    __syncthreads();

    const uint32_t g0 = blockIdx.x * rounds * PALETTE_THREADS + threadIdx.x;
    for (uint32_t it = 0; it < rounds; it++) {
        uint32_t src[4], n[4], k[4];
        const uint32_t g = g0 + it * PALETTE_THREADS;
        const bool full = load_group<VEC>(fb, g, n_px, lead, src, n);
        const uint32_t base = 4u * g - lead;  // (as load_group forms it; used only where a pixel exists)
        if (full && index_words) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(index + base);
            for (int i = 0; i < 4; i++) k[i] = (w >> (8 * i)) & 0xFFu;
        } else {
            for (int i = 0; i < 4; i++) k[i] = n[i] ? index[base + i] : 0u;
        }
        for (int i = 0; i < 4; i++) src[i] &= QUANT_RGB;
        // a wavefront of one index and one colour adds once
        const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)k[0]);
        const uint32_t c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)src[0]);
        const bool one = full && k[0] == k0 && k[1] == k0 && k[2] == k0 && k[3] == k0 && src[0] == c0 && src[1] == c0 &&
                         src[2] == c0 && src[3] == c0;
        if (__ballot(one) == ~0ull) {
            if ((threadIdx.x & 63) == 0) tally_add<LO>(t, high, k0, c0, 256u);
            continue;
        }
        // equal neighbours merge to the right (a pixel that does not exist counts 0 wherever it lands)
        for (int i = 1; i < 4; i++) {
            if (k[i] == k[i - 1] && src[i] == src[i - 1]) { n[i] += n[i - 1]; n[i - 1] = 0u; }
        }
        for (int i = 0; i < 4; i++) {
            if (n[i]) tally_add<LO>(t, high, k[i], src[i], n[i]);
        }
    }
    __syncthreads();

    uint32_t* const bins = &work->bins[0][0][0];
    for (int i = threadIdx.x; i < REFINE_BINS / 4; i += PALETTE_THREADS) {
        const u32x4 v = reinterpret_cast<const u32x4*>(t)[i];
        for (int j = 0; j < 4; j++) {
            if (v[j]) atomicAdd(&bins[4 * i + j], v[j]);
        }
    }
}

// One lane per entry. Stage hi (LO false): per channel n is the sum of the 16 bins and the rank (n - 1) / 2; the high
// nibble is the first at which the running count passes the rank; it goes to `high`, the rank within it to `rank`, n to
// rank[k][3]. Stage lo: the low nibble likewise from the rank within; an entry with pixels gets its three medians and
// alpha 255; the entries that changed are counted into changed[0] where `changed` is given. Both leave the bins zero.
template <bool LO>
__global__ __launch_bounds__(PAR_MAX_PALETTE) void select_kernel(par_palette_refine_work* work, uint32_t* palette,
                                                                 int n_colors, int32_t* changed) {
    const int k = threadIdx.x;
    const uint32_t high = LO ? work->high[k] : 0u;
    uint32_t n_k = LO ? work->rank[k][3] : 0u, picked = 0u;
    for (int c = 0; c < 3; c++) {
        uint32_t* const row = work->bins[k][c];
        uint32_t b[16], n = 0u;
        // (the block is 8-byte aligned, and so is a row of 16 dwords in it)
        for (int v = 0; v < 16; v += 2) {
            const uint2 two = *reinterpret_cast<const uint2*>(row + v);
            b[v] = two.x; b[v + 1] = two.y;
            n += two.x + two.y;
            *reinterpret_cast<uint2*>(row + v) = make_uint2(0u, 0u);
        }
        const uint32_t rank = LO ? work->rank[k][c] : (n ? (n - 1u) / 2u : 0u);
        uint32_t nibble = 0u, below = 0u, cum = 0u;
        bool found = false;
        for (int v = 0; v < 16; v++) {
            if (!found && cum + b[v] > rank) { nibble = (uint32_t)v; below = cum; found = true; }
            cum += b[v];
        }
        if (LO) {
            picked |= (((high >> (8 * c)) & 0xF0u) | nibble) << (8 * c);
        } else {
            picked |= nibble << (8 * c + 4);
            work->rank[k][c] = rank - below;
            n_k = n;
        }
    }
    if (LO) {
        bool moved = false;
        if (k < n_colors && n_k > 0u) {
            const uint32_t entry = picked | 0xFF000000u;
            moved = palette[k] != entry;
            palette[k] = entry;
        }
        const int total = __syncthreads_count(moved);
        if (changed && k == 0) changed[0] = total;
    } else {
        work->rank[k][3] = n_k;
        work->high[k] = picked;
    }
}

template <bool LO>
hipError_t launch_tally(hipStream_t stream, int width, const par_color* fb, int row_begin, int row_end,
                        const uint8_t* d_index, par_palette_refine_work* work) {
    return launch_over_rows(
        fb, width, row_begin, row_end,
        [&](const uint32_t* src, uint32_t n_px, uint32_t lead, bool vec, uint32_t rounds, uint32_t blocks) {
            const dim3 grid(blocks), block(PALETTE_THREADS);
            const uint8_t* index = d_index + (src - reinterpret_cast<const uint32_t*>(fb));
            // a whole group's first pixel is 4 * g - lead
            const bool index_words = ((reinterpret_cast<uintptr_t>(index) - lead) & 3u) == 0;
            if (vec) hipLaunchKernelGGL((tally_kernel<true, LO>), grid, block, 0, stream, src, index, index_words, work, n_px, lead, rounds);
            else hipLaunchKernelGGL((tally_kernel<false, LO>), grid, block, 0, stream, src, index, index_words, work, n_px, lead, rounds);
        });
}

template <bool LO>
hipError_t launch_select(hipStream_t stream, par_palette_refine_work* work, par_color* d_palette, int n_colors,
                         int32_t* d_changed) {
    hipLaunchKernelGGL(select_kernel<LO>, dim3(1), dim3(PAR_MAX_PALETTE), 0, stream, work, reinterpret_cast<uint32_t*>(d_palette),
                       n_colors, d_changed);
    return hipGetLastError();
}

// The rounds of a refinement on `stream`, the arguments checked: a par_status.
int run_refine(const par_params* params, hipStream_t stream, const par_color* fb, int row_begin, int row_end,
               par_color* d_palette, int n_colors, int iterations, uint8_t* d_index, par_palette_refine_work* work,
               int32_t* d_changed) {
    const int W = params->width;
    if (launch_zero(stream, work->bins, sizeof(work->bins)) != hipSuccess) return PAR_ERR_HIP;
    for (int it = 0; it < iterations; it++) {
        const int rc = par_quantize_device(params, stream, d_palette, n_colors, 0, fb, row_begin, row_end, nullptr, d_index);
        if (rc != PAR_OK) return rc;
        hipError_t e = launch_tally<false>(stream, W, fb, row_begin, row_end, d_index, work);
        if (e == hipSuccess) e = launch_select<false>(stream, work, d_palette, n_colors, nullptr);
        if (e == hipSuccess) e = launch_tally<true>(stream, W, fb, row_begin, row_end, d_index, work);
        if (e == hipSuccess) e = launch_select<true>(stream, work, d_palette, n_colors, it == iterations - 1 ? d_changed : nullptr);
        if (e != hipSuccess) return PAR_ERR_HIP;
    }
    return PAR_OK;
}

bool work_ok(const par_palette_work* work) { return work && (reinterpret_cast<uintptr_t>(work) & 7u) == 0; }
bool colors_ok(int n_colors) { return n_colors >= 1 && n_colors <= PAR_MAX_PALETTE; }
bool plane_args_ok(const par_params* p, const par_color* fb, int row_begin, int row_end) {
    return p && fb && p->width > 0 && row_begin >= 0 && row_begin < row_end && row_end <= p->height;
}

int status_of_launch() { return hipGetLastError() == hipSuccess ? PAR_OK : PAR_ERR_HIP; }

// PAR_OK, or the status the contract gives these arguments of a refinement (`palette`: the host's or the device's)
int refine_args_status(const par_params* params, const par_color* fb, int row_begin, int row_end, const par_color* palette,
                       int n_colors, int iterations) {
    if (!plane_args_ok(params, fb, row_begin, row_end) || !palette || !colors_ok(n_colors) || iterations < 1 ||
        iterations > REFINE_MAX_ITERATIONS) {
        return PAR_ERR_INVALID_ARG;
    }
    // the tallies are 32-bit
    return (int64_t)(row_end - row_begin) * (int64_t)params->width >= (1ll << 32) ? PAR_ERR_UNSUPPORTED : PAR_OK;
}

}  // namespace

extern "C" {

int par_palette_reset_device(void* stream, par_palette_work* work) {
    if (!work_ok(work)) return PAR_ERR_INVALID_ARG;
    return launch_zero((hipStream_t)stream, work, sizeof(par_palette_work)) == hipSuccess ? PAR_OK : PAR_ERR_HIP;
}

int par_palette_count_device(const par_params* params, void* stream, const par_color* fb, int row_begin, int row_end,
                             par_palette_work* work) {
    if (!plane_args_ok(params, fb, row_begin, row_end) || !work_ok(work)) return PAR_ERR_INVALID_ARG;
    return launch_count((hipStream_t)stream, params->width, fb, row_begin, row_end, work) == hipSuccess ? PAR_OK : PAR_ERR_HIP;
}

int par_palette_cut_device(void* stream, par_palette_work* work, int n_colors) {
    if (!work_ok(work) || !colors_ok(n_colors)) return PAR_ERR_INVALID_ARG;
    hipLaunchKernelGGL(cut_kernel, dim3(1), dim3(PALETTE_THREADS), 0, (hipStream_t)stream, work, n_colors);
    return status_of_launch();
}

int par_palette_sum_device(const par_params* params, void* stream, const par_color* fb, int row_begin, int row_end,
                           par_palette_work* work) {
    if (!plane_args_ok(params, fb, row_begin, row_end) || !work_ok(work)) return PAR_ERR_INVALID_ARG;
    return launch_sum((hipStream_t)stream, params->width, fb, row_begin, row_end, work) == hipSuccess ? PAR_OK : PAR_ERR_HIP;
}

int par_palette_emit_device(void* stream, const par_palette_work* work, int n_colors, par_color* d_palette) {
    if (!work_ok(work) || !colors_ok(n_colors) || !d_palette) return PAR_ERR_INVALID_ARG;
    hipLaunchKernelGGL(emit_kernel, dim3(1), dim3(PAR_MAX_PALETTE), 0, (hipStream_t)stream, work, n_colors,
                       reinterpret_cast<uint32_t*>(d_palette));
    return status_of_launch();
}

int par_palette_fit_host(const par_params* params, int device, const par_color* fb, int row_begin, int row_end,
                         int n_colors, par_color* palette_out, int* n_entries_out) {
    if (!plane_args_ok(params, fb, row_begin, row_end) || !colors_ok(n_colors) || !palette_out || !n_entries_out) {
        return PAR_ERR_INVALID_ARG;
    }
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    const size_t n = (size_t)(row_end - row_begin) * (size_t)params->width;
    par_device_buffer d_fb(e, fb, n * sizeof(par_color), true);
    // (neither buffer is uploaded: `palette_out` only says that they are in use)
    par_device_buffer d_work(e, palette_out, sizeof(par_palette_work), false);
    par_device_buffer d_palette(e, palette_out, (size_t)n_colors * sizeof(par_color), false);
    par_palette_work* work = d_work.as<par_palette_work>();
    if (e == hipSuccess) e = launch_zero(nullptr, work, sizeof(par_palette_work));
    if (e == hipSuccess) e = launch_count(nullptr, params->width, d_fb.as<par_color>(), row_begin, row_end, work);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(cut_kernel, dim3(1), dim3(PALETTE_THREADS), 0, nullptr, work, n_colors);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = launch_sum(nullptr, params->width, d_fb.as<par_color>(), row_begin, row_end, work);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(emit_kernel, dim3(1), dim3(PAR_MAX_PALETTE), 0, nullptr, work, n_colors, d_palette.as<uint32_t>());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    int n_entries = 0;
    if (e == hipSuccess) e = hipMemcpy(&n_entries, &work->n_entries, sizeof(int), hipMemcpyDeviceToHost);
    d_palette.download(palette_out);
    if (e == hipSuccess) *n_entries_out = n_entries;
    return par_status_of(e);
}

int par_palette_refine_device(const par_params* params, void* stream, const par_color* fb, int row_begin, int row_end,
                              par_color* d_palette, int n_colors, int iterations, uint8_t* d_index,
                              par_palette_refine_work* work, int32_t* d_changed) {
    if (!d_index || !work || (reinterpret_cast<uintptr_t>(work) & 7u) != 0) return PAR_ERR_INVALID_ARG;
    const int rc = refine_args_status(params, fb, row_begin, row_end, d_palette, n_colors, iterations);
    if (rc != PAR_OK) return rc;
    return run_refine(params, (hipStream_t)stream, fb, row_begin, row_end, d_palette, n_colors, iterations, d_index, work,
                      d_changed);
}

int par_palette_refine_host(const par_params* params, int device, const par_color* fb, int row_begin, int row_end,
                            par_color* palette, int n_colors, int iterations, int* changed_out) {
    int rc = refine_args_status(params, fb, row_begin, row_end, palette, n_colors, iterations);
    if (rc != PAR_OK) return rc;
    rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    const size_t n = (size_t)(row_end - row_begin) * (size_t)params->width;
    par_device_buffer d_fb(e, fb, n * sizeof(par_color), true);
    par_device_buffer d_palette(e, palette, (size_t)n_colors * sizeof(par_color), true);
    // (none of the three is uploaded: `palette` only says that they are in use)
    par_device_buffer d_index(e, palette, n, false);
    par_device_buffer d_work(e, palette, sizeof(par_palette_refine_work), false);
    par_device_buffer d_changed(e, palette, sizeof(int32_t), false);
    if (e != hipSuccess) return par_status_of(e);
    rc = run_refine(params, nullptr, d_fb.as<par_color>(), row_begin, row_end, d_palette.as<par_color>(), n_colors,
                    iterations, d_index.as<uint8_t>(), d_work.as<par_palette_refine_work>(), d_changed.as<int32_t>());
    if (rc != PAR_OK) return rc;
    e = hipDeviceSynchronize();
    int32_t changed = 0;
    d_changed.download(&changed);
    d_palette.download(palette);
    if (e == hipSuccess && changed_out) *changed_out = changed;
    return par_status_of(e);
}

}  // extern "C"
