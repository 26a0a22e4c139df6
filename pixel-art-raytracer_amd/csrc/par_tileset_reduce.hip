// par_tileset_reduce.hip — the tile-budget add-on (libpar_tileset_reduce.so): a tile set and its map reduced to at most
// K tiles (par_tileset_reduce_device, par_tileset_reduce_host). The contract is beside the declarations in
// addons/include/par_tileset_reduce.h; nothing here knows a par_context or a par_params, and nothing here is linked
// into libpar_raytracer.so.
//
// The launches of a call, budget + 6 of them, none sized by T:
//   entry    T = min(*count, capacity) into the work block's head, the usage counts to 0
//   usage    u[i]: a histogram a workgroup in LDS, flushed with integer atomics (a sum of integers has no order)
//   start    d, a, g and the kept marks of every tile, and a partial maximum of u a workgroup
//   step     `budget` times: the new centre is the maximum of the partial maxima the launch before left (every workgroup
//            takes it for itself: 128 eight-byte words at most), its allowed images go to LDS as colours, every tile's
//            (d, a, g) takes the lexicographic minimum with (D, centre, f), and the workgroup leaves the partial maximum
//            of u * d over its tiles outside the kept set for the next launch. The two sets of partials alternate.
//   number   one workgroup: the kept marks scanned into new numbers, the remap, the count and the error
//   compact  the kept tiles to tiles_out
//   map      map_out
// One launch a step and not one workgroup that loops: a step over 4096 tiles of 16 x 16 under four images is 4 M pixel
// differences, tens of microseconds on one compute unit and a few on 128 (8.7 us a step measured, 4.2 to 4.8 us for a
// few hundred tiles of 8 x 8: DESIGN, "Tile budgets"), and a kernel boundary is the only wait between workgroups that
// costs nothing to get right: no workgroup waits on another, nothing spins.
// A maximum is taken on one 64-bit key, 1 << 63 | (u * d) << 12 | (4095 - i): the largest product, the lowest number
// among equals; 0 is "no tile left". u < 2^21 and d <= 256 * 765 < 2^18, so the product stays below 2^39.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_hostcall.h"
#include "par_tileset_reduce.h"

namespace {

constexpr uint32_t TR_THREADS = 256;
constexpr uint32_t TR_LANES_PER_TILE = 8;
constexpr uint32_t TR_TILES_PER_GROUP = TR_THREADS / TR_LANES_PER_TILE;  // 32
constexpr uint32_t TR_MAX_GROUPS = PAR_TILESET_REDUCE_MAX_TILES / TR_TILES_PER_GROUP;  // 128
constexpr uint32_t TR_HEAD_BYTES = 4096;  // T, min(T, K); the partials at 1024 and 2048
constexpr uint32_t TR_WORDS_PER_TILE = 5;
constexpr uint32_t TR_ID_MASK = 0x3FFFFFFFu;
constexpr uint32_t TR_NUMBER_THREADS = 1024;
constexpr uint32_t TR_TILES_PER_THREAD = PAR_TILESET_REDUCE_MAX_TILES / TR_NUMBER_THREADS;  // 4
constexpr uint32_t TR_USAGE_CELLS_PER_GROUP = TR_THREADS * 16;
constexpr uint64_t TR_LIVE = 1ull << 63;
static_assert(TR_MAX_GROUPS * 8 <= 1024 && TR_MAX_GROUPS <= 2 * 64, "a set of partials fits its 1024 bytes and two loads a lane");
static_assert(PAR_TILESET_REDUCE_MAX_TILES == 4096, "the key holds 4095 - i in 12 bits");

struct Work {
    uint32_t* head;     // [0] T, [1] min(T, K)
    uint64_t* part[2];  // the partial maxima a step reads and the ones it writes
    uint32_t *u, *d, *ag, *kept, *remap;
};

Work work_of(void* block, uint32_t capacity) {
    char* b = static_cast<char*>(block);
    uint32_t* per_tile = reinterpret_cast<uint32_t*>(b + TR_HEAD_BYTES);
    return {reinterpret_cast<uint32_t*>(b),
            {reinterpret_cast<uint64_t*>(b + 1024), reinterpret_cast<uint64_t*>(b + 2048)},
            per_tile, per_tile + capacity, per_tile + 2 * (size_t)capacity, per_tile + 3 * (size_t)capacity,
            per_tile + 4 * (size_t)capacity};
}

__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
    for (int s = 32; s; s >>= 1) v = std::max(v, (uint64_t)__shfl_xor((unsigned long long)v, s));
    return v;
}

__device__ __forceinline__ uint64_t key_of(uint64_t score, uint32_t i) {
    return TR_LIVE | (score << 12) | (uint64_t)(PAR_TILESET_REDUCE_MAX_TILES - 1 - i);
}

__global__ __launch_bounds__(TR_THREADS) void reduce_entry_kernel(Work w, const uint32_t* count, uint32_t capacity,
                                                                  uint32_t budget) {
    const uint32_t i = blockIdx.x * TR_THREADS + threadIdx.x;
    if (i == 0) {
        const uint32_t T = std::min(*count, capacity);
        w.head[0] = T;
        w.head[1] = std::min(T, budget);
    }
    if (i < capacity) w.u[i] = 0;
}

__global__ __launch_bounds__(TR_THREADS) void reduce_usage_kernel(Work w, const uint32_t* map, uint32_t n_cells) {
    __shared__ uint32_t hist[PAR_TILESET_REDUCE_MAX_TILES];
    const uint32_t T = w.head[0];
    if (T == 0) return;
    for (uint32_t b = threadIdx.x; b < T; b += TR_THREADS) hist[b] = 0;
    __syncthreads();
    const uint32_t begin = blockIdx.x * TR_USAGE_CELLS_PER_GROUP;
    const uint32_t end = std::min(n_cells, begin + TR_USAGE_CELLS_PER_GROUP);
    for (uint32_t c = begin + threadIdx.x; c < end; c += TR_THREADS) atomicAdd(&hist[std::min(map[c] & TR_ID_MASK, T - 1)], 1u);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < T; b += TR_THREADS) {
        if (hist[b]) atomicAdd(&w.u[b], hist[b]);
    }
}

// One wavefront a group of TR_TILES_PER_GROUP tiles: the groups are the step kernel's, so that the partials are.
__global__ __launch_bounds__(64) void reduce_start_kernel(Work w, uint32_t budget) {
    const uint32_t T = w.head[0], i = blockIdx.x * TR_TILES_PER_GROUP + threadIdx.x;
    const bool all = T <= budget;
    uint64_t key = 0;
    if (threadIdx.x < TR_TILES_PER_GROUP && i < T) {
        w.d[i] = all ? 0u : 0xFFFFFFFFu;
        w.ag[i] = i;
        w.kept[i] = all ? 1u : 0u;
        if (!all) key = key_of(w.u[i], i);
    }
    key = wave_max(key);
    if (threadIdx.x == 0) w.part[0][blockIdx.x] = key;
}

// Step `step` (0 .. budget - 1) adds the (step + 1)th tile to the kept set. lw and lh are the binary logarithms of the
// tile's width and height, Q the pixels a lane takes of its tile (a tile's pixels over TR_LANES_PER_TILE). The steps are
// a chain of launches, so a step is as long as its chain of dependent loads: everything that does not depend on the new
// centre (the partial maxima, the palette entry, the lane's own pixels, its tile's u, d, a and kept mark) is loaded
// before the centre is known, and only the centre's bytes wait for it. A lane whose tile is at or beyond T reads the
// stored tile min(i, capacity - 1), inside `tiles`, and drops what it computes.
template <uint32_t Q>
__global__ __launch_bounds__(TR_THREADS) void reduce_step_kernel(Work w, const uint8_t* tiles, uint32_t capacity,
                                                                 const uint8_t* palette, uint32_t n_colors, uint32_t step,
                                                                 uint32_t groups, uint32_t lw, uint32_t lh, uint32_t flips) {
    constexpr uint32_t P = Q * TR_LANES_PER_TILE;
    __shared__ uint32_t pal[256];
    __shared__ uint32_t img[4][P];
    __shared__ uint64_t wave_best[TR_THREADS / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t i = blockIdx.x * TR_TILES_PER_GROUP + (t >> 3), j = t & 7u;
    const uint32_t tw = 1u << lw, th = 1u << lh;
    // the new centre: every wavefront takes the maximum for itself (the same words, so the same answer)
    const uint64_t* in = w.part[step & 1u];
    uint64_t best = 0;
    for (uint32_t k = lane; k < groups; k += 64) best = std::max(best, in[k]);
    // ... and what does not wait for it
    const uint32_t T = w.head[0];
    const uint8_t* e = palette + 4u * std::min(t, n_colors - 1u);
    const uint32_t entry = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16);
    const uint8_t* mine = tiles + (size_t)std::min(i, capacity - 1u) * P + j;
    uint8_t own[Q];
#pragma unroll
    for (uint32_t q = 0; q < Q; q++) own[q] = mine[q * TR_LANES_PER_TILE];
    const bool holder = j == 0 && i < capacity;  // (the lane that keeps its tile's state; i < T is checked below)
    uint32_t d = 0, a = 0, kept = 1, u = 0;
    if (holder) {
        d = w.d[i];
        a = w.ag[i] & TR_ID_MASK;
        kept = w.kept[i];
        u = w.u[i];
    }
    best = wave_max(best);
    if (!(best & TR_LIVE)) {  // nothing outside the kept set (T <= K): nor for the next step
        if (t == 0) w.part[(step + 1u) & 1u][blockIdx.x] = 0;
        return;
    }
    // (a live key names a tile below T)
    const uint32_t c = (uint32_t)(PAR_TILESET_REDUCE_MAX_TILES - 1) - (uint32_t)(best & (PAR_TILESET_REDUCE_MAX_TILES - 1));
    const uint8_t* centre = tiles + (size_t)c * P;
    uint8_t image[4] = {0, 0, 0, 0};
    if (t < P) {
        const uint32_t x = t & (tw - 1u), y = t >> lw;
#pragma unroll
        for (uint32_t f = 0; f < 4; f++) {
            if (f & ~flips) continue;
            const uint32_t sx = (f & 1u) ? tw - 1u - x : x, sy = (f & 2u) ? th - 1u - y : y;
            image[f] = centre[(sy << lw) | sx];
        }
    }
    pal[t] = entry;
    __syncthreads();
    if (t < P) {
#pragma unroll
        for (uint32_t f = 0; f < 4; f++) {
            if (!(f & ~flips)) img[f][t] = pal[image[f]];
        }
    }
    __syncthreads();
    // eight lanes a tile, lane j the pixels j, j + 8, ...: D under every allowed image, four bytes a v_sad_u8 (the
    // fourth byte of both colours is 0)
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t q = 0; q < Q; q++) {
        const uint32_t colour = pal[own[q]], p = j + q * TR_LANES_PER_TILE;
#pragma unroll
        for (uint32_t f = 0; f < 4; f++) {
            if (f & ~flips) continue;
            acc[f] = __builtin_amdgcn_sad_u8(colour, img[f][p], acc[f]);
        }
    }
#pragma unroll
    for (uint32_t f = 0; f < 4; f++) {
        for (int s = 1; s < (int)TR_LANES_PER_TILE; s <<= 1) acc[f] += __shfl_xor(acc[f], s);
    }
    uint64_t key = 0;
    if (holder && i < T) {
        uint32_t D = 0xFFFFFFFFu, g = 0;
#pragma unroll
        for (uint32_t f = 0; f < 4; f++) {
            if (!(f & ~flips) && acc[f] < D) {
                D = acc[f];
                g = f;
            }
        }
        if (i == c) {
            kept = 1u;
            w.kept[i] = 1u;
        }
        // the lexicographic minimum of (D, k, f): the centre is new to the set, so c != a, and g is the lowest f of D
        if (D < d || (D == d && c < a)) {
            d = D;
            w.d[i] = D;
            w.ag[i] = c | (g << 30);
        }
        if (!kept) key = key_of((uint64_t)u * (uint64_t)d, i);
    }
    key = wave_max(key);
    if (lane == 0) wave_best[t >> 6] = key;
    __syncthreads();
    if (t == 0) {
        for (uint32_t k = 1; k < TR_THREADS / 64; k++) key = std::max(key, wave_best[k]);
        w.part[(step + 1u) & 1u][blockIdx.x] = key;
    }
}

// One workgroup, TR_TILES_PER_THREAD consecutive tiles a thread: the kept marks scanned into the new numbers, then the
// remap, the count and the error.
__global__ __launch_bounds__(TR_NUMBER_THREADS) void reduce_number_kernel(Work w, uint32_t* remap_out, uint32_t* count_out,
                                                                          uint64_t* error_out) {
    __shared__ uint32_t newn[PAR_TILESET_REDUCE_MAX_TILES];
    __shared__ uint32_t sums[TR_NUMBER_THREADS];
    __shared__ uint64_t errs[TR_NUMBER_THREADS / 64];
    const uint32_t T = w.head[0], t = threadIdx.x, first = t * TR_TILES_PER_THREAD;
    uint32_t kept[TR_TILES_PER_THREAD], mine = 0;
    for (uint32_t k = 0; k < TR_TILES_PER_THREAD; k++) {
        kept[k] = first + k < T ? w.kept[first + k] : 0u;
        mine += kept[k];
    }
    sums[t] = mine;
    __syncthreads();
    for (uint32_t s = 1; s < TR_NUMBER_THREADS; s <<= 1) {
        const uint32_t add = t >= s ? sums[t - s] : 0u;
        __syncthreads();
        sums[t] += add;
        __syncthreads();
    }
    uint32_t n = sums[t] - mine;  // the kept tiles before this thread's
    for (uint32_t k = 0; k < TR_TILES_PER_THREAD; k++) {
        newn[first + k] = n;
        n += kept[k];
    }
    __syncthreads();
    uint64_t err = 0;
    for (uint32_t k = 0; k < TR_TILES_PER_THREAD; k++) {
        const uint32_t i = first + k;
        if (i >= T) break;
        uint32_t r = newn[i];
        if (!kept[k]) {
            const uint32_t ag = w.ag[i];
            r = newn[ag & TR_ID_MASK] | (ag & ~TR_ID_MASK);
            err += (uint64_t)w.u[i] * (uint64_t)w.d[i];
        }
        w.remap[i] = r;
        if (remap_out) remap_out[i] = r;
    }
    for (int s = 32; s; s >>= 1) err += (uint64_t)__shfl_xor((unsigned long long)err, s);
    if ((t & 63u) == 0) errs[t >> 6] = err;
    __syncthreads();
    if (t == 0) {
        for (uint32_t k = 1; k < TR_NUMBER_THREADS / 64; k++) err += errs[k];
        *count_out = sums[TR_NUMBER_THREADS - 1];
        if (error_out) *error_out = err;
    }
}

__global__ __launch_bounds__(TR_THREADS) void reduce_compact_kernel(Work w, const uint8_t* tiles, uint32_t P, uint8_t* tiles_out) {
    const uint32_t T = w.head[0], i = blockIdx.x * TR_TILES_PER_GROUP + (threadIdx.x >> 3), j = threadIdx.x & 7u;
    if (i >= T || !w.kept[i]) return;
    const uint8_t* src = tiles + (size_t)i * P;
    uint8_t* dst = tiles_out + (size_t)w.remap[i] * P;
    for (uint32_t p = j; p < P; p += TR_LANES_PER_TILE) dst[p] = src[p];
}

__global__ __launch_bounds__(TR_THREADS) void reduce_map_kernel(Work w, const uint32_t* map, uint32_t n_cells, uint32_t* map_out) {
    const uint32_t T = w.head[0], c = blockIdx.x * TR_THREADS + threadIdx.x;
    if (c >= n_cells) return;
    const uint32_t m = map[c];
    if (T == 0) {
        map_out[c] = m;
        return;
    }
    const uint32_t r = w.remap[std::min(m & TR_ID_MASK, T - 1u)];
    map_out[c] = (r & TR_ID_MASK) | (((m >> 30) ^ (r >> 30)) << 30);
}

bool tile_dim_ok(int v) { return v == 8 || v == 16; }

// What both forms check of the geometry and the limits (`capacity` is n_tiles through the host form).
bool reduce_args_ok(const uint8_t* tiles, int capacity, int tile_w, int tile_h, int flips, const uint32_t* map, int n_cells,
                    const uint8_t* palette, int n_colors, int budget, const uint8_t* tiles_out, const uint32_t* map_out,
                    const void* count_out) {
    if (!tiles || !map || !palette || !tiles_out || !map_out || !count_out) return false;
    if (capacity < 1 || capacity > PAR_TILESET_REDUCE_MAX_TILES || budget < 1 || budget > PAR_TILESET_REDUCE_MAX_BUDGET) return false;
    if (n_cells < 1 || n_cells > PAR_TILESET_REDUCE_MAX_CELLS || n_colors < 1 || n_colors > 256) return false;
    if (!tile_dim_ok(tile_w) || !tile_dim_ok(tile_h) || flips < 0 || flips > 3) return false;
    const uintptr_t P = (uintptr_t)(tile_w * tile_h);
    const uintptr_t a = reinterpret_cast<uintptr_t>(tiles), b = reinterpret_cast<uintptr_t>(tiles_out);
    return a + (uintptr_t)capacity * P <= b || b + (uintptr_t)budget * P <= a;
}

hipError_t launch_reduce(hipStream_t stream, const uint8_t* tiles, int capacity, const uint32_t* count, int tile_w, int tile_h,
                         int flips, const uint32_t* map, int n_cells, const uint8_t* palette, int n_colors, int budget,
                         void* work_block, uint8_t* tiles_out, uint32_t* map_out, uint32_t* remap_out, uint32_t* count_out,
                         uint64_t* error_out) {
    const Work w = work_of(work_block, (uint32_t)capacity);
    const uint32_t cap = (uint32_t)capacity, cells = (uint32_t)n_cells;
    const uint32_t groups = (cap + TR_TILES_PER_GROUP - 1) / TR_TILES_PER_GROUP;
    const uint32_t lw = tile_w == 8 ? 3u : 4u, lh = tile_h == 8 ? 3u : 4u;
    hipLaunchKernelGGL(reduce_entry_kernel, dim3((cap + TR_THREADS - 1) / TR_THREADS), dim3(TR_THREADS), 0, stream, w, count, cap,
                       (uint32_t)budget);
    hipLaunchKernelGGL(reduce_usage_kernel, dim3((cells + TR_USAGE_CELLS_PER_GROUP - 1) / TR_USAGE_CELLS_PER_GROUP),
                       dim3(TR_THREADS), 0, stream, w, map, cells);
    hipLaunchKernelGGL(reduce_start_kernel, dim3(groups), dim3(64), 0, stream, w, (uint32_t)budget);
    hipError_t e = hipGetLastError();
    const auto step_kernel = lw + lh == 6 ? reduce_step_kernel<8> : (lw + lh == 7 ? reduce_step_kernel<16> : reduce_step_kernel<32>);
    for (uint32_t step = 0; step < (uint32_t)budget && e == hipSuccess; step++) {
        hipLaunchKernelGGL(step_kernel, dim3(groups), dim3(TR_THREADS), 0, stream, w, tiles, cap, palette, (uint32_t)n_colors, step,
                           groups, lw, lh, (uint32_t)flips);
        if ((step & 63u) == 63u) e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(reduce_number_kernel, dim3(1), dim3(TR_NUMBER_THREADS), 0, stream, w, remap_out, count_out, error_out);
    hipLaunchKernelGGL(reduce_compact_kernel, dim3(groups), dim3(TR_THREADS), 0, stream, w, tiles, 1u << (lw + lh), tiles_out);
    hipLaunchKernelGGL(reduce_map_kernel, dim3((cells + TR_THREADS - 1) / TR_THREADS), dim3(TR_THREADS), 0, stream, w, map, cells,
                       map_out);
    return hipGetLastError();
}

}  // namespace

extern "C" {

size_t par_tileset_reduce_work_bytes(int n_cells, int capacity) {
    if (n_cells < 1 || n_cells > PAR_TILESET_REDUCE_MAX_CELLS || capacity < 1 || capacity > PAR_TILESET_REDUCE_MAX_TILES) return 0;
    return TR_HEAD_BYTES + (size_t)(4 * TR_WORDS_PER_TILE) * (size_t)capacity;
}

int par_tileset_reduce_device(void* stream, const uint8_t* tiles, int capacity, const uint32_t* count, int tile_w,
                              int tile_h, int flips, const uint32_t* map, int n_cells, const uint8_t* palette,
                              int n_colors, int budget, void* work, uint8_t* tiles_out, uint32_t* map_out,
                              uint32_t* remap_out, uint32_t* count_out, uint64_t* error_out) {
    if (!reduce_args_ok(tiles, capacity, tile_w, tile_h, flips, map, n_cells, palette, n_colors, budget, tiles_out, map_out,
                        count_out) ||
        !count || !work || (reinterpret_cast<uintptr_t>(work) & 7u) != 0) {
        return PAR_ERR_INVALID_ARG;
    }
    return launch_reduce((hipStream_t)stream, tiles, capacity, count, tile_w, tile_h, flips, map, n_cells, palette, n_colors,
                         budget, work, tiles_out, map_out, remap_out, count_out, error_out) == hipSuccess
               ? PAR_OK
               : PAR_ERR_HIP;
}

int par_tileset_reduce_host(int device, const uint8_t* tiles, int n_tiles, int tile_w, int tile_h, int flips,
                            const uint32_t* map, int n_cells, const uint8_t* palette, int n_colors, int budget,
                            uint8_t* tiles_out, uint32_t* map_out, uint32_t* remap_out, int* count_out,
                            uint64_t* error_out) {
    if (!reduce_args_ok(tiles, n_tiles, tile_w, tile_h, flips, map, n_cells, palette, n_colors, budget, tiles_out, map_out,
                        count_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    const size_t tile_bytes = (size_t)(tile_w * tile_h);
    const uint32_t t_in = (uint32_t)n_tiles, kept = (uint32_t)std::min(n_tiles, budget);
    uint32_t t_out = 0;
    par_device_buffer d_tiles(e, tiles, (size_t)n_tiles * tile_bytes, true);
    par_device_buffer d_count(e, &t_in, sizeof(t_in), true);
    par_device_buffer d_map(e, map, (size_t)n_cells * sizeof(uint32_t), true);
    par_device_buffer d_palette(e, palette, (size_t)n_colors * 4, true);
    par_device_buffer d_work(e, &t_in, par_tileset_reduce_work_bytes(n_cells, n_tiles), false);  // (device memory only)
    par_device_buffer d_tiles_out(e, tiles_out, (size_t)kept * tile_bytes, false);  // (T is known here: min(T, K) tiles)
    par_device_buffer d_map_out(e, map_out, (size_t)n_cells * sizeof(uint32_t), false);
    par_device_buffer d_remap(e, remap_out, (size_t)n_tiles * sizeof(uint32_t), false);
    par_device_buffer d_count_out(e, &t_out, sizeof(t_out), false);
    par_device_buffer d_error(e, error_out, sizeof(uint64_t), false);
    if (e == hipSuccess) {
        e = launch_reduce(nullptr, d_tiles.as<uint8_t>(), n_tiles, d_count.as<uint32_t>(), tile_w, tile_h, flips,
                          d_map.as<uint32_t>(), n_cells, d_palette.as<uint8_t>(), n_colors, budget, d_work.as<void>(),
                          d_tiles_out.as<uint8_t>(), d_map_out.as<uint32_t>(), d_remap.as<uint32_t>(),
                          d_count_out.as<uint32_t>(), d_error.as<uint64_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    d_tiles_out.download(tiles_out);
    d_map_out.download(map_out);
    if (remap_out) d_remap.download(remap_out);
    d_count_out.download(&t_out);
    if (error_out) d_error.download(error_out);
    if (e == hipSuccess) *count_out = (int)t_out;
    return par_status_of(e);
}

}  // extern "C"
