// par_delta.hip — changed tiles: which bin-sized tiles of a finished `fb` plane differ from the previous frame's
// (par_tiles_changed_device), those tiles packed by a count that stays on the device (par_tiles_pack_counted), and the
// one call that waits and copies them to the host (par_tiles_fetch). The contract is beside the declarations in
// par_raytracer.h; par_tiles_apply_host, the host arithmetic that ends the chain, is in par_scene.cpp. Nothing here
// knows a par_context, and the render kernels (par_kernels.hip) know nothing of this.
//
// Ordering is by kernel boundaries alone: no flag is polled, no workgroup waits for another, and no global atomic is
// used, so nothing a workgroup's arrival order could change reaches the result.
//   1. tiles_flag_kernel: a workgroup owns T whole, consecutive tiles of one bin row. Its 256 threads are laid out as
//      `rw` pieces along the row (a piece is 4 pixels = 16 bytes in the wide form, one pixel otherwise) by 256 / rw row
//      lanes; a thread keeps its piece column, hence its tile, and ORs a ^ b down the tile's rows, four rows' loads of
//      both planes issued before the first use. A thread that saw a difference stores 1 to its tile's word in LDS
//      (every such store writes the same value); after the barrier the tile's 0 / 1 goes to d_map with one plain store.
//      Every tile of the block's bin rows is written exactly once, by the one workgroup that owns it.
//   2. tiles_rank_kernel: ONE workgroup turns the flags into ranks in place, RANK_ITEMS entries a round: ballots give a
//      wave's count and a lane's place in it, the waves' counts meet in LDS, and the running base is carried in a
//      register. Entries of bin rows outside the block are not read (the first launch did not write them) and become
//      -1. The list and the count are written here.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "par_internal.h"
#include "par_raytracer.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int DELTA_THREADS = 256;
constexpr int FLAG_ROWS_IN_FLIGHT = 4;
constexpr int RANK_THREADS = 1024;
constexpr int RANK_WAVES = RANK_THREADS / 64;
constexpr int RANK_SUB = 4;  // entries per thread and round, RANK_THREADS apart (coalesced)
constexpr int RANK_ITEMS = RANK_THREADS * RANK_SUB;
static_assert(RANK_WAVES * RANK_SUB == 64, "one wave scans the round's wave counts, one per lane");

// How 256 threads lie over the tiles a workgroup owns (flag kernel) or over one slot (counted pack): `rw` pieces along
// a row, `rs` rows side by side. The threads from rw * rs on idle.
struct delta_shape {
    int tiles;  // tiles of a bin row per workgroup (flag kernel only)
    int rw, rs;
};

delta_shape flag_shape(int B, bool vec) {
    const int per_piece = vec ? 4 : 1;
    delta_shape s;
    s.tiles = (vec ? 64 : DELTA_THREADS) * per_piece / B;  // the wide form keeps a row of pieces within one wave
    if (s.tiles < 1) s.tiles = 1;
    s.rw = s.tiles * B / per_piece;
    s.rs = DELTA_THREADS / s.rw;
    return s;
}

template <bool VEC>
__global__ __launch_bounds__(DELTA_THREADS) void tiles_flag_kernel(const uint32_t* __restrict__ a,
                                                                    const uint32_t* __restrict__ b, int W, int H, int B,
                                                                    int gx, int row_begin, int row_end, int by_lo, int tiles,
                                                                    int rw, int rs, int32_t* __restrict__ map) {
    __shared__ uint32_t changed[DELTA_THREADS];
    const int t = (int)threadIdx.x;
    const int by = by_lo + (int)blockIdx.y, bx0 = (int)blockIdx.x * tiles;
    const int n_tiles = min(tiles, gx - bx0);
    changed[t] = 0u;
    __syncthreads();
    const int ty = t / rw, tx = t - ty * rw;
    const int px = tx * (VEC ? 4 : 1);                    // pixel column within the workgroup's tiles
    const int x = bx0 * B + px;                           // and in the view
    const int rows_lo = max(by * B, row_begin), rows_hi = min(min(by * B + B, H), row_end);
    if (ty < rs && x < W && rows_lo + ty < rows_hi) {
        uint32_t acc = 0u;
        for (int y = rows_lo + ty; y < rows_hi; y += FLAG_ROWS_IN_FLIGHT * rs) {
            // a row beyond the tile's last is replaced by row y, which is in range: its difference is ORed in twice
            size_t at[FLAG_ROWS_IN_FLIGHT];
            for (int k = 0; k < FLAG_ROWS_IN_FLIGHT; k++) {
                const int yk = y + k * rs < rows_hi ? y + k * rs : y;
                at[k] = (size_t)(yk - row_begin) * (size_t)W + (size_t)x;
            }
            if (VEC) {
                u32x4 va[FLAG_ROWS_IN_FLIGHT], vb[FLAG_ROWS_IN_FLIGHT];
                for (int k = 0; k < FLAG_ROWS_IN_FLIGHT; k++) {
                    va[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a + at[k]));
                    vb[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(b + at[k]));
                }
                for (int k = 0; k < FLAG_ROWS_IN_FLIGHT; k++) {
                    const u32x4 d = va[k] ^ vb[k];
                    acc |= d[0] | d[1] | d[2] | d[3];
                }
            } else {
                uint32_t va[FLAG_ROWS_IN_FLIGHT], vb[FLAG_ROWS_IN_FLIGHT];
                for (int k = 0; k < FLAG_ROWS_IN_FLIGHT; k++) {
                    va[k] = a[at[k]];
                    vb[k] = b[at[k]];
                }
                for (int k = 0; k < FLAG_ROWS_IN_FLIGHT; k++) acc |= va[k] ^ vb[k];
            }
        }
        if (acc != 0u) changed[px / B] = 1u;
    }
    __syncthreads();
    if (t < n_tiles) map[(size_t)by * (size_t)gx + (size_t)(bx0 + t)] = (int32_t)changed[t];
}

// map[i]: 0 / 1 for the tiles of bin rows [by_lo, by_hi], anything elsewhere -> rank or -1 everywhere.
__global__ __launch_bounds__(RANK_THREADS) void tiles_rank_kernel(int32_t* map, int gx, int n, int by_lo, int by_hi,
                                                                  int32_t* __restrict__ tiles, int capacity,
                                                                  int32_t* __restrict__ count) {
    __shared__ int wave_count[2][64];  // [round parity][sub * RANK_WAVES + wave]
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int lo = by_lo * gx, hi = (by_hi + 1) * gx;  // entries the flag launch wrote
    int base = 0;
    for (int start = 0, round = 0; start < n; start += RANK_ITEMS, round++) {
        int flag[RANK_SUB];
        for (int j = 0; j < RANK_SUB; j++) {
            const int i = start + j * RANK_THREADS + t;
            flag[j] = (i < n && i >= lo && i < hi) ? map[i] : 0;
        }
        int below[RANK_SUB];
        int* counts = wave_count[round & 1];
        for (int j = 0; j < RANK_SUB; j++) {
            const unsigned long long m = __ballot(flag[j] != 0);
            below[j] = __popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) counts[j * RANK_WAVES + wave] = __popcll(m);
        }
        // one barrier a round: the other parity's counts are overwritten only after every thread has passed this
        // barrier, which it reaches after its reads of the round before
        __syncthreads();
        // every wave scans the 64 counts of the round, one per lane
        const int own = counts[lane];
        int incl = own;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const int excl = incl - own;
        for (int j = 0; j < RANK_SUB; j++) {
            const int i = start + j * RANK_THREADS + t;
            const int rank = base + __shfl(excl, j * RANK_WAVES + wave) + below[j];
            if (i < n) {
                map[i] = flag[j] != 0 ? rank : -1;
                if (flag[j] != 0 && rank < capacity) {
                    const int by = i / gx;
                    tiles[rank] = (i - by * gx) | (by << 16);
                }
            }
        }
        base += __shfl(incl, 63);
    }
    if (t == 0) count[0] = base;
}

// The counted pack: one workgroup per slot of `capacity`; those from min(max(count, 0), capacity) on leave after one
// (wave-uniform) load of the count. A slot's row is B pixels in the frame and in the slot; PIECE pixels per thread.
template <bool VEC>
__global__ __launch_bounds__(DELTA_THREADS) void tiles_pack_counted_kernel(const int32_t* __restrict__ tiles,
                                                                            const int32_t* __restrict__ count, int capacity,
                                                                            int W, int H, int B, int gx, int gy,
                                                                            int row_begin, int row_end, int rw, int rs,
                                                                            const uint32_t* __restrict__ src,
                                                                            uint32_t* __restrict__ dst) {
    const int slot = (int)blockIdx.x;
    const int m = min(max(count[0], 0), capacity);
    if (slot >= m) return;
    const int tile = tiles[slot];
    const int bx = tile & 0xFFFF, by = tile >> 16;
    if (bx >= gx || by < 0 || by >= gy) return;
    const int t = (int)threadIdx.x;
    const int ty = t / rw, tx = t - ty * rw;
    const int px = tx * (VEC ? 4 : 1);
    const int c0 = bx * B, r0 = by * B;
    if (ty >= rs || c0 + px >= W) return;
    const int rows_lo = max(r0, row_begin), rows_hi = min(min(r0 + B, H), row_end);
    for (int row = r0 + ty; row < rows_hi; row += rs) {
        if (row < rows_lo) continue;
        const size_t in_frame = (size_t)(row - row_begin) * (size_t)W + (size_t)(c0 + px);
        const size_t in_slot = (size_t)slot * (size_t)(B * B) + (size_t)((row - r0) * B + px);
        if (VEC) *reinterpret_cast<u32x4*>(dst + in_slot) = *reinterpret_cast<const u32x4*>(src + in_frame);
        else dst[in_slot] = src[in_frame];
    }
}

bool params_ok(const par_params* p) {
    return p && p->width > 0 && p->height > 0 && p->bin_size >= PAR_MIN_BIN && p->bin_size <= PAR_MAX_BIN;
}

bool on_16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int status_of(hipError_t e) {
    if (e == hipSuccess) return PAR_OK;
    return e == hipErrorNoDevice || e == hipErrorInvalidDevice ? PAR_ERR_NO_DEVICE : PAR_ERR_HIP;
}

}  // namespace

extern "C" {

int par_tiles_changed_device(const par_params* params, void* stream, const par_color* a, const par_color* b,
                             int row_begin, int row_end, int32_t* d_map, int32_t* d_tiles, int capacity,
                             int32_t* d_count) {
    if (!params_ok(params) || !a || !b || !d_map || !d_count || capacity < 0 || (capacity > 0 && !d_tiles) ||
        row_begin < 0 || row_begin >= row_end || row_end > params->height) {
        return PAR_ERR_INVALID_ARG;
    }
    const int W = params->width, H = params->height, B = params->bin_size;
    const int gx = (W + B - 1) / B, gy = (H + B - 1) / B;
    if (gx > PAR_MAX_GRID_DIM || gy > PAR_MAX_GRID_DIM) return PAR_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    int by_lo = row_begin / B, by_hi = (row_end - 1) / B;
    if (a == b) {
        by_hi = by_lo - 1;  // nothing can differ: no tile is looked at, the rank launch writes -1 and 0
    } else {
        const bool vec = W % 4 == 0 && B % 4 == 0 && on_16(a) && on_16(b);
        const delta_shape f = flag_shape(B, vec);
        const dim3 grid((unsigned)((gx + f.tiles - 1) / f.tiles), (unsigned)(by_hi - by_lo + 1));
        const uint32_t* pa = reinterpret_cast<const uint32_t*>(a);
        const uint32_t* pb = reinterpret_cast<const uint32_t*>(b);
        if (vec) {
            hipLaunchKernelGGL(tiles_flag_kernel<true>, grid, dim3(DELTA_THREADS), 0, s, pa, pb, W, H, B, gx, row_begin,
                               row_end, by_lo, f.tiles, f.rw, f.rs, d_map);
        } else {
            hipLaunchKernelGGL(tiles_flag_kernel<false>, grid, dim3(DELTA_THREADS), 0, s, pa, pb, W, H, B, gx, row_begin,
                               row_end, by_lo, f.tiles, f.rw, f.rs, d_map);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return status_of(e);
    }
    hipLaunchKernelGGL(tiles_rank_kernel, dim3(1), dim3(RANK_THREADS), 0, s, d_map, gx, gx * gy, by_lo, by_hi, d_tiles,
                       capacity, d_count);
    return status_of(hipGetLastError());
}

int par_tiles_pack_counted(const par_params* params, void* stream, const int32_t* d_tiles, const int32_t* d_count,
                           int capacity, const par_color* fb_block, int row_begin, int row_end, par_color* packed) {
    if (!params_ok(params) || capacity < 0 || !d_count || (capacity > 0 && (!d_tiles || !fb_block || !packed)) ||
        row_begin < 0 || row_end > params->height || row_begin > row_end) {
        return PAR_ERR_INVALID_ARG;
    }
    if (capacity == 0) return PAR_OK;
    const int W = params->width, H = params->height, B = params->bin_size;
    const int gx = (W + B - 1) / B, gy = (H + B - 1) / B;
    const bool vec = W % 4 == 0 && B % 4 == 0 && on_16(fb_block) && on_16(packed);
    const int rw = vec ? B / 4 : B, rs = DELTA_THREADS / rw;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(fb_block);
    uint32_t* dst = reinterpret_cast<uint32_t*>(packed);
    if (vec) {
        hipLaunchKernelGGL(tiles_pack_counted_kernel<true>, dim3((unsigned)capacity), dim3(DELTA_THREADS), 0,
                           (hipStream_t)stream, d_tiles, d_count, capacity, W, H, B, gx, gy, row_begin, row_end, rw, rs, src,
                           dst);
    } else {
        hipLaunchKernelGGL(tiles_pack_counted_kernel<false>, dim3((unsigned)capacity), dim3(DELTA_THREADS), 0,
                           (hipStream_t)stream, d_tiles, d_count, capacity, W, H, B, gx, gy, row_begin, row_end, rw, rs, src,
                           dst);
    }
    return status_of(hipGetLastError());
}

int par_tiles_fetch(const par_params* params, void* stream, const int32_t* d_count, const int32_t* d_tiles,
                    const par_color* d_packed, int capacity, int32_t* tiles, par_color* packed, int* n, int* count) {
    if (!params_ok(params) || capacity < 0 || !d_count || !d_tiles || !d_packed || !tiles || !packed || !n || !count) {
        return PAR_ERR_INVALID_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PAR_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    int32_t total = 0;
    hipError_t e = hipMemcpyAsync(&total, d_count, sizeof(total), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return status_of(e);
    *count = total;
    *n = 0;
    if (total <= 0 || total > capacity) return PAR_OK;
    const size_t slot = (size_t)params->bin_size * (size_t)params->bin_size * sizeof(par_color);
    e = hipMemcpyAsync(tiles, d_tiles, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(packed, d_packed, (size_t)total * slot, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return status_of(e);
    *n = total;
    return PAR_OK;
}

}  // extern "C"
