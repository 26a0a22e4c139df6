// par_delta.hip — the tile calls on the device: bin-sized tiles of a finished plane packed into slots, unpacked and
// assembled (sharded frames), and changed tiles: which tiles of a plane differ from the previous frame's, those tiles
// packed by a count that stays on the device, and the one call that waits and copies them to the host. One set of
// kernels serves both families of entry points: par_plane_tiles_* over planes of 1-, 4- and 28-byte elements (palidx /
// lit / index / edge planes, fb / brightness, the G-buffer) and par_tiles_* over `fb` planes, which are the same calls
// at 4 bytes. The contracts are beside the declarations in par_raytracer.h; the host arithmetic that ends the chain
// (par_plane_tiles_apply_host, par_tiles_apply_host) is in par_scene.cpp. Nothing here knows a par_context, and the
// render kernels (par_kernels.hip) know nothing of this.
//
// The kernels work in bytes and are described where they stand. Changed tiles are two launches, ordered by the kernel
// boundary alone: no flag is polled, no workgroup waits for another, and no global atomic is used, so nothing a
// workgroup's arrival order could change reaches the result.
//   1. plane_flag_kernel: a workgroup owns whole, consecutive tiles of one bin row. Its 256 threads are laid out as `rw`
//      access units along the row by 256 / rw row lanes; a thread keeps its unit column, hence its tile, and ORs a ^ b
//      down the tile's rows, four rows' loads of both planes issued before the first use. A thread that saw a difference
//      stores 1 to its tile's word in LDS (every such store writes the same value); after the barrier the tile's 0 / 1
//      goes to d_map with one plain store. Every tile of the block's bin rows is written exactly once, by the one
//      workgroup that owns it.
//   2. tiles_rank_kernel: ONE workgroup turns the flags into ranks in place, RANK_ITEMS entries a round: ballots give a
//      wave's count and a lane's place in it, the waves' counts meet in LDS, and the running base is carried in a
//      register. Entries of bin rows outside the block are not read (the first launch did not write them) and become
//      -1. The list and the count are written here. It knows no element size.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <type_traits>

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

// How 256 threads lie over the tiles a workgroup owns (flag kernel) or over one slot (pack and unpack): `rw` units along
// a row, `rs` rows side by side. The threads from rw * rs on idle.
struct delta_shape {
    int tiles;  // tiles of a bin row per workgroup (flag kernel only)
    int rw, rs;
};

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

// ---- the kernels that touch planes, over elements of 1, 4 and 28 bytes ----------------------------------------------
// Everything is in bytes: a plane row is RB = W * E bytes, a tile's row is B * E bytes, and a kernel moves access units
// of U bytes, U in {16, 8, 4, 1}. The host picks the largest U that divides RB and B * E and the address of every plane
// and slot buffer involved (plane_unit), so a unit is aligned, lies inside one row and inside ONE tile; `upt` is the
// units of a tile's row. The element size enters nowhere else, except where assemble lays the fill element out.

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <int U> struct unit_of;
template <> struct unit_of<16> { typedef u32x4 type; };
template <> struct unit_of<8> { typedef u32x2 type; };
template <> struct unit_of<4> { typedef uint32_t type; };
template <> struct unit_of<1> { typedef uint8_t type; };

__device__ inline uint32_t unit_diff(u32x4 a, u32x4 b) {
    const u32x4 d = a ^ b;
    return d[0] | d[1] | d[2] | d[3];
}
__device__ inline uint32_t unit_diff(u32x2 a, u32x2 b) {
    const u32x2 d = a ^ b;
    return d[0] | d[1];
}
__device__ inline uint32_t unit_diff(uint32_t a, uint32_t b) { return a ^ b; }
__device__ inline uint32_t unit_diff(uint8_t a, uint8_t b) { return (uint32_t)(a ^ b); }

// The wide units stream past the caches; dwords and bytes are plain accesses.
template <int U>
__device__ inline typename unit_of<U>::type unit_load(const uint8_t* p) {
    typedef typename unit_of<U>::type unit;
    if constexpr (U >= 8) return __builtin_nontemporal_load(reinterpret_cast<const unit*>(p));
    else return *reinterpret_cast<const unit*>(p);
}

// Which tiles differ, pass 1. A workgroup owns `tiles` whole, consecutive tiles of one bin row: `rw` units along the
// row by `rs` row lanes. Where the tiles' row holds more than 256 units (28-byte elements in large bins) the workgroup
// owns one tile and a thread walks the row in steps of rw. Four rows of both planes are in flight before the first use.
template <int U>
__global__ __launch_bounds__(DELTA_THREADS) void plane_flag_kernel(const uint8_t* __restrict__ a,
                                                                    const uint8_t* __restrict__ b, size_t RB, int H, int B,
                                                                    int upt, int gx, int row_begin, int row_end, int by_lo,
                                                                    int tiles, int rw, int rs, int32_t* __restrict__ map) {
    typedef typename unit_of<U>::type unit;
    __shared__ uint32_t changed[DELTA_THREADS];
    const int t = (int)threadIdx.x;
    const int by = by_lo + (int)blockIdx.y, bx0 = (int)blockIdx.x * tiles;
    const int n_tiles = min(tiles, gx - bx0);
    changed[t] = 0u;
    __syncthreads();
    const int ty = t / rw, tx = t - ty * rw;
    const int rows_lo = max(by * B, row_begin), rows_hi = min(min(by * B + B, H), row_end);
    if (ty < rs && rows_lo + ty < rows_hi) {
        for (int c = tx; c < n_tiles * upt; c += rw) {  // unit within the workgroup's tiles
            const size_t xb = ((size_t)bx0 * (size_t)upt + (size_t)c) * U;  // its first byte within a plane row
            if (xb >= RB) break;                                             // (RB % U == 0: a unit is in the row or not)
            uint32_t acc = 0u;
            for (int y = rows_lo + ty; y < rows_hi; y += FLAG_ROWS_IN_FLIGHT * rs) {
                // a row beyond the tile's last is replaced by row y, which is in range: its difference is ORed in twice
                size_t at[FLAG_ROWS_IN_FLIGHT];
                for (int k = 0; k < FLAG_ROWS_IN_FLIGHT; k++) {
                    const int yk = y + k * rs < rows_hi ? y + k * rs : y;
                    at[k] = (size_t)(yk - row_begin) * RB + xb;
                }
                unit va[FLAG_ROWS_IN_FLIGHT], vb[FLAG_ROWS_IN_FLIGHT];
                for (int k = 0; k < FLAG_ROWS_IN_FLIGHT; k++) {
                    va[k] = unit_load<U>(a + at[k]);
                    vb[k] = unit_load<U>(b + at[k]);
                }
                for (int k = 0; k < FLAG_ROWS_IN_FLIGHT; k++) acc |= unit_diff(va[k], vb[k]);
            }
            if (acc != 0u) changed[c / upt] = 1u;
        }
    }
    __syncthreads();
    if (t < n_tiles) map[(size_t)by * (size_t)gx + (size_t)(bx0 + t)] = (int32_t)changed[t];
}

// Pack (frame block -> slots) and unpack (slots -> frame block): one workgroup per list entry, `rw` units along the
// tile's row by `rs` rows. With a `count` the entries from min(max(count[0], 0), capacity) on leave after one
// (wave-uniform) load of it; without one every entry of `capacity` is taken. An entry outside the grid is skipped.
template <int U, bool PACK>
__global__ __launch_bounds__(DELTA_THREADS) void plane_copy_kernel(const int32_t* __restrict__ tiles,
                                                                    const int32_t* __restrict__ count, int capacity,
                                                                    size_t RB, int H, int B, int upt, int gx, int gy,
                                                                    int row_begin, int row_end, int rw, int rs,
                                                                    const uint8_t* __restrict__ src,
                                                                    uint8_t* __restrict__ dst) {
    typedef typename unit_of<U>::type unit;
    const int slot = (int)blockIdx.x;
    const int m = count ? min(max(count[0], 0), capacity) : capacity;
    if (slot >= m) return;
    const int tile = tiles[slot];
    const int bx = tile & 0xFFFF, by = tile >> 16;
    if (bx >= gx || by < 0 || by >= gy) return;
    const int t = (int)threadIdx.x;
    const int ty = t / rw, tx = t - ty * rw;
    if (ty >= rs) return;
    const int r0 = by * B;
    const int rows_lo = max(r0, row_begin), rows_hi = min(min(r0 + B, H), row_end);
    const size_t c0 = (size_t)bx * (size_t)upt * U;                      // the tile's first byte within a plane row
    const size_t slot_at = (size_t)slot * (size_t)B * (size_t)upt * U;   // the slot's first byte: B rows of upt units
    for (int row = rows_lo + ty; row < rows_hi; row += rs) {
        for (int c = tx; c < upt; c += rw) {
            const size_t xb = c0 + (size_t)c * U;
            if (xb >= RB) break;
            const size_t in_frame = (size_t)(row - row_begin) * RB + xb;
            const size_t in_slot = slot_at + ((size_t)(row - r0) * (size_t)upt + (size_t)c) * U;
            if (PACK) *reinterpret_cast<unit*>(dst + in_slot) = *reinterpret_cast<const unit*>(src + in_frame);
            else *reinterpret_cast<unit*>(dst + in_frame) = *reinterpret_cast<const unit*>(src + in_slot);
        }
    }
}

// The element that goes where no tile does, by value: seven words hold a 28-byte element; the host repeats a 1- or
// 4-byte element through all of them, so that the units of those sizes need no phase.
struct plane_fill {
    uint32_t w[7];
};

__device__ inline uint32_t fill_word(const plane_fill& f, int i) {  // (selects: no indexed read of a kernel argument)
    uint32_t v = f.w[0];
    for (int k = 1; k < 7; k++) v = i == k ? f.w[k] : v;
    return v;
}

// The unit of the fill that starts at byte `xb` of a plane row of E-byte elements (every row starts a new element).
template <int U>
__device__ inline typename unit_of<U>::type fill_unit(const plane_fill& f, int E, size_t xb) {
    if constexpr (U == 1) {
        const int k = (int)(xb % (size_t)E);
        return (uint8_t)(fill_word(f, k >> 2) >> (8 * (k & 3)));
    } else {
        const int d0 = E == 28 ? (int)((xb >> 2) % 7u) : 0;
        uint32_t w[U / 4];
        for (int j = 0; j < U / 4; j++) w[j] = fill_word(f, E == 28 ? (d0 + j) % 7 : 0);
        if constexpr (U == 4) return w[0];
        else if constexpr (U == 8) return u32x2{w[0], w[1]};
        else return u32x4{w[0], w[1], w[2], w[3]};
    }
}

// Assemble: rows [row_begin, row_end) of `frame` in one pass, each written exactly once, a thread keeping its unit column
// (hence its tile column, its place in the tile's row and its unit of the fill) and streaming down the rows; the bin row
// of a row through the reciprocal `magic_b` (0: the rows are too many for it to be exact, divide).
template <int U>
__global__ __launch_bounds__(DELTA_THREADS) void plane_assemble_kernel(const int32_t* __restrict__ map, int gx, size_t RB,
                                                                        int B, int upt, int E, int row_begin, int row_end,
                                                                        const uint8_t* __restrict__ packed,
                                                                        uint8_t* __restrict__ frame, plane_fill fill,
                                                                        uint32_t magic_b) {
    typedef typename unit_of<U>::type unit;
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;  // unit within a plane row
    const size_t xb = (size_t)q * U;
    if (xb >= RB) return;
    const int bx = (int)(q / (uint32_t)upt), cin = (int)(q - (uint32_t)bx * (uint32_t)upt);
    const unit fv = fill_unit<U>(fill, E, xb);
    const size_t slot_bytes = (size_t)B * (size_t)upt * U;
#pragma unroll 4
    for (int y = row_begin + (int)blockIdx.y; y < row_end; y += (int)gridDim.y) {
        const int by = magic_b ? (int)__umulhi((uint32_t)y, magic_b) : y / B;
        const int slot = map[(size_t)by * (size_t)gx + (size_t)bx];
        unit v = fv;
        if (slot >= 0) {
            v = unit_load<U>(packed + (size_t)slot * slot_bytes + ((size_t)(y - by * B) * (size_t)upt + (size_t)cin) * U);
        }
        unit* at = reinterpret_cast<unit*>(frame + (size_t)y * RB + xb);
        if constexpr (U >= 8) __builtin_nontemporal_store(v, at);
        else *at = v;
    }
}

// The largest unit that divides a plane row, a tile row and every address involved.
int plane_unit(int W, int B, int E, const void* p0, const void* p1) {
    const uintptr_t bits = (uintptr_t)((size_t)W * (size_t)E) | (uintptr_t)(B * E) | reinterpret_cast<uintptr_t>(p0) |
                           reinterpret_cast<uintptr_t>(p1);
    return bits % 16 == 0 ? 16 : bits % 8 == 0 ? 8 : bits % 4 == 0 ? 4 : 1;
}

// f(std::integral_constant<int, u>) for the unit picked at run time.
template <class F>
void with_unit(int u, F&& f) {
    if (u == 16) f(std::integral_constant<int, 16>());
    else if (u == 8) f(std::integral_constant<int, 8>());
    else if (u == 4) f(std::integral_constant<int, 4>());
    else f(std::integral_constant<int, 1>());
}

// `lanes` units of a row per workgroup where whole tiles fit in them, else one tile.
delta_shape plane_shape(int upt, int lanes) {
    delta_shape s;
    s.tiles = lanes / upt < 1 ? 1 : lanes / upt;
    s.rw = s.tiles * upt < DELTA_THREADS ? s.tiles * upt : DELTA_THREADS;
    s.rs = DELTA_THREADS / s.rw;
    return s;
}

bool elem_ok(int e) { return e == 1 || e == 4 || e == 28; }

bool params_ok(const par_params* p) {
    return p && p->width > 0 && p->height > 0 && p->bin_size >= PAR_MIN_BIN && p->bin_size <= PAR_MAX_BIN;
}

int status_of(hipError_t e) {
    if (e == hipSuccess) return PAR_OK;
    return e == hipErrorNoDevice || e == hipErrorInvalidDevice ? PAR_ERR_NO_DEVICE : PAR_ERR_HIP;
}

// par_tiles_pack, par_tiles_unpack and par_tiles_assemble report every HIP failure, a missing device included, as
// PAR_ERR_HIP.
int hip_only(int rc) { return rc == PAR_ERR_NO_DEVICE ? PAR_ERR_HIP : rc; }

// ---- the six operations, once each: the argument checks both families share, then the launch; E is the element size --

int plane_changed(const par_params* p, hipStream_t s, int E, const void* a, const void* b, int row_begin, int row_end,
                  int32_t* d_map, int32_t* d_tiles, int capacity, int32_t* d_count) {
    if (!params_ok(p) || !elem_ok(E) || !a || !b || !d_map || !d_count || capacity < 0 || (capacity > 0 && !d_tiles) ||
        row_begin < 0 || row_begin >= row_end || row_end > p->height) {
        return PAR_ERR_INVALID_ARG;
    }
    const int W = p->width, H = p->height, B = p->bin_size;
    const int gx = (W + B - 1) / B, gy = (H + B - 1) / B;
    if (gx > PAR_MAX_GRID_DIM || gy > PAR_MAX_GRID_DIM) return PAR_ERR_UNSUPPORTED;
    int by_lo = row_begin / B, by_hi = (row_end - 1) / B;
    if (a == b) {
        by_hi = by_lo - 1;  // nothing can differ: no tile is looked at, the rank launch writes -1 and 0
    } else {
        const int u = plane_unit(W, B, E, a, b);
        const int upt = B * E / u;
        const delta_shape f = plane_shape(upt, u >= 8 ? 64 : DELTA_THREADS);  // wide units: a row of them within one wave
        const dim3 grid((unsigned)((gx + f.tiles - 1) / f.tiles), (unsigned)(by_hi - by_lo + 1));
        with_unit(u, [&](auto U) {
            hipLaunchKernelGGL(plane_flag_kernel<U()>, grid, dim3(DELTA_THREADS), 0, s, static_cast<const uint8_t*>(a),
                               static_cast<const uint8_t*>(b), (size_t)W * (size_t)E, H, B, upt, gx, row_begin, row_end, by_lo,
                               f.tiles, f.rw, f.rs, d_map);
        });
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return status_of(e);
    }
    hipLaunchKernelGGL(tiles_rank_kernel, dim3(1), dim3(RANK_THREADS), 0, s, d_map, gx, gx * gy, by_lo, by_hi, d_tiles,
                       capacity, d_count);
    return status_of(hipGetLastError());
}

// Pack, counted pack and unpack: `n` list entries (by the device's count where `d_count` is given, `n` then being the
// capacity) with the unit the operands allow. An unpack is over the rows [0, height).
int plane_copy(bool pack, const par_params* p, hipStream_t s, int E, const int32_t* d_tiles, const int32_t* d_count, int n,
               int row_begin, int row_end, const void* src, void* dst) {
    if (!params_ok(p) || !elem_ok(E) || n < 0 || (n > 0 && (!d_tiles || !src || !dst)) || row_begin < 0 ||
        row_end > p->height || row_begin > row_end) {
        return PAR_ERR_INVALID_ARG;
    }
    if (n == 0) return PAR_OK;
    const int W = p->width, H = p->height, B = p->bin_size;
    const int gx = (W + B - 1) / B, gy = (H + B - 1) / B;
    const int u = plane_unit(W, B, E, src, dst);
    const int upt = B * E / u;
    const delta_shape f = plane_shape(upt, 1);  // one tile a workgroup
    with_unit(u, [&](auto U) {
        if (pack) {
            hipLaunchKernelGGL((plane_copy_kernel<U(), true>), dim3((unsigned)n), dim3(DELTA_THREADS), 0, s, d_tiles, d_count,
                               n, (size_t)W * (size_t)E, H, B, upt, gx, gy, row_begin, row_end, f.rw, f.rs,
                               static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dst));
        } else {
            hipLaunchKernelGGL((plane_copy_kernel<U(), false>), dim3((unsigned)n), dim3(DELTA_THREADS), 0, s, d_tiles, d_count,
                               n, (size_t)W * (size_t)E, H, B, upt, gx, gy, row_begin, row_end, f.rw, f.rs,
                               static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dst));
        }
    });
    return status_of(hipGetLastError());
}

// `fill`: E bytes on the host. The bin size is checked as par_grid_dims checks it (> 0), not against [8, 160].
int plane_assemble(const par_params* p, hipStream_t s, int E, const int32_t* d_map, const void* packed, const void* fill,
                   void* frame, int row_begin, int row_end) {
    int gx;
    if (par_grid_dims(p, &gx, nullptr, nullptr) != PAR_OK || !elem_ok(E) || !d_map || !frame || !packed || !fill ||
        row_begin < 0 || row_end > p->height || row_begin > row_end) {
        return PAR_ERR_INVALID_ARG;
    }
    if (row_begin == row_end) return PAR_OK;
    const int W = p->width, H = p->height, B = p->bin_size;
    plane_fill f;
    if (E == 28) {
        std::memcpy(f.w, fill, 28);
    } else {
        uint32_t word = 0;
        if (E == 4) std::memcpy(&word, fill, 4);
        else word = (uint32_t)(*static_cast<const uint8_t*>(fill)) * 0x01010101u;
        for (uint32_t& w : f.w) w = word;
    }
    const int u = plane_unit(W, B, E, packed, frame);
    const int upt = B * E / u;
    const size_t RB = (size_t)W * (size_t)E;
    // (the reciprocal is exact while row * B < 2^32)
    const uint32_t magic_b = (uint64_t)H * (uint64_t)B < (1ull << 32) ? (uint32_t)((1ull << 32) / (uint64_t)B + 1ull) : 0u;
    const unsigned bx = (unsigned)((RB / (size_t)u + DELTA_THREADS - 1) / DELTA_THREADS);
    // each workgroup streams a few rows: about 2 048 workgroups write at the rate HBM takes
    const unsigned rows = (unsigned)(row_end - row_begin);
    unsigned by = 2048u / bx;
    by = by < 1u ? 1u : by;
    by = by > rows ? rows : by;
    by = by > 65535u ? 65535u : by;
    with_unit(u, [&](auto U) {
        hipLaunchKernelGGL(plane_assemble_kernel<U()>, dim3(bx, by), dim3(DELTA_THREADS), 0, s, d_map, gx, RB, B, upt, E,
                           row_begin, row_end, static_cast<const uint8_t*>(packed), static_cast<uint8_t*>(frame), f, magic_b);
    });
    return status_of(hipGetLastError());
}

int plane_fetch(const par_params* p, hipStream_t s, int E, const int32_t* d_count, const int32_t* d_tiles,
                const void* d_packed, int capacity, int32_t* tiles, void* packed, int* n, int* count) {
    if (!params_ok(p) || !elem_ok(E) || capacity < 0 || !d_count || !d_tiles || !d_packed || !tiles || !packed || !n ||
        !count) {
        return PAR_ERR_INVALID_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PAR_ERR_NO_DEVICE;
    int32_t total = 0;
    hipError_t e = hipMemcpyAsync(&total, d_count, sizeof(total), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return status_of(e);
    *count = total;
    *n = 0;
    if (total <= 0 || total > capacity) return PAR_OK;
    const size_t slot = (size_t)p->bin_size * (size_t)p->bin_size * (size_t)E;
    e = hipMemcpyAsync(tiles, d_tiles, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(packed, d_packed, (size_t)total * slot, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return status_of(e);
    *n = total;
    return PAR_OK;
}

}  // namespace

extern "C" {

// ---- plane tiles: what only these calls check, then the operation ------------------------------------------------------

int par_plane_tiles_changed_device(const par_params* params, void* stream, int elem_bytes, const void* a, const void* b,
                                   int row_begin, int row_end, int32_t* d_map, int32_t* d_tiles, int capacity,
                                   int32_t* d_count) {
    return plane_changed(params, (hipStream_t)stream, elem_bytes, a, b, row_begin, row_end, d_map, d_tiles, capacity,
                         d_count);
}

int par_plane_tiles_pack(const par_params* params, void* stream, int elem_bytes, const int32_t* d_tiles, int n,
                         const void* block, int row_begin, int row_end, void* packed) {
    return plane_copy(true, params, (hipStream_t)stream, elem_bytes, d_tiles, nullptr, n, row_begin, row_end, block, packed);
}

int par_plane_tiles_pack_counted(const par_params* params, void* stream, int elem_bytes, const int32_t* d_tiles,
                                 const int32_t* d_count, int capacity, const void* block, int row_begin, int row_end,
                                 void* packed) {
    if (!d_count) return PAR_ERR_INVALID_ARG;
    return plane_copy(true, params, (hipStream_t)stream, elem_bytes, d_tiles, d_count, capacity, row_begin, row_end, block,
                      packed);
}

int par_plane_tiles_unpack(const par_params* params, void* stream, int elem_bytes, const int32_t* d_tiles, int n,
                           const void* packed, void* frame) {
    if (!params) return PAR_ERR_INVALID_ARG;
    return plane_copy(false, params, (hipStream_t)stream, elem_bytes, d_tiles, nullptr, n, 0, params->height, packed, frame);
}

int par_plane_tiles_assemble(const par_params* params, void* stream, int elem_bytes, const int32_t* d_map,
                             const void* packed, const void* fill, void* frame, int row_begin, int row_end) {
    return plane_assemble(params, (hipStream_t)stream, elem_bytes, d_map, packed, fill, frame, row_begin, row_end);
}

int par_plane_tiles_fetch(const par_params* params, void* stream, int elem_bytes, const int32_t* d_count,
                          const int32_t* d_tiles, const void* d_packed, int capacity, int32_t* tiles, void* packed, int* n,
                          int* count) {
    return plane_fetch(params, (hipStream_t)stream, elem_bytes, d_count, d_tiles, d_packed, capacity, tiles, packed, n,
                       count);
}

// ---- the 4-byte calls: the same operations on `fb` planes -------------------------------------------------------------
// Pack and unpack had a kernel of their own once, which had no test for a list entry outside the grid (bx >= gx, by
// outside [0, gy), a negative word) but whose edge arithmetic wrote nothing for one: the skip in plane_copy_kernel gives
// the same bytes.

int par_tiles_pack(const par_params* params, void* stream, const int32_t* d_tiles, int n, const par_color* fb_block,
                   int row_begin, int row_end, par_color* packed) {
    return hip_only(plane_copy(true, params, (hipStream_t)stream, 4, d_tiles, nullptr, n, row_begin, row_end, fb_block,
                               packed));
}

int par_tiles_unpack(const par_params* params, void* stream, const int32_t* d_tiles, int n, const par_color* packed,
                     par_color* frame) {
    if (!params) return PAR_ERR_INVALID_ARG;
    return hip_only(plane_copy(false, params, (hipStream_t)stream, 4, d_tiles, nullptr, n, 0, params->height, packed,
                               frame));
}

// The fill is the background, and this call alone reads the ambient.
int par_tiles_assemble(const par_params* params, void* stream, const int32_t* d_map, const par_color* packed,
                       par_color* frame, int row_begin, int row_end) {
    if (!params || !(params->ambient >= 0.f && params->ambient <= 1.f)) return PAR_ERR_INVALID_ARG;
    const uint8_t ch = (uint8_t)((float)params->background * params->ambient);  // Color{127,127,127,0} * ambient
    const uint8_t fill[4] = {ch, ch, ch, 0};
    return hip_only(plane_assemble(params, (hipStream_t)stream, 4, d_map, packed, fill, frame, row_begin, row_end));
}

int par_tiles_changed_device(const par_params* params, void* stream, const par_color* a, const par_color* b,
                             int row_begin, int row_end, int32_t* d_map, int32_t* d_tiles, int capacity,
                             int32_t* d_count) {
    return plane_changed(params, (hipStream_t)stream, 4, a, b, row_begin, row_end, d_map, d_tiles, capacity, d_count);
}

int par_tiles_pack_counted(const par_params* params, void* stream, const int32_t* d_tiles, const int32_t* d_count,
                           int capacity, const par_color* fb_block, int row_begin, int row_end, par_color* packed) {
    if (!d_count) return PAR_ERR_INVALID_ARG;
    return plane_copy(true, params, (hipStream_t)stream, 4, d_tiles, d_count, capacity, row_begin, row_end, fb_block, packed);
}

int par_tiles_fetch(const par_params* params, void* stream, const int32_t* d_count, const int32_t* d_tiles,
                    const par_color* d_packed, int capacity, int32_t* tiles, par_color* packed, int* n, int* count) {
    return plane_fetch(params, (hipStream_t)stream, 4, d_count, d_tiles, d_packed, capacity, tiles, packed, n, count);
}

}  // extern "C"
