// par_cells_fit_steps.h — the steps of a cells fit, shared by the fitted-cells add-on (par_cells_fit.hip) and the
// machine-fit add-on (par_machine_fit.hip): the work block's head, the entry, the cell pass, A_0, a seed step, the assign
// pass with its tallies as a policy, the two-nibble selection and the emit. One implementation per step: kernels and
// __forceinline__ device code in an unnamed namespace, every unit gets its own copy and emits what it launches.
//
// The pixel arithmetic is cells_kernel's (par_cells.hip), through par_cells_lanes.h: four pixels a lane, a cell is 16, 32
// or 64 lanes of one wavefront, a workgroup of 256 threads takes the 16, 8 or 4 cells side by side in one cell row (a
// "group"), v_sad_u8 and min3 for distances, the DPP row sum and the cell sums for E. Nothing per pixel is stored: the
// work block holds 25 bytes a cell and a fixed head.
//   entry    H, the arg-max words and the tallies to 0, the errors to 0, seeds_out[0]
//   cells    m(p) against the master in LDS, h_c as a histogram a cell in LDS (integer adds), H as the workgroup's
//            sum of them flushed with integer atomics, W_c by K maxima of (h_c + 1) << 8 | 255 - j over
//            the cell's lanes, own(c) along the way
//   top      one workgroup: A_0, K maxima of (H + 1) << 8 | 255 - j, into the table
//   step m   m = 0 .. S - 1: the sub-palette is table[0, K) for m == 0, else W_c* of the cell the 64-bit maximum slot[m]
//            names (every workgroup reads the one word; workgroup 0 also writes table[m * K ..] and seeds_out[m]); e(c, A_m)
//            of its cells, best, and, but for the last, one atomicMax a workgroup of (gain + 2^18) << 20 | 2^20 - 1 - c
//            into slot[m + 1]: the largest signed gain, the lowest cell among equals, whatever the order
//   assign   fit_assign: a mode (choose s* and keep it, read it back, or choose for the error alone) and a tally policy:
//            what a pixel adds to the workgroup's LDS tallies under its entry, and how they are flushed. NibbleTally is
//            the medians': HI the tallies of the high nibbles, LO of the low nibbles of the values whose high nibble was
//            chosen. A policy also says where an entry of the table is read and tallied (a pooled entry is one entry).
//   select   par_palette_refine_device's two-nibble selection, one lane an entry; LO moves the table's entries
//   emit     the table to table_out, byte by byte
// In the cell pass, the steps and the assign passes a workgroup walks the groups blockIdx.x, + gridDim.x, ...: at most
// 2048 workgroups (768 where each holds the 48 KiB of tallies), so that H, the arg-max word and the tallies take a few
// thousand atomics a launch and not one set a group (a launch of 16 384 workgroups each ending in an atomicMax on one word
// took three times what the same arithmetic takes in par_quantize_cells_device).
// No workgroup waits on another and nothing spins: a kernel boundary is the only wait.
#ifndef PAR_CELLS_FIT_STEPS_H
#define PAR_CELLS_FIT_STEPS_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_cells_lanes.h"

namespace {

typedef unsigned long long u64;

constexpr uint32_t CF_THREADS = 256;
constexpr uint32_t CF_MAX_TABLE = 256;
constexpr uint32_t CF_MAX_CELLS = 1u << 20, CF_MAX_SUB_SIZE = 16, CF_MAX_ROUNDS = 32;  // both headers' limits
constexpr uint32_t CF_BINS = CF_MAX_TABLE * 3 * 16;  // dwords
constexpr uint32_t CF_OFF_H = 0, CF_OFF_SLOT = 1024, CF_OFF_TABLE = 3072, CF_OFF_HIGH = 4096, CF_OFF_RANK = 5120;
constexpr uint32_t CF_OFF_BINS = 10240, CF_HEAD_BYTES = CF_OFF_BINS + 4 * CF_BINS;  // 59392
constexpr uint32_t CF_BYTES_PER_CELL = 25;
constexpr uint32_t CF_CELL_MASK = CF_MAX_CELLS - 1;
constexpr int CF_GAIN_BIAS = 1 << 18;  // above 256 * 765
constexpr uint32_t CF_TALLY_GROUPS = 768;  // workgroups of an assign pass that holds tallies: three a compute unit
constexpr uint32_t CF_WALK_GROUPS = 2048;  // workgroups of the cell pass and of a step: eight a compute unit
static_assert(CF_HEAD_BYTES == 59392 && CF_HEAD_BYTES % 16 == 0, "the header's formula; a wanted list is 16 bytes, aligned");
static_assert(CF_MAX_CELLS == 1 << 20, "the arg-max key holds 2^20 - 1 - c in 20 bits");

struct Fit {
    uint32_t* H;      // [256]
    u64* slot;        // [256]: slot[m] names c* of step m
    uint32_t* table;  // [256]: the current table, four bytes an entry
    uint32_t* high;   // [256]
    uint32_t* rank;   // [256][4]
    uint32_t* bins;   // [256][3][16]
    uint4* W;         // a cell's wanted list, a byte an index
    uint32_t *own, *best;
    uint8_t* sel;     // a cell's s* of the round
};

Fit fit_of(void* block, size_t cells) {
    char* b = static_cast<char*>(block);
    char* per_cell = b + CF_HEAD_BYTES;
    return {reinterpret_cast<uint32_t*>(b + CF_OFF_H),    reinterpret_cast<u64*>(b + CF_OFF_SLOT),
            reinterpret_cast<uint32_t*>(b + CF_OFF_TABLE), reinterpret_cast<uint32_t*>(b + CF_OFF_HIGH),
            reinterpret_cast<uint32_t*>(b + CF_OFF_RANK),  reinterpret_cast<uint32_t*>(b + CF_OFF_BINS),
            reinterpret_cast<uint4*>(per_cell),            reinterpret_cast<uint32_t*>(per_cell + 16 * cells),
            reinterpret_cast<uint32_t*>(per_cell + 20 * cells), reinterpret_cast<uint8_t*>(per_cell + 24 * cells)};
}

struct Geo {
    uint32_t width, height, gcx, gx, groups;  // gx: groups a cell row; groups = gx * gcy
};

__device__ __forceinline__ uint32_t entry_bytes(const uint8_t* palette, uint32_t i) {
    const uint8_t* e = palette + 4u * i;
    return (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16) | ((uint32_t)e[3] << 24);
}

__device__ __forceinline__ u64 wave_max(u64 v) {
    for (int s = 32; s; s >>= 1) v = std::max(v, (u64)__shfl_xor(v, s));
    return v;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
    for (int s = 32; s; s >>= 1) v += (u64)__shfl_xor(v, s);
    return v;
}

// The four pixels of this lane in group `group`: its cell (cx, cy), which of them exist, and their colours (alpha 0).
template <int CW, int CH>
__device__ __forceinline__ void lane_pixels(const uint32_t* fb, const Geo& g, uint32_t group, uint32_t& cx, uint32_t& cy,
                                            bool live[4], uint32_t rgb[4]) {
    constexpr uint32_t LANES = CW * CH / 4, QUADS = CW / 4, CELLS = CF_THREADS / LANES;
    const uint32_t t = threadIdx.x, j = t % LANES;
    cy = group / g.gx;
    cx = (group - cy * g.gx) * CELLS + t / LANES;
    const uint32_t x0 = cx * CW + (j % QUADS) * 4u, y = cy * CH + j / QUADS;
    const size_t at = (size_t)y * g.width + x0;
    for (int i = 0; i < 4; i++) {
        live[i] = y < g.height && x0 + i < g.width;
        rgb[i] = live[i] ? fb[at + i] & QUANT_RGB : 0u;
    }
}

// The sum over a cell of its lanes' `v` (at most 4 * 765 a lane), in every lane of the cell.
template <int LANES>
__device__ __forceinline__ uint32_t cell_sum(uint32_t v) {
    uint32_t sum, unused;
    cell_sums<LANES>(row_sum(v), sum, unused);
    return sum;
}

__global__ __launch_bounds__(CF_THREADS) void fit_entry_kernel(Fit w, uint32_t* seeds_out, u64* errors_out, uint32_t rounds) {
    const uint32_t i = blockIdx.x * CF_THREADS + threadIdx.x;
    if (i < 256u) {
        w.H[i] = 0u;
        w.slot[i] = 0ull;
    }
    if (errors_out && i <= rounds) errors_out[i] = 0ull;
    if (seeds_out && i == 0u) seeds_out[0] = 0xFFFFFFFFu;
    if (i < CF_BINS) w.bins[i] = 0u;
}

template <int CW, int CH>
__global__ __launch_bounds__(CF_THREADS) void fit_cells_kernel(Fit w, const uint32_t* fb, Geo g, const uint8_t* palette,
                                                               uint32_t n_colors, uint32_t K) {
    constexpr uint32_t LANES = CW * CH / 4, CELLS = CF_THREADS / LANES, PER = 256u / LANES;
    __shared__ __attribute__((aligned(16))) uint32_t pal[256];
    __shared__ uint32_t hc[CELLS][256];
    const uint32_t t = threadIdx.x, j = t % LANES, cell = t / LANES;
    pal[t] = entry_bytes(palette, std::min(t, n_colors - 1u)) & QUANT_RGB;
    uint32_t total = 0u;  // H[t] over this workgroup's groups
    for (uint32_t group = blockIdx.x; group < g.groups; group += gridDim.x) {  // (as many rounds for every lane)
        for (uint32_t c = 0; c < CELLS; c++) hc[c][t] = 0u;
        uint32_t cx, cy, rgb[4];
        bool live[4];
        lane_pixels<CW, CH>(fb, g, group, cx, cy, live, rgb);
        __syncthreads();

        // m(p): (L1 distance << 16) + index, the minimum takes the lowest index among equals
        uint32_t key[4] = {~0u, ~0u, ~0u, ~0u};
        uint32_t k = 0;
        for (; k + 4 <= n_colors; k += 4) {
            const uint4 e = *reinterpret_cast<const uint4*>(&pal[k]);
            for (int i = 0; i < 4; i++) {
                key[i] = min3u(key[i], __builtin_amdgcn_sad_hi_u8(rgb[i], e.x, k), __builtin_amdgcn_sad_hi_u8(rgb[i], e.y, k + 1u));
                key[i] = min3u(key[i], __builtin_amdgcn_sad_hi_u8(rgb[i], e.z, k + 2u), __builtin_amdgcn_sad_hi_u8(rgb[i], e.w, k + 3u));
            }
        }
        for (; k < n_colors; k++) {
            for (int i = 0; i < 4; i++) key[i] = std::min(key[i], __builtin_amdgcn_sad_hi_u8(rgb[i], pal[k], k));
        }
        // h_c: equal neighbours merge to the right, a pixel that does not exist counts 0 wherever it lands
        uint32_t m[4], n[4];
        for (int i = 0; i < 4; i++) {
            m[i] = key[i] & 0xFFFFu;
            n[i] = live[i] ? 1u : 0u;
        }
        for (int i = 1; i < 4; i++) {
            if (m[i] == m[i - 1]) { n[i] += n[i - 1]; n[i - 1] = 0u; }
        }
        for (int i = 0; i < 4; i++) {
            if (n[i]) atomicAdd(&hc[cell][m[i]], n[i]);
        }
        __syncthreads();

        for (uint32_t c = 0; c < CELLS; c++) total += hc[c][t];

        // W_c and own(c): lane j of the cell holds the keys of the indices j, j + LANES, ...; K times the cell's maximum
        // leaves, and every lane of the cell learns it (all 64 lanes are here: K is a kernel argument)
        uint32_t keys[PER];
        for (uint32_t i = 0; i < PER; i++) {
            const uint32_t idx = j + i * LANES;
            keys[i] = idx < n_colors ? ((hc[cell][idx] + 1u) << 8) | (255u - idx) : 0u;
        }
        uint32_t d[4] = {~0u, ~0u, ~0u, ~0u};
        u64 lo = 0ull, hi = 0ull;
        for (uint32_t r = 0; r < K; r++) {
            uint32_t top = 0u;
            for (uint32_t i = 0; i < PER; i++) top = std::max(top, keys[i]);
            for (uint32_t s = 1; s < LANES; s <<= 1) top = std::max(top, (uint32_t)__shfl_xor((int)top, (int)s));
            for (uint32_t i = 0; i < PER; i++) keys[i] = keys[i] == top ? 0u : keys[i];
            const uint32_t idx = 255u - (top & 255u);
            const uint32_t e = pal[idx];
            for (int i = 0; i < 4; i++) d[i] = std::min(d[i], __builtin_amdgcn_sad_u8(rgb[i], e, 0u));
            if (r < 8u) lo |= (u64)idx << (8u * r);
            else hi |= (u64)idx << (8u * (r - 8u));
        }
        uint32_t mine = 0u;
        for (int i = 0; i < 4; i++) mine += live[i] ? d[i] : 0u;
        const uint32_t own = cell_sum<LANES>(mine);
        if (j == 0u && cx < g.gcx) {
            const uint32_t c = cx + cy * g.gcx;
            w.W[c] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
            w.own[c] = own;
        }
        __syncthreads();  // (the histograms are read to the end before the next group zeroes them)
    }
    if (total) atomicAdd(&w.H[t], total);
}

// One workgroup: A_0 into table[0, K).
__global__ __launch_bounds__(CF_THREADS) void fit_top_kernel(Fit w, const uint8_t* palette, uint32_t n_colors, uint32_t K) {
    __shared__ u64 wave_top[CF_THREADS / 64];
    const uint32_t t = threadIdx.x;
    u64 key = t < n_colors ? (((u64)w.H[t] + 1ull) << 8) | (u64)(255u - t) : 0ull;
    for (uint32_t r = 0; r < K; r++) {
        u64 top = wave_max(key);
        if ((t & 63u) == 0u) wave_top[t >> 6] = top;
        __syncthreads();
        for (uint32_t k = 0; k < CF_THREADS / 64; k++) top = std::max(top, wave_top[k]);
        if (key == top) {  // (one thread: a key holds its index)
            key = 0ull;
            w.table[r] = entry_bytes(palette, t);
        }
        __syncthreads();
    }
}

// Evaluation m of the seed: e(c, A_m) of the group's cells. `last`: no arg-max is wanted behind it.
template <int CW, int CH>
__global__ __launch_bounds__(CF_THREADS) void fit_step_kernel(Fit w, const uint32_t* fb, Geo g, const uint8_t* palette,
                                                              uint32_t K, uint32_t m, bool last, uint32_t* seeds_out) {
    constexpr uint32_t LANES = CW * CH / 4;
    __shared__ __attribute__((aligned(16))) uint32_t sub[CF_MAX_SUB_SIZE];
    __shared__ u64 wave_best[CF_THREADS / 64];
    const uint32_t t = threadIdx.x, j = t % LANES;
    if (t < CF_MAX_SUB_SIZE) {
        uint32_t e = 0u;
        if (t < K) {
            if (m == 0u) {
                e = w.table[t];
            } else {
                const uint32_t c = CF_CELL_MASK - (uint32_t)(w.slot[m] & CF_CELL_MASK);  // (a cell of the frame: slot[m] is not 0)
                const uint4 wl = w.W[c];
                const uint32_t word = t < 4u ? wl.x : (t < 8u ? wl.y : (t < 12u ? wl.z : wl.w));
                e = entry_bytes(palette, (word >> (8u * (t & 3u))) & 0xFFu);
                if (blockIdx.x == 0u) {
                    w.table[m * K + t] = e;
                    if (t == 0u && seeds_out) seeds_out[m] = c;
                }
            }
        }
        sub[t] = e;  // (nearest_distances masks alpha)
    }
    __syncthreads();

    u64 key = 0ull;
    for (uint32_t group = blockIdx.x; group < g.groups; group += gridDim.x) {  // (as many rounds for every lane)
        uint32_t cx, cy, rgb[4], d[4];
        bool live[4];
        lane_pixels<CW, CH>(fb, g, group, cx, cy, live, rgb);
        nearest_distances(rgb, sub, (int)K, d);
        uint32_t mine = 0u;
        for (int i = 0; i < 4; i++) mine += live[i] ? d[i] : 0u;
        const uint32_t e = cell_sum<LANES>(mine);
        if (j == 0u && cx < g.gcx) {
            const uint32_t c = cx + cy * g.gcx;
            const uint32_t best = m == 0u ? e : std::min(w.best[c], e);
            w.best[c] = best;
            if (!last) key = std::max(key, ((u64)(uint32_t)((int)best - (int)w.own[c] + CF_GAIN_BIAS) << 20) | (u64)(CF_CELL_MASK - c));
        }
    }
    if (last) return;
    key = wave_max(key);
    if ((t & 63u) == 0u) wave_best[t >> 6] = key;
    __syncthreads();
    if (t == 0u) {
        for (uint32_t k = 1; k < CF_THREADS / 64; k++) key = std::max(key, wave_best[k]);
        atomicMax(&w.slot[m + 1u], key);
    }
}

constexpr int CF_HI = 0, CF_LO = 1, CF_ERROR = 2;

// Every entry of the table is its own: read where it stands, tallied where it stands.
struct OwnEntries {
    __device__ __forceinline__ uint32_t source(uint32_t t) const { return t; }
    __device__ __forceinline__ uint32_t tally_at(uint32_t chosen, uint32_t K, uint32_t k) const { return chosen * K + k; }
};

// The medians' tallies: [256][3][16] counts of a nibble in a workgroup's LDS, flushed once with integer atomics; LO tallies
// the low nibbles of the values whose high nibble is the chosen one (w.high). No tallies at all where BINS is 4.
template <bool LO, bool TALLY = true, class ENTRIES = OwnEntries>
struct NibbleTally {
    static constexpr uint32_t BINS = TALLY ? CF_BINS : 4, HIGH = LO ? CF_MAX_TABLE : 1, PERIOD = 0;
    ENTRIES entries;
    __device__ __forceinline__ void begin(const Fit& w, uint32_t* bins, uint32_t* high) const {
        const uint32_t t = threadIdx.x;
        if (TALLY) {
            const u32x4 zero = {0u, 0u, 0u, 0u};
            for (uint32_t i = t; i < CF_BINS / 4; i += CF_THREADS) reinterpret_cast<u32x4*>(bins)[i] = zero;
        }
        if (LO) high[t] = w.high[t];
    }
    __device__ __forceinline__ void add(uint32_t* bins, const uint32_t* high, uint32_t at, uint32_t rgb, uint32_t n) const {
        tally_add<LO>(bins, high, at, rgb, n);
    }
    __device__ __forceinline__ void flush(const Fit& w, uint32_t* bins) const {
        for (uint32_t i = threadIdx.x; i < CF_BINS / 4; i += CF_THREADS) {
            const u32x4 v = reinterpret_cast<const u32x4*>(bins)[i];
            for (int k = 0; k < 4; k++) {
                if (v[k]) atomicAdd(&w.bins[4 * i + k], v[k]);
            }
        }
    }
};

// The assign step of a round over the groups blockIdx.x, + gridDim.x, ...: MODE CF_HI chooses s*, keeps it, adds the
// error to *error_out (where given) and tallies; CF_LO reads s* back and tallies; CF_ERROR chooses and adds the error
// alone. What is tallied is the policy's; a policy with a PERIOD flushes after that many groups too (its counts are
// narrow) and then leaves its LDS zero.
template <int CW, int CH, int MODE, class TALLY>
__device__ __forceinline__ void fit_assign(const Fit& w, const uint32_t* fb, const Geo& g, int S, int K, u64* error_out,
                                           const TALLY& tally) {
    constexpr uint32_t LANES = CW * CH / 4;
    constexpr bool TALLIES = MODE != CF_ERROR;
    __shared__ __attribute__((aligned(16))) uint32_t tab[CF_MAX_TABLE];
    __shared__ __attribute__((aligned(16))) uint32_t bins[TALLY::BINS];
    __shared__ uint32_t high[TALLY::HIGH];
    __shared__ u64 wave_err[CF_THREADS / 64];
    const uint32_t t = threadIdx.x, j = t % LANES;
    tab[t] = t < (uint32_t)(S * K) ? w.table[tally.entries.source(t)] & QUANT_RGB : 0u;
    tally.begin(w, bins, high);
    __syncthreads();

    u64 err = 0ull;
    uint32_t walked = 0u;
    for (uint32_t group = blockIdx.x; group < g.groups; group += gridDim.x) {  // (as many rounds for every lane)
        uint32_t cx, cy, rgb[4];
        bool live[4];
        lane_pixels<CW, CH>(fb, g, group, cx, cy, live, rgb);
        const bool holder = j == 0u && cx < g.gcx;
        const uint32_t c = cx + cy * g.gcx;
        uint32_t chosen;
        if (MODE == CF_LO) {
            chosen = cx < g.gcx ? w.sel[c] : 0u;
        } else {
            // cells_kernel's pass 1: E(s) a pair of sub-palettes at a time, the minimum of (E(s) << 8) | s
            uint32_t best = ~0u;
            for (int s = 0; s < S; s += 2) {
                const bool two = s + 1 < S;
                uint32_t d0[4], d1[4] = {0u, 0u, 0u, 0u};
                nearest_distances(rgb, tab + s * K, K, d0);
                if (two) nearest_distances(rgb, tab + (s + 1) * K, K, d1);
                uint32_t v = 0;
                for (int i = 0; i < 4; i++) v += live[i] ? d0[i] | (d1[i] << 16) : 0u;
                uint32_t even, odd;
                cell_sums<LANES>(row_sum(v), even, odd);
                best = std::min(best, (even << 8) | (uint32_t)s);
                if (two) best = std::min(best, (odd << 8) | (uint32_t)(s + 1));
            }
            chosen = best & 0xFFu;
            if (holder) {
                err += best >> 8;
                if (MODE == CF_HI) w.sel[c] = (uint8_t)chosen;
            }
        }
        if (TALLIES) {
            // pass 2: k(p, s*), every lane under its own cell's sub-palette
            const uint32_t* sub = tab + chosen * (uint32_t)K;
            uint32_t key[4] = {~0u, ~0u, ~0u, ~0u};
            for (int k = 0; k < K; k++) {
                const uint32_t e = sub[k];
                for (int i = 0; i < 4; i++) key[i] = std::min(key[i], __builtin_amdgcn_sad_hi_u8(rgb[i], e, (uint32_t)k));
            }
            uint32_t at[4], n[4];
            for (int i = 0; i < 4; i++) {
                at[i] = tally.entries.tally_at(chosen, (uint32_t)K, key[i] & 0xFFFFu);
                n[i] = live[i] ? 1u : 0u;
            }
            for (int i = 1; i < 4; i++) {
                if (at[i] == at[i - 1] && rgb[i] == rgb[i - 1]) { n[i] += n[i - 1]; n[i - 1] = 0u; }
            }
            for (int i = 0; i < 4; i++) {
                if (n[i]) tally.add(bins, high, at[i], rgb[i], n[i]);
            }
            if (TALLY::PERIOD != 0 && ++walked == TALLY::PERIOD) {  // (every lane alike: as many rounds for every lane)
                walked = 0u;
                __syncthreads();
                tally.flush(w, bins);
                __syncthreads();
            }
        }
    }
    if (MODE != CF_LO && error_out) {
        err = wave_sum(err);
        if ((t & 63u) == 0u) wave_err[t >> 6] = err;
    }
    __syncthreads();
    if (MODE != CF_LO && error_out && t == 0u) {
        for (uint32_t k = 1; k < CF_THREADS / 64; k++) err += wave_err[k];
        atomicAdd(error_out, err);
    }
    if (TALLIES) tally.flush(w, bins);
}

template <int CW, int CH, int MODE>
__global__ __launch_bounds__(CF_THREADS) void fit_assign_kernel(Fit w, const uint32_t* fb, Geo g, int S, int K, u64* error_out) {
    fit_assign<CW, CH, MODE>(w, fb, g, S, K, error_out, NibbleTally<MODE == CF_LO, MODE != CF_ERROR>{});
}

// One lane an entry, par_palette_refine_device's selection. Stage hi: a channel's n is the sum of its 16 bins and its
// rank (n - 1) / 2; the high nibble is the first at which the running count passes the rank. Stage lo: the low nibble
// likewise from the rank within; an entry of the table with pixels gets its three medians and alpha 255. Both leave the
// bins zero.
template <bool LO>
__global__ __launch_bounds__(CF_MAX_TABLE) void fit_select_kernel(Fit w, uint32_t entries) {
    const uint32_t k = threadIdx.x;
    const uint32_t high = LO ? w.high[k] : 0u;
    uint32_t n_k = LO ? w.rank[4 * k + 3] : 0u, picked = 0u;
    for (int c = 0; c < 3; c++) {
        uint32_t* const row = w.bins + 48u * k + 16u * c;
        uint32_t b[16], n = 0u;
        for (int v = 0; v < 16; v++) {
            b[v] = row[v];
            n += b[v];
            row[v] = 0u;
        }
        const uint32_t rank = LO ? w.rank[4 * k + c] : (n ? (n - 1u) / 2u : 0u);
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
            w.rank[4 * k + c] = rank - below;
            n_k = n;
        }
    }
    if (LO) {
        if (k < entries && n_k > 0u) w.table[k] = picked | 0xFF000000u;
    } else {
        w.rank[4 * k + 3] = n_k;
        w.high[k] = picked;
    }
}

// Entry k of table_out is the table's entry `from`.
__device__ __forceinline__ void fit_emit(const Fit& w, uint32_t k, uint32_t from, uint8_t* table_out) {
    const uint32_t e = w.table[from];
    for (uint32_t b = 0; b < 4; b++) table_out[4u * k + b] = (uint8_t)(e >> (8u * b));
}

bool cell_dim_ok(int v) { return v == 8 || v == 16; }

// The cells of a frame, 0 outside the limits.
size_t cells_of(int width, int height, int cell_w, int cell_h) {
    if (width < 1 || height < 1 || !cell_dim_ok(cell_w) || !cell_dim_ok(cell_h)) return 0;
    const uint64_t cells = (uint64_t)(((int64_t)width + cell_w - 1) / cell_w) * (uint64_t)(((int64_t)height + cell_h - 1) / cell_h);
    return cells <= CF_MAX_CELLS ? (size_t)cells : 0;
}

bool fit_args_ok(const uint8_t* fb, int width, int height, int cell_w, int cell_h, const uint8_t* palette, int n_colors,
                 int n_sub, int sub_size, int rounds, const uint8_t* table_out) {
    if (!fb || !palette || !table_out || cells_of(width, height, cell_w, cell_h) == 0) return false;
    if (sub_size < 1 || sub_size > (int)CF_MAX_SUB_SIZE || n_colors < sub_size || n_colors > 256) return false;
    if (n_sub < 1 || (int64_t)n_sub * sub_size > (int64_t)CF_MAX_TABLE) return false;
    return rounds >= 0 && rounds <= (int)CF_MAX_ROUNDS;
}

// The frame's geometry under cells of CW x CH.
template <int CW, int CH>
Geo geo_of(int width, int height) {
    constexpr uint32_t CELLS = CF_THREADS / (CW * CH / 4);
    const uint32_t W = (uint32_t)width, H = (uint32_t)height;
    const uint32_t gcx = (W + CW - 1) / CW, gcy = (H + CH - 1) / CH, gx = (gcx + CELLS - 1) / CELLS;
    return {W, H, gcx, gx, gx * gcy};
}

struct FitCall {
    const uint8_t* fb;
    int width, height;
    const uint8_t* palette;
    int n_colors, n_sub, sub_size, rounds;
    void* work;
    uint8_t* table_out;
    uint32_t* seeds_out;
    uint64_t* errors_out;
};

// The seed's first three launches: the entry, the cell pass and A_0, against the master at `palette`.
template <int CW, int CH>
hipError_t launch_lists(hipStream_t stream, const FitCall& a, const Fit& w, const Geo& g, const uint8_t* palette) {
    const uint32_t* fb = reinterpret_cast<const uint32_t*>(a.fb);
    const uint32_t K = (uint32_t)a.sub_size, N = (uint32_t)a.n_colors;
    const dim3 block(CF_THREADS), all(std::min(g.groups, CF_WALK_GROUPS));
    hipLaunchKernelGGL(fit_entry_kernel, dim3(CF_BINS / CF_THREADS), block, 0, stream, w, a.seeds_out,
                       reinterpret_cast<u64*>(a.errors_out), (uint32_t)a.rounds);
    hipLaunchKernelGGL((fit_cells_kernel<CW, CH>), all, block, 0, stream, w, fb, g, palette, N, K);
    hipLaunchKernelGGL(fit_top_kernel, dim3(1), block, 0, stream, w, palette, N, K);
    return hipGetLastError();
}

// The seed's S steps behind them.
template <int CW, int CH>
hipError_t launch_steps(hipStream_t stream, const FitCall& a, const Fit& w, const Geo& g, const uint8_t* palette) {
    const uint32_t* fb = reinterpret_cast<const uint32_t*>(a.fb);
    const uint32_t S = (uint32_t)a.n_sub, K = (uint32_t)a.sub_size;
    const dim3 block(CF_THREADS), all(std::min(g.groups, CF_WALK_GROUPS));
    hipError_t e = hipSuccess;
    for (uint32_t m = 0; m < S && e == hipSuccess; m++) {
        hipLaunchKernelGGL((fit_step_kernel<CW, CH>), all, block, 0, stream, w, fb, g, palette, K, m, m + 1 == S, a.seeds_out);
        if ((m & 63u) == 63u) e = hipGetLastError();
    }
    return e;
}

}  // namespace

#endif
