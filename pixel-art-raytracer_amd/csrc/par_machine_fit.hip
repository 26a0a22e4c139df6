// par_machine_fit.hip — the machine-fit add-on (libpar_machine_fit.so): par_cells_fit_device's table fitted under a tile
// machine's colour depth and backdrop rule (par_machine_round, par_machine_fit_device, par_machine_fit_host). The
// contract is beside the declarations in addons/include/par_machine_fit.h; nothing here knows a par_context or a
// par_params, and nothing here is linked into another library.
//
// The cell pass, A_0, the steps, the assign pass, the two-nibble selection and the emit are par_cells_fit_steps.h's, one
// copy that par_cells_fit.hip launches too. What is this unit's own:
//   round    the master rounded to the lattice into the work block (every later launch reads that copy), and this unit's
//            tallies to 0
//   own      backdrop alone: b0 from H (every workgroup finds it for itself, one maximum over 256 keys), then every W_c
//            becomes b0 and the first K - 1 others of it, and own(c) is evaluated again. A_0 needs nothing: it begins
//            with b0 as it is.
//   move     below 8 bits, two tally policies for the shared assign pass. LatticeCount: a pixel adds 1 at the level
//            below it, [256][3][32] counts, 16 bits each in LDS so that they take the plain fit's 48 KiB (96 KiB of
//            dwords would leave one workgroup a compute unit of its 160 KiB, four wavefronts to hide a frame's loads
//            behind); a workgroup flushes them every 63 groups, 64 512 pixels, before a half-word can carry. A lane an
//            entry-channel then finds the interval [a, b) of the lower median, the count below it and the count in it.
//            IntervalSum: a pixel in the chosen interval adds 1 at x == a, else x - a to a sum (under 2^25 a workgroup:
//            342 groups of 1024 pixels, 84 at the most each; the sums are flushed with 64-bit adds, since 2^28 pixels
//            pass 2^32). A lane an entry then takes b where g(b) - g(a) = (b - a) * (n[x <= a] - n[x >= b]) +
//            n_mid * (b - a) - 2 * sum is negative. At 8 bits the move is the medians' two nibbles, the shared policy.
//   pooled   backdrop alone: the S entries at position 0 are entry 0: every reader of the table reads entry 0 for them
//            and every tally lands there, so the selections move entry 0 alone and need not know.
// No workgroup waits on another and nothing spins: a kernel boundary is the only wait.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_machine_fit.h"
#include "par_cells_fit_steps.h"
#include "par_hostcall.h"

namespace {

static_assert(PAR_MACHINE_FIT_MAX_CELLS == CF_MAX_CELLS && PAR_MACHINE_FIT_MAX_SUB_SIZE == CF_MAX_SUB_SIZE &&
              PAR_MACHINE_FIT_MAX_ROUNDS == CF_MAX_ROUNDS, "the limits are the plain fit's");

constexpr uint32_t MF_LEVELS = 32, MF_ROW = 3 * MF_LEVELS, MF_LAT = CF_MAX_TABLE * MF_ROW;  // counts an entry; in all
constexpr uint32_t MF_STAT = 12;                                                            // words an entry
constexpr uint32_t MF_OFF_SUMS = 0, MF_OFF_EQ = 6144, MF_OFF_STAT = 9216, MF_OFF_LAT = 21504, MF_OFF_MASTER = 119808;
constexpr uint32_t MF_HEAD_BYTES = MF_OFF_MASTER + 1024;  // 120832, then the plain fit's block
constexpr uint32_t MF_PERIOD = 63;  // groups between two flushes: 63 * 1024 pixels stay below 2^16
static_assert(MF_OFF_EQ == 8 * CF_MAX_TABLE * 3 && MF_OFF_STAT == MF_OFF_EQ + 4 * CF_MAX_TABLE * 3 &&
              MF_OFF_LAT == MF_OFF_STAT + 4 * CF_MAX_TABLE * MF_STAT && MF_OFF_MASTER == MF_OFF_LAT + 4 * MF_LAT, "the block");
static_assert(MF_HEAD_BYTES + CF_HEAD_BYTES == 180224 && MF_HEAD_BYTES % 16 == 0, "the header's formula");
static_assert(MF_LAT / 2 == CF_BINS && MF_PERIOD * 1024 < 65536, "two counts a dword in the plain fit's LDS");

struct Machine {
    u64* sums;        // [256][3]: the sum of x - a over a < x < b
    uint32_t* eq;     // [256][3]: the count of x == a
    uint32_t* stat;   // [256][3][4]: the count below a, the count in [a, b), n
    uint32_t* lat;    // [256][3][32]: the counts per lattice interval
    uint8_t* master;  // the rounded master
    uint32_t bits;
};

Machine machine_of(void* block, uint32_t bits) {
    char* b = static_cast<char*>(block);
    return {reinterpret_cast<u64*>(b + MF_OFF_SUMS), reinterpret_cast<uint32_t*>(b + MF_OFF_EQ), reinterpret_cast<uint32_t*>(b + MF_OFF_STAT),
            reinterpret_cast<uint32_t*>(b + MF_OFF_LAT), reinterpret_cast<uint8_t*>(b + MF_OFF_MASTER), bits};
}

// ---- the lattice -----------------------------------------------------------------------------------------------------

constexpr int MF_DEPTHS = 4;
const uint32_t MF_BITS[MF_DEPTHS] = {5, 3, 2, 8};

// w(l): par_screen.h's bit replication
__host__ __device__ __forceinline__ uint32_t widen(uint32_t bits, uint32_t l) {
    return bits == 5 ? (l << 3) | (l >> 2) : (bits == 3 ? (l << 5) | (l << 2) | (l >> 1) : (bits == 2 ? l * 0x55u : l));
}

// The highest level whose w(l) is not above x: x's own top bits, or the level below them.
__host__ __device__ __forceinline__ uint32_t level_below(uint32_t bits, uint32_t x) {
    const uint32_t l = x >> (8u - bits);
    return widen(bits, l) > x ? l - 1u : l;
}

// The nearest w(l), the lower of two equally near.
__host__ __device__ __forceinline__ uint32_t rounded(uint32_t bits, uint32_t x) {
    const uint32_t l = level_below(bits, x), a = widen(bits, l);
    if (l + 1u == (1u << bits)) return a;
    const uint32_t b = widen(bits, l + 1u);
    return b - x < x - a ? b : a;
}

__global__ __launch_bounds__(CF_THREADS) void mf_round_kernel(Machine m, const uint8_t* palette, uint32_t n_colors) {
    const uint32_t i = blockIdx.x * CF_THREADS + threadIdx.x;
    if (i < MF_LAT) m.lat[i] = 0u;
    if (i < CF_MAX_TABLE * 3) {
        m.eq[i] = 0u;
        m.sums[i] = 0ull;
    }
    if (i < 4u * n_colors) m.master[i] = (i & 3u) == 3u ? palette[i] : (uint8_t)rounded(m.bits, palette[i]);
}

// ---- the backdrop ----------------------------------------------------------------------------------------------------

// The S entries at position 0 are entry 0 where `pooled`.
struct PooledEntries {
    uint32_t K;
    bool pooled;
    __device__ __forceinline__ uint32_t source(uint32_t t) const { return pooled && t % K == 0u ? 0u : t; }
    __device__ __forceinline__ uint32_t tally_at(uint32_t chosen, uint32_t, uint32_t k) const {
        return pooled && k == 0u ? 0u : chosen * K + k;
    }
};

// b0 at the head of every wanted list, and own(c) under the new list.
template <int CW, int CH>
__global__ __launch_bounds__(CF_THREADS) void mf_own_kernel(Fit w, const uint32_t* fb, Geo g, const uint8_t* palette,
                                                            uint32_t n_colors, uint32_t K) {
    constexpr uint32_t LANES = CW * CH / 4;
    __shared__ uint32_t pal[256];
    __shared__ u64 wave_top[CF_THREADS / 64];
    const uint32_t t = threadIdx.x, j = t % LANES;
    pal[t] = entry_bytes(palette, std::min(t, n_colors - 1u)) & QUANT_RGB;
    u64 top = wave_max(t < n_colors ? (((u64)w.H[t] + 1ull) << 8) | (u64)(255u - t) : 0ull);
    if ((t & 63u) == 0u) wave_top[t >> 6] = top;
    __syncthreads();
    for (uint32_t k = 0; k < CF_THREADS / 64; k++) top = std::max(top, wave_top[k]);
    const uint32_t b0 = 255u - (uint32_t)(top & 255ull);

    for (uint32_t group = blockIdx.x; group < g.groups; group += gridDim.x) {  // (as many rounds for every lane)
        uint32_t cx, cy, rgb[4], d[4];
        bool live[4];
        lane_pixels<CW, CH>(fb, g, group, cx, cy, live, rgb);
        const bool inside = cx < g.gcx;
        const uint32_t c = cx + cy * g.gcx;
        const uint4 wl = inside ? w.W[c] : make_uint4(0u, 0u, 0u, 0u);
        const u64 old_lo = (u64)wl.x | ((u64)wl.y << 32), old_hi = (u64)wl.z | ((u64)wl.w << 32);
        u64 lo = b0, hi = 0ull;
        uint32_t at = 1u;
        const uint32_t e0 = pal[b0];
        for (int i = 0; i < 4; i++) d[i] = __builtin_amdgcn_sad_u8(rgb[i], e0, 0u);
        for (uint32_t r = 0; r < K; r++) {
            const uint32_t idx = (uint32_t)((r < 8u ? old_lo >> (8u * r) : old_hi >> (8u * (r - 8u))) & 0xFFull);
            if (idx != b0 && at < K) {
                const uint32_t e = pal[idx];
                for (int i = 0; i < 4; i++) d[i] = std::min(d[i], __builtin_amdgcn_sad_u8(rgb[i], e, 0u));
                if (at < 8u) lo |= (u64)idx << (8u * at);
                else hi |= (u64)idx << (8u * (at - 8u));
                at++;
            }
        }
        uint32_t mine = 0u;
        for (int i = 0; i < 4; i++) mine += live[i] ? d[i] : 0u;
        const uint32_t own = cell_sum<LANES>(mine);
        if (j == 0u && inside) {  // (the cell's lanes, one wavefront, have read the list above)
            w.W[c] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
            w.own[c] = own;
        }
    }
}

// ---- the move below 8 bits -------------------------------------------------------------------------------------------

// The counts per lattice interval: count l of channel c of entry k is half-word k * 96 + c * 32 + l of the LDS.
struct LatticeCount {
    static constexpr uint32_t BINS = CF_BINS, HIGH = 1, PERIOD = MF_PERIOD;
    PooledEntries entries;
    uint32_t* lat;
    uint32_t bits;
    __device__ __forceinline__ void begin(const Fit&, uint32_t* bins, uint32_t*) const {
        const u32x4 zero = {0u, 0u, 0u, 0u};
        for (uint32_t i = threadIdx.x; i < CF_BINS / 4; i += CF_THREADS) reinterpret_cast<u32x4*>(bins)[i] = zero;
    }
    __device__ __forceinline__ void add(uint32_t* bins, const uint32_t*, uint32_t at, uint32_t rgb, uint32_t n) const {
        for (int c = 0; c < 3; c++) {
            const uint32_t i = at * MF_ROW + (uint32_t)c * MF_LEVELS + level_below(bits, (rgb >> (8 * c)) & 0xFFu);
            atomicAdd(&bins[i >> 1], n << (16u * (i & 1u)));
        }
    }
    // (every thread its own dwords, read and zeroed: the LDS is zero again behind a flush)
    __device__ __forceinline__ void flush(const Fit&, uint32_t* bins) const {
        for (uint32_t i = threadIdx.x; i < CF_BINS; i += CF_THREADS) {
            const uint32_t v = bins[i];
            if (v) {
                bins[i] = 0u;
                if (v & 0xFFFFu) atomicAdd(&lat[2u * i], v & 0xFFFFu);
                if (v >> 16) atomicAdd(&lat[2u * i + 1u], v >> 16);
            }
        }
    }
};

// Inside the chosen interval of a channel of an entry (w.high holds the three levels): the count of x == a and the sum
// of x - a, dwords k * 6 + c * 2 and + 1 of the LDS.
struct IntervalSum {
    static constexpr uint32_t BINS = CF_MAX_TABLE * 6, HIGH = CF_MAX_TABLE, PERIOD = 0;
    PooledEntries entries;
    uint32_t* eq;
    u64* sums;
    uint32_t bits;
    __device__ __forceinline__ void begin(const Fit& w, uint32_t* bins, uint32_t* high) const {
        for (uint32_t i = threadIdx.x; i < BINS; i += CF_THREADS) bins[i] = 0u;
        high[threadIdx.x] = w.high[threadIdx.x];
    }
    __device__ __forceinline__ void add(uint32_t* bins, const uint32_t* high, uint32_t at, uint32_t rgb, uint32_t n) const {
        const uint32_t levels = high[at];
        for (int c = 0; c < 3; c++) {
            const uint32_t x = (rgb >> (8 * c)) & 0xFFu, l = (levels >> (8 * c)) & 0xFFu;
            if (level_below(bits, x) != l) continue;
            const uint32_t a = widen(bits, l);
            if (x == a) atomicAdd(&bins[at * 6u + 2u * (uint32_t)c], n);
            else atomicAdd(&bins[at * 6u + 2u * (uint32_t)c + 1u], n * (x - a));
        }
    }
    __device__ __forceinline__ void flush(const Fit&, uint32_t* bins) const {
        for (uint32_t i = threadIdx.x; i < BINS; i += CF_THREADS) {
            const uint32_t v = bins[i];
            if (v == 0u) continue;
            if (i & 1u) atomicAdd(&sums[i >> 1], (u64)v);
            else atomicAdd(&eq[i >> 1], v);
        }
    }
};

template <int CW, int CH, int MODE, class TALLY>
__global__ __launch_bounds__(CF_THREADS) void mf_assign_kernel(Fit w, const uint32_t* fb, Geo g, int S, int K, u64* error_out,
                                                               TALLY tally) {
    fit_assign<CW, CH, MODE>(w, fb, g, S, K, error_out, tally);
}

// One lane a channel of an entry (768 of them): n, the rank (n - 1) / 2 of the lower median, the first level at which the
// running count passes it, the count below that level and the count at it. The 32 counts are loaded at once (one lane an
// entry and a loop to a run-time bound took 192 loads one behind the other, 33 us a round). Leaves the counts zero.
__global__ __launch_bounds__(3 * CF_MAX_TABLE) void mf_interval_kernel(Fit w, Machine m) {
    const uint32_t t = threadIdx.x, k = t / 3u, c = t - 3u * k, levels = 1u << m.bits;
    uint32_t* const row = m.lat + k * MF_ROW + c * MF_LEVELS;
    uint32_t b[MF_LEVELS], n = 0u;
    for (uint32_t l = 0; l < MF_LEVELS; l++) b[l] = l < levels ? row[l] : 0u;
    for (uint32_t l = 0; l < MF_LEVELS; l++) {
        n += b[l];
        if (b[l]) row[l] = 0u;
    }
    const uint32_t rank = n ? (n - 1u) / 2u : 0u;
    uint32_t level = 0u, below = 0u, inside = 0u, cum = 0u;
    bool found = false;
    for (uint32_t l = 0; l < MF_LEVELS; l++) {
        if (!found && cum + b[l] > rank) { level = l; below = cum; inside = b[l]; found = true; }
        cum += b[l];
    }
    reinterpret_cast<uint8_t*>(w.high)[4u * k + c] = (uint8_t)level;  // (byte 3 of the word is never read)
    uint32_t* const stat = m.stat + k * MF_STAT + c * 4u;
    stat[0] = below;
    stat[1] = inside;
    stat[2] = n;
}

// One lane an entry: a or b per channel; an entry of the table with pixels moves and gets alpha 255. Leaves the counts
// and the sums zero.
__global__ __launch_bounds__(CF_MAX_TABLE) void mf_move_kernel(Fit w, Machine m, uint32_t entries) {
    const uint32_t k = threadIdx.x, levels = w.high[k], last = (1u << m.bits) - 1u;
    uint32_t picked = 0u, n_k = 0u;
    for (uint32_t c = 0; c < 3u; c++) {
        const uint32_t* const stat = m.stat + k * MF_STAT + c * 4u;
        const long long below = stat[0], inside = stat[1], n = stat[2];
        const long long eq = m.eq[k * 3u + c], sum = (long long)m.sums[k * 3u + c];
        m.eq[k * 3u + c] = 0u;
        m.sums[k * 3u + c] = 0ull;
        const uint32_t l = (levels >> (8u * c)) & 0xFFu, a = widen(m.bits, l);
        uint32_t value = a;
        if (l < last) {
            const long long width = (long long)(widen(m.bits, l + 1u) - a), above = n - below - inside, mid = inside - eq;
            if (width * (below + eq - above) + mid * width - 2 * sum < 0) value = a + (uint32_t)width;
        }
        picked |= value << (8u * c);
        n_k = (uint32_t)n;
    }
    if (k < entries && n_k > 0u) w.table[k] = picked | 0xFF000000u;
}

__global__ __launch_bounds__(CF_MAX_TABLE) void mf_emit_kernel(Fit w, uint32_t entries, PooledEntries from, uint8_t* table_out) {
    const uint32_t k = threadIdx.x;
    if (k < entries) fit_emit(w, k, from.source(k), table_out);
}

// ---- the call --------------------------------------------------------------------------------------------------------

bool machine_args_ok(int sub_size, int depth, int backdrop) {
    return depth >= 0 && depth < MF_DEPTHS && (backdrop == 0 || (backdrop == 1 && sub_size >= 2));
}

template <int CW, int CH>
hipError_t launch_machine_fit(hipStream_t stream, const FitCall& a, int depth, int backdrop) {
    const Geo g = geo_of<CW, CH>(a.width, a.height);
    char* const block = static_cast<char*>(a.work);
    const Machine m = machine_of(block, MF_BITS[depth]);
    const Fit w = fit_of(block + MF_HEAD_BYTES, cells_of(a.width, a.height, CW, CH));
    const uint32_t* fb = reinterpret_cast<const uint32_t*>(a.fb);
    const uint32_t S = (uint32_t)a.n_sub, K = (uint32_t)a.sub_size, N = (uint32_t)a.n_colors;
    const PooledEntries entries{K, backdrop == 1};
    u64* errors = reinterpret_cast<u64*>(a.errors_out);
    const dim3 block_dim(CF_THREADS), all(std::min(g.groups, CF_WALK_GROUPS)), some(std::min(g.groups, CF_TALLY_GROUPS));
    const dim3 one(1), lanes(CF_MAX_TABLE);

    hipLaunchKernelGGL(mf_round_kernel, dim3(MF_LAT / CF_THREADS), block_dim, 0, stream, m, a.palette, N);
    hipError_t e = launch_lists<CW, CH>(stream, a, w, g, m.master);
    if (e == hipSuccess && backdrop == 1) {
        hipLaunchKernelGGL((mf_own_kernel<CW, CH>), all, block_dim, 0, stream, w, fb, g, m.master, N, K);
    }
    if (e == hipSuccess) e = launch_steps<CW, CH>(stream, a, w, g, m.master);
    for (int r = 0; r < a.rounds && e == hipSuccess; r++) {
        u64* const error = errors ? errors + r : nullptr;
        if (m.bits == 8u) {
            hipLaunchKernelGGL((mf_assign_kernel<CW, CH, CF_HI, NibbleTally<false, true, PooledEntries>>), some, block_dim, 0, stream,
                               w, fb, g, a.n_sub, a.sub_size, error, NibbleTally<false, true, PooledEntries>{entries});
            hipLaunchKernelGGL(fit_select_kernel<false>, one, lanes, 0, stream, w, S * K);
            hipLaunchKernelGGL((mf_assign_kernel<CW, CH, CF_LO, NibbleTally<true, true, PooledEntries>>), some, block_dim, 0, stream,
                               w, fb, g, a.n_sub, a.sub_size, nullptr, NibbleTally<true, true, PooledEntries>{entries});
            hipLaunchKernelGGL(fit_select_kernel<true>, one, lanes, 0, stream, w, S * K);
        } else {
            hipLaunchKernelGGL((mf_assign_kernel<CW, CH, CF_HI, LatticeCount>), some, block_dim, 0, stream, w, fb, g, a.n_sub,
                               a.sub_size, error, LatticeCount{entries, m.lat, m.bits});
            hipLaunchKernelGGL(mf_interval_kernel, one, dim3(3 * CF_MAX_TABLE), 0, stream, w, m);
            hipLaunchKernelGGL((mf_assign_kernel<CW, CH, CF_LO, IntervalSum>), some, block_dim, 0, stream, w, fb, g, a.n_sub,
                               a.sub_size, nullptr, IntervalSum{entries, m.eq, m.sums, m.bits});
            hipLaunchKernelGGL(mf_move_kernel, one, lanes, 0, stream, w, m, S * K);
        }
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mf_emit_kernel, one, lanes, 0, stream, w, S * K, entries, a.table_out);
    if (errors) {
        hipLaunchKernelGGL((mf_assign_kernel<CW, CH, CF_ERROR, NibbleTally<false, false, PooledEntries>>),
                           dim3(std::min(g.groups, 4u * CF_TALLY_GROUPS)), block_dim, 0, stream, w, fb, g, a.n_sub, a.sub_size,
                           errors + a.rounds, NibbleTally<false, false, PooledEntries>{entries});
    }
    return hipGetLastError();
}

hipError_t launch_machine_fit(hipStream_t stream, int cell_w, int cell_h, const FitCall& a, int depth, int backdrop) {
    if (cell_w == 8) return cell_h == 8 ? launch_machine_fit<8, 8>(stream, a, depth, backdrop) : launch_machine_fit<8, 16>(stream, a, depth, backdrop);
    return cell_h == 8 ? launch_machine_fit<16, 8>(stream, a, depth, backdrop) : launch_machine_fit<16, 16>(stream, a, depth, backdrop);
}

}  // namespace

extern "C" {

size_t par_machine_round(const uint8_t* palette, int n, int depth, uint8_t* out) {
    if (!palette || !out || n < 1 || n > 256 || depth < 0 || depth >= MF_DEPTHS) return 0;
    for (int i = 0; i < 4 * n; i++) out[i] = (i & 3) == 3 ? palette[i] : (uint8_t)rounded(MF_BITS[depth], palette[i]);
    return 4 * (size_t)n;
}

size_t par_machine_fit_work_bytes(int width, int height, int cell_w, int cell_h) {
    const size_t cells = cells_of(width, height, cell_w, cell_h);
    return cells ? MF_HEAD_BYTES + CF_HEAD_BYTES + CF_BYTES_PER_CELL * cells : 0;
}

int par_machine_fit_device(void* stream, const uint8_t* fb, int width, int height, int cell_w, int cell_h,
                           const uint8_t* palette, int n_colors, int n_sub, int sub_size, int rounds, int depth,
                           int backdrop, void* work, uint8_t* table_out, uint32_t* seeds_out, uint64_t* errors_out) {
    if (!fit_args_ok(fb, width, height, cell_w, cell_h, palette, n_colors, n_sub, sub_size, rounds, table_out) ||
        !machine_args_ok(sub_size, depth, backdrop) || !work || (reinterpret_cast<uintptr_t>(work) & 7u) != 0) {
        return PAR_ERR_INVALID_ARG;
    }
    const FitCall a{fb, width, height, palette, n_colors, n_sub, sub_size, rounds, work, table_out, seeds_out, errors_out};
    return launch_machine_fit((hipStream_t)stream, cell_w, cell_h, a, depth, backdrop) == hipSuccess ? PAR_OK : PAR_ERR_HIP;
}

int par_machine_fit_host(int device, const uint8_t* fb, int width, int height, int cell_w, int cell_h,
                         const uint8_t* palette, int n_colors, int n_sub, int sub_size, int rounds, int depth, int backdrop,
                         uint8_t* table_out, uint32_t* seeds_out, uint64_t* errors_out) {
    if (!fit_args_ok(fb, width, height, cell_w, cell_h, palette, n_colors, n_sub, sub_size, rounds, table_out) ||
        !machine_args_ok(sub_size, depth, backdrop)) {
        return PAR_ERR_INVALID_ARG;
    }
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    par_device_buffer d_fb(e, fb, (size_t)width * (size_t)height * 4, true);
    par_device_buffer d_palette(e, palette, (size_t)n_colors * 4, true);
    par_device_buffer d_work(e, fb, par_machine_fit_work_bytes(width, height, cell_w, cell_h), false);  // (device memory only)
    par_device_buffer d_table(e, table_out, (size_t)n_sub * (size_t)sub_size * 4, false);
    par_device_buffer d_seeds(e, seeds_out, (size_t)n_sub * sizeof(uint32_t), false);
    par_device_buffer d_errors(e, errors_out, (size_t)(rounds + 1) * sizeof(uint64_t), false);
    if (e == hipSuccess) {
        const FitCall a{d_fb.as<uint8_t>(), width, height, d_palette.as<uint8_t>(), n_colors, n_sub, sub_size, rounds,
                        d_work.as<void>(), d_table.as<uint8_t>(), d_seeds.as<uint32_t>(), d_errors.as<uint64_t>()};
        e = launch_machine_fit(nullptr, cell_w, cell_h, a, depth, backdrop);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    d_table.download(table_out);
    if (seeds_out) d_seeds.download(seeds_out);
    if (errors_out) d_errors.download(errors_out);
    return par_status_of(e);
}

}  // extern "C"
