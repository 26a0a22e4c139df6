// par_tileset.hip — tile sets: an index plane deduplicated into its distinct tiles and a tile map
// (par_tileset_build_device, par_tileset_build_host), and the map drawn back into a plane (par_tileset_expand_device,
// par_tileset_expand_host). The contract is beside the declarations in par_tileset.h; nothing here knows a par_context,
// and the statuses are par_raytracer.h's.
//
// A build is six launches on the call's stream. The first, second and last use cells_kernel's layout: a lane holds FOUR
// consecutive bytes of one row of a cell, lane j of a cell the bytes [4j, 4j + 4) of its row-major string, so a cell is
// 16, 32 or 64 lanes and a workgroup of 256 threads takes the 16, 8 or 4 cells side by side in one cell row.
//   hash    every cell's canonical form and f*: the x mirror is the word of the lane whose quad is mirrored, byte-swapped,
//           the y mirror the word of the lane whose row is mirrored (two ds_bpermute each). Two strings compare as their
//           byte-swapped words at the first lane of the cell that differs, which a ballot gives. A 64-bit hash of the
//           canonical form with f* in its two low bits goes to work.hash[c]. The same launch empties the table (a kernel,
//           not a memset node: the call has to be right under graph replay).
//   insert  a cell whose canonical form equals its left neighbour's in the workgroup follows it (a run: background); the
//           heads of the runs look for their class in an open-addressed table of P >= 2N slots that hold a cell number. The hash
//           ONLY PLACES: it says where the probe starts. An empty slot is claimed by compare-and-swap; an occupied one
//           is tested by comparing the BYTES of its cell's canonical form (loaded from the plane under that cell's f*)
//           with one's own, all lanes of the cell at once; equal: atomicMin of one's number, and that only where the
//           slot's number read first is not already lower; different: the next slot. Two different tiles whose hashes
//           collide therefore stay two tiles. A slot's numbers all have the content of the first, and only decrease, so at
//           the end of the launch the slot of a class holds the class's lowest cell number whatever the order of arrival;
//           which slot a class sits in does depend on the order, and nothing reads that.
//   count   flag[c] = (table[slot[c]] == c): the cell is its class's first appearance. A workgroup's 1024 flags are
//           summed (ballots, then the 16 wavefronts' counts through LDS) into work.partial[workgroup].
//   scan    one workgroup: the exclusive prefix sum of the up to 1024 partial sums, and T to count_out.
//   number  the same 1024 flags again; a first appearance's tile number is its workgroup's prefix plus the flags before
//           it in the workgroup. Integers, no atomics: the numbers are those of a host loop over the cells.
//   emit    map_out[c] = number[representative of c] | f* << 30, and a representative whose number is below `capacity`
//           writes its canonical form to tiles_out.
// Expand is one launch in the same layout: a lane gathers its four bytes of the map entry's tile under the entry's flips
// and stores them as one word where the plane's phase allows, else byte by byte.
//
// An extend (par_tileset_extend.h: par_tileset_extend_device, par_tileset_extend_host) is a build whose table holds two
// sources, in eight launches: hash as above; entry, which copies T_in and S = min(T_in, capacity) into the work block
// and empties the slots the hash launch's cells do not reach; stored, which inserts the S stored tiles as the bytes they
// are under the VIRTUAL numbers [0, S); then insert, count, scan, number and emit with cell c numbered capacity + c.
// The stages are the same device functions (insert_forms, count_cells, scan_partials, number_cells, emit_cells), and
// the build's kernels call them with no set and a base of 0. The argument for order independence is the one above: a
// slot's numbers all have the content of the first and only decrease, so a class's slot ends with the lowest virtual
// number of the class, from whichever source and in whatever order they arrived; a stored tile's is below every
// cell's, and the lowest of duplicate stored tiles is the lowest number. Only cells are flagged and counted, and a cell
// whose class a stored tile owns maps to that tile's index.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "par_fastdiv.h"
#include "par_hostcall.h"
#include "par_raytracer.h"
#include "par_tileset.h"
#include "par_tileset_extend.h"

namespace {

constexpr int TS_THREADS = 256;          // the kernels in the cell layout
constexpr int TS_SCAN = 1024;            // cells a workgroup of the count and number kernels, and the partial sums' limit
constexpr uint32_t TS_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t TS_ID_MASK = 0x3FFFFFFFu;
constexpr size_t TS_PARTIAL_BYTES = TS_SCAN * sizeof(uint32_t);
static_assert((size_t)TS_SCAN * TS_SCAN >= PAR_TILESET_MAX_CELLS, "one scan of the partial sums covers every cell");

// What every kernel knows of the call: the plane (of the call's first row), its width, the call's rows and cells.
struct Plane {
    const uint8_t* index;
    uint32_t width, rows, gcx, n_cells, pad;
};

// The parts of the work block (par_tileset_work_bytes).
struct Work {
    uint32_t* partial;  // TS_SCAN sums
    uint64_t* hash;     // a cell: the hash of its canonical form, f* in the two low bits
    uint32_t* rep;      // a cell: its class's slot (insert), then its class's lowest cell number (count)
    uint32_t* number;   // a first appearance: its tile number
    uint32_t* table;    // table_size slots
    uint32_t table_size;
};

uint32_t table_size_of(uint32_t n_cells) {
    uint32_t p = 2;
    while (p < 2 * n_cells) p *= 2;
    return p;
}

// `capacity` is an extend's (par_tileset_extend_work_bytes): its table holds the stored tiles too, and the two words
// after the table are its KeptSet::entry.
Work work_of(void* block, uint32_t n_cells, uint32_t capacity = 0) {
    char* base = static_cast<char*>(block);
    Work w;
    w.partial = reinterpret_cast<uint32_t*>(base);
    w.hash = reinterpret_cast<uint64_t*>(base + TS_PARTIAL_BYTES);
    w.rep = reinterpret_cast<uint32_t*>(base + TS_PARTIAL_BYTES + (size_t)8 * n_cells);
    w.number = w.rep + n_cells;
    w.table = w.number + n_cells;
    w.table_size = table_size_of(n_cells + capacity);
    return w;
}

// The bytes of columns [x0, x0 + 4) of row y of the call's plane as one little-endian word; a byte beyond the width or
// the call's rows is `pad`. One load where the four bytes exist and lie on a word boundary, else a load a byte: the
// plane may begin at any byte and a width that is no multiple of 4 moves every row's phase.
__device__ __forceinline__ uint32_t plane_word(const Plane& g, uint32_t x0, uint32_t y) {
    uint32_t w = g.pad * 0x01010101u;
    if (y >= g.rows || x0 >= g.width) return w;
    const uint8_t* p = g.index + (size_t)y * g.width + x0;
    if (x0 + 4 <= g.width && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) return *reinterpret_cast<const uint32_t*>(p);
    for (uint32_t i = 0; i < 4; i++) {
        if (x0 + i < g.width) w = (w & ~(0xFFu << (8 * i))) | ((uint32_t)p[i] << (8 * i));
    }
    return w;
}

// Four bytes at `p` as one little-endian word, by one load where `aligned` (p on a word boundary), and the store.
__device__ __forceinline__ uint32_t load_word(const uint8_t* p, bool aligned) {
    if (aligned) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ void store_word(uint8_t* p, bool aligned, uint32_t w) {
    if (aligned) {
        *reinterpret_cast<uint32_t*>(p) = w;
    } else {
        for (int i = 0; i < 4; i++) p[i] = (uint8_t)(w >> (8 * i));
    }
}

// Lane j's word of the image of cell (cx, cy) under the flip code f: the x mirror takes the mirrored quad's bytes in
// reverse, the y mirror the mirrored row's.
template <int CW, int CH>
__device__ __forceinline__ uint32_t flipped_word(const Plane& g, uint32_t cx, uint32_t cy, uint32_t f, uint32_t j) {
    constexpr uint32_t QUADS = CW / 4;
    uint32_t r = j / QUADS, q = j % QUADS;
    if (f & 2u) r = CH - 1 - r;
    if (f & 1u) q = QUADS - 1 - q;
    const uint32_t w = plane_word(g, cx * CW + q * 4u, cy * CH + r);
    return (f & 1u) ? __builtin_bswap32(w) : w;
}

// The bits of a ballot that belong to this lane's cell, from bit 0 on.
template <int LANES>
__device__ __forceinline__ uint64_t cell_bits(uint64_t ballot, uint32_t lane) {
    if (LANES == 64) return ballot;
    return (ballot >> (lane & ~(uint32_t)(LANES - 1))) & ((1ull << (LANES & 63)) - 1ull);
}

// The cell's string of words `v` is smaller than that of `best`, bytes compared as unsigned in row-major order: the
// byte-swapped words of the first lane that differs decide. Every lane of the wavefront is active here.
template <int LANES>
__device__ __forceinline__ bool cell_less(uint32_t v, uint32_t best, uint32_t lane) {
    const uint64_t ne = cell_bits<LANES>(__ballot(v != best), lane);
    const int first = (int)(lane & ~(uint32_t)(LANES - 1)) + (ne ? __builtin_ctzll(ne) : 0);
    const uint32_t a = (uint32_t)__shfl((int)__builtin_bswap32(v), first);
    const uint32_t b = (uint32_t)__shfl((int)__builtin_bswap32(best), first);
    return ne != 0 && a < b;
}

__device__ __forceinline__ uint64_t mixed(uint64_t x) {
    x *= 0x9E3779B97F4A7C15ull;
    x ^= x >> 32;
    x *= 0xD6E8FEB86659FD93ull;
    x ^= x >> 32;
    return x;
}

// The hash of a form whose lane j holds `word`: a sum over the lanes of a mix of (position, word), so any order of the
// lanes gives the same sum. Every lane of the wavefront is active here.
template <int LANES>
__device__ __forceinline__ uint64_t form_hash(uint32_t word, uint32_t j) {
    uint64_t h = mixed(((uint64_t)(j + 1u) << 32) | word);
    for (int m = 1; m < LANES; m <<= 1) h += (uint64_t)__shfl_xor((unsigned long long)h, m);
    return mixed(h);
}

// blockIdx.y is the cell row within the launch, cy0 the launch's first cell row within the call; blockIdx.x the group of
// CELLS cells. A cell of the group past gcx computes on `pad` and stores nothing.
template <int CW, int CH>
__global__ __launch_bounds__(TS_THREADS) void tileset_hash_kernel(Plane g, uint32_t cy0, uint32_t flips, Work w) {
    static_assert((CW == 8 || CW == 16) && (CH == 8 || CH == 16), "a cell is 1, 2 or 4 rows of 16 lanes");
    constexpr int LANES = CW * CH / 4, QUADS = CW / 4, CELLS = TS_THREADS / LANES;
    const uint32_t t = threadIdx.x, lane = t & 63u, j = t % LANES;
    const uint32_t cx = blockIdx.x * (uint32_t)CELLS + t / LANES, cy = cy0 + blockIdx.y;
    const uint32_t own = plane_word(g, cx * CW + (j % QUADS) * 4u, cy * CH + j / QUADS);

    // the smallest image, the lowest code among equals: the codes in ascending order, replaced only by a smaller one
    // (`flips` is a kernel argument: all 64 lanes reach every cross-lane step)
    uint32_t best = own, f_star = 0;
    if (flips & 1u) {
        const uint32_t v = __builtin_bswap32((uint32_t)__shfl_xor((int)own, QUADS - 1));
        const bool less = cell_less<LANES>(v, best, lane);
        best = less ? v : best;
        f_star = less ? 1u : f_star;
    }
    if (flips & 2u) {
        const uint32_t v = (uint32_t)__shfl_xor((int)own, (CH - 1) * QUADS);
        const bool less = cell_less<LANES>(v, best, lane);
        best = less ? v : best;
        f_star = less ? 2u : f_star;
    }
    if (flips == 3u) {
        const uint32_t up = (uint32_t)__shfl_xor((int)own, (CH - 1) * QUADS);
        const uint32_t v = __builtin_bswap32((uint32_t)__shfl_xor((int)up, QUADS - 1));
        const bool less = cell_less<LANES>(v, best, lane);
        best = less ? v : best;
        f_star = less ? 3u : f_star;
    }

    const uint64_t h = form_hash<LANES>(best, j);

    if (cx >= g.gcx) return;
    const uint32_t c = cx + cy * g.gcx;
    if (j == 0) w.hash[c] = (h & ~3ull) | f_star;
    // the table's slots [4c, 4c + 4): table_size < 4 * n_cells, so the cells cover it
    if (j < 4 && 4u * c + j < w.table_size) w.table[4u * c + j] = TS_EMPTY;
}

// The kept set of an extend (par_tileset_extend.h). The table then holds VIRTUAL numbers: stored tile i is i, cell c of
// the call is capacity + c, so "a slot holds the lowest number of its class" puts a stored tile before every cell and
// the lowest of duplicate stored tiles first. `entry` is the pair the first launch copies into the work block:
// entry[0] = T_in, entry[1] = S. A build has no set: its virtual numbers are its cell numbers.
struct KeptSet {
    uint8_t* tiles;
    uint32_t capacity;
    const uint32_t* entry;
};
struct NoSet {};
__device__ __forceinline__ uint32_t first_cell_number(const NoSet&) { return 0u; }
__device__ __forceinline__ uint32_t first_cell_number(const KeptSet& s) { return s.capacity; }

// Lane j's word of the form that owns virtual number `seen`: a stored tile as it is, a cell under its f*.
template <int CW, int CH, class Set>
__device__ __forceinline__ uint32_t owner_word(const Plane& g, par_udiv31 by_gcx, const Work& w, const Set& set, uint32_t seen,
                                               uint32_t j) {
    if constexpr (std::is_same<Set, KeptSet>::value) {
        if (seen < set.capacity) {
            return load_word(set.tiles + (size_t)seen * (CW * CH) + 4u * j, (reinterpret_cast<uintptr_t>(set.tiles) & 3u) == 0);
        }
        seen -= set.capacity;
    }
    const uint32_t scy = par_udiv31_quotient(seen, by_gcx), scx = seen - scy * g.gcx;
    return flipped_word<CW, CH>(g, scx, scy, (uint32_t)w.hash[seen] & 3u, j);
}

// The insert of the forms a workgroup holds, one a group of LANES lanes: the form `mine` (lane j's word) with the hash
// h and the virtual number v, where `exists`. CELL: the form is cell c of the call and w.rep[c] takes its slot; else it
// is a stored tile, which nothing looks up afterwards.
template <int CW, int CH, bool CELL, class Set>
__device__ __forceinline__ void insert_forms(const Plane& g, par_udiv31 by_gcx, const Work& w, const Set& set, bool exists,
                                             uint32_t v, uint32_t c, uint64_t h, uint32_t mine) {
    constexpr int LANES = CW * CH / 4, CELLS = TS_THREADS / LANES;
    const uint32_t t = threadIdx.x, lane = t & 63u, j = t % LANES;
    const int leader_lane = (int)(lane & ~(uint32_t)(LANES - 1));
    const bool leader = j == 0;
    const uint32_t mask = w.table_size - 1u;

    // Runs first: a real frame is mostly background, and every cell of it would read the one slot of its class, which is
    // the many-on-one-address shape that is slow whatever the operation. A cell whose canonical form equals, byte for
    // byte, that of its left neighbour in the workgroup FOLLOWS it; only the first cell of a run, its head, goes to the
    // table, and the followers take the head's slot afterwards. The head has the run's lowest number, so the slot's
    // minimum is what it would have been.
    __shared__ uint32_t words[TS_THREADS];
    __shared__ uint32_t run_slot[CELLS];
    __shared__ uint32_t follows[CELLS];
    const uint32_t cell = t / LANES;
    words[t] = mine;
    __syncthreads();
    const bool differs_left = cell == 0 || words[t - LANES] != mine;
    const bool follows_left = cell_bits<LANES>(__ballot(differs_left), lane) == 0;  // (never for cell 0)
    if (leader) follows[cell] = follows_left ? 1u : 0u;
    __syncthreads();
    uint32_t head = cell;
    while (follows[head]) head--;
    const bool is_head = head == cell;

    // The loop is the wavefront's: every lane stays in it until every cell of the wavefront is done, so that the
    // cross-lane steps always see 64 active lanes. A cell that is done takes no part in the atomics or the loads.
    uint32_t slot = (uint32_t)(h >> 32) & mask;
    bool done = !exists || !is_head;
    while (__ballot(!done) != 0) {
        // the slot's cell number: the one found there, or one's own where the slot was empty and the claim succeeded
        uint32_t seen = v;
        if (leader && !done) {
            seen = __hip_atomic_load(&w.table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (seen == TS_EMPTY) {
                uint32_t expected = TS_EMPTY;
                const bool claimed = __hip_atomic_compare_exchange_strong(&w.table[slot], &expected, v, __ATOMIC_RELAXED,
                                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                seen = claimed ? v : expected;
            }
        }
        seen = (uint32_t)__shfl((int)seen, leader_lane);
        // EQUALITY IS DECIDED BY BYTES: the slot's owner's form against one's own, word by word
        bool differs = false;
        if (!done && seen != v) differs = owner_word<CW, CH>(g, by_gcx, w, set, seen, j) != mine;
        const bool other_tile = cell_bits<LANES>(__ballot(differs), lane) != 0;
        if (!done) {
            if (other_tile) {
                slot = (slot + 1u) & mask;
            } else {
                if (leader) {
                    // (the number read first: no atomic on a slot that already holds a lower one)
                    if (seen > v) __hip_atomic_fetch_min(&w.table[slot], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (CELL) w.rep[c] = slot;
                    run_slot[cell] = slot;
                }
                done = true;
            }
        }
    }
    if (!CELL) return;
    __syncthreads();
    if (exists && !is_head && leader) w.rep[c] = run_slot[head];
}

// The call's cells into the table. A build's set is NoSet; an extend's is its KeptSet, whose stored tiles are in the
// table already (tileset_stored_insert_kernel, the launch before).
template <int CW, int CH, class Set>
__device__ __forceinline__ void insert_cells(const Plane& g, uint32_t cy0, par_udiv31 by_gcx, const Work& w, const Set& set) {
    constexpr int LANES = CW * CH / 4, CELLS = TS_THREADS / LANES;
    const uint32_t t = threadIdx.x, j = t % LANES;
    const uint32_t cx = blockIdx.x * (uint32_t)CELLS + t / LANES, cy = cy0 + blockIdx.y;
    const bool exists = cx < g.gcx;
    const uint32_t c = cx + cy * g.gcx;
    const uint64_t h = exists ? w.hash[c] : 0ull;
    const uint32_t mine = flipped_word<CW, CH>(g, cx, cy, (uint32_t)h & 3u, j);
    insert_forms<CW, CH, true>(g, by_gcx, w, set, exists, first_cell_number(set) + c, c, h, mine);
}

template <int CW, int CH>
__global__ __launch_bounds__(TS_THREADS) void tileset_insert_kernel(Plane g, uint32_t cy0, par_udiv31 by_gcx, Work w) {
    insert_cells<CW, CH>(g, cy0, by_gcx, w, NoSet{});
}

template <int CW, int CH>
__global__ __launch_bounds__(TS_THREADS) void tileset_extend_insert_kernel(Plane g, uint32_t cy0, par_udiv31 by_gcx, Work w,
                                                                           KeptSet set) {
    insert_cells<CW, CH>(g, cy0, by_gcx, w, set);
}

// The stored tiles into the table, as the bytes they are: no mirrors, code 0, the lane layout and the hash of a cell's
// canonical form, so that equal bytes start their probe at the same slot. The launch is sized by `capacity`; S is a
// device value, and a workgroup at or beyond it leaves after reading it. blockIdx.x is the group of CELLS stored tiles.
// Only stored tiles are in the table during this launch (it follows the launches that empty it and precedes the
// cells'), so every owner met here is a stored tile; owner_word would serve a cell as well.
template <int CW, int CH>
__global__ __launch_bounds__(TS_THREADS) void tileset_stored_insert_kernel(Plane g, par_udiv31 by_gcx, Work w, KeptSet set) {
    constexpr int LANES = CW * CH / 4, CELLS = TS_THREADS / LANES;
    const uint32_t stored = set.entry[1];
    if (blockIdx.x * (uint32_t)CELLS >= stored) return;  // (the whole workgroup)
    const uint32_t t = threadIdx.x, j = t % LANES, i = blockIdx.x * (uint32_t)CELLS + t / LANES;
    const bool exists = i < stored;
    const uint32_t mine =
        exists ? load_word(set.tiles + (size_t)i * (CW * CH) + 4u * j, (reinterpret_cast<uintptr_t>(set.tiles) & 3u) == 0) : 0u;
    const uint64_t h = form_hash<LANES>(mine, j);
    insert_forms<CW, CH, false>(g, by_gcx, w, set, exists, i, 0u, h, mine);
}

// The first launch of an extend's own: T_in and S into the work block, where every later launch reads them (the scan
// overwrites *count), T_in to first_new_out, and the slots of the table the hash launch's cells do not reach emptied
// (a kernel, not a memcpy or memset node with a baked-in value: the call has to be right under graph replay).
__global__ __launch_bounds__(TS_THREADS) void tileset_entry_kernel(Work w, uint32_t first_slot, const uint32_t* count,
                                                                   uint32_t capacity, uint32_t* entry, uint32_t* first_new_out) {
    const uint32_t slot = first_slot + blockIdx.x * (uint32_t)TS_THREADS + threadIdx.x;
    if (slot < w.table_size) w.table[slot] = TS_EMPTY;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t t_in = *count;
        entry[0] = t_in;
        entry[1] = std::min(t_in, capacity);
        if (first_new_out) *first_new_out = t_in;
    }
}

// The flags of the TS_SCAN cells of a workgroup: the count before this thread within the workgroup, and (in every
// thread) the workgroup's count.
__device__ __forceinline__ uint32_t flags_before(bool flag, uint32_t& total) {
    __shared__ uint32_t waves[TS_SCAN / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64u;
    const uint64_t ballot = __ballot(flag);
    if (lane == 0) waves[wave] = (uint32_t)__builtin_popcountll(ballot);
    __syncthreads();
    uint32_t before = (uint32_t)__builtin_popcountll(ballot & ((1ull << lane) - 1ull));
    total = 0;
    for (uint32_t i = 0; i < TS_SCAN / 64; i++) {
        before += i < wave ? waves[i] : 0u;
        total += waves[i];
    }
    return before;
}

// The four stages after the inserts, for a build and for an extend. `base` is the virtual number of cell 0 (0 in a
// build, `capacity` in an extend) and `first` the number the first new tile takes (0, T_in): only the call's own cells
// are flagged, counted and scanned, and a first appearance is a cell whose class's lowest virtual number is its own.
__device__ __forceinline__ void count_cells(const Work& w, uint32_t n_cells, uint32_t base) {
    const uint32_t c = blockIdx.x * (uint32_t)TS_SCAN + threadIdx.x;
    bool flag = false;
    if (c < n_cells) {
        const uint32_t lowest = w.table[w.rep[c]];
        w.rep[c] = lowest;
        flag = lowest == base + c;
    }
    uint32_t total;
    (void)flags_before(flag, total);
    if (threadIdx.x == 0) w.partial[blockIdx.x] = total;
}

__device__ __forceinline__ void scan_partials(const Work& w, uint32_t n_partials, uint32_t first, uint32_t* count_out) {
    __shared__ uint32_t sums[TS_SCAN];
    const uint32_t t = threadIdx.x, own = t < n_partials ? w.partial[t] : 0u;
    sums[t] = own;
    __syncthreads();
    for (uint32_t step = 1; step < TS_SCAN; step *= 2) {
        const uint32_t add = t >= step ? sums[t - step] : 0u;
        __syncthreads();
        sums[t] += add;
        __syncthreads();
    }
    if (t < n_partials) w.partial[t] = sums[t] - own;
    if (t == TS_SCAN - 1) *count_out = first + sums[t];
}

__device__ __forceinline__ void number_cells(const Work& w, uint32_t n_cells, uint32_t base, uint32_t first) {
    const uint32_t c = blockIdx.x * (uint32_t)TS_SCAN + threadIdx.x;
    const bool flag = c < n_cells && w.rep[c] == base + c;
    uint32_t total;
    const uint32_t before = flags_before(flag, total);
    if (flag) w.number[c] = first + w.partial[blockIdx.x] + before;
}

// EXTEND: a class a stored tile owns takes that tile's index and writes nothing; a new tile's number is kept to the
// map's 30 bits, and a number that wrapped round 2^32 (the caller's T_in + N is to stay below 2^30) stores no tile.
template <int CW, int CH, bool EXTEND>
__device__ __forceinline__ void emit_cells(const Plane& g, uint32_t cy0, const Work& w, uint8_t* tiles, uint32_t capacity,
                                           uint32_t* map, uint32_t base, uint32_t first) {
    constexpr int LANES = CW * CH / 4, CELLS = TS_THREADS / LANES;
    const uint32_t t = threadIdx.x, j = t % LANES;
    const uint32_t cx = blockIdx.x * (uint32_t)CELLS + t / LANES, cy = cy0 + blockIdx.y;
    if (cx >= g.gcx) return;
    const uint32_t c = cx + cy * g.gcx, lowest = w.rep[c], f = (uint32_t)w.hash[c] & 3u;
    const uint32_t id = EXTEND && lowest < base ? lowest : w.number[lowest - base];
    if (map && j == 0) map[c] = (EXTEND ? id & TS_ID_MASK : id) | (f << 30);
    if (lowest == base + c && id < capacity && (!EXTEND || id >= first)) {
        uint8_t* out = tiles + (size_t)id * (CW * CH) + 4u * j;
        store_word(out, (reinterpret_cast<uintptr_t>(tiles) & 3u) == 0, flipped_word<CW, CH>(g, cx, cy, f, j));
    }
}

__global__ __launch_bounds__(TS_SCAN) void tileset_count_kernel(Work w, uint32_t n_cells) { count_cells(w, n_cells, 0u); }

__global__ __launch_bounds__(TS_SCAN) void tileset_scan_kernel(Work w, uint32_t n_partials, uint32_t* count_out) {
    scan_partials(w, n_partials, 0u, count_out);
}

__global__ __launch_bounds__(TS_SCAN) void tileset_number_kernel(Work w, uint32_t n_cells) { number_cells(w, n_cells, 0u, 0u); }

template <int CW, int CH>
__global__ __launch_bounds__(TS_THREADS) void tileset_emit_kernel(Plane g, uint32_t cy0, Work w, uint8_t* tiles,
                                                                  uint32_t capacity, uint32_t* map) {
    emit_cells<CW, CH, false>(g, cy0, w, tiles, capacity, map, 0u, 0u);
}

__global__ __launch_bounds__(TS_SCAN) void tileset_extend_count_kernel(Work w, uint32_t n_cells, KeptSet set) {
    count_cells(w, n_cells, set.capacity);
}

__global__ __launch_bounds__(TS_SCAN) void tileset_extend_scan_kernel(Work w, uint32_t n_partials, KeptSet set, uint32_t* count) {
    scan_partials(w, n_partials, set.entry[0], count);
}

__global__ __launch_bounds__(TS_SCAN) void tileset_extend_number_kernel(Work w, uint32_t n_cells, KeptSet set) {
    number_cells(w, n_cells, set.capacity, set.entry[0]);
}

template <int CW, int CH>
__global__ __launch_bounds__(TS_THREADS) void tileset_extend_emit_kernel(Plane g, uint32_t cy0, Work w, KeptSet set,
                                                                         uint32_t* map) {
    emit_cells<CW, CH, true>(g, cy0, w, set.tiles, set.capacity, map, set.capacity, set.entry[0]);
}

// g.index is unused here: `out` is the plane. A lane draws the four pixels of its quad.
template <int CW, int CH>
__global__ __launch_bounds__(TS_THREADS) void tileset_expand_kernel(Plane g, uint32_t cy0, const uint8_t* tiles,
                                                                    uint32_t n_tiles, const uint32_t* map, uint8_t* out) {
    constexpr int LANES = CW * CH / 4, QUADS = CW / 4, CELLS = TS_THREADS / LANES;
    const uint32_t t = threadIdx.x, j = t % LANES;
    const uint32_t cx = blockIdx.x * (uint32_t)CELLS + t / LANES, cy = cy0 + blockIdx.y;
    const uint32_t x0 = cx * CW + (j % QUADS) * 4u, y = cy * CH + j / QUADS;
    if (x0 >= g.width || y >= g.rows) return;
    const uint32_t entry = map[cx + cy * g.gcx], id = std::min(entry & TS_ID_MASK, n_tiles - 1u), f = entry >> 30;
    uint32_t r = j / QUADS, q = j % QUADS;
    if (f & 2u) r = CH - 1 - r;
    if (f & 1u) q = QUADS - 1 - q;
    uint32_t v = load_word(tiles + (size_t)id * (CW * CH) + r * CW + q * 4u, (reinterpret_cast<uintptr_t>(tiles) & 3u) == 0);
    if (f & 1u) v = __builtin_bswap32(v);
    uint8_t* p = out + (size_t)y * g.width + x0;
    if (x0 + 4 <= g.width) {
        store_word(p, (reinterpret_cast<uintptr_t>(p) & 3u) == 0, v);
    } else {
        for (uint32_t i = 0; x0 + i < g.width; i++) p[i] = (uint8_t)(v >> (8 * i));
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------

// The geometry every call checks: the tile size, the width, the rows and their cut, and the cell count.
bool geometry_ok(const par_params* p, int tile_w, int tile_h, int row_begin, int row_end) {
    if (!p || (tile_w != 8 && tile_w != 16) || (tile_h != 8 && tile_h != 16)) return false;
    if (p->width <= 0 || row_begin < 0 || row_begin >= row_end || row_end > p->height) return false;
    if (row_begin % tile_h != 0 || (row_end % tile_h != 0 && row_end != p->height)) return false;
    const int64_t gcx = ((int64_t)p->width + tile_w - 1) / tile_w, gcy = ((int64_t)(row_end - row_begin) + tile_h - 1) / tile_h;
    return gcx * gcy <= PAR_TILESET_MAX_CELLS;
}

Plane plane_of(const par_params* p, const uint8_t* index, int tile_w, int tile_h, int row_begin, int row_end, int pad) {
    Plane g;
    g.index = index;
    g.width = (uint32_t)p->width;
    g.rows = (uint32_t)(row_end - row_begin);
    g.gcx = (g.width + (uint32_t)tile_w - 1u) / (uint32_t)tile_w;
    g.n_cells = g.gcx * ((g.rows + (uint32_t)tile_h - 1u) / (uint32_t)tile_h);
    g.pad = (uint32_t)pad;
    return g;
}

bool build_args_ok(const par_params* p, const uint8_t* index, int row_begin, int row_end, int tile_w, int tile_h, int pad,
                   int flips, const uint8_t* tiles_out, int capacity, const void* count_out) {
    if (!geometry_ok(p, tile_w, tile_h, row_begin, row_end) || !index || !count_out) return false;
    if (capacity < 0 || (capacity > 0 && !tiles_out)) return false;
    return pad >= 0 && pad <= 255 && flips >= 0 && flips <= 3;
}

bool expand_args_ok(const par_params* p, const uint8_t* tiles, int n_tiles, int tile_w, int tile_h, const uint32_t* map,
                    int row_begin, int row_end, const uint8_t* index_out) {
    return geometry_ok(p, tile_w, tile_h, row_begin, row_end) && tiles && map && index_out && n_tiles >= 1;
}

// fn(std::integral_constant<int, CW>, std::integral_constant<int, CH>) for the tile size of the call
template <class Fn>
hipError_t with_tile(int tile_w, int tile_h, Fn fn) {
    using I8 = std::integral_constant<int, 8>;
    using I16 = std::integral_constant<int, 16>;
    if (tile_w == 8) return tile_h == 8 ? fn(I8{}, I8{}) : fn(I8{}, I16{});
    return tile_h == 8 ? fn(I16{}, I8{}) : fn(I16{}, I16{});
}

// One launch a cut of the call's cell rows (par_tile_row_cuts: one launch for up to 65535 cell rows) of a kernel in the
// cell layout: launch(grid, cy0) with cy0 the cut's first cell row within the call.
template <int CW, int CH, class Launch>
hipError_t cell_launches(const Plane& g, Launch launch) {
    constexpr uint32_t CELLS = TS_THREADS / (CW * CH / 4);
    return (hipError_t)par_tile_row_cuts(0, (int)g.rows, g.width, CH, [&](int ra, int, uint32_t cell_rows) {
        launch(dim3((g.gcx + CELLS - 1) / CELLS, cell_rows), (uint32_t)ra / CH);
        return (int)hipGetLastError();
    });
}

hipError_t launch_build(hipStream_t stream, const Plane& g, int tile_w, int tile_h, int flips, void* work_block,
                        uint8_t* tiles_out, int capacity, uint32_t* map_out, uint32_t* count_out) {
    const Work w = work_of(work_block, g.n_cells);
    const uint32_t n_partials = (g.n_cells + TS_SCAN - 1) / TS_SCAN;
    return with_tile(tile_w, tile_h, [&](auto cw, auto ch) {
        constexpr int CW = decltype(cw)::value, CH = decltype(ch)::value;
        hipError_t e = cell_launches<CW, CH>(g, [&](dim3 grid, uint32_t cy0) {
            hipLaunchKernelGGL((tileset_hash_kernel<CW, CH>), grid, dim3(TS_THREADS), 0, stream, g, cy0, (uint32_t)flips, w);
        });
        if (e != hipSuccess) return e;
        e = cell_launches<CW, CH>(g, [&](dim3 grid, uint32_t cy0) {
            hipLaunchKernelGGL((tileset_insert_kernel<CW, CH>), grid, dim3(TS_THREADS), 0, stream, g, cy0,
                               par_udiv31_make(g.gcx), w);
        });
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(tileset_count_kernel, dim3(n_partials), dim3(TS_SCAN), 0, stream, w, g.n_cells);
        hipLaunchKernelGGL(tileset_scan_kernel, dim3(1), dim3(TS_SCAN), 0, stream, w, n_partials, count_out);
        if ((e = hipGetLastError()) != hipSuccess || (!map_out && capacity == 0)) return e;
        hipLaunchKernelGGL(tileset_number_kernel, dim3(n_partials), dim3(TS_SCAN), 0, stream, w, g.n_cells);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        return cell_launches<CW, CH>(g, [&](dim3 grid, uint32_t cy0) {
            hipLaunchKernelGGL((tileset_emit_kernel<CW, CH>), grid, dim3(TS_THREADS), 0, stream, g, cy0, w, tiles_out,
                               (uint32_t)capacity, map_out);
        });
    });
}

// An extend: the hash launch as a build's (it empties the table's first 4N slots), the entry launch (T_in, S and the rest
// of the table), the stored tiles' insert, sized by `capacity`, then a build's stages on virtual numbers.
hipError_t launch_extend(hipStream_t stream, const Plane& g, int tile_w, int tile_h, int flips, void* work_block, uint8_t* tiles,
                         int capacity, uint32_t* count, uint32_t* map_out, uint32_t* first_new_out) {
    const Work w = work_of(work_block, g.n_cells, (uint32_t)capacity);
    uint32_t* entry = w.table + w.table_size;
    const KeptSet set{tiles, (uint32_t)capacity, entry};
    const uint32_t n_partials = (g.n_cells + TS_SCAN - 1) / TS_SCAN;
    const uint32_t first_slot = std::min(4u * g.n_cells, w.table_size);
    const uint32_t entry_groups = std::max(1u, (w.table_size - first_slot + TS_THREADS - 1) / TS_THREADS);
    const par_udiv31 by_gcx = par_udiv31_make(g.gcx);
    return with_tile(tile_w, tile_h, [&](auto cw, auto ch) {
        constexpr int CW = decltype(cw)::value, CH = decltype(ch)::value;
        constexpr uint32_t CELLS = TS_THREADS / (CW * CH / 4);
        hipError_t e = cell_launches<CW, CH>(g, [&](dim3 grid, uint32_t cy0) {
            hipLaunchKernelGGL((tileset_hash_kernel<CW, CH>), grid, dim3(TS_THREADS), 0, stream, g, cy0, (uint32_t)flips, w);
        });
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(tileset_entry_kernel, dim3(entry_groups), dim3(TS_THREADS), 0, stream, w, first_slot, count,
                           (uint32_t)capacity, entry, first_new_out);
        if (capacity > 0) {
            hipLaunchKernelGGL((tileset_stored_insert_kernel<CW, CH>), dim3(((uint32_t)capacity + CELLS - 1) / CELLS),
                               dim3(TS_THREADS), 0, stream, g, by_gcx, w, set);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        e = cell_launches<CW, CH>(g, [&](dim3 grid, uint32_t cy0) {
            hipLaunchKernelGGL((tileset_extend_insert_kernel<CW, CH>), grid, dim3(TS_THREADS), 0, stream, g, cy0, by_gcx, w, set);
        });
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(tileset_extend_count_kernel, dim3(n_partials), dim3(TS_SCAN), 0, stream, w, g.n_cells, set);
        hipLaunchKernelGGL(tileset_extend_scan_kernel, dim3(1), dim3(TS_SCAN), 0, stream, w, n_partials, set, count);
        if ((e = hipGetLastError()) != hipSuccess || (!map_out && capacity == 0)) return e;
        hipLaunchKernelGGL(tileset_extend_number_kernel, dim3(n_partials), dim3(TS_SCAN), 0, stream, w, g.n_cells, set);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        return cell_launches<CW, CH>(g, [&](dim3 grid, uint32_t cy0) {
            hipLaunchKernelGGL((tileset_extend_emit_kernel<CW, CH>), grid, dim3(TS_THREADS), 0, stream, g, cy0, w, set, map_out);
        });
    });
}

hipError_t launch_expand(hipStream_t stream, const Plane& g, int tile_w, int tile_h, const uint8_t* tiles, int n_tiles,
                         const uint32_t* map, uint8_t* index_out) {
    return with_tile(tile_w, tile_h, [&](auto cw, auto ch) {
        constexpr int CW = decltype(cw)::value, CH = decltype(ch)::value;
        return cell_launches<CW, CH>(g, [&](dim3 grid, uint32_t cy0) {
            hipLaunchKernelGGL((tileset_expand_kernel<CW, CH>), grid, dim3(TS_THREADS), 0, stream, g, cy0, tiles,
                               (uint32_t)n_tiles, map, index_out);
        });
    });
}

}  // namespace

extern "C" {

size_t par_tileset_work_bytes(int n_cells) {
    if (n_cells < 1 || n_cells > PAR_TILESET_MAX_CELLS) return 0;
    return TS_PARTIAL_BYTES + (size_t)16 * (size_t)n_cells + (size_t)4 * table_size_of((uint32_t)n_cells);
}

int par_tileset_build_device(const par_params* params, void* stream, const uint8_t* index, int row_begin, int row_end,
                             int tile_w, int tile_h, int pad, int flips, void* work, uint8_t* tiles_out, int capacity,
                             uint32_t* map_out, uint32_t* count_out) {
    if (!build_args_ok(params, index, row_begin, row_end, tile_w, tile_h, pad, flips, tiles_out, capacity, count_out) ||
        !work || (reinterpret_cast<uintptr_t>(work) & 7u) != 0) {
        return PAR_ERR_INVALID_ARG;
    }
    const Plane g = plane_of(params, index, tile_w, tile_h, row_begin, row_end, pad);
    return launch_build((hipStream_t)stream, g, tile_w, tile_h, flips, work, tiles_out, capacity, map_out, count_out) == hipSuccess
               ? PAR_OK
               : PAR_ERR_HIP;
}

int par_tileset_expand_device(const par_params* params, void* stream, const uint8_t* tiles, int n_tiles, int tile_w,
                              int tile_h, const uint32_t* map, int row_begin, int row_end, uint8_t* index_out) {
    if (!expand_args_ok(params, tiles, n_tiles, tile_w, tile_h, map, row_begin, row_end, index_out)) return PAR_ERR_INVALID_ARG;
    const Plane g = plane_of(params, nullptr, tile_w, tile_h, row_begin, row_end, 0);
    return launch_expand((hipStream_t)stream, g, tile_w, tile_h, tiles, n_tiles, map, index_out) == hipSuccess ? PAR_OK
                                                                                                               : PAR_ERR_HIP;
}

int par_tileset_build_host(const par_params* params, int device, const uint8_t* index, int row_begin, int row_end,
                           int tile_w, int tile_h, int pad, int flips, uint8_t* tiles_out, int capacity, uint32_t* map_out,
                           int* count_out) {
    if (!build_args_ok(params, index, row_begin, row_end, tile_w, tile_h, pad, flips, tiles_out, capacity, count_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    Plane g = plane_of(params, nullptr, tile_w, tile_h, row_begin, row_end, pad);
    uint32_t count = 0;
    const size_t tile_bytes = (size_t)capacity * (size_t)(tile_w * tile_h);
    par_device_buffer d_index(e, index, (size_t)g.rows * g.width, true);
    par_device_buffer d_work(e, &count, par_tileset_work_bytes((int)g.n_cells), false);  // (device memory only)
    par_device_buffer d_tiles(e, tiles_out, tile_bytes, true);  // (the tiles from T on keep the caller's bytes)
    par_device_buffer d_map(e, map_out, (size_t)g.n_cells * sizeof(uint32_t), false);
    par_device_buffer d_count(e, &count, sizeof(count), false);
    if (e == hipSuccess) {
        g.index = d_index.as<uint8_t>();
        e = launch_build(nullptr, g, tile_w, tile_h, flips, d_work.as<void>(), d_tiles.as<uint8_t>(), capacity,
                         d_map.as<uint32_t>(), d_count.as<uint32_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    d_tiles.download(tiles_out);
    d_map.download(map_out);
    d_count.download(&count);
    if (e == hipSuccess) *count_out = (int)count;
    return par_status_of(e);
}

int par_tileset_expand_host(const par_params* params, int device, const uint8_t* tiles, int n_tiles, int tile_w,
                            int tile_h, const uint32_t* map, int row_begin, int row_end, uint8_t* index_out) {
    if (!expand_args_ok(params, tiles, n_tiles, tile_w, tile_h, map, row_begin, row_end, index_out)) return PAR_ERR_INVALID_ARG;
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    const Plane g = plane_of(params, nullptr, tile_w, tile_h, row_begin, row_end, 0);
    par_device_buffer d_tiles(e, tiles, (size_t)n_tiles * (size_t)(tile_w * tile_h), true);
    par_device_buffer d_map(e, map, (size_t)g.n_cells * sizeof(uint32_t), true);
    par_device_buffer d_index(e, index_out, (size_t)g.rows * g.width, false);
    if (e == hipSuccess) {
        e = launch_expand(nullptr, g, tile_w, tile_h, d_tiles.as<uint8_t>(), n_tiles, d_map.as<uint32_t>(), d_index.as<uint8_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    d_index.download(index_out);
    return par_status_of(e);
}

// ---- par_tileset_extend.h ---------------------------------------------------------------------------------------------

size_t par_tileset_extend_work_bytes(int n_cells, int capacity) {
    if (n_cells < 1 || n_cells > PAR_TILESET_MAX_CELLS || capacity < 0 || capacity > PAR_TILESET_MAX_CELLS) return 0;
    return TS_PARTIAL_BYTES + (size_t)16 * (size_t)n_cells + (size_t)4 * table_size_of((uint32_t)n_cells + (uint32_t)capacity) +
           2 * sizeof(uint32_t);
}

int par_tileset_extend_device(const par_params* params, void* stream, const uint8_t* index, int row_begin, int row_end,
                              int tile_w, int tile_h, int pad, int flips, void* work, uint8_t* tiles, int capacity,
                              uint32_t* count, uint32_t* map_out, uint32_t* first_new_out) {
    if (!build_args_ok(params, index, row_begin, row_end, tile_w, tile_h, pad, flips, tiles, capacity, count) ||
        capacity > PAR_TILESET_MAX_CELLS || !work || (reinterpret_cast<uintptr_t>(work) & 7u) != 0) {
        return PAR_ERR_INVALID_ARG;
    }
    const Plane g = plane_of(params, index, tile_w, tile_h, row_begin, row_end, pad);
    return launch_extend((hipStream_t)stream, g, tile_w, tile_h, flips, work, tiles, capacity, count, map_out, first_new_out) ==
                   hipSuccess
               ? PAR_OK
               : PAR_ERR_HIP;
}

int par_tileset_extend_host(const par_params* params, int device, const uint8_t* index, int row_begin, int row_end,
                            int tile_w, int tile_h, int pad, int flips, uint8_t* tiles, int capacity, int* count,
                            uint32_t* map_out, int* first_new_out) {
    if (!build_args_ok(params, index, row_begin, row_end, tile_w, tile_h, pad, flips, tiles, capacity, count) ||
        capacity > PAR_TILESET_MAX_CELLS || *count < 0) {
        return PAR_ERR_INVALID_ARG;
    }
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    Plane g = plane_of(params, nullptr, tile_w, tile_h, row_begin, row_end, pad);
    uint32_t t_in = (uint32_t)*count, t_out = t_in, first_new = t_in;
    const size_t tile_bytes = (size_t)(tile_w * tile_h);
    par_device_buffer d_index(e, index, (size_t)g.rows * g.width, true);
    par_device_buffer d_work(e, &t_in, par_tileset_extend_work_bytes((int)g.n_cells, capacity), false);  // (device memory only)
    par_device_buffer d_tiles(e, tiles, (size_t)capacity * tile_bytes, false);  // (only the stored tiles go up, below)
    par_device_buffer d_map(e, map_out, (size_t)g.n_cells * sizeof(uint32_t), false);
    par_device_buffer d_count(e, &t_in, sizeof(t_in), true);
    par_device_buffer d_first(e, &first_new, sizeof(first_new), false);
    const par_tile_spans up = par_tileset_extend_spans(t_in, t_in, (uint64_t)capacity, tile_bytes);
    if (e == hipSuccess && up.upload_bytes) e = hipMemcpy(d_tiles.as<uint8_t>(), tiles, up.upload_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        g.index = d_index.as<uint8_t>();
        e = launch_extend(nullptr, g, tile_w, tile_h, flips, d_work.as<void>(), d_tiles.as<uint8_t>(), capacity,
                          d_count.as<uint32_t>(), d_map.as<uint32_t>(), d_first.as<uint32_t>());
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    d_count.download(&t_out);
    d_first.download(&first_new);
    const par_tile_spans down = par_tileset_extend_spans(t_in, t_out, (uint64_t)capacity, tile_bytes);
    if (e == hipSuccess && down.download_bytes) {
        e = hipMemcpy(tiles + down.download_offset, d_tiles.as<uint8_t>() + down.download_offset, down.download_bytes,
                      hipMemcpyDeviceToHost);
    }
    d_map.download(map_out);
    if (e == hipSuccess) {
        *count = (int)t_out;
        if (first_new_out) *first_new_out = (int)first_new;
    }
    return par_status_of(e);
}

}  // extern "C"
