/*
 * par_tileset_extend.h — shared tile sets: a build that starts from a tile set that already exists, with the set and its
 * count staying on the device (nothing in the reference). Plain C, beside par_tileset.h, whose contract it extends: the
 * statuses are par_raytracer.h's par_status, the symbols are exported from libpar_raytracer.so like any other.
 *
 * par_tileset_build_device numbers tiles per call. A sprite sheet, a tile map's set or a texture atlas is ONE set that
 * every frame's map indexes, and a frame uploads only the few tiles it adds. par_tileset_extend_device is that: call it
 * frame after frame on the same `tiles` and `count` (and replay it from a graph), on the row blocks of a frame in
 * ascending order, or on a finished set to merge it into another.
 *
 * The plane, the cells, `pad`, the row-cut rule, the cell numbering c, N, `flips`, the canonical form and f* are word for
 * word those of par_tileset.h (PAR_TILESET_MAX_CELLS is its limit, 1 << 20).
 * The set on entry: `tiles` and `count` are read AND written. T_in = *count as the stream finds it, and
 * S = min(T_in, capacity) tiles are stored: stored tile i is the tile_w * tile_h bytes at tiles + i * tile_w * tile_h.
 * Stored tiles are taken as the bytes they are; they are neither canonicalised nor checked for duplicates.
 * For every cell of the call: if its canonical form equals, byte for byte, a stored tile i < S, its tile number is the
 * LOWEST such i. Otherwise the cells of the call with equal canonical forms are one NEW tile, and the new tiles are
 * numbered T_in, T_in + 1, ... in the order of the lowest cell number c in which each appears.
 * Outputs:
 *     map_out[c]     = id | (f* << 30), as a build's; nullable
 *     tiles + id * tile_w * tile_h = the canonical form of every new tile whose number is below `capacity`
 *     *count         = T_out = T_in + the number of new tiles (a uint32_t in device memory; an int through the host form)
 *     *first_new_out = T_in; nullable
 * Tiles [first_new, min(count, capacity)) are exactly what the call added: the upload list of the frame. No other byte of
 * `tiles` is touched: stored tiles keep their bytes, and nothing from min(T_out, capacity) tiles on is written.
 * Numbers: the caller keeps T_in + N below 2^30; beyond that the map holds the low 30 bits of a number.
 * Capacity lies in [0, PAR_TILESET_MAX_CELLS]; `tiles` may be null only with capacity == 0. With capacity 0 nothing is
 * stored, nothing can match, and the call only adds this plane's T to the count.
 * Consequences:
 *  1. With *count == 0 on entry, `tiles`, map_out and *count are byte for byte par_tileset_build_device's for the same
 *     arguments.
 *  2. A sequence of calls on one tiles / count pair gives, while T_out <= capacity, what ONE host loop with one dict over
 *     all the calls' cells in call order gives.
 *  3. So the row blocks of a frame in ascending order from count 0 give the whole frame's build, and the concatenated
 *     maps are the frame's map;
 *  4. and two frames of the same width, the first a multiple of tile_h high, give the build of the first stacked on the
 *     second.
 *  5. Calling again with the same plane adds nothing: the count and `tiles` are unchanged and the map is the same.
 *  6. Merge: a stored set B of T_B tiles is an index plane of width tile_w and T_B * tile_h rows whose cells are its
 *     tiles. Extending a set A with that plane makes the merged set, and map_out is B's renumbering into it; if B is
 *     canonical under the same `flips`, every flip code is 0. This needs a par_params of that width and height.
 *  7. Overflow: once T_out > capacity, tiles that were not stored cannot be matched, a later cell equal to one of them
 *     counts again, and *count is an upper bound; *count <= capacity holds exactly when the set is complete.
 *  8. A caller-made set: among duplicate stored tiles the lowest number wins. A stored tile that is no cell's canonical
 *     form is never matched: under flips == 3 a cell that equals such a tile bytewise, but whose canonical form is a
 *     mirror, makes a new tile.
 *  9. No output depends on the order in which the device runs anything.
 * PAR_ERR_INVALID_ARG, before any device work and with nothing written (no GPU is needed to get it), for par_tileset.h's
 * list of a build with `count` in count_out's place and `tiles` in tiles_out's, and for capacity >
 * PAR_TILESET_MAX_CELLS; through the host form also for *count < 0.
 * Left out on purpose: removing tiles from a set; lossy merging of similar tiles to meet a budget; a hash table that
 * persists between calls (every call hashes the stored tiles again); rotations; and the torch.distributed plumbing of a
 * sharded merge (the sharded path has never run on more than one GPU). The lossy merge now exists, in an add-on beside
 * the library: addons/include/par_tileset_reduce.h.
 */
#ifndef PAR_TILESET_EXTEND_H
#define PAR_TILESET_EXTEND_H

#include <stddef.h>

#include "par_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host arithmetic: the bytes of the work block an extend call over n_cells cells into a set of `capacity` tiles needs,
 * 0 for n_cells outside [1, PAR_TILESET_MAX_CELLS] or capacity outside [0, PAR_TILESET_MAX_CELLS]. With P the smallest
 * power of two >= 2 * (n_cells + capacity) it is
 *     4096 + 16 * n_cells + 4 * P + 8
 * (the scan's 1024 partial sums; a 64-bit hash, a representative and a number a cell; a table of P four-byte slots for
 * the cells and the stored tiles; T_in and S as the call found them), which is at most
 * 4104 + 32 * (n_cells + capacity) because P < 4 * (n_cells + capacity). */
size_t par_tileset_extend_work_bytes(int n_cells, int capacity);
/* device pointers, asynchronous on `stream` (a hipStream_t), no allocation, no sync. `work` is aligned to 8 bytes and
 * holds par_tileset_extend_work_bytes(N, capacity) bytes of anything: the call prepares what it needs of it itself, on
 * the stream, and keeps no state between calls, so it can be captured into a graph, and every replay extends the set as
 * the stream then finds it. */
int par_tileset_extend_device(const par_params* params, void* stream, const uint8_t* index, int row_begin, int row_end,
                              int tile_w, int tile_h, int pad, int flips, void* work, uint8_t* tiles, int capacity,
                              uint32_t* count, uint32_t* map_out, uint32_t* first_new_out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device): allocates (the work block
 * too), copies the min(*count, capacity) stored tiles up, launches, synchronises, copies the added tiles, the map, the
 * count and first_new back and frees. Tiles from min(T_out, capacity) on keep the caller's bytes. PAR_ERR_NO_DEVICE /
 * PAR_ERR_OOM / PAR_ERR_HIP as par_tileset_build_host */
int par_tileset_extend_host(const par_params* params, int device, const uint8_t* index, int row_begin, int row_end,
                            int tile_w, int tile_h, int pad, int flips, uint8_t* tiles, int capacity, int* count,
                            uint32_t* map_out, int* first_new_out);

#ifdef __cplusplus
}
#endif

#endif
