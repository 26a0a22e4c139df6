/*
 * par_tileset_reduce.h — tile budgets: a tile set and its map reduced to at most K tiles, on the device (nothing in the
 * reference). An ADD-ON: plain C with <stddef.h> and <stdint.h> alone, no other header of the project; its symbols are
 * exported from libpar_tileset_reduce.so, not from libpar_raytracer.so, and the statuses it returns are the values of
 * par_raytracer.h's par_status (PAR_OK 0, PAR_ERR_INVALID_ARG 1, PAR_ERR_NO_DEVICE 2, PAR_ERR_HIP 3, PAR_ERR_OOM 4).
 *
 * par_tileset_build_device answers "does this frame fit 256 tiles?"; where the answer is no, this call makes a set
 * that does: it KEEPS K of the tiles, bytes unchanged, and sends every other tile to the kept tile (and mirror) nearest
 * to it in colour. It is a pass over a finished tile set and its map, whatever made them; it takes no context and no
 * par_params.
 *
 * Inputs: `tiles`, `capacity` and `count` are as a build or an extend leaves them: stored tile i is the tile_w * tile_h
 * bytes at tiles + i * tile_w * tile_h, `count` is a uint32_t in device memory, and T = min(*count, capacity) as the
 * stream finds it (the host never learns T). `map` has n_cells entries of id | f << 30 (par_tileset.h's map word); an
 * id at or above T is read as T - 1, the clamp par_tileset_expand_device applies. `palette` is n_colors entries of four
 * bytes, red, green, blue, alpha: par_quantize_device's palette. A tile byte b has the colour
 * palette[min(b, n_colors - 1)]; alpha is not counted, as in quantise. `flips` is par_tileset.h's mask: a flip code f
 * (bit 0: x, bit 1: y) is allowed when (f & ~flips) == 0. Tiles and the palette have no alignment beyond a byte, the
 * maps, the remap and the counts are aligned to 4 bytes, error_out and `work` to 8.
 * Limits: capacity in [1, PAR_TILESET_REDUCE_MAX_TILES]; budget K in [1, PAR_TILESET_REDUCE_MAX_BUDGET]; n_cells in
 * [1, 1 << 20]; n_colors in [1, 256]; tile_w and tile_h each 8 or 16.
 * Definitions:
 *     u[i]        the number of map entries whose clamped id is i
 *     D(i, k, f)  the sum, over the tile's pixels and the three channels, of
 *                 |colour(t_i[y][x]) - colour(flip_f(t_k)[y][x])|; at most 256 * 765, so u * D fits 64 bits with room
 *     d_S(i)      for a set S of tiles, the least D(i, k, f) over k in S and the allowed codes f
 *     (a_S(i), g_S(i))  the pair (k, f) that gives d_S(i): the lowest k, then the lowest f
 * The kept set: if T <= K every tile is kept. Otherwise S_1 holds the tile of largest u, the lowest number among equals;
 * S_(m+1) adds to S_m the tile i outside it of largest u[i] * d_S_m(i), the lowest number among equals (a product of 0
 * is a value like any other); S = S_K. Kept tiles get the new numbers 0, 1, ... in ascending order of their old numbers.
 * Outputs:
 *     tiles_out      the min(T, K) kept tiles at their new numbers, bytes unchanged. It holds `budget` tiles; nothing
 *                    beyond min(T, K) tiles is touched. It must not overlap `tiles`.
 *     remap_out[i]   for i < T, nullable: for a kept tile its new number with flip 0; for a dropped tile
 *                    new(a_S(i)) | g_S(i) << 30. Entries from T on are not written.
 *     map_out[c]     = (r & 0x3FFFFFFF) | (((map[c] >> 30) ^ (r >> 30)) << 30), r the remap of the entry's clamped id:
 *                    flips commute and are involutions, so the codes compose by XOR. map_out may be `map`.
 *     *count_out     = min(T, K) (a uint32_t in device memory; an int through the host form). It may be `count`.
 *     *error_out     nullable, a uint64_t: the sum over dropped i of u[i] * d_S(i).
 * With T == 0 the count is 0, the error is 0, map_out takes map's words, and nothing else is written.
 * Consequences:
 *  1. T <= K is the identity: the first T tiles come back byte for byte, the map keeps its flips and has clamped ids, the
 *     remap is 0 .. T - 1 and the error is 0.
 *  2. K == 1 keeps the most used tile.
 *  3. The kept sets are nested in K, so the error never rises as K grows.
 *  4. Expanding (tiles_out, map_out) and expanding (tiles, map), each viewed through the palette, differ by a summed L1
 *     equal to the error: exactly when the frame's width and height are multiples of the tile's, and by at most the error
 *     where a ragged edge shows `pad`.
 *  5. A build of the expanded reduced plane under the same `flips` counts at most K tiles.
 *  6. Palette entries with equal colours make D == 0: merging such tiles costs nothing, and a padded fitted palette
 *     (copies of entry 0) does not disturb anything.
 *  7. A stored tile no map entry uses has u == 0: it is kept only on a tie at 0.
 *  8. No output depends on the order in which the device runs anything.
 * PAR_ERR_INVALID_ARG, before any device work, with nothing written and without a GPU present, for: a null `tiles`,
 * `count`, `map`, `palette`, `work`, `tiles_out`, `map_out` or `count_out`, or a `work` that is not aligned to 8 bytes;
 * tiles_out's `budget` tiles overlapping tiles' `capacity` tiles; any value outside the limits above; flips outside
 * [0, 3]; and through the host form, which takes n_tiles in count's and capacity's place, n_tiles outside
 * [1, PAR_TILESET_REDUCE_MAX_TILES].
 * Left out on purpose: changing a kept tile's bytes (k-medoid rounds over a cluster); agglomerative merging; a budget per
 * sub-palette; reducing a shared set across frames without one map; rotations.
 */
#ifndef PAR_TILESET_REDUCE_H
#define PAR_TILESET_REDUCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAR_TILESET_REDUCE_MAX_TILES 4096
#define PAR_TILESET_REDUCE_MAX_BUDGET 1024
#define PAR_TILESET_REDUCE_MAX_CELLS (1 << 20)

/* Host arithmetic: the bytes of the work block of a reduce over n_cells map entries and a set of `capacity` tiles, 0 for
 * n_cells outside [1, 1 << 20] or capacity outside [1, PAR_TILESET_REDUCE_MAX_TILES]. It is
 *     4096 + 20 * capacity
 * (T and min(T, K); the two sets of at most 128 eight-byte partial maxima the selection steps hand to each other; then
 * five words a tile: u, d, a | g << 30, the kept mark, the remap). Nothing is kept per cell: the bound
 * O(n_cells + capacity) holds with no term in n_cells, and there is no T x T matrix. */
size_t par_tileset_reduce_work_bytes(int n_cells, int capacity);
/* device pointers, asynchronous on `stream` (a hipStream_t), no allocation, no sync. `work` is aligned to 8 bytes and
 * holds par_tileset_reduce_work_bytes(n_cells, capacity) bytes of anything: the call prepares what it needs of it
 * itself, on the stream, and keeps no state between calls, so it can be captured into a graph, and every replay reduces
 * the set and the count the stream then finds. budget + 6 launches, whatever T is: the entry, the usage count, the
 * start, `budget` selection steps (one launch a step, ceil(capacity / 32) workgroups each; a step with nothing left to
 * add ends at once), the numbering, the compaction and the map. */
int par_tileset_reduce_device(void* stream, const uint8_t* tiles, int capacity, const uint32_t* count, int tile_w,
                              int tile_h, int flips, const uint32_t* map, int n_cells, const uint8_t* palette,
                              int n_colors, int budget, void* work, uint8_t* tiles_out, uint32_t* map_out,
                              uint32_t* remap_out, uint32_t* count_out, uint64_t* error_out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device): allocates (the work block
 * too), copies the n_tiles tiles, the map and the palette up, launches, synchronises, copies the min(n_tiles, budget)
 * kept tiles, the map, the n_tiles remap entries, the count and the error back and frees; tiles_out beyond the kept
 * tiles keeps the caller's bytes. PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as par_tileset_build_host */
int par_tileset_reduce_host(int device, const uint8_t* tiles, int n_tiles, int tile_w, int tile_h, int flips,
                            const uint32_t* map, int n_cells, const uint8_t* palette, int n_colors, int budget,
                            uint8_t* tiles_out, uint32_t* map_out, uint32_t* remap_out, int* count_out,
                            uint64_t* error_out);

#ifdef __cplusplus
}
#endif

#endif
