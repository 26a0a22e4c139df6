/*
 * par_tileset.h — tile sets: an index plane deduplicated into its distinct tiles and a tile map, and the map drawn back
 * into a plane (nothing in the reference, which presents RGBA8). Plain C, beside par_raytracer.h and par_cells.h: the
 * statuses are par_raytracer.h's par_status, the symbols are exported from libpar_raytracer.so like any other.
 *
 * The machines par_quantize_cells_device models do not store a picture. They store the distinct cells of it, the TILE
 * SET, and a TILE MAP of one entry a cell that names a tile and, on everything after the NES, whether it is mirrored.
 * These calls are a pass over a finished index plane, whatever made it; they take no context.
 *
 * Planes: `index` / `index_out` is a byte per pixel, dense and row-major, addresses the element of (row_begin, column 0)
 * and holds (row_end - row_begin) * width bytes (width = params->width). It has no alignment beyond a byte: a width that
 * is not a multiple of 4 puts every row at another phase. `tiles` / `tiles_out` and the map have no alignment beyond
 * their element's either (a byte, a uint32_t); `work` is aligned to 8 bytes.
 * Tiles: tile_w and tile_h are each 8 or 16. Cell (cx, cy) covers the columns [cx * tile_w, (cx + 1) * tile_w) and the
 * ABSOLUTE rows [cy * tile_h, (cy + 1) * tile_h); a pixel of the cell that lies beyond params->width or params->height
 * has the value `pad` (0 .. 255). gcx = ceil(width / tile_w). Rows are cut as the cells contract cuts them:
 * row_begin % tile_h == 0, and row_end % tile_h == 0 or row_end == height. The call's cells are numbered
 *     c = cx + (cy - row_begin / tile_h) * gcx,        N = gcx * ceil((row_end - row_begin) / tile_h) of them,
 * and N <= PAR_TILESET_MAX_CELLS.
 * Flips: `flips` is a mask in [0, 3]. Bit 0 allows a mirror in x, t'[y][x] = t[y][tile_w - 1 - x]; bit 1 allows a mirror
 * in y, t'[y][x] = t[tile_h - 1 - y][x]. A flip code f (bit 0: x, bit 1: y) is allowed when (f & ~flips) == 0.
 *     The CANONICAL FORM of a cell is the smallest, as a row-major string of tile_w * tile_h unsigned bytes, of its
 *     images under the allowed codes, and f* is the lowest code that gives it.
 * Flips are involutions, so the cell is its canonical form under f*. With flips == 0 the canonical form is the cell.
 * Numbering: two cells belong to the same tile exactly when their canonical forms are equal byte for byte. Tiles are
 * numbered 0, 1, ... in the order of the lowest cell number c in which each appears (the order a host loop over the
 * cells gives), and T is their count.
 * Outputs of a build:
 *     map_out[c]  = id | (f* << 30): a uint32_t a cell, the tile number in the low 30 bits, the x flip in bit 30, the y
 *                   flip in bit 31
 *     tiles_out + i * tile_w * tile_h = the canonical form of tile i, row-major, for every i < min(T, capacity). Tiles
 *                   from `capacity` on are not written and no byte beyond `capacity` tiles is touched; the map still
 *                   numbers them.
 *     *count_out  = T (a uint32_t in device memory; an int through par_tileset_build_host)
 * map_out and tiles_out are each nullable, count_out is not, and capacity may be 0 with a null tiles_out: that is how to
 * count tiles without storing any ("does this frame fit 256 tiles?").
 * Expand draws a tile map: with (id, f) = (map[c] & 0x3FFFFFFF, map[c] >> 30) every pixel of the frame's rows takes its
 * byte of tile min(id, n_tiles - 1) under the flips f (the clamp par_present_device applies to a palette: it only keeps
 * the load inside the tile set). Pixels of a cell beyond the frame are not written. It is the inverse of build, and the
 * call that scrolls or recomposes a background from a tile set without rendering.
 * Consequences: T and all outputs depend on nothing but the call's bytes, the geometry, `pad` and `flips`; in particular
 * not on the order in which the device runs anything. A row block's result is that of a frame consisting of those rows:
 * tile numbers are per call. With one colour everywhere T == 1, or 2 where a ragged edge shows `pad`. Allowing more
 * flips never raises T. A cell that equals its own mirror takes the lower flip code. par_tileset_expand_device on the
 * outputs of a build gives the input plane back byte for byte when T <= capacity.
 * PAR_ERR_INVALID_ARG, before any device work and with nothing written (no GPU is needed to get it), for: a null
 * `params`, `index`, `work` or `count_out`, a `work` that is not aligned to 8 bytes; tiles_out null with capacity > 0, or
 * capacity < 0; a tile dimension that is not 8 or 16; pad outside [0, 255] or flips outside [0, 3]; params->width <= 0,
 * rows that are not 0 <= row_begin < row_end <= params->height, a row cut that breaks the rule, or N >
 * PAR_TILESET_MAX_CELLS; and for expand: a null `tiles`, `map` or `index_out`, or n_tiles < 1.
 * Left out on purpose: rotations (no tile hardware of the kind has them); matching tiles across palette remaps; merging
 * the sets of shards (tile numbers are per call); lossy merging of similar tiles to meet a budget; the sub-palette number
 * in the map word (par_quantize_cells_device's cell_out holds it, one byte a cell in the same numbering); and fusing
 * into the cells kernel. The lossy merge now exists, in an add-on beside the library: addons/include/par_tileset_reduce.h.
 * So do the match across palette remaps and the sub-palette number in a machine's map word: addons/include/par_vram.h.
 */
#ifndef PAR_TILESET_H
#define PAR_TILESET_H

#include <stddef.h>

#include "par_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PAR_TILESET_MAX_CELLS (1 << 20)
#define PAR_TILESET_FLIP_X 1
#define PAR_TILESET_FLIP_Y 2

/* Host arithmetic: the bytes of the work block a build call over n_cells cells needs, 0 for n_cells outside
 * [1, PAR_TILESET_MAX_CELLS]. With P the smallest power of two >= 2 * n_cells it is
 *     4096 + 16 * n_cells + 4 * P
 * (the scan's 1024 partial sums; a 64-bit hash, a representative and a number a cell; a table of P four-byte slots),
 * which is at most 4096 + 32 * n_cells because P < 4 * n_cells. */
size_t par_tileset_work_bytes(int n_cells);
/* device pointers, asynchronous on `stream` (a hipStream_t), no allocation, no sync. `work` holds
 * par_tileset_work_bytes(N) bytes of anything: the call prepares what it needs of it itself, on the stream, so a second
 * call on the same block needs no reset and the call can be captured into a graph and replayed. */
int par_tileset_build_device(const par_params* params, void* stream, const uint8_t* index, int row_begin, int row_end,
                             int tile_w, int tile_h, int pad, int flips, void* work, uint8_t* tiles_out, int capacity,
                             uint32_t* map_out, uint32_t* count_out);
/* device pointers, asynchronous on `stream`, no allocation, no sync, no work block */
int par_tileset_expand_device(const par_params* params, void* stream, const uint8_t* tiles, int n_tiles, int tile_w,
                              int tile_h, const uint32_t* map, int row_begin, int row_end, uint8_t* index_out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device): allocates (the work block
 * too), copies, launches, synchronises, copies back and frees; T through count_out. PAR_ERR_NO_DEVICE / PAR_ERR_OOM /
 * PAR_ERR_HIP as par_quantize_host */
int par_tileset_build_host(const par_params* params, int device, const uint8_t* index, int row_begin, int row_end,
                           int tile_w, int tile_h, int pad, int flips, uint8_t* tiles_out, int capacity, uint32_t* map_out,
                           int* count_out);
int par_tileset_expand_host(const par_params* params, int device, const uint8_t* tiles, int n_tiles, int tile_w,
                            int tile_h, const uint32_t* map, int row_begin, int row_end, uint8_t* index_out);

#ifdef __cplusplus
}
#endif

#endif
