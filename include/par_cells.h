/*
 * par_cells.h — colour cells: a frame quantised under per-cell sub-palettes (nothing in the reference, which presents
 * RGBA8). Plain C, beside par_raytracer.h: the statuses are that header's par_status, the symbols are exported from
 * libpar_raytracer.so like any other.
 *
 * par_quantize_device models one flat palette that any pixel may use. The tile hardware this renderer imitates cuts the
 * frame into cells of 8 x 8 or 16 x 16 pixels, and a cell may use only ONE small sub-palette out of a few (NES
 * background: 4 of 4 colours, 16 x 16; Game Boy Color: 8 of 4, 8 x 8; Mega Drive / SNES: 4 to 8 of 16, 8 x 8; ZX Spectrum
 * and C64 hires: any two colours of the palette, 8 x 8). The choice is made per cell and depends on all of its pixels.
 * These calls are a pass over a finished `fb` plane, whatever made it; they take no context.
 *
 * Planes: exactly par_quantize_device's. `fb`, `fb_out` and `index_out` address the element of (row_begin, column 0)
 * and hold (row_end - row_begin) * width elements, dense and row-major; fb_out == fb (in place) is allowed, any other
 * overlap is undefined. Alpha takes no part in the search; the pixel's own alpha passes through.
 * Palette: with S = n_sub and K = sub_size it is a flat table of S * K entries, sub-palette s being entries
 * [s * K, (s + 1) * K); 1 <= S, 1 <= K and S * K <= PAR_MAX_PALETTE. index_out holds indices into the FLAT table, so
 * the same table is the palette of par_present_device / par_upscale_device, and rotating it is palette cycling.
 * Cells: cell_w and cell_h are each 8 or 16. Cell (cx, cy) covers the columns [cx * cell_w, min((cx + 1) * cell_w, width))
 * and the ABSOLUTE rows [cy * cell_h, min((cy + 1) * cell_h, height)); gcx = ceil(width / cell_w). Rows are cut at cell
 * rows: row_begin % cell_h == 0, and row_end % cell_h == 0 or row_end == height. With that a row block of a sharded
 * frame equals those rows of the whole frame.
 * For every pixel p of a cell, in integers:
 *     c'      = the dithered colour of the quantise contract at `spread` (B4, the floor and the clamp on the absolute
 *               row and column; at spread 0 the pixel itself)
 *     d(p, s) = min over k < K of |r' - P.red| + |g' - P.green| + |b' - P.blue|,  P = palette[s * K + k]      (L1)
 *     k(p, s) = the lowest such k among equals
 * For every cell:
 *     E(s) = the sum of d(p, s) over the cell's pixels that exist            (<= 256 * 765, under 2^18)
 *     s*   = the s with the smallest E(s), the lowest s among equals: the minimum of (E(s) << 8) | s
 * Outputs, each nullable, at least one of fb_out and index_out:
 *     index_out = (uint8_t)(s* * K + k(p, s*))
 *     fb_out    = {that entry's red, green, blue, the pixel's own alpha}
 *     cell_out[cx + (cy - row_begin / cell_h) * gcx] = (uint8_t)s*
 * cell_out is one byte per cell of the block's cell rows and addresses the cell row row_begin / cell_h.
 * Consequences: with S == 1 the index plane and the frame are par_quantize_device's for the K-entry palette at the
 * same spread, byte for byte, and cell_out is all 0. With two identical sub-palettes the lower one is always chosen. A
 * cell whose pixels, after the dither, are all entries of sub-palette s has E(s) == 0 and takes the lowest such s. The
 * result depends on nothing but the cell's pixels and their absolute position.
 * PAR_ERR_INVALID_ARG, before any device work and with nothing written (no GPU is needed to get it), for a null
 * `params`, palette or `fb`, both fb_out and index_out null, S < 1, K < 1 or S * K > PAR_MAX_PALETTE, a cell dimension
 * that is not 8 or 16, spread outside [0, 255], params->width <= 0, rows that are not
 * 0 <= row_begin < row_end <= params->height, or a row cut that breaks the cell rule.
 * Left out on purpose: no fitting of sub-palettes to a frame (the fitted-palette calls give a flat palette; how to
 * group it is the caller's art direction; the add-on addons/include/par_cells_fit.h fits a table to a frame on the
 * device, in a library of its own), no pattern dither inside cells, no cell sizes other than the four, no fusing
 * into par_finish_device, and no row cuts through a cell. The add-on addons/include/par_vram.h takes index_out apart
 * into what a tile stores (% K) and packs cell_out into a machine's map words.
 */
#ifndef PAR_CELLS_H
#define PAR_CELLS_H

#include "par_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* device pointers (`d_palette` too), asynchronous on `stream` (a hipStream_t), no allocation, no sync: in a frame loop
 * it takes par_quantize_device's place on the frame's own stream */
int par_quantize_cells_device(const par_params* params, void* stream, const par_color* d_palette, int n_sub,
                              int sub_size, int cell_w, int cell_h, int spread, const par_color* fb, int row_begin,
                              int row_end, par_color* fb_out, uint8_t* index_out, uint8_t* cell_out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device): allocates, copies, launches,
 * synchronises, copies back and frees; PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as par_quantize_host */
int par_quantize_cells_host(const par_params* params, int device, const par_color* palette, int n_sub, int sub_size,
                            int cell_w, int cell_h, int spread, const par_color* fb, int row_begin, int row_end,
                            par_color* fb_out, uint8_t* index_out, uint8_t* cell_out);
/* The sub-palettes of the mode in which a cell may use any two colours of a palette. Host arithmetic, no GPU needed:
 * `out` gets the flat table of every unordered pair (i, j), i < j, of the n_colors entries of `palette`, in ascending
 * order of (i, j), each pair as {palette[i], palette[j]}; that is S = n_colors * (n_colors - 1) / 2 and K = 2.
 * n_colors must lie in [2, 16]: 16 gives 120 pairs, 240 entries. Returns S and writes at most `capacity` ENTRIES, or
 * minus PAR_ERR_INVALID_ARG for a null pointer, capacity < 0 or n_colors out of range. */
int par_cells_pairs(const par_color* palette, int n_colors, par_color* out, int capacity);

#ifdef __cplusplus
}
#endif

#endif
