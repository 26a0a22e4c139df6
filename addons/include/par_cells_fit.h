/*
 * par_cells_fit.h — fitted cells: the table of per-cell sub-palettes that par_quantize_cells_device takes, fitted to a
 * frame on the device (nothing in the reference). An ADD-ON: plain C with <stddef.h> and <stdint.h> alone, no other
 * header of the project; its symbols are exported from libpar_cells_fit.so, not from libpar_raytracer.so, and the
 * statuses it returns are the values of par_raytracer.h's par_status (PAR_OK 0, PAR_ERR_INVALID_ARG 1,
 * PAR_ERR_NO_DEVICE 2, PAR_ERR_HIP 3, PAR_ERR_OOM 4).
 *
 * par_quantize_cells_device (par_cells.h) picks, per cell, one of S = n_sub sub-palettes of K = sub_size entries; this
 * call makes that table from a frame and a master palette: a greedy seed that takes whole cells' wanted lists, then R
 * rounds of assign-and-median. It is a pass over a finished `fb`, whatever made it; it takes no context and no
 * par_params.
 *
 * Inputs: `fb` is a whole frame of width * height four-byte pixels, red, green, blue, alpha, dense and row-major, aligned
 * to 4 bytes; alpha takes no part. `palette` is the master palette, n_colors four-byte entries (a fitted, refined or
 * hardware palette), of no alignment beyond a byte. Cells and the ragged edge are par_cells.h's: cell (cx, cy) covers the
 * columns [cx * cell_w, min((cx + 1) * cell_w, width)) and the rows [cy * cell_h, min((cy + 1) * cell_h, height));
 * gcx = ceil(width / cell_w), gcy = ceil(height / cell_h), and a cell's number is c = cx + cy * gcx.
 * Limits: cell_w and cell_h each 8 or 16; width and height at least 1 and at most PAR_CELLS_FIT_MAX_CELLS (1 << 20)
 * cells, so no 32-bit tally can overflow; 1 <= K <= PAR_CELLS_FIT_MAX_SUB_SIZE (16); K <= n_colors <= 256; 1 <= S;
 * S * K <= 256; rounds R in [0, PAR_CELLS_FIT_MAX_ROUNDS] (32).
 * The seed, in integers, L1(p, q) = |p.red - q.red| + |p.green - q.green| + |p.blue - q.blue|:
 *     m(p)       the L1-nearest master entry of pixel p, the lowest index among equals (quantise at spread 0)
 *     h_c[j]     the number of pixels of cell c with m(p) = j;  H[j] the sum of h_c[j] over all cells
 *     W_c        the cell's wanted list: the first K master indices in the order (h_c[j] descending, j ascending);
 *                entries with a count of 0 fill it up, lowest index first
 *     A_0        the first K indices in the order (H[j] descending, j ascending)
 *     e(c, A)    the sum over the cell's existing pixels of min over j in A of L1(p, palette[j])   (<= 256 * 765)
 *     own(c)     = e(c, W_c);   best_1(c) = e(c, A_0)
 *     for m = 1 .. S - 1:  c* = the cell with the largest SIGNED gain best_m(c) - own(c), the lowest c among equals (a
 *                gain of 0 or below is a value like any other);  A_m = W_c*;  best_(m+1)(c) = min(best_m(c), e(c, A_m))
 *     the seed table: table[s * K + k] = palette[A_s[k]], all four bytes, in list order
 *     seeds_out[0] = 0xFFFFFFFF, seeds_out[m] = c* of step m
 * The rounds, R of them, each two steps:
 *     assign     as par_quantize_cells_device does at spread 0 under the current table: every cell takes s*, the lowest s
 *                of the smallest E(s), every pixel k(p, s*), the lowest k of the smallest distance
 *     move       every entry that got pixels moves to the per-channel LOWER MEDIAN of them, element (n - 1) / 2 of the
 *                sorted values (par_palette_refine_device's rule), and its alpha becomes 255; an entry without pixels
 *                keeps its four bytes
 * Outputs:
 *     table_out      the S * K entries after R rounds, four bytes each, of no alignment beyond a byte
 *     seeds_out[m]   nullable, S words aligned to 4 bytes
 *     errors_out[r]  nullable, R + 1 uint64_t aligned to 8 bytes: for r = 0 .. R the sum over all cells of E(s*) under the
 *                    table before round r + 1; errors_out[R] is the error under table_out and costs one more assign pass,
 *                    which is skipped when errors_out is null
 * Consequences:
 *  1. errors_out never rises with r (a lower median minimises a channel's summed distance, a new choice only lowers it).
 *  2. At R == 0 the seed sets are nested in S, so errors_out[0] never rises as S grows.
 *  3. errors_out[R] equals the summed L1 difference between fb and the fb_out of
 *     par_quantize_cells_device(table_out, S, K, spread 0): the table feeds that call, present and upscale unchanged.
 *  4. With S == 1 and R == 0 the table is the K most used master entries.
 *  5. A frame of one colour gives S equal sub-palettes, and an error equal to its distance to the master at R == 0.
 *  6. Equal sub-palettes do no harm: cells take the lowest.
 *  7. A padded master (copies of entry 0 behind it) gets no pixel at the copies, and they are wanted last.
 *  8. No output depends on the order in which the device runs anything: every sum is a sum of integers, the arg-max
 *     is a 64-bit integer maximum of (gain + 2^18) << 20 | (2^20 - 1 - c).
 * PAR_ERR_INVALID_ARG, before any device work, with nothing written and without a GPU present, for: a null `fb`,
 * `palette`, `table_out` or (device form) `work`; a `work` that is not aligned to 8 bytes; any value outside the limits
 * above.
 * Left out on purpose: row blocks and several frames; dither awareness (the fit is at spread 0); entries restricted to
 * the master palette after the rounds; other seeds (summed-gain facility location, k-means++); a budget of distinct
 * colours across sub-palettes.
 */
#ifndef PAR_CELLS_FIT_H
#define PAR_CELLS_FIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAR_CELLS_FIT_MAX_CELLS (1 << 20)
#define PAR_CELLS_FIT_MAX_SUB_SIZE 16
#define PAR_CELLS_FIT_MAX_ROUNDS 32

/* Host arithmetic: the bytes of the work block of a fit over a width x height frame under cells of cell_w x cell_h, 0
 * outside the limits (a dimension below 1, a cell dimension that is not 8 or 16, more than 1 << 20 cells). It is
 *     59392 + 25 * cells,    cells = ceil(width / cell_w) * ceil(height / cell_h)
 * (H, the S arg-max words, the table, the medians' chosen nibbles and ranks and their 256 * 3 * 16 tallies; then a cell's
 * own and best, four bytes each, its wanted list in 16 bytes and its s* in one). O(cells), with no term in pixels: m(p)
 * and k(p) are computed again where they are needed, never stored. */
size_t par_cells_fit_work_bytes(int width, int height, int cell_w, int cell_h);
/* device pointers, asynchronous on `stream` (a hipStream_t), no allocation, no sync. `work` is aligned to 8 bytes and
 * holds par_cells_fit_work_bytes(...) bytes of anything: the call prepares what it needs of it itself, on the stream, and
 * keeps no state between calls, so it can be captured into a graph, and every replay fits the frame and the master the
 * stream then finds. 4 + S + 4 * R launches, one more with errors_out: the entry, the cell pass (m, h_c, W_c, own, H), A_0,
 * S evaluations of one K-entry sub-palette over all cells (the first gives best_1, each later one is a seed step), per
 * round two assign-and-tally passes (the medians' high nibbles, then their low nibbles) with a select behind each, the
 * table's copy to table_out, and the last assign pass for errors_out[R]. S + 1 + 2 * R (+ 1) of them read the frame. */
int par_cells_fit_device(void* stream, const uint8_t* fb, int width, int height, int cell_w, int cell_h,
                         const uint8_t* palette, int n_colors, int n_sub, int sub_size, int rounds, void* work,
                         uint8_t* table_out, uint32_t* seeds_out, uint64_t* errors_out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device): allocates (the work block
 * too), copies the frame and the master up, launches, synchronises, copies the table, the n_sub seeds and the
 * rounds + 1 errors back and frees. PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as par_quantize_cells_host */
int par_cells_fit_host(int device, const uint8_t* fb, int width, int height, int cell_w, int cell_h,
                       const uint8_t* palette, int n_colors, int n_sub, int sub_size, int rounds, uint8_t* table_out,
                       uint32_t* seeds_out, uint64_t* errors_out);

#ifdef __cplusplus
}
#endif

#endif
