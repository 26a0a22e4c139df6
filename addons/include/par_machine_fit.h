/*
 * par_machine_fit.h — machine fit: par_cells_fit.h's table of per-cell sub-palettes, fitted under a tile machine's colour
 * depth and backdrop rule, so that what the fit minimises and reports is the error of the picture the machine shows
 * (nothing in the reference). An ADD-ON: plain C with <stddef.h> and <stdint.h> alone, no other header of the project;
 * its symbols are exported from libpar_machine_fit.so, not from libpar_raytracer.so or another add-on, and the statuses it
 * returns are the values of par_raytracer.h's par_status (PAR_OK 0, PAR_ERR_INVALID_ARG 1, PAR_ERR_NO_DEVICE 2,
 * PAR_ERR_HIP 3, PAR_ERR_OOM 4).
 *
 * Inputs, cells, the ragged edge, limits, outputs and alignments are par_cells_fit.h's: `fb` a whole frame of
 * width * height four-byte pixels aligned to 4 bytes, `palette` the master of n_colors four-byte entries of no alignment,
 * cell_w and cell_h each 8 or 16, at most PAR_MACHINE_FIT_MAX_CELLS (1 << 20) cells, 1 <= K = sub_size <= 16,
 * K <= n_colors <= 256, 1 <= S = n_sub, S * K <= 256, rounds R in [0, 32]; table_out S * K entries of no alignment,
 * seeds_out nullable S words aligned to 4, errors_out nullable R + 1 uint64_t aligned to 8. Two more arguments: `depth`,
 * a par_machine_depth, and `backdrop`, 0 or 1; with backdrop == 1, K is at least 2.
 * 1. The lattice. A level l of a depth of b bits (5, 3, 2 or 8) widens to w(l) by par_screen.h's bit replication:
 *        5 bits  l << 3 | l >> 2;   3 bits  l << 5 | l << 2 | l >> 1;   2 bits  l * 0x55;   8 bits  l
 *    Rounding a channel value x gives w(l) for the l with the smallest |x - w(l)|, the lowest l among equals.
 *    par_machine_round does that to red, green and blue of n entries and keeps alpha. w(l) >> (8 - b) == l for every
 *    level, so par_vram_palette_words followed by par_screen_palette_rgba gives a rounded entry back.
 * 2. The master. The fit reads `palette` through that rounding (the call rounds it itself into its work block, on the
 *    stream); below, palette[j] is the rounded entry. At PAR_MACHINE_RGBA8 the rounding is the identity.
 * 3. The seed. m(p), h_c, H, e, own, best, the signed gain, its tie rule (the lowest c among equals) and seeds_out are
 *    par_cells_fit.h's. With backdrop == 0 the lists W_c and A_0 are too. With backdrop == 1, b0 is the first index in
 *    the order (H[j] descending, j ascending), and every list, W_c and A_0, is b0 followed by the first K - 1 indices
 *    other than b0 in the list's usual order; own(c) is e under that list. So table[s * K + 0] == palette[b0] for every s.
 * 4. The rounds, R of them. Assign is par_cells_fit.h's: par_quantize_cells_device at spread 0 under the current table.
 *    Move: an entry that got pixels moves, per channel, to w(l) for the level l that minimises the sum over its pixels of
 *    |x - w(l)|, the lowest l among equals, and its alpha becomes 255; an entry without pixels keeps its four bytes.
 *    With backdrop == 1 the S entries at position 0 are ONE entry for the move: the pixels assigned to any s * K + 0 are
 *    pooled, and all S positions take the pooled optimum, or keep their bytes if no pixel took any of them. At 8 bits the
 *    lowest minimiser is the lower median, element (n - 1) / 2 of the sorted values: par_cells_fit.h's rule.
 * 5. Outputs. table_out, seeds_out (seeds_out[0] = 0xFFFFFFFF) and errors_out[0 .. R] are as in par_cells_fit.h.
 * Consequences:
 *  1. errors_out never rises with r: every entry is on the lattice from the seed on, a move minimises each channel's sum
 *     over the lattice, the pooled move the pooled sum, and a new choice only lowers it.
 *  2. Every channel of table_out is a w(l); with backdrop == 1, table_out[s * K] is the same four bytes for every s.
 *  3. At PAR_MACHINE_RGBA8 with backdrop == 0 every output equals par_cells_fit_device's byte for byte.
 *  4. errors_out[R] equals the summed L1 difference between fb and the fb_out of
 *     par_quantize_cells_device(table_out, S, K, spread 0).
 *  5. The closing identity under the machine's own rules: machine fit, cells, par_vram_local_device, the tile set under
 *     any flip mask, the encoded tiles, the map encoded with cell_out and par_vram_palette_words(table_out, f), drawn by
 *     par_screen_draw_device with pal_format f (BGR555, BGR333_MD and BGR222 are the depths of the same value), scroll 0
 *     and the fit's backdrop, give the cells frame with alpha 255 byte for byte wherever bad_out is 0; with the fit's
 *     backdrop == 1 a draw with screen backdrop 0 gives the same picture. The shown frame's error is errors_out[R].
 *  6. With S == 1, R == 0 and backdrop == 0 the table is the K most used rounded master entries.
 *  7. A frame of one colour gives S equal sub-palettes, and an error equal to its distance to the rounded master at R == 0.
 *  8. No output depends on the order in which the device runs anything: every sum is a sum of integers, the arg-max is
 *     par_cells_fit.h's 64-bit integer maximum of (gain + 2^18) << 20 | (2^20 - 1 - c).
 * PAR_ERR_INVALID_ARG, before any device work, with nothing written and without a GPU present, for: a null `fb`,
 * `palette`, `table_out` or (device form) `work`; a `work` that is not aligned to 8 bytes; any value outside the limits
 * above; a `depth` that is none of the four values; a `backdrop` that is not 0 or 1; backdrop == 1 with sub_size < 2.
 * Left out on purpose: the NES's fixed master palette as a lattice (a caller passes its 52 colours as the master at
 * PAR_MACHINE_RGBA8 with R == 0); a caller-chosen backdrop colour; dither awareness; a budget of distinct colours across
 * sub-palettes; row blocks and several frames.
 */
#ifndef PAR_MACHINE_FIT_H
#define PAR_MACHINE_FIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAR_MACHINE_FIT_MAX_CELLS (1 << 20)
#define PAR_MACHINE_FIT_MAX_SUB_SIZE 16
#define PAR_MACHINE_FIT_MAX_ROUNDS 32

/* equal in value to par_screen.h's par_screen_palette_format; 5, 3, 2 and 8 bits a channel */
enum par_machine_depth { PAR_MACHINE_BGR555 = 0, PAR_MACHINE_BGR333_MD = 1, PAR_MACHINE_BGR222 = 2, PAR_MACHINE_RGBA8 = 3 };

/* Host arithmetic: red, green and blue of the n (1 to 256) four-byte entries at `palette` rounded to the lattice of
 * `depth` into `out` (which may be `palette`), alpha kept. Returns the bytes written, 4 * n, or 0 with nothing written
 * for a null pointer, an n outside [1, 256] or a depth that is none of the four. */
size_t par_machine_round(const uint8_t* palette, int n, int depth, uint8_t* out);
/* Host arithmetic: the bytes of the work block, 0 outside the limits (par_cells_fit_work_bytes's rules). It is
 *     180224 + 25 * cells,    cells = ceil(width / cell_w) * ceil(height / cell_h)
 * (the rounded master in 1024 bytes, the 256 * 3 * 32 lattice counts, twelve words an entry of what the first selection
 * found, the 256 * 3 counts of x == a and 64-bit sums of x - a, then par_cells_fit.h's block of 59392 + 25 * cells).
 * O(cells), with no term in pixels. */
size_t par_machine_fit_work_bytes(int width, int height, int cell_w, int cell_h);
/* device pointers, asynchronous on `stream` (a hipStream_t), no allocation, no sync. `work` is aligned to 8 bytes and
 * holds par_machine_fit_work_bytes(...) bytes of anything: the call prepares what it needs of it itself, on the stream,
 * and keeps no state between calls, so it can be captured into a graph, and every replay fits the frame and the master the
 * stream then finds. 5 + S + 4 * R launches, one more with backdrop == 1 and one more with errors_out: the master's
 * rounding, then par_cells_fit_device's entry, cell pass and A_0, with backdrop == 1 a pass that puts b0 at the head of
 * every W_c and evaluates own(c) again, the S steps, per round two assign-and-tally passes with a select behind each (the
 * counts per lattice interval, which give the interval [a, b) of the lower median and the counts either side, then the
 * count of x == a and the sum of x - a inside it, which decide between a and b; at 8 bits the medians' two nibbles), the
 * table's copy to table_out, and the last assign pass for errors_out[R]. S + 1 + 2 * R (+ 1) (+ 1) of them read the frame. */
int par_machine_fit_device(void* stream, const uint8_t* fb, int width, int height, int cell_w, int cell_h,
                           const uint8_t* palette, int n_colors, int n_sub, int sub_size, int rounds, int depth,
                           int backdrop, void* work, uint8_t* table_out, uint32_t* seeds_out, uint64_t* errors_out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device): allocates (the work block
 * too), copies the frame and the master up, launches, synchronises, copies the table, the n_sub seeds and the
 * rounds + 1 errors back and frees. PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as par_cells_fit_host */
int par_machine_fit_host(int device, const uint8_t* fb, int width, int height, int cell_w, int cell_h,
                         const uint8_t* palette, int n_colors, int n_sub, int sub_size, int rounds, int depth, int backdrop,
                         uint8_t* table_out, uint32_t* seeds_out, uint64_t* errors_out);

#ifdef __cplusplus
}
#endif

#endif
