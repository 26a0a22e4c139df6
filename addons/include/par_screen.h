/*
 * par_screen.h — Screen: one background layer of a tile machine drawn from its VRAM bytes, the machine's own last step
 * (nothing in the reference, which presents RGBA8). An ADD-ON: plain C with <stddef.h> and <stdint.h> alone, no other
 * header of the project; its symbols are exported from libpar_screen.so, not from libpar_raytracer.so or libpar_vram.so,
 * and the statuses it returns are the values of par_raytracer.h's par_status (PAR_OK 0, PAR_ERR_INVALID_ARG 1,
 * PAR_ERR_NO_DEVICE 2, PAR_ERR_HIP 3, PAR_ERR_OOM 4).
 *
 * par_vram.h ends the chain in the bytes a machine loads: tile data in bit planes or nibbles, map words, colour words.
 * This header reads them back: a tile map with wrap-around scroll and per-scanline scroll, tile data in the machine's
 * format, colour words widened to RGBA8, and the rule that a tile pixel of value 0 shows ONE backdrop colour whatever the
 * cell's sub-palette. It is the measurement of what the export shows, the scrolling of a frame rendered once, and the way
 * back for tile data and maps that come from a ROM. What par_vram.h says of formats, words and colours is RESTATED here,
 * not included; the enumerations have equal values and par_screen_map_layout is par_vram_map_layout field for field (same
 * names, order, meaning and rules), so a caller that includes both may cast one to the other.
 *
 * Every device call: asynchronous on `stream` (a hipStream_t); allocates nothing, waits for nothing, keeps no state and
 * can be captured into a graph; integers only; its outputs depend on nothing but its inputs (a count is a sum of integers,
 * which has no order); at most one fill (the four bytes of a bad_out, to 0) and ONE launch; PAR_ERR_INVALID_ARG before any
 * device work, with nothing written and with no GPU present.
 *
 * 1. The descriptor. par_screen_desc is int32_t fields alone, 108 bytes, no padding:
 *     the eleven fields of the layout (section 3);
 *     tile_w, tile_h        8 or 16
 *     tile_format           a par_screen_tile_format (section 2)
 *     n_tiles               1 to PAR_SCREEN_MAX_TILES: the tiles at `chr`
 *     map_w, map_h          cells, each at least 1, product at most PAR_SCREEN_MAX_CELLS
 *     ratio_x, ratio_y      1 or 2, used with `attr`
 *     pal_format            a par_screen_palette_format (section 4)
 *     n_colors              1 to 256: the entries at `pal_words`
 *     sub_size              K, 1 to 256: the entries of a sub-palette
 *     backdrop              0 or 1
 *     width, height         the screen in pixels, 1 to PAR_SCREEN_MAX_SIDE each
 *     scroll_x, scroll_y    any int32_t
 * It is read on the host, at the call.
 *
 * 2. Tile formats. `chr` is n_tiles tiles of par_screen_tile_bytes(format, tile_w, tile_h) bytes each, no alignment
 * beyond a byte. A tile 16 wide or high is its 8 x 8 sub-tiles one after the other, row-major over sub-tiles: left then
 * right, top pair then bottom pair. For a sub-tile, pixel (x, y) with value v, bit b of v written v_b:
 *     format                                          bpp  bytes  where v_b is
 *     PAR_SCREEN_1BPP                                  1     8    byte y, bit 7 - x
 *     PAR_SCREEN_2BPP_PLANAR      (NES)                2    16    byte 8 b + y, bit 7 - x
 *     PAR_SCREEN_2BPP_ROWS        (Game Boy, SNES 2bpp) 2   16    byte 2 y + b, bit 7 - x
 *     PAR_SCREEN_4BPP_ROWS        (SNES 4bpp)          4    32    byte 16 (b >> 1) + 2 y + (b & 1), bit 7 - x
 *     PAR_SCREEN_4BPP_PACKED_HI   (Mega Drive)         4    32    byte 4 y + (x >> 1); the high nibble for even x, the
 *                                                                 low nibble for odd x
 *     PAR_SCREEN_4BPP_PACKED_LO   (GBA 4bpp)           4    32    the same byte, low nibble for even x
 *     PAR_SCREEN_4BPP_ROW_PLANES  (Master System)      4    32    byte 4 y + b, bit 7 - x
 * par_screen_tile_bytes = bytes * (tile_w / 8) * (tile_h / 8), 0 outside the limits.
 *
 * 3. Map words. par_screen_map_layout says where a machine's map word keeps what: word_bytes (1, 2 or 4), big_endian (0
 * or 1), tile_shift and tile_bits (>= 1), pal_shift and pal_bits (>= 0), flip_x_bit and flip_y_bit (-1: the machine has
 * none), tile_step (1 to 16), tile_base (0 to 65535) and set_bits (within the word; IGNORED when a word is read). Every
 * field must lie within the word; overlaps between fields are the caller's business. `map_words` is map_w * map_h words
 * of word_bytes bytes in the stated byte order, cell c at map_words + c * word_bytes, no alignment beyond a byte. Of a
 * word w: t = (w >> tile_shift) & (2^tile_bits - 1), p = (w >> pal_shift) & (2^pal_bits - 1), fx and fy the flip bits, 0
 * where the layout has none. The tile is id = (t - tile_base) / tile_step, and the cell is BAD when t < tile_base, when
 * the division leaves a remainder, or (for a draw) when id >= n_tiles. The known layouts (tile_step 1, tile_base 0):
 *     machine       bytes  byte order  tile (shift / bits)  palette  x flip  y flip
 *     NES             1       -            0 / 8            none     none    none
 *     GBC             2     little         0 / 8            8 / 3     13      14
 *     SMS             2     little         0 / 9            11 / 1     9      10
 *     Mega Drive      2     BIG            0 / 11           13 / 2    11      12
 *     SNES            2     little         0 / 10           10 / 3    14      15
 *     GBA             2     little         0 / 10           12 / 4    10      11
 * Anchors: tile 5, palette 3, x flip is 0x4C05 (bytes 05 4C) on the SNES, 0x6805 (bytes 68 05) on the Mega Drive and
 * 0x3405 (bytes 05 34) on the GBA.
 *
 * 4. Colour words. `pal_words` is n_colors entries, no alignment beyond a byte:
 *     PAR_SCREEN_BGR555     2 bytes, little-endian   r = w & 31, g = (w >> 5) & 31, b = (w >> 10) & 31     5 bits each
 *     PAR_SCREEN_BGR333_MD  2 bytes, BIG-endian      r = (w >> 1) & 7, g = (w >> 5) & 7, b = (w >> 9) & 7  3 bits each
 *     PAR_SCREEN_BGR222     1 byte                   r = w & 3, g = (w >> 2) & 3, b = (w >> 4) & 3         2 bits each
 *     PAR_SCREEN_RGBA8      4 bytes: red, green, blue as they are; the fourth byte is not shown
 * Widening a field q to eight bits is bit replication:
 *     5 bits   q << 3 | q >> 2
 *     3 bits   q << 5 | q << 2 | q >> 1
 *     2 bits   q * 0x55
 * so the largest field is 255 and 0 is 0. Alpha is 255 in every format. par_screen_palette_rgba is this table on the
 * host: n entries (1 to 256) of `format` at `words` to 4 n bytes red, green, blue, 255 at rgba_out; it returns the bytes
 * written, or 0 for a bad argument (a null pointer, n or format outside the limits), with nothing written.
 *
 * 5. The pixel, in integers. For screen pixel (x, y), with mathematical (floor) modulo and sums that do not overflow:
 *     mx = (x + scroll_x + lx) mod (map_w * tile_w),  my = (y + scroll_y + ly) mod (map_h * tile_h)
 * where (lx, ly) = (line_scroll[2 y], line_scroll[2 y + 1]), or (0, 0) when line_scroll is null. line_scroll is nullable,
 * 2 * height words, aligned to 4 bytes: per-scanline scroll, what parallax is made of. The cell is (cx, cy) =
 * (mx / tile_w, my / tile_h), c = cx + cy * map_w; t, p, fx, fy and id come from its word (section 3). When `attr` is
 * given, p is instead the byte attr[(cx / ratio_x) + (cy / ratio_y) * ceil(map_w / ratio_x)]: the NES attribute grid, and
 * the cell_out of par_quantize_cells_device as it stands. `attr` is ceil(map_w / ratio_x) * ceil(map_h / ratio_y) bytes.
 * For a good cell the tile pixel is (mx mod tile_w, my mod tile_h), mirrored to (tile_w - 1 - x, .) by fx and to
 * (., tile_h - 1 - y) by fy; its value v is read from tile id's bytes at chr + id * tile_bytes (section 2). The colour
 * index is i = min(p * K + v, n_colors - 1), the clamp of par_present_device; with backdrop 1 and v == 0, i = 0. A bad
 * cell shows i = 0.
 * Outputs: index_out (nullable, width * height bytes, dense, no alignment beyond a byte) gets i; fb_out (nullable,
 * 4 * width * height bytes, dense, aligned to 4 bytes) gets entry i widened: red, green, blue, 255. Not both may be null.
 * pal_words is not read, and may be null, when fb_out is null. bad_out (nullable, a uint32_t aligned to 4 bytes) gets the
 * number of bad cells of the WHOLE map, visible or not, each once; it is always written when given.
 *
 * 6. par_screen_decode_map_device inverts par_vram_encode_map_device at ratio 1, for n_cells (1 to PAR_SCREEN_MAX_CELLS)
 * words: map_out[c] = id | fx << 30 | fy << 31 (uint32_t words aligned to 4 bytes, what par_tileset_expand_device reads)
 * and pal_out[c] = p & 255 (nullable, a byte a cell). Bad cells are those of section 3 without the n_tiles condition, and
 * an id of 2^30 or more, which map_out cannot hold; they get id 0, keep their flips and palette, and are counted in
 * bad_out (nullable, aligned to 4 bytes). par_tileset_expand_device and the rest of the chain then work on ROM data.
 *
 * Consequences, each held by a test:
 *   1. The closing identity. A cells index plane of width and height that are multiples of the tile size; its local plane
 *      (par_vram_local_device), a tile set built under any flip mask, par_vram_encode_tiles_device,
 *      par_vram_encode_map_device with cell_out; pal_format PAR_SCREEN_RGBA8 over the cells call's table, backdrop 0,
 *      scroll 0 and a screen the size of the frame: index_out is the cells index plane and fb_out is the cells call's
 *      fb_out with alpha 255, byte for byte. For ragged frames the same holds over width x height with `pad` 0.
 *   2. A scroll by whole map periods (map_w * tile_w, map_h * tile_h) changes nothing.
 *   3. A scroll of (s, 0) equals a line_scroll of (s, 0) on every row.
 *   4. Setting fx in a word whose tile is stored mirrored left to right changes nothing; the same for fy.
 *   5. With backdrop 1 the picture differs from backdrop 0 exactly at the pixels with v == 0 in cells with p > 0 (as
 *      indices; where min(p * K, n_colors - 1) is not 0).
 *   6. A draw through pal_format f equals a draw through PAR_SCREEN_RGBA8 over par_screen_palette_rgba(words, f).
 *   7. decode_map(encode_map(m)) gives m and the cells bytes wherever encode_map counted nothing bad.
 *
 * PAR_ERR_INVALID_ARG, before any device work, with nothing written and without a GPU present, for: a null `desc`,
 * `layout`, `chr`, `map_words` or `map_out`; fb_out and index_out both null; a null pal_words with an fb_out; a
 * line_scroll, fb_out, map_out or bad_out that is not aligned to 4 bytes; any value outside the limits above; and for the
 * host forms a null `bad`.
 * Left out on purpose: sprites and OAM; several layers and priority; windows and mosaic; 8bpp and affine backgrounds; the
 * SNES 16 x 16 tile numbering; the GBC bank bit; mid-line register changes other than scroll; the NES's fixed master
 * palette as colour words (a caller draws the NES through PAR_SCREEN_RGBA8 over its table); and changing the fit so that
 * the backdrop and the colour depth stop costing error: that is the next add-on, and this call is what will measure it.
 */
#ifndef PAR_SCREEN_H
#define PAR_SCREEN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAR_SCREEN_MAX_TILES (1 << 20)
#define PAR_SCREEN_MAX_CELLS (1 << 20)
#define PAR_SCREEN_MAX_SIDE 4096

enum par_screen_tile_format {
    PAR_SCREEN_1BPP = 0,
    PAR_SCREEN_2BPP_PLANAR = 1,
    PAR_SCREEN_2BPP_ROWS = 2,
    PAR_SCREEN_4BPP_ROWS = 3,
    PAR_SCREEN_4BPP_PACKED_HI = 4,
    PAR_SCREEN_4BPP_PACKED_LO = 5,
    PAR_SCREEN_4BPP_ROW_PLANES = 6
};

enum par_screen_palette_format { PAR_SCREEN_BGR555 = 0, PAR_SCREEN_BGR333_MD = 1, PAR_SCREEN_BGR222 = 2, PAR_SCREEN_RGBA8 = 3 };

/* int32_t fields alone: 44 bytes, no padding; par_vram_map_layout field for field */
typedef struct par_screen_map_layout {
    int32_t word_bytes, big_endian;
    int32_t tile_shift, tile_bits;
    int32_t pal_shift, pal_bits;
    int32_t flip_x_bit, flip_y_bit;
    int32_t tile_step, tile_base;
    int32_t set_bits;
} par_screen_map_layout;

/* int32_t fields alone: 108 bytes, no padding */
typedef struct par_screen_desc {
    par_screen_map_layout layout;
    int32_t tile_w, tile_h;
    int32_t tile_format;
    int32_t n_tiles;
    int32_t map_w, map_h;
    int32_t ratio_x, ratio_y;
    int32_t pal_format;
    int32_t n_colors;
    int32_t sub_size;
    int32_t backdrop;
    int32_t width, height;
    int32_t scroll_x, scroll_y;
} par_screen_desc;

/* Host arithmetic: the bytes of one tile_w x tile_h tile in `format`, 0 outside the limits. */
size_t par_screen_tile_bytes(int format, int tile_w, int tile_h);
/* Host arithmetic: the n entries of `words` in `format` widened to red, green, blue, 255 at rgba_out; the bytes written, 0
 * for a bad argument. */
size_t par_screen_palette_rgba(const uint8_t* words, int n, int format, uint8_t* rgba_out);
/* device pointers (`desc` is read on the host, at the call), asynchronous on `stream`: a fill of bad_out when given, one
 * launch of a thread an eight-pixel segment of a tile row */
int par_screen_draw_device(void* stream, const par_screen_desc* desc, const uint8_t* chr, const uint8_t* map_words,
                           const uint8_t* attr, const uint8_t* pal_words, const int32_t* line_scroll, uint8_t* fb_out,
                           uint8_t* index_out, uint32_t* bad_out);
/* device pointers (`layout` is read on the host, at the call), asynchronous on `stream`: a fill of bad_out when given, one
 * launch of a thread a cell */
int par_screen_decode_map_device(void* stream, const par_screen_map_layout* layout, const uint8_t* map_words, int n_cells,
                                 uint32_t* map_out, uint8_t* pal_out, uint32_t* bad_out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device): allocate, copy, launch,
 * synchronise, copy back and free. The bad count comes back through `bad`, which is not nullable.
 * PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as par_quantize_cells_host */
int par_screen_draw_host(int device, const par_screen_desc* desc, const uint8_t* chr, const uint8_t* map_words,
                         const uint8_t* attr, const uint8_t* pal_words, const int32_t* line_scroll, uint8_t* fb_out,
                         uint8_t* index_out, int* bad);
int par_screen_decode_map_host(int device, const par_screen_map_layout* layout, const uint8_t* map_words, int n_cells,
                               uint32_t* map_out, uint8_t* pal_out, int* bad);

#ifdef __cplusplus
}
#endif

#endif
