/*
 * par_vram.h — VRAM export: a tile set, its map and its palette packed into the formats tile hardware loads (nothing in
 * the reference, which presents RGBA8). An ADD-ON: plain C with <stddef.h> and <stdint.h> alone, no other header of the
 * project; its symbols are exported from libpar_vram.so, not from libpar_raytracer.so, and the statuses it returns are the
 * values of par_raytracer.h's par_status (PAR_OK 0, PAR_ERR_INVALID_ARG 1, PAR_ERR_NO_DEVICE 2, PAR_ERR_HIP 3,
 * PAR_ERR_OOM 4).
 *
 * The chain so far ends in a tile set of one byte a pixel that holds flat-table indices s * K + k, a 32-bit map word of the
 * project's own and RGBA8 palette entries. A machine wants the pixel's k alone in a tile, packed into bit planes or
 * nibbles, the sub-palette number s in the map word beside the tile number and the flips, and its palette in a few bits a
 * channel. These calls are passes over finished planes, sets and maps, whatever made them; they take no context and no
 * par_params.
 *
 * Every device call: asynchronous on `stream` (a hipStream_t); allocates nothing, waits for nothing, keeps no state and
 * can be captured into a graph; integers only; its outputs depend on nothing but its inputs (a count is a sum of integers,
 * which has no order); at most one fill (the four bytes of a bad_out, to 0) and ONE launch; PAR_ERR_INVALID_ARG before any
 * device work, with nothing written and with no GPU present.
 *
 * 1. The local plane. par_vram_local_device: local_out[i] = index[i] % sub_size, for n_bytes bytes; sub_size in [1, 256],
 * n_bytes in [1, 2^31 - 1], neither pointer aligned beyond a byte; in place (local_out == index) is allowed, any other
 * overlap is not checked. The index plane of par_quantize_cells_device holds s * K + k, so % K is what a tile stores and
 * / K is that call's cell_out. par_tileset_build_device or par_tileset_extend_device on the local plane is the dedupe
 * MODULO THE PALETTE: two cells with one pattern under different sub-palettes are one tile, as on the machine.
 * Consequence: the tile count of the local plane never exceeds that of the flat plane, under every flip mask (flips
 * commute with an elementwise map, so equal flat canonical forms imply equal local ones).
 *
 * 2. Tile formats. `tiles` is `capacity` tiles of tile_w * tile_h bytes, row-major, as build, extend and reduce write
 * them; tile_w and tile_h are each 8 or 16; capacity in [1, PAR_VRAM_MAX_TILES]. `count` is a uint32_t in DEVICE memory,
 * the one those calls write, aligned to 4 bytes; a null count means all `capacity` tiles. The call encodes
 * n = min(*count, capacity) tiles, and no byte of `out` beyond n tiles is written. `tiles` and `out` need no alignment
 * beyond a byte.
 * Sub-tiles: a tile 16 wide or high is its 8 x 8 sub-tiles one after the other, row-major over sub-tiles: left then
 * right, top pair then bottom pair. For 8 x 16 this is the NES and Game Boy tall-sprite order.
 * Bit layout: for a sub-tile, pixel (x, y) with value v, bit b of v written v_b:
 *     format                                        bpp  bytes  where v_b goes
 *     PAR_VRAM_1BPP                                  1     8    byte y, bit 7 - x
 *     PAR_VRAM_2BPP_PLANAR      (NES)                2    16    byte 8 b + y, bit 7 - x
 *     PAR_VRAM_2BPP_ROWS        (Game Boy, SNES 2bpp) 2   16    byte 2 y + b, bit 7 - x
 *     PAR_VRAM_4BPP_ROWS        (SNES 4bpp)          4    32    byte 16 (b >> 1) + 2 y + (b & 1), bit 7 - x
 *     PAR_VRAM_4BPP_PACKED_HI   (Mega Drive)         4    32    byte 4 y + (x >> 1); v & 15 in the high nibble for even x,
 *                                                               the low nibble for odd x
 *     PAR_VRAM_4BPP_PACKED_LO   (GBA 4bpp)           4    32    the same byte, low nibble for even x
 *     PAR_VRAM_4BPP_ROW_PLANES  (Master System)      4    32    byte 4 y + b, bit 7 - x
 * par_vram_tile_bytes(format, tile_w, tile_h) = bytes * (tile_w / 8) * (tile_h / 8).
 * Values too large: only the low bpp bits of a byte are encoded. bad_out is a nullable uint32_t aligned to 4 bytes; it
 * gets the number of tiles among the n that hold a byte >= 2^bpp, is always written when given and is 0 for a clean set.
 * Decode is the inverse for n_tiles given on the host (a ROM's tile data has no device count; n_tiles in
 * [1, PAR_VRAM_MAX_TILES]): bytes in, one byte a pixel out, every byte < 2^bpp.
 *     decode(encode(t)) == t & (2^bpp - 1) for every set, and encode(decode(d)) == d for every byte string d.
 * Hand-worked anchors, each a tile that is 0 elsewhere:
 *     1BPP, value 1 at (0, 0): byte 0 is 0x80.
 *     2BPP_ROWS, value 3 at (0, 0): bytes 0 and 1 are 0x80.
 *     2BPP_ROWS, value 2 at (7, 0): byte 0 is 0x00 and byte 1 is 0x01.
 *     2BPP_PLANAR, value 2 at (7, 3): byte 11 is 0x01, everything else is 0.
 *     4BPP_ROWS, value 0xA at (0, 0): bytes 1 and 17 are 0x80.
 *     Packed, 0xA at (0, 0) and 0x5 at (1, 0): byte 0 is 0xA5 for HI and 0x5A for LO.
 *     4BPP_ROW_PLANES, value 0xA at (0, 0): bytes 1 and 3 are 0x80.
 *
 * 3. Map words. par_vram_map_layout says where a machine's map word keeps what: word_bytes (1, 2 or 4), big_endian (0 or
 * 1), tile_shift and tile_bits (>= 1), pal_shift and pal_bits (>= 0), flip_x_bit and flip_y_bit (-1: the machine has
 * none), tile_step (1 to 16), tile_base (0 to 65535) and set_bits. Every field must lie within the word; overlaps between
 * fields are the caller's business.
 * `map` is gcx * gcy words of build, extend or reduce, id | fx << 30 | fy << 31, aligned to 4 bytes; gcx * gcy is at most
 * PAR_VRAM_MAX_CELLS. `cells` is nullable (null: the palette is 0) and is the cell_out of par_quantize_cells_device, a
 * byte a colour cell: the colour cell of tile cell (tx, ty) is (tx / ratio_x) + (ty / ratio_y) * ceil(gcx / ratio_x);
 * ratio_x and ratio_y are 1 or 2, and a ratio of 2 covers 16 x 16 colour cells over 8 x 8 tiles, the NES attribute grid.
 * The word: with t = id * tile_step + tile_base and p the cell's byte,
 *     w = (t & (2^tile_bits - 1)) << tile_shift | (p & (2^pal_bits - 1)) << pal_shift
 *       | fx << flip_x_bit | fy << flip_y_bit | set_bits
 * where a flip term is present only where the layout has that bit. The word is stored in word_bytes bytes in the stated
 * byte order at out + c * word_bytes; `out` needs no alignment beyond a byte.
 * bad_out (nullable, aligned to 4 bytes) counts the CELLS where one of these holds: t >= 2^tile_bits; p >= 2^pal_bits; a
 * flip is set that the layout has no bit for. A cell that is bad twice over counts once.
 * par_vram_map_layout_preset fills the known layouts (tile_step 1, tile_base 0, set_bits 0):
 *     machine              bytes  byte order  tile (shift / bits)  palette  x flip  y flip
 *     PAR_VRAM_NES           1       -            0 / 8            none     none    none
 *     PAR_VRAM_GBC           2     little         0 / 8            8 / 3     13      14
 *     PAR_VRAM_SMS           2     little         0 / 9            11 / 1     9      10
 *     PAR_VRAM_MEGADRIVE     2     BIG            0 / 11           13 / 2    11      12
 *     PAR_VRAM_SNES          2     little         0 / 10           10 / 3    14      15
 *     PAR_VRAM_GBA           2     little         0 / 10           12 / 4    10      11
 * For the Game Boy Color the low byte is the tile map and the high byte is the attribute map; the machine keeps the two in
 * separate banks, so the caller de-interleaves them.
 * Anchors: tile 5, palette 3, x flip. SNES: 0x4C05, bytes 05 4C. Mega Drive: 0x6805, bytes 68 05. GBA: 0x3405, bytes
 * 05 34. NES: byte 05, and the cell counts as bad twice over, once for the palette and once for the flip; bad_out counts
 * cells, so it is 1.
 *
 * 4. Palette words. par_vram_palette_words is host arithmetic only, from n four-byte entries red, green, blue, alpha
 * (n in [1, 256]; a table is at most 1 KiB, so the caller copies it):
 *     PAR_VRAM_BGR555     (SNES, GBC, GBA; 2 bytes, little-endian)   r >> 3 | (g >> 3) << 5 | (b >> 3) << 10
 *     PAR_VRAM_BGR333_MD  (2 bytes, big-endian)                      (r >> 5) << 1 | (g >> 5) << 5 | (b >> 5) << 9
 *     PAR_VRAM_BGR222     (SMS; 1 byte)                              r >> 6 | (g >> 6) << 2 | (b >> 6) << 4
 * It returns the bytes written, or 0 for a bad argument. Truncation changes the colours shown: a caller who wants the
 * fit's error to be the machine's rounds the master palette to the machine's depth first.
 *
 * PAR_ERR_INVALID_ARG, before any device work, with nothing written and without a GPU present, for: a null `index`,
 * `local_out`, `tiles`, `out`, `data`, `tiles_out`, `layout` or `map`; a `count`, `bad_out` or `map` that is not aligned to
 * 4 bytes; any value outside the limits above; a format or machine that is not one of the enumerations; and for the host
 * forms a negative count or a null `bad`.
 * Left out on purpose: NES attribute-table packing (64 bytes a screen, a host loop over cell_out); a shared backdrop
 * colour across sub-palettes; the SNES 16 x 16 tile numbering; the GBC bank bit; sprites and OAM; 8bpp (one byte a pixel
 * is the tile set as it is); rounding the master to the machine's colour depth.
 */
#ifndef PAR_VRAM_H
#define PAR_VRAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAR_VRAM_MAX_TILES (1 << 20)
#define PAR_VRAM_MAX_CELLS (1 << 20)

enum par_vram_tile_format {
    PAR_VRAM_1BPP = 0,
    PAR_VRAM_2BPP_PLANAR = 1,
    PAR_VRAM_2BPP_ROWS = 2,
    PAR_VRAM_4BPP_ROWS = 3,
    PAR_VRAM_4BPP_PACKED_HI = 4,
    PAR_VRAM_4BPP_PACKED_LO = 5,
    PAR_VRAM_4BPP_ROW_PLANES = 6
};

enum par_vram_machine {
    PAR_VRAM_NES = 0,
    PAR_VRAM_GBC = 1,
    PAR_VRAM_SMS = 2,
    PAR_VRAM_MEGADRIVE = 3,
    PAR_VRAM_SNES = 4,
    PAR_VRAM_GBA = 5
};

enum par_vram_palette_format { PAR_VRAM_BGR555 = 0, PAR_VRAM_BGR333_MD = 1, PAR_VRAM_BGR222 = 2 };

/* int32_t fields alone: 44 bytes, no padding */
typedef struct par_vram_map_layout {
    int32_t word_bytes, big_endian;
    int32_t tile_shift, tile_bits;
    int32_t pal_shift, pal_bits;
    int32_t flip_x_bit, flip_y_bit;
    int32_t tile_step, tile_base;
    int32_t set_bits;
} par_vram_map_layout;

/* Host arithmetic: the bytes of one tile_w x tile_h tile in `format`, 0 outside the limits. */
size_t par_vram_tile_bytes(int format, int tile_w, int tile_h);
/* device pointers, asynchronous on `stream`: no fill, one launch */
int par_vram_local_device(void* stream, const uint8_t* index, int n_bytes, int sub_size, uint8_t* local_out);
/* device pointers (`count` too), asynchronous on `stream`: a fill of bad_out when given, one launch of a wavefront a
 * sub-tile, sized by `capacity`; a wavefront past n tiles does nothing */
int par_vram_encode_tiles_device(void* stream, const uint8_t* tiles, int capacity, const uint32_t* count, int tile_w,
                                 int tile_h, int format, uint8_t* out, uint32_t* bad_out);
/* device pointers, asynchronous on `stream`: no fill, one launch */
int par_vram_decode_tiles_device(void* stream, const uint8_t* data, int n_tiles, int tile_w, int tile_h, int format,
                                 uint8_t* tiles_out);
/* Host arithmetic: the layout of `machine`; PAR_ERR_INVALID_ARG for a null layout or an unknown machine. */
int par_vram_map_layout_preset(int machine, par_vram_map_layout* layout);
/* device pointers (`layout` is read on the host, at the call), asynchronous on `stream`: a fill of bad_out when given, one
 * launch of a thread a cell */
int par_vram_encode_map_device(void* stream, const par_vram_map_layout* layout, const uint32_t* map, int gcx, int gcy,
                               const uint8_t* cells, int ratio_x, int ratio_y, uint8_t* out, uint32_t* bad_out);
/* Host arithmetic: the n entries of `palette` as words of `format` to `out`; the bytes written, 0 for a bad argument. */
size_t par_vram_palette_words(const uint8_t* palette, int n, int format, uint8_t* out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device): allocate, copy, launch,
 * synchronise, copy back and free. The count is a plain int (0 <= count; min(count, capacity) tiles are encoded and that
 * many tiles of `out` written) and the bad count comes back through `bad`, which is not nullable.
 * PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as par_quantize_cells_host */
int par_vram_encode_tiles_host(int device, const uint8_t* tiles, int capacity, int count, int tile_w, int tile_h,
                               int format, uint8_t* out, int* bad);
int par_vram_decode_tiles_host(int device, const uint8_t* data, int n_tiles, int tile_w, int tile_h, int format,
                               uint8_t* tiles_out);
int par_vram_encode_map_host(int device, const par_vram_map_layout* layout, const uint32_t* map, int gcx, int gcy,
                             const uint8_t* cells, int ratio_x, int ratio_y, uint8_t* out, int* bad);

#ifdef __cplusplus
}
#endif

#endif
