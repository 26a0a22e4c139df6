/*
 * par_objects.h — Objects: a tile machine's sprite layer drawn over its background from tile bytes and an object table, and
 * the object table a frame needs over a kept background (nothing in the reference, which redraws every frame). An ADD-ON:
 * plain C with <stddef.h> and <stdint.h> alone, no other header of the project; its symbols are exported from
 * libpar_objects.so, not from libpar_raytracer.so or another add-on's library, and the statuses it returns are the values of
 * par_raytracer.h's par_status (PAR_OK 0, PAR_ERR_INVALID_ARG 1, PAR_ERR_NO_DEVICE 2, PAR_ERR_HIP 3, PAR_ERR_OOM 4).
 *
 * par_screen.h draws one background layer and leaves out "sprites and OAM". OAM (object attribute memory) is the machine's
 * table of sprites, here OBJECTS. No machine of the presets shows a moving thing by rewriting its background: the level
 * stays in VRAM and what moves is an object drawn over it. What par_screen.h says of tile formats (its section 2), colour
 * words (4) and flips (5), and par_vram.h of machines, is RESTATED here, not included; the enumerations have equal values.
 *
 * Every device call: asynchronous on `stream` (a hipStream_t); allocates nothing, waits for nothing, keeps no state in its
 * work block (a dirty block is fine, and a block may serve any number of calls one after the other) and can be captured into
 * a graph; integers only; its outputs depend on nothing but its inputs (a count is a sum of integers, which has no order,
 * and no order of anything else depends on the order the device runs anything in); PAR_ERR_INVALID_ARG before any device
 * work, with nothing written and with no GPU present.
 *
 * 1. The record. par_object is four int32_t, 16 bytes: x, y, tile, attr. (x, y) is the screen position of its top-left
 * pixel. Of attr: bits 0 to 7 the sub-palette p, bit 8 fx, bit 9 fy, bit 10 `behind`, bit 11 `hidden`; higher bits are
 * ignored. An object that is not hidden is BAD, and treated as hidden, when tile < 0, when tile >= n_tiles, or when x or y
 * lies outside [-32768, 32767]. The other objects that are not hidden are LIVE.
 *
 * 2. The descriptor. par_objects_desc is int32_t fields alone, 56 bytes, no padding:
 *     tile_w, tile_h        8 or 16: one object size a call, as the NES and the Game Boy have one mode
 *     tile_format           a par_objects_tile_format (section 3)
 *     n_tiles               1 to PAR_OBJECTS_MAX_TILES (2^20): the tiles at `chr`
 *     n_objects             1 to PAR_OBJECTS_MAX (65536): the records at `objects`
 *     line_limit            1 to PAR_OBJECTS_MAX_LINE (128): the objects a scanline shows
 *     pal_format            a par_objects_palette_format (section 4)
 *     n_colors              1 to 256: the entries at `pal_words`
 *     sub_size              K, 1 to 256: the entries of a sub-palette
 *     pal_base              0 to 255: where the objects' sub-palettes start in the colour words, as on the SNES and the GBA
 *     bg_sub_size           1 to 256: the K of the background whose indices are at `bg_index`
 *     opaque                0 or 1
 *     width, height         the screen in pixels, 1 to PAR_OBJECTS_MAX_SIDE (4096) each
 * It is read on the host, at the call.
 *
 * 3. Tile formats (par_screen.h section 2, restated). `chr` is n_tiles tiles of tile_bytes bytes each (below), no
 * alignment beyond a byte. A tile 16 wide or high is its 8 x 8 sub-tiles one after the other, row-major over sub-tiles: left
 * then right, top pair then bottom pair. For a sub-tile, pixel (x, y) with value v, bit b of v written v_b:
 *     format                                bpp  bytes  where v_b is
 *     PAR_OBJECTS_1BPP                       1     8    byte y, bit 7 - x
 *     PAR_OBJECTS_2BPP_PLANAR (NES)          2    16    byte 8 b + y, bit 7 - x
 *     PAR_OBJECTS_2BPP_ROWS (Game Boy)       2    16    byte 2 y + b, bit 7 - x
 *     PAR_OBJECTS_4BPP_ROWS (SNES)           4    32    byte 16 (b >> 1) + 2 y + (b & 1), bit 7 - x
 *     PAR_OBJECTS_4BPP_PACKED_HI (Mega Drive) 4   32    byte 4 y + (x >> 1); the high nibble for even x, the low for odd x
 *     PAR_OBJECTS_4BPP_PACKED_LO (GBA)       4    32    the same byte, low nibble for even x
 *     PAR_OBJECTS_4BPP_ROW_PLANES (SMS)      4    32    byte 4 y + b, bit 7 - x
 * The bytes of a tile are bytes * (tile_w / 8) * (tile_h / 8).
 *
 * 4. Colour words (par_screen.h section 4, restated). `pal_words` is n_colors entries, no alignment beyond a byte:
 *     PAR_OBJECTS_BGR555     2 bytes, little-endian   r = w & 31, g = (w >> 5) & 31, b = (w >> 10) & 31     5 bits each
 *     PAR_OBJECTS_BGR333_MD  2 bytes, BIG-endian      r = (w >> 1) & 7, g = (w >> 5) & 7, b = (w >> 9) & 7  3 bits each
 *     PAR_OBJECTS_BGR222     1 byte                   r = w & 3, g = (w >> 2) & 3, b = (w >> 4) & 3         2 bits each
 *     PAR_OBJECTS_RGBA8      4 bytes: red, green, blue as they are; the fourth byte is not shown
 * Widening a field q to eight bits is bit replication: 5 bits q << 3 | q >> 2, 3 bits q << 5 | q << 2 | q >> 1, 2 bits
 * q * 0x55. Alpha is 255 in every format.
 *
 * 5. par_objects_draw_device. `count` is a nullable uint32_t in device memory, aligned to 4 bytes, as in
 * par_vram_encode_tiles_device: the call uses n = min(*count, n_objects) records; null means n_objects.
 * The LINE LIST of scanline y (0 <= y < height) is the live objects j < n with y_j <= y < y_j + tile_h, whatever their x, in
 * ascending j. The first line_limit of the list are SHOWN on the line; the rest are DROPPED. over_out (nullable uint32_t,
 * aligned to 4 bytes) gets the sum over the screen's scanlines of the objects dropped; bad_out (the same) gets the bad
 * objects among the n. Both are always written when given.
 * Pixel (x, y): walk the line's shown objects in ascending j. An object covers x when x_j <= x < x_j + tile_w. Its tile
 * pixel is (x - x_j, y - y_j), mirrored to (tile_w - 1 - ., .) by fx and to (., tile_h - 1 - .) by fy (par_screen.h section
 * 5, restated); its value v is read from tile `tile`'s bytes at chr + tile * tile_bytes (section 3). The WINNER is the first
 * covering object with v != 0, or the first covering object at all when `opaque` is 1. With no winner the pixel is not
 * written in either plane. If the winner has `behind` set, bg_index is given, and bg_index[y * width + x] % bg_sub_size
 * != 0, the pixel is not written either: a behind object of low index MASKS a front object of higher index, which is the
 * NES's and the Game Boy's rule (the priority among objects is decided first, and the winner alone meets the background).
 * Otherwise i = min(pal_base + p * K + v, n_colors - 1); index_io gets i, and fb_io gets entry i widened (section 4): red,
 * green, blue, 255.
 * fb_io (RGBA8, 4 * width * height bytes, aligned to 4 bytes) and index_io (a byte a pixel, no alignment) are dense,
 * nullable, and not both null; both are read-modify-write: a pixel that is not written keeps its bytes. pal_words is not
 * read, and may be null, without fb_io. bg_index is a nullable const plane of width * height bytes; it may be index_io
 * itself; any other overlap is not checked. `work` is par_objects_work_bytes(height, line_limit) bytes, aligned to 4:
 *     par_objects_work_bytes = 4 * height * (1 + line_limit)     (a count a line, then line_limit indices a line)
 * 0 outside the limits. Launch budget: at most two four-byte fills (bad_out, over_out) and TWO launches: a wavefront a
 * scanline builds the line lists, then a thread takes eight consecutive pixels of a row.
 *
 * 6. par_objects_from_maps_device makes the objects a frame needs over a kept background. map_bg and map are gcx * gcy
 * words id | fx << 30 | fy << 31 of par_tileset_build_device, par_tileset_extend_device or par_tileset_reduce_device,
 * aligned to 4 bytes, both numbered against ONE set, which is what par_tileset_extend_device gives; gcx * gcy is at most
 * PAR_OBJECTS_MAX_CELLS (2^20). cells_bg and cells are a byte a cell, both given or both null. Cell c DIFFERS when the two
 * words differ as whole words, or when the two bytes differ. With D the number of differing cells, the first
 * min(D, capacity) of them in ascending c become records, cell c = cx + cy * gcx:
 *     x = x0 + cx * tile_w,  y = y0 + cy * tile_h,  tile = map[c] & 0x3FFFFFFF,  attr = cells[c] | fx << 8 | fy << 9
 * with p 0 when `cells` is null. count_out (a device uint32_t aligned to 4 bytes, not null) gets D, always; records from
 * min(D, capacity) on are not written. capacity is 1 to PAR_OBJECTS_MAX; tile_w and tile_h are 8 or 16; the positions must
 * lie within [-32768, 32767] for every cell of the grid. `work` is par_objects_from_maps_work_bytes(n_cells) bytes, aligned
 * to 4:
 *     par_objects_from_maps_work_bytes = 4 * ceil(n_cells / 1024)     (a count, then a base, a workgroup of 1024 cells)
 * 0 outside the limits. Launch budget: no fill and three launches (count, scan, scatter). The order is the cells' order:
 * ranks come from ballots and prefix popcounts, no atomic places anything.
 *
 * 7. Host arithmetic. par_objects_machine_limits gives the machines' nominal figures, objects a scanline / objects in all:
 *     PAR_OBJECTS_NES 8 / 64, PAR_OBJECTS_GBC 10 / 40, PAR_OBJECTS_SMS 8 / 64, PAR_OBJECTS_MEGADRIVE 20 / 80,
 *     PAR_OBJECTS_SNES 32 / 128, PAR_OBJECTS_GBA 128 / 128
 * (the values of par_vram_machine, restated). par_objects_pack and par_objects_unpack handle the two four-byte OAM layouts,
 * n (1 to PAR_OBJECTS_MAX) objects to and from 4 n bytes:
 *     format               byte 0   byte 1   byte 2                                      byte 3
 *     PAR_OBJECTS_OAM_NES  y - 1    tile     (p & 3) | behind << 5 | fx << 6 | fy << 7   x
 *     PAR_OBJECTS_OAM_GB   y + 16   x + 8    tile                                        (p & 7) | fx << 5 | fy << 6 | behind << 7
 * An object FITS the NES when 1 <= y <= 256, 0 <= x <= 255, 0 <= tile <= 255 and p <= 3; the Game Boy when -16 <= y <= 239,
 * -8 <= x <= 247, 0 <= tile <= 255 and p <= 7. A hidden object packs byte 0 as 0xFF on the NES and 0 on the Game Boy; its
 * other bytes are packed as they are. `bad` (not null) gets the objects that are not hidden and do not fit; their fields
 * are cut to the field widths. Unpack is the inverse on the fitting ones and never sets `hidden`.
 * Anchors: x 100, y 50, tile 7, p 2, fx and behind is 31 07 62 64 on the NES; x 20, y 30, tile 9, p 5, fy and behind is
 * 2E 1C 09 C5 on the Game Boy.
 *
 * Consequences, each held by a test:
 *   1. The closing identity. Two maps over one tile set, with their cell bytes; the screen of the first
 *      (par_screen_draw_device, RGBA8 entries, backdrop 0, scroll 0) in both planes; from_maps with capacity >= D; a draw
 *      with opaque 1, pal_base 0, the same K, table and chr, line_limit at least the largest line count and no `behind`:
 *      both planes are the screen of the second map, byte for byte, with over_out 0 and bad_out 0.
 *   2. With opaque 0 the result differs from (1) exactly at the pixels of differing cells whose new value is 0; those keep
 *      the first screen's bytes.
 *   3. n = 0 through a device count of 0, or every object hidden or bad, leaves both planes untouched.
 *   4. Raising line_limit beyond the largest line count changes nothing; with line_limit L the planes equal a draw of the
 *      table with every dropped (object, line) pair removed.
 *   5. Setting fx on a tile stored mirrored left to right changes nothing; the same for fy.
 *   6. A draw through pal_format f equals a draw through PAR_OBJECTS_RGBA8 over the widened table.
 *   7. Under a sufficient limit, objects that share no pixel may be permuted freely.
 *   8. unpack(pack(o)) == o for every fitting, visible object.
 *
 * PAR_ERR_INVALID_ARG for: a null desc, chr, objects, work, map_bg, map, objects_out, count_out, out, data, line_limit,
 * max_objects or (pack, host forms) a null count pointer; fb_io and index_io both null; a null pal_words with an fb_io; one
 * of cells_bg and cells without the other; an objects, count, work, fb_io, bad_out, over_out, map_bg, map, objects_out or
 * count_out that is not aligned to 4 bytes; any value outside the limits above; a negative count of a host form.
 * Left out on purpose: the SNES's high table, the Mega Drive's link list, the GBA's shape and size bits and the
 * tile-numbering quirks of the 8 x 16 modes; several background layers and their priority; windows, mosaic and affine
 * objects; per-object sizes; sprite-zero hit; and choosing WHICH objects to drop, or merging neighbouring differing cells
 * into 16 x 16 objects to get under a line limit: that is the next add-on, and this call is what will measure it.
 */
#ifndef PAR_OBJECTS_H
#define PAR_OBJECTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAR_OBJECTS_MAX 65536
#define PAR_OBJECTS_MAX_LINE 128
#define PAR_OBJECTS_MAX_TILES (1 << 20)
#define PAR_OBJECTS_MAX_CELLS (1 << 20)
#define PAR_OBJECTS_MAX_SIDE 4096

/* the bits of par_object.attr above the sub-palette */
#define PAR_OBJECTS_FLIP_X (1 << 8)
#define PAR_OBJECTS_FLIP_Y (1 << 9)
#define PAR_OBJECTS_BEHIND (1 << 10)
#define PAR_OBJECTS_HIDDEN (1 << 11)

enum par_objects_tile_format {
    PAR_OBJECTS_1BPP = 0,
    PAR_OBJECTS_2BPP_PLANAR = 1,
    PAR_OBJECTS_2BPP_ROWS = 2,
    PAR_OBJECTS_4BPP_ROWS = 3,
    PAR_OBJECTS_4BPP_PACKED_HI = 4,
    PAR_OBJECTS_4BPP_PACKED_LO = 5,
    PAR_OBJECTS_4BPP_ROW_PLANES = 6
};

enum par_objects_palette_format { PAR_OBJECTS_BGR555 = 0, PAR_OBJECTS_BGR333_MD = 1, PAR_OBJECTS_BGR222 = 2, PAR_OBJECTS_RGBA8 = 3 };

enum par_objects_machine {
    PAR_OBJECTS_NES = 0,
    PAR_OBJECTS_GBC = 1,
    PAR_OBJECTS_SMS = 2,
    PAR_OBJECTS_MEGADRIVE = 3,
    PAR_OBJECTS_SNES = 4,
    PAR_OBJECTS_GBA = 5
};

enum par_objects_oam_format { PAR_OBJECTS_OAM_NES = 0, PAR_OBJECTS_OAM_GB = 1 };

/* four int32_t: 16 bytes, no padding */
typedef struct par_object {
    int32_t x, y;
    int32_t tile;
    int32_t attr;
} par_object;

/* int32_t fields alone: 56 bytes, no padding */
typedef struct par_objects_desc {
    int32_t tile_w, tile_h;
    int32_t tile_format;
    int32_t n_tiles;
    int32_t n_objects;
    int32_t line_limit;
    int32_t pal_format;
    int32_t n_colors;
    int32_t sub_size;
    int32_t pal_base;
    int32_t bg_sub_size;
    int32_t opaque;
    int32_t width, height;
} par_objects_desc;

/* Host arithmetic: the bytes of the work block of a draw, 4 * height * (1 + line_limit); 0 outside the limits. */
size_t par_objects_work_bytes(int height, int line_limit);
/* Host arithmetic: the bytes of the work block of a from_maps, 4 * ceil(n_cells / 1024); 0 outside the limits. */
size_t par_objects_from_maps_work_bytes(int n_cells);
/* Host arithmetic: the nominal objects a scanline and objects in all of a par_objects_machine. */
int par_objects_machine_limits(int machine, int* line_limit, int* max_objects);
/* Host arithmetic: n objects to 4 n bytes of OAM in `format` at `out`; `bad` gets those that are shown and do not fit. */
int par_objects_pack(int format, const par_object* objects, int n, uint8_t* out, int* bad);
/* Host arithmetic: 4 n bytes of OAM in `format` to n objects. */
int par_objects_unpack(int format, const uint8_t* data, int n, par_object* objects_out);
/* device pointers (`desc` is read on the host, at the call), asynchronous on `stream`: the fills of bad_out and over_out
 * when given, and two launches */
int par_objects_draw_device(void* stream, const par_objects_desc* desc, const uint8_t* chr, const par_object* objects,
                            const uint32_t* count, const uint8_t* pal_words, const uint8_t* bg_index, void* work,
                            uint8_t* fb_io, uint8_t* index_io, uint32_t* bad_out, uint32_t* over_out);
/* device pointers, asynchronous on `stream`: three launches */
int par_objects_from_maps_device(void* stream, const uint32_t* map_bg, const uint8_t* cells_bg, const uint32_t* map,
                                 const uint8_t* cells, int gcx, int gcy, int tile_w, int tile_h, int x0, int y0, int capacity,
                                 void* work, par_object* objects_out, uint32_t* count_out);
/* host pointers, synchronous, everything on HIP device `device` (-1: the current device): allocate, copy, launch,
 * synchronise, copy back and free. `count` is the n of the device form as a plain int, at least 0; the planes are read and
 * written; a bg_index that is index_io itself stays so on the device. The counts come back through `bad` and `over`, which
 * are not nullable. PAR_ERR_NO_DEVICE / PAR_ERR_OOM / PAR_ERR_HIP as par_quantize_cells_host */
int par_objects_draw_host(int device, const par_objects_desc* desc, const uint8_t* chr, const par_object* objects, int count,
                          const uint8_t* pal_words, const uint8_t* bg_index, uint8_t* fb_io, uint8_t* index_io, int* bad,
                          int* over);
/* the same for from_maps: objects_out holds `capacity` records, of which the first min(D, capacity) are written; D comes
 * back through `count`, which is not nullable */
int par_objects_from_maps_host(int device, const uint32_t* map_bg, const uint8_t* cells_bg, const uint32_t* map,
                               const uint8_t* cells, int gcx, int gcy, int tile_w, int tile_h, int x0, int y0, int capacity,
                               par_object* objects_out, int* count);

#ifdef __cplusplus
}
#endif

#endif
