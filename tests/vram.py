"""The VRAM-export contract of addons/include/par_vram.h restated in numpy, twice: vectorised (encode_tiles, decode_tiles,
encode_map, palette_words: what the GPU tests compare with byte for byte) and as loops over pixels and bits in Python
integers (the *_loop forms, which test_vram_cpu.py holds the vectorised forms to). Tiles are (n, th, tw) uint8 arrays, a
tile map is a uint32 array of id | fx << 30 | fy << 31, a layout is a dict of the header's field names."""
import numpy as np

TILES = ((8, 8), (8, 16), (16, 8), (16, 16))
F_1BPP, F_2BPP_PLANAR, F_2BPP_ROWS, F_4BPP_ROWS, F_4BPP_PACKED_HI, F_4BPP_PACKED_LO, F_4BPP_ROW_PLANES = range(7)
FORMATS = tuple(range(7))
FORMAT_NAMES = ("1bpp", "2bpp planar", "2bpp rows", "4bpp rows", "4bpp packed hi", "4bpp packed lo", "4bpp row planes")
BPP = (1, 2, 2, 4, 4, 4, 4)
PACKED = (F_4BPP_PACKED_HI, F_4BPP_PACKED_LO)
NES, GBC, SMS, MEGADRIVE, SNES, GBA = range(6)
MACHINES = ("nes", "gbc", "sms", "megadrive", "snes", "gba")
BGR555, BGR333_MD, BGR222 = range(3)
MAX_TILES = MAX_CELLS = 1 << 20
ID_MASK = 0x3FFFFFFF
FIELDS = ("word_bytes", "big_endian", "tile_shift", "tile_bits", "pal_shift", "pal_bits", "flip_x_bit", "flip_y_bit", "tile_step",
          "tile_base", "set_bits")
# the header's table: bytes, big-endian, tile shift / bits, palette shift / bits, x flip, y flip; step 1, base 0, no set bits
PRESETS = {
    NES: (1, 0, 0, 8, 0, 0, -1, -1, 1, 0, 0),
    GBC: (2, 0, 0, 8, 8, 3, 13, 14, 1, 0, 0),
    SMS: (2, 0, 0, 9, 11, 1, 9, 10, 1, 0, 0),
    MEGADRIVE: (2, 1, 0, 11, 13, 2, 11, 12, 1, 0, 0),
    SNES: (2, 0, 0, 10, 10, 3, 14, 15, 1, 0, 0),
    GBA: (2, 0, 0, 10, 12, 4, 10, 11, 1, 0, 0),
}
# what par_demo --vram takes a machine for: (tile format, palette format or None, the most sub-palettes its word names)
MACHINE_FORMATS = {NES: (F_2BPP_PLANAR, None), GBC: (F_2BPP_ROWS, BGR555), SMS: (F_4BPP_ROW_PLANES, BGR222),
                   MEGADRIVE: (F_4BPP_PACKED_HI, BGR333_MD), SNES: (F_4BPP_ROWS, BGR555), GBA: (F_4BPP_PACKED_LO, BGR555)}


def preset(machine):
    return dict(zip(FIELDS, PRESETS[machine]))


def layout_of(**over):
    """A two-byte little-endian layout with every field spelled out, and `over` on top."""
    base = dict(word_bytes=2, big_endian=0, tile_shift=0, tile_bits=10, pal_shift=10, pal_bits=3, flip_x_bit=14, flip_y_bit=15,
                tile_step=1, tile_base=0, set_bits=0)
    base.update(over)
    return base


def tile_bytes(fmt, tile):
    if fmt not in FORMATS or tile[0] not in (8, 16) or tile[1] not in (8, 16):
        return 0
    return 8 * BPP[fmt] * (tile[0] // 8) * (tile[1] // 8)


def plane_byte(fmt, b, y):
    """The byte of a sub-tile that holds bit plane b of row y (the planar formats)."""
    return {F_1BPP: y, F_2BPP_PLANAR: 8 * b + y, F_2BPP_ROWS: 2 * y + b, F_4BPP_ROWS: 16 * (b >> 1) + 2 * y + (b & 1),
            F_4BPP_ROW_PLANES: 4 * y + b}[fmt]


def sub_tiles(tiles, tile):
    """(n * subs, 8, 8): the 8 x 8 sub-tiles of (n, th, tw) tiles, row-major over sub-tiles."""
    tw, th = tile
    t = np.asarray(tiles, dtype=np.uint8).reshape(-1, th // 8, 8, tw // 8, 8)
    return np.ascontiguousarray(t.transpose(0, 1, 3, 2, 4)).reshape(-1, 8, 8)


def from_sub_tiles(subs, tile):
    tw, th = tile
    s = np.asarray(subs, dtype=np.uint8).reshape(-1, th // 8, tw // 8, 8, 8)
    return np.ascontiguousarray(s.transpose(0, 1, 3, 2, 4)).reshape(-1, th, tw)


# ---- tiles, vectorised ---------------------------------------------------------------------------------------------------

def encode_tiles(tiles, tile, fmt):
    """(the bytes of the tiles in `fmt`, a flat uint8 array; the number of tiles with a byte >= 2^bpp)."""
    tiles = np.asarray(tiles, dtype=np.uint8).reshape(-1, tile[1], tile[0])
    bpp = BPP[fmt]
    bad = int((tiles.reshape(len(tiles), -1) >> bpp).any(axis=1).sum()) if len(tiles) else 0
    s = sub_tiles(tiles, tile)  # (m, y, x)
    out = np.zeros((len(s), 8 * bpp), dtype=np.uint8)
    if fmt in PACKED:
        even, odd = s[:, :, 0::2] & 15, s[:, :, 1::2] & 15
        pair = (even << 4 | odd) if fmt == F_4BPP_PACKED_HI else (odd << 4 | even)
        out[:] = pair.reshape(len(s), 32)
    else:
        for b in range(bpp):
            rows = np.packbits((s >> b) & 1, axis=2, bitorder="big").reshape(len(s), 8)  # bit 7 - x
            out[:, [plane_byte(fmt, b, y) for y in range(8)]] = rows
    return out.reshape(-1), bad


def decode_tiles(data, tile, fmt):
    """(n, th, tw): a byte a pixel, every byte < 2^bpp."""
    bpp = BPP[fmt]
    d = np.asarray(data, dtype=np.uint8).reshape(-1, 8 * bpp)
    s = np.zeros((len(d), 8, 8), dtype=np.uint8)
    if fmt in PACKED:
        pair = d.reshape(len(d), 8, 4)
        high, low = pair >> 4, pair & 15
        s[:, :, 0::2], s[:, :, 1::2] = (high, low) if fmt == F_4BPP_PACKED_HI else (low, high)
    else:
        for b in range(bpp):
            rows = d[:, [plane_byte(fmt, b, y) for y in range(8)]]
            s |= np.unpackbits(rows.reshape(len(d), 8, 1), axis=2, bitorder="big") << b
    return from_sub_tiles(s, tile)


# ---- tiles, per pixel and per bit ----------------------------------------------------------------------------------------

def encode_tiles_loop(tiles, tile, fmt):
    tw, th = tile
    tiles = np.asarray(tiles, dtype=np.uint8).reshape(-1, th, tw)
    bpp, each = BPP[fmt], tile_bytes(fmt, tile)
    out, bad = bytearray(len(tiles) * each), 0
    for i in range(len(tiles)):
        over = False
        for py in range(th):
            for px in range(tw):
                v = int(tiles[i, py, px])
                over = over or v >= 1 << bpp
                sub = (py // 8) * (tw // 8) + px // 8
                x, y = px % 8, py % 8
                base = i * each + sub * 8 * bpp
                if fmt in PACKED:
                    high = (x % 2 == 0) == (fmt == F_4BPP_PACKED_HI)
                    out[base + 4 * y + x // 2] |= (v & 15) << (4 if high else 0)
                else:
                    for b in range(bpp):
                        out[base + plane_byte(fmt, b, y)] |= ((v >> b) & 1) << (7 - x)
        bad += int(over)
    return np.frombuffer(bytes(out), dtype=np.uint8), bad


def decode_tiles_loop(data, tile, fmt):
    tw, th = tile
    data = bytes(np.asarray(data, dtype=np.uint8).reshape(-1))
    bpp, each = BPP[fmt], tile_bytes(fmt, tile)
    n = len(data) // each
    out = np.zeros((n, th, tw), dtype=np.uint8)
    for i in range(n):
        for py in range(th):
            for px in range(tw):
                sub = (py // 8) * (tw // 8) + px // 8
                x, y = px % 8, py % 8
                base = i * each + sub * 8 * bpp
                if fmt in PACKED:
                    byte = data[base + 4 * y + x // 2]
                    high = (x % 2 == 0) == (fmt == F_4BPP_PACKED_HI)
                    v = byte >> 4 if high else byte & 15
                else:
                    v = 0
                    for b in range(bpp):
                        v |= ((data[base + plane_byte(fmt, b, y)] >> (7 - x)) & 1) << b
                out[i, py, px] = v
    return out


# ---- map words -------------------------------------------------------------------------------------------------------------

def layout_ok(L):
    if L["word_bytes"] not in (1, 2, 4) or L["big_endian"] not in (0, 1):
        return False
    bits = 8 * L["word_bytes"]
    if L["tile_bits"] < 1 or L["tile_shift"] < 0 or L["tile_shift"] + L["tile_bits"] > bits:
        return False
    if L["pal_bits"] < 0 or L["pal_shift"] < 0 or L["pal_shift"] + L["pal_bits"] > bits:
        return False
    if not (-1 <= L["flip_x_bit"] < bits and -1 <= L["flip_y_bit"] < bits):
        return False
    if not (1 <= L["tile_step"] <= 16 and 0 <= L["tile_base"] <= 65535):
        return False
    return (L["set_bits"] & 0xFFFFFFFF) >> bits == 0


def colour_cells(gcx, gcy, ratio):
    return -(-gcx // ratio[0]) * -(-gcy // ratio[1])


def encode_map(L, tile_map, gcx, gcy, cells=None, ratio=(1, 1)):
    """(the words' bytes, a flat uint8 array of word_bytes a cell; the number of bad cells)."""
    assert layout_ok(L)
    m = np.asarray(tile_map, dtype=np.uint32).reshape(-1).astype(np.uint64)
    assert len(m) == gcx * gcy
    c = np.arange(gcx * gcy)
    tx, ty = c % gcx, c // gcx
    ccx = -(-gcx // ratio[0])
    p = np.zeros(len(m), dtype=np.uint64)
    if cells is not None:
        cells = np.asarray(cells, dtype=np.uint8).reshape(-1)
        assert len(cells) == colour_cells(gcx, gcy, ratio)
        p = cells[tx // ratio[0] + (ty // ratio[1]) * ccx].astype(np.uint64)
    fx, fy = (m >> np.uint64(30)) & np.uint64(1), m >> np.uint64(31)
    t = (m & np.uint64(ID_MASK)) * np.uint64(L["tile_step"]) + np.uint64(L["tile_base"])
    tile_mask, pal_mask = np.uint64((1 << L["tile_bits"]) - 1), np.uint64((1 << L["pal_bits"]) - 1)
    w = ((t & tile_mask) << np.uint64(L["tile_shift"])) | ((p & pal_mask) << np.uint64(L["pal_shift"]))
    w |= np.uint64(L["set_bits"] & 0xFFFFFFFF)
    bad = (t > tile_mask) | (p > pal_mask)
    for f, bit in ((fx, L["flip_x_bit"]), (fy, L["flip_y_bit"])):
        if bit >= 0:
            w |= f << np.uint64(bit)
        else:
            bad |= f != 0
    wb = L["word_bytes"]
    order = range(wb - 1, -1, -1) if L["big_endian"] else range(wb)
    out = np.stack([((w >> np.uint64(8 * k)) & np.uint64(0xFF)).astype(np.uint8) for k in order], axis=1)
    return np.ascontiguousarray(out).reshape(-1), int(bad.sum())


def encode_map_loop(L, tile_map, gcx, gcy, cells=None, ratio=(1, 1)):
    assert layout_ok(L)
    out, bad = bytearray(), 0
    ccx = -(-gcx // ratio[0])
    for c in range(gcx * gcy):
        entry = int(tile_map[c])
        ident, fx, fy = entry & ID_MASK, (entry >> 30) & 1, (entry >> 31) & 1
        tx, ty = c % gcx, c // gcx
        p = 0 if cells is None else int(cells[tx // ratio[0] + (ty // ratio[1]) * ccx])
        t = ident * L["tile_step"] + L["tile_base"]
        w = (t % (1 << L["tile_bits"])) << L["tile_shift"] | (p % (1 << L["pal_bits"])) << L["pal_shift"] | (L["set_bits"] & 0xFFFFFFFF)
        wrong = t >= 1 << L["tile_bits"] or p >= 1 << L["pal_bits"]
        if L["flip_x_bit"] >= 0:
            w |= fx << L["flip_x_bit"]
        elif fx:
            wrong = True
        if L["flip_y_bit"] >= 0:
            w |= fy << L["flip_y_bit"]
        elif fy:
            wrong = True
        bad += int(wrong)
        out += w.to_bytes(L["word_bytes"], "big" if L["big_endian"] else "little")
    return np.frombuffer(bytes(out), dtype=np.uint8), bad


def unpack_map(L, data):
    """(tile map words id | fx << 30 | fy << 31, the palette field) of the words' bytes, for a layout of step 1 and base 0
    without set bits: what a machine reads back."""
    wb = L["word_bytes"]
    d = np.asarray(data, dtype=np.uint8).reshape(-1, wb).astype(np.uint64)
    order = range(wb - 1, -1, -1) if L["big_endian"] else range(wb)
    w = np.zeros(len(d), dtype=np.uint64)
    for at, k in enumerate(order):
        w |= d[:, at] << np.uint64(8 * k)
    ident = (w >> np.uint64(L["tile_shift"])) & np.uint64((1 << L["tile_bits"]) - 1)
    pal = (w >> np.uint64(L["pal_shift"])) & np.uint64((1 << L["pal_bits"]) - 1)
    fx = (w >> np.uint64(L["flip_x_bit"])) & np.uint64(1) if L["flip_x_bit"] >= 0 else np.zeros(len(d), dtype=np.uint64)
    fy = (w >> np.uint64(L["flip_y_bit"])) & np.uint64(1) if L["flip_y_bit"] >= 0 else np.zeros(len(d), dtype=np.uint64)
    return (ident | fx << np.uint64(30) | fy << np.uint64(31)).astype(np.uint32), pal.astype(np.uint8)


# ---- palette words ---------------------------------------------------------------------------------------------------------

def palette_words(palette, fmt):
    """The words' bytes of (n, 4) uint8 entries red, green, blue, alpha."""
    p = np.asarray(palette, dtype=np.uint8).reshape(-1, 4).astype(np.uint32)
    r, g, b = p[:, 0], p[:, 1], p[:, 2]
    if fmt == BGR555:
        w = r >> 3 | (g >> 3) << 5 | (b >> 3) << 10
        return np.stack([w & 0xFF, w >> 8], axis=1).astype(np.uint8).reshape(-1)
    if fmt == BGR333_MD:
        w = (r >> 5) << 1 | (g >> 5) << 5 | (b >> 5) << 9
        return np.stack([w >> 8, w & 0xFF], axis=1).astype(np.uint8).reshape(-1)
    return (r >> 6 | (g >> 6) << 2 | (b >> 6) << 4).astype(np.uint8)


def palette_words_loop(palette, fmt):
    out = bytearray()
    for entry in np.asarray(palette, dtype=np.uint8).reshape(-1, 4).tolist():
        r, g, b = entry[:3]
        if fmt == BGR555:
            out += (r // 8 + (g // 8) * 32 + (b // 8) * 1024).to_bytes(2, "little")
        elif fmt == BGR333_MD:
            out += ((r // 32) * 2 + (g // 32) * 32 + (b // 32) * 512).to_bytes(2, "big")
        else:
            out += (r // 64 + (g // 64) * 4 + (b // 64) * 16).to_bytes(1, "little")
    return np.frombuffer(bytes(out), dtype=np.uint8)


# ---- the chain -------------------------------------------------------------------------------------------------------------

def export(TS, index, cell_out, sub_size, w, h, cell, machine, flips):
    """What the chain gives for a cells index plane under 8 x 8 tiles: a dict of the local and the flat tile counts, the
    local tile set and map, the encoded tiles, the map words and the two bad counts."""
    tile = (8, 8)
    fmt = MACHINE_FORMATS[machine][0]
    L = preset(machine)
    local = np.asarray(index, dtype=np.uint8) % sub_size
    tiles, tile_map, count = TS.model(local, w, h, tile, 0, flips)
    flat = TS.model(index, w, h, tile, 0, flips)[2]
    chr_bytes, bad_tiles = encode_tiles(tiles, tile, fmt)
    gcx, gcy = TS.grid(w, h, tile)
    ratio = (cell[0] // 8, cell[1] // 8)
    map_bytes, bad_cells = encode_map(L, tile_map, gcx, gcy, cell_out, ratio)
    return {"count": count, "flat": flat, "tiles": tiles, "map": tile_map, "chr": chr_bytes, "map_bytes": map_bytes,
            "bad": bad_tiles + bad_cells, "layout": L, "format": fmt, "ratio": ratio}


def closing_identity(TS, exp, cell_out, sub_size, w, h):
    """The cells index plane a machine would show from an export: decode the tiles, unpack the words, expand, and add
    K * the palette field of every pixel's tile cell."""
    tile = (8, 8)
    tiles = decode_tiles(exp["chr"], tile, exp["format"])
    tile_map, pal = unpack_map(exp["layout"], exp["map_bytes"])
    plane = TS.expand_model(tiles, tile, tile_map, w, h).reshape(h, w).astype(np.uint32)
    gcx, gcy = TS.grid(w, h, tile)
    per_pixel = np.repeat(np.repeat(pal.reshape(gcy, gcx), 8, axis=0), 8, axis=1)[:h, :w]
    return (plane + sub_size * per_pixel).astype(np.uint8).reshape(-1)
