"""The screen contract of addons/include/par_screen.h restated in numpy, twice: vectorised (draw, decode_map,
palette_rgba: what the GPU tests compare with byte for byte) and as loops over pixels and bits in Python integers (the
*_loop forms, which test_screen_cpu.py holds the vectorised forms to). Inputs come from tests/vram.py's encoders. A
descriptor is a dict of the header's field names with the layout (a dict, as in tests/vram.py) under "layout"."""
import numpy as np

import vram as V

BGR555, BGR333_MD, BGR222, RGBA8 = range(4)
PAL_FORMATS = (BGR555, BGR333_MD, BGR222, RGBA8)
PAL_NAMES = ("bgr555", "bgr333 md", "bgr222", "rgba8")
ENTRY_BYTES = (2, 2, 1, 4)
MAX_TILES = MAX_CELLS = 1 << 20
MAX_SIDE = 4096
DESC_FIELDS = ("tile_w", "tile_h", "tile_format", "n_tiles", "map_w", "map_h", "ratio_x", "ratio_y", "pal_format", "n_colors", "sub_size",
               "backdrop", "width", "height", "scroll_x", "scroll_y")


def desc_of(L, **over):
    """A descriptor over layout L: 8 x 8 tiles of 4bpp rows, a 4 x 3 map of 12 tiles under a 32 x 24 screen, 16 RGBA8
    colours in sub-palettes of 4, and `over` on top."""
    d = dict(layout=dict(L), tile_w=8, tile_h=8, tile_format=V.F_4BPP_ROWS, n_tiles=12, map_w=4, map_h=3, ratio_x=1, ratio_y=1,
             pal_format=RGBA8, n_colors=16, sub_size=4, backdrop=0, width=32, height=24, scroll_x=0, scroll_y=0)
    d.update(over)
    assert set(d) == set(DESC_FIELDS) | {"layout"}
    return d


def attr_cells(d):
    return -(-d["map_w"] // d["ratio_x"]) * -(-d["map_h"] // d["ratio_y"])


# ---- colour words ----------------------------------------------------------------------------------------------------------

def widen(q, bits):
    """The header's table: a field of `bits` bits to eight by bit replication."""
    return {5: q << 3 | q >> 2, 3: q << 5 | q << 2 | q >> 1, 2: q * 0x55}[bits]


def palette_rgba(words, fmt, n=None):
    """(n, 4) uint8: red, green, blue, 255."""
    b = np.asarray(words, dtype=np.uint8).reshape(-1).astype(np.uint32)
    n = len(b) // ENTRY_BYTES[fmt] if n is None else n
    b = b[:n * ENTRY_BYTES[fmt]]
    if fmt == RGBA8:
        e = b.reshape(n, 4)
        r, g, bl = e[:, 0], e[:, 1], e[:, 2]
    elif fmt == BGR555:
        w = b[0::2] | b[1::2] << 8
        r, g, bl = (widen(q & 31, 5) for q in (w, w >> 5, w >> 10))
    elif fmt == BGR333_MD:
        w = b[0::2] << 8 | b[1::2]
        r, g, bl = (widen(q & 7, 3) for q in (w >> 1, w >> 5, w >> 9))
    else:
        r, g, bl = (widen(q & 3, 2) for q in (b, b >> 2, b >> 4))
    return np.stack([r, g, bl, np.full(n, 255, np.uint32)], axis=1).astype(np.uint8)


def palette_rgba_loop(words, fmt, n=None):
    data = bytes(np.asarray(words, dtype=np.uint8).reshape(-1))
    n = len(data) // ENTRY_BYTES[fmt] if n is None else n
    out = []
    for i in range(n):
        if fmt == RGBA8:
            r, g, b = data[4 * i], data[4 * i + 1], data[4 * i + 2]
        elif fmt == BGR555:
            w = int.from_bytes(data[2 * i:2 * i + 2], "little")
            r, g, b = ((q % 32) * 8 + (q % 32) // 4 for q in (w, w // 32, w // 1024))
        elif fmt == BGR333_MD:
            w = int.from_bytes(data[2 * i:2 * i + 2], "big")
            r, g, b = ((q % 8) * 32 + (q % 8) * 4 + (q % 8) // 2 for q in (w // 2, w // 32, w // 512))
        else:
            w = data[i]
            r, g, b = ((q % 4) * 85 for q in (w, w // 4, w // 16))
        out.append((r, g, b, 255))
    return np.array(out, dtype=np.uint8).reshape(n, 4)


# ---- map words -------------------------------------------------------------------------------------------------------------

def read_cells(L, data, limit):
    """(id, p, fx, fy, bad) of the words' bytes, as uint64 arrays and a bool array; `limit` is the first id that is bad."""
    assert V.layout_ok(L)
    wb = L["word_bytes"]
    d = np.asarray(data, dtype=np.uint8).reshape(-1, wb).astype(np.uint64)
    order = range(wb - 1, -1, -1) if L["big_endian"] else range(wb)
    w = np.zeros(len(d), dtype=np.uint64)
    for at, k in enumerate(order):
        w |= d[:, at] << np.uint64(8 * k)
    t = ((w >> np.uint64(L["tile_shift"])) & np.uint64((1 << L["tile_bits"]) - 1)).astype(np.int64)
    p = (w >> np.uint64(L["pal_shift"])) & np.uint64((1 << L["pal_bits"]) - 1)
    zero = np.zeros(len(d), dtype=np.uint64)
    fx = (w >> np.uint64(L["flip_x_bit"])) & np.uint64(1) if L["flip_x_bit"] >= 0 else zero
    fy = (w >> np.uint64(L["flip_y_bit"])) & np.uint64(1) if L["flip_y_bit"] >= 0 else zero
    above = t - L["tile_base"]
    ident = above // L["tile_step"]
    bad = (above < 0) | (above % L["tile_step"] != 0) | (ident >= limit)
    return np.where(bad, 0, ident).astype(np.uint64), p, fx, fy, bad


def decode_map(L, data):
    """(map_out uint32, pal_out uint8, the bad cells)."""
    ident, p, fx, fy, bad = read_cells(L, data, 1 << 30)
    return (ident | fx << np.uint64(30) | fy << np.uint64(31)).astype(np.uint32), (p & np.uint64(255)).astype(np.uint8), int(bad.sum())


def decode_map_loop(L, data):
    data, wb = bytes(np.asarray(data, dtype=np.uint8).reshape(-1)), L["word_bytes"]
    words, pals, n_bad = [], [], 0
    for c in range(len(data) // wb):
        ident, p, fx, fy, bad = cell_loop(L, data, c, 1 << 30)
        n_bad += int(bad)
        words.append(ident | fx << 30 | fy << 31)
        pals.append(p % 256)
    return np.array(words, dtype=np.uint32), np.array(pals, dtype=np.uint8), n_bad


def cell_loop(L, data, c, limit):
    wb = L["word_bytes"]
    w = int.from_bytes(data[c * wb:(c + 1) * wb], "big" if L["big_endian"] else "little")
    t = (w >> L["tile_shift"]) % (1 << L["tile_bits"])
    p = (w >> L["pal_shift"]) % (1 << L["pal_bits"])
    fx = (w >> L["flip_x_bit"]) & 1 if L["flip_x_bit"] >= 0 else 0
    fy = (w >> L["flip_y_bit"]) & 1 if L["flip_y_bit"] >= 0 else 0
    ident, rest = divmod(t - L["tile_base"], L["tile_step"])
    bad = t < L["tile_base"] or rest != 0 or ident >= limit
    return (0 if bad else ident), p, fx, fy, bad


# ---- the screen ------------------------------------------------------------------------------------------------------------

def pixels(d, chr_bytes, map_words, attr=None, line_scroll=None):
    """(v, p, whether the cell is bad) of every screen pixel as (height, width) arrays, and the bad cells of the map."""
    L, tw, th, fmt = d["layout"], d["tile_w"], d["tile_h"], d["tile_format"]
    w, h, mw, mh = d["width"], d["height"], d["map_w"], d["map_h"]
    tiles = V.decode_tiles(np.asarray(chr_bytes, dtype=np.uint8)[:d["n_tiles"] * V.tile_bytes(fmt, (tw, th))], (tw, th), fmt)
    ident, p, fx, fy, bad = read_cells(L, np.asarray(map_words, dtype=np.uint8)[:mw * mh * L["word_bytes"]], d["n_tiles"])
    lines = np.zeros((h, 2), dtype=np.int64) if line_scroll is None else np.asarray(line_scroll, dtype=np.int32).reshape(h, 2).astype(np.int64)
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    mx = (x + d["scroll_x"] + lines[:, 0:1]) % (mw * tw) + 0 * y  # (numpy's % is the floor modulo)
    my = (y + d["scroll_y"] + lines[:, 1:2]) % (mh * th) + 0 * x
    cx, cy = mx // tw, my // th
    c = cx + cy * mw
    pal = p[c].astype(np.int64)
    if attr is not None:
        pal = np.asarray(attr, dtype=np.uint8)[cx // d["ratio_x"] + (cy // d["ratio_y"]) * -(-mw // d["ratio_x"])].astype(np.int64)
    px, py = mx % tw, my % th
    px = np.where(fx[c] != 0, tw - 1 - px, px)
    py = np.where(fy[c] != 0, th - 1 - py, py)
    v = tiles[ident[c].astype(np.int64), py, px].astype(np.int64)
    return v, pal, bad[c], int(bad.sum())


def draw(d, chr_bytes, map_words, pal_words=None, attr=None, line_scroll=None):
    """(fb (height, width, 4) uint8 or None without pal_words, index (height, width) uint8, the bad cells of the map)."""
    v, pal, bad, n_bad = pixels(d, chr_bytes, map_words, attr, line_scroll)
    i = np.minimum(pal * d["sub_size"] + v, d["n_colors"] - 1)
    if d["backdrop"]:
        i = np.where(v == 0, 0, i)
    i = np.where(bad, 0, i).astype(np.uint8)
    fb = None if pal_words is None else palette_rgba(pal_words, d["pal_format"], d["n_colors"])[i]
    return fb, i, n_bad


def pixel_value_loop(data, fmt, tile, ident, px, py):
    """Tile ident's pixel (px, py) read from the bytes bit by bit."""
    tw, _ = tile
    each, bpp = V.tile_bytes(fmt, tile), V.BPP[fmt]
    base = ident * each + ((py // 8) * (tw // 8) + px // 8) * 8 * bpp
    x, y = px % 8, py % 8
    if fmt in V.PACKED:
        byte = data[base + 4 * y + x // 2]
        high = (x % 2 == 0) == (fmt == V.F_4BPP_PACKED_HI)
        return byte >> 4 if high else byte & 15
    v = 0
    for b in range(bpp):
        v |= ((data[base + V.plane_byte(fmt, b, y)] >> (7 - x)) & 1) << b
    return v


def draw_loop(d, chr_bytes, map_words, pal_words=None, attr=None, line_scroll=None):
    L, tw, th, fmt = d["layout"], d["tile_w"], d["tile_h"], d["tile_format"]
    w, h, mw, mh = d["width"], d["height"], d["map_w"], d["map_h"]
    data, words = bytes(np.asarray(chr_bytes, dtype=np.uint8).reshape(-1)), bytes(np.asarray(map_words, dtype=np.uint8).reshape(-1))
    colours = None if pal_words is None else palette_rgba_loop(pal_words, d["pal_format"], d["n_colors"])
    index = np.zeros((h, w), dtype=np.uint8)
    for y in range(h):
        lx, ly = (0, 0) if line_scroll is None else (int(line_scroll[2 * y]), int(line_scroll[2 * y + 1]))
        for x in range(w):
            mx, my = (x + d["scroll_x"] + lx) % (mw * tw), (y + d["scroll_y"] + ly) % (mh * th)  # (Python's % is the floor modulo)
            cx, cy = mx // tw, my // th
            ident, p, fx, fy, bad = cell_loop(L, words, cx + cy * mw, d["n_tiles"])
            if attr is not None:
                p = int(attr[cx // d["ratio_x"] + (cy // d["ratio_y"]) * -(-mw // d["ratio_x"])])
            if bad:
                continue
            px, py = mx % tw, my % th
            v = pixel_value_loop(data, fmt, (tw, th), ident, tw - 1 - px if fx else px, th - 1 - py if fy else py)
            index[y, x] = 0 if d["backdrop"] and v == 0 else min(p * d["sub_size"] + v, d["n_colors"] - 1)
    n_bad = sum(int(cell_loop(L, words, c, d["n_tiles"])[4]) for c in range(mw * mh))
    return (None if colours is None else colours[index]), index, n_bad


# ---- the chain -------------------------------------------------------------------------------------------------------------

def desc_of_export(exp, w, h, n_colors, sub_size, **over):
    """The descriptor that shows an export of tests/vram.py's export() (8 x 8 tiles, the palette in the words) on a screen
    the size of the frame's tile grid."""
    gcx, gcy = -(-w // 8), -(-h // 8)
    d = desc_of(exp["layout"], tile_format=exp["format"], n_tiles=max(1, min(exp["count"], len(exp["chr"]) // V.tile_bytes(exp["format"], (8, 8)))),
                map_w=gcx, map_h=gcy, n_colors=n_colors, sub_size=sub_size, width=w, height=h)
    d.update(over)
    return d


def export(TS, index, chosen, sub_size, w, h, cell, tile, L, fmt, flips):
    """The chain over a cells index plane under tiles of any size: the local plane, its tile set under `flips`, the tiles
    in `fmt`, the map words of layout L with the cells' sub-palettes in them. A dict as tests/vram.py's export()."""
    local = np.asarray(index, dtype=np.uint8) % sub_size
    tiles, tile_map, count = TS.model(local, w, h, tile, 0, flips)
    chr_bytes, bad_tiles = V.encode_tiles(tiles, tile, fmt)
    gcx, gcy = TS.grid(w, h, tile)
    ratio = (cell[0] // tile[0], cell[1] // tile[1])
    map_bytes, bad_cells = V.encode_map(L, tile_map, gcx, gcy, chosen, ratio)
    d = desc_of(L, tile_w=tile[0], tile_h=tile[1], tile_format=fmt, n_tiles=count, map_w=gcx, map_h=gcy, sub_size=sub_size, width=w, height=h)
    return {"count": count, "tiles": tiles, "map": tile_map, "chr": chr_bytes, "map_bytes": map_bytes, "bad": bad_tiles + bad_cells,
            "ratio": ratio, "desc": d}
