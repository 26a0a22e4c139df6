"""The objects contract of addons/include/par_objects.h restated in numpy, twice: vectorised (draw, from_maps, pack, unpack:
what the GPU tests compare with byte for byte) and as loops over objects, pixels and bits in Python integers (the *_loop
forms, which test_objects_cpu.py holds the vectorised forms to). Tile bytes come from tests/vram.py's encoders, colour words
go through tests/screen.py's widening. A descriptor is a dict of the header's field names; objects are an array of OBJECT
records (x, y, tile, attr)."""
import numpy as np

import screen as S
import vram as V

OBJECT = np.dtype([("x", np.int32), ("y", np.int32), ("tile", np.int32), ("attr", np.int32)])
FLIP_X, FLIP_Y, BEHIND, HIDDEN = 1 << 8, 1 << 9, 1 << 10, 1 << 11
MAX_OBJECTS, MAX_LINE, MAX_TILES, MAX_CELLS, MAX_SIDE = 65536, 128, 1 << 20, 1 << 20, 4096
OAM_NES, OAM_GB = range(2)
DESC_FIELDS = ("tile_w", "tile_h", "tile_format", "n_tiles", "n_objects", "line_limit", "pal_format", "n_colors", "sub_size", "pal_base",
               "bg_sub_size", "opaque", "width", "height")
# the header's table: objects a scanline, objects in all, by par_vram_machine
LIMITS = {V.NES: (8, 64), V.GBC: (10, 40), V.SMS: (8, 64), V.MEGADRIVE: (20, 80), V.SNES: (32, 128), V.GBA: (128, 128)}


def desc_of(**over):
    """8 x 8 objects of 4bpp rows over 12 tiles, 16 of them, 8 a line, 16 RGBA8 colours in sub-palettes of 4 from entry 0,
    transparent, on a 32 x 24 screen, and `over` on top."""
    d = dict(tile_w=8, tile_h=8, tile_format=V.F_4BPP_ROWS, n_tiles=12, n_objects=16, line_limit=8, pal_format=S.RGBA8, n_colors=16,
             sub_size=4, pal_base=0, bg_sub_size=4, opaque=0, width=32, height=24)
    d.update(over)
    assert set(d) == set(DESC_FIELDS)
    return d


def objects_of(records):
    """OBJECT records of (x, y, tile, attr) tuples."""
    return np.array([tuple(r) for r in records], dtype=OBJECT).reshape(-1)


def work_bytes(height, line_limit):
    return 4 * height * (1 + line_limit) if 1 <= height <= MAX_SIDE and 1 <= line_limit <= MAX_LINE else 0


def from_maps_work_bytes(n_cells):
    return 4 * -(-n_cells // 1024) if 1 <= n_cells <= MAX_CELLS else 0


# ---- the table -------------------------------------------------------------------------------------------------------------

def judge(d, objects, n):
    """(live, bad) bool arrays over the first n records."""
    o = objects[:n]
    x, y, t = (o[f].astype(np.int64) for f in ("x", "y", "tile"))
    hidden = (o["attr"].astype(np.int64) & HIDDEN) != 0
    bad = ~hidden & ((t < 0) | (t >= d["n_tiles"]) | (x < -32768) | (x > 32767) | (y < -32768) | (y > 32767))
    return ~hidden & ~bad, bad


def lines(d, objects, n):
    """(shown (n, height) bool: object j is shown on line y; the objects dropped over the lines; the largest line count)."""
    live, _ = judge(d, objects, n)
    y = objects["y"][:n].astype(np.int64)[:, None]
    row = np.arange(d["height"], dtype=np.int64)[None, :]
    covers = live[:, None] & (y <= row) & (row < y + d["tile_h"])
    rank = np.cumsum(covers, axis=0) - 1
    shown = covers & (rank < d["line_limit"])
    return shown, int(covers.sum() - shown.sum()), int(covers.sum(axis=0).max()) if n else 0


def draw(d, chr_bytes, objects, pal_words=None, bg_index=None, fb=None, index=None, count=None, shown=None):
    """(fb or None, index or None, the bad objects, the objects dropped): copies of the planes with the objects drawn over
    them. bg_index "index" is the index plane as it comes in. `shown` replaces the line lists (consequence 4)."""
    w, h, tw, th = d["width"], d["height"], d["tile_w"], d["tile_h"]
    n = d["n_objects"] if count is None else min(count, d["n_objects"])
    objects = np.asarray(objects, dtype=OBJECT).reshape(-1)
    fb = None if fb is None else np.array(fb, dtype=np.uint8).reshape(h, w, 4)
    index = None if index is None else np.array(index, dtype=np.uint8).reshape(h, w)
    if isinstance(bg_index, str):
        bg_index = index.copy()
    elif bg_index is not None:
        bg_index = np.asarray(bg_index, dtype=np.uint8).reshape(h, w)
    _, bad = judge(d, objects, n)
    over = 0
    if shown is None:
        shown, over, _ = lines(d, objects, n)
    tiles = V.decode_tiles(np.asarray(chr_bytes, dtype=np.uint8)[:d["n_tiles"] * V.tile_bytes(d["tile_format"], (tw, th))], (tw, th),
                           d["tile_format"])
    have = np.zeros((h, w), dtype=bool)
    value, base, behind = (np.zeros((h, w), dtype=np.int64) for _ in range(3))
    for j in range(n - 1, -1, -1):  # the lowest index is painted last, so it wins
        rows = np.flatnonzero(shown[j])
        if len(rows) == 0:
            continue
        o = objects[j]
        ox, oy, attr = int(o["x"]), int(o["y"]), int(o["attr"])
        xs = np.arange(max(0, ox), min(w, ox + tw), dtype=np.int64)
        if len(xs) == 0:
            continue
        px, py = xs - ox, rows - oy
        px = tw - 1 - px if attr & FLIP_X else px
        py = th - 1 - py if attr & FLIP_Y else py
        v = tiles[int(o["tile"])][py[:, None], px[None, :]].astype(np.int64)
        solid = np.ones_like(v, dtype=bool) if d["opaque"] else v != 0
        at = (rows[:, None], xs[None, :])
        have[at] |= solid
        value[at] = np.where(solid, v, value[at])
        base[at] = np.where(solid, d["pal_base"] + (attr & 0xFF) * d["sub_size"], base[at])
        behind[at] = np.where(solid, int(bool(attr & BEHIND)), behind[at])
    written = have.copy()
    if bg_index is not None:
        written &= ~((behind != 0) & (bg_index.astype(np.int64) % d["bg_sub_size"] != 0))
    i = np.minimum(base + value, d["n_colors"] - 1).astype(np.uint8)
    if index is not None:
        index[written] = i[written]
    if fb is not None:
        fb[written] = S.palette_rgba(pal_words, d["pal_format"], d["n_colors"])[i[written]]
    return fb, index, int(bad.sum()), over


def draw_loop(d, chr_bytes, objects, pal_words=None, bg_index=None, fb=None, index=None, count=None):
    w, h, tw, th = d["width"], d["height"], d["tile_w"], d["tile_h"]
    n = d["n_objects"] if count is None else min(count, d["n_objects"])
    data = bytes(np.asarray(chr_bytes, dtype=np.uint8).reshape(-1))
    records = [tuple(int(v) for v in o) for o in np.asarray(objects, dtype=OBJECT).reshape(-1)[:n].tolist()]
    fb = None if fb is None else np.array(fb, dtype=np.uint8).reshape(h, w, 4)
    index = None if index is None else np.array(index, dtype=np.uint8).reshape(h, w)
    if isinstance(bg_index, str):
        bg_index = index.copy()
    elif bg_index is not None:
        bg_index = np.asarray(bg_index, dtype=np.uint8).reshape(h, w)
    colours = None if fb is None else S.palette_rgba_loop(pal_words, d["pal_format"], d["n_colors"])
    live, n_bad = [], 0
    for x, y, tile, attr in records:
        if attr & HIDDEN:
            live.append(False)
            continue
        wrong = tile < 0 or tile >= d["n_tiles"] or not -32768 <= x <= 32767 or not -32768 <= y <= 32767
        n_bad += int(wrong)
        live.append(not wrong)
    over = 0
    for y in range(h):
        on_line = [j for j in range(n) if live[j] and records[j][1] <= y < records[j][1] + th]
        over += max(0, len(on_line) - d["line_limit"])
        on_line = on_line[:d["line_limit"]]
        for x in range(w):
            for j in on_line:
                ox, oy, tile, attr = records[j]
                if not ox <= x < ox + tw:
                    continue
                px, py = x - ox, y - oy
                v = S.pixel_value_loop(data, d["tile_format"], (tw, th), tile, tw - 1 - px if attr & FLIP_X else px,
                                       th - 1 - py if attr & FLIP_Y else py)
                if v == 0 and not d["opaque"]:
                    continue
                if attr & BEHIND and bg_index is not None and int(bg_index[y, x]) % d["bg_sub_size"] != 0:
                    break  # the winner is behind the background: nothing is written
                i = min(d["pal_base"] + (attr & 0xFF) * d["sub_size"] + v, d["n_colors"] - 1)
                if index is not None:
                    index[y, x] = i
                if fb is not None:
                    fb[y, x] = colours[i]
                break
    return fb, index, n_bad, over


# ---- from_maps -------------------------------------------------------------------------------------------------------------

def from_maps(map_bg, map_words, grid, tile, capacity, cells_bg=None, cells=None, origin=(0, 0)):
    """(the min(D, capacity) OBJECT records, D)."""
    map_bg, map_words = (np.asarray(m, dtype=np.uint32).reshape(-1) for m in (map_bg, map_words))
    differs = map_bg != map_words
    if cells is not None:
        differs |= np.asarray(cells_bg, dtype=np.uint8).reshape(-1) != np.asarray(cells, dtype=np.uint8).reshape(-1)
    c = np.flatnonzero(differs)
    total = len(c)
    c = c[:capacity]
    out = np.zeros(len(c), dtype=OBJECT)
    word = map_words[c].astype(np.int64)
    out["x"], out["y"] = origin[0] + (c % grid[0]) * tile[0], origin[1] + (c // grid[0]) * tile[1]
    out["tile"] = word & V.ID_MASK
    p = np.zeros(len(c), dtype=np.int64) if cells is None else np.asarray(cells, dtype=np.uint8).reshape(-1)[c].astype(np.int64)
    out["attr"] = p | ((word >> 30) & 1) << 8 | ((word >> 31) & 1) << 9
    return out, total


def from_maps_loop(map_bg, map_words, grid, tile, capacity, cells_bg=None, cells=None, origin=(0, 0)):
    records, total = [], 0
    for c in range(grid[0] * grid[1]):
        a, b = int(map_bg[c]), int(map_words[c])
        if a == b and (cells is None or int(cells_bg[c]) == int(cells[c])):
            continue
        total += 1
        if len(records) < capacity:
            p = 0 if cells is None else int(cells[c])
            records.append((origin[0] + (c % grid[0]) * tile[0], origin[1] + (c // grid[0]) * tile[1], b % (1 << 30),
                            p + 256 * ((b >> 30) & 1) + 512 * (b >> 31)))
    return objects_of(records) if records else np.zeros(0, dtype=OBJECT), total


# ---- OAM -------------------------------------------------------------------------------------------------------------------

def fits(fmt, objects):
    o = np.asarray(objects, dtype=OBJECT).reshape(-1)
    x, y, t, p = o["x"].astype(np.int64), o["y"].astype(np.int64), o["tile"].astype(np.int64), o["attr"].astype(np.int64) & 0xFF
    if fmt == OAM_NES:
        return (1 <= y) & (y <= 256) & (0 <= x) & (x <= 255) & (0 <= t) & (t <= 255) & (p <= 3)
    return (-16 <= y) & (y <= 239) & (-8 <= x) & (x <= 247) & (0 <= t) & (t <= 255) & (p <= 7)


def pack(fmt, objects):
    """((n, 4) uint8, the shown objects that do not fit)."""
    o = np.asarray(objects, dtype=OBJECT).reshape(-1)
    x, y, t, a = (o[f].astype(np.int64) for f in ("x", "y", "tile", "attr"))
    hidden = (a & HIDDEN) != 0
    fx, fy, behind = (a >> 8) & 1, (a >> 9) & 1, (a >> 10) & 1
    if fmt == OAM_NES:
        cols = [np.where(hidden, 0xFF, y - 1), t, (a & 3) | behind << 5 | fx << 6 | fy << 7, x]
    else:
        cols = [np.where(hidden, 0, y + 16), x + 8, t, (a & 7) | fx << 5 | fy << 6 | behind << 7]
    return np.stack([c & 0xFF for c in cols], axis=1).astype(np.uint8), int((~hidden & ~fits(fmt, o)).sum())


def pack_loop(fmt, objects):
    out, bad = [], 0
    for x, y, t, a in np.asarray(objects, dtype=OBJECT).reshape(-1).tolist():
        hidden, p, fx, fy, behind = bool(a & HIDDEN), a % 256, (a >> 8) % 2, (a >> 9) % 2, (a >> 10) % 2
        if fmt == OAM_NES:
            ok = 1 <= y <= 256 and 0 <= x <= 255 and 0 <= t <= 255 and p <= 3
            row = [255 if hidden else (y - 1) % 256, t % 256, p % 4 + 32 * behind + 64 * fx + 128 * fy, x % 256]
        else:
            ok = -16 <= y <= 239 and -8 <= x <= 247 and 0 <= t <= 255 and p <= 7
            row = [0 if hidden else (y + 16) % 256, (x + 8) % 256, t % 256, p % 8 + 32 * fx + 64 * fy + 128 * behind]
        bad += int(not hidden and not ok)
        out.append(row)
    return np.array(out, dtype=np.uint8).reshape(-1, 4), bad


def unpack(fmt, data):
    b = np.asarray(data, dtype=np.uint8).reshape(-1, 4).astype(np.int64)
    out = np.zeros(len(b), dtype=OBJECT)
    if fmt == OAM_NES:
        a = b[:, 2]
        out["y"], out["tile"], out["x"] = b[:, 0] + 1, b[:, 1], b[:, 3]
        out["attr"] = (a & 3) | ((a >> 6) & 1) << 8 | ((a >> 7) & 1) << 9 | ((a >> 5) & 1) << 10
    else:
        a = b[:, 3]
        out["y"], out["x"], out["tile"] = b[:, 0] - 16, b[:, 1] - 8, b[:, 2]
        out["attr"] = (a & 7) | ((a >> 5) & 1) << 8 | ((a >> 6) & 1) << 9 | ((a >> 7) & 1) << 10
    return out


def unpack_loop(fmt, data):
    records = []
    for b in np.asarray(data, dtype=np.uint8).reshape(-1, 4).tolist():
        if fmt == OAM_NES:
            a = b[2]
            records.append((b[3], b[0] + 1, b[1], a % 4 + 256 * ((a // 64) % 2) + 512 * (a // 128) + 1024 * ((a // 32) % 2)))
        else:
            a = b[3]
            records.append((b[1] - 8, b[0] - 16, b[2], a % 8 + 256 * ((a // 32) % 2) + 512 * ((a // 64) % 2) + 1024 * (a // 128)))
    return objects_of(records)


# ---- inputs ----------------------------------------------------------------------------------------------------------------

def random_table(rng, d, n, spread=24, hidden_share=0.1, bad_share=0.1, behind_share=0.0, sub_palettes=4):
    """n random objects round the screen of descriptor d, edge-straddling and off-screen ones among them, with flips, some
    hidden, some bad (a tile past n_tiles, a negative tile, a position past int16)."""
    o = np.zeros(n, dtype=OBJECT)
    o["x"] = rng.integers(-spread, d["width"] + spread, n)
    o["y"] = rng.integers(-spread, d["height"] + spread, n)
    o["tile"] = rng.integers(0, d["n_tiles"], n)
    attr = rng.integers(0, sub_palettes, n) | rng.integers(0, 4, n) << 8 | rng.integers(0, 16, n) << 12
    attr |= (rng.random(n) < behind_share).astype(np.int64) << 10
    attr |= (rng.random(n) < hidden_share).astype(np.int64) << 11
    o["attr"] = attr
    wrong = np.flatnonzero(rng.random(n) < bad_share)
    for k, j in enumerate(wrong):
        if k % 4 == 0:
            o["tile"][j] = d["n_tiles"] + k
        elif k % 4 == 1:
            o["tile"][j] = -1 - k
        elif k % 4 == 2:
            o["x"][j] = 32768 + k
        else:
            o["y"][j] = -32769 - k
    return o


def random_chr(rng, d):
    tiles = rng.integers(0, 1 << V.BPP[d["tile_format"]], (d["n_tiles"], d["tile_h"], d["tile_w"]), dtype=np.uint8)
    tiles[rng.random(tiles.shape) < 0.4] = 0  # holes to see through
    return V.encode_tiles(tiles, (d["tile_w"], d["tile_h"]), d["tile_format"])[0]
