"""Objects: a tile machine's sprite layer drawn over its background, and the object table a frame needs over a kept
background (addons/include/par_objects.h). An add-on: the nine calls live in a library of their own,
lib/libpar_objects.so, which this module loads itself at the first call; their signatures are ABI_OBJECTS below, a table
that is NOT one of abi.py's (the core library exports none of them), and the package does not import this module. The calls
raise the package's ParError with the symbol's name; a device pointer or a stream is an int or None.

    objects = importlib.import_module("pixel-art-raytracer_amd.objects")
"""
import ctypes as C
import os
import sys

import numpy as np

from .types import ptr

_par = sys.modules[__package__]  # the package module: its ParError, _ok and _dp, and the HIP runtime it shares with torch

_p, _i = C.c_void_p, C.c_int
# addons/include/par_objects.h, in its order
ABI_OBJECTS = {
    "par_objects_work_bytes": (C.c_size_t, [_i, _i]),
    "par_objects_from_maps_work_bytes": (C.c_size_t, [_i]),
    "par_objects_machine_limits": [_i, _p, _p],
    "par_objects_pack": [_i, _p, _i, _p, _p],
    "par_objects_unpack": [_i, _p, _i, _p],
    "par_objects_draw_device": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p],
    "par_objects_from_maps_device": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p],
    "par_objects_draw_host": [_i, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p],
    "par_objects_from_maps_host": [_i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p],
}
ABI_OBJECTS_SYMBOLS = tuple(ABI_OBJECTS)
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libpar_objects.so")
MAX_OBJECTS, MAX_LINE, MAX_TILES, MAX_CELLS, MAX_SIDE = 65536, 128, 1 << 20, 1 << 20, 4096
# the bits of par_object.attr above the sub-palette
FLIP_X, FLIP_Y, BEHIND, HIDDEN = 1 << 8, 1 << 9, 1 << 10, 1 << 11
# enum par_objects_tile_format
FORMAT_1BPP, FORMAT_2BPP_PLANAR, FORMAT_2BPP_ROWS, FORMAT_4BPP_ROWS, FORMAT_4BPP_PACKED_HI, FORMAT_4BPP_PACKED_LO, \
    FORMAT_4BPP_ROW_PLANES = range(7)
FORMATS = tuple(range(7))
BPP = (1, 2, 2, 4, 4, 4, 4)
# enum par_objects_palette_format, and the bytes of an entry
BGR555, BGR333_MD, BGR222, RGBA8 = range(4)
PALETTE_ENTRY_BYTES = (2, 2, 1, 4)
# enum par_objects_machine, enum par_objects_oam_format
NES, GBC, SMS, MEGADRIVE, SNES, GBA = range(6)
OAM_NES, OAM_GB = range(2)
DESC_FIELDS = ("tile_w", "tile_h", "tile_format", "n_tiles", "n_objects", "line_limit", "pal_format", "n_colors", "sub_size",
               "pal_base", "bg_sub_size", "opaque", "width", "height")
# par_object as a numpy record: four int32, 16 bytes
OBJECT = np.dtype([("x", np.int32), ("y", np.int32), ("tile", np.int32), ("attr", np.int32)])


class Desc(C.Structure):
    """par_objects_desc: the tiles, the table, the palette and the screen."""
    _fields_ = [(name, C.c_int32) for name in DESC_FIELDS]


def desc(**fields):
    """A Desc with `fields` on top of a bg_sub_size of 1."""
    d = Desc()
    d.bg_sub_size = 1
    for name, value in fields.items():
        if name not in DESC_FIELDS:
            raise TypeError(f"desc: par_objects_desc has no field {name}")
        setattr(d, name, value)
    return d


_lib = None


def lib():
    """libpar_objects.so with the table set on its functions, loaded at the first call (the package's loader). No fallback."""
    global _lib
    if _lib is None:
        _lib = _par._load(LIB_PATH, ABI_OBJECTS)
    return _lib


def work_bytes(height, line_limit):
    """The bytes of the work block of a draw (par_objects_work_bytes); 0 outside the limits."""
    return lib().par_objects_work_bytes(height, line_limit)


def from_maps_work_bytes(n_cells):
    """The bytes of the work block of a from_maps (par_objects_from_maps_work_bytes); 0 outside the limits."""
    return lib().par_objects_from_maps_work_bytes(n_cells)


def machine_limits(machine):
    """(objects a scanline, objects in all) of a machine (par_objects_machine_limits)."""
    line, most = C.c_int(0), C.c_int(0)
    _par._ok(lib().par_objects_machine_limits, machine, C.byref(line), C.byref(most))
    return line.value, most.value


def _records(who, objects):
    objects = np.ascontiguousarray(objects)
    if objects.dtype != OBJECT:
        raise ValueError(f"{who}: the objects are {objects.dtype}, not OBJECT records")
    return objects.reshape(-1)


def pack(fmt, objects):
    """OBJECT records as OAM bytes of format `fmt` (par_objects_pack): ((n, 4) uint8, the shown objects that do not fit)."""
    objects = _records("pack", objects)
    out, bad = np.zeros((max(1, len(objects)), 4), dtype=np.uint8), C.c_int(0)
    _par._ok(lib().par_objects_pack, fmt, ptr(objects), len(objects), ptr(out), C.byref(bad))
    return out[:len(objects)], bad.value


def unpack(fmt, data):
    """OAM bytes of format `fmt` as OBJECT records (par_objects_unpack)."""
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    if len(data) % 4:
        raise ValueError(f"unpack: the data holds {len(data)} bytes, no whole number of objects of 4")
    out = np.zeros(max(1, len(data) // 4), dtype=OBJECT)
    _par._ok(lib().par_objects_unpack, fmt, ptr(data), len(data) // 4, ptr(out))
    return out[:len(data) // 4]


def draw(d, chr_data, objects, work, pal_words=None, fb_io=None, index_io=None, count=None, bg_index=None, bad_out=None,
         over_out=None, stream=None):
    """Device pointers (ints): the objects at `objects` drawn from the tile data at `chr_data` and the colour words at
    `pal_words` over fb_io (RGBA8) and/or index_io (a byte a pixel), under Desc `d` (par_objects_draw_device). `count` is a
    device uint32 or None (n_objects), bg_index the background's indices for `behind` or None, `work`
    work_bytes(height, line_limit) bytes of anything; bad_out and over_out are uint32s that get the bad objects and the
    objects dropped over the scanlines. Asynchronous on `stream`."""
    dp = _par._dp
    _par._ok(lib().par_objects_draw_device, dp(stream), C.byref(d), dp(chr_data), dp(objects), dp(count), dp(pal_words), dp(bg_index),
             dp(work), dp(fb_io), dp(index_io), dp(bad_out), dp(over_out))


def from_maps(map_bg, map_words, grid, tile, capacity, work, objects_out, count_out, cells_bg=None, cells=None, origin=(0, 0),
              stream=None):
    """Device pointers (ints): the cells of the grid[0] x grid[1] tile map at `map_words` that differ from those at `map_bg`
    (or whose cell bytes differ) as objects of tile[0] x tile[1] pixels from `origin` on, at most `capacity` at
    objects_out and their number at count_out (par_objects_from_maps_device). `work` is from_maps_work_bytes(cells) bytes.
    Asynchronous on `stream`."""
    dp = _par._dp
    _par._ok(lib().par_objects_from_maps_device, dp(stream), dp(map_bg), dp(cells_bg), dp(map_words), dp(cells), grid[0], grid[1], tile[0],
             tile[1], origin[0], origin[1], capacity, dp(work), dp(objects_out), dp(count_out))


def _bytes_of(who, what, array, want):
    array = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
    if len(array) != want:
        raise ValueError(f"{who}: {what} holds {len(array)} bytes, the descriptor wants {want}")
    return array


def draw_host(d, chr_data, objects, pal_words=None, fb=None, index=None, count=None, bg_index=None, device=-1):
    """The same on host arrays (par_objects_draw_host). `fb` ((height, width, 4) uint8) and `index` ((height, width) uint8)
    are the planes to draw over, or None; they are not changed. bg_index is an array, None, or the string "index" for the
    index plane itself. Returns {"fb": the plane drawn over or None, "index": the same, "bad": the bad objects, "over":
    the objects dropped}."""
    who = "draw_host"
    w, h = max(0, d.width), max(0, d.height)
    each = 8 * BPP[d.tile_format] * (d.tile_w // 8) * (d.tile_h // 8) if 0 <= d.tile_format < 7 else 0
    chr_data = _bytes_of(who, "chr", chr_data, max(0, d.n_tiles) * max(0, each))
    objects = _records(who, objects)
    if len(objects) != d.n_objects:
        raise ValueError(f"{who}: {len(objects)} objects, the descriptor wants {d.n_objects}")
    if pal_words is not None:
        pal_words = _bytes_of(who, "the palette", pal_words, max(0, d.n_colors) * (PALETTE_ENTRY_BYTES[d.pal_format] if 0 <= d.pal_format < 4 else 1))
    fb_io = None if fb is None else _bytes_of(who, "fb", fb, 4 * w * h).copy().reshape(h, w, 4)
    index_io = None if index is None else _bytes_of(who, "index", index, w * h).copy().reshape(h, w)
    if isinstance(bg_index, str):
        if bg_index != "index" or index_io is None:
            raise ValueError(f"{who}: bg_index names a plane that is not given")
        bg_index = index_io
    elif bg_index is not None:
        bg_index = _bytes_of(who, "bg_index", bg_index, w * h)
    bad, over = C.c_int(0), C.c_int(0)

    def p(a):
        return None if a is None else ptr(a)

    _par._ok(lib().par_objects_draw_host, device, C.byref(d), p(chr_data), p(objects), d.n_objects if count is None else count,
             p(pal_words), p(bg_index), p(fb_io), p(index_io), C.byref(bad), C.byref(over))
    return {"fb": fb_io, "index": index_io, "bad": bad.value, "over": over.value}


def from_maps_host(map_bg, map_words, grid, tile, capacity, cells_bg=None, cells=None, origin=(0, 0), device=-1):
    """The same on host arrays (par_objects_from_maps_host). Returns {"objects": the min(D, capacity) OBJECT records,
    "count": D}."""
    who = "from_maps_host"
    n = max(0, grid[0]) * max(0, grid[1])
    map_bg, map_words = (np.ascontiguousarray(m, dtype=np.uint32).reshape(-1) for m in (map_bg, map_words))
    if len(map_bg) != n or len(map_words) != n:
        raise ValueError(f"{who}: the maps hold {len(map_bg)} and {len(map_words)} words, the grid has {n} cells")
    if cells_bg is not None:
        cells_bg = _bytes_of(who, "cells_bg", cells_bg, n)
    if cells is not None:
        cells = _bytes_of(who, "cells", cells, n)
    out, count = np.zeros(max(1, capacity), dtype=OBJECT), C.c_int(0)

    def p(a):
        return None if a is None else ptr(a)

    _par._ok(lib().par_objects_from_maps_host, device, p(map_bg), p(cells_bg), p(map_words), p(cells), grid[0], grid[1], tile[0], tile[1],
             origin[0], origin[1], capacity, p(out), C.byref(count))
    return {"objects": out[:max(0, min(count.value, capacity))], "count": count.value}
