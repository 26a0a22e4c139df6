"""ctypes / numpy mirrors of include/par_types.h.

Layouts follow the reference byte for byte (spr = src/sprites.hpp, alt = src/alternative.cpp):
Color spr:5-17, Vector<float> spr:20-51, Pixel spr:53-58, Sprite spr:67-71, AABB alt:35-38,88, Light alt:619-622,
Ray alt:30-33.
"""
import ctypes as C

import numpy as np

SPRITE_W = 20
SPRITE_H = 40
SPRITE_TEXELS = SPRITE_W * SPRITE_H
SLOTS = 8
MAX_PALETTE = 256
PALIDX_BACKGROUND = 0xFF
MAX_SCALE = 16
PRESENT_RGBA, PRESENT_BGRA = 0, 1
UPSCALE_SCALE2X, UPSCALE_SCALE3X, UPSCALE_SCALE4X = 2, 3, 4  # the value is the factor

COLOR = np.dtype([("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
VEC3 = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
PIXEL = np.dtype([("normal", VEC3), ("color", COLOR), ("y", "<i4"), ("z", "<i4"), ("entity_index", "<i4")])
SPRITE = np.dtype([("color", "<i4", (SPRITE_TEXELS,)), ("depth", "<i4", (SPRITE_TEXELS,)),
                   ("normal", VEC3, (SPRITE_TEXELS,))])
AABB = np.dtype([("px", "<i2"), ("py", "<i2"), ("pz", "<i2"), ("ex", "<i2"), ("ey", "<i2"), ("ez", "<i2"),
                 ("pad", "<i2", (2,))])
LIGHT = np.dtype([("x", "<i2"), ("y", "<i2"), ("z", "<i2"), ("radius", "<i2")])
LIGHT_TINT = np.dtype([("r", "<f4"), ("g", "<f4"), ("b", "<f4")])  # par_light_tint
OUTLINE_STYLE = np.dtype([("depth_step", "<i4"), ("silhouette_scale", "<i4"), ("crease_scale", "<i4")])  # par_outline_style
PRESENT_DESC = np.dtype([("scale_x", "<i4"), ("scale_y", "<i4"), ("pitch", "<i4"), ("order", "<i4")])  # par_present_desc
UPSCALE_DESC = np.dtype([("scaler", "<i4"), ("pitch", "<i4"), ("order", "<i4")])  # par_upscale_desc
PALETTE_CELLS = 32768  # PAR_PALETTE_CELLS
# par_palette_work: one element is the whole block (np.zeros(1, dtype=PALETTE_WORK))
PALETTE_WORK = np.dtype([("hist", "<u4", (PALETTE_CELLS,)), ("sums", "<u8", (MAX_PALETTE, 4)),
                         ("lut", "u1", (PALETTE_CELLS,)), ("n_entries", "<i4"), ("reserved", "<i4", (3,))])
# par_palette_refine_work: one element is the whole block
PALETTE_REFINE_WORK = np.dtype([("bins", "<u4", (MAX_PALETTE, 3, 16)), ("rank", "<u4", (MAX_PALETTE, 4)),
                                ("high", "<u4", (MAX_PALETTE,))])
RAY = np.dtype([("inv_x", "<f4"), ("inv_y", "<f4"), ("inv_z", "<f4"), ("ox", "<i2"), ("oy", "<i2"), ("oz", "<i2"),
                ("pad", "<i2")])

assert COLOR.itemsize == 4 and VEC3.itemsize == 12 and PIXEL.itemsize == 28
assert SPRITE.itemsize == 16000 and AABB.itemsize == 16 and LIGHT.itemsize == 8 and RAY.itemsize == 20
assert LIGHT_TINT.itemsize == 12 and OUTLINE_STYLE.itemsize == 12 and PRESENT_DESC.itemsize == 16
assert UPSCALE_DESC.itemsize == 12 and PALETTE_WORK.itemsize == 172048 and PALETTE_REFINE_WORK.itemsize == 54272


class Color(C.Structure):
    _fields_ = [("red", C.c_uint8), ("green", C.c_uint8), ("blue", C.c_uint8), ("alpha", C.c_uint8)]


class Params(C.Structure):
    """par_params: the reference's constexpr view/grid constants (alt:116-131) as run-time values."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("length", C.c_int32), ("bin_size", C.c_int32),
                ("ambient", C.c_float), ("background", C.c_uint8), ("reserved_", C.c_uint8 * 3),
                ("palette_size", C.c_int32), ("palette", Color * MAX_PALETTE)]

    def grid_dims(self):
        b = self.bin_size
        return ((self.width + b - 1) // b, (self.height + b - 1) // b, (self.length + b - 1) // b)


class Outputs(C.Structure):
    """par_outputs: nullable output planes, each addressing the element of (row_begin, 0)."""
    _fields_ = [("fb", C.c_void_p), ("gbuf", C.c_void_p), ("palidx", C.c_void_p), ("brightness", C.c_void_p),
                ("lit", C.c_void_p)]


class FrameStats(C.Structure):
    _fields_ = [("entities", C.c_int64), ("bin_insertions", C.c_int64), ("shadow_rays", C.c_int64),
                ("occupied_columns", C.c_int64), ("overflow_columns", C.c_int64),
                ("ms_bin", C.c_float), ("ms_fill", C.c_float), ("ms_render", C.c_float),
                ("ms_overflow", C.c_float), ("ms_launch", C.c_float * 5), ("render_merged", C.c_int32)]


class PaletteWork(C.Structure):
    """par_palette_work as a ctypes structure (PALETTE_WORK is the same layout as a numpy dtype)."""
    _fields_ = [("hist", C.c_uint32 * PALETTE_CELLS), ("sums", (C.c_uint64 * 4) * MAX_PALETTE),
                ("lut", C.c_uint8 * PALETTE_CELLS), ("n_entries", C.c_int32), ("reserved", C.c_int32 * 3)]


assert C.sizeof(PaletteWork) == PALETTE_WORK.itemsize


class PaletteRefineWork(C.Structure):
    """par_palette_refine_work as a ctypes structure (PALETTE_REFINE_WORK is the same layout as a numpy dtype)."""
    _fields_ = [("bins", ((C.c_uint32 * 16) * 3) * MAX_PALETTE), ("rank", (C.c_uint32 * 4) * MAX_PALETTE),
                ("high", C.c_uint32 * MAX_PALETTE)]


assert C.sizeof(PaletteRefineWork) == PALETTE_REFINE_WORK.itemsize


def palette_cell(colors):
    """The histogram cell of each entry of a COLOR array: red >> 3 | green >> 3 << 5 | blue >> 3 << 10."""
    return ((colors["red"].astype(np.int32) >> 3) | ((colors["green"].astype(np.int32) >> 3) << 5) |
            ((colors["blue"].astype(np.int32) >> 3) << 10))


def default_params(width=480, height=320, length=None, bin_size=40):
    """Reference defaults (alt:116-119, 281, 702; spr:60-65) with an optional view size; length defaults to height
    as in the reference (alt:118-119)."""
    p = Params()
    p.width, p.height = width, height
    p.length = height if length is None else length
    p.bin_size = bin_size
    p.ambient = 0.25
    p.background = 255 // 2
    p.palette_size = 4
    for i, g in enumerate((100, 140, 200, 240)):
        p.palette[i] = Color(g, g, g, 0)
    return p


def make_light(x, y, z, radius=10):
    l = np.zeros(1, dtype=LIGHT)
    l["x"], l["y"], l["z"], l["radius"] = x, y, z, radius
    return l


def make_tints(rows):
    """LIGHT_TINT array from an iterable of (r, g, b), one per light (par_set_light_tints; white is (1, 1, 1))."""
    rows = list(rows)
    t = np.zeros(len(rows), dtype=LIGHT_TINT)
    for i, rgb in enumerate(rows):
        t[i]["r"], t[i]["g"], t[i]["b"] = rgb
    return t


def make_outline_style(depth_step=4, silhouette_scale=128, crease_scale=320):
    """1-element OUTLINE_STYLE array (par_outline_device): the depth difference from which an edge between two entities
    is a silhouette, and the 8.8 fixed-point factors of a silhouette's and a crease's colour (256 = unchanged)."""
    s = np.zeros(1, dtype=OUTLINE_STYLE)
    s["depth_step"], s["silhouette_scale"], s["crease_scale"] = depth_step, silhouette_scale, crease_scale
    return s


def make_present_desc(scale_x=1, scale_y=None, pitch=None, order=PRESENT_RGBA, width=None):
    """1-element PRESENT_DESC array (par_present_device): the integer scales (scale_y defaults to scale_x), the bytes
    from one output row to the next (default: tight, 4 * width * scale_x, which needs `width`) and the byte order."""
    scale_y = scale_x if scale_y is None else scale_y
    if pitch is None:
        if width is None:
            raise ValueError("make_present_desc: give pitch, or width for a tight pitch")
        pitch = 4 * width * scale_x
    d = np.zeros(1, dtype=PRESENT_DESC)
    d["scale_x"], d["scale_y"], d["pitch"], d["order"] = scale_x, scale_y, pitch, order
    return d


def make_upscale_desc(scaler, pitch=None, order=PRESENT_RGBA, width=None):
    """1-element UPSCALE_DESC array (par_upscale_device): the scaler (its value is the factor), the bytes from one row
    of the surface to the next (default: tight, 4 * width * scaler, which needs `width`) and the byte order."""
    if pitch is None:
        if width is None:
            raise ValueError("make_upscale_desc: give pitch, or width for a tight pitch")
        pitch = 4 * width * scaler
    d = np.zeros(1, dtype=UPSCALE_DESC)
    d["scaler"], d["pitch"], d["order"] = scaler, pitch, order
    return d


def make_aabbs(rows):
    """AABB array from an iterable of (px, py, pz, ex, ey, ez)."""
    rows = list(rows)
    a = np.zeros(len(rows), dtype=AABB)
    for i, r in enumerate(rows):
        a[i]["px"], a[i]["py"], a[i]["pz"], a[i]["ex"], a[i]["ey"], a[i]["ez"] = r
    return a


def ptr(a):
    """void* of a C-contiguous numpy array (None -> NULL)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)
