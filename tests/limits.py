"""Scenes, views and helpers of the tests at the size limits (test_limits_cpu.py, test_gpu_limits.py): grids 1024 bins
wide, tall or deep, coordinates at the ends of int16, and the row-block form of the oracle that a view of 8192 x 8192
needs (its whole G-buffer is 1.9 GB). Imports without a GPU.

Where a box lands: it covers the columns [px, px + ex) and the screen rows [top, top + ey + ez) with
top = H - (py + pz) - (ey + ez), lies in the z bins of [pz, pz + ez], and the tile floor's depths put its pixels at
z = pz .. pz + 19. `box()` places one by its top row."""
import ctypes as C
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import sequences as SQ
import sprites as SP

T = SP.T
NTHREADS = min(os.cpu_count() or 8, 16)
ALL = ("fb", "gbuf", "palidx", "brightness", "lit")
STACK = 43  # boxes of one bin: the slot counter wraps five times and ends at 3; more pairs than a column record holds
I16_MIN, I16_MAX = -32768, 32767

# name: (width, height, length, bin size, the axes at their limit, the row blocks rendered (None: the whole frame))
VIEWS = {"widest grid": (8192, 48, 64, 8, "x", None),
         "tallest grid": (64, 8192, 64, 8, "y", None),
         "wide and tall": (8192, 8192, 8, 8, "xy", ((0, 24), (4093, 4107), (8168, 8192))),
         "int16 wide": (32767, 64, 64, 32, "x", None),
         "int16 tall": (64, 32767, 64, 32, "y", None),
         "int16 deep": (64, 64, 32767, 32, "z", None)}
GRIDS = {"widest grid": (1024, 6, 8), "tallest grid": (8, 1024, 8), "wide and tall": (1024, 1024, 1),
         "int16 wide": (1024, 2, 2), "int16 tall": (2, 1024, 2), "int16 deep": (2, 2, 1024)}
INT16_VIEWS = ("int16 wide", "int16 tall", "int16 deep")
# the boxes every int16 view gets: (px, py, pz, ex, ey, ez)
INT16_PX = (32747, 32766, 32767, -20, -19)
SEED = 20261020


def params_of(view):
    W, H, L, B = VIEWS[view][:4]
    return T.default_params(W, H, L, B)


def blocks_of(view):
    return VIEWS[view][5] or ((0, VIEWS[view][1]),)


def box(H, x, top, z, e):
    """(px, py, pz, ex, ey, ez) of the box of extents `e` whose first screen row is `top`, or None when py leaves int16."""
    py = H - top - (e[1] + e[2]) - z
    if not (I16_MIN <= py <= I16_MAX and I16_MIN <= x <= I16_MAX and I16_MIN <= z <= I16_MAX):
        return None
    return (x, py, z) + tuple(e)


def _spans(n, B, lead):
    """Ranges of an axis of n units to draw positions from: around its first bin (from `lead` before it), its middle, and
    across its last two bins, the clipped last one included."""
    last = (n - 1) // B * B
    return [(-lead, min(n, B + 12)), (max(0, n // 2 - 20), min(n, n // 2 + 20)), (max(-lead, last - B - lead), n)]


@functools.lru_cache(maxsize=None)
def scene(view):
    """(params, aabbs, sprites, sprite ids, info) of a view: `info` names the entities of each purpose."""
    W, H, L, B, _, blocks = VIEWS[view]
    gx, gy, gz = GRIDS[view]
    params = params_of(view)
    assert params.grid_dims() == (gx, gy, gz)
    rng = np.random.default_rng(SEED + list(VIEWS).index(view))
    rows, info = [], {}

    # windows of the screen (x0, x1, row0, row1) kept clear of every box but those placed there on purpose: a box at an end
    # of int16 is seen only where nothing nearer covers it, and py = -32768 with pz = 32767 is the farthest box there is
    clear = {"int16 wide": [(W - 21, W, 0, 50), (0, 1, 0, 30)], "int16 deep": [(2, 24, 24, H)]}.get(view, [])

    def add(b, meant=False):
        if b is None:
            return False
        top = H - (b[1] + b[2]) - (b[4] + b[5])
        if not meant and any(b[0] < x1 and b[0] + b[3] > x0 and top < r1 and top + b[4] + b[5] > r0 for x0, x1, r0, r1 in clear):
            return False
        rows.append(b)
        return True

    def extent():
        ex, ey, ez = int(rng.integers(1, 21)), int(rng.integers(0, 21)), int(rng.integers(0, 21))
        return (ex, ey, ez) if ey + ez else (ex, 1, 0)

    xs, zs = _spans(W, B, 19), _spans(L, B, 15)
    tops = [(max(-39, r0 - 39), r1) for r0, r1 in blocks] if blocks else _spans(H, B, 39)  # (rows: around every block)
    # every extent the sprite allows, in and across the first and the last bins of every axis
    for xr in xs:
        for tr in tops:
            for zr in zs:
                for _ in range(7):
                    add(box(H, int(rng.integers(*xr)), int(rng.integers(*tr)), int(rng.integers(*zr)), extent()))
    # whole cubes down the last bin column, along the last bin row, and in the last z bin
    x_last, z_last = (gx - 1) * B, (gz - 1) * B
    for tr in tops:
        for top in range(tr[0], tr[1], 37):
            add(box(H, W - 14, top, int(rng.integers(0, max(1, min(L, 3 * B)))), (20, 20, 20)))
            add(box(H, max(0, x_last - 60), top, z_last, (20, 20, 20)))
    last_top = blocks[-1][1] if blocks else H
    for xr in xs:
        for x in range(xr[0], xr[1], 23):
            add(box(H, x, last_top - 27, int(rng.integers(0, max(1, min(L, 3 * B)))), (20, 20, 20)))
    if view in INT16_VIEWS:
        first = len(rows)
        for k, px in enumerate(INT16_PX):  # px + ex leaves int16; 32767 is culled where the view is 32767 wide
            add(box(H, px, 12 - 4 * k, 8, (20, 20, 20)), True)  # (each nearer than the one before)
            add(box(H, px, int(rng.integers(0, 30)), int(rng.integers(0, 20)), extent()))
        for py in (32700, 32720, 32727, 32767):  # py + ey + pz + ez leaves int16 (visible at the top of the tall view)
            for x in (5, 30, W - 10):
                add((x, py, int(rng.integers(0, 12)), 20, 20, 20))
        for x in (2, 40, W - 25, W - 3):  # seen in the last z bin of the deep view only
            add((x, I16_MIN, I16_MAX, 20, 20, 20), True)
            add((x + 2, I16_MIN, I16_MAX - 12, int(rng.integers(1, 21)), 13, 20), True)
        info["int16"] = list(range(first, len(rows)))
    # what the cull must drop
    first = len(rows)
    for k in range(4):
        add((I16_MIN, H // 2 - 10 * k, 5 * k, 20, 20, 20))
        add((10 * k, H // 2 - 10 * k, I16_MIN, 20, 20, 20))
    info["culled"] = list(range(first, len(rows)))
    # the stack: STACK small boxes of one bin of the last column, in the last bin row
    first = len(rows)
    top = (gy - 1) * B + 1
    for k in range(STACK):
        ok = add(box(H, x_last + 1 + k % 3, top, 1 + k % 2, (int(rng.integers(1, 5)), 2, 2)))
        assert ok
    info["stack"] = list(range(first, len(rows)))
    info["stack_bin"] = (gx - 1, gy - 1, 0)
    # a bin holds at most SLOTS - 1 records once its counter has wrapped, so only a column of many z bins can hold more
    # than the device's record takes (sequences.COL_ENT records, COL_NB occupied bins): there, a box in each of 40 z bins
    info["deep_stack"] = gz * (T.SLOTS - 1) > SQ.COL_ENT
    if info["deep_stack"]:
        for bz in range(gz - 40, gz):
            ok = add(box(H, x_last + 2 + bz % 3, top + 6, bz * B + 4, (4, 3, 3)), True)
            assert ok
    aabbs = T.make_aabbs(rows)
    base = oracle().tile_floor()
    sprites = np.concatenate([base, SP.sprite(base, "unit", SP.SPRITE_SEED)])
    ids = SP.sprite_ids(len(aabbs))
    return params, aabbs, sprites, ids, info


@functools.lru_cache(maxsize=None)
def oracle():
    from oracle.oracle import Oracle
    return Oracle()


def inside_lights(view):
    """Three lights inside the view (0 <= x <= W, 0 <= z < L, 1 <= y + z <= H): mid view, by the last corner, by the first."""
    W, H, L = VIEWS[view][:3]
    out = []
    for x, s, z in ((W * 3 // 5, H // 2, L // 4), (W - 5, 6, L - 3), (3, H - 2, 2)):
        out.append((x, s - z, z))
    return out


def end_lights(view):
    """Lights at the int16 ends of each axis, the other two coordinates the first inside light's: as
    test_gpu_lights_edges.py has its lights far outside the volume, their bins are out of range and their flat indices
    alias; the oracle is the contract."""
    x, y, z = inside_lights(view)[0]
    return {"x-": (I16_MIN, y, z), "x+": (I16_MAX, y, z), "y-": (x, I16_MIN, z), "y+": (x, I16_MAX, z),
            "z-": (x, y, I16_MIN), "z+": (x, y, I16_MAX)}


def lights_array(positions):
    a = np.zeros(len(positions), dtype=T.LIGHT)
    for i, (x, y, z) in enumerate(positions):
        a[i]["x"], a[i]["y"], a[i]["z"], a[i]["radius"] = x, y, z, 10
    return a


# ---- the oracle for row blocks -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def grid(view):
    """The oracle's hash of a view's scene (computed once, left unchanged)."""
    params, aabbs = scene(view)[:2]
    return oracle().bin(params, aabbs)


def _shifted(a, r0, W):
    """The address the oracle's row entries take for a block's plane: that of row 0 of the whole plane, were it there.
    They touch rows [r0, r1) alone."""
    return None if a is None else C.c_void_p(a.ctypes.data - r0 * W * a.itemsize)


def render_block(params, grid_, sprites, ids, light, rows, planes=ALL, gbuf=None, nthreads=NTHREADS):
    """Rows [r0, r1) of the frame as oracle.render gives them, with memory for the block only: par_oracle_primary and
    par_oracle_shade on planes of the block's size. With `gbuf` (the block's G-buffer of an earlier call) the primary
    pass is skipped. Returns {plane: flat array of the block}."""
    lib = oracle().lib
    W = params.width
    r0, r1 = rows
    n = (r1 - r0) * W
    out = {k: np.zeros(n, dtype=SQ.DTYPE[k]) for k in ALL if k in planes or k == "gbuf"}
    if gbuf is not None:
        out["gbuf"] = gbuf
    g = grid_.c()
    light = np.ascontiguousarray(light, dtype=T.LIGHT)
    ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    shade = any(k in planes for k in ("fb", "brightness", "lit"))

    def part(t):
        a, b = r0 + (r1 - r0) * t // nthreads, r0 + (r1 - r0) * (t + 1) // nthreads
        if a == b:
            return
        if gbuf is None:
            lib.par_oracle_primary(C.byref(params), C.byref(g), T.ptr(sprites), T.ptr(ids), _shifted(out["gbuf"], r0, W),
                                   _shifted(out.get("palidx"), r0, W), a, b)
        if shade:
            lib.par_oracle_shade(C.byref(params), C.byref(g), _shifted(out["gbuf"], r0, W), T.ptr(light),
                                 _shifted(out.get("fb"), r0, W), _shifted(out.get("brightness"), r0, W),
                                 _shifted(out.get("lit"), r0, W), a, b)

    nthreads = max(1, min(nthreads, r1 - r0))
    if nthreads == 1:
        part(0)
    else:
        with ThreadPoolExecutor(nthreads) as ex:
            list(ex.map(part, range(nthreads)))
    return {k: v for k, v in out.items() if k in planes}


@functools.lru_cache(maxsize=None)
def base_frame(view):
    """The blocks' G-buffers and palette indices (they do not depend on a light): {rows: {"gbuf", "palidx"}}."""
    params, aabbs, sprites, ids, _ = scene(view)
    return {rows: render_block(params, grid(view), sprites, ids, lights_array([(0, 0, 0)]), rows, ("gbuf", "palidx"))
            for rows in blocks_of(view)}


@functools.lru_cache(maxsize=None)
def lit_frame(view, at):
    """The oracle's frame of a view under the one light at `at`, per rendered block: {rows: {plane: array}} (computed
    once, left unchanged). A whole view has the one block (0, H)."""
    params, aabbs, sprites, ids, _ = scene(view)
    out = {}
    for rows, base in base_frame(view).items():
        lit = render_block(params, grid(view), sprites, ids, lights_array([at]), rows, ("fb", "brightness", "lit"),
                           gbuf=base["gbuf"])
        out[rows] = dict(base, **lit)
    return out


def default_light(view):
    """The inside light of a view's one-light frames: the first under which the covered pixels of the last bin column, of
    the last bin row and of the last z bin each hold lit and shadowed ones (test_limits_cpu.py)."""
    return inside_lights(view)[{"tallest grid": 2, "int16 tall": 1}.get(view, 0)]


def covered(planes):
    return planes["palidx"] != T.PALIDX_BACKGROUND


def _tdiv(a, b):
    q = np.abs(a) // b  # C's division truncates towards zero
    return np.where(a < 0, -q, q)


def shadow_rays(params, grid_, gbuf, mask, at):
    """The lit plane of a block at the pixels of `mask` (its covered ones), zero elsewhere: alt:705-742 restated in numpy float32 per
    covered pixel around par_oracle_shadow. A light at an end of int16 is tens of thousands of probes from every pixel,
    and the background's rays are most of a frame's (test_limits_cpu.py holds this to par_oracle_shade)."""
    from helpers import light_bin
    f32 = np.float32
    W, H, B = params.width, params.height, params.bin_size
    idx = np.nonzero(mask)[0]
    wx = (idx % W).astype(np.int64)
    wy, wz = gbuf["y"][idx].astype(np.int64), gbuf["z"][idx].astype(np.int64)
    lx, ly, lz = (int(v) for v in at)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = [(lx - wx).astype(f32), (ly - wy).astype(f32), (lz - wz).astype(f32)]
        length = (np.abs(d[0]) + np.abs(d[1])) + np.abs(d[2])
        rays = np.zeros(len(idx), dtype=T.RAY)
        for k, v in zip(("inv_x", "inv_y", "inv_z"), d):
            rays[k] = f32(1) / (v / length)
    for k, v in zip(("ox", "oy", "oz"), (wx, wy, wz)):
        rays[k] = v.astype(np.int16)  # (short) casts of alt:720-722
    sb = np.stack([wx // B, _tdiv(H - wy - wz, B), _tdiv(wz, B)], axis=1)
    lb = light_bin(params, at)
    ent = gbuf["entity_index"][idx]
    lit = np.zeros(len(gbuf), dtype=np.uint8)
    shadow, g = oracle().lib.par_oracle_shadow, grid_.c()
    base, step = rays.ctypes.data, rays.itemsize
    for n in range(len(idx)):
        lit[idx[n]] = shadow(C.byref(g), int(sb[n, 0]), int(sb[n, 1]), int(sb[n, 2]), lb[0], lb[1], lb[2], int(ent[n]),
                             C.c_void_p(base + n * step), None)
    return lit


@functools.lru_cache(maxsize=None)
def covered_lit(view, at):
    """{rows: lit plane of the covered pixels} of a view under the one light at `at` (computed once, left unchanged)."""
    params = params_of(view)
    return {rows: shadow_rays(params, grid(view), base["gbuf"], covered(base), at) for rows, base in base_frame(view).items()}


def composed(view, positions):
    """({rows: expected planes}, the LIGHT array) of a frame under the lights at `positions`: test_gpu_lights.compose over
    the oracle's whole frame under the view's default light (a background pixel's fb and brightness are the same under
    every light: its normal is zero) and, for every other light, the lit plane of the covered pixels alone. The `lit`
    plane of such a frame is right at covered pixels only: compare the other planes."""
    from test_gpu_lights import compose
    params, lights = params_of(view), lights_array(positions)
    whole = lit_frame(view, default_light(view))
    out = {}
    for rows in blocks_of(view):
        lit = [whole[rows]["lit"] if tuple(p) == default_light(view) else covered_lit(view, tuple(p))[rows] for p in positions]
        outs = [dict(whole[rows], lit=lit[0])] + [{"lit": l} for l in lit[1:]]
        out[rows] = compose(params, outs, lights)[0]
    return out, lights


def where(view, rows, planes):
    """(x, row, bin column, bin row, z bin) of every pixel of a block, flat as the planes are."""
    W, B = VIEWS[view][0], VIEWS[view][3]
    r0, r1 = rows
    idx = np.arange((r1 - r0) * W)
    x, row = idx % W, r0 + idx // W
    return x, row, x // B, row // B, planes["gbuf"]["z"] // B
