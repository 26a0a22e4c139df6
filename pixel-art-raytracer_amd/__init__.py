"""pixel-art-raytracer_amd — MI355X-native drop-in for the render call of Cons-Cat/Pixel-Art-Raytracer.

Python plumbing (ctypes) over the C ABI of libpar_raytracer.so (include/par_raytracer.h). The product is the
shared library: hand-written HIP kernels for gfx950 behind an extern-"C" boundary that replaces
src/alternative.cpp:690-760 of the reference. This module only moves pointers around; it computes nothing and has
no CPU rendering path — without the library, or without a gfx950 GPU, rendering fails loudly.

The package directory name carries a hyphen, so import it with
    par = importlib.import_module("pixel-art-raytracer_amd")
"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

from . import types as T
from .abi import ABI, ABI_DEBUG_HOOKS, ABI_HEADERS, install
from .types import (AABB, COLOR, LIGHT, LIGHT_TINT, MAX_SCALE, OUTLINE_STYLE, PIXEL, PRESENT_BGRA, PRESENT_DESC,
                    PRESENT_RGBA, SPRITE, UPSCALE_DESC, UPSCALE_SCALE2X, UPSCALE_SCALE3X, UPSCALE_SCALE4X, FrameStats,
                    Outputs, Params, default_params, make_aabbs, make_light, make_outline_style, make_present_desc,
                    make_tints, make_upscale_desc, ptr)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpar_raytracer.so")

PAR_OK = 0
STATUS_NAMES = {0: "PAR_OK", 1: "PAR_ERR_INVALID_ARG", 2: "PAR_ERR_NO_DEVICE", 3: "PAR_ERR_HIP", 4: "PAR_ERR_OOM",
                5: "PAR_ERR_UNSUPPORTED", 6: "PAR_ERR_EXTENT", 7: "PAR_ERR_SPRITE_ID", 8: "PAR_ERR_NOT_READY", 9: "PAR_ERR_DEVICE"}
RENDER_TRACE_BACKGROUND = 1 << 0
RENDER_COUNT_RAYS = 1 << 1
RENDER_PIPELINED = 1 << 2
RENDER_TIMED_AS_LAUNCHED = 1 << 3
# The planes are the ones this context's last frame was rendered into, same rows, untouched since (par_raytracer.h):
# the frame clears that frame's tiles instead of filling every pixel. Ignored wherever the library's record disagrees.
RENDER_KEPT_OUTPUTS = 1 << 4

ABI_SYMBOLS = tuple(ABI)  # every symbol include/par_raytracer.h declares
MAX_LIGHTS = 8  # PAR_MAX_LIGHTS
LIGHTS_UNBOUNDED, LIGHTS_RANGED = 0, 1  # par_set_light_model


class ParError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {detail}")


_lib = None
_hip = None


def _torch_hip_path():
    """The libamdhip64.so that an installed torch bundles, or None. Does not import torch."""
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return None
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    return cand if os.path.exists(cand) else None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process. PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7)
    and link it by FILE name; our library links the SONAME. If ours is loaded first the dynamic loader brings in
    /opt/rocm's copy and a later `import torch` adds a second runtime that sees no device. Loading torch's copy
    first (when torch is installed and not yet imported) makes both resolve to the same one; with torch already
    imported, or absent, there is nothing to do."""
    if "torch" in sys.modules:
        return
    cand = _torch_hip_path()
    if cand:
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def hip_runtime():
    """The HIP runtime this process holds, for the few runtime calls the plumbing and the tools make themselves: torch's
    own copy where it ships one, else the system's. One handle a process."""
    global _hip
    if _hip is None:
        _hip = C.CDLL(_torch_hip_path() or "libamdhip64.so")
        _hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        _hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        _hip.hipGetDevice.argtypes = [C.c_void_p]
    return _hip


def _load(path, *tables):
    """The library at `path` (built in-tree by __graft_entry__.build() / csrc/Makefile) with `tables` set on its
    functions (none: every table of abi.py). The core lib() and every add-on module's lib() load through here. No
    fallback."""
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `make -C pixel-art-raytracer_amd/csrc` "
                          "(or __graft_entry__.build()). There is no CPU fallback.")
    _share_hip_runtime_with_torch()
    L = C.CDLL(path)
    install(L, *tables)
    return L


def lib():
    """libpar_raytracer.so with every table of abi.py set on its functions, loaded at the first call."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH)
    return _lib


# The call path of the free functions: _ok(lib().par_x, ...), the symbol looked up on lib() at the call and named once.
# (A context's calls go through Renderer._check, whose detail is par_last_error.)

def _ok(fn, *args):
    """Call a library function that returns a status; any but PAR_OK raises ParError with the symbol's name."""
    rc = fn(*args)
    if rc:
        raise ParError(rc, fn.__name__)


def _count(fn, *args):
    """Call a library function that returns a count, or minus the status."""
    n = fn(*args)
    if n < 0:
        raise ParError(-n, fn.__name__)
    return n


# A device pointer or a stream handle, an int or None, for a void* parameter. The wrappers convert it themselves: the
# conversion ctypes applies to a c_void_p argument takes a str or bytes too (and passes its buffer), this constructor
# raises TypeError for anything but an int or None.
_dp = C.c_void_p


def debug_units(kind, in_a, in_b=None, device=0):
    """The reference's arithmetic units as the device kernels compute them (par_debug_units). kind 0: intersect
    (AABB[n], RAY[n]) -> uint8[n]; 1: color scale (float32[n, 5]) -> uint8[n, 4]; 2: normalize (float32[n, 3]) ->
    float32[n, 3]; 3, 4: intersect as the render kernel runs it on a shadow walk's records (floats, packed; 3: hardware
    min / max where the inverse direction is finite, 4: the reference's compare-selects throughout)."""
    a = np.ascontiguousarray(in_a)
    b = None if in_b is None else np.ascontiguousarray(in_b)
    n = len(a)
    out = np.zeros(n, dtype=np.uint8) if kind in (0, 3, 4) else (np.zeros((n, 4), dtype=np.uint8) if kind == 1
                                                         else np.zeros((n, 3), dtype=np.float32))
    _ok(lib().par_debug_units, device, kind, ptr(a), ptr(b), n, ptr(out))
    return out


def row_block(rank, ranks, height, bin_size=40):
    """Rows [begin, end) of `rank` of `ranks` GPUs sharing one frame (par_row_block): cut at bin rows."""
    b, e = C.c_int(0), C.c_int(0)
    lib().par_row_block(rank, ranks, height, bin_size, C.byref(b), C.byref(e))
    return b.value, e.value


def device_count():
    return int(lib().par_device_count())


# ---- host-side scene helpers (C++ in the library; no GPU needed) ------------------------------------------------

def tile_floor():
    """`make_tile_floor` (spr:73-364) as a 1-element SPRITE array."""
    s = np.zeros(1, dtype=SPRITE)
    lib().par_sprite_tile_floor(ptr(s))
    return s


def scene_graybox(view_width=480, view_length=320):
    """The reference's default world, alt:517-599 (162 308 entities at 480 x 320)."""
    n = lib().par_scene_graybox(view_width, view_length, None, 0)
    a = np.zeros(n, dtype=AABB)
    lib().par_scene_graybox(view_width, view_length, ptr(a), n)
    return a


def scene_synthetic(n, width, height, length, seed):
    """SURVEY §8d synthetic scene: (aabbs, light)."""
    a = np.zeros(n, dtype=AABB)
    l = np.zeros(1, dtype=LIGHT)
    _ok(lib().par_scene_synthetic, n, width, height, length, C.c_uint64(seed), ptr(a), ptr(l))
    return a, l


def debug_line(params, pick_pixel, mouse_x, light, fb):
    """alt:763-772 overlay into a host frame (flat COLOR array)."""
    lib().par_debug_line(C.byref(params), ptr(pick_pixel), mouse_x, ptr(light), ptr(fb))


# ---- the renderer ------------------------------------------------------------------------------------------------

_PLANES = ("fb", "gbuf", "palidx", "brightness", "lit")
_PLANE_DTYPE = {"fb": COLOR, "gbuf": PIXEL, "palidx": np.uint8, "brightness": np.float32, "lit": np.uint8}
_PLANE_BYTES = {"fb": 4, "gbuf": 28, "palidx": 1, "brightness": 4, "lit": 1}


class Renderer:
    """One GPU's renderer: the counterpart of the reference's work arrays + render call (alt:503-517, 690-760)."""

    def __init__(self, params=None, device=-1):
        self.params = params or default_params()
        self._ctx = C.c_void_p()
        rc = lib().par_create(C.byref(self.params), device, C.byref(self._ctx))
        if rc != PAR_OK:
            raise ParError(rc, lib().par_status_string(rc).decode())
        self.width, self.height = self.params.width, self.params.height
        self._out_cache = {}

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            lib().par_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != PAR_OK:
            raise ParError(rc, lib().par_last_error(self._ctx).decode())

    # scene surface -----------------------------------------------------------------------------------------
    def set_sprites(self, sprites):
        sprites = np.ascontiguousarray(sprites, dtype=SPRITE)
        self._check(lib().par_set_sprites(self._ctx, ptr(sprites), len(sprites)))

    def set_entities(self, aabbs, sprite_ids=None):
        aabbs = np.ascontiguousarray(aabbs, dtype=AABB)
        ids = None if sprite_ids is None else np.ascontiguousarray(sprite_ids, dtype=np.int32)
        self._check(lib().par_set_entities(self._ctx, ptr(aabbs), ptr(ids), len(aabbs)))

    def set_entities_ref_layout(self, aabbs, sprite_per_entity):
        aabbs = np.ascontiguousarray(aabbs, dtype=AABB)
        sprites = np.ascontiguousarray(sprite_per_entity, dtype=SPRITE)
        assert len(aabbs) == len(sprites)
        self._check(lib().par_set_entities_ref_layout(self._ctx, ptr(aabbs), ptr(sprites), len(aabbs)))

    def update_aabbs(self, aabbs, first=0, stream=None):
        """Overwrite aabbs[first, first+len). With `stream` (the hipStream_t this renderer's frames are enqueued on)
        the copy is ordered on that stream instead of blocking."""
        aabbs = np.ascontiguousarray(aabbs, dtype=AABB)
        if stream is None:
            self._check(lib().par_update_aabbs(self._ctx, ptr(aabbs), first, len(aabbs)))
        else:
            self._check(lib().par_update_aabbs_async(self._ctx, ptr(aabbs), first, len(aabbs), C.c_void_p(stream)))

    def set_light(self, light):
        light = np.ascontiguousarray(light, dtype=LIGHT)
        self._check(lib().par_set_light(self._ctx, ptr(light)))

    def set_lights(self, lights):
        """All lights of the scene (par_set_lights): a LIGHT array of 1 .. MAX_LIGHTS entries. Each covered pixel sums
        the diffuse terms of the lights that reach it; bit l of the `lit` plane says whether light l does."""
        lights = np.ascontiguousarray(lights, dtype=LIGHT)
        self._check(lib().par_set_lights(self._ctx, ptr(lights), len(lights)))

    def set_light_model(self, model):
        """LIGHTS_UNBOUNDED (a new renderer: `radius` is not read) or LIGHTS_RANGED (par_set_light_model): a light with
        radius > 0 reaches the pixels whose L1 distance to it is below the radius and fades out towards it; a radius
        <= 0 leaves a light unbounded. A different model drops captured graphs."""
        self._check(lib().par_set_light_model(self._ctx, int(model)))

    def set_light_tints(self, tints):
        """The lights' colours (par_set_light_tints): a LIGHT_TINT array (types.make_tints) of 1 .. MAX_LIGHTS entries, by
        light index, white for the lights beyond it; a lit light's term is multiplied by its tint channel by channel.
        None makes the renderer untinted again (a new renderer). A change between the two states drops captured graphs;
        new values alone reach a captured graph's next launch."""
        if tints is None:
            self._check(lib().par_set_light_tints(self._ctx, None, 0))
            return
        tints = np.ascontiguousarray(tints, dtype=LIGHT_TINT)
        self._check(lib().par_set_light_tints(self._ctx, ptr(tints), len(tints)))

    def set_scene(self, aabbs, sprites, light, sprite_ids=None):
        self.set_sprites(sprites)
        self.set_entities(aabbs, sprite_ids)
        self.set_light(light)

    # render ------------------------------------------------------------------------------------------------
    def _host_frame(self, symbol, planes, rows, flags):
        """render and relight: rows [r0, r1) from `symbol` into fresh host arrays."""
        r0, r1 = rows or (0, self.height)
        n = (r1 - r0) * self.width
        out = {k: np.zeros(n, dtype=_PLANE_DTYPE[k]) for k in planes}
        o = Outputs(*[out[k].ctypes.data if k in out else None for k in _PLANES])
        self._check(getattr(lib(), symbol)(self._ctx, r0, r1, C.byref(o), flags))
        return out

    def render(self, planes=("fb",), rows=None, flags=0):
        """One frame (or rows [r0, r1)) into fresh host arrays; returns {plane: flat row-major array}."""
        return self._host_frame("par_render_rows", planes, rows, flags)

    def render_device(self, device_ptrs, rows=None, flags=0, stream=0, timed=False):
        """Asynchronous render into device memory. `device_ptrs` maps plane name -> raw device pointer (int) that
        addresses (row_begin, 0). `stream` is a hipStream_t handle (e.g. torch.cuda.current_stream().cuda_stream)."""
        r0, r1 = rows or (0, self.height)
        # (the Outputs struct of a pointer set is cached by the pointer VALUES: this is the per-frame call of a render
        # loop, and a caller may well put a new pointer into the same dict)
        key = tuple(device_ptrs.get(k) for k in _PLANES)
        o = self._out_cache.get(key)
        if o is None:
            if len(self._out_cache) >= 64:
                self._out_cache.clear()
            o = self._out_cache[key] = Outputs(*key)
        if timed:
            st = FrameStats()
            self._check(lib().par_render_device_timed(self._ctx, C.c_void_p(stream), r0, r1, C.byref(o), flags,
                                                      C.byref(st)))
            return st
        self._check(lib().par_render_device(self._ctx, C.c_void_p(stream), r0, r1, C.byref(o), flags))
        return None

    def relight(self, planes=("fb",), rows=None, flags=0):
        """The last render() again under the lights, light model and tints of now (par_relight_rows): no hash build, no
        primary pass. That render must have had a "gbuf" plane (the renderer keeps its device copy) and cover `rows`;
        planes out of "fb", "brightness", "lit". Returns {plane: flat row-major array}."""
        return self._host_frame("par_relight_rows", planes, rows, flags)

    def relight_device(self, gbuf_ptr, device_ptrs, rows=None, flags=0, stream=0):
        """Asynchronous relit frame (par_relight_device): `gbuf_ptr` is the device pointer of the retained frame's gbuf
        plane at (row_begin, 0); `device_ptrs` maps "fb", "brightness", "lit" to device pointers as render_device
        takes them (no "gbuf" or "palidx": they do not depend on lights). Enqueue it on the retained frame's stream."""
        r0, r1 = rows or (0, self.height)
        o = Outputs(*[device_ptrs.get(k) for k in _PLANES])
        self._check(lib().par_relight_device(self._ctx, _dp(stream), r0, r1, _dp(gbuf_ptr), C.byref(o), flags))

    def _capture(self, symbol, device_ptrs, rows, flags, stream):
        r0, r1 = rows or (0, self.height)
        o = Outputs(*[device_ptrs.get(k) for k in _PLANES])
        self._check(getattr(lib(), symbol)(self._ctx, _dp(stream), r0, r1, C.byref(o), flags))

    def graph_capture(self, device_ptrs, rows=None, flags=0, stream=0):
        self._capture("par_graph_capture", device_ptrs, rows, flags, stream)

    def graph_capture_lights(self, device_ptrs, rows=None, flags=0, stream=0):
        """A graph of the light path (par_graph_capture_lights): its launches render whatever lights the context holds
        then, 1 .. MAX_LIGHTS of them."""
        self._capture("par_graph_capture_lights", device_ptrs, rows, flags, stream)

    def graph_stage(self, aabbs=None, first=0, light=None, lights=None):
        """The next graph frame's AABBs [first, first + len(aabbs)), and either lights[0] (`light`, par_graph_stage) or
        the whole light set (`lights`, a LIGHT array: par_graph_stage_lights)."""
        a = None if aabbs is None else np.ascontiguousarray(aabbs, dtype=AABB)
        n = 0 if a is None else len(a)
        if lights is not None:
            if light is not None:
                raise ValueError("graph_stage: pass light or lights, not both")
            ls = np.ascontiguousarray(lights, dtype=LIGHT).reshape(-1)
            self._check(lib().par_graph_stage_lights(self._ctx, ptr(a), first, n, ptr(ls), len(ls)))
            return
        l = None if light is None else np.ascontiguousarray(light, dtype=LIGHT)
        self._check(lib().par_graph_stage(self._ctx, ptr(a), first, n, ptr(l)))

    def graph_launch(self, stream=0):
        self._check(lib().par_graph_launch(self._ctx, C.c_void_p(stream)))

    def pick(self, x, y):
        px = np.zeros(1, dtype=PIXEL)
        self._check(lib().par_pick(self._ctx, x, y, ptr(px)))
        return px

    def stats(self):
        st = FrameStats()
        self._check(lib().par_get_stats(self._ctx, C.byref(st)))
        return st

    def set_test_hooks(self, force_generic=False, two_launch_build=False, record_items=False, lose_build_wg=False,
                       bad_alloc=False, col_roles=0, lights_path=False):
        """Tests only (par_debug_set_hooks, not part of the public header): switches read by the frames enqueued from
        now on. force_generic: every column through the overflow kernel; two_launch_build: the hash build always takes
        two launches; record_items: every column rendered from its record; lose_build_wg: a build workgroup never
        arrives at the one-launch build's barrier (PAR_ERR_DEVICE); bad_alloc: the host-allocating entry points fail
        with PAR_ERR_OOM; col_roles: 1, 2, 4 or 8 wavefronts per column (0: the library's choice); lights_path: a
        one-light frame takes the path of several lights (the light kernel). No arguments: production behaviour."""
        hooks = (int(force_generic) | int(two_launch_build) << 1 | int(record_items) << 2 | int(lose_build_wg) << 3 |
                 int(bad_alloc) << 4 | int(lights_path) << 5)
        self._check(lib().par_debug_set_hooks(self._ctx, hooks, col_roles))

    def light_walks(self):
        """Tests only (par_debug_read_light_walks, not part of the public header): the (start bin, light) pairs the
        ranged light kernel (walked, culled) in the last frame, which must have been rendered with RENDER_COUNT_RAYS
        (else (-1, -1))."""
        out = np.zeros(2, dtype=np.int64)
        self._check(lib().par_debug_read_light_walks(self._ctx, ptr(out)))
        return int(out[0]), int(out[1])

    def read_grid(self):
        """(count, map, bins) of the last frame in the reference's layout (alt:503-509); parity tooling."""
        gx, gy, gz = self.params.grid_dims()
        v = gx * gy * gz
        count = np.zeros(v, dtype=np.int32)
        map_ = np.zeros(v * T.SLOTS, dtype=np.int32)
        bins = np.zeros(v * T.SLOTS, dtype=AABB)
        self._check(lib().par_read_grid(self._ctx, ptr(count), ptr(map_), ptr(bins)))
        return count, map_, bins


def plane_bytes(plane):
    return _PLANE_BYTES[plane]


def scene_tiles(params, aabbs):
    """The screen tiles (bx | by << 16, sorted by bin row then bin column) that can show a primitive of the scene
    (par_scene_tiles: host arithmetic, the same list on every rank of a sharded frame)."""
    a = np.ascontiguousarray(aabbs, dtype=AABB)
    gx, gy, _ = params.grid_dims()
    tiles = np.zeros(gx * gy, dtype=np.int32)
    n = _count(lib().par_scene_tiles, C.byref(params), ptr(a), len(a), ptr(tiles), len(tiles))
    return tiles[:n].copy()


def scene_tile_map(params, tiles):
    """tile column + tile row * grid-x -> index of the tile in `tiles` (its slot in a packed buffer), -1 elsewhere."""
    t = np.ascontiguousarray(tiles, dtype=np.int32)
    gx, gy, _ = params.grid_dims()
    m = np.empty(gx * gy, dtype=np.int32)
    _ok(lib().par_scene_tile_map, C.byref(params), ptr(t), len(t), ptr(m), len(m))
    return m


def tiles_assemble(params, d_map, packed, frame, rows, stream=0):
    """Device pointers (ints): rows [rows[0], rows[1]) of the frame at `frame` (row 0) from the packed tiles the map
    names and the background elsewhere, in one pass (asynchronous)."""
    _ok(lib().par_tiles_assemble, C.byref(params), _dp(stream), _dp(d_map), _dp(packed), _dp(frame), rows[0], rows[1])


def tiles_pack(params, d_tiles, n, fb_block, rows, packed, stream=0):
    """Device pointers (ints): tiles d_tiles[0, n) of the frame block `rows` at fb_block -> packed slots (asynchronous)."""
    _ok(lib().par_tiles_pack, C.byref(params), _dp(stream), _dp(d_tiles), n, _dp(fb_block), rows[0], rows[1],
        _dp(packed))


def tiles_unpack(params, d_tiles, n, packed, frame, stream=0):
    _ok(lib().par_tiles_unpack, C.byref(params), _dp(stream), _dp(d_tiles), n, _dp(packed), _dp(frame))


def background_fill(params, rows_ptr, n_rows, stream=0):
    _ok(lib().par_background_fill, C.byref(params), _dp(stream), _dp(rows_ptr), n_rows)


# ---- changed tiles -----------------------------------------------------------------------------------------------

def tiles_changed(params, a, b, rows, d_map, d_tiles, capacity, d_count, stream=0):
    """Device pointers (ints): the tiles of the frame block `rows` that differ between the planes at `a` and `b`
    (par_tiles_changed_device, asynchronous): ranks or -1 into d_map (grid-x * grid-y entries), the first `capacity`
    tile words into d_tiles, the total into d_count[0]."""
    _ok(lib().par_tiles_changed_device, C.byref(params), _dp(stream), _dp(a), _dp(b), rows[0], rows[1], _dp(d_map),
        _dp(d_tiles), capacity, _dp(d_count))


def tiles_pack_counted(params, d_tiles, d_count, capacity, fb_block, rows, packed, stream=0):
    """Device pointers (ints): tiles_pack with n = min(max(d_count[0], 0), capacity) read on the device (asynchronous)."""
    _ok(lib().par_tiles_pack_counted, C.byref(params), _dp(stream), _dp(d_tiles), _dp(d_count), capacity, _dp(fb_block),
        rows[0], rows[1], _dp(packed))


def tiles_fetch(params, d_count, d_tiles, d_packed, capacity, tiles, packed, stream=0):
    """Waits for `stream`, then copies the count and, when it is within `capacity`, that many tile words and slots from
    the device pointers (ints) into the host arrays `tiles` (int32) and `packed` (COLOR), pageable or pinned
    (par_tiles_fetch). Returns (n, count): n == count when the list is complete, else n == 0 and nothing was copied."""
    n, count = C.c_int(0), C.c_int(0)
    _ok(lib().par_tiles_fetch, C.byref(params), _dp(stream), _dp(d_count), _dp(d_tiles), _dp(d_packed), capacity,
        _host_ptr(tiles), _host_ptr(packed), C.byref(n), C.byref(count))
    return n.value, count.value


def tiles_apply_host(params, tiles, n, packed, rows, frame):
    """Host arrays (or host addresses as ints): slots packed[0, n) of the tiles tiles[0, n) to their place in the whole
    host frame `frame`, on the rows `rows` only (par_tiles_apply_host: host arithmetic, no GPU needed)."""
    _ok(lib().par_tiles_apply_host, C.byref(params), _host_ptr(tiles), n, _host_ptr(packed), rows[0], rows[1],
        _host_ptr(frame))


def _host_ptr(a):
    """A host array, or a host address as an int (pinned staging)."""
    return C.c_void_p(a) if isinstance(a, int) else ptr(a)


# ---- plane tiles: the tile calls with an element size (1: palidx / lit / index / edge, 4: fb / brightness, 28: gbuf) --

def plane_tiles_changed(params, elem_bytes, a, b, rows, d_map, d_tiles, capacity, d_count, stream=0):
    """Device pointers (ints): tiles_changed on planes of `elem_bytes`-byte elements (par_plane_tiles_changed_device,
    asynchronous)."""
    _ok(lib().par_plane_tiles_changed_device, C.byref(params), _dp(stream), elem_bytes, _dp(a), _dp(b), rows[0],
        rows[1], _dp(d_map), _dp(d_tiles), capacity, _dp(d_count))


def plane_tiles_pack(params, elem_bytes, d_tiles, n, block, rows, packed, stream=0):
    """Device pointers (ints): tiles d_tiles[0, n) of the plane block `rows` at `block` -> packed slots of
    bin_size * bin_size * elem_bytes bytes (par_plane_tiles_pack, asynchronous)."""
    _ok(lib().par_plane_tiles_pack, C.byref(params), _dp(stream), elem_bytes, _dp(d_tiles), n, _dp(block), rows[0],
        rows[1], _dp(packed))


def plane_tiles_pack_counted(params, elem_bytes, d_tiles, d_count, capacity, block, rows, packed, stream=0):
    """Device pointers (ints): plane_tiles_pack with n = min(max(d_count[0], 0), capacity) read on the device
    (par_plane_tiles_pack_counted, asynchronous)."""
    _ok(lib().par_plane_tiles_pack_counted, C.byref(params), _dp(stream), elem_bytes, _dp(d_tiles), _dp(d_count),
        capacity, _dp(block), rows[0], rows[1], _dp(packed))


def plane_tiles_unpack(params, elem_bytes, d_tiles, n, packed, frame, stream=0):
    """Device pointers (ints): slots -> their place in the whole plane at `frame` (par_plane_tiles_unpack, asynchronous)."""
    _ok(lib().par_plane_tiles_unpack, C.byref(params), _dp(stream), elem_bytes, _dp(d_tiles), n, _dp(packed),
        _dp(frame))


def plane_tiles_assemble(params, elem_bytes, d_map, packed, fill, frame, rows, stream=0):
    """Device pointers (ints) and `fill`, the `elem_bytes` bytes of the element that goes where the map names no slot:
    rows [rows[0], rows[1]) of the plane at `frame` (row 0) in one pass (par_plane_tiles_assemble, asynchronous)."""
    fill = bytes(fill)
    if len(fill) != elem_bytes:
        raise ParError(1, f"par_plane_tiles_assemble: a fill of {len(fill)} bytes for elements of {elem_bytes}")
    _ok(lib().par_plane_tiles_assemble, C.byref(params), _dp(stream), elem_bytes, _dp(d_map), _dp(packed),
        C.c_char_p(fill), _dp(frame), rows[0], rows[1])


def plane_tiles_fetch(params, elem_bytes, d_count, d_tiles, d_packed, capacity, tiles, packed, stream=0):
    """tiles_fetch with slots of bin_size * bin_size * elem_bytes bytes (par_plane_tiles_fetch): waits for `stream`.
    Returns (n, count): n == count when the list is complete, else n == 0 and nothing was copied."""
    n, count = C.c_int(0), C.c_int(0)
    _ok(lib().par_plane_tiles_fetch, C.byref(params), _dp(stream), elem_bytes, _dp(d_count), _dp(d_tiles),
        _dp(d_packed), capacity, _host_ptr(tiles), _host_ptr(packed), C.byref(n), C.byref(count))
    return n.value, count.value


def plane_tiles_apply_host(params, elem_bytes, tiles, n, packed, rows, frame):
    """Host arrays (or host addresses as ints): tiles_apply_host on a plane of `elem_bytes`-byte elements
    (par_plane_tiles_apply_host: host arithmetic, no GPU needed)."""
    _ok(lib().par_plane_tiles_apply_host, C.byref(params), elem_bytes, _host_ptr(tiles), n, _host_ptr(packed), rows[0],
        rows[1], _host_ptr(frame))


# ---- what the *_host forms of the post passes share: preparing their arrays ---------------------------------------

def _rows(params, rows):
    return rows or (0, params.height)


def _flat(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def _plane(who, name, a, dtype, params, rows):
    """`a` as a flat contiguous `dtype` plane that holds the rows [rows[0], rows[1]) of the frame."""
    a = _flat(a, dtype)
    n = (rows[1] - rows[0]) * params.width
    if len(a) != n:
        raise ValueError(f"{who}: {name} holds {len(a)} elements, rows {rows[0]}..{rows[1]} of width {params.width} "
                         f"hold {n}")
    return a


def _out_planes(who, planes, first, n):
    """The output dict of a pass that writes a uint8 plane called `first` and / or a COLOR plane "fb", n elements each."""
    unknown = set(planes) - {first, "fb"}
    if unknown:
        raise ValueError(f"{who}: unknown planes {sorted(unknown)}")
    out = {}
    if first in planes:
        out[first] = np.zeros(n, dtype=np.uint8)
    if "fb" in planes:
        out["fb"] = np.zeros(n, dtype=COLOR)
    return out


def _palette(palette):
    """(flat COLOR array, its length), or (None, 0)."""
    if palette is None:
        return None, 0
    palette = _flat(palette, COLOR)
    return palette, len(palette)


def _surface(n_rows, scale, pitch):
    """A zeroed surface of n_rows * scale rows, `pitch` bytes each (the library leaves a row's gap bytes alone)."""
    return np.zeros((max(0, n_rows) * max(0, int(scale)), max(0, int(pitch))), dtype=np.uint8)


# ---- outlines ----------------------------------------------------------------------------------------------------

def outline(params, style, gbuf, gbuf_rows, fb, rows, fb_out=None, edge_out=None, stream=0):
    """Device pointers (ints): silhouettes and creases of rows [rows[0], rows[1]) drawn from the G-buffer block at
    `gbuf`, which holds rows [gbuf_rows[0], gbuf_rows[1]) (par_outline_device: the rows beyond `rows` are the halo a row
    block needs to equal the whole frame). `style` is an OUTLINE_STYLE array (types.make_outline_style). The class plane
    (2 silhouette, 1 crease, 0 neither) goes to edge_out and / or the frame block at `fb` with the lines' colours scaled
    to fb_out (fb_out == fb: in place; fb may be None without fb_out). Asynchronous on `stream`: in a frame loop after
    the render or relight call and before quantize."""
    style = np.ascontiguousarray(style, dtype=OUTLINE_STYLE).reshape(-1)
    _ok(lib().par_outline_device, C.byref(params), _dp(stream), ptr(style), _dp(gbuf), gbuf_rows[0], gbuf_rows[1],
        _dp(fb), rows[0], rows[1], _dp(fb_out), _dp(edge_out))


def outline_host(params, style, gbuf, fb=None, rows=None, gbuf_rows=None, planes=("edge",), device=-1):
    """The same on host arrays (par_outline_host): `gbuf` is a PIXEL array holding rows `gbuf_rows` (default: `rows`),
    `fb` a COLOR array holding rows `rows` (default: the whole frame; needed for the "fb" plane only). Returns
    {"edge": uint8 array, "fb": COLOR array} for the planes asked for."""
    r0, r1 = _rows(params, rows)
    g0, g1 = gbuf_rows or (r0, r1)
    style = _flat(style, OUTLINE_STYLE)
    gbuf = _plane("outline_host", "gbuf", gbuf, PIXEL, params, (g0, g1))
    if fb is not None:
        fb = _plane("outline_host", "fb", fb, COLOR, params, (r0, r1))
    out = _out_planes("outline_host", planes, "edge", (r1 - r0) * params.width)
    _ok(lib().par_outline_host, C.byref(params), device, ptr(style), ptr(gbuf), g0, g1, ptr(fb), r0, r1,
        ptr(out.get("fb")), ptr(out.get("edge")))
    return out


# ---- palette output ----------------------------------------------------------------------------------------------

def quantize(params, d_palette, n_colors, fb, rows, fb_out=None, index_out=None, spread=0, stream=0):
    """Device pointers (ints): rows [rows[0], rows[1]) of the frame block at `fb` quantised to the n_colors entries at
    d_palette (par_quantize_device: L1-nearest entry, lowest index among equals, 4x4 ordered dither of strength
    `spread`) into the index plane at index_out and / or the RGBA plane at fb_out (fb_out == fb: in place).
    Asynchronous on `stream`."""
    _ok(lib().par_quantize_device, C.byref(params), _dp(stream), _dp(d_palette), n_colors, spread, _dp(fb), rows[0],
        rows[1], _dp(fb_out), _dp(index_out))


def _quantize_host(who, params, palette, dither, fb, rows, planes, device):
    """quantize_host and quantize_pattern_host: par_<who>, whose prototypes differ in the `dither` arguments alone."""
    r0, r1 = _rows(params, rows)
    palette = _flat(palette, COLOR)
    fb = _plane(who, "fb", fb, COLOR, params, (r0, r1))
    out = _out_planes(who, planes, "index", len(fb))
    _ok(getattr(lib(), "par_" + who), C.byref(params), device, ptr(palette), len(palette), *dither, ptr(fb), r0, r1,
        ptr(out.get("fb")), ptr(out.get("index")))
    return out


def quantize_host(params, palette, fb, rows=None, spread=0, planes=("index",), device=-1):
    """The same on host arrays (par_quantize_host): `palette` and `fb` are COLOR arrays, fb the rows `rows` (default:
    the whole frame). Returns {"index": uint8 array, "fb": COLOR array} for the planes asked for."""
    return _quantize_host("quantize_host", params, palette, (spread,), fb, rows, planes, device)


def quantize_pattern(params, d_palette, n_colors, fb, rows, depth, strength=256, fb_out=None, index_out=None, stream=0):
    """Device pointers (ints): rows [rows[0], rows[1]) of the frame block at `fb` quantised to the n_colors entries at
    d_palette by pattern dithering (par_quantize_pattern_device: `depth` candidates a pixel, 1..16, their error fed back
    at strength / 256, 0..256, the 4x4 Bayer matrix picking one by luma rank) into the index plane at index_out and / or
    the RGBA plane at fb_out (fb_out == fb: in place). Asynchronous on `stream`."""
    _ok(lib().par_quantize_pattern_device, C.byref(params), _dp(stream), _dp(d_palette), n_colors, depth, strength,
        _dp(fb), rows[0], rows[1], _dp(fb_out), _dp(index_out))


def quantize_pattern_host(params, palette, fb, depth, strength=256, rows=None, planes=("index",), device=-1):
    """The same on host arrays (par_quantize_pattern_host): `palette` and `fb` are COLOR arrays, fb the rows `rows`
    (default: the whole frame). Returns {"index": uint8 array, "fb": COLOR array} for the planes asked for."""
    return _quantize_host("quantize_pattern_host", params, palette, (depth, strength), fb, rows, planes, device)


def palette_ramp(params, levels):
    """The natural output palette of a scene (par_palette_ramp): every sprite-palette entry at `levels` brightness bands
    from ambient to full, then the background; a COLOR array of palette_size * levels + 1 entries."""
    out = np.zeros(T.MAX_PALETTE, dtype=COLOR)
    n = _count(lib().par_palette_ramp, C.byref(params), levels, ptr(out), len(out))
    return out[:n].copy()


# ---- fitted palettes ---------------------------------------------------------------------------------------------

def palette_reset(work, stream=0):
    """Device pointer (int) of a par_palette_work block (types.PALETTE_WORK, 8-byte aligned): zeroes it
    (par_palette_reset_device). Asynchronous on `stream`, as all five calls are: reset, count, cut, sum, emit, then
    quantize with the same n_colors, with no host wait between."""
    _ok(lib().par_palette_reset_device, _dp(stream), _dp(work))


def palette_count(params, fb, rows, work, stream=0):
    """Device pointers (ints): adds rows [rows[0], rows[1]) of the frame block at `fb` to the block's 15-bit colour
    histogram (par_palette_count_device). Several frames or row blocks counted in turn give the histogram of all."""
    _ok(lib().par_palette_count_device, C.byref(params), _dp(stream), _dp(fb), rows[0], rows[1], _dp(work))


def palette_cut(work, n_colors, stream=0):
    """Device pointer (int): the median cut of the block's histogram into at most n_colors regions
    (par_palette_cut_device): writes the cell -> entry table and n_entries and zeroes the sums."""
    _ok(lib().par_palette_cut_device, _dp(stream), _dp(work), n_colors)


def palette_sum(params, fb, rows, work, stream=0):
    """Device pointers (ints): adds the channels and the count of every pixel of the rows to the sums of the entry its
    cell maps to (par_palette_sum_device)."""
    _ok(lib().par_palette_sum_device, C.byref(params), _dp(stream), _dp(fb), rows[0], rows[1], _dp(work))


def palette_emit(work, n_colors, d_palette, stream=0):
    """Device pointers (ints): the n_colors palette entries at d_palette from the block's sums, each region's rounded
    mean, padded with copies of entry 0 beyond the entries the cut made (par_palette_emit_device)."""
    _ok(lib().par_palette_emit_device, _dp(stream), _dp(work), n_colors, _dp(d_palette))


def palette_fit_host(params, fb, n_colors, rows=None, device=-1):
    """One frame on host arrays (par_palette_fit_host): `fb` is a COLOR array holding rows `rows` (default: the whole
    frame). Returns (palette, n_entries): a COLOR array of n_colors entries and the number the cut made."""
    r0, r1 = _rows(params, rows)
    fb = _plane("palette_fit_host", "fb", fb, COLOR, params, (r0, r1))
    out = np.zeros(max(0, n_colors), dtype=COLOR)
    n_entries = C.c_int(0)
    _ok(lib().par_palette_fit_host, C.byref(params), device, ptr(fb), r0, r1, n_colors, ptr(out), C.byref(n_entries))
    return out, n_entries.value


def palette_refine_device(params, fb, rows, d_palette, n_colors, iterations, d_index, work, d_changed=None, stream=0):
    """Device pointers (ints): `iterations` k-medians rounds over the n_colors entries at d_palette against rows
    [rows[0], rows[1]) of the frame block at `fb` (par_palette_refine_device): assign as quantize does at spread 0, move
    every entry to the per-channel lower median of its pixels. `d_index` is a byte per pixel of scratch and holds the last
    round's assignment afterwards, `work` a par_palette_refine_work block (types.PALETTE_REFINE_WORK, 8-byte aligned),
    `d_changed` (None or an int32) gets the number of entries the last round changed. After palette_emit, before
    quantize, on the same stream."""
    _ok(lib().par_palette_refine_device, C.byref(params), _dp(stream), _dp(fb), rows[0], rows[1], _dp(d_palette),
        n_colors, iterations, _dp(d_index), _dp(work), _dp(d_changed))


def palette_refine_host(params, fb, palette, iterations, rows=None, device=-1):
    """The same on host arrays (par_palette_refine_host): `fb` is a COLOR array holding rows `rows` (default: the whole
    frame), `palette` a COLOR array, which is not changed. Returns (palette, changed): the refined entries and the number
    of entries the last round changed (0: a fixed point)."""
    r0, r1 = _rows(params, rows)
    fb = _plane("palette_refine_host", "fb", fb, COLOR, params, (r0, r1))
    out = np.array(palette, dtype=COLOR).reshape(-1)
    changed = C.c_int(0)
    _ok(lib().par_palette_refine_host, C.byref(params), device, ptr(fb), r0, r1, ptr(out), len(out), iterations,
        C.byref(changed))
    return out, changed.value


# ---- present -----------------------------------------------------------------------------------------------------

def present(params, desc, out, rows, fb=None, index=None, d_palette=None, n_colors=0, stream=0):
    """Device pointers (ints): rows [rows[0], rows[1]) of the frame block at `fb`, or of the index plane at `index` through
    the n_colors palette entries at d_palette, scaled onto the surface at `out` (par_present_device: nearest neighbour at
    the integer scales, byte order and pitch of `desc`, a PRESENT_DESC array from types.make_present_desc; `out`
    addresses output row rows[0] * scale_y). Asynchronous on `stream`: the last call of a frame loop."""
    desc = np.ascontiguousarray(desc, dtype=PRESENT_DESC).reshape(-1)
    _ok(lib().par_present_device, C.byref(params), _dp(stream), ptr(desc), _dp(fb), _dp(index), _dp(d_palette),
        n_colors, rows[0], rows[1], _dp(out))


def present_host(params, desc, rows=None, fb=None, index=None, palette=None, device=-1):
    """The same on host arrays (par_present_host): `fb` a COLOR array or `index` a uint8 array holding rows `rows`
    (default: the whole frame), `palette` a COLOR array with `index`. Returns the surface's rows as a
    (rows * scale_y, pitch) uint8 array; the bytes of a row beyond 4 * width * scale_x are not written (zeros here)."""
    r0, r1 = _rows(params, rows)
    desc = _flat(desc, PRESENT_DESC)
    if fb is not None:
        fb = _plane("present_host", "fb", fb, COLOR, params, (r0, r1))
    if index is not None:
        index = _plane("present_host", "index", index, np.uint8, params, (r0, r1))
    palette, n_colors = _palette(palette)
    out = _surface(r1 - r0, desc["scale_y"][0], desc["pitch"][0])
    _ok(lib().par_present_host, C.byref(params), device, ptr(desc), ptr(fb), ptr(index), ptr(palette), n_colors, r0, r1,
        ptr(out))
    return out


# ---- finish ------------------------------------------------------------------------------------------------------

def finish(params, desc, out, rows, fb, style=None, gbuf=None, gbuf_rows=None, d_palette=None, n_colors=0, spread=0,
           index_out=None, stream=0):
    """Device pointers (ints): outline, quantize and present in one launch (par_finish_device). Rows [rows[0], rows[1]) of
    the frame block at `fb` are outlined from the G-buffer block at `gbuf` (rows `gbuf_rows`, default `rows`) when `style`
    (an OUTLINE_STYLE array) is given, quantised to the n_colors entries at d_palette with dither `spread` when d_palette
    is given (the index plane to index_out when asked for), and scaled onto the surface at `out` as `desc` (a PRESENT_DESC
    array) says. At least one of style and d_palette. Asynchronous on `stream`: the call after render or relight."""
    desc = np.ascontiguousarray(desc, dtype=PRESENT_DESC).reshape(-1)
    if style is not None:
        style = np.ascontiguousarray(style, dtype=OUTLINE_STYLE).reshape(-1)
    g0, g1 = gbuf_rows or rows
    _ok(lib().par_finish_device, C.byref(params), _dp(stream), ptr(style), _dp(gbuf), g0, g1, _dp(d_palette), n_colors,
        spread, ptr(desc), _dp(fb), rows[0], rows[1], _dp(out), _dp(index_out))


def finish_host(params, desc, fb, rows=None, style=None, gbuf=None, gbuf_rows=None, palette=None, spread=0,
                want_index=False, device=-1):
    """The same on host arrays (par_finish_host): `fb` a COLOR array holding rows `rows` (default: the whole frame), `gbuf`
    a PIXEL array holding rows `gbuf_rows` (default: `rows`) with `style`, `palette` a COLOR array. Returns the surface's
    rows as a (rows * scale_y, pitch) uint8 array as present_host does (zeros in the gap bytes), or (surface, index plane)
    with want_index."""
    r0, r1 = _rows(params, rows)
    g0, g1 = gbuf_rows or (r0, r1)
    desc = _flat(desc, PRESENT_DESC)
    fb = _plane("finish_host", "fb", fb, COLOR, params, (r0, r1))
    if style is not None:
        style = _flat(style, OUTLINE_STYLE)
    if gbuf is not None:
        gbuf = _plane("finish_host", "gbuf", gbuf, PIXEL, params, (g0, g1))
    palette, n_colors = _palette(palette)
    out = _surface(r1 - r0, desc["scale_y"][0], desc["pitch"][0])
    index = np.zeros(len(fb), dtype=np.uint8) if want_index else None
    _ok(lib().par_finish_host, C.byref(params), device, ptr(style), ptr(gbuf), g0, g1, ptr(palette), n_colors, spread,
        ptr(desc), ptr(fb), r0, r1, ptr(out), ptr(index))
    return (out, index) if want_index else out


# ---- upscale -----------------------------------------------------------------------------------------------------

def upscale(params, desc, out, rows, fb=None, index=None, d_palette=None, n_colors=0, src_rows=None, index_out=None,
            stream=0):
    """Device pointers (ints): rows [rows[0], rows[1]) of the frame block at `fb`, or of the index plane at `index`,
    through the pixel-art scaler of `desc` (par_upscale_device: Scale2x, Scale3x or Scale4x; an UPSCALE_DESC array from
    types.make_upscale_desc) onto the surface at `out` (None: no surface; an index source then needs no palette), the
    raw scaled index plane to index_out when given. The source holds rows `src_rows` (default: `rows`): the halo of a row
    block. `out` and `index_out` address output row rows[0] * scaler. Asynchronous on `stream`."""
    desc = np.ascontiguousarray(desc, dtype=UPSCALE_DESC).reshape(-1)
    s0, s1 = src_rows or rows
    _ok(lib().par_upscale_device, C.byref(params), _dp(stream), ptr(desc), _dp(fb), _dp(index), _dp(d_palette),
        n_colors, s0, s1, rows[0], rows[1], _dp(out), _dp(index_out))


def upscale_host(params, desc, rows=None, fb=None, index=None, palette=None, src_rows=None, want_index=False,
                 device=-1):
    """The same on host arrays (par_upscale_host): `fb` a COLOR array or `index` a uint8 array holding rows `src_rows`
    (default: `rows`, which defaults to the whole frame), `palette` a COLOR array with `index` (None with `index`: no
    surface, which needs want_index). Returns the surface's rows as a (rows * scaler, pitch) uint8 array as present_host
    does (zeros in the gap bytes), or (surface or None, the (rows * scaler, width * scaler) index plane) with
    want_index."""
    r0, r1 = _rows(params, rows)
    s0, s1 = src_rows or (r0, r1)
    desc = _flat(desc, UPSCALE_DESC)
    if fb is not None:
        fb = _plane("upscale_host", "fb", fb, COLOR, params, (s0, s1))
    if index is not None:
        index = _plane("upscale_host", "index", index, np.uint8, params, (s0, s1))
    palette, n_colors = _palette(palette)
    k = max(0, int(desc["scaler"][0]))
    out = None
    if fb is not None or palette is not None or not want_index:
        out = _surface(r1 - r0, k, desc["pitch"][0])
    scaled = _surface(r1 - r0, k, max(0, params.width) * k) if want_index else None
    _ok(lib().par_upscale_host, C.byref(params), device, ptr(desc), ptr(fb), ptr(index), ptr(palette), n_colors, s0, s1,
        r0, r1, ptr(out), ptr(scaled))
    return (out, scaled) if want_index else out
