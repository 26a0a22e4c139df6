"""CPU-side checks of relit frames (par_relight_device, par_relight_rows): the header declares both calls and the
binding lists them, both refuse a null context, and the condition on the inputs of tests/test_gpu_relight.py: on the
oracle's frames of its scenes a pixel is covered (palidx != 0xFF) exactly when its G-buffer texel differs from the
background texel, which is how the relight kernel tells the two apart."""
import os
import re

import numpy as np
import pytest

from helpers import graybox, random_stage_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = 1
NTHREADS = min(os.cpu_count() or 8, 16)


def background_texel(T, params):
    """What fill_generic_kernel writes: normal 0, colour {bg, bg, bg, 0}, y, z and entity 0."""
    t = np.zeros(1, dtype=T.PIXEL)
    for ch in ("red", "green", "blue"):
        t["color"][ch] = params.background
    return t


def is_background_texel(T, params, gbuf):
    raw = np.ascontiguousarray(gbuf).view(np.uint8).reshape(-1, T.PIXEL.itemsize)
    return (raw == background_texel(T, params).view(np.uint8).reshape(1, -1)).all(axis=1)


def test_header_declares_and_binding_lists_both_calls(par):
    header = open(os.path.join(ROOT, "include", "par_raytracer.h")).read()
    for name, args in (("par_relight_device", r"par_context\* ctx, void\* stream, int row_begin, int row_end, "
                                              r"const par_pixel\* gbuf,\s+const par_outputs\* device_out, unsigned flags"),
                       ("par_relight_rows", r"par_context\* ctx, int row_begin, int row_end, "
                                            r"const par_outputs\* host_out, unsigned flags")):
        assert re.search(rf"^int {name}\({args}\);", header, flags=re.M), name
        assert name in par.ABI_SYMBOLS
        assert getattr(par.lib(), name) is not None
    for word in ("no graph capture of relit frames", "no timed variant", "no par_render_device_slots counterpart",
                 "the library does not\n * check it"):
        assert word in header, word
    assert callable(par.Renderer.relight) and callable(par.Renderer.relight_device)


def test_null_context_is_an_invalid_argument(par, T):
    L = par.lib()
    px = np.zeros(4, dtype=T.PIXEL)
    fb = np.zeros(4, dtype=T.COLOR)
    o = T.Outputs(fb.ctypes.data, None, None, None, None)
    import ctypes as C
    assert L.par_relight_device(None, None, 0, 1, px.ctypes.data, C.byref(o), 0) == ERR_INVALID_ARG
    assert L.par_relight_rows(None, 0, 1, C.byref(o), 0) == ERR_INVALID_ARG


@pytest.mark.parametrize("name", ["graybox", "random0", "random2", "random5", "random7", "random9"])
def test_covered_pixels_are_the_texels_that_differ_from_the_background(par, oracle, T, name):
    params = T.default_params()
    if name == "graybox":
        aabbs, light = graybox(par), T.make_light(480, 160, 80)
    else:
        aabbs, light = random_stage_scene(int(name[6:]))
    out = oracle.render(params, aabbs, par.tile_floor(), light, nthreads=NTHREADS, planes=("gbuf", "palidx"))
    covered = out["palidx"] != 0xFF
    bg = is_background_texel(T, params, out["gbuf"])
    print(f"{name}: {int(covered.sum())} covered pixels of {covered.size}, {int((covered & bg).sum())} of them with the "
          f"background texel, {int((~covered & ~bg).sum())} background pixels with another texel")
    assert covered.any() and not covered.all()
    assert not (covered & bg).any(), "a covered pixel with the background texel would be relit as background"
    assert bg[~covered].all(), "every background pixel holds the background texel"
    if name == "graybox":
        assert (int(covered.sum()), covered.size) == (150400, 153600)


def test_the_tile_floor_sprite_has_no_zero_normal(par):
    n = par.tile_floor()["normal"].reshape(-1)
    assert ((n["x"] != 0) | (n["y"] != 0) | (n["z"] != 0)).all()
