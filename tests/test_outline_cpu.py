"""Outlines without a GPU: the two calls are declared, exported and bound; every PAR_ERR_INVALID_ARG of both comes back
before any device work and with nothing written; the vectorised model the GPU tests lean on (outline.model) equals a
per-pixel loop on random texel planes and on an oracle G-buffer; and the halo statement of the contract holds on that
frame: a row block with one more G-buffer row on each side equals the whole frame's rows, one without does not."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import headers
import outline as O
from helpers import random_stage_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = 1

DECLARATIONS = {
    "par_outline_device": "const par_params* params, void* stream, const par_outline_style* style, "
                          "const par_pixel* gbuf, int gbuf_row_begin, int gbuf_row_end, "
                          "const par_color* fb, int row_begin, int row_end, par_color* fb_out, uint8_t* edge_out",
    "par_outline_host": "const par_params* params, int device, const par_outline_style* style, "
                        "const par_pixel* gbuf, int gbuf_row_begin, int gbuf_row_end, "
                        "const par_color* fb, int row_begin, int row_end, par_color* fb_out, uint8_t* edge_out",
}


def test_declared_exported_and_bound(par, T):
    headers.assert_declared(par, "par_raytracer.h", DECLARATIONS, ("outline", "outline_host"))
    types = open(os.path.join(ROOT, "include", "par_types.h")).read()
    m = re.search(r"typedef struct par_outline_style \{([^}]*)\} par_outline_style;", types)
    assert m and re.findall(r"int32_t\s+(\w+);", m.group(1)) == ["depth_step", "silhouette_scale", "crease_scale"]
    assert T.OUTLINE_STYLE.names == ("depth_step", "silhouette_scale", "crease_scale") and T.OUTLINE_STYLE.itemsize == 12
    s = T.make_outline_style(3, 100, 400)
    assert s.dtype == T.OUTLINE_STYLE and s.view(np.int32).tolist() == [3, 100, 400]


# ---- argument errors: no device needed, nothing written -----------------------------------------------------------

BAD_CALLS = [
    # (tag, overrides) — one case per condition of the contract; the good call's arguments are the defaults:
    # an 8 x 6 frame, G-buffer rows (1, 5), rows (2, 4)
    ("null params", dict(params=None)),
    ("null style", dict(style=None)),
    ("null gbuf", dict(gbuf=None)),
    ("both outputs null", dict(fb_out=None, edge_out=None)),
    ("fb_out without fb", dict(fb=None)),
    ("width 0", dict(width=0)),
    ("width negative", dict(width=-8)),
    ("depth_step 0", dict(style_values=(0, 128, 320))),
    ("depth_step negative", dict(style_values=(-4, 128, 320))),
    ("silhouette_scale -1", dict(style_values=(4, -1, 320))),
    ("silhouette_scale 1025", dict(style_values=(4, 1025, 320))),
    ("crease_scale -1", dict(style_values=(4, 128, -1))),
    ("crease_scale 1025", dict(style_values=(4, 128, 1025))),
    ("g0 negative", dict(grows=(-1, 5))),
    ("g0 > r0", dict(grows=(3, 5))),
    ("r0 == r1", dict(rows=(3, 3))),
    ("r0 > r1", dict(rows=(4, 2))),
    ("r1 > g1", dict(grows=(1, 3))),
    ("g1 > height", dict(grows=(1, 7), rows=(2, 7))),
    ("rows outside the G-buffer rows on both sides", dict(grows=(2, 4), rows=(1, 5))),
]


@pytest.mark.parametrize("call", ["device", "host"])
def test_invalid_arguments_need_no_device_and_write_nothing(par, T, call):
    L = par.lib()
    fn = L.par_outline_device if call == "device" else L.par_outline_host
    first = C.c_void_p(0) if call == "device" else -1  # the stream / the device

    def status(arg):
        p = None if arg["params"] is None else C.byref(arg["params"])
        return fn(p, first, T.ptr(arg["style"]), T.ptr(arg["gbuf"]), arg["grows"][0], arg["grows"][1], T.ptr(arg["fb"]),
                  arg["rows"][0], arg["rows"][1], T.ptr(arg["fb_out"]), T.ptr(arg["edge_out"]))

    for tag, over in BAD_CALLS:
        params = T.default_params(8, 6)
        params.width = over.get("width", 8)
        gbuf = np.full(8 * 6 * 28, 0x5A, dtype=np.uint8).view(T.PIXEL)  # host dummies: never dereferenced
        fb = np.full(8 * 6 * 4, 0xA5, dtype=np.uint8).view(T.COLOR)
        fb_out = np.full(8 * 6 * 4, 0xC3, dtype=np.uint8).view(T.COLOR)
        edge_out = np.full(8 * 6, 0x3C, dtype=np.uint8)
        style = T.make_outline_style(*over.get("style_values", (4, 128, 320)))
        arg = dict(params=params, style=style, gbuf=gbuf, fb=fb, fb_out=fb_out, edge_out=edge_out, grows=(1, 5), rows=(2, 4))
        arg.update({k: v for k, v in over.items() if k not in ("width", "style_values")})
        rc = status(arg)
        assert rc == ERR_INVALID_ARG, f"{call}: {tag}: status {rc}"
        assert (gbuf.view(np.uint8) == 0x5A).all() and (fb.view(np.uint8) == 0xA5).all() and \
            (fb_out.view(np.uint8) == 0xC3).all() and (edge_out == 0x3C).all(), f"{call}: {tag}: something was written"


def test_binding_raises_invalid_arg(par, T):
    params = T.default_params(8, 6)
    style = T.make_outline_style()
    with pytest.raises(par.ParError) as e:
        par.outline(params, style, 0, (0, 6), None, (0, 6), edge_out=0)  # null gbuf
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(par.ParError) as e:
        par.outline_host(params, T.make_outline_style(0), np.zeros(48, dtype=T.PIXEL))
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(par.ParError) as e:
        par.outline_host(params, style, np.zeros(48, dtype=T.PIXEL), planes=("fb",))  # fb_out without fb
    assert e.value.status == ERR_INVALID_ARG


# ---- the model the GPU tests compare with --------------------------------------------------------------------------

@pytest.mark.parametrize("grows,rows", [((0, 7), (0, 7)), ((1, 6), (2, 5)), ((2, 5), (2, 5)), ((0, 4), (3, 4))])
@pytest.mark.parametrize("step", [1, 3])
def test_model_equals_the_per_pixel_loop_on_random_texels(T, step, grows, rows):
    rng = np.random.default_rng(21)
    params = T.default_params(9, 7)
    gbuf = O.random_texels(T, rng, params, (grows[1] - grows[0]) * 9)
    fb = O.random_colors(T, rng, (rows[1] - rows[0]) * 9)
    style = T.make_outline_style(step, 128, 320)
    edge, out = O.model(params, style, gbuf, grows, fb, rows)
    edge_l, out_l = O.model_loop(params, style, gbuf, grows, fb, rows)
    assert edge.tobytes() == edge_l.tobytes() and out.tobytes() == out_l.tobytes()
    assert np.array_equal(out["alpha"], fb["alpha"])
    if rows == (0, 7):
        assert all((edge == c).sum() > 0 for c in (0, 1, 2)), f"the inputs should reach every class: {np.bincount(edge)}"
        assert (out.view(np.uint32) != fb.view(np.uint32)).any()
    only_edge, nothing = O.model(params, style, gbuf, grows, None, rows)
    assert nothing is None and only_edge.tobytes() == edge.tobytes()


def test_model_equals_the_per_pixel_loop_on_arbitrary_bits(T):
    rng = np.random.default_rng(22)
    params = T.default_params(11, 5)
    gbuf = rng.integers(0, 256, 11 * 5 * 28, dtype=np.uint8).view(T.PIXEL)
    fb = O.random_colors(T, rng, 11 * 5)
    for style in ((1, 0, 1024), (1 << 30, 255, 257)):
        a, b = O.model(params, style, gbuf, (0, 5), fb, (0, 5)), O.model_loop(params, style, gbuf, (0, 5), fb, (0, 5))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.fixture(scope="module")
def oracle_gbuf(oracle, T):
    """The G-buffer of helpers.random_stage_scene(3) at 480 x 320, from the oracle's hash build and primary pass."""
    params = T.default_params(480, 320)
    aabbs, _ = random_stage_scene(3)
    gbuf, _ = oracle.primary(params, oracle.bin(params, aabbs), oracle.tile_floor())
    return params, gbuf


def test_model_equals_the_per_pixel_loop_on_an_oracle_gbuffer(T, oracle_gbuf):
    params, gbuf = oracle_gbuf
    W = params.width
    style = T.make_outline_style(4, 128, 320)
    whole, _ = O.model(params, style, gbuf, (0, 320), None, (0, 320))
    # the loop on 60 rows of it (one Python iteration per pixel and neighbour): rows and halo as a sharded caller's
    rows = (100, 160)
    grows = O.halo(rows, 320)
    fb = O.random_colors(T, np.random.default_rng(23), 60 * W)
    edge, out = O.model(params, style, O.block(gbuf, W, grows), grows, fb, rows)
    edge_l, out_l = O.model_loop(params, style, O.block(gbuf, W, grows), grows, fb, rows)
    assert edge.tobytes() == edge_l.tobytes() == O.block(whole, W, rows).tobytes() and out.tobytes() == out_l.tobytes()
    assert all((edge == c).sum() > 0 for c in (0, 1, 2))


def test_halo_rows_make_a_row_block_equal_the_whole_frame(T, oracle_gbuf):
    """The halo statement on the oracle frame, depth_step 4, row block [106, 213). The model counts 71 529 covered, 18 186
    silhouette and 1 435 crease pixels, and the unhaloed block differs at 12 pixels (printed, not asserted: only that each
    is above zero). A model without the contract's clause "the neighbour does not meet the silhouette condition against
    T" would count 2 020 creases and 15 differing pixels."""
    params, gbuf = oracle_gbuf
    W, H = params.width, params.height
    style = T.make_outline_style(4, 128, 320)
    whole = O.classes(params, style, gbuf, (0, H), (0, H))
    n_covered, n_sil, n_crease = int(O.covered(params, gbuf).sum()), int((whole == 2).sum()), int((whole == 1).sum())
    rows = (106, 213)
    assert O.halo(rows, H) == (105, 214)
    with_halo = O.classes(params, style, O.block(gbuf, W, (105, 214)), (105, 214), rows)
    without = O.classes(params, style, O.block(gbuf, W, rows), rows, rows)
    n_differ = int((without != O.block(whole, W, rows)).sum())
    print(f"covered {n_covered}, silhouette {n_sil}, crease {n_crease}, the unhaloed block differs at {n_differ} pixels")
    assert n_covered > 0 and n_sil > 0 and n_crease > 0 and n_differ > 0
    assert with_halo.tobytes() == O.block(whole, W, rows).tobytes()
    # one halo row alone mends its side only
    for grows in ((105, 213), (106, 214)):
        one = O.classes(params, style, O.block(gbuf, W, grows), grows, rows)
        assert 0 < int((one != O.block(whole, W, rows)).sum()) < n_differ
