"""What the Python binding hands to the C ABI, without a library and without a GPU: a stand-in in the place of
par.lib() records every call's symbol and arguments, and each wrapper is called with values that cannot be mistaken for
one another (pointers 0x1000, 0x2000, ...; rows (3, 7); G-buffer rows (2, 9); counts that all differ). The expected
argument lists below are written out from the prototypes of include/par_raytracer.h, position by position; they are
not derived from the binding's own signature table (tests/test_abi_cpu.py holds that table to the header).

An argument is recorded as an int (a scalar, or the address a pointer carries), None (NULL) or, for the one
`const void* fill` that travels as bytes, those bytes."""
import ctypes as C

import numpy as np
import pytest

S = 0x5000  # the stream of every call
R = (3, 7)  # rows
G = (2, 9)  # G-buffer / source rows: the halo
ADDR = object()  # "some address": a by-reference output, or an array the wrapper allocates and does not return
_BYREF = type(C.byref(C.c_int()))


def norm(a):
    if a is None or isinstance(a, bytes):
        return a
    if isinstance(a, int):
        return int(a)
    if isinstance(a, _BYREF):
        return C.addressof(a._obj)
    if isinstance(a, (C.c_void_p, C.c_char_p, C.c_int, C.c_uint, C.c_uint64)):
        return a.value
    raise AssertionError(f"an argument of {type(a)} reached the library")


class StandIn:
    """What par.lib() returns during these tests. Every par_* attribute is a function that records (symbol, arguments),
    writes `writes[symbol][position]` through the by-reference argument at that position and returns
    `returns[symbol]`, or `status` for the symbols not named there."""

    def __init__(self, status=0, returns=None, writes=None):
        self.status, self.returns, self.writes = status, returns or {}, writes or {}
        self.calls, self.raw = [], []

    def __getattr__(self, name):
        if not name.startswith("par_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, [norm(a) for a in args]))
            self.raw.append(args)
            for pos, value in self.writes.get(name, {}).items():
                args[pos]._obj.value = value
            return self.returns.get(name, self.status)

        fn.__name__ = name
        return fn


def A(x):
    """The address of a numpy array's first byte or of a ctypes object."""
    return x.ctypes.data if isinstance(x, np.ndarray) else C.addressof(x)


class Env:
    def __init__(self, T):
        self.P = T.default_params(140, 20, bin_size=10)  # 14 x 2 tiles
        self.fb = np.zeros(4 * 140, dtype=T.COLOR)  # rows R
        self.index = np.zeros(4 * 140, dtype=np.uint8)
        self.gbuf = np.zeros(7 * 140, dtype=T.PIXEL)  # rows G
        self.src = np.zeros(7 * 140, dtype=np.uint8)
        self.whole_fb = np.zeros(20 * 140, dtype=T.COLOR)
        self.whole_gbuf = np.zeros(20 * 140, dtype=T.PIXEL)
        self.palette = np.zeros(5, dtype=T.COLOR)
        self.style = T.make_outline_style()
        self.pdesc = T.make_present_desc(2, 3, pitch=1136)  # 16 gap bytes a row
        self.udesc = T.make_upscale_desc(2, pitch=1136)
        self.tiles = np.zeros(8, dtype=np.int32)
        self.aabbs = T.make_aabbs([(1, 2, 3, 4, 5, 6)] * 3)
        self.light = T.make_light(1, 2, 3)
        self.pick = np.zeros(1, dtype=T.PIXEL)
        self.vecs = np.zeros((4, 3), dtype=np.float32)


@pytest.fixture(scope="module")
def env(T):
    return Env(T)


# name -> (wrapper, keyword arguments, symbol, expected arguments, a device-pointer argument or None, returns, writes).
# An expected argument that is a function takes the wrapper's result.
def build_cases(e):
    P, pa = e.P, A(e.P)
    c = {}

    def case(name, kw, symbol, expected, pointer=None, returns=None, writes=None, wrapper=None):
        c[name] = (wrapper or name, kw, symbol, expected, pointer, returns, writes)

    # sharded frames
    case("tiles_assemble", dict(params=P, d_map=0x1000, packed=0x2000, frame=0x3000, rows=R, stream=S),
         "par_tiles_assemble", [pa, S, 0x1000, 0x2000, 0x3000, 3, 7], "d_map")
    case("tiles_pack", dict(params=P, d_tiles=0x1000, n=11, fb_block=0x2000, rows=R, packed=0x3000, stream=S),
         "par_tiles_pack", [pa, S, 0x1000, 11, 0x2000, 3, 7, 0x3000], "fb_block")
    case("tiles_unpack", dict(params=P, d_tiles=0x1000, n=11, packed=0x2000, frame=0x3000, stream=S),
         "par_tiles_unpack", [pa, S, 0x1000, 11, 0x2000, 0x3000], "frame")
    case("background_fill", dict(params=P, rows_ptr=0x1000, n_rows=13, stream=S),
         "par_background_fill", [pa, S, 0x1000, 13], "rows_ptr")
    case("scene_tiles", dict(params=P, aabbs=e.aabbs), "par_scene_tiles", [pa, A(e.aabbs), 3, ADDR, 28],
         returns={"par_scene_tiles": 2})
    case("scene_tile_map", dict(params=P, tiles=e.tiles), "par_scene_tile_map",
         [pa, A(e.tiles), 8, lambda r: A(r), 28])
    # changed tiles
    case("tiles_changed", dict(params=P, a=0x1000, b=0x2000, rows=R, d_map=0x3000, d_tiles=0x4000, capacity=17,
                               d_count=0x6000, stream=S),
         "par_tiles_changed_device", [pa, S, 0x1000, 0x2000, 3, 7, 0x3000, 0x4000, 17, 0x6000], "b")
    case("tiles_pack_counted", dict(params=P, d_tiles=0x1000, d_count=0x2000, capacity=17, fb_block=0x3000, rows=R,
                                    packed=0x4000, stream=S),
         "par_tiles_pack_counted", [pa, S, 0x1000, 0x2000, 17, 0x3000, 3, 7, 0x4000], "d_count")
    case("tiles_fetch", dict(params=P, d_count=0x1000, d_tiles=0x2000, d_packed=0x3000, capacity=17, tiles=e.tiles,
                             packed=0x7000, stream=S),
         "par_tiles_fetch", [pa, S, 0x1000, 0x2000, 0x3000, 17, A(e.tiles), 0x7000, ADDR, ADDR], "d_packed",
         writes={"par_tiles_fetch": {8: 5, 9: 6}})
    case("tiles_apply_host", dict(params=P, tiles=e.tiles, n=8, packed=0x7000, rows=R, frame=e.whole_fb),
         "par_tiles_apply_host", [pa, A(e.tiles), 8, 0x7000, 3, 7, A(e.whole_fb)])
    # plane tiles
    case("plane_tiles_changed", dict(params=P, elem_bytes=28, a=0x1000, b=0x2000, rows=R, d_map=0x3000, d_tiles=0x4000,
                                     capacity=17, d_count=0x6000, stream=S),
         "par_plane_tiles_changed_device", [pa, S, 28, 0x1000, 0x2000, 3, 7, 0x3000, 0x4000, 17, 0x6000], "a")
    case("plane_tiles_pack", dict(params=P, elem_bytes=28, d_tiles=0x1000, n=11, block=0x2000, rows=R, packed=0x3000,
                                  stream=S),
         "par_plane_tiles_pack", [pa, S, 28, 0x1000, 11, 0x2000, 3, 7, 0x3000], "packed")
    case("plane_tiles_pack_counted", dict(params=P, elem_bytes=28, d_tiles=0x1000, d_count=0x2000, capacity=17,
                                          block=0x3000, rows=R, packed=0x4000, stream=S),
         "par_plane_tiles_pack_counted", [pa, S, 28, 0x1000, 0x2000, 17, 0x3000, 3, 7, 0x4000], "block")
    case("plane_tiles_unpack", dict(params=P, elem_bytes=28, d_tiles=0x1000, n=11, packed=0x2000, frame=0x3000,
                                    stream=S),
         "par_plane_tiles_unpack", [pa, S, 28, 0x1000, 11, 0x2000, 0x3000], "d_tiles")
    case("plane_tiles_assemble", dict(params=P, elem_bytes=1, d_map=0x1000, packed=0x2000, fill=b"\xfe", frame=0x3000,
                                      rows=R, stream=S),
         "par_plane_tiles_assemble", [pa, S, 1, 0x1000, 0x2000, b"\xfe", 0x3000, 3, 7], "frame")
    case("plane_tiles_fetch", dict(params=P, elem_bytes=28, d_count=0x1000, d_tiles=0x2000, d_packed=0x3000,
                                   capacity=17, tiles=0x7000, packed=e.whole_gbuf, stream=S),
         "par_plane_tiles_fetch", [pa, S, 28, 0x1000, 0x2000, 0x3000, 17, 0x7000, A(e.whole_gbuf), ADDR, ADDR],
         "d_count", writes={"par_plane_tiles_fetch": {9: 5, 10: 6}})
    case("plane_tiles_apply_host", dict(params=P, elem_bytes=28, tiles=e.tiles, n=8, packed=0x7000, rows=R,
                                        frame=e.whole_gbuf),
         "par_plane_tiles_apply_host", [pa, 28, A(e.tiles), 8, 0x7000, 3, 7, A(e.whole_gbuf)])
    # outlines
    case("outline", dict(params=P, style=e.style, gbuf=0x1000, gbuf_rows=G, fb=0x2000, rows=R, fb_out=0x3000,
                         edge_out=0x4000, stream=S),
         "par_outline_device", [pa, S, A(e.style), 0x1000, 2, 9, 0x2000, 3, 7, 0x3000, 0x4000], "gbuf")
    case("outline_host", dict(params=P, style=e.style, gbuf=e.gbuf, fb=e.fb, rows=R, gbuf_rows=G,
                              planes=("edge", "fb"), device=2),
         "par_outline_host", [pa, 2, A(e.style), A(e.gbuf), 2, 9, A(e.fb), 3, 7, lambda r: A(r["fb"]),
                              lambda r: A(r["edge"])])
    case("outline_host defaults", dict(params=P, style=e.style, gbuf=e.whole_gbuf), "par_outline_host",
         [pa, -1, A(e.style), A(e.whole_gbuf), 0, 20, None, 0, 20, None, lambda r: A(r["edge"])],
         wrapper="outline_host")
    # palette output
    case("quantize", dict(params=P, d_palette=0x1000, n_colors=5, fb=0x2000, rows=R, fb_out=0x3000, index_out=0x4000,
                          spread=19, stream=S),
         "par_quantize_device", [pa, S, 0x1000, 5, 19, 0x2000, 3, 7, 0x3000, 0x4000], "d_palette")
    case("quantize_host", dict(params=P, palette=e.palette, fb=e.fb, rows=R, spread=19, planes=("index", "fb"),
                               device=2),
         "par_quantize_host", [pa, 2, A(e.palette), 5, 19, A(e.fb), 3, 7, lambda r: A(r["fb"]),
                               lambda r: A(r["index"])])
    case("quantize_host defaults", dict(params=P, palette=e.palette, fb=e.whole_fb), "par_quantize_host",
         [pa, -1, A(e.palette), 5, 0, A(e.whole_fb), 0, 20, None, lambda r: A(r["index"])], wrapper="quantize_host")
    case("quantize_pattern", dict(params=P, d_palette=0x1000, n_colors=5, fb=0x2000, rows=R, depth=12, strength=200,
                                  fb_out=0x3000, index_out=0x4000, stream=S),
         "par_quantize_pattern_device", [pa, S, 0x1000, 5, 12, 200, 0x2000, 3, 7, 0x3000, 0x4000], "index_out")
    case("quantize_pattern_host", dict(params=P, palette=e.palette, fb=e.fb, depth=12, strength=200, rows=R,
                                       planes=("fb",), device=2),
         "par_quantize_pattern_host", [pa, 2, A(e.palette), 5, 12, 200, A(e.fb), 3, 7, lambda r: A(r["fb"]), None])
    case("palette_ramp", dict(params=P, levels=8), "par_palette_ramp", [pa, 8, ADDR, 256],
         returns={"par_palette_ramp": 9})
    # fitted and refined palettes
    case("palette_reset", dict(work=0x1000, stream=S), "par_palette_reset_device", [S, 0x1000], "work")
    case("palette_count", dict(params=P, fb=0x1000, rows=R, work=0x2000, stream=S),
         "par_palette_count_device", [pa, S, 0x1000, 3, 7, 0x2000], "fb")
    case("palette_cut", dict(work=0x1000, n_colors=5, stream=S), "par_palette_cut_device", [S, 0x1000, 5], "work")
    case("palette_sum", dict(params=P, fb=0x1000, rows=R, work=0x2000, stream=S),
         "par_palette_sum_device", [pa, S, 0x1000, 3, 7, 0x2000], "work")
    case("palette_emit", dict(work=0x1000, n_colors=5, d_palette=0x2000, stream=S),
         "par_palette_emit_device", [S, 0x1000, 5, 0x2000], "d_palette")
    case("palette_fit_host", dict(params=P, fb=e.fb, n_colors=6, rows=R, device=2),
         "par_palette_fit_host", [pa, 2, A(e.fb), 3, 7, 6, lambda r: A(r[0]), ADDR],
         writes={"par_palette_fit_host": {7: 4}})
    case("palette_refine_device", dict(params=P, fb=0x1000, rows=R, d_palette=0x2000, n_colors=5, iterations=3,
                                       d_index=0x3000, work=0x4000, d_changed=0x6000, stream=S),
         "par_palette_refine_device", [pa, S, 0x1000, 3, 7, 0x2000, 5, 3, 0x3000, 0x4000, 0x6000], "d_index")
    case("palette_refine_host", dict(params=P, fb=e.fb, palette=e.palette, iterations=3, rows=R, device=2),
         "par_palette_refine_host", [pa, 2, A(e.fb), 3, 7, lambda r: A(r[0]), 5, 3, ADDR],
         writes={"par_palette_refine_host": {8: 2}})
    # present, finish, upscale
    case("present", dict(params=P, desc=e.pdesc, out=0x1000, rows=R, fb=0x2000, index=0x3000, d_palette=0x4000,
                         n_colors=5, stream=S),
         "par_present_device", [pa, S, A(e.pdesc), 0x2000, 0x3000, 0x4000, 5, 3, 7, 0x1000], "out")
    case("present_host", dict(params=P, desc=e.pdesc, rows=R, fb=e.fb, index=e.index, palette=e.palette, device=2),
         "par_present_host", [pa, 2, A(e.pdesc), A(e.fb), A(e.index), A(e.palette), 5, 3, 7, lambda r: A(r)])
    case("finish", dict(params=P, desc=e.pdesc, out=0x1000, rows=R, fb=0x2000, style=e.style, gbuf=0x3000, gbuf_rows=G,
                        d_palette=0x4000, n_colors=5, spread=19, index_out=0x6000, stream=S),
         "par_finish_device", [pa, S, A(e.style), 0x3000, 2, 9, 0x4000, 5, 19, A(e.pdesc), 0x2000, 3, 7, 0x1000,
                               0x6000], "fb")
    case("finish defaults", dict(params=P, desc=e.pdesc, out=0x1000, rows=R, fb=0x2000, d_palette=0x4000, n_colors=5),
         "par_finish_device", [pa, None, None, None, 3, 7, 0x4000, 5, 0, A(e.pdesc), 0x2000, 3, 7, 0x1000, None],  # stream 0: NULL
         wrapper="finish")
    case("finish_host", dict(params=P, desc=e.pdesc, fb=e.fb, rows=R, style=e.style, gbuf=e.gbuf, gbuf_rows=G,
                             palette=e.palette, spread=19, want_index=True, device=2),
         "par_finish_host", [pa, 2, A(e.style), A(e.gbuf), 2, 9, A(e.palette), 5, 19, A(e.pdesc), A(e.fb), 3, 7,
                             lambda r: A(r[0]), lambda r: A(r[1])])
    case("finish_host defaults", dict(params=P, desc=e.pdesc, fb=e.whole_fb, palette=e.palette), "par_finish_host",
         [pa, -1, None, None, 0, 20, A(e.palette), 5, 0, A(e.pdesc), A(e.whole_fb), 0, 20, lambda r: A(r), None],
         wrapper="finish_host")
    case("upscale", dict(params=P, desc=e.udesc, out=0x1000, rows=R, fb=0x2000, index=0x3000, d_palette=0x4000,
                         n_colors=5, src_rows=G, index_out=0x6000, stream=S),
         "par_upscale_device", [pa, S, A(e.udesc), 0x2000, 0x3000, 0x4000, 5, 2, 9, 3, 7, 0x1000, 0x6000], "index")
    case("upscale_host", dict(params=P, desc=e.udesc, rows=R, index=e.src, palette=e.palette, src_rows=G,
                              want_index=True, device=2),
         "par_upscale_host", [pa, 2, A(e.udesc), None, A(e.src), A(e.palette), 5, 2, 9, 3, 7, lambda r: A(r[0]),
                              lambda r: A(r[1])])
    case("upscale_host defaults", dict(params=P, desc=e.udesc, fb=e.whole_fb), "par_upscale_host",
         [pa, -1, A(e.udesc), A(e.whole_fb), None, None, 0, 0, 20, 0, 20, lambda r: A(r), None],
         wrapper="upscale_host")
    # host-side helpers
    case("row_block", dict(rank=1, ranks=2, height=320, bin_size=16), "par_row_block", [1, 2, 320, 16, ADDR, ADDR],
         writes={"par_row_block": {4: 160, 5: 320}})
    case("debug_units", dict(kind=2, in_a=e.vecs, device=3), "par_debug_units",
         [3, 2, A(e.vecs), None, 4, lambda r: A(r)])
    case("scene_synthetic", dict(n=4, width=100, height=200, length=300, seed=(1 << 40) + 5), "par_scene_synthetic",
         [4, 100, 200, 300, (1 << 40) + 5, lambda r: A(r[0]), lambda r: A(r[1])])
    case("debug_line", dict(params=P, pick_pixel=e.pick, mouse_x=11, light=e.light, fb=e.whole_fb), "par_debug_line",
         [pa, A(e.pick), 11, A(e.light), A(e.whole_fb)])
    case("tile_floor", dict(), "par_sprite_tile_floor", [lambda r: A(r)])
    case("device_count", dict(), "par_device_count", [], returns={"par_device_count": 3})
    return c


NAMES = [
    "tiles_assemble", "tiles_pack", "tiles_unpack", "background_fill", "scene_tiles", "scene_tile_map", "tiles_changed",
    "tiles_pack_counted", "tiles_fetch", "tiles_apply_host", "plane_tiles_changed", "plane_tiles_pack",
    "plane_tiles_pack_counted", "plane_tiles_unpack", "plane_tiles_assemble", "plane_tiles_fetch",
    "plane_tiles_apply_host", "outline", "outline_host", "outline_host defaults", "quantize", "quantize_host",
    "quantize_host defaults", "quantize_pattern", "quantize_pattern_host", "palette_ramp", "palette_reset",
    "palette_count", "palette_cut", "palette_sum", "palette_emit", "palette_fit_host", "palette_refine_device",
    "palette_refine_host", "present", "present_host", "finish", "finish defaults", "finish_host",
    "finish_host defaults", "upscale", "upscale_host", "upscale_host defaults", "row_block", "debug_units",
    "scene_synthetic", "debug_line", "tile_floor", "device_count"]
NEGATIVE_RETURN = ("par_scene_tiles", "par_palette_ramp")  # a negative return is minus the status
NO_STATUS = ("par_row_block", "par_debug_line", "par_sprite_tile_floor", "par_device_count")  # void, or a count


@pytest.fixture(scope="module")
def cases(env):
    c = build_cases(env)
    assert sorted(c) == sorted(NAMES)
    return c


def put(monkeypatch, par, **kw):
    stand_in = StandIn(**kw)
    monkeypatch.setattr(par, "lib", lambda: stand_in)
    return stand_in


@pytest.mark.parametrize("name", NAMES)
def test_arguments_reach_the_library_in_the_headers_order(par, cases, monkeypatch, name):
    wrapper, kw, symbol, expected, _, returns, writes = cases[name]
    lib = put(monkeypatch, par, returns=returns, writes=writes)
    result = getattr(par, wrapper)(**kw)
    assert [s for s, _ in lib.calls] == [symbol]
    got = lib.calls[0][1]
    assert len(got) == len(expected), got
    for i, (g, want) in enumerate(zip(got, expected)):
        if want is ADDR:
            assert isinstance(g, int) and g != 0, f"{symbol} argument {i}: {g!r} is no address"
            continue
        want = want(result) if callable(want) else want
        assert g == want and type(g) is type(want), f"{symbol} argument {i}: {g!r}, expected {want!r}"


@pytest.mark.parametrize("name", [n for n in NAMES if " " not in n])
def test_a_status_raises_with_that_status_and_the_symbols_name(par, cases, monkeypatch, name):
    wrapper, kw, symbol, _, _, _, writes = cases[name]
    if symbol in NO_STATUS:
        return
    put(monkeypatch, par, status=-6 if symbol in NEGATIVE_RETURN else 6, writes=writes)
    with pytest.raises(par.ParError) as e:
        getattr(par, wrapper)(**kw)
    assert e.value.status == 6
    assert str(e.value) == f"PAR_ERR_EXTENT: {symbol}"


def test_what_the_by_reference_outputs_and_counts_become(par, cases, monkeypatch):
    def run(name):
        wrapper, kw, _, _, _, returns, writes = cases[name]
        put(monkeypatch, par, returns=returns, writes=writes)
        return getattr(par, wrapper)(**kw)

    assert run("tiles_fetch") == (5, 6)
    assert run("plane_tiles_fetch") == (5, 6)
    assert run("row_block") == (160, 320)
    palette, n_entries = run("palette_fit_host")
    assert n_entries == 4 and palette.shape == (6,) and palette.dtype == par.COLOR
    palette, changed = run("palette_refine_host")
    assert changed == 2 and palette.shape == (5,) and palette.dtype == par.COLOR
    assert run("scene_tiles").shape == (2,) and run("scene_tiles").dtype == np.int32
    assert run("palette_ramp").shape == (9,) and run("palette_ramp").dtype == par.COLOR
    assert run("device_count") == 3


def test_what_the_host_forms_return(par, cases, monkeypatch):
    def run(name):
        wrapper, kw = cases[name][:2]
        put(monkeypatch, par)
        return getattr(par, wrapper)(**kw)

    n = 4 * 140
    out = run("outline_host")
    assert list(out) == ["edge", "fb"] and out["edge"].shape == out["fb"].shape == (n,)
    assert out["edge"].dtype == np.uint8 and out["fb"].dtype == par.COLOR
    assert list(run("outline_host defaults")) == ["edge"]
    out = run("quantize_host")
    assert list(out) == ["index", "fb"] and out["index"].shape == out["fb"].shape == (n,)
    assert out["index"].dtype == np.uint8 and out["fb"].dtype == par.COLOR
    assert list(run("quantize_host defaults")) == ["index"] and list(run("quantize_pattern_host")) == ["fb"]
    for name, shape in (("present_host", (4 * 3, 1136)), ("finish_host defaults", (20 * 3, 1136)),
                        ("upscale_host defaults", (20 * 2, 1136))):
        surface = run(name)
        assert surface.shape == shape and surface.dtype == np.uint8 and not surface.any()
    surface, index = run("finish_host")
    assert surface.shape == (4 * 3, 1136) and index.shape == (n,) and index.dtype == np.uint8
    surface, scaled = run("upscale_host")
    assert surface.shape == (4 * 2, 1136) and scaled.shape == (4 * 2, 140 * 2) and scaled.dtype == np.uint8


def test_the_host_forms_refuse_planes_of_another_length(par, env, monkeypatch):
    lib = put(monkeypatch, par)
    P, short = env.P, env.fb[:-1]
    calls = {
        "outline_host": [dict(style=env.style, gbuf=env.gbuf[:-1], rows=R, gbuf_rows=G),
                         dict(style=env.style, gbuf=env.gbuf, fb=short, rows=R, gbuf_rows=G),
                         dict(style=env.style, gbuf=env.gbuf, rows=R, gbuf_rows=G, planes=("edge", "lit"))],
        "quantize_host": [dict(palette=env.palette, fb=short, rows=R),
                          dict(palette=env.palette, fb=env.fb, rows=R, planes=("palidx",))],
        "quantize_pattern_host": [dict(palette=env.palette, fb=short, depth=4, rows=R),
                                  dict(palette=env.palette, fb=env.fb, depth=4, rows=R, planes=("palidx",))],
        "palette_fit_host": [dict(fb=short, n_colors=6, rows=R)],
        "palette_refine_host": [dict(fb=short, palette=env.palette, iterations=3, rows=R)],
        "present_host": [dict(desc=env.pdesc, rows=R, fb=short), dict(desc=env.pdesc, rows=R, index=env.index[:-1])],
        "finish_host": [dict(desc=env.pdesc, fb=short, rows=R),
                        dict(desc=env.pdesc, fb=env.fb, rows=R, style=env.style, gbuf=env.gbuf[:-1], gbuf_rows=G)],
        "upscale_host": [dict(desc=env.udesc, rows=R, src_rows=G, fb=env.fb),  # the source holds src_rows
                         dict(desc=env.udesc, rows=R, src_rows=G, index=env.src[:-1])],
    }
    for wrapper, kws in calls.items():
        for kw in kws:
            with pytest.raises(ValueError, match=wrapper + ": "):
                getattr(par, wrapper)(P, **kw)
    assert lib.calls == []


def test_a_length_error_names_the_wrapper_the_plane_and_both_lengths(par, env, monkeypatch):
    put(monkeypatch, par)
    with pytest.raises(ValueError) as e:
        par.finish_host(env.P, env.pdesc, env.fb, rows=R, style=env.style, gbuf=env.gbuf[:-1], gbuf_rows=G)
    for word in ("finish_host", "gbuf", "979", "980"):
        assert word in str(e.value)


BAD_POINTERS = ("s", 1.5, np.int64(0x1000))


@pytest.mark.parametrize("name", [n for n in NAMES if " " not in n])
def test_device_pointers_are_ints_or_none(par, cases, monkeypatch, name):
    """c_void_p's own conversion of an argument would take a str; the wrappers take an int or None."""
    wrapper, kw, _, _, pointer, _, writes = cases[name]
    if pointer is None:
        return
    lib = put(monkeypatch, par, writes=writes)
    for arg in ("stream", pointer):
        assert isinstance(kw[arg], int)
        for bad in BAD_POINTERS:
            with pytest.raises(TypeError):
                getattr(par, wrapper)(**dict(kw, **{arg: bad}))
        getattr(par, wrapper)(**dict(kw, **{arg: None}))
    assert len(lib.calls) == 2 and all(None in args for _, args in lib.calls)


def test_every_wrapper_with_a_stream_is_among_the_cases(par, cases):
    import inspect
    with_stream = {n for n, f in vars(par).items() if inspect.isfunction(f) and f.__module__ == par.__name__
                   and not n.startswith("_") and "stream" in inspect.signature(f).parameters}
    assert len(with_stream) == 25
    assert with_stream == {c[0] for c in cases.values() if c[4] is not None}


# ---- the renderer's calls ------------------------------------------------------------------------------------------

CTX = 0xC0DE0


def test_the_renderers_calls(par, T, env, monkeypatch):
    lib = put(monkeypatch, par, returns={"par_last_error": b"why"}, writes={"par_create": {2: CTX}})
    P = T.default_params(140, 20, bin_size=10)
    with par.Renderer(P, device=2) as r:
        assert lib.calls.pop() == ("par_create", [A(P), 2, A(r._ctx)])

        def last():
            lib.raw.clear()
            return lib.calls.pop()

        def outputs_of(args, position):
            o = args[position]._obj
            return [getattr(o, k) for k in ("fb", "gbuf", "palidx", "brightness", "lit")]

        for method, symbol in (("render", "par_render_rows"), ("relight", "par_relight_rows")):
            out = getattr(r, method)(planes=("fb", "lit"), rows=R, flags=2)
            raw = lib.raw[-1]
            assert list(out) == ["fb", "lit"] and out["fb"].shape == out["lit"].shape == (4 * 140,)
            assert out["fb"].dtype == par.COLOR and out["lit"].dtype == np.uint8
            assert outputs_of(raw, 3) == [A(out["fb"]), None, None, None, A(out["lit"])]
            assert last() == (symbol, [CTX, 3, 7, C.addressof(raw[3]._obj), 2])
            assert getattr(r, method)()["fb"].shape == (20 * 140,)
            assert last()[1][1:3] == [0, 20]
        ptrs = {"fb": 0x1000, "gbuf": 0x2000, "lit": 0x3000}
        for method, symbol in (("graph_capture", "par_graph_capture"), ("graph_capture_lights", "par_graph_capture_lights"),
                               ("render_device", "par_render_device")):
            getattr(r, method)(ptrs, rows=R, flags=4, stream=S)
            raw = lib.raw[-1]
            assert outputs_of(raw, 4) == [0x1000, 0x2000, None, None, 0x3000]
            assert last() == (symbol, [CTX, S, 3, 7, C.addressof(raw[4]._obj), 4])
            for bad in BAD_POINTERS:
                with pytest.raises(TypeError):
                    getattr(r, method)(ptrs, rows=R, stream=bad)
        stats = r.render_device(ptrs, rows=R, flags=4, stream=S, timed=True)
        raw = lib.raw[-1]
        assert last() == ("par_render_device_timed", [CTX, S, 3, 7, C.addressof(raw[4]._obj), 4, A(stats)])
        r.relight_device(0x2000, {"fb": 0x1000}, rows=R, flags=1, stream=S)
        raw = lib.raw[-1]
        assert outputs_of(raw, 5) == [0x1000, None, None, None, None]
        assert last() == ("par_relight_device", [CTX, S, 3, 7, 0x2000, C.addressof(raw[5]._obj), 1])
        r.update_aabbs(env.aabbs, first=9)
        assert last() == ("par_update_aabbs", [CTX, A(env.aabbs), 9, 3])
        r.update_aabbs(env.aabbs, first=9, stream=S)
        assert last() == ("par_update_aabbs_async", [CTX, A(env.aabbs), 9, 3, S])
        r.graph_stage(env.aabbs, first=9, light=env.light)
        assert last() == ("par_graph_stage", [CTX, A(env.aabbs), 9, 3, A(env.light)])
        lights = np.zeros(2, dtype=T.LIGHT)
        r.graph_stage(env.aabbs, first=9, lights=lights)
        assert last() == ("par_graph_stage_lights", [CTX, A(env.aabbs), 9, 3, A(lights), 2])
        r.graph_launch(stream=S)
        assert last() == ("par_graph_launch", [CTX, S])
        # a context call's failure carries par_last_error, not the symbol
        lib.status = 8
        with pytest.raises(par.ParError) as e:
            r.render(rows=R)
        assert e.value.status == 8 and str(e.value) == "PAR_ERR_NOT_READY: why"
        lib.status = 0
        lib.calls.clear()
    assert lib.calls == [("par_destroy", [CTX])] and not r._ctx.value
