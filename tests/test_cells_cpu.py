"""Colour cells without a GPU: the three calls are declared in include/par_cells.h (and nowhere in par_raytracer.h),
exported and wrapped by the cells module (tests/test_abi_cpu.py holds the binding's table to the header's prototypes and
compiles the header as pedantic C11); every PAR_ERR_INVALID_ARG of both forms comes back before any
device work and with nothing written, each rule on its own; the vectorised model the GPU tests lean on (cells.model)
equals a per-cell, per-pixel, per-entry loop on random frames, on frames drawn near sub-palettes and on crafted cells
whose planes are worked out by hand; the consequences the contract states hold; and par_cells_pairs is
itertools.combinations."""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

import cells as CM
import headers
import quantize as Q

ERR_INVALID_ARG = 1
HEADER = "par_cells.h"
SYMBOLS = ("par_quantize_cells_device", "par_quantize_cells_host", "par_cells_pairs")


@pytest.fixture(scope="module")
def cells(par):
    return importlib.import_module("pixel-art-raytracer_amd.cells")


# ---- declared, exported, bound -------------------------------------------------------------------------------------

def test_declared_exported_and_bound(par, cells):
    assert [(ret, name) for ret, name, _ in headers.prototypes(HEADER)] == [("int", name) for name in SYMBOLS]
    assert SYMBOLS == tuple(cells.ABI_CELLS) == cells.ABI_CELLS_SYMBOLS and cells.ABI_CELLS is par.ABI_HEADERS[HEADER]
    main = headers.text("par_raytracer.h")
    assert "par_cells" not in main and "par_quantize_cells" not in main
    headers.assert_apart(par, HEADER, cells, ("quantize_cells", "quantize_cells_host", "cells_pairs"))


def test_the_prototypes_are_the_contracts():
    header = " ".join(headers.without_comments(HEADER).split())
    for proto in (
            "int par_quantize_cells_device(const par_params* params, void* stream, const par_color* d_palette, int n_sub, "
            "int sub_size, int cell_w, int cell_h, int spread, const par_color* fb, int row_begin, int row_end, "
            "par_color* fb_out, uint8_t* index_out, uint8_t* cell_out);",
            "int par_quantize_cells_host(const par_params* params, int device, const par_color* palette, int n_sub, "
            "int sub_size, int cell_w, int cell_h, int spread, const par_color* fb, int row_begin, int row_end, "
            "par_color* fb_out, uint8_t* index_out, uint8_t* cell_out);",
            "int par_cells_pairs(const par_color* palette, int n_colors, par_color* out, int capacity);"):
        assert proto in header, proto


# ---- argument errors: no device needed, nothing written -----------------------------------------------------------

W, H = 8, 40
BAD = [
    ("null params", dict(params=None)),
    ("null palette", dict(palette=None)),
    ("null fb", dict(fb=None)),
    ("both outputs null", dict(fb_out=None, index_out=None)),
    ("all three outputs null", dict(fb_out=None, index_out=None, cell_out=None)),
    ("n_sub 0", dict(n_sub=0)),
    ("n_sub negative", dict(n_sub=-1)),
    ("sub_size 0", dict(sub_size=0)),
    ("sub_size negative", dict(sub_size=-4)),
    ("both negative", dict(n_sub=-4, sub_size=-4)),
    ("S * K = 257", dict(n_sub=257, sub_size=1)),
    ("S * K = 260", dict(n_sub=65, sub_size=4)),
    ("S * K wraps an int", dict(n_sub=1 << 16, sub_size=1 << 16)),
    ("cell_w 4", dict(cell=(4, 8))),
    ("cell_w 12", dict(cell=(12, 8))),
    ("cell_w 32", dict(cell=(32, 8))),
    ("cell_w 0", dict(cell=(0, 8))),
    ("cell_h 4", dict(cell=(8, 4))),
    ("cell_h 32", dict(cell=(8, 32))),
    ("cell_h 0", dict(cell=(8, 0))),
    ("cell_h negative", dict(cell=(8, -8))),
    ("spread -1", dict(spread=-1)),
    ("spread 256", dict(spread=256)),
    ("width 0", dict(width=0)),
    ("width negative", dict(width=-8)),
    ("row_begin negative", dict(rows=(-8, 8))),
    ("row_begin == row_end", dict(rows=(8, 8))),
    ("row_begin > row_end", dict(rows=(16, 8))),
    ("row_end > height", dict(rows=(0, 48))),
    ("cell_h 8: row_begin inside a cell", dict(rows=(4, 16))),
    ("cell_h 8: row_end inside a cell", dict(rows=(8, 12))),
    ("cell_h 16: row_begin inside a cell", dict(rows=(8, 32), cell=(8, 16))),
    ("cell_h 16: row_end inside a cell", dict(rows=(16, 24), cell=(8, 16))),
    ("cell_h 16: row_end inside the last cell", dict(rows=(32, 36), cell=(16, 16), height=37)),
    ("cell_h 8: row_end inside the last cell", dict(rows=(32, 36), height=37)),
]


def raw_call(par, T, call, over, fill=True):
    """One call of the raw symbol on host dummies: (status, whether any buffer changed)."""
    L = importlib.import_module("pixel-art-raytracer_amd.cells").lib()
    params = T.default_params(W, over.get("height", H))
    params.width = over.get("width", W)
    n = W * params.height
    palette = np.full(256 * 4, 0x5A, dtype=np.uint8).view(T.COLOR)
    fb = np.full(n * 4, 0xA5, dtype=np.uint8).view(T.COLOR)
    fb_out = np.full(n * 4, 0xC3, dtype=np.uint8).view(T.COLOR)
    index_out = np.full(n, 0x3C, dtype=np.uint8)
    cell_out = np.full(n, 0x69, dtype=np.uint8)
    arg = dict(params=params, palette=palette, fb=fb, fb_out=fb_out, index_out=index_out, cell_out=cell_out, n_sub=4,
               sub_size=4, cell=(8, 8), spread=0, rows=(0, params.height))
    arg.update({k: v for k, v in over.items() if k not in ("width", "height")})
    p = None if arg["params"] is None else C.byref(arg["params"])
    first = C.c_void_p(0) if call == "device" else -1  # the stream / the device
    fn = L.par_quantize_cells_device if call == "device" else L.par_quantize_cells_host
    rc = fn(p, first, T.ptr(arg["palette"]), arg["n_sub"], arg["sub_size"], arg["cell"][0], arg["cell"][1], arg["spread"],
            T.ptr(arg["fb"]), arg["rows"][0], arg["rows"][1], T.ptr(arg["fb_out"]), T.ptr(arg["index_out"]),
            T.ptr(arg["cell_out"]))
    same = (fb.view(np.uint8) == 0xA5).all() and (fb_out.view(np.uint8) == 0xC3).all() and (index_out == 0x3C).all() and \
        (cell_out == 0x69).all() and (palette.view(np.uint8) == 0x5A).all()
    return rc, not same


@pytest.mark.parametrize("call", ["device", "host"])
def test_invalid_arguments_need_no_device_and_write_nothing(par, T, call):
    assert len({tag for tag, _ in BAD}) == len(BAD)
    for tag, over in BAD:
        rc, changed = raw_call(par, T, call, over)
        assert rc == ERR_INVALID_ARG, f"{call}: {tag}: status {rc}"
        assert not changed, f"{call}: {tag}: something was written"


def test_the_row_cuts_the_rule_admits_are_not_refused(par, T):
    """The host form on the cuts next to the refused ones (the device form would take host dummies for device memory):
    any status but PAR_ERR_INVALID_ARG, which without a GPU is PAR_ERR_NO_DEVICE."""
    for over in (dict(rows=(8, 16)), dict(rows=(16, 32), cell=(8, 16)), dict(rows=(32, 37), cell=(16, 16), height=37),
                 dict(rows=(32, 37), height=37), dict(rows=(0, 37), cell=(8, 16), height=37),
                 dict(n_sub=256, sub_size=1), dict(n_sub=1, sub_size=256), dict(spread=255), dict(cell_out=None),
                 dict(fb_out=None), dict(index_out=None)):
        rc, _ = raw_call(par, T, "host", over)
        assert rc in (0, 2), (over, rc)
        assert rc == (0 if par.device_count() > 0 else 2), (over, rc)


def test_binding_raises_invalid_arg(par, T, cells):
    params = T.default_params(8, 16)
    with pytest.raises(par.ParError) as e:
        cells.quantize_cells(params, 0, 4, 4, (8, 8), 0, (0, 16), index_out=0)
    assert e.value.status == ERR_INVALID_ARG and str(e.value) == "PAR_ERR_INVALID_ARG: par_quantize_cells_device"
    pal, fb = np.zeros(16, dtype=T.COLOR), np.zeros(8 * 16, dtype=T.COLOR)
    with pytest.raises(par.ParError) as e:
        cells.quantize_cells_host(params, pal, 4, 4, (8, 12), fb)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(par.ParError) as e:
        cells.quantize_cells_host(params, pal, 4, 4, (8, 16), fb[:64], rows=(8, 16))
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(ValueError, match="quantize_cells_host: "):
        cells.quantize_cells_host(params, pal, 4, 4, (8, 8), fb[:-1])
    with pytest.raises(ValueError, match="quantize_cells_host: "):
        cells.quantize_cells_host(params, pal, 4, 3, (8, 8), fb)
    with pytest.raises(ValueError, match="quantize_cells_host: "):
        cells.quantize_cells_host(params, pal, 4, 4, (8, 8), fb, planes=("palidx",))
    for bad in ("s", 1.5, np.int64(0x1000)):
        with pytest.raises(TypeError):
            cells.quantize_cells(params, bad, 4, 4, (8, 8), 0x1000, (0, 16), index_out=0x2000)
        with pytest.raises(TypeError):
            cells.quantize_cells(params, 0x1000, 4, 4, (8, 8), 0x2000, (0, 16), index_out=0x3000, stream=bad)


def test_arguments_reach_the_library_in_the_headers_order(par, T, cells, monkeypatch):
    from test_binding_cpu import A, StandIn
    stand_in = StandIn()
    monkeypatch.setattr(par, "lib", lambda: stand_in)
    P = T.default_params(140, 40)
    cells.quantize_cells(P, 0x1000, 5, 3, (8, 16), 0x2000, (16, 32), fb_out=0x3000, index_out=0x4000, cell_out=0x6000,
                         spread=19, stream=0x5000)
    assert stand_in.calls.pop() == ("par_quantize_cells_device", [A(P), 0x5000, 0x1000, 5, 3, 8, 16, 19, 0x2000, 16, 32,
                                                                  0x3000, 0x4000, 0x6000])
    cells.quantize_cells(P, 0x1000, 5, 3, (16, 8), 0x2000, (16, 32), index_out=0x4000)
    assert stand_in.calls.pop() == ("par_quantize_cells_device", [A(P), None, 0x1000, 5, 3, 16, 8, 0, 0x2000, 16, 32, None,
                                                                  0x4000, None])
    pal, fb = np.zeros(15, dtype=T.COLOR), np.zeros(16 * 140, dtype=T.COLOR)
    out = cells.quantize_cells_host(P, pal, 5, 3, (8, 16), fb, rows=(16, 32), spread=19, planes=("index", "fb", "cells"),
                                    device=2)
    assert list(out) == ["index", "fb", "cells"] and out["cells"].shape == (18,) and out["cells"].dtype == np.uint8
    assert out["index"].shape == out["fb"].shape == (16 * 140,)
    assert stand_in.calls.pop() == ("par_quantize_cells_host", [A(P), 2, A(pal), 5, 3, 8, 16, 19, A(fb), 16, 32, A(out["fb"]),
                                                                A(out["index"]), A(out["cells"])])
    whole = np.zeros(40 * 140, dtype=T.COLOR)
    out = cells.quantize_cells_host(P, pal, 5, 3, (16, 16), whole)
    assert list(out) == ["index"]
    assert stand_in.calls.pop() == ("par_quantize_cells_host", [A(P), -1, A(pal), 5, 3, 16, 16, 0, A(whole), 0, 40, None,
                                                                A(out["index"]), None])
    stand_in.status = 6
    with pytest.raises(par.ParError) as e:
        cells.quantize_cells(P, 0x1000, 5, 3, (8, 16), 0x2000, (16, 32), index_out=0x4000)
    assert e.value.status == 6 and str(e.value) == "PAR_ERR_EXTENT: par_quantize_cells_device"
    stand_in.status = -6
    with pytest.raises(par.ParError) as e:
        cells.cells_pairs(pal)
    assert e.value.status == 6 and str(e.value) == "PAR_ERR_EXTENT: par_cells_pairs"


# ---- the model the GPU tests compare with --------------------------------------------------------------------------

def same(a, b, tag):
    for name, x, y in zip(("index", "fb_out", "cell plane"), a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{tag}: {name}"


SK = [(1, 1), (1, 9), (2, 2), (4, 4), (7, 9), (9, 1), (21, 2)]


@pytest.mark.parametrize("cell", CM.CELLS)
def test_model_equals_the_loop_on_random_frames(T, cell):
    """21 x 19 whole (ragged in both directions, one edge cell 5 wide and 3 or 11 high) and 21 x 40 in row blocks."""
    for w, h, rows in ((21, 19, None), (21, 40, (16, 32)), (21, 40, (32, 40)), (9, 9, None), (1, 1, None)):
        assert CM.admits(rows, h, cell)
        r0, r1 = rows or (0, h)
        params = T.default_params(w, h)
        for n_sub, sub_size in SK:
            rng = np.random.default_rng(100 * w + 10 * n_sub + sub_size + cell[0] + 2 * cell[1])
            palette = Q.random_colors(T, rng, n_sub * sub_size)
            fb = Q.random_colors(T, rng, (r1 - r0) * w)
            for spread in (0, 24):
                got = CM.model(params, palette, n_sub, sub_size, cell, fb, rows, spread)
                same(got, CM.model_loop(params, palette, n_sub, sub_size, cell, fb, rows, spread),
                     f"{w}x{h} rows {rows} cells {cell} S {n_sub} K {sub_size} spread {spread}")
                assert len(got[2]) == -(-w // cell[0]) * -(-(r1 - r0) // cell[1])


@pytest.mark.parametrize("cell", CM.CELLS)
def test_model_equals_the_loop_on_cells_drawn_near_sub_palettes(T, cell):
    rng = np.random.default_rng(31 + cell[0] + 2 * cell[1])
    params = T.default_params(45, 35)
    for n_sub, sub_size in ((4, 4), (8, 4), (6, 2)):
        palette = Q.random_colors(T, rng, n_sub * sub_size)
        fb, drawn = CM.near_sub_palettes(T, rng, params, palette, n_sub, sub_size, cell, 6)
        got = CM.model(params, palette, n_sub, sub_size, cell, fb, None, 0)
        same(got, CM.model_loop(params, palette, n_sub, sub_size, cell, fb, None, 0), f"cells {cell} S {n_sub} K {sub_size}")
        assert len(np.unique(got[2])) > 1, "the winners differ between cells"
        assert (got[2] == drawn).mean() > 0.8, "mostly the sub-palette a cell was drawn from"
        assert (got[0] // sub_size == got[2][cell_of(params, cell)]).all(), "every pixel indexes its cell's sub-palette"


def cell_of(params, cell):
    i = np.arange(params.width * params.height)
    return (i % params.width) // cell[0] + ((i // params.width) // cell[1]) * -(-params.width // cell[0])


def colors(T, rgb, alpha=255):
    a = np.zeros(len(rgb), dtype=T.COLOR)
    for j, c in enumerate(Q.CHANNELS):
        a[c] = [e[j] for e in rgb]
    a["alpha"] = alpha
    return a


def crafted(T):
    """name -> (params, palette, n_sub, sub_size, cell, fb, spread, (index, cell plane) worked out by hand)."""
    out = {}
    one = T.default_params(8, 8)
    # E(0) == E(1): every pixel lies 10 from either one-entry sub-palette; the lower one. With a third, worse one in front
    # the two equal ones are 1 and 2.
    fb = colors(T, [(20, 0, 0)] * 64, alpha=7)
    out["equal E, two"] = (one, colors(T, [(10, 0, 0), (30, 0, 0)]), 2, 1, (8, 8), fb, 0,
                           (np.zeros(64, np.uint8), np.array([0], np.uint8)))
    out["equal E, behind a worse one"] = (one, colors(T, [(100, 0, 0), (30, 0, 0), (10, 0, 0)]), 3, 1, (8, 8), fb, 0,
                                          (np.full(64, 1, np.uint8), np.array([1], np.uint8)))
    # equal distances within the chosen sub-palette: entries 2 and 3 both lie 10 from every pixel; the lower k, entry 2
    out["equal d within one"] = (one, colors(T, [(0, 0, 0), (200, 200, 200), (10, 0, 0), (30, 0, 0)]), 2, 2, (8, 8), fb, 0,
                                 (np.full(64, 2, np.uint8), np.array([1], np.uint8)))
    # the clamp at both ends under spread 255: off <= -8 where B4 < 8 and >= 7 where B4 >= 8, so 5 + off clamps to 0 and
    # 250 + off to 255 everywhere: every pixel IS an entry of sub-palette 0 and E(0) == 0. B4 >= 8 exactly where x + y is
    # odd.
    yy, xx = np.divmod(np.arange(64), 8)
    odd = ((xx + yy) & 1).astype(np.uint8)
    fb = colors(T, [(250, 250, 250) if o else (5, 5, 5) for o in odd])
    out["the clamp at both ends"] = (one, colors(T, [(0, 0, 0), (255, 255, 255), (1, 1, 1), (254, 254, 254)]), 2, 2,
                                     (8, 8), fb, 255, (odd, np.array([0], np.uint8)))
    # edge cells one pixel wide and one pixel high, 9 x 9: the cells (1, 0) of 1 x 8 pixels is black, the cell (0, 1) of
    # 8 x 1 and the corner cell of one pixel are white among white and black neighbours
    nine = T.default_params(9, 9)
    yy, xx = np.divmod(np.arange(81), 9)
    white = ((xx < 8) | (yy == 8)).astype(np.uint8)
    fb = colors(T, [(250, 240, 230) if w else (10, 20, 30) for w in white])
    out["edge cells one pixel wide"] = (nine, colors(T, [(0, 0, 0), (255, 255, 255)]), 2, 1, (8, 8), fb, 0,
                                        (white, np.array([1, 0, 1, 1], np.uint8)))
    # and under 16 x 16 cells the same frame is one cell, 73 white pixels against 8 black ones: all white
    out["one ragged 16 x 16 cell"] = (nine, colors(T, [(0, 0, 0), (255, 255, 255)]), 2, 1, (16, 16), fb, 0,
                                      (np.ones(81, np.uint8), np.array([1], np.uint8)))
    return out


CRAFTED = ["equal E, two", "equal E, behind a worse one", "equal d within one", "the clamp at both ends",
           "edge cells one pixel wide", "one ragged 16 x 16 cell"]


@pytest.mark.parametrize("name", CRAFTED)
def test_crafted_cells(T, name):
    cases = crafted(T)
    assert sorted(cases) == sorted(CRAFTED)
    params, palette, n_sub, sub_size, cell, fb, spread, (index, plane) = cases[name]
    got = CM.model(params, palette, n_sub, sub_size, cell, fb, None, spread)
    same(got, CM.model_loop(params, palette, n_sub, sub_size, cell, fb, None, spread), name)
    assert np.array_equal(got[0], index) and np.array_equal(got[2], plane), name
    assert np.array_equal(got[1]["alpha"], fb["alpha"])
    for c in Q.CHANNELS:
        assert np.array_equal(got[1][c], palette[c][index])
    d, _ = CM.nearest(params, palette, n_sub, sub_size, fb, None, spread)
    if name.startswith("equal E"):
        E = d.sum(axis=0)
        assert E[plane[0]] == E[plane[0] + 1] == 640 and (E >= 640).all()
    if name == "equal d within one":
        pal = np.stack([palette[c].astype(int) for c in Q.CHANNELS], axis=1)
        assert (np.abs(pal[2] - [20, 0, 0]).sum(), np.abs(pal[3] - [20, 0, 0]).sum()) == (10, 10)
    if name == "the clamp at both ends":
        _, raw = Q.dithered(params, fb, None, spread)
        assert raw.min() < 0 and raw.max() > 255 and ((raw < 0) | (raw > 255)).all(), "every channel clamps"
        assert d[:, 0].sum() == 0 and d[:, 1].sum() == 3 * 64


# ---- the consequences ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", CM.CELLS)
def test_one_sub_palette_is_quantise(T, cell):
    rng = np.random.default_rng(41)
    params = T.default_params(37, 23)
    fb = Q.random_colors(T, rng, 37 * 23)
    for K in (1, 9, 256):
        palette = Q.random_colors(T, rng, K)
        for spread in (0, 24, 255):
            index, out, plane = CM.model(params, palette, 1, K, cell, fb, None, spread)
            q_index, q_out = Q.model(params, palette, fb, None, spread)
            assert index.tobytes() == q_index.tobytes() and out.tobytes() == q_out.tobytes() and not plane.any()


def test_of_identical_sub_palettes_the_lower_one_is_chosen(T):
    rng = np.random.default_rng(42)
    params = T.default_params(37, 23)
    fb = Q.random_colors(T, rng, 37 * 23)
    a, b = Q.random_colors(T, rng, 4), Q.random_colors(T, rng, 4)
    single = CM.model(params, np.concatenate([a, b]), 2, 4, (8, 8), fb, None, 24)
    assert len(np.unique(single[2])) == 2
    doubled = CM.model(params, np.concatenate([a, b, a, b]), 4, 4, (8, 8), fb, None, 24)
    same(single, doubled, "a second copy of every sub-palette never wins")
    twice = CM.model(params, np.concatenate([a, a]), 2, 4, (8, 8), fb, None, 24)
    assert not twice[2].any() and twice[0].max() < 4


def test_a_cell_of_a_sub_palettes_entries_takes_it(T):
    rng = np.random.default_rng(43)
    params = T.default_params(93, 75)
    for cell in CM.CELLS:
        palette = Q.random_colors(T, rng, 6 * 3)
        palette[4 * 3:5 * 3] = palette[1 * 3:2 * 3]  # sub-palette 4 is a copy of 1: the lowest such s is 1
        fb, drawn = CM.near_sub_palettes(T, rng, params, palette, 6, 3, cell, 0)
        assert (drawn == 4).any() and len(np.unique(drawn)) == 6
        index, out, plane = CM.model(params, palette, 6, 3, cell, fb, None, 0)
        assert np.array_equal(plane, np.where(drawn == 4, 1, drawn))
        assert out.tobytes() == fb.tobytes()
        d, _ = CM.nearest(params, palette, 6, 3, fb, None, 0)
        assert (d[np.arange(len(fb)), plane[cell_of(params, cell)]] == 0).all()


def test_a_cell_depends_on_its_own_pixels_alone(T):
    rng = np.random.default_rng(44)
    params = T.default_params(37, 23)
    palette = Q.random_colors(T, rng, 16)
    fb = Q.random_colors(T, rng, 37 * 23)
    for cell in CM.CELLS:
        of = cell_of(params, cell)
        base = CM.model(params, palette, 4, 4, cell, fb, None, 24)
        other = fb.copy()
        other[of == 1] = Q.random_colors(T, rng, int((of == 1).sum()))
        moved = CM.model(params, palette, 4, 4, cell, other, None, 24)
        keep = of != 1
        assert np.array_equal(moved[0][keep], base[0][keep]) and moved[1][keep].tobytes() == base[1][keep].tobytes()
        assert np.array_equal(np.delete(moved[2], 1), np.delete(base[2], 1))
        assert not np.array_equal(moved[0][~keep], base[0][~keep])


@pytest.mark.parametrize("cell", CM.CELLS)
def test_a_row_block_equals_the_whole_frames_rows(T, cell):
    rng = np.random.default_rng(45)
    w, h = 37, 43
    params = T.default_params(w, h)
    palette = Q.random_colors(T, rng, 32)
    fb = Q.random_colors(T, rng, w * h)
    whole = CM.model(params, palette, 8, 4, cell, fb, None, 24)
    gcx = -(-w // cell[0])
    for r0, r1 in ((0, 16), (16, 32), (32, 43), (16, 43)):
        part = CM.model(params, palette, 8, 4, cell, fb[r0 * w:r1 * w], (r0, r1), 24)
        assert np.array_equal(part[0], whole[0][r0 * w:r1 * w]), (r0, r1)
        assert part[1].tobytes() == whole[1][r0 * w:r1 * w].tobytes(), (r0, r1)
        assert np.array_equal(part[2], whole[2][r0 // cell[1] * gcx:-(-r1 // cell[1]) * gcx]), (r0, r1)
    # the cells are cut at ABSOLUTE rows: the same block taken for rows that start 8 lower falls into other cells
    if cell[1] == 16:
        shifted = CM.model(T.default_params(w, h + 8), palette, 8, 4, (cell[0], 8), fb[16 * w:32 * w], (24, 40), 24)
        assert not np.array_equal(shifted[0], whole[0][16 * w:32 * w])


# ---- par_cells_pairs -------------------------------------------------------------------------------------------------

def test_pairs_are_itertools_combinations(par, T, cells):
    rng = np.random.default_rng(46)
    for n in range(2, 17):
        palette = Q.random_colors(T, rng, n)
        got = cells.cells_pairs(palette)
        combos = list(itertools.combinations(range(n), 2))
        assert len(got) == 2 * len(combos) == n * (n - 1)
        for q, (i, j) in enumerate(combos):
            assert got[2 * q] == palette[i] and got[2 * q + 1] == palette[j], (n, q)
        assert got.tobytes() == CM.pairs(palette).tobytes()
    assert len(cells.cells_pairs(Q.random_colors(T, rng, 16))) == 240


def test_pairs_errors_and_the_capacity_clip(par, T, cells):
    L = cells.lib()
    rng = np.random.default_rng(47)
    palette = Q.random_colors(T, rng, 16)
    full = CM.pairs(palette)
    for capacity in (0, 1, 2, 7, 239, 240, 256):
        out = np.full(256 * 4, 0x77, dtype=np.uint8).view(T.COLOR)
        assert L.par_cells_pairs(T.ptr(palette), 16, T.ptr(out), capacity) == 120
        kept = min(capacity, 240)
        assert out[:kept].tobytes() == full[:kept].tobytes() and (out[kept:].view(np.uint8) == 0x77).all(), capacity
    out = np.full(256 * 4, 0x77, dtype=np.uint8).view(T.COLOR)
    for pal, n, o, capacity in ((None, 4, out, 256), (palette, 4, None, 256), (palette, 4, out, -1), (palette, 1, out, 256),
                                (palette, 0, out, 256), (palette, -3, out, 256), (palette, 17, out, 256)):
        assert L.par_cells_pairs(T.ptr(pal), n, T.ptr(o), capacity) == -ERR_INVALID_ARG
    assert (out.view(np.uint8) == 0x77).all()
    for n in (1, 17):
        with pytest.raises(par.ParError) as e:
            cells.cells_pairs(palette[:n] if n == 1 else np.concatenate([palette, palette[:1]]))
        assert e.value.status == ERR_INVALID_ARG
