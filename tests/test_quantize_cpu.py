"""Palette output without a GPU: the three calls are declared, exported and bound; every PAR_ERR_INVALID_ARG of the two
quantise calls comes back before any device work and with nothing written; par_palette_ramp equals its restatement
(quantize.ramp) byte for byte; and the vectorised model the GPU tests lean on (quantize.model) equals a per-pixel loop."""
import ctypes as C

import numpy as np
import pytest

import headers
import quantize as Q

ERR_INVALID_ARG = 1

DECLARATIONS = {
    "par_quantize_device": "const par_params* params, void* stream, const par_color* d_palette, int n_colors, int spread, "
                           "const par_color* fb, int row_begin, int row_end, par_color* fb_out, uint8_t* index_out",
    "par_quantize_host": "const par_params* params, int device, const par_color* palette, int n_colors, int spread, "
                         "const par_color* fb, int row_begin, int row_end, par_color* fb_out, uint8_t* index_out",
    "par_palette_ramp": "const par_params* params, int levels, par_color* out, int capacity",
}


def test_declared_exported_and_bound(par):
    headers.assert_declared(par, "par_raytracer.h", DECLARATIONS, ("quantize", "quantize_host", "palette_ramp"))


# ---- argument errors: no device needed, nothing written -----------------------------------------------------------

def _bad_calls(T):
    """(tag, overrides) — one case per condition of the contract; the good call's arguments are the defaults."""
    return [
        ("null params", dict(params=None)),
        ("null palette", dict(palette=None)),
        ("null fb", dict(fb=None)),
        ("both outputs null", dict(fb_out=None, index_out=None)),
        ("n_colors 0", dict(n_colors=0)),
        ("n_colors 257", dict(n_colors=257)),
        ("spread -1", dict(spread=-1)),
        ("spread 256", dict(spread=256)),
        ("width 0", dict(width=0)),
        ("width negative", dict(width=-8)),
        ("row_begin negative", dict(rows=(-1, 4))),
        ("row_begin == row_end", dict(rows=(3, 3))),
        ("row_begin > row_end", dict(rows=(5, 2))),
        ("row_end > height", dict(rows=(0, 7))),
    ]


@pytest.mark.parametrize("call", ["device", "host"])
def test_invalid_arguments_need_no_device_and_write_nothing(par, T, call):
    L = par.lib()
    for tag, over in _bad_calls(T):
        params = T.default_params(8, 6)
        params.width = over.get("width", 8)
        palette = np.full(256, 0x5A, dtype=np.uint8).view(T.COLOR)  # host dummies: never dereferenced
        fb = np.full(8 * 6 * 4, 0xA5, dtype=np.uint8).view(T.COLOR)
        fb_out = np.full(8 * 6 * 4, 0xC3, dtype=np.uint8).view(T.COLOR)
        index_out = np.full(8 * 6, 0x3C, dtype=np.uint8)
        arg = dict(params=params, palette=palette, fb=fb, fb_out=fb_out, index_out=index_out, n_colors=4, spread=0,
                   rows=(0, 6))
        arg.update({k: v for k, v in over.items() if k != "width"})
        p = None if arg["params"] is None else C.byref(arg["params"])
        first = C.c_void_p(0) if call == "device" else -1  # the stream / the device
        fn = L.par_quantize_device if call == "device" else L.par_quantize_host
        rc = fn(p, first, T.ptr(arg["palette"]), arg["n_colors"], arg["spread"], T.ptr(arg["fb"]), arg["rows"][0],
                arg["rows"][1], T.ptr(arg["fb_out"]), T.ptr(arg["index_out"]))
        assert rc == ERR_INVALID_ARG, f"{call}: {tag}: status {rc}"
        assert (fb.view(np.uint8) == 0xA5).all() and (fb_out.view(np.uint8) == 0xC3).all() and \
            (index_out == 0x3C).all() and (palette.view(np.uint8) == 0x5A).all(), f"{call}: {tag}: something was written"


def test_binding_raises_invalid_arg(par, T):
    params = T.default_params(8, 6)
    with pytest.raises(par.ParError) as e:
        par.quantize(params, 0, 4, 0, (0, 6), index_out=0)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(par.ParError) as e:
        par.quantize_host(params, np.zeros(4, dtype=T.COLOR), np.zeros(48, dtype=T.COLOR), spread=300)
    assert e.value.status == ERR_INVALID_ARG


# ---- par_palette_ramp ----------------------------------------------------------------------------------------------

def _as_rows(a):
    return [tuple(int(v) for v in e) for e in a]


@pytest.mark.parametrize("levels", [2, 3, 8, 63])
def test_ramp_of_the_default_params(par, T, levels):
    params = T.default_params()
    got = par.palette_ramp(params, levels)
    assert len(got) == 4 * levels + 1
    assert _as_rows(got) == Q.ramp(params, levels)
    assert got.tobytes() == Q.ramp_array(T, params, levels).tobytes()
    for p in range(4):  # the top band is the palette colour itself
        e = params.palette[p]
        assert _as_rows(got[p * levels + levels - 1:p * levels + levels]) == [(e.red, e.green, e.blue, e.alpha)]
    assert _as_rows(got[-1:]) == [(31, 31, 31, 0)]  # (uint8_t)(127 * 0.25f)
    a = int(0.25 * 255)
    assert _as_rows(got[:1]) == [((100 * a) // 255,) * 3 + (0,)]  # the bottom band is the colour at ambient


@pytest.mark.parametrize("ambient", [0.1, 0.3, 0.0, 1.0])
def test_ramp_with_an_ambient_that_is_inexact_in_binary_and_a_coloured_palette(par, T, ambient):
    rng = np.random.default_rng(5)
    params = T.default_params()
    params.ambient = ambient
    params.background = 201
    params.palette_size = 7
    for i in range(7):
        params.palette[i] = T.Color(*(int(v) for v in rng.integers(0, 256, 4)))
    for levels in (2, 5, 36):
        got = par.palette_ramp(params, levels)
        assert _as_rows(got) == Q.ramp(params, levels), (ambient, levels)
        assert got["alpha"][levels - 1] == params.palette[0].alpha


def test_ramp_capacity_smaller_than_the_count(par, T):
    params = T.default_params()
    full = par.palette_ramp(params, 8)
    for capacity in (0, 1, 10, 32, 33, 40):
        out = np.full(64 * 4, 0xEE, dtype=np.uint8).view(T.COLOR)
        n = par.lib().par_palette_ramp(C.byref(params), 8, T.ptr(out), capacity)
        assert n == 33
        k = min(capacity, 33)
        assert out[:k].tobytes() == full[:k].tobytes()
        assert (out[k:].view(np.uint8) == 0xEE).all(), f"capacity {capacity}: wrote past it"


def test_ramp_errors(par, T):
    L = par.lib()
    out = np.full(256 * 4, 0xEE, dtype=np.uint8).view(T.COLOR)

    def status(params, levels, o=out, capacity=256):
        return L.par_palette_ramp(None if params is None else C.byref(params), levels, T.ptr(o), capacity)

    good = T.default_params()
    assert status(good, 8) == 33
    assert status(None, 8) == -ERR_INVALID_ARG
    assert status(good, 8, o=None) == -ERR_INVALID_ARG
    for levels in (-1, 0, 1, 256):
        assert status(good, levels) == -ERR_INVALID_ARG, levels
    assert status(good, 63) == 253 and status(good, 64) == -ERR_INVALID_ARG  # 4 * 64 + 1 = 257 entries
    full = T.default_params()
    full.palette_size = 256
    for levels in (2, 8, 255):
        assert status(full, levels) == -ERR_INVALID_ARG, "a 256-entry palette leaves no room for any ramp"
    for size in (0, -3, 257):
        p = T.default_params()
        p.palette_size = size
        assert status(p, 2) == -ERR_INVALID_ARG, size
    for ambient in (-0.01, 1.5, float("nan")):
        p = T.default_params()
        p.ambient = ambient
        assert status(p, 2) == -ERR_INVALID_ARG, ambient
    out[:] = np.full(256 * 4, 0xEE, dtype=np.uint8).view(T.COLOR)
    for call in (lambda: status(good, 64), lambda: status(full, 2), lambda: status(good, 1)):
        call()
        assert (out.view(np.uint8) == 0xEE).all(), "a refused call wrote entries"
    with pytest.raises(par.ParError) as e:
        par.palette_ramp(good, 64)
    assert e.value.status == ERR_INVALID_ARG


# ---- the model the GPU tests compare with --------------------------------------------------------------------------

@pytest.mark.parametrize("spread", [0, 200])
@pytest.mark.parametrize("rows", [None, (1, 6), (3, 4)])
def test_model_equals_the_per_pixel_loop(T, spread, rows):
    rng = np.random.default_rng(11)
    params = T.default_params(9, 7)
    r0, r1 = rows or (0, 7)
    fb = Q.random_colors(T, rng, (r1 - r0) * 9)
    fb[:4] = np.array([(0, 1, 2, 9), (255, 254, 253, 7), (40, 40, 40, 1), (41, 40, 40, 2)], dtype=T.COLOR)
    palette = np.array([(40, 40, 40, 3), (200, 10, 90, 255), (40, 40, 40, 77), (0, 0, 0, 0), (250, 250, 250, 1)],
                       dtype=T.COLOR)  # entries 0 and 2 are the same colour
    index, out = Q.model(params, palette, fb, rows, spread)
    index_l, out_l = Q.model_loop(params, palette, fb, rows, spread)
    assert index.tobytes() == index_l.tobytes() and out.tobytes() == out_l.tobytes()
    assert (index != 2).all(), "a duplicate never wins over its first copy"
    assert np.array_equal(out["alpha"], fb["alpha"])
    _, raw = Q.dithered(params, fb, rows, spread)
    if spread:
        assert (raw < 0).any() and (raw > 255).any(), "the inputs should clamp at both ends"
        assert (index != Q.model(params, palette, fb, rows, 0)[0]).any(), "the dither should move some pixel"
    else:
        assert index[2] == 0 and index[3] == 0


def test_model_dither_phase_follows_the_absolute_row(T):
    """A row block is dithered by its absolute rows: rows (1, 6) of a frame equal the same rows of the whole frame."""
    rng = np.random.default_rng(12)
    params = T.default_params(9, 7)
    fb = Q.random_colors(T, rng, 63)
    palette = Q.random_colors(T, rng, 6)
    whole, _ = Q.model(params, palette, fb, None, 200)
    part, _ = Q.model(params, palette, fb[9:54], (1, 6), 200)
    assert np.array_equal(whole[9:54], part)
    shifted, _ = Q.model(params, palette, fb[9:54], (0, 5), 200)
    assert not np.array_equal(shifted, part), "the phase should show"
