"""Pattern dither without a GPU: the two calls are declared, exported and bound; every PAR_ERR_INVALID_ARG of both forms
comes back before any device work and with nothing written; the vectorised model the GPU tests lean on (pattern.model)
equals a per-pixel, per-entry, per-candidate loop over every depth, the strengths at the ends of the range and palettes of
1, 2, 9 and 256 entries; crafted frames reach the parts most likely to go wrong; the consequences the contract states
hold; and on the tinted graybox frame the 4 x 4 block error of pattern dithering lies below that of every ordered spread
tried, with the exact figures of the model."""
import ctypes as C

import numpy as np
import pytest

import headers
import palette as P
import palette_refine as R
import pattern as D
import quantize as Q

ERR_INVALID_ARG = 1

DECLARATIONS = {
    "par_quantize_pattern_device": "const par_params* params, void* stream, const par_color* d_palette, int n_colors, "
                                   "int depth, int strength, const par_color* fb, int row_begin, int row_end, "
                                   "par_color* fb_out, uint8_t* index_out",
    "par_quantize_pattern_host": "const par_params* params, int device, const par_color* palette, int n_colors, "
                                 "int depth, int strength, const par_color* fb, int row_begin, int row_end, "
                                 "par_color* fb_out, uint8_t* index_out",
}


def test_declared_exported_and_bound(par):
    headers.assert_declared(par, "par_raytracer.h", DECLARATIONS, ("quantize_pattern", "quantize_pattern_host"))


# ---- argument errors: no device needed, nothing written -----------------------------------------------------------

BAD = [
    ("null params", dict(params=None)),
    ("null palette", dict(palette=None)),
    ("null fb", dict(fb=None)),
    ("both outputs null", dict(fb_out=None, index_out=None)),
    ("n_colors 0", dict(n_colors=0)),
    ("n_colors 257", dict(n_colors=257)),
    ("depth 0", dict(depth=0)),
    ("depth 17", dict(depth=17)),
    ("depth negative", dict(depth=-1)),
    ("strength -1", dict(strength=-1)),
    ("strength 257", dict(strength=257)),
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
    for tag, over in BAD:
        params = T.default_params(8, 6)
        params.width = over.get("width", 8)
        palette = np.full(256 * 4, 0x5A, dtype=np.uint8).view(T.COLOR)  # host dummies: never dereferenced
        fb = np.full(8 * 6 * 4, 0xA5, dtype=np.uint8).view(T.COLOR)
        fb_out = np.full(8 * 6 * 4, 0xC3, dtype=np.uint8).view(T.COLOR)
        index_out = np.full(8 * 6, 0x3C, dtype=np.uint8)
        arg = dict(params=params, palette=palette, fb=fb, fb_out=fb_out, index_out=index_out, n_colors=4, depth=4,
                   strength=256, rows=(0, 6))
        arg.update({k: v for k, v in over.items() if k != "width"})
        p = None if arg["params"] is None else C.byref(arg["params"])
        first = C.c_void_p(0) if call == "device" else -1  # the stream / the device
        fn = L.par_quantize_pattern_device if call == "device" else L.par_quantize_pattern_host
        rc = fn(p, first, T.ptr(arg["palette"]), arg["n_colors"], arg["depth"], arg["strength"], T.ptr(arg["fb"]),
                arg["rows"][0], arg["rows"][1], T.ptr(arg["fb_out"]), T.ptr(arg["index_out"]))
        assert rc == ERR_INVALID_ARG, f"{call}: {tag}: status {rc}"
        assert (fb.view(np.uint8) == 0xA5).all() and (fb_out.view(np.uint8) == 0xC3).all() and \
            (index_out == 0x3C).all() and (palette.view(np.uint8) == 0x5A).all(), f"{call}: {tag}: something was written"


def test_binding_raises_invalid_arg(par, T):
    params = T.default_params(8, 6)
    with pytest.raises(par.ParError) as e:
        par.quantize_pattern(params, 0, 4, 0, (0, 6), 4, index_out=0)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(par.ParError) as e:
        par.quantize_pattern_host(params, np.zeros(4, dtype=T.COLOR), np.zeros(48, dtype=T.COLOR), 17)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(par.ParError) as e:
        par.quantize_pattern_host(params, np.zeros(4, dtype=T.COLOR), np.zeros(48, dtype=T.COLOR), 4, strength=300)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(ValueError):
        par.quantize_pattern_host(params, np.zeros(4, dtype=T.COLOR), np.zeros(40, dtype=T.COLOR), 4)


# ---- the model the GPU tests compare with --------------------------------------------------------------------------

STRENGTHS = [0, 1, 255, 256]


@pytest.mark.parametrize("n_colors", [1, 2, 9, 256])
def test_model_equals_the_loop(T, n_colors):
    """13 x 9 with rows (2, 7): 65 pixels that hold every (x & 3, y & 3); every depth, the strengths at both ends."""
    rng = np.random.default_rng(50 + n_colors)
    params = T.default_params(13, 9)
    rows = (2, 7)
    fb = Q.random_colors(T, rng, 5 * 13)
    palette = Q.random_colors(T, rng, n_colors)
    if n_colors >= 9:
        palette[5] = palette[1]  # a duplicate
        fb[:3] = palette[:3]     # and pixels that are entries
    moved = 0
    for depth in range(1, 17):
        for strength in STRENGTHS:
            index, out = D.model(params, palette, fb, rows, depth, strength)
            index_l, out_l = D.model_loop(params, palette, fb, rows, depth, strength)
            assert index.tobytes() == index_l.tobytes() and out.tobytes() == out_l.tobytes(), (depth, strength)
            assert np.array_equal(out["alpha"], fb["alpha"])
            moved += int((index != D.model(params, palette, fb, rows, 1, 0)[0]).sum())
    if n_colors > 1:
        assert moved > 0, "the dither should move some pixel"
        assert (index != 5).all() or n_colors < 9, "a duplicate never wins over its first copy"


def colors(T, rows):
    return np.array([tuple(r) for r in rows], dtype=T.COLOR)


def tiled(T, pixel, w=8, h=4):
    """A w x h frame of one colour, the alpha bytes all different."""
    fb = np.zeros(w * h, dtype=T.COLOR)
    fb["red"], fb["green"], fb["blue"] = pixel
    fb["alpha"] = (np.arange(w * h) * 7 + 3) & 0xFF
    return fb


def bayer_of(w, h, r0=0):
    i = np.arange(w * h)
    return np.array(Q.BAYER4)[(r0 + i // w) & 3, (i % w) & 3]


def crafted(T):
    """name -> (params, palette, fb, depth, strength, expected index plane): the situations of the contract as tiny frames
    of one colour over all sixteen matrix positions, shared with test_gpu_pattern.py. The expected planes are worked out
    by hand in the comments, not taken from the model."""
    params = T.default_params(8, 4)
    b4 = bayer_of(8, 4)
    out = {}
    # the clamp at the top: 250 with entries at 0 and 128. t = 250, then 250 + 122 j, clamped to 255: entry 1 every time.
    # (A byte that wraps instead would be 56 at j = 11 and find entry 0.)
    out["clamp at 255"] = (params, colors(T, [(0, 0, 0, 1), (128, 128, 128, 2)]), tiled(T, (250, 250, 250)), 16, 256,
                           np.ones(32, dtype=np.uint8))
    # the mirror image: 5 with entries at 255 and 127. t = 5, then 5 - 122 j, clamped to 0: entry 1 every time.
    out["clamp at 0"] = (params, colors(T, [(255, 255, 255, 1), (127, 127, 127, 2)]), tiled(T, (5, 5, 5)), 16, 256,
                         np.ones(32, dtype=np.uint8))
    # the largest |e|: white against the single entry black, e = 255 * 16 = 4080 a channel at the end
    out["largest e"] = (params, colors(T, [(0, 0, 0, 9)]), tiled(T, (255, 255, 255)), 16, 256, np.zeros(32, dtype=np.uint8))
    # the floor of a negative product: 10 against 11 (entry 0) and 8 (entry 1) at strength 255. j = 0: t = 10, entry 0
    # (3 against 6), e = -1. j = 1: floor(-255 / 256) = -1, t = 9, entry 1 (3 against 6); a division that truncates gives
    # t = 10 and entry 0 again. Sorted: entry 1 (darker), entry 0; rank = B4 * 2 >> 4.
    out["floor of a negative product"] = (params, colors(T, [(11, 11, 11, 0), (8, 8, 8, 0)]), tiled(T, (10, 10, 10)), 2, 255,
                                          np.where(b4 < 8, 1, 0).astype(np.uint8))
    # two entries of equal luma, 77 * 150 = 150 * 77: {150, 0, 0} and {0, 77, 0} against (75, 38, 0). j = 0: 113 against
    # 114, the red one, e = (-75, 38, 0). j = 1: t = (0, 76, 0), the green one. The keys tie on luma: the lower index
    # takes the lower rank, whichever colour it holds.
    tie = tiled(T, (75, 38, 0))
    out["equal luma, red first"] = (params, colors(T, [(150, 0, 0, 0), (0, 77, 0, 0), (255, 255, 255, 0)]), tie, 2, 256,
                                    np.where(b4 < 8, 0, 1).astype(np.uint8))
    out["equal luma, green first"] = (params, colors(T, [(0, 77, 0, 0), (150, 0, 0, 0), (255, 255, 255, 0)]), tie, 2, 256,
                                      np.where(b4 < 8, 0, 1).astype(np.uint8))
    # duplicates and padded copies of entry 0: 100 between 96 (entries 0, 2, 4, 5) and 104 (entries 1, 3). j = 0: 12
    # against 12, entry 0, e = 4. j = 1: t = 104, entry 1, e = 0, and so on: depth 5 finds entry 0 three times and entry 1
    # twice, rank = B4 * 5 >> 4 is below 3 for B4 <= 9. (A depth that is no power of two: the rank is seen to floor.)
    dup = colors(T, [(96, 96, 96, 1), (104, 104, 104, 2), (96, 96, 96, 3), (104, 104, 104, 4), (96, 96, 96, 1), (96, 96, 96, 1)])
    out["duplicates and padded copies, depth 5"] = (params, dup, tiled(T, (100, 100, 100)), 5, 256,
                                                    np.where(b4 <= 9, 0, 1).astype(np.uint8))
    # the same at depth 3: entries 0, 1, 0; rank = B4 * 3 >> 4 is 0 for B4 <= 5, 1 for B4 <= 10, else 2
    out["every matrix position, depth 3"] = (params, dup, tiled(T, (100, 100, 100)), 3, 256,
                                             np.where(b4 <= 10, 0, 1).astype(np.uint8))
    return out


CRAFTED = ["clamp at 255", "clamp at 0", "largest e", "floor of a negative product", "equal luma, red first",
           "equal luma, green first", "duplicates and padded copies, depth 5", "every matrix position, depth 3"]


@pytest.mark.parametrize("name", CRAFTED)
def test_crafted_cases(T, name):
    params, palette, fb, depth, strength, expected = crafted(T)[name]
    assert sorted(crafted(T)) == sorted(CRAFTED)
    index, out = D.model(params, palette, fb, None, depth, strength)
    index_l, out_l = D.model_loop(params, palette, fb, None, depth, strength)
    assert index.tobytes() == index_l.tobytes() and out.tobytes() == out_l.tobytes()
    assert np.array_equal(index, expected), (name, index.reshape(4, 8))
    assert np.array_equal(out["alpha"], fb["alpha"])
    keys, largest = D.candidates(palette, fb, depth, strength)
    if name.startswith("clamp"):
        assert largest == 122 * 16 and largest > 255, "t leaves the byte range from the second candidate on"
    if name == "largest e":
        assert largest == 255 * 16
    if name.startswith("equal luma"):
        assert len(set((keys[0] >> 8).tolist())) == 1 and len(set((keys[0] & 255).tolist())) == 2
    if "depth" in name:
        assert sorted(set(index.tolist())) == [0, 1] and len(set(D.ranks(params, 32, None, depth).tolist())) == depth


# ---- the consequences the contract states -----------------------------------------------------------------------------

def test_depth_1_and_strength_0_are_quantise_at_spread_0(T):
    rng = np.random.default_rng(61)
    params = T.default_params(13, 9)
    fb = Q.random_colors(T, rng, 13 * 9)
    for n_colors in (1, 7, 40):
        palette = Q.random_colors(T, rng, n_colors)
        plain = Q.model(params, palette, fb, None, 0)
        for depth, strength in ((1, 0), (1, 256), (1, 77), (16, 0), (5, 0)):
            got = D.model(params, palette, fb, None, depth, strength)
            assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes(), (depth, strength)


def test_a_frame_of_palette_colours_comes_back_as_it_is(T):
    rng = np.random.default_rng(62)
    params = T.default_params(13, 9)
    palette = Q.random_colors(T, rng, 7)
    palette = np.concatenate([palette, palette[:1], palette[:1]])  # padded copies of entry 0
    pick = rng.integers(0, 7, 13 * 9)
    fb = palette[pick]
    fb["alpha"] = rng.integers(0, 256, len(fb))
    for depth, strength in ((16, 256), (7, 255), (2, 1)):
        index, out = D.model(params, palette, fb, None, depth, strength)
        assert np.array_equal(index, pick) and out.tobytes() == fb.tobytes()
    # and on any frame a padded copy never shows
    fb = Q.random_colors(T, rng, 13 * 9)
    assert D.model(params, palette, fb, None, 16, 256)[0].max() < 7


def test_a_row_block_equals_the_whole_frames_rows(T):
    rng = np.random.default_rng(63)
    params = T.default_params(13, 9)
    fb = Q.random_colors(T, rng, 13 * 9)
    palette = Q.random_colors(T, rng, 6)
    whole, _ = D.model(params, palette, fb, None, 7, 256)
    part, _ = D.model(params, palette, fb[2 * 13:7 * 13], (2, 7), 7, 256)
    assert np.array_equal(whole[2 * 13:7 * 13], part)
    shifted, _ = D.model(params, palette, fb[2 * 13:7 * 13], (1, 6), 7, 256)
    assert not np.array_equal(shifted, part), "the phase should show"


# ---- the gap this closes: the tinted graybox frame ------------------------------------------------------------------

SPREADS = [0, 8, 16, 32, 64]
# block_error of the committed model: (ordered dither at SPREADS, pattern at depth 16 and strength 256)
GRAYBOX_FITTED = ([648209, 482570, 720775, 1102968, 2282529], 317970)
GRAYBOX_REFINED = ([472426, 296803, 607620, 908325, 2255299], 121671)


def graybox_palettes(par, oracle, T):
    """(params, fb, the 33-entry fitted palette, the same refined six rounds) of the tinted graybox frame."""
    from test_palette_refine_cpu import graybox_frame
    params, fb = graybox_frame(par, oracle, T)
    fitted, n_entries, _ = P.fit(T, fb, 33)
    assert n_entries == 33
    refined, _, _ = R.refine(T, params, fb, None, fitted, 6)
    return params, fb, fitted, refined


def test_pattern_dither_on_the_tinted_graybox_frame(par, oracle, T):
    """The 4 x 4 block error on this frame at 33 entries, depth 16 and strength 256: 317 970 with the fitted palette
    against 482 570 for the best ordered spread (8), 121 671 with the refined palette against 296 803."""
    params, fb, fitted, refined = graybox_palettes(par, oracle, T)
    assert (params.width, params.height) == (480, 320)
    for name, palette, (exp_ordered, exp_pattern) in (("fitted", fitted, GRAYBOX_FITTED), ("refined", refined, GRAYBOX_REFINED)):
        ordered = [D.block_error(params, None, fb, Q.model(params, palette, fb, None, s)[1]) for s in SPREADS]
        out = D.model(params, palette, fb, None, 16, 256)[1]
        pattern = D.block_error(params, None, fb, out)
        per_pixel = R.error(params, palette, fb)[0]
        print(f"{name}: block error {ordered} at spreads {SPREADS}, pattern {pattern}; per-pixel L1 at spread 0 {per_pixel}")
        for s, v in zip(SPREADS, ordered):
            assert pattern < v, f"{name}: pattern {pattern} against {v} at spread {s}"
        assert ordered == exp_ordered and pattern == exp_pattern, name
