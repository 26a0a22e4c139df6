"""Finish without a GPU: the two calls are declared, exported and bound; every PAR_ERR_INVALID_ARG of the contract comes
back from both calls before any device work and with nothing written; the model the GPU tests lean on (finish.model) equals
the composition of the three per-pixel loops; the inputs the GPU tests use reach what they are chosen for; and the cut of a
call's rows into launches, which this call shares with par_outline_device, holds its four properties under a sanitiser
(tests/tile_row_cuts_check.cpp, a stand-alone program)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import finish as F
import headers
import outline as O
import present as P
import quantize as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = 1

DECLARATIONS = {
    "par_finish_device": "const par_params* params, void* stream, const par_outline_style* style, const par_pixel* gbuf, "
                         "int gbuf_row_begin, int gbuf_row_end, const par_color* d_palette, int n_colors, int spread, "
                         "const par_present_desc* desc, const par_color* fb, int row_begin, int row_end, void* out, "
                         "uint8_t* index_out",
    "par_finish_host": "const par_params* params, int device, const par_outline_style* style, const par_pixel* gbuf, "
                       "int gbuf_row_begin, int gbuf_row_end, const par_color* palette, int n_colors, int spread, "
                       "const par_present_desc* desc, const par_color* fb, int row_begin, int row_end, void* out, "
                       "uint8_t* index_out",
}


def test_declared_exported_and_bound(par):
    headers.assert_declared(par, "par_raytracer.h", DECLARATIONS, ("finish", "finish_host"))


# ---- argument errors: no device needed, nothing written -----------------------------------------------------------

NO_STYLE = dict(style=None, gbuf=None)
NO_PALETTE = dict(palette=None, n_colors=0, spread=0, index_out=None)

# (tag, overrides): one case per condition of the contract; each breaks that one condition alone. The good call is a
# frame of 8 x 6 with both stages: style (2, 128, 320), G-buffer rows (0, 6), 4 colours at spread 32, scale (2, 3) with
# a pitch of 80 (a gap of 16 bytes), rows (0, 6), an index plane asked for.
BAD_CALLS = [
    ("null params", dict(params=None)),
    ("null desc", dict(desc=None)),
    ("null fb", dict(fb=None)),
    ("null out", dict(out=None)),
    ("neither stage", dict(**NO_STYLE, **NO_PALETTE)),
    ("index_out without a palette", dict(palette=None, n_colors=0, spread=0)),
    ("spread != 0 without a palette", dict(palette=None, n_colors=0, index_out=None)),
    ("n_colors != 0 without a palette", dict(palette=None, spread=0, index_out=None)),
    ("style without gbuf", dict(gbuf=None)),
    ("gbuf without style", dict(style=None)),
    ("depth_step 0", dict(style=(0, 128, 320))),
    ("silhouette_scale -1", dict(style=(2, -1, 320))),
    ("silhouette_scale 1025", dict(style=(2, 1025, 320))),
    ("crease_scale -1", dict(style=(2, 128, -1))),
    ("crease_scale 1025", dict(style=(2, 128, 1025))),
    ("gbuf_row_begin negative", dict(grows=(-1, 6))),
    ("gbuf_row_begin > row_begin", dict(grows=(1, 6))),
    ("row_begin == row_end", dict(rows=(3, 3))),
    ("row_begin > row_end", dict(rows=(5, 2))),
    ("row_end > gbuf_row_end", dict(grows=(0, 5))),
    ("gbuf_row_end > height", dict(grows=(0, 7), rows=(0, 6))),
    ("no style: row_begin negative", dict(**NO_STYLE, rows=(-1, 4))),
    ("no style: row_begin == row_end", dict(**NO_STYLE, rows=(3, 3))),
    ("no style: row_begin > row_end", dict(**NO_STYLE, rows=(5, 2))),
    ("no style: row_end > height", dict(**NO_STYLE, rows=(0, 7))),
    ("n_colors 0", dict(n_colors=0)),
    ("n_colors 257", dict(n_colors=257)),
    ("spread -1", dict(spread=-1)),
    ("spread 256", dict(spread=256)),
    ("width 0", dict(width=0)),
    ("width negative", dict(width=-8)),
    ("scale_x 0", dict(scale_x=0)),
    ("scale_x 17", dict(scale_x=17, pitch=4 * 8 * 17)),
    ("scale_y 0", dict(scale_y=0)),
    ("scale_y 17", dict(scale_y=17)),
    ("order 2", dict(order=2)),
    ("order -1", dict(order=-1)),
    ("pitch not a multiple of 4", dict(pitch=82)),
    ("pitch below 4 * width * sx", dict(pitch=60)),
    ("4 * width * sx beyond an int32", dict(width=1 << 27, scale_x=16, pitch=0x7FFFFFFC)),
    ("no outline: 4 * width * sx beyond an int32", dict(**NO_STYLE, width=1 << 27, scale_x=16, pitch=0x7FFFFFFC)),
]

# every one of these passes the argument checks (the host form then needs a device)
GOOD_CALLS = [
    ("both stages", dict()),
    ("outline only", dict(**NO_PALETTE)),
    ("quantise only", dict(**NO_STYLE)),
    ("quantise only: the G-buffer rows are not read", dict(**NO_STYLE, grows=(-5, 1000))),
    ("no index plane", dict(index_out=None)),
    ("a block with its halo", dict(rows=(2, 4), grows=(1, 5))),
    ("spread 0 and 255, n_colors 1 and 256", dict(spread=255, n_colors=256)),
    ("the style's limits", dict(style=(1, 0, 1024))),
]


def call(par, T, which, over):
    """(status, nothing was written) of one call with the good arguments overridden by `over`."""
    L = par.lib()
    fn = L.par_finish_device if which == "device" else L.par_finish_host
    first = C.c_void_p(0) if which == "device" else -1  # the stream / the device
    params = T.default_params(8, 6)
    params.width = over.get("width", 8)
    palette = np.full(256 * 4, 0x5A, dtype=np.uint8).view(T.COLOR)  # host dummies: never dereferenced by a refused call
    fb = np.full(8 * 6 * 4, 0xA5, dtype=np.uint8).view(T.COLOR)
    gbuf = np.full(8 * 6 * 28, 0x69, dtype=np.uint8).view(T.PIXEL)
    index = np.full(8 * 6, 0x3C, dtype=np.uint8)
    out = np.full(6 * 3 * 80, 0xC3, dtype=np.uint8)
    desc = T.make_present_desc(over.get("scale_x", 2), over.get("scale_y", 3), over.get("pitch", 80), over.get("order", 0))
    arg = dict(params=params, desc=desc, fb=fb, out=out, style=(2, 128, 320), gbuf=gbuf, grows=(0, 6), palette=palette,
               n_colors=4, spread=32, rows=(0, 6), index_out=index)
    arg.update({k: v for k, v in over.items() if k in arg})
    style = None if arg["style"] is None else T.make_outline_style(*arg["style"])
    rc = fn(None if arg["params"] is None else C.byref(arg["params"]), first, T.ptr(style), T.ptr(arg["gbuf"]),
            arg["grows"][0], arg["grows"][1], T.ptr(arg["palette"]), arg["n_colors"], arg["spread"], T.ptr(arg["desc"]),
            T.ptr(arg["fb"]), arg["rows"][0], arg["rows"][1], T.ptr(arg["out"]), T.ptr(arg["index_out"]))
    untouched = bool((fb.view(np.uint8) == 0xA5).all() and (index == 0x3C).all() and (out == 0xC3).all() and
                     (palette.view(np.uint8) == 0x5A).all() and (gbuf.view(np.uint8) == 0x69).all())
    return rc, untouched


def test_the_good_calls_of_the_bad_calls_are_good(par, T):
    """What the cases start from passes every check of the contract, so each case breaks one condition alone: the host
    form gets past its argument checks (to PAR_OK with a device, PAR_ERR_NO_DEVICE without)."""
    assert 4 * (1 << 27) * 16 > 0x7FFFFFFF and ((4 * (1 << 27) * 16) & 0xFFFFFFFF) == 0 and 0x7FFFFFFC % 4 == 0
    assert len({tag for tag, _ in BAD_CALLS}) == len(BAD_CALLS)
    for tag, over in GOOD_CALLS:
        rc, _ = call(par, T, "host", over)
        assert rc in (0, 2), f"{tag}: status {rc}"


@pytest.mark.parametrize("which", ["device", "host"])
def test_invalid_arguments_need_no_device_and_write_nothing(par, T, which):
    for tag, over in BAD_CALLS:
        rc, untouched = call(par, T, which, over)
        assert rc == ERR_INVALID_ARG, f"{which}: {tag}: status {rc}"
        assert untouched, f"{which}: {tag}: something was written"


def test_binding_raises_invalid_arg(par, T):
    params = T.default_params(8, 6)
    with pytest.raises(par.ParError) as e:  # neither stage
        par.finish(params, T.make_present_desc(2, width=8), 0, (0, 6), 0)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(par.ParError) as e:
        par.finish_host(params, T.make_present_desc(17, pitch=4 * 8 * 17), np.zeros(48, dtype=T.COLOR),
                        palette=np.zeros(4, dtype=T.COLOR))
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(ValueError):
        par.finish_host(params, T.make_present_desc(2, width=8), np.zeros(47, dtype=T.COLOR),
                        palette=np.zeros(4, dtype=T.COLOR))
    with pytest.raises(ValueError):
        par.finish_host(params, T.make_present_desc(2, width=8), np.zeros(48, dtype=T.COLOR),
                        style=T.make_outline_style(2, 128, 320), gbuf=np.zeros(47, dtype=T.PIXEL))


# ---- the model the GPU tests compare with --------------------------------------------------------------------------

@pytest.mark.parametrize("stage_set", F.STAGE_SETS)
def test_model_equals_the_three_per_pixel_loops(T, stage_set):
    """7 x 5 frames: whole and a block with and without its halo, two scales, both orders, a gap."""
    params, gbuf, fb, palette = F.inputs(T, 7, 5, n_colors=6, seed=77)
    assert len(np.unique(O.classes(params, F.STYLE, gbuf, (0, 5), (0, 5)))) == 3
    for rows, grows in (((0, 5), (0, 5)), ((1, 4), (0, 5)), ((1, 4), (1, 4)), ((2, 5), (1, 5))):
        g, f = F.block_inputs(params, gbuf, fb, rows, grows)
        style, g, gr, pal, spread = F.stages(stage_set, F.STYLE, g, grows, palette, F.SPREAD)
        for sx, sy, order, gap in ((1, 1, P.RGBA, 0), (3, 2, P.BGRA, 12), (2, 5, P.RGBA, 4)):
            desc = T.make_present_desc(sx, sy, 4 * 7 * sx + gap, order)
            surface, index = F.model(params, style, g, gr, pal, spread, desc, f, rows, guard=0xEE)
            a = f if style is None else O.model_loop(params, style, g, gr, f, rows)[1]
            if pal is None:
                exp, exp_index = P.slow_model(params, desc, rows, fb=a, guard=0xEE), None
                assert index is None
            else:
                exp_index = Q.model_loop(params, pal, a, rows, spread)[0]
                exp = P.slow_model(params, desc, rows, index=exp_index, palette=pal, guard=0xEE)
                assert np.array_equal(index, exp_index), (rows, grows, sx, sy)
            assert surface.shape == ((rows[1] - rows[0]) * sy, 4 * 7 * sx + gap)
            assert surface.tobytes() == exp.tobytes(), (rows, grows, sx, sy, order, gap)
            assert (surface[:, 4 * 7 * sx:] == 0xEE).all()


FRAMES = [(37, 23, (5, 18)), (64, 16, (5, 16)), (130, 35, (5, 18)), (16, 64, (5, 18))]


@pytest.mark.parametrize("w,h,rows", FRAMES)
def test_the_gpu_tests_inputs_reach_what_they_are_chosen_for(T, w, h, rows):
    """The composition on the shapes of tests/test_gpu_finish.py: all three classes, the outlines change the indices, the
    whole palette is used, a block with halo rows equals those rows of the whole frame's and one without does not."""
    params, gbuf, fb, palette = F.inputs(T, w, h)
    cls = O.classes(params, F.STYLE, gbuf, (0, h), (0, h))
    counts = np.bincount(cls, minlength=3)
    assert (counts >= 50).all(), counts
    if (w, h) == (37, 23):
        assert counts.tolist() == [98, 308, 445]
    desc = T.make_present_desc(3, 2, 4 * w * 3 + 4, P.BGRA)
    surface, index = F.model(params, F.STYLE, gbuf, (0, h), palette, F.SPREAD, desc, fb, None, guard=0xEE)
    plain = Q.model(params, palette, fb, None, F.SPREAD)[0]
    assert (index != plain).sum() > 500 and len(np.unique(index)) == 17
    grows = O.halo(rows, h)
    g, f = F.block_inputs(params, gbuf, fb, rows, grows)
    s_halo, i_halo = F.model(params, F.STYLE, g, grows, palette, F.SPREAD, desc, f, rows, guard=0xEE)
    assert np.array_equal(s_halo, surface[rows[0] * 2:rows[1] * 2]) and np.array_equal(i_halo, index[rows[0] * w:rows[1] * w])
    g, f = F.block_inputs(params, gbuf, fb, rows, rows)
    i_bare = F.model(params, F.STYLE, g, rows, palette, F.SPREAD, desc, f, rows, guard=0xEE)[1]
    differ = (i_bare != index[rows[0] * w:rows[1] * w]).sum()
    assert 0 < differ < 2 * w, "without the halo a few pixels of the block's first and last row differ"


# ---- the cut of a call's rows into launches -------------------------------------------------------------------------

def test_tile_row_cuts_under_a_sanitiser(tmp_path):
    """tests/tile_row_cuts_check.cpp with csrc/par_hostcall.h alone (no HIP), address and undefined-behaviour sanitisers
    on, as a child process."""
    exe = tmp_path / "tile_row_cuts_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "pixel-art-raytracer_amd", "csrc"),
           os.path.join(ROOT, "tests", "tile_row_cuts_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "warning" not in p.stderr, p.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith(" checks, 0 failures"), out.stdout[-2000:]
    assert int(out.stdout.strip().splitlines()[-1].split()[0]) >= 90
