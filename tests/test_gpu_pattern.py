"""GPU tests of pattern dither (par_quantize_pattern_device, par_quantize_pattern_host): every index plane and every
quantised frame byte for byte against the contract restated in numpy (pattern.model; tests/test_pattern_cpu.py holds it to
a per-pixel, per-candidate loop without a GPU). The shapes are the smallest at which each mechanism of the kernel can go
wrong: a lane takes two pixels, a workgroup 512, so 1 x 1 and 3 x 1 are groups that hang over an end, 37 x 23 has an odd
pixel count and rows (5, 18), and 131 x 67 is more than one workgroup (it would be at four pixels a lane too). The entry
counts go round the search's unroll by eight and its tail; every depth goes through its own count of candidates and one
of the three sorting networks (4, 8, 16).

Every plane is carved out of a guard-filled tensor (Carved of test_gpu_quantize.py) and the guards are checked after every
call."""
import numpy as np
import pytest

import palette as P
import palette_refine as R
import pattern as D
import present as PR
import quantize as Q
from test_gpu_quantize import Carved, check
from test_pattern_cpu import CRAFTED, GRAYBOX_REFINED, crafted

pytestmark = pytest.mark.gpu


def run(par, T, params, palette, fb, rows, depth, strength, want=("index", "fb"), in_place=False, shifts=(0, 0, 0),
        ordered=False):
    """One par_quantize_pattern_device call on carved device planes: ({"index": ..., "fb": ...} for the planes asked for,
    and the source as it is afterwards under "src"), with every guard byte checked. shifts: elements past a 16-byte
    boundary of the source and fb_out, bytes past one of index_out. ordered: par_quantize_device at spread 0 in its
    place, on the same buffers."""
    import torch
    r0, r1 = rows or (0, params.height)
    n = (r1 - r0) * params.width
    assert len(fb) == n
    d_pal = Carved(4 * len(palette), 4, palette)
    src = Carved(4 * n, 4 * shifts[0], fb)
    dst = src if in_place else (Carved(4 * n, 4 * shifts[1]) if "fb" in want else None)
    idx = Carved(n, shifts[2]) if "index" in want else None
    torch.cuda.synchronize()
    if ordered:
        par.quantize(params, d_pal.ptr, len(palette), src.ptr, (r0, r1), fb_out=dst.ptr if dst else None,
                     index_out=idx.ptr if idx else None, spread=0)
    else:
        par.quantize_pattern(params, d_pal.ptr, len(palette), src.ptr, (r0, r1), depth, strength,
                             fb_out=dst.ptr if dst else None, index_out=idx.ptr if idx else None)
    torch.cuda.synchronize()
    out = {"src": src.host(T.COLOR)}
    for name, plane in (("palette", d_pal), ("source", src), ("fb_out", dst), ("index_out", idx)):
        assert plane is None or plane.guards_intact(), f"{name}: bytes outside the plane were written"
    assert d_pal.host(T.COLOR).tobytes() == palette.tobytes(), "the palette was written"
    if dst is not None:
        out["fb"] = dst.host(T.COLOR)
    if idx is not None:
        out["index"] = idx.host(np.uint8)
    return out


def inputs(T, w, h, rows, n_colors, seed=0):
    rng = np.random.default_rng(7000 + 1000 * w + n_colors + seed)
    params = T.default_params(w, h)
    r0, r1 = rows or (0, h)
    return params, Q.random_colors(T, rng, n_colors), Q.random_colors(T, rng, (r1 - r0) * w)


# ---- 1. shapes and entry counts ------------------------------------------------------------------------------------

N_COLORS = [1, 2, 7, 8, 9, 255, 256]
OUTPUTS = [(("index", "fb"), False), (("index",), False), (("fb",), False), (("fb",), True), (("index", "fb"), True)]
SHAPES = [(1, 1, None), (3, 1, None), (37, 23, (5, 18)), (37, 23, None), (131, 67, None)]


@pytest.mark.parametrize("w,h,rows", SHAPES)
def test_shapes_and_entry_counts(par, T, w, h, rows):
    assert (37 * 23) % 2 == 1 and (13 * 37) % 2 == 1 and 131 * 67 > 4 * 256 * 8
    for n_colors in N_COLORS:
        params, palette, fb = inputs(T, w, h, rows, n_colors)
        for depth, strength in ((16, 256), (5, 255)):
            exp_index, exp_fb = D.model(params, palette, fb, rows, depth, strength)
            if n_colors > 1 and w > 3:
                assert len(np.unique(exp_index)) > 1, "the inputs should use more than one entry"
                assert (exp_index != Q.model(params, palette, fb, rows, 0)[0]).any(), "the dither should move some pixel"
            for want, in_place in (OUTPUTS if depth == 16 else OUTPUTS[:1]):
                tag = f"{w}x{h} rows {rows} n_colors {n_colors} depth {depth} strength {strength} {want} in place {in_place}"
                check(run(par, T, params, palette, fb, rows, depth, strength, want, in_place), fb, exp_index, exp_fb, tag,
                      in_place)


# ---- 2. every depth, the strengths at both ends -------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [None, (5, 18)])
def test_every_depth(par, T, rows):
    params, palette, fb = inputs(T, 37, 23, rows, 9, seed=1)
    distinct = set()
    for depth in range(1, 17):
        for strength in (256, 255):
            exp_index, exp_fb = D.model(params, palette, fb, rows, depth, strength)
            distinct.add(exp_index.tobytes())
            check(run(par, T, params, palette, fb, rows, depth, strength), fb, exp_index, exp_fb,
                  f"rows {rows} depth {depth} strength {strength}")
    assert len(distinct) >= 24, "the depths should give different planes"


@pytest.mark.parametrize("strength", [0, 1, 255, 256])
def test_strengths(par, T, strength):
    for n_colors, depth in ((9, 16), (33, 7), (2, 2)):
        params, palette, fb = inputs(T, 37, 23, None, n_colors, seed=2)
        exp_index, exp_fb = D.model(params, palette, fb, None, depth, strength)
        if strength == 0:
            assert exp_index.tobytes() == Q.model(params, palette, fb, None, 0)[0].tobytes()
        check(run(par, T, params, palette, fb, None, depth, strength), fb, exp_index, exp_fb,
              f"strength {strength} depth {depth} n_colors {n_colors}")
    # strengths 255 and 256 differ, and 1 differs from 0 only where floor(-e / 256) = -1 moves a tie or a boundary
    params, palette, fb = inputs(T, 37, 23, None, 9, seed=2)
    assert D.model(params, palette, fb, None, 16, 255)[0].tobytes() != D.model(params, palette, fb, None, 16, 256)[0].tobytes()


# ---- 3. alignment and bounds ----------------------------------------------------------------------------------------

def test_alignment_and_bounds(par, T):
    """The three planes at every 16-byte phase, independently: exact results whichever path the kernel takes (the vector
    form needs the source and fb_out at one 8-byte phase and index_out at the matching 2-byte phase), and no byte outside
    a plane written (run checks the guards round all of them)."""
    params, palette, fb = inputs(T, 37, 23, None, 17, seed=3)
    exp_index, exp_fb = D.model(params, palette, fb, None, 6, 256)
    for s in range(4):
        for f in range(4):
            for i in range(4):
                got = run(par, T, params, palette, fb, None, 6, 256, shifts=(s, f, i))
                check(got, fb, exp_index, exp_fb, f"source +{s}, fb_out +{f}, index_out +{i}")
        for i in range(16):
            got = run(par, T, params, palette, fb, None, 6, 256, want=("index",), shifts=(s, 0, i))
            check(got, fb, exp_index, exp_fb, f"source +{s}, index_out +{i}, index only")
        for f in range(4):
            got = run(par, T, params, palette, fb, None, 6, 256, want=("fb",), shifts=(s, f, 0))
            check(got, fb, exp_index, exp_fb, f"source +{s}, fb_out +{f}, fb only")
        for i in range(4):
            got = run(par, T, params, palette, fb, None, 6, 256, want=("index", "fb"), in_place=True, shifts=(s, s, i))
            check(got, fb, exp_index, exp_fb, f"source +{s} in place, index_out +{i}", in_place=True)
    # a block of rows: the planes of rows (5, 18) at odd phases
    blk = fb[5 * 37:18 * 37]
    e_index, e_fb = D.model(params, palette, blk, (5, 18), 6, 256)
    for shifts in ((1, 1, 3), (3, 2, 1), (2, 2, 2), (1, 3, 1)):
        check(run(par, T, params, palette, blk, (5, 18), 6, 256, shifts=shifts), blk, e_index, e_fb, f"rows (5, 18) at {shifts}")


# ---- 4. the crafted cases of test_pattern_cpu.py ---------------------------------------------------------------------

@pytest.mark.parametrize("name", CRAFTED)
def test_crafted_cases(par, T, name):
    """The clamp at both ends, the largest e, the floor of a negative product, two entries of equal luma, duplicates and
    padded copies (that each frame reaches its situation, and the expected plane worked out by hand, are in
    test_pattern_cpu.py)."""
    params, palette, fb, depth, strength, expected = crafted(T)[name]
    exp_index, exp_fb = D.model(params, palette, fb, None, depth, strength)
    assert np.array_equal(exp_index, expected)
    for shifts in ((0, 0, 0), (1, 1, 1), (1, 2, 0)):
        check(run(par, T, params, palette, fb, None, depth, strength, shifts=shifts), fb, exp_index, exp_fb, f"{name} at {shifts}")


# ---- 5. alpha ------------------------------------------------------------------------------------------------------------

def test_alpha_takes_no_part_and_passes_through(par, T):
    rng = np.random.default_rng(75)
    params = T.default_params(37, 23)
    palette = Q.random_colors(T, rng, 16, alpha=(1, 255))
    fb = Q.random_colors(T, rng, 37 * 23)
    assert len(np.unique(fb["alpha"])) > 100 and (palette["alpha"] != 0).all()
    exp_index, exp_fb = D.model(params, palette, fb, None, 8, 256)
    assert np.array_equal(exp_fb["alpha"], fb["alpha"])
    other = fb.copy()
    other["alpha"] = 255 - fb["alpha"]
    got = run(par, T, params, palette, fb, None, 8, 256)
    check(got, fb, exp_index, exp_fb, "alpha")
    assert np.array_equal(got["fb"]["alpha"], fb["alpha"])
    flipped = run(par, T, params, palette, other, None, 8, 256)
    assert np.array_equal(flipped["index"], exp_index) and np.array_equal(flipped["fb"]["alpha"], other["alpha"])
    got = run(par, T, params, palette, fb, None, 8, 256, want=("fb",), in_place=True)
    check(got, fb, exp_index, exp_fb, "alpha in place", in_place=True)


# ---- 6. the consequences ---------------------------------------------------------------------------------------------------

def test_depth_1_and_strength_0_are_quantise_at_spread_0(par, T):
    for n_colors in (1, 9, 256):
        params, palette, fb = inputs(T, 37, 23, None, n_colors, seed=6)
        plain = run(par, T, params, palette, fb, None, 0, 0, ordered=True, shifts=(1, 1, 3))
        assert plain["index"].tobytes() == Q.model(params, palette, fb, None, 0)[0].tobytes()
        for depth, strength in ((1, 0), (1, 256), (1, 131), (16, 0), (6, 0)):
            got = run(par, T, params, palette, fb, None, depth, strength, shifts=(1, 1, 3))
            assert got["index"].tobytes() == plain["index"].tobytes() and got["fb"].tobytes() == plain["fb"].tobytes(), \
                (n_colors, depth, strength)


def test_a_frame_of_palette_colours_and_padded_copies(par, T):
    rng = np.random.default_rng(76)
    params = T.default_params(37, 23)
    palette = Q.random_colors(T, rng, 7)
    palette = np.concatenate([palette, palette[:1], palette[:1]])  # padded copies of entry 0
    pick = rng.integers(0, 7, 37 * 23).astype(np.uint8)
    fb = palette[pick]
    fb["alpha"] = rng.integers(0, 256, len(fb))
    got = run(par, T, params, palette, fb, None, 16, 256)
    assert np.array_equal(got["index"], pick) and got["fb"].tobytes() == fb.tobytes()
    fb = Q.random_colors(T, rng, 37 * 23)
    exp_index, exp_fb = D.model(params, palette, fb, None, 16, 256)
    assert exp_index.max() < 7
    check(run(par, T, params, palette, fb, None, 16, 256), fb, exp_index, exp_fb, "padded copies never show")


def test_a_row_block_at_absolute_rows_equals_the_whole_frames_rows(par, T):
    params, palette, fb = inputs(T, 37, 23, None, 9, seed=7)
    whole = run(par, T, params, palette, fb, None, 7, 256)
    for r0, r1 in ((5, 18), (0, 1), (22, 23), (1, 23)):
        part = run(par, T, params, palette, fb[r0 * 37:r1 * 37], (r0, r1), 7, 256, shifts=(r0 & 3, 0, r1 & 3))
        assert np.array_equal(part["index"], whole["index"][r0 * 37:r1 * 37]), (r0, r1)
        assert part["fb"].tobytes() == whole["fb"][r0 * 37:r1 * 37].tobytes(), (r0, r1)
    assert not np.array_equal(D.model(params, palette, fb[5 * 37:18 * 37], (4, 17), 7, 256)[0], whole["index"][5 * 37:18 * 37]), \
        "the phase should show"


# ---- 7. in a frame loop ----------------------------------------------------------------------------------------------------

def test_in_a_frame_loop(par, oracle, T):
    """The graybox scene under two tinted ranged lights: render_device, then reset, count, cut, sum, emit at 33, six rounds
    of refine, the pattern quantise and present on one stream with no host wait between. The index plane and the surface
    are the model's, and the block error is the figure test_pattern_cpu.py asserts."""
    import torch
    from test_gpu_light_range import scene
    from test_gpu_light_tints import COLOUR, TINTS, expected
    from test_gpu_lights_graph import Planes
    from test_gpu_palette import Block, garbage_work
    from test_gpu_palette_refine import Call
    from test_gpu_parity import ALL, assert_planes_equal

    sc = scene("graybox", par, oracle, T)
    params = sc.params
    W, H = params.width, params.height
    lights, exp, _ = expected(T, sc, [3, 6], [200, 300], TINTS[:2], COLOUR, "graybox, two tinted ranged lights")
    fb = exp["fb"]
    N, ROUNDS, DEPTH, STRENGTH = 33, 6, 16, 256
    fitted, n_entries, _ = P.fit(T, fb, N)
    refined = R.refine(T, params, fb, None, fitted, ROUNDS)[0]
    exp_index, exp_fb = D.model(params, refined, fb, None, DEPTH, STRENGTH)
    figure = D.block_error(params, None, fb, exp_fb)
    print(f"block error of the refined palette under pattern dither: {figure}")
    assert figure == GRAYBOX_REFINED[1]
    desc = T.make_present_desc(2, 2, order=T.PRESENT_BGRA, width=W)
    exp_surface = PR.model(params, desc, None, index=exp_index, palette=refined)

    stream = torch.cuda.Stream()
    out = Planes(params, ALL)
    block = Block(T, garbage_work(T, 81))
    call = Call(T, fb[:1], fitted)  # (its palette, work block and changed count; the source is the rendered frame)
    scratch, index, quantised = Carved(W * H, 1), Carved(W * H, 0), Carved(4 * W * H, 0)
    surface = Carved(exp_surface.size, 0)
    torch.cuda.synchronize()
    with sc.renderer(par, par.LIGHTS_RANGED) as r:
        r.set_lights(lights)
        r.set_light_tints(T.make_tints(TINTS[:2]))
        s = stream.cuda_stream
        r.render_device(out.ptrs, flags=par.RENDER_COUNT_RAYS, stream=s)
        # (no host wait: the calls are ordered behind the frame and behind one another by the stream alone)
        par.palette_reset(block.ptr, stream=s)
        par.palette_count(params, out.ptrs["fb"], (0, H), block.ptr, stream=s)
        par.palette_cut(block.ptr, N, stream=s)
        par.palette_sum(params, out.ptrs["fb"], (0, H), block.ptr, stream=s)
        par.palette_emit(block.ptr, N, call.palette.ptr, stream=s)
        par.palette_refine_device(params, out.ptrs["fb"], (0, H), call.palette.ptr, N, ROUNDS, scratch.ptr, call.work.ptr,
                                  call.changed.ptr, stream=s)
        par.quantize_pattern(params, call.palette.ptr, N, out.ptrs["fb"], (0, H), DEPTH, STRENGTH, fb_out=quantised.ptr,
                             index_out=index.ptr, stream=s)
        par.present(params, desc, surface.ptr, (0, H), index=index.ptr, d_palette=call.palette.ptr, n_colors=N, stream=s)
        stream.synchronize()
        assert_planes_equal(out.host(T), exp, ALL, "the frame itself")
        for plane in (call.palette, call.work, call.changed, scratch, index, quantised, surface):
            assert plane.guards_intact()
        assert call.palette.host(T.COLOR).tobytes() == refined.tobytes(), "the refined palette"
        got_index, got_fb = index.host(np.uint8), quantised.host(T.COLOR)
        bad = np.nonzero(got_index != exp_index)[0]
        assert len(bad) == 0, f"index differs at {len(bad)} pixels, first {bad[:4]}"
        assert got_fb.tobytes() == exp_fb.tobytes(), "the quantised frame"
        assert D.block_error(params, None, out.host(T)["fb"], got_fb) == GRAYBOX_REFINED[1]
        assert surface.host(np.uint8).tobytes() == exp_surface.tobytes(), "the presented surface"
        r.stats()


# ---- 8. host form --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [None, (5, 18)])
def test_host_form_equals_the_device_path(par, T, rows):
    for n_colors, depth, strength in ((17, 6, 256), (256, 16, 255), (1, 3, 1)):
        params, palette, fb = inputs(T, 37, 23, rows, n_colors, seed=8)
        exp_index, exp_fb = D.model(params, palette, fb, rows, depth, strength)
        dev = run(par, T, params, palette, fb, rows, depth, strength)
        keep = fb.copy()
        got = par.quantize_pattern_host(params, palette, fb, depth, strength, rows=rows, planes=("index", "fb"))
        assert fb.tobytes() == keep.tobytes()
        assert got["index"].tobytes() == dev["index"].tobytes() == exp_index.tobytes()
        assert got["fb"].tobytes() == dev["fb"].tobytes() == exp_fb.tobytes()
        only = par.quantize_pattern_host(params, palette, fb, depth, strength, rows=rows)
        assert set(only) == {"index"} and only["index"].tobytes() == exp_index.tobytes()
        only = par.quantize_pattern_host(params, palette, fb, depth, strength, rows=rows, planes=("fb",), device=0)
        assert set(only) == {"fb"} and only["fb"].tobytes() == exp_fb.tobytes()
