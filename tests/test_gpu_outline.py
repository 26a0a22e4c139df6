"""GPU tests of outlines (par_outline_device, par_outline_host): every class plane and every outlined frame byte for byte
against the contract restated in numpy (outline.model; tests/test_outline_cpu.py holds it to a per-pixel loop without a
GPU), with guard bytes round every plane. Most cases render nothing: the call takes any G-buffer, and the planes are
built in numpy at the smallest shapes at which each mechanism of the kernel can go wrong.

Each case first asserts on the host, from the model, that its input reaches the situation it is named for.

The kernel's tile, as these shapes assume it: TILE_W x TILE_H = 64 x 16 pixels a workgroup, staged with a one-texel halo;
the grid's y extent allows MAX_TILE_ROWS tile rows a launch."""
import numpy as np
import pytest

import outline as O
import quantize as Q

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 16
MAX_TILE_ROWS = 65535
STYLE = (2, 128, 320)
OUTPUTS = [(("edge", "fb"), False), (("edge",), False), (("fb",), False), (("fb",), True)]


def run_and_check(par, T, params, style, gbuf, grows, fb, rows, tag, want=("edge", "fb"), in_place=False,
                  shifts=(0, 0, 0, 0)):
    exp_edge, exp_fb = O.model(params, style, gbuf, grows, fb, rows)
    got = O.run(par, T, params, T.make_outline_style(*O.style_ints(style)), gbuf, grows, fb, rows, want, in_place, shifts)
    O.check(got, gbuf, fb, exp_edge, exp_fb, tag, in_place)
    return got, exp_edge, exp_fb


# ---- 1. shapes -------------------------------------------------------------------------------------------------------

WIDTHS = [1, 2, 3, TILE_W - 1, TILE_W, TILE_W + 1, 2 * TILE_W]
HEIGHTS = [1, 2, 3, TILE_H - 1, TILE_H, TILE_H + 1, 2 * TILE_H]


def blocks_of(h):
    """(rows, G-buffer rows) of a shape of height h: whole, and a row block with both halos, one halo each, and none."""
    r0 = h // 3
    rows = (r0, max(r0 + 1, h - h // 3))
    both = O.halo(rows, h)
    return [((0, h), (0, h)), (rows, both), (rows, (both[0], rows[1])), (rows, (rows[0], both[1])), (rows, rows)]


def shape_case(par, T, w, h):
    rng = np.random.default_rng(100 * w + h)
    params = T.default_params(w, h)
    gbuf = O.random_texels(T, rng, params, w * h)
    fb = O.random_colors(T, rng, w * h)
    whole = O.classes(params, STYLE, gbuf, (0, h), (0, h))
    if w * h >= 100:
        assert all((whole == c).sum() > 0 for c in (0, 1, 2)), f"{w}x{h}: the input should reach every class"
    for rows, grows in blocks_of(h):
        tag = f"{w}x{h} rows {rows} G-buffer rows {grows}"
        _, exp_edge, _ = run_and_check(par, T, params, STYLE, O.block(gbuf, w, grows), grows, O.block(fb, w, rows), rows, tag)
        if grows == O.halo(rows, h):
            assert exp_edge.tobytes() == O.block(whole, w, rows).tobytes(), f"{tag}: the haloed block is the frame's rows"
    return params, gbuf, whole


@pytest.mark.parametrize("w", WIDTHS)
def test_shapes_round_the_tile(par, T, w):
    halo_matters = 0
    for h in HEIGHTS:
        params, gbuf, whole = shape_case(par, T, w, h)
        rows, _ = blocks_of(h)[1]
        bare = O.classes(params, STYLE, O.block(gbuf, w, rows), rows, rows)
        halo_matters += int((bare != O.block(whole, w, rows)).sum())
    if w >= TILE_W - 1:
        assert halo_matters > 0, "somewhere the unhaloed block should differ from the frame's rows"


@pytest.mark.parametrize("w,h", [(37, 23), (130, 19)])
def test_odd_shapes(par, T, w, h):
    assert w % 4 != 0 and h % TILE_H != 0
    shape_case(par, T, w, h)


def test_more_rows_than_one_launch_takes(par, T):
    """A frame two pixels wide with more tile rows than the grid's y extent: the host cuts it into two launches, and the
    rows beside the cut see each other."""
    w, h = 2, MAX_TILE_ROWS * TILE_H + TILE_H + 3
    rng = np.random.default_rng(8)
    params = T.default_params(w, h)
    gbuf = O.random_texels(T, rng, params, w * h)
    fb = O.random_colors(T, rng, w * h)
    cut = MAX_TILE_ROWS * TILE_H
    _, exp_edge, _ = run_and_check(par, T, params, STYLE, gbuf, (0, h), fb, (0, h), "two launches")
    beside = exp_edge[(cut - 1) * w:(cut + 1) * w]
    bare = np.concatenate([O.classes(params, STYLE, gbuf[:cut * w], (0, cut), (cut - 1, cut)),
                           O.classes(params, STYLE, gbuf[cut * w:], (cut, h), (cut, cut + 1))])
    print(f"rows {cut - 1} and {cut}: {beside} with each other, {bare} without")
    assert (beside != bare).any() and (exp_edge[cut * w:] != 0).any()


# ---- 2. situations -----------------------------------------------------------------------------------------------------

N_A, N_B = (0x3F800000, 0, 0), (0, 0x3F800000, 0)  # two normals, as words
W7, H5 = 7, 5
CX, CY = 3, 2  # the pixel the situations are about


def texel(normal=N_A, colour=0x11223344, y=100, z=60, entity=7):
    return np.array([normal[0], normal[1], normal[2], colour, y & O.M32, z & O.M32, entity & O.M32], dtype=np.uint32)


def frame_of(T, params, base):
    """A W7 x H5 G-buffer of the texel `base` everywhere (None: background), as (PIXEL array, its (H5, W7, 7) words)."""
    g = np.zeros(W7 * H5, dtype=T.PIXEL)
    w = g.view(np.uint32).reshape(H5, W7, 7)
    w[:] = np.array([0, 0, 0, O.background_word(params), 0, 0, 0], dtype=np.uint32) if base is None else base
    return g, w


def at(edge, x=CX, y=CY):
    return int(edge[y * W7 + x])


def situation(par, T, params, gbuf, step, tag, expect):
    """Runs the W7 x H5 frame; `expect`: {(x, y): class} the model must give (the situation), then the GPU the model."""
    rng = np.random.default_rng(5)
    fb = O.random_colors(T, rng, W7 * H5)
    style = (step, 100, 300)
    edge = O.classes(params, style, gbuf, (0, H5), (0, H5))
    for (x, y), c in expect.items():
        assert at(edge, x, y) == c, f"{tag}: the model gives ({x}, {y}) class {at(edge, x, y)}, the situation needs {c}"
    run_and_check(par, T, params, style, gbuf, (0, H5), fb, (0, H5), tag)
    return edge


SIDES = {"left": (-1, 0), "right": (1, 0), "up": (0, -1), "down": (0, 1)}


def test_silhouette_against_the_background_on_each_side(par, T):
    params = T.default_params(W7, H5)
    gbuf, w = frame_of(T, params, texel())
    assert not O.classes(params, (4, 0, 0), gbuf, (0, H5), (0, H5)).any(), "one entity, one normal, no background: no line"
    bg = np.array([0, 0, 0, O.background_word(params), 0, 0, 0], dtype=np.uint32)
    for side, (dx, dy) in SIDES.items():
        gbuf, w = frame_of(T, params, texel())
        w[CY + dy, CX + dx] = bg
        edge = situation(par, T, params, gbuf, 4, f"background to the {side}", {(CX, CY): 2, (CX + dx, CY + dy): 0})
        assert (edge == 2).sum() == 4, "the four pixels round the hole, and never the hole"


def test_entity_edges_at_the_depth_step(par, T):
    params = T.default_params(W7, H5)
    step = 5
    for side, (dx, dy) in SIDES.items():
        for d, mine, theirs in ((step - 1, 0, 0), (step, 2, 0), (-step, 0, 2), (-(step - 1), 0, 0)):
            gbuf, w = frame_of(T, params, texel())
            w[CY + dy, CX + dx] = texel(y=100 - d, entity=8)  # key(T) - key(N) = d
            edge = situation(par, T, params, gbuf, step, f"{side} neighbour of another entity at d = {d}",
                             {(CX, CY): mine, (CX + dx, CY + dy): theirs})
            # (a neighbour that lies a step behind is a hole to the four pixels round it; one a step in front is the line)
            assert (edge != 0).sum() == {step: 4, -step: 1}.get(d, 0), "the line lies on the nearer object only"
    # z counts as y does: key = y - z
    gbuf, w = frame_of(T, params, texel())
    w[CY, CX + 1] = texel(z=60 + step, entity=8)
    situation(par, T, params, gbuf, step, "the depth step in z", {(CX, CY): 2, (CX + 1, CY): 0})


def test_equal_entities_with_a_large_depth_difference_are_no_silhouette(par, T):
    params = T.default_params(W7, H5)
    for side, (dx, dy) in SIDES.items():
        gbuf, w = frame_of(T, params, texel())
        w[CY + dy, CX + dx] = texel(y=100 - 90)
        edge = situation(par, T, params, gbuf, 1, f"same entity, d = 90, {side}", {(CX, CY): 0, (CX + dx, CY + dy): 0})
        assert not edge.any()


def test_creases_look_right_and_down_only(par, T):
    params = T.default_params(W7, H5)
    for side, (dx, dy) in SIDES.items():
        gbuf, w = frame_of(T, params, texel())
        w[CY + dy, CX + dx] = texel(normal=N_B)
        # the odd texel out is a crease itself where ITS right or down neighbour is the plain one: always, here
        mine = 1 if side in ("right", "down") else 0
        edge = situation(par, T, params, gbuf, 4, f"another normal to the {side}", {(CX, CY): mine, (CX + dx, CY + dy): 1})
        assert (edge == 2).sum() == 0
        # left and up neighbours of the odd one see it to their right / below: creases; (CX, CY) is one only by right / down
        assert (edge == 1).sum() == 3
    # a crease gives way to a silhouette, and is not drawn on the far side of one
    gbuf, w = frame_of(T, params, texel())
    w[CY, CX + 1] = texel(normal=N_B, y=100 - 9, entity=8)  # to the right: another normal, but 9 further away
    situation(par, T, params, gbuf, 4, "crease or silhouette", {(CX, CY): 2})
    gbuf, w = frame_of(T, params, texel())
    w[CY, CX + 1] = texel(normal=N_B, y=100 + 9, entity=8)  # to the right: another normal, 9 nearer: ITS silhouette
    situation(par, T, params, gbuf, 4, "no crease behind a silhouette", {(CX, CY): 0, (CX + 1, CY): 2})
    gbuf, w = frame_of(T, params, texel())
    w[CY, CX + 1] = texel(normal=N_B, y=100 + 3, entity=8)  # 3 nearer, below the step: a crease between two entities
    situation(par, T, params, gbuf, 4, "a crease between two entities", {(CX, CY): 1, (CX + 1, CY): 1})


def test_minus_zero_differs_from_plus_zero(par, T):
    params = T.default_params(W7, H5)
    for k in range(3):
        gbuf, w = frame_of(T, params, texel(normal=(0, 0, 0)))
        odd = [0, 0, 0]
        odd[k] = 0x80000000
        w[CY, CX + 1] = texel(normal=tuple(odd))
        assert np.float32(0.0) == w[CY, CX + 1, :3].view(np.float32)[k], "equal as floats"
        situation(par, T, params, gbuf, 4, f"-0.0 in normal word {k}", {(CX, CY): 1})
    # and NaN words that are equal bit for bit are no crease
    gbuf, w = frame_of(T, params, texel(normal=(0x7FC00000, 0x7FC00000, 0x7FC00000)))
    assert not situation(par, T, params, gbuf, 4, "NaN normals, all alike", {(CX, CY): 0}).any()


@pytest.mark.parametrize("word", range(7))
def test_one_byte_off_the_background_is_covered(par, T, word):
    params = T.default_params(W7, H5)
    for byte in range(4):
        gbuf, w = frame_of(T, params, None)
        w[CY, CX, word] ^= np.uint32(1 << (8 * byte + (7 if byte == 3 else 0)))
        assert O.covered(params, gbuf).sum() == 1
        edge = situation(par, T, params, gbuf, 4, f"word {word} byte {byte} off the background", {(CX, CY): 2})
        assert (edge != 0).sum() == 1, "background pixels are never outlined"


def test_keys_whose_difference_wraps(par, T):
    params = T.default_params(W7, H5)
    step = 4
    # key(T) = 0x7FFFFFFF, key(N) = 0x80000003: N is 4 nearer in wrapping arithmetic, and the far smaller int32
    gbuf, w = frame_of(T, params, texel(y=0x7FFFFFFF, z=0))
    w[CY, CX + 1] = texel(y=0x80000003, z=0, entity=8)
    w[CY + 1, CX] = texel(y=0x80000003, z=0, entity=8)
    situation(par, T, params, gbuf, step, "keys either side of 2^31", {(CX, CY): 0, (CX + 1, CY): 2, (CX, CY + 1): 2})
    # y - z itself wraps: y = -2^31, z = 1 gives key 0x7FFFFFFF
    gbuf, w = frame_of(T, params, texel(y=-(1 << 31), z=1))
    w[CY, CX + 1] = texel(y=-(1 << 31) + 4, z=0, entity=8)  # key 0x80000004: 5 nearer
    situation(par, T, params, gbuf, step + 1, "y - z wraps", {(CX, CY): 0, (CX + 1, CY): 2})
    # a difference of exactly 2^31 is negative both ways round: no silhouette either side
    gbuf, w = frame_of(T, params, texel(y=0, z=0))
    w[CY, CX + 1] = texel(y=-(1 << 31), z=0, entity=8)
    situation(par, T, params, gbuf, 1, "d = -2^31", {(CX, CY): 0, (CX + 1, CY): 0})
    # the largest step
    gbuf, w = frame_of(T, params, texel(y=0x7FFFFFFF, z=0))
    w[CY, CX + 1] = texel(y=0, z=0, entity=8)
    situation(par, T, params, gbuf, 0x7FFFFFFF, "depth_step 2^31 - 1", {(CX, CY): 2, (CX + 1, CY): 0})


def test_texels_of_arbitrary_bits(par, T):
    rng = np.random.default_rng(9)
    for w, h in ((37, 23), (TILE_W + 4, TILE_H + 1)):
        params = T.default_params(w, h)
        gbuf = rng.integers(0, 256, w * h * 28, dtype=np.uint8).view(T.PIXEL)
        gbuf[rng.integers(0, w * h, w * h // 4)] = gbuf[0]  # some equal neighbours
        fb = O.random_colors(T, rng, w * h)
        for step in (1, 1 << 30):
            _, edge, _ = run_and_check(par, T, params, (step, 0, 1024), gbuf, (0, h), fb, (0, h), f"random bits {w}x{h}")
            assert (edge == 2).any() and (edge != 2).any()


# ---- 3. scales and outputs -------------------------------------------------------------------------------------------

def three_class_input(T, w, h, seed):
    rng = np.random.default_rng(seed)
    params = T.default_params(w, h)
    gbuf = O.random_texels(T, rng, params, w * h)
    edge = O.classes(params, STYLE, gbuf, (0, h), (0, h))
    assert all((edge == c).sum() >= 16 for c in (0, 1, 2)), np.bincount(edge)
    return params, gbuf, edge, rng


def test_scales_at_their_ends(par, T):
    w, h = 68, 20
    params, gbuf, edge, rng = three_class_input(T, w, h, 31)
    ends = np.array([0, 1, 254, 255], dtype=np.uint8)
    fb = np.zeros(w * h, dtype=T.COLOR)
    for ch in Q.CHANNELS + ("alpha",):
        fb[ch] = ends[rng.integers(0, 4, w * h)]
    for c in (1, 2):  # every end value under every class
        assert all(v in fb["red"][edge == c] for v in ends)
    scales = (0, 255, 256, 257, 1024)
    for s in scales:
        for c in scales:
            style = (STYLE[0], s, c)
            got, exp_edge, exp_fb = run_and_check(par, T, params, style, gbuf, (0, h), fb, (0, h), f"scales {s}, {c}")
            assert np.array_equal(got["fb"]["alpha"], fb["alpha"]), "alpha passes through"
            assert exp_edge.tobytes() == edge.tobytes(), "the class does not depend on the scales"
            if (s, c) == (256, 256):
                assert got["fb"].tobytes() == fb.tobytes() and (got["edge"] != 0).any(), "classes reported, fb unchanged"
            if s == 0:
                assert not got["fb"]["red"][edge == 2].any()
            if c == 1024:
                assert (got["fb"]["green"][(edge == 1) & (fb["green"] >= 254)] == 255).all(), "clamped at 255"
                assert (got["fb"]["green"][(edge == 1) & (fb["green"] == 1)] == 4).all()
    assert (255 * 257) >> 8 == 255 and (254 * 257) >> 8 == 254 and (254 * 255) >> 8 == 253 and (1 * 255) >> 8 == 0


@pytest.mark.parametrize("w,h", [(68, 20), (37, 23)])
def test_every_set_of_outputs(par, T, w, h):
    params, gbuf, edge, rng = three_class_input(T, w, h, 32)
    fb = O.random_colors(T, rng, w * h)
    for want, in_place in OUTPUTS:
        got, _, _ = run_and_check(par, T, params, STYLE, gbuf, (0, h), fb, (0, h), f"{w}x{h} {want} in place {in_place}",
                                  want, in_place)
        assert set(got) == set(want) | {"gbuf", "src"}
    # the mask alone needs no frame at all
    got = O.run(par, T, params, T.make_outline_style(*STYLE), gbuf, (0, h), None, (0, h), want=("edge",))
    assert got["edge"].tobytes() == edge.tobytes()


# ---- 4. alignment and bounds -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(68, 18), (37, 23)])
def test_alignment_and_bounds(par, T, w, h):
    """Every plane at every phase of a 16-byte line, independently: gbuf, fb and fb_out at the four 4-byte phases, edge_out
    at every byte phase. Exact results whichever path the kernel takes, and no byte outside a plane written (run checks
    the guards round all of them). 68 is a multiple of 4: the phases decide between the vector and the per-pixel outputs."""
    params, gbuf, edge, rng = three_class_input(T, w, h, 41)
    fb = O.random_colors(T, rng, w * h)
    exp_fb = O.apply_scale(STYLE, edge, fb)
    style = T.make_outline_style(*STYLE)

    def one(shifts, want=("edge", "fb"), in_place=False):
        got = O.run(par, T, params, style, gbuf, (0, h), fb, (0, h), want, in_place, shifts)
        O.check(got, gbuf, fb, edge, exp_fb, f"{w}x{h} gbuf +{shifts[0]}, fb +{shifts[1]}, fb_out +{shifts[2]}, edge_out "
                                            f"+{shifts[3]}, {want}, in place {in_place}", in_place)

    for g in range(0, 16, 4):
        for f in range(0, 16, 4):
            for o in range(0, 16, 4):
                for e in range(4):
                    one((g, f, o, e))
            one((g, f, f, (g + f) // 4 % 4), in_place=True)
            one((g, f, 0, 0), want=("fb",))
        for e in range(16):
            one((g, 0, 0, e), want=("edge",))
            one((g, 4 * (e % 4), 4 * (e // 4), e))
    # a row block with its halo: the planes of rows (5, 14) at odd phases
    rows, grows = (5, 14), (4, 15)
    for shifts in ((4, 4, 12, 3), (12, 8, 4, 1), (8, 0, 0, 2), (0, 0, 0, 0)):
        run_and_check(par, T, params, STYLE, O.block(gbuf, w, grows), grows, O.block(fb, w, rows), rows,
                      f"{w}x{h} rows {rows} at {shifts}", shifts=shifts)


# ---- 5. in a frame loop ----------------------------------------------------------------------------------------------

def test_in_a_frame_loop(par, oracle, T):
    """The graybox scene under two tinted ranged lights: render_device, outline and quantize on one stream with no host
    wait between; the result equals the models applied to the oracle's planes; two haloed row blocks equal the whole
    frame; the renderer's statistics and a following relit frame are as they are without the calls."""
    import torch
    from test_gpu_light_range import scene
    from test_gpu_light_tints import COLOUR, TINTS, expected
    from test_gpu_lights_graph import Planes
    from test_gpu_parity import ALL, assert_planes_equal
    from test_gpu_relight import LIT, KEPT, expect, relight_in_place, set_state

    sc = scene("graybox", par, oracle, T)
    params = sc.params
    W, H = params.width, params.height
    assert (W, H) == (480, 320)
    which, radii, tints = [3, 6], [200, 300], TINTS[:2]
    lights, exp, _ = expected(T, sc, which, radii, tints, COLOUR, "graybox, two tinted ranged lights")
    style_values = (4, 128, 320)
    style = T.make_outline_style(*style_values)
    edge, outlined = O.model(params, style_values, exp["gbuf"], (0, H), exp["fb"], (0, H))
    counts = np.bincount(edge, minlength=3)
    print(f"graybox: classes {counts}")
    assert (counts > 100).all(), "the frame should hold background, creases and silhouettes"
    assert (outlined.view(np.uint32) != exp["fb"].view(np.uint32)).sum() > 100
    ramp = par.palette_ramp(params, 8)
    index, quantised = Q.model(params, ramp, outlined, None, 32)
    assert (index != Q.model(params, ramp, exp["fb"], None, 32)[0]).any(), "the lines should show in the palette's indices"
    cut = 120  # a bin row: where a sharded frame is cut
    bare = np.concatenate([O.classes(params, style_values, O.block(exp["gbuf"], W, b), b, b) for b in ((0, cut), (cut, H))])
    assert (bare != edge).any(), "without their halo rows the two blocks should differ from the frame"

    d_ramp = torch.from_numpy(ramp.view(np.uint8).copy()).cuda()
    n = W * H
    planes = {k: torch.full((n * b,), O.GUARD, dtype=torch.uint8, device="cuda")
              for k, b in (("edge", 1), ("outlined", 4), ("index", 1), ("quantised", 4), ("edge_blocks", 1), ("fb_blocks", 4))}
    ptr = {k: v.data_ptr() for k, v in planes.items()}
    stream = torch.cuda.Stream()
    out = Planes(params, ALL)
    torch.cuda.synchronize()
    with sc.renderer(par, par.LIGHTS_RANGED) as r, sc.renderer(par, par.LIGHTS_RANGED) as plain:
        for c in (r, plain):
            c.set_lights(lights)
            c.set_light_tints(T.make_tints(tints))
        s = stream.cuda_stream
        r.render_device(out.ptrs, flags=par.RENDER_COUNT_RAYS, stream=s)
        # (no host wait: outline and quantise are ordered behind the frame by the stream alone)
        par.outline(params, style, out.ptrs["gbuf"], (0, H), out.ptrs["fb"], (0, H), fb_out=ptr["outlined"],
                    edge_out=ptr["edge"], stream=s)
        par.quantize(params, d_ramp.data_ptr(), len(ramp), ptr["outlined"], (0, H), fb_out=ptr["quantised"],
                     index_out=ptr["index"], spread=32, stream=s)
        for rows in ((0, cut), (cut, H)):  # two row blocks, each with the G-buffer rows of its halo
            grows = O.halo(rows, H)
            par.outline(params, style, out.ptrs["gbuf"] + 28 * grows[0] * W, grows, out.ptrs["fb"] + 4 * rows[0] * W, rows,
                        fb_out=ptr["fb_blocks"] + 4 * rows[0] * W, edge_out=ptr["edge_blocks"] + rows[0] * W, stream=s)
        stream.synchronize()
        assert_planes_equal(out.host(T), exp, ALL, "the frame itself")
        host = {k: v.cpu().numpy() for k, v in planes.items()}
        assert np.array_equal(host["edge"], edge), "class plane"
        assert host["outlined"].tobytes() == outlined.tobytes(), "outlined frame"
        assert np.array_equal(host["index"], index), "index plane of the outlined frame"
        assert host["quantised"].tobytes() == quantised.tobytes(), "outlined, then quantised"
        assert np.array_equal(host["edge_blocks"], edge), "two haloed row blocks against the whole frame: classes"
        assert host["fb_blocks"].tobytes() == outlined.tobytes(), "two haloed row blocks against the whole frame: colours"

        # the renderer: statistics and the retained frame as without the calls
        plain_out = Planes(params, ALL)
        plain.render_device(plain_out.ptrs, flags=par.RENDER_COUNT_RAYS, stream=s)
        stream.synchronize()
        a, b = r.stats(), plain.stats()
        for field in ("entities", "bin_insertions", "shadow_rays", "occupied_columns", "overflow_columns"):
            assert getattr(a, field) == getattr(b, field), field
        assert a.shadow_rays > 0
        which_b, radii_b, tints_b = [0, 7, 2], [0, 150, 250], TINTS[2:5]
        lights_b, exp_b, _ = expect(T, sc, which_b, radii_b, tints_b, "graybox relit", COLOUR)
        assert exp_b["fb"].tobytes() != exp["fb"].tobytes()
        set_state(par, T, r, lights_b, radii_b, tints_b)
        got = relight_in_place(r, out, stream, T)
        assert_planes_equal(got, exp_b, LIT, "relit after the outline calls")
        assert_planes_equal(got, exp, KEPT, "relit after the outline calls: gbuf and palidx stay")
        # and the relit frame outlined in place, then quantised in place, on its stream
        par.outline(params, style, out.ptrs["gbuf"], (0, H), out.ptrs["fb"], (0, H), fb_out=out.ptrs["fb"], stream=s)
        par.quantize(params, d_ramp.data_ptr(), len(ramp), out.ptrs["fb"], (0, H), fb_out=out.ptrs["fb"], spread=32, stream=s)
        stream.synchronize()
        relit_outlined = O.model(params, style_values, exp["gbuf"], (0, H), exp_b["fb"], (0, H))[1]
        assert out.host(T)["fb"].tobytes() == Q.model(params, ramp, relit_outlined, None, 32)[1].tobytes()
        r.stats()


# ---- 6. host form ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,grows", [(None, None), ((5, 18), (4, 19)), ((5, 18), (5, 18))])
def test_host_form_equals_the_device_path(par, T, rows, grows):
    w, h = 37, 23
    params, gbuf, _, rng = three_class_input(T, w, h, 61)
    fb = O.random_colors(T, rng, w * h)
    r, g = rows or (0, h), grows or rows or (0, h)
    gb, fbb = O.block(gbuf, w, g), O.block(fb, w, r)
    exp_edge, exp_fb = O.model(params, STYLE, gb, g, fbb, r)
    style = T.make_outline_style(*STYLE)
    dev = O.run(par, T, params, style, gb, g, fbb, r)
    keep_g, keep_f = gb.copy(), fbb.copy()
    got = par.outline_host(params, style, gb, fbb, rows=rows, gbuf_rows=grows, planes=("edge", "fb"))
    assert gb.tobytes() == keep_g.tobytes() and fbb.tobytes() == keep_f.tobytes()
    assert got["edge"].tobytes() == dev["edge"].tobytes() == exp_edge.tobytes()
    assert got["fb"].tobytes() == dev["fb"].tobytes() == exp_fb.tobytes()
    only = par.outline_host(params, style, gb, rows=rows, gbuf_rows=grows)
    assert set(only) == {"edge"} and only["edge"].tobytes() == exp_edge.tobytes()
    only = par.outline_host(params, style, gb, fbb, rows=rows, gbuf_rows=grows, planes=("fb",), device=0)
    assert set(only) == {"fb"} and only["fb"].tobytes() == exp_fb.tobytes()
