"""GPU tests of present (par_present_device, par_present_host): every surface byte for byte against the contract
restated in numpy (present.model; tests/test_present_cpu.py holds it to a per-pixel loop without a GPU), the gap bytes of
every row and the guard bytes round every plane included. The shapes are the smallest at which each mechanism of the
kernel can go wrong, not the workload's.

Each case first asserts on the host that its inputs reach the situation it is named for.

Shapes of case 1: a frame of 64 x 16 has no rows (5, 18), so its block is rows (5, 16); 16 x 64 and 37 x 23 take rows
(5, 18). Every frame is presented whole as well: a block is compared with those output rows of the whole frame's."""
import ctypes as C

import numpy as np
import pytest

import present as P
from test_gpu_quantize import GUARD, Carved

pytestmark = pytest.mark.gpu


def run(par, T, params, desc, rows, fb=None, index=None, palette=None, shifts=(0, 0)):
    """One par_present_device call on carved device planes: the (rows * sy, pitch) surface block as it is afterwards, gap
    bytes included (they were filled with the guard), with the guard bytes round the source and the surface checked and
    the source and the palette unchanged. shifts: BYTES past a 16-byte boundary of the source and of `out`."""
    import torch
    r0, r1 = rows or (0, params.height)
    sx, sy, pitch, _ = P._desc(desc)
    n = (r1 - r0) * params.width
    source = fb if index is None else index
    assert len(source) == n
    src = Carved(source.itemsize * n, shifts[0], source)
    out = Carved((r1 - r0) * sy * pitch, shifts[1])
    d_pal = None if palette is None else torch.from_numpy(palette.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    if index is None:
        par.present(params, desc, out.ptr, (r0, r1), fb=src.ptr)
    else:
        par.present(params, desc, out.ptr, (r0, r1), index=src.ptr, d_palette=d_pal.data_ptr(), n_colors=len(palette))
    torch.cuda.synchronize()
    assert src.guards_intact(), "bytes outside the source were written"
    assert out.guards_intact(), "bytes outside the surface were written"
    assert src.host(np.uint8).tobytes() == source.tobytes(), "the source was written"
    assert d_pal is None or d_pal.cpu().numpy().tobytes() == palette.tobytes(), "the palette was written"
    return out.host(np.uint8).reshape((r1 - r0) * sy, pitch)


def check(got, exp, tag):
    """Byte for byte, the gaps (guard bytes in `exp`) included."""
    assert got.shape == exp.shape, tag
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, f"{tag}: {len(bad)} bytes differ, first (row, byte) {bad[:4].tolist()}"


def sources(T, rng, n, n_colors=17):
    """A random frame, a random palette of non-zero varied alpha and an index plane that stays inside it."""
    return (P.random_colors(T, rng, n), P.random_colors(T, rng, n_colors, alpha=(1, 255)),
            rng.integers(0, n_colors, n).astype(np.uint8))


def kwargs(source, fb, index, palette, block=None):
    a, b = block or (0, None)
    return dict(fb=fb[a:b]) if source == "fb" else dict(index=index[a:b], palette=palette)


# ---- 1. scales and shapes ---------------------------------------------------------------------------------------------

FRAMES = [(37, 23, (5, 18)), (64, 16, (5, 16)), (16, 64, (5, 18))]
SCALES = [(1, 1), (2, 2), (3, 3), (4, 4), (5, 2), (1, 3), (2, 1), (7, 16), (16, 16)]
GAPS = [0, 4, 16, 52]


@pytest.mark.parametrize("w,h,rows", FRAMES)
def test_scales_and_shapes(par, T, w, h, rows):
    rng = np.random.default_rng(1000 * w + h)
    params = T.default_params(w, h)
    fb, palette, index = sources(T, rng, w * h)
    assert (fb["red"] != fb["blue"]).any() and len(np.unique(index)) == 17
    # what the shapes are chosen for: a row tail for the narrow path, 16-byte groups that begin at every phase of a
    # source pixel, and pitches on and off the 16-byte phase
    assert (37 * 3) % 4 != 0
    for s in (3, 5, 7):
        assert {(4 * g) % s for g in range(16 * s // 4)} == set(range(s))
    wide = {(4 * w * sx + gap) % 16 == 0 for sx, _ in SCALES for gap in GAPS}
    assert wide == {True, False}
    block = (rows[0] * w, rows[1] * w)
    for sx, sy in SCALES:
        for gap in GAPS:
            for order in (P.RGBA, P.BGRA):
                desc = T.make_present_desc(sx, sy, 4 * w * sx + gap, order)
                for source in ("fb", "index"):
                    tag = f"{w}x{h} scale ({sx}, {sy}) gap {gap} order {order} {source}"
                    whole = run(par, T, params, desc, None, **kwargs(source, fb, index, palette))
                    check(whole, P.model(params, desc, None, guard=GUARD, **kwargs(source, fb, index, palette)), tag)
                    part = run(par, T, params, desc, rows, **kwargs(source, fb, index, palette, block))
                    check(part, P.model(params, desc, rows, guard=GUARD, **kwargs(source, fb, index, palette, block)),
                          f"{tag} rows {rows}")
                    assert np.array_equal(part, whole[rows[0] * sy:rows[1] * sy]), f"{tag}: rows {rows} of the whole frame's"


# ---- 2. alignment and bounds ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("source", ["fb", "index"])
def test_alignment_and_bounds(par, T, source):
    """The source, `out` and the pitch at every phase, independently: exact bytes whichever path the kernel takes, and no
    byte outside a plane or inside a gap written (run checks the guards, check the gaps)."""
    rng = np.random.default_rng(2)
    w, h, sx, sy = 37, 23, 3, 2
    params = T.default_params(w, h)
    fb, palette, index = sources(T, rng, w * h)
    kw = kwargs(source, fb, index, palette)
    pitches = [4 * w * sx + gap for gap in (4, 8, 12, 0)]
    assert [p % 16 for p in pitches] == [0, 4, 8, 12]
    source_shifts = (0, 4, 8, 12) if source == "fb" else (0, 1, 2, 3)
    for pitch in pitches:
        for order in (P.RGBA, P.BGRA):
            desc = T.make_present_desc(sx, sy, pitch, order)
            exp = P.model(params, desc, None, guard=GUARD, **kw)
            for s in source_shifts:
                for o in (0, 4, 8, 12):
                    check(run(par, T, params, desc, None, shifts=(s, o), **kw), exp,
                          f"{source} +{s}, out +{o}, pitch {pitch}, order {order}")
    # a block of rows at odd phases
    desc = T.make_present_desc(sx, sy, pitches[0], P.RGBA)
    blk = kwargs(source, fb, index, palette, (5 * w, 18 * w))
    exp = P.model(params, desc, (5, 18), guard=GUARD, **blk)
    for shifts in ((source_shifts[1], 12), (source_shifts[3], 4), (source_shifts[2], 0)):
        check(run(par, T, params, desc, (5, 18), shifts=shifts, **blk), exp, f"{source} rows (5, 18) at {shifts}")


# ---- 3. index source --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_colors", [1, 2, 17, 256])
def test_index_source_clamps_to_the_last_entry(par, T, n_colors):
    rng = np.random.default_rng(30 + n_colors)
    w, h = 37, 23
    params = T.default_params(w, h)
    palette = P.random_colors(T, rng, n_colors, alpha=(1, 255))
    assert (palette["alpha"] != 0).all() and (n_colors < 3 or len(np.unique(palette["alpha"])) > 2)
    index = rng.integers(0, 256, w * h).astype(np.uint8)
    index[rng.choice(w * h, 60, replace=False)] = T.PALIDX_BACKGROUND
    beyond = index >= n_colors
    if n_colors < 256:
        assert beyond.sum() >= 50 and (index[beyond] == T.PALIDX_BACKGROUND).sum() >= 50
    else:
        assert not beyond.any() and (index == 255).sum() >= 50, "a full palette: the largest index is an entry"
    for order in (P.RGBA, P.BGRA):
        for sx, sy, gap in ((3, 2, 0), (4, 1, 12), (1, 1, 4)):
            desc = T.make_present_desc(sx, sy, 4 * w * sx + gap, order)
            exp = P.model(params, desc, None, index=index, palette=palette, guard=GUARD)
            got = run(par, T, params, desc, None, index=index, palette=palette)
            check(got, exp, f"n_colors {n_colors} scale ({sx}, {sy}) order {order}")
            if order == P.RGBA:  # the pixels beyond the palette show its last entry, alpha included
                px = got[::sy, :4 * w * sx].reshape(h, w * sx, 4)[:, ::sx].reshape(-1, 4)
                assert (px[beyond] == palette[-1:].view(np.uint8)).all()


def test_palette_cycling(par, T):
    """The same index plane presented with the palette rotated by one, three times over."""
    rng = np.random.default_rng(34)
    w, h = 37, 23
    params = T.default_params(w, h)
    _, palette, index = sources(T, rng, w * h)
    assert len(np.unique(palette.view(np.uint32))) == len(palette) == 17
    desc = T.make_present_desc(3, 2, 4 * w * 3 + 4, P.BGRA)
    before = run(par, T, params, desc, None, index=index, palette=palette)
    check(before, P.model(params, desc, None, index=index, palette=palette, guard=GUARD), "cycle 0")
    for turn in range(1, 4):
        rotated = np.roll(palette, turn)
        got = run(par, T, params, desc, None, index=index, palette=rotated)
        check(got, P.model(params, desc, None, index=index, palette=rotated, guard=GUARD), f"cycle {turn}")
        assert (got != before).any(), f"cycle {turn} should differ from the one before"
        before = got


# ---- 4. order ---------------------------------------------------------------------------------------------------------

def test_order_exchanges_red_and_blue_only(par, T):
    rng = np.random.default_rng(4)
    w, h, sx, sy = 37, 23, 3, 2
    params = T.default_params(w, h)
    fb = P.random_colors(T, rng, w * h)
    fb["blue"] = fb["red"] + rng.integers(1, 256, w * h).astype(np.uint8)  # (wraps) never the red value
    assert (fb["red"] != fb["blue"]).all() and len(np.unique(fb["alpha"])) > 100
    got = {}
    for order in (P.RGBA, P.BGRA):
        desc = T.make_present_desc(sx, sy, 4 * w * sx + 12, order)
        got[order] = run(par, T, params, desc, None, fb=fb)
        check(got[order], P.model(params, desc, None, fb=fb, guard=GUARD), f"order {order}")
    a, b = (got[o][:, :4 * w * sx].reshape(h * sy, w * sx, 4) for o in (P.RGBA, P.BGRA))
    assert (a.view(np.uint32) != b.view(np.uint32)).all(), "every pixel differs between the orders"
    assert np.array_equal(a[..., 0], b[..., 2]) and np.array_equal(a[..., 2], b[..., 0])
    assert np.array_equal(a[..., 1], b[..., 1]) and np.array_equal(a[..., 3], b[..., 3]), "green and alpha stay"


# ---- 5. the reference's pitched row copy ------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,gap", [(37, 23, 52), (64, 16, 16), (64, 16, 4)])
def test_scale_one_is_a_pitched_row_copy(par, T, w, h, gap):
    """alt:776-780: each source row copied to the start of a surface row `pitch` bytes after the one before."""
    rng = np.random.default_rng(5)
    params = T.default_params(w, h)
    fb = P.random_colors(T, rng, w * h)
    desc = T.make_present_desc(1, 1, 4 * w + gap, P.RGBA)
    assert int(desc["pitch"][0]) > 4 * w
    got = run(par, T, params, desc, None, fb=fb)
    check(got, P.model(params, desc, None, fb=fb, guard=GUARD), f"{w}x{h} gap {gap}")
    assert got[:, :4 * w].tobytes() == fb.tobytes(), "the output rows are the source rows"
    assert (got[:, 4 * w:] == GUARD).all(), "the gaps are intact"


# ---- 6. more than one workgroup ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,sx,sy", [(1000, 70, 2, 2), (300, 20, 16, 16)])
def test_more_than_one_workgroup(par, T, w, h, sx, sy):
    rng = np.random.default_rng(6)
    params = T.default_params(w, h)
    fb, palette, index = sources(T, rng, w * h, 33)
    assert h * ((w * sx + 3) // 4) > 8 * 256, "several workgroups"
    desc = T.make_present_desc(sx, sy, 4 * w * sx, P.BGRA)
    assert int(desc["pitch"][0]) % 16 == 0
    for source in ("fb", "index"):
        kw = kwargs(source, fb, index, palette)
        exp = P.model(params, desc, None, guard=GUARD, **kw)
        check(run(par, T, params, desc, None, **kw), exp, f"{w}x{h} ({sx}, {sy}) {source}")
        check(run(par, T, params, desc, None, shifts=(0, 4), **kw), exp,
              f"{w}x{h} ({sx}, {sy}) {source}, out one word past a 16-byte boundary")


# ---- 7. in a frame loop -----------------------------------------------------------------------------------------------

def test_in_a_frame_loop(par, oracle, T):
    """The graybox scene under two tinted ranged lights: render_device, outline in place, quantize and two presents on
    one stream with no host wait between; the surfaces equal the model applied to the models of the earlier stages; two
    row blocks presented into one surface equal the whole frame's; the renderer's statistics and a following relit frame
    are as they are without the calls."""
    import torch
    import outline as O
    import quantize as Q
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
    assert (outlined.view(np.uint32) != exp["fb"].view(np.uint32)).sum() > 100, "the lines should show"
    ramp = par.palette_ramp(params, 8)
    assert len(ramp) == 33
    index = Q.model(params, ramp, outlined, None, 32)[0]
    assert len(np.unique(index)) > 8
    desc_i = T.make_present_desc(3, 3, order=P.BGRA, width=W)
    desc_f = T.make_present_desc(2, 2, order=P.RGBA, width=W)
    exp_i = P.model(params, desc_i, None, index=index, palette=ramp)
    exp_f = P.model(params, desc_f, None, fb=outlined)
    assert exp_i.shape == (3 * H, 12 * W) and exp_f.shape == (2 * H, 8 * W)
    cut = 120  # a bin row: where a sharded frame is cut

    d_ramp = torch.from_numpy(ramp.view(np.uint8).copy()).cuda()
    planes = {k: torch.full((n,), GUARD, dtype=torch.uint8, device="cuda")
              for k, n in (("index", W * H), ("from_index", exp_i.size), ("from_fb", exp_f.size),
                           ("from_index_blocks", exp_i.size), ("from_fb_blocks", exp_f.size))}
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
        # (no host wait: every later call is ordered behind the frame by the stream alone)
        par.outline(params, style, out.ptrs["gbuf"], (0, H), out.ptrs["fb"], (0, H), fb_out=out.ptrs["fb"], stream=s)
        par.quantize(params, d_ramp.data_ptr(), len(ramp), out.ptrs["fb"], (0, H), index_out=ptr["index"], spread=32, stream=s)
        par.present(params, desc_i, ptr["from_index"], (0, H), index=ptr["index"], d_palette=d_ramp.data_ptr(),
                    n_colors=len(ramp), stream=s)
        par.present(params, desc_f, ptr["from_fb"], (0, H), fb=out.ptrs["fb"], stream=s)
        for r0, r1 in ((0, cut), (cut, H)):  # two row blocks into one surface
            par.present(params, desc_i, ptr["from_index_blocks"] + r0 * 3 * 12 * W, (r0, r1), index=ptr["index"] + r0 * W,
                        d_palette=d_ramp.data_ptr(), n_colors=len(ramp), stream=s)
            par.present(params, desc_f, ptr["from_fb_blocks"] + r0 * 2 * 8 * W, (r0, r1), fb=out.ptrs["fb"] + 4 * r0 * W,
                        stream=s)
        stream.synchronize()
        frame = out.host(T)
        assert_planes_equal(frame, exp, [k for k in ALL if k != "fb"], "the frame itself")
        assert frame["fb"].tobytes() == outlined.tobytes(), "outlined in place"
        host = {k: v.cpu().numpy() for k, v in planes.items()}
        assert np.array_equal(host["index"], index), "index plane of the outlined frame"
        check(host["from_index"].reshape(exp_i.shape), exp_i, "present from the index plane, (3, 3) BGRA")
        check(host["from_fb"].reshape(exp_f.shape), exp_f, "present from fb, (2, 2)")
        check(host["from_index_blocks"].reshape(exp_i.shape), exp_i, "two row blocks from the index plane")
        check(host["from_fb_blocks"].reshape(exp_f.shape), exp_f, "two row blocks from fb")

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
        assert_planes_equal(got, exp_b, LIT, "relit after the present calls")
        assert_planes_equal(got, exp, KEPT, "relit after the present calls: gbuf and palidx stay")
        r.stats()


# ---- 8. host form -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [None, (5, 18)])
@pytest.mark.parametrize("source", ["fb", "index"])
def test_host_form_equals_the_device_path(par, T, source, rows):
    rng = np.random.default_rng(8)
    w, h, sx, sy = 37, 23, 3, 2
    params = T.default_params(w, h)
    r0, r1 = rows or (0, h)
    fb, palette, index = sources(T, rng, (r1 - r0) * w)
    index[:60] = T.PALIDX_BACKGROUND  # beyond the palette
    kw = kwargs(source, fb, index, palette)
    keep = {k: v.copy() for k, v in kw.items()}
    for gap in (0, 12):
        desc = T.make_present_desc(sx, sy, 4 * w * sx + gap, P.BGRA)
        exp = P.model(params, desc, rows, guard=GUARD, **kw)
        dev = run(par, T, params, desc, rows, **kw)
        check(dev, exp, f"device path, gap {gap}")
        got = par.present_host(params, desc, rows=rows, **kw)
        assert got.shape == ((r1 - r0) * sy, 4 * w * sx + gap) and got.dtype == np.uint8
        assert np.array_equal(got[:, :4 * w * sx], dev[:, :4 * w * sx]), f"host form against the device path, gap {gap}"
        assert (got[:, 4 * w * sx:] == 0).all(), "the binding's zeros in the gap"
        # the C call on an array of the caller's: its gap bytes stay as they are
        mine = np.full(exp.shape, GUARD, dtype=np.uint8)
        rc = par.lib().par_present_host(C.byref(params), 0, T.ptr(desc), T.ptr(kw.get("fb")), T.ptr(kw.get("index")),
                                        T.ptr(kw.get("palette")), len(palette) if source == "index" else 0, r0, r1,
                                        T.ptr(mine))
        assert rc == 0
        check(mine, exp, f"host form, gap {gap}: the model, the gap bytes untouched")
        for k, v in kw.items():
            assert v.tobytes() == keep[k].tobytes(), f"{k} was written"
