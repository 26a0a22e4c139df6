"""GPU tests of finish (par_finish_device, par_finish_host): every surface and index plane byte for byte against the
composition of the three passes' contracts restated in numpy (finish.model; tests/test_finish_cpu.py holds it to the three
per-pixel loops without a GPU), the gap bytes of every row and the guard bytes round every plane included, and against
the chain of the three device calls themselves. The shapes are the smallest at which each mechanism of the kernel can go
wrong, not the workload's: a tile is 64 x 16 source pixels.

Each case first asserts on the host that its inputs reach the situation it is named for."""
import ctypes as C

import numpy as np
import pytest

import finish as F
import outline as O
import present as P
import quantize as Q
from test_gpu_quantize import GUARD, Carved

pytestmark = pytest.mark.gpu


def run(par, T, params, desc, rows, fb, style=None, gbuf=None, grows=None, palette=None, spread=0, want_index=True,
        shifts=(0, 0, 0, 0)):
    """One par_finish_device call on carved device planes: (the (rows * sy, pitch) surface block as it is afterwards, gap
    bytes included (they were filled with the guard), the index plane or None), with the guard bytes round every plane
    checked and the inputs unchanged. shifts: BYTES past a 16-byte boundary of gbuf, fb, `out` and index_out."""
    import torch
    r0, r1 = rows or (0, params.height)
    sx, sy, pitch, _ = P._desc(desc)
    n = (r1 - r0) * params.width
    assert len(fb) == n and (style is None) == (gbuf is None)
    g = None if gbuf is None else Carved(28 * len(gbuf), shifts[0], gbuf)
    src = Carved(4 * n, shifts[1], fb)
    out = Carved((r1 - r0) * sy * pitch, shifts[2])
    idx = Carved(n, shifts[3]) if palette is not None and want_index else None
    d_pal = None if palette is None else torch.from_numpy(palette.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    par.finish(params, desc, out.ptr, (r0, r1), src.ptr, style=None if style is None else T.make_outline_style(*style),
               gbuf=g.ptr if g else None, gbuf_rows=grows, d_palette=d_pal.data_ptr() if d_pal is not None else None,
               n_colors=0 if palette is None else len(palette), spread=spread, index_out=idx.ptr if idx else None)
    torch.cuda.synchronize()
    for name, plane in (("gbuf", g), ("fb", src), ("out", out), ("index_out", idx)):
        assert plane is None or plane.guards_intact(), f"{name}: bytes outside the plane were written"
    assert src.host(np.uint8).tobytes() == fb.tobytes(), "fb was written"
    assert g is None or g.host(np.uint8).tobytes() == gbuf.tobytes(), "the G-buffer was written"
    assert d_pal is None or d_pal.cpu().numpy().tobytes() == palette.tobytes(), "the palette was written"
    return out.host(np.uint8).reshape((r1 - r0) * sy, pitch), (idx.host(np.uint8) if idx else None)


def check(got, exp, tag):
    """Byte for byte, the gaps (guard bytes in `exp`) included; the index plane too."""
    (surface, index), (exp_surface, exp_index) = got, exp
    assert surface.shape == exp_surface.shape, tag
    bad = np.argwhere(surface != exp_surface)
    assert len(bad) == 0, f"{tag}: {len(bad)} surface bytes differ, first (row, byte) {bad[:4].tolist()}"
    if exp_index is not None and index is not None:
        bad = np.nonzero(index != exp_index)[0]
        assert len(bad) == 0, f"{tag}: {len(bad)} indices differ, first {bad[:4].tolist()}"


def both(par, T, params, desc, rows, fb, stage, tag, **kw):
    """Run and model of one call with the stages `stage` = (style, gbuf, grows, palette, spread); returns what ran."""
    style, gbuf, grows, palette, spread = stage
    got = run(par, T, params, desc, rows, fb, style, gbuf, grows, palette, spread, **kw)
    check(got, F.model(params, style, gbuf, grows, palette, spread, desc, fb, rows, guard=GUARD), tag)
    return got


# ---- 1. shapes, stages and scales -------------------------------------------------------------------------------------

FRAMES = [(37, 23, (5, 18)), (64, 16, (5, 16)), (130, 35, (5, 18)), (16, 64, (5, 18))]
SCALES = [(1, 1), (2, 2), (3, 3), (5, 2), (1, 3), (7, 16), (16, 16)]
GAPS = [0, 4, 16, 52]


@pytest.mark.parametrize("stage_set", F.STAGE_SETS)
@pytest.mark.parametrize("w,h,rows", FRAMES)
def test_shapes_stages_and_scales(par, T, w, h, rows, stage_set):
    params, gbuf, fb, palette = F.inputs(T, w, h)
    cls = O.classes(params, F.STYLE, gbuf, (0, h), (0, h))
    assert (np.bincount(cls, minlength=3) >= 50).all(), "each class at least 50 times"
    assert len(palette) == 17 and (palette["alpha"] != 0).all() and len(np.unique(palette["alpha"])) > 2
    assert {(4 * w * sx + gap) % 16 == 0 for sx, _ in SCALES for gap in GAPS} == {True, False}, "both 16-byte phases"
    grows = O.halo(rows, h)
    assert grows == (rows[0] - 1, min(h, rows[1] + 1))
    whole_stage = F.stages(stage_set, F.STYLE, gbuf, (0, h), palette, F.SPREAD)
    g, f = F.block_inputs(params, gbuf, fb, rows, grows)
    block_stage = F.stages(stage_set, F.STYLE, g, grows, palette, F.SPREAD)
    # the stages before the present stage do not depend on the desc: their models once
    first = T.make_present_desc(1, 1, 4 * w, P.RGBA)
    exp_index, exp_block_index = (F.model(params, *s, first, b, r)[1]
                                  for s, b, r in ((whole_stage, fb, None), (block_stage, f, rows)))
    if "quantise" in stage_set:
        assert len(np.unique(exp_index)) == 17
        assert np.array_equal(exp_block_index, exp_index[rows[0] * w:rows[1] * w])
    for sx, sy in SCALES:
        for gap in GAPS:
            for order in (P.RGBA, P.BGRA):
                desc = T.make_present_desc(sx, sy, 4 * w * sx + gap, order)
                tag = f"{w}x{h} {stage_set} scale ({sx}, {sy}) gap {gap} order {order}"
                whole, index = both(par, T, params, desc, None, fb, whole_stage, tag)
                part, part_index = both(par, T, params, desc, rows, f, block_stage, f"{tag} rows {rows}")
                assert np.array_equal(part, whole[rows[0] * sy:rows[1] * sy]), f"{tag}: rows {rows} of the whole frame's"
                if index is not None:
                    assert np.array_equal(part_index, index[rows[0] * w:rows[1] * w]), f"{tag}: index rows {rows}"


# ---- 2. equals the chain of the three calls on the device -------------------------------------------------------------

@pytest.mark.parametrize("stage_set", F.STAGE_SETS)
@pytest.mark.parametrize("w,h,sx,sy,order", [(130, 35, 3, 2, P.BGRA), (37, 23, 1, 1, P.RGBA)])
def test_equals_the_chain_on_the_device(par, T, w, h, sx, sy, order, stage_set):
    import torch
    params, gbuf, fb, palette = F.inputs(T, w, h)
    style, g, grows, pal, spread = F.stages(stage_set, F.STYLE, gbuf, (0, h), palette, F.SPREAD)
    desc = T.make_present_desc(sx, sy, 4 * w * sx, order)
    d_g = torch.from_numpy(gbuf.view(np.uint8).copy()).cuda()
    d_fb = torch.from_numpy(fb.view(np.uint8).copy()).cuda()  # outlined in place by the chain
    d_pal = torch.from_numpy(palette.view(np.uint8).copy()).cuda()
    d_index = torch.full((w * h,), GUARD, dtype=torch.uint8, device="cuda")
    d_out = torch.full((h * sy * 4 * w * sx,), GUARD, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    torch.cuda.synchronize()
    if style is not None:
        par.outline(params, T.make_outline_style(*style), d_g.data_ptr(), (0, h), d_fb.data_ptr(), (0, h),
                    fb_out=d_fb.data_ptr(), stream=s)
    if pal is not None:
        par.quantize(params, d_pal.data_ptr(), len(pal), d_fb.data_ptr(), (0, h), index_out=d_index.data_ptr(),
                     spread=spread, stream=s)
        par.present(params, desc, d_out.data_ptr(), (0, h), index=d_index.data_ptr(), d_palette=d_pal.data_ptr(),
                    n_colors=len(pal), stream=s)
    else:
        par.present(params, desc, d_out.data_ptr(), (0, h), fb=d_fb.data_ptr(), stream=s)
    stream.synchronize()
    chain = d_out.cpu().numpy().reshape(h * sy, 4 * w * sx)
    chain_index = d_index.cpu().numpy() if pal is not None else None
    if style is not None:
        assert d_fb.cpu().numpy().tobytes() != fb.tobytes(), "the chain's outline should show"
    got = run(par, T, params, desc, None, fb, style, g, grows, pal, spread)
    check(got, (chain, chain_index), f"{w}x{h} {stage_set}: the chain of the three calls")


# ---- 3. alignment and bounds ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stage_set", F.STAGE_SETS)
def test_alignment_and_bounds(par, T, stage_set):
    """gbuf, fb, `out` with the pitch, and index_out at every phase, independently: exact bytes whichever path the kernel
    takes, and no byte outside a plane or inside a gap written (run checks the guards, check the gaps)."""
    w, h, sx, sy = 37, 23, 3, 2
    params, gbuf, fb, palette = F.inputs(T, w, h)
    stage = F.stages(stage_set, F.STYLE, gbuf, (0, h), palette, F.SPREAD)
    pitches = [4 * w * sx + gap for gap in (4, 8, 12, 0)]
    assert [p % 16 for p in pitches] == [0, 4, 8, 12]
    desc = T.make_present_desc(sx, sy, pitches[0], P.BGRA)
    for gs in ((0, 4, 8, 12) if "outline" in stage_set else (0,)):
        for fs in (0, 4, 8, 12):
            both(par, T, params, desc, None, fb, stage, f"{stage_set}: gbuf +{gs}, fb +{fs}", shifts=(gs, fs, 0, 0))
    for pitch in pitches:
        for order in (P.RGBA, P.BGRA):
            d = T.make_present_desc(sx, sy, pitch, order)
            for o in (0, 4, 8, 12):
                both(par, T, params, d, None, fb, stage, f"{stage_set}: out +{o}, pitch {pitch}, order {order}",
                     shifts=(0, 0, o, 0))
    if "quantise" in stage_set:
        for i in (0, 1, 2, 3):
            both(par, T, params, desc, None, fb, stage, f"{stage_set}: index_out +{i}", shifts=(0, 0, 0, i))
    # a frame whose width is a multiple of 4 takes the index plane's dword stores at shift 0 alone
    w4 = 64
    params4, gbuf4, fb4, _ = F.inputs(T, w4, 16)
    if "quantise" in stage_set:
        stage4 = F.stages(stage_set, F.STYLE, gbuf4, (0, 16), palette, F.SPREAD)
        d4 = T.make_present_desc(sx, sy, 4 * w4 * sx, P.RGBA)
        for i in (0, 1, 2, 3):
            both(par, T, params4, d4, None, fb4, stage4, f"{stage_set}: 64 x 16, index_out +{i}", shifts=(0, 0, 0, i))
    # a block of rows with its halo at odd phases
    rows, grows = (5, 18), (4, 19)
    g, f = F.block_inputs(params, gbuf, fb, rows, grows)
    block_stage = F.stages(stage_set, F.STYLE, g, grows, palette, F.SPREAD)
    for shifts in ((4, 12, 8, 1), (12, 4, 0, 3), (8, 8, 4, 2)):
        both(par, T, params, desc, rows, f, block_stage, f"{stage_set}: rows {rows} at {shifts}", shifts=shifts)


# ---- 4. palettes and dither -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_colors", [1, 2, 17, 33, 256])
def test_palettes_and_dither(par, T, n_colors):
    w, h = 37, 23
    params, gbuf, fb, palette = F.inputs(T, w, h, n_colors=n_colors, seed=42 + n_colors)
    if n_colors == 33:
        palette = par.palette_ramp(params, 8)
    assert len(palette) == n_colors
    outlined = O.model(params, F.STYLE, gbuf, (0, h), fb, (0, h))[1]
    desc = T.make_present_desc(3, 2, 4 * w * 3 + 4, P.BGRA)
    for spread in (0, 32, 255):
        _, raw = Q.dithered(params, outlined, None, spread)
        if spread == 255:
            assert (raw < 0).sum() > 50 and (raw > 255).sum() > 50, "spread 255 clamps at both ends"
        for stage_set in ("outline+quantise", "quantise"):
            stage = F.stages(stage_set, F.STYLE, gbuf, (0, h), palette, spread)
            _, index = both(par, T, params, desc, None, fb, stage, f"n_colors {n_colors} spread {spread} {stage_set}")
            if n_colors == 256:
                assert (index == 255).any(), "a full palette: the largest index is an entry"
            if n_colors > 2 and spread == 32 and stage_set == "quantise":
                plain = Q.model(params, palette, fb, None, 0)[0]
                assert (index != plain).any(), "the dither should show"


# ---- 5. order ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stage_set", ["outline+quantise", "outline"], ids=["palette path", "fb path"])
def test_order_exchanges_red_and_blue_only(par, T, stage_set):
    w, h, sx, sy = 37, 23, 3, 2
    params, gbuf, fb, palette = F.inputs(T, w, h)
    rng = np.random.default_rng(5)
    fb["blue"] = fb["red"] + rng.integers(1, 256, w * h).astype(np.uint8)  # (wraps) never the red value
    palette["blue"] = palette["red"] + rng.integers(1, 256, len(palette)).astype(np.uint8)
    assert (fb["red"] != fb["blue"]).all() and (palette["red"] != palette["blue"]).all()
    stage = F.stages(stage_set, F.STYLE, gbuf, (0, h), palette, F.SPREAD)
    got = {}
    for order in (P.RGBA, P.BGRA):
        desc = T.make_present_desc(sx, sy, 4 * w * sx + 12, order)
        got[order] = both(par, T, params, desc, None, fb, stage, f"{stage_set} order {order}")[0]
    a, b = (got[o][:, :4 * w * sx].reshape(h * sy, w * sx, 4) for o in (P.RGBA, P.BGRA))
    differ = a[..., 0] != a[..., 2]  # (a scaled pixel's red and blue can meet: halved, or clamped to 255)
    assert differ.mean() > 0.9
    assert np.array_equal((a != b).any(axis=2), differ), "the orders differ exactly where red and blue do"
    assert np.array_equal(a[..., 0], b[..., 2]) and np.array_equal(a[..., 2], b[..., 0])
    assert np.array_equal(a[..., 1], b[..., 1]) and np.array_equal(a[..., 3], b[..., 3]), "green and alpha stay"
    if stage_set != "outline":
        assert differ.all(), "every palette entry's red and blue differ"


# ---- 6. halo ----------------------------------------------------------------------------------------------------------

def test_block_without_halo_rows_is_the_model_of_those_rows(par, T):
    """A neighbour row outside the G-buffer rows that were passed is absent, exactly like a row outside the frame."""
    w, h, rows = 37, 23, (5, 18)
    params, gbuf, fb, palette = F.inputs(T, w, h)
    desc = T.make_present_desc(3, 2, 4 * w * 3 + 4, P.RGBA)
    whole = F.model(params, F.STYLE, gbuf, (0, h), palette, F.SPREAD, desc, fb, None, guard=GUARD)
    g, f = F.block_inputs(params, gbuf, fb, rows, rows)
    bare = F.model(params, F.STYLE, g, rows, palette, F.SPREAD, desc, f, rows, guard=GUARD)
    assert (bare[1] != whole[1][rows[0] * w:rows[1] * w]).any(), "without the halo the block differs from the whole frame's"
    assert (bare[0] != whole[0][rows[0] * 2:rows[1] * 2]).any()
    check(run(par, T, params, desc, rows, f, F.STYLE, g, rows, palette, F.SPREAD), bare, "rows (5, 18), gbuf rows (5, 18)")


# ---- 7. several workgroups --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stage_set", F.STAGE_SETS)
@pytest.mark.parametrize("w,h,sx,sy", [(1000, 70, 2, 2), (300, 20, 16, 16)])
def test_several_workgroups(par, T, w, h, sx, sy, stage_set):
    params, gbuf, fb, palette = F.inputs(T, w, h, n_colors=33)
    assert ((w + 63) // 64) * ((h + 15) // 16) >= 10, "several workgroups in both directions"
    stage = F.stages(stage_set, F.STYLE, gbuf, (0, h), palette, F.SPREAD)
    desc = T.make_present_desc(sx, sy, 4 * w * sx, P.BGRA)
    assert int(desc["pitch"][0]) % 16 == 0
    exp = F.model(params, *stage, desc, fb, None, guard=GUARD)
    style, g, grows, pal, spread = stage
    check(run(par, T, params, desc, None, fb, style, g, grows, pal, spread), exp, f"{w}x{h} ({sx}, {sy}) {stage_set}")
    check(run(par, T, params, desc, None, fb, style, g, grows, pal, spread, shifts=(0, 0, 4, 0)), exp,
          f"{w}x{h} ({sx}, {sy}) {stage_set}, out one word past a 16-byte boundary")


# ---- 8. in a frame loop -----------------------------------------------------------------------------------------------

def test_in_a_frame_loop(par, oracle, T):
    """The graybox scene under two tinted ranged lights: render_device, then one finish on one stream with no host wait;
    the surface and the index plane equal the models applied to the oracle's frame; two row blocks cut at row 120, with
    halo rows, written into one surface equal the whole frame's; the frame's planes are left as rendered; the renderer's
    statistics and a following relit frame are as they are without the call."""
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
    ramp = par.palette_ramp(params, 8)
    assert len(ramp) == 33
    desc = T.make_present_desc(3, 3, order=P.BGRA, width=W)
    exp_surface, exp_index = F.model(params, style_values, exp["gbuf"], (0, H), ramp, 32, desc, exp["fb"], None)
    assert exp_surface.shape == (3 * H, 12 * W) and len(np.unique(exp_index)) > 8
    assert (exp_index != Q.model(params, ramp, exp["fb"], None, 32)[0]).sum() > 100, "the lines should show"
    cut = 120  # a bin row: where a sharded frame is cut

    d_ramp = torch.from_numpy(ramp.view(np.uint8).copy()).cuda()
    planes = {k: torch.full((n,), GUARD, dtype=torch.uint8, device="cuda")
              for k, n in (("surface", exp_surface.size), ("index", W * H), ("surface_blocks", exp_surface.size),
                           ("index_blocks", W * H))}
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
        # (no host wait: the call is ordered behind the frame by the stream alone)
        par.finish(params, desc, ptr["surface"], (0, H), out.ptrs["fb"], style=style, gbuf=out.ptrs["gbuf"],
                   d_palette=d_ramp.data_ptr(), n_colors=len(ramp), spread=32, index_out=ptr["index"], stream=s)
        for r0, r1 in ((0, cut), (cut, H)):  # two row blocks with their halo rows into one surface
            g0, g1 = O.halo((r0, r1), H)
            par.finish(params, desc, ptr["surface_blocks"] + r0 * 3 * 12 * W, (r0, r1), out.ptrs["fb"] + 4 * r0 * W,
                       style=style, gbuf=out.ptrs["gbuf"] + 28 * g0 * W, gbuf_rows=(g0, g1), d_palette=d_ramp.data_ptr(),
                       n_colors=len(ramp), spread=32, index_out=ptr["index_blocks"] + r0 * W, stream=s)
        stream.synchronize()
        frame = out.host(T)
        assert_planes_equal(frame, exp, ALL, "the frame itself: finish only reads it")
        host = {k: v.cpu().numpy() for k, v in planes.items()}
        check((host["surface"].reshape(exp_surface.shape), host["index"]), (exp_surface, exp_index), "finish, (3, 3) BGRA")
        check((host["surface_blocks"].reshape(exp_surface.shape), host["index_blocks"]), (exp_surface, exp_index),
              "two row blocks with halo rows")

        # the renderer: statistics and the retained frame as without the call
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
        assert_planes_equal(got, exp_b, LIT, "relit after the finish calls")
        assert_planes_equal(got, exp, KEPT, "relit after the finish calls: gbuf and palidx stay")
        r.stats()


# ---- 9. host form -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [None, (5, 18)])
@pytest.mark.parametrize("stage_set", F.STAGE_SETS)
def test_host_form_equals_the_device_path(par, T, stage_set, rows):
    w, h, sx, sy = 37, 23, 3, 2
    params, gbuf, fb, palette = F.inputs(T, w, h)
    r0, r1 = rows or (0, h)
    grows = O.halo((r0, r1), h)
    g, f = F.block_inputs(params, gbuf, fb, (r0, r1), grows)
    style, g, grows, pal, spread = F.stages(stage_set, F.STYLE, g, grows, palette, F.SPREAD)
    keep = [None if v is None else v.copy() for v in (g, f, pal)]
    for gap in (0, 12):
        desc = T.make_present_desc(sx, sy, 4 * w * sx + gap, P.BGRA)
        exp = F.model(params, style, g, grows, pal, spread, desc, f, rows, guard=GUARD)
        dev = run(par, T, params, desc, rows, f, style, g, grows, pal, spread)
        check(dev, exp, f"device path, gap {gap}")
        kw = dict(rows=rows, style=None if style is None else T.make_outline_style(*style), gbuf=g, gbuf_rows=grows,
                  palette=pal, spread=spread)
        got = par.finish_host(params, desc, f, want_index=pal is not None, **kw)
        surface, index = got if pal is not None else (got, None)
        assert surface.shape == ((r1 - r0) * sy, 4 * w * sx + gap) and surface.dtype == np.uint8
        assert np.array_equal(surface[:, :4 * w * sx], dev[0][:, :4 * w * sx]), f"host form against the device path, gap {gap}"
        assert (surface[:, 4 * w * sx:] == 0).all(), "the binding's zeros in the gap"
        assert pal is None or np.array_equal(index, dev[1])
        if pal is not None:  # and without the index plane
            assert np.array_equal(par.finish_host(params, desc, f, **kw), surface)
        # the C call on an array of the caller's: its gap bytes stay as they are
        mine = np.full(exp[0].shape, GUARD, dtype=np.uint8)
        mine_index = None if pal is None else np.full((r1 - r0) * w, GUARD, dtype=np.uint8)
        g0, g1 = grows or (0, 0)
        rc = par.lib().par_finish_host(C.byref(params), 0, T.ptr(kw["style"]), T.ptr(g), g0, g1, T.ptr(pal),
                                       0 if pal is None else len(pal), spread, T.ptr(desc), T.ptr(f), r0, r1, T.ptr(mine),
                                       T.ptr(mine_index))
        assert rc == 0
        check((mine, mine_index), exp, f"host form, gap {gap}: the model, the gap bytes untouched")
        for v, k in zip((g, f, pal), keep):
            assert v is None or v.tobytes() == k.tobytes(), "an input was written"
