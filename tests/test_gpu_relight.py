"""GPU tests of relit frames (par_relight_device, par_relight_rows): a frame is rendered once, the lights change, and
the relit fb, brightness and lit planes equal, byte for byte, the full frame of the new lights as the existing composers
give it from the pinned oracle (test_gpu_lights.compose, light_range.compose_ranged, light_tints.compose_tinted), and in
places also a fresh full render in a second context. The gbuf and palidx planes are never written.

Condition on the inputs (tests/test_relight_cpu.py holds it on the oracle's frames without a GPU): a pixel is covered
exactly when its G-buffer texel differs from the background texel. The composers' own conditions (LT.conditions,
relied_on) are asserted on the expected frames as test_gpu_light_tints.py and test_gpu_light_range.py do."""
import numpy as np
import pytest

import light_range as LR
import light_tints as LT
from helpers import LIGHT_KEYS, apply_key
from test_gpu_light_range import Scene, relied_on, scene
from test_gpu_light_tints import BLACK, COLOUR, EVERY, TINTS, model_of
from test_gpu_lights import compose, expected as composed, lights_of
from test_gpu_lights_edges import (MANY_BINS_LIGHTS, MIXED_STAGE_LIGHTS, background_bytes, host_path_scene,
                                   many_bins_scene, mixed_stage_scene)
from test_gpu_lights_graph import BYTES, Planes
from test_gpu_parity import ALL, assert_planes_equal

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_NOT_READY = 1, 8
LIT = ("fb", "brightness", "lit")   # what a relit frame writes
KEPT = ("gbuf", "palidx")           # what it leaves alone


@pytest.fixture(scope="module")
def sprite(par):
    return par.tile_floor()


def status(par, fn, *args, **kw):
    with pytest.raises(par.ParError) as e:
        fn(*args, **kw)
    return e.value.status


def expect(T, sc, which, radii, tints, tag, need=(), rely=()):
    """(lights, expected planes, shadow rays) of lights `which` of the scene's pool, by the composer of the case's kind;
    the composer's conditions on the expected frame asserted: `need` (tinted), `rely` (ranged lights with all three
    classes of covered pixels)."""
    lights, outs = sc.pick(T, which, radii or [10] * len(which))
    if tints is not None:
        exp, info = LT.compose_tinted(sc.params, outs, lights, tints, ranged=radii is not None)
        black = BLACK if len(which) > BLACK and all(v == 0 for v in info["tints"][BLACK]) else None
        cond = LT.conditions(exp, info, lights, black)
        print(f"{tag}: {cond}")
        for k in need:
            assert cond[k] > 0, f"{tag}: the expected frame must show '{k}', has {cond}"
        rays = info["rays"]
    elif radii is not None:
        exp, per_light, _, rays = LR.compose_ranged(sc.params, outs, lights)
        relied_on(per_light, lights, rely, None, tag)
    else:
        exp, per_light = compose(sc.params, outs, lights)
        for l, v in enumerate(per_light):
            assert v.any() and not v.all(), f"{tag}: light {l} should reach some covered pixels and not others"
        rays = len(which) * int((exp["palidx"] != 0xFF).sum())
    return lights, exp, rays


def set_state(par, T, r, lights, radii, tints):
    r.set_light_model(model_of(par, radii))
    r.set_light_tints(None if tints is None else T.make_tints(tints))
    r.set_lights(lights)


def rows_of(planes, params, rows, keys):
    r0, r1 = rows or (0, params.height)
    W = params.width
    return {k: planes[k][r0 * W:r1 * W] for k in keys}


def relight_in_place(r, out, stream, T, planes=LIT, flags=0):
    """A relit frame over the device planes `out` of the retained frame, on its stream; their host copies."""
    r.relight_device(out.ptrs["gbuf"], {k: out.ptrs[k] for k in planes}, rows=(out.r0, out.r1), flags=flags,
                     stream=stream.cuda_stream)
    stream.synchronize()
    return out.host(T)


# ---- 1. every light state ---------------------------------------------------------------------------------------

# scene: lights A of the retained frame, then (tag, lights B, radii, tints, tinted conditions, ranged lights relied on)
STATES = {
    "graybox": ([5, 2], [
        ("n=1", [0], None, None, (), ()),
        ("n=2", [0, 3], None, None, (), ()),
        ("n=4 a sun beside torches", [0, 3, 6, 7], [0, 200, 300, 150], None, (), (1, 2)),
        ("n=4 tinted", [0, 3, 6, 7], None, TINTS[:4], EVERY, ()),
        ("n=8 ranged and tinted", [0, 3, 6, 7, 1, 2, 4, 5], [0, 200, 300, 150, 300, 90, 60, 0], TINTS, EVERY, ()),
        ("n=8", [0, 3, 6, 7, 1, 2, 4, 5], None, None, (), ()),
    ]),
    "random0": ([7, 4, 3], [
        ("n=2 ranged", [0, 1], [250, 200], None, (), (0, 1)),
        ("n=4 tinted", [0, 1, 2, 6], None, TINTS[:4], EVERY, ()),
        ("n=1 tinted", [2], None, TINTS[:1], COLOUR, ()),
    ]),
    "random7": ([5], [
        ("n=1 ranged and tinted", [0], [300], TINTS[:1], COLOUR, ()),
        ("n=4 a sun beside torches, tinted", [0, 1, 2, 6], [0, 200, 300, 150], TINTS[:4], EVERY, ()),
        ("n=8 ranged", [0, 1, 2, 6, 3, 4, 5, 7], [0, 200, 300, 150, 60, 300, 90, 0], None, (), (1, 2)),
        ("n=2", [1, 6], None, None, (), ()),
    ]),
}


@pytest.mark.parametrize("name", list(STATES))
def test_every_light_state(par, oracle, T, name):
    import torch
    sc = scene(name, par, oracle, T)
    first, cases = STATES[name]
    lights_a, exp_a, _ = expect(T, sc, first, None, None, f"{name} retained frame")
    stream = torch.cuda.Stream()
    out = Planes(sc.params, ALL)
    with sc.renderer(par) as r:
        r.set_lights(lights_a)
        r.render_device(out.ptrs, stream=stream.cuda_stream)
        stream.synchronize()
        assert_planes_equal(out.host(T), exp_a, ALL, f"{name}: the retained frame")
        for tag, which, radii, tints, need, rely in cases:
            tag = f"{name} {tag}"
            lights, exp, _ = expect(T, sc, which, radii, tints, tag, need, rely)
            assert exp["fb"].tobytes() != exp_a["fb"].tobytes(), f"{tag}: the new lights should show"
            set_state(par, T, r, lights, radii, tints)
            for k in range(3):  # (the atomics' order decides the walk area's layout)
                got = relight_in_place(r, out, stream, T)
                assert_planes_equal(got, exp, LIT, f"{tag}, relit frame {k}")
                assert_planes_equal(got, exp_a, KEPT, f"{tag}, relit frame {k}: gbuf and palidx stay")
        r.stats()


# ---- 2. one white unbounded light: the retained frame comes from the one-light production path -------------------

KEY_SCRIPT = "okuohjak"  # eight of the reference's light keys (alt:641-681)
GOLDEN_WITH_PRIMITIVES = ["uniform64", "uniform256", "uniform1024", "floor600", "floor600_lowlight", "clump200", "edges300",
                          "uniform512_axis_light", "floor500_light_in_floor", "single"]


@pytest.mark.parametrize("name", GOLDEN_WITH_PRIMITIVES)
def test_one_white_light_walks_the_key_script(par, oracle, golden_frames, sprite, T, name):
    import torch
    assert all(k in LIGHT_KEYS for k in KEY_SCRIPT)
    assert set(GOLDEN_WITH_PRIMITIVES) == {k for k, (_, a, _) in golden_frames.items() if len(a)}
    params = T.default_params()
    _, aabbs, light = golden_frames[name]
    light = light.copy()
    stream = torch.cuda.Stream()
    out = Planes(params, ALL)
    with par.Renderer(params) as r:
        r.set_sprites(sprite)
        r.set_entities(aabbs)
        r.set_light(light)
        r.render_device(out.ptrs, stream=stream.cuda_stream)  # (no hook: the production path)
        stream.synchronize()
        first = oracle.render(params, aabbs, sprite, light)
        assert_planes_equal(out.host(T), first, ALL, f"{name}: the retained frame")
        for step, key in enumerate(KEY_SCRIPT):
            apply_key(key, aabbs, light)
            r.set_light(light)
            exp = oracle.render(params, aabbs, sprite, light, planes=LIT)
            got = relight_in_place(r, out, stream, T)
            assert_planes_equal(got, exp, LIT, f"{name} step {step} key {key}")
            assert_planes_equal(got, first, KEPT, f"{name} step {step}: gbuf and palidx stay")
        r.stats()


# ---- 3. the limits of phases A and B in the relight form ---------------------------------------------------------

def relit_after_the_lights_moved(par, T, sc, first, which, radii, tints, tag):
    import torch
    lights_a, exp_a, _ = expect(T, sc, first, None, None, f"{tag} retained frame")
    lights, exp, _ = expect(T, sc, which, radii, tints, tag, COLOUR if tints else ())
    stream = torch.cuda.Stream()
    out = Planes(sc.params, ALL)
    with sc.renderer(par) as r:
        r.set_lights(lights_a)
        r.render_device(out.ptrs, stream=stream.cuda_stream)
        stream.synchronize()
        assert_planes_equal(out.host(T), exp_a, ALL, f"{tag}: the retained frame")
        set_state(par, T, r, lights, radii, tints)
        for k in range(3):
            got = relight_in_place(r, out, stream, T)
            assert_planes_equal(got, exp, LIT, f"{tag}, relit frame {k}")
            assert_planes_equal(got, exp_a, KEPT, f"{tag}, relit frame {k}: gbuf and palidx stay")
        r.stats()


@pytest.mark.parametrize("radii,tints", [(None, None), ([500, 0, 300, 250], TINTS[:4])])
def test_limit_mixed_stage(par, oracle, T, radii, tints):
    """A start bin whose walk is recorded towards one light and too long for a stage towards another (the scene and
    its proof: test_gpu_lights_edges.test_mixed_stage_fits_within_one_start_bin): per-lane walks in the relight form."""
    params, aabbs = mixed_stage_scene(T)
    sc = Scene(par, oracle, T, params, aabbs, MIXED_STAGE_LIGHTS)
    relit_after_the_lights_moved(par, T, sc, [4, 5, 6, 7], [0, 1, 2, 3], radii, tints, f"mixed stage {radii}")


def test_limit_more_than_64_occupied_bins(par, oracle, T):
    """A column with 80 occupied bins (test_more_than_64_occupied_bins_in_a_column): walks that are not recorded."""
    params, aabbs = many_bins_scene(T)
    sc = Scene(par, oracle, T, params, aabbs, MANY_BINS_LIGHTS[:6])
    relit_after_the_lights_moved(par, T, sc, [4, 5], [0, 1, 2, 3], None, None, "many bins")


def test_limit_1024_view(par, oracle, T):
    sc = scene("syn1024", par, oracle, T)
    relit_after_the_lights_moved(par, T, sc, [2, 1], [3, 0, 1, 2], [0, 900, 700, 900], TINTS[:4], "syn1024 a sun beside torches")


# ---- 4. rows and planes ------------------------------------------------------------------------------------------

def test_rows_and_planes(par, oracle, sprite, T):
    import torch
    params, aabbs, pos = host_path_scene(par, oracle, sprite, T, "graybox", 3)
    W = params.width
    lights = lights_of(T, pos)
    exp, _ = composed(params, oracle, aabbs, sprite, lights, tag="rows and planes")
    bg = background_bytes(exp)
    print(f"background bytes of the expected lit plane {[int(b) for b in bg]}")
    assert len(bg[bg != 0]) >= 2, f"a misplaced background bit needs two different non-zero bytes: {bg}"
    lights_a = lights_of(T, [(480, 160, 80), (20, 300, 10)])
    kept_rows = (40, 200)
    stream = torch.cuda.Stream()
    kept = Planes(params, ALL, kept_rows)
    with par.Renderer(params) as r:
        r.set_sprites(sprite)
        r.set_entities(aabbs)
        r.set_lights(lights_a)
        r.render_device(kept.ptrs, rows=kept_rows, stream=stream.cuda_stream)
        stream.synchronize()
        before = kept.host(T)
        r.set_lights(lights)
        for rows in ((80, 160), kept_rows):
            gbuf = kept.ptrs["gbuf"] + (rows[0] - kept_rows[0]) * W * BYTES["gbuf"]
            for planes, flags in [(LIT, 0), (("fb",), 0), (("lit",), 0), (("brightness",), 0),
                                  (("fb", "brightness"), par.RENDER_TRACE_BACKGROUND)]:
                out = Planes(params, planes, rows)
                for k in range(2):
                    r.relight_device(gbuf, out.ptrs, rows=rows, flags=flags, stream=stream.cuda_stream)
                    stream.synchronize()
                    assert_planes_equal(out.host(T), rows_of(exp, params, rows, planes), planes,
                                        f"rows {rows} planes {planes} flags {flags}, relit frame {k}")
        assert_planes_equal(kept.host(T), before, ALL, "the retained frame's planes were only read")
        r.stats()


# ---- 5. counts ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [None, (80, 160)])
def test_counted_rays_and_pairs(par, oracle, T, rows):
    import torch
    sc = scene("graybox", par, oracle, T)
    which, radii = [0, 3, 6, 7], [0, 200, 300, 150]
    lights, exp, rays = expect(T, sc, which, radii, None, "counts, ranged", rely=(1, 2))
    plain_lights, plain, plain_rays = expect(T, sc, which, None, None, "counts, unbounded")
    W = sc.params.width
    if rows:  # the rays of the rows alone
        idx = np.nonzero(exp["palidx"] != 0xFF)[0]
        in_rows = (idx >= rows[0] * W) & (idx < rows[1] * W)
        _, per_light, _, _ = LR.compose_ranged(sc.params, sc.pick(T, which, radii)[1], lights)
        rays = sum(int((p[0] & in_rows).sum()) for p in per_light)
        plain_rays = len(which) * int(in_rows.sum())
    stream = torch.cuda.Stream()
    out = Planes(sc.params, ALL)
    with sc.renderer(par, par.LIGHTS_RANGED) as full:
        full.set_lights(lights)
        want = full.render(LIT, rows=rows, flags=par.RENDER_COUNT_RAYS)
        assert full.stats().shadow_rays == rays, "the full frame's own count"
        walks = full.light_walks()
    assert walks[0] > 0 and walks[1] > 0, f"pairs walked and culled {walks}"
    with sc.renderer(par) as r:
        r.set_lights(lights_of(T, [sc.positions[5]]))
        r.render_device(out.ptrs, stream=stream.cuda_stream)
        stream.synchronize()
        gbuf = out.ptrs["gbuf"] + (rows[0] if rows else 0) * W * BYTES["gbuf"]
        relit = Planes(sc.params, LIT, rows)
        r.set_light_model(par.LIGHTS_RANGED)
        r.set_lights(lights)
        for k in range(2):
            r.relight_device(gbuf, relit.ptrs, rows=rows, flags=par.RENDER_COUNT_RAYS, stream=stream.cuda_stream)
            stream.synchronize()
            assert_planes_equal(relit.host(T), want, LIT, f"ranged rows {rows}, relit frame {k}")
            assert r.stats().shadow_rays == rays, f"rows {rows}: shadow_rays of a ranged relit frame"
            assert r.light_walks() == walks, f"rows {rows}: pairs walked and culled"
        r.set_light_model(par.LIGHTS_UNBOUNDED)
        r.set_lights(plain_lights)
        r.relight_device(gbuf, relit.ptrs, rows=rows, flags=par.RENDER_COUNT_RAYS, stream=stream.cuda_stream)
        stream.synchronize()
        assert_planes_equal(relit.host(T), rows_of(plain, sc.params, rows, LIT), LIT, f"unbounded rows {rows}")
        assert r.stats().shadow_rays == plain_rays, f"rows {rows}: shadow_rays of an unbounded relit frame"
        r.relight_device(gbuf, relit.ptrs, rows=rows, stream=stream.cuda_stream)
        assert r.stats().shadow_rays == -1 and r.light_walks() == (-1, -1), "an uncounted relit frame"


# ---- 6. state ----------------------------------------------------------------------------------------------------

def test_state_around_relit_frames(par, oracle, T):
    import torch
    sc = scene("random7", par, oracle, T)
    lights_a, exp_a, _ = expect(T, sc, [5, 3], None, None, "state, retained frame")
    stream = torch.cuda.Stream()
    out = Planes(sc.params, ALL)
    with sc.renderer(par) as r:
        r.set_lights(lights_a)
        r.render_device(out.ptrs, stream=stream.cuda_stream)
        stream.synchronize()
        st = r.stats()
        kept_stats = (st.entities, st.bin_insertions, st.occupied_columns)
        assert st.bin_insertions > 0 and st.occupied_columns > 0
        grid = r.read_grid()
        # relit frames follow one another through set_lights, set_light_model and set_light_tints
        for tag, which, radii, tints, need in [("lights", [0, 1], None, None, ()),
                                               ("model", [0, 1, 2, 6], [0, 200, 300, 150], None, ()),
                                               ("tints", [0, 1, 2, 6], [0, 200, 300, 150], TINTS[:4], EVERY),
                                               ("untinted, unbounded again", [1, 6], None, None, ())]:
            lights, exp, _ = expect(T, sc, which, radii, tints, f"state, {tag}", need)
            set_state(par, T, r, lights, radii, tints)
            got = relight_in_place(r, out, stream, T)
            assert_planes_equal(got, exp, LIT, f"relit frame after a change of {tag}")
            assert_planes_equal(got, exp_a, KEPT, f"{tag}: gbuf and palidx stay")
            st = r.stats()
            assert (st.entities, st.bin_insertions, st.occupied_columns) == kept_stats, f"{tag}: stats of the retained frame"
            for a, b in zip(r.read_grid(), grid):
                assert a.tobytes() == b.tobytes(), f"{tag}: read_grid changed"
        # a full render after relit frames, and relit frames after it
        full = Planes(sc.params, ALL)
        r.render_device(full.ptrs, stream=stream.cuda_stream)
        stream.synchronize()
        assert_planes_equal(full.host(T), exp, ALL, "a full render after relit frames")
        r.set_lights(lights_a)
        assert_planes_equal(relight_in_place(r, full, stream, T), exp_a, ALL, "a relit frame of the new retained frame")
        assert_planes_equal(r.render(ALL), exp_a, ALL, "a host render after relit frames")
        r.stats()


# ---- 7. refusals -------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(par, oracle, T):
    import ctypes as C
    import torch
    sc = scene("graybox", par, oracle, T)
    lights, exp, _ = expect(T, sc, [0, 3], None, None, "refusals")
    one, exp_one, _ = expect(T, sc, [0], None, None, "refusals, one light")
    stream = torch.cuda.Stream()
    out, relit = Planes(sc.params, ALL), Planes(sc.params, LIT)
    h = sc.params.height

    def relight(r, rows=None, flags=0, gbuf=None, ptrs=None):
        r.relight_device(out.ptrs["gbuf"] if gbuf is None else gbuf, relit.ptrs if ptrs is None else ptrs, rows=rows,
                         flags=flags, stream=stream.cuda_stream)

    def full_render_is_right(r, want, tag):
        r.render_device(out.ptrs, stream=stream.cuda_stream)
        stream.synchronize()
        assert_planes_equal(out.host(T), want, ALL, f"a full render after the refusal: {tag}")

    with par.Renderer(sc.params) as r:  # before sprites, entities, a light, and before any frame
        assert status(par, relight, r) == ERR_NOT_READY
        r.set_sprites(sc.sprite)
        assert status(par, relight, r) == ERR_NOT_READY
        r.set_entities(sc.aabbs)
        assert status(par, relight, r) == ERR_NOT_READY
        r.set_lights(lights)
        assert status(par, relight, r) == ERR_NOT_READY
        assert "retained" in par.lib().par_last_error(r._ctx).decode()
        assert status(par, r.relight) == ERR_NOT_READY
        full_render_is_right(r, exp, "no frame yet")
        relight(r)  # (now there is one)
        stream.synchronize()
        assert_planes_equal(relit.host(T), exp, LIT, "a relit frame of the same lights")
        # what ends the retained frame
        enders = [("update_aabbs", lambda: r.update_aabbs(sc.aabbs[0:1], 0)),
                  ("update_aabbs(stream)", lambda: r.update_aabbs(sc.aabbs[0:1], 0, stream=stream.cuda_stream)),
                  ("set_entities", lambda: r.set_entities(sc.aabbs)),
                  ("set_sprites", lambda: r.set_sprites(sc.sprite))]
        for tag, end in enders:
            end()
            assert status(par, relight, r) == ERR_NOT_READY, tag
            full_render_is_right(r, exp, tag)
            relight(r)
        # rows outside the retained ones
        r.render_device(out.ptrs, rows=(40, 200), stream=stream.cuda_stream)
        for rows in ((0, 200), (40, 201), (0, h), (200, 240), (0, 40)):
            assert status(par, relight, r, rows) == ERR_NOT_READY, rows
        relight(r, (40, 200))
        relight(r, (80, 120))
        full_render_is_right(r, exp, "rows outside the retained ones")
        # arguments: INVALID_ARG comes before NOT_READY and leaves the retained frame
        L = par.lib()
        o = T.Outputs(*[relit.ptrs.get(k) for k in ALL])
        assert L.par_relight_device(r._ctx, stream.cuda_stream, 0, h, None, C.byref(o), 0) == ERR_INVALID_ARG
        assert L.par_relight_device(r._ctx, stream.cuda_stream, 0, h, out.ptrs["gbuf"], None, 0) == ERR_INVALID_ARG
        assert L.par_relight_rows(r._ctx, 0, h, None, 0) == ERR_INVALID_ARG
        for k in KEPT:
            assert status(par, relight, r, ptrs=dict(relit.ptrs, **{k: out.ptrs[k]})) == ERR_INVALID_ARG, k
        assert status(par, relight, r, flags=1 << 7) == ERR_INVALID_ARG
        assert status(par, r.relight, flags=1 << 7) == ERR_INVALID_ARG
        for rows in ((-1, 10), (10, 10), (20, 10), (0, h + 1)):
            assert status(par, relight, r, rows) == ERR_INVALID_ARG, rows
        assert status(par, r.relight, rows=(0, h + 1)) == ERR_INVALID_ARG
        relight(r, flags=par.RENDER_PIPELINED | par.RENDER_TIMED_AS_LAUNCHED)  # (accepted, and the frame is still there)
        stream.synchronize()
        assert_planes_equal(relit.host(T), exp, LIT, "a relit frame after the refused calls")
        # the host call needs a host frame with a gbuf plane
        assert status(par, r.relight) == ERR_NOT_READY  # (the retained frame is a device frame)
        assert_planes_equal(r.render(("fb",)), exp, ("fb",), "render(fb)")
        assert status(par, r.relight) == ERR_NOT_READY
        assert "gbuf" in par.lib().par_last_error(r._ctx).decode()
        r.render(ALL)
        assert_planes_equal(r.relight(LIT), exp, LIT, "relight() after render(ALL)")
        r.pick(240, 160)
        assert status(par, r.relight, rows=(160, 161)) == ERR_NOT_READY  # (par_pick's row is for par_relight_device)
        full_render_is_right(r, exp, "the host call")
        # graphs (one light: par_graph_capture)
        r.set_lights(one)
        r.graph_capture(out.ptrs, stream=stream.cuda_stream)
        assert status(par, relight, r) == ERR_NOT_READY, "graph capture"
        full_render_is_right(r, exp_one, "graph capture")
        relight(r)
        r.graph_launch(stream.cuda_stream)
        assert status(par, relight, r) == ERR_NOT_READY, "graph launch"
        full_render_is_right(r, exp_one, "graph launch")
        relight(r)
        r.graph_stage(light=one)
        assert status(par, relight, r) == ERR_NOT_READY, "graph stage"
        full_render_is_right(r, exp_one, "graph stage")
        r.stats()


# ---- 8. the host path --------------------------------------------------------------------------------------------

def test_host_path(par, oracle, T):
    sc = scene("random0", par, oracle, T)
    lights_a, exp_a, _ = expect(T, sc, [7, 4], None, None, "host path, retained frame")
    which, radii = [0, 1, 2, 6], [0, 200, 300, 150]
    lights, exp, rays = expect(T, sc, which, radii, TINTS[:4], "host path", EVERY)
    with sc.renderer(par) as r:
        r.set_lights(lights_a)
        assert_planes_equal(r.render(ALL), exp_a, ALL, "the retained frame")
        set_state(par, T, r, lights, radii, TINTS[:4])
        for k in range(2):
            assert_planes_equal(r.relight(LIT), exp, LIT, f"relight(), frame {k}")
        assert_planes_equal(r.relight(LIT, flags=par.RENDER_COUNT_RAYS), exp, LIT, "relight(), counted")
        assert r.stats().shadow_rays == rays
        for rows, planes in [((37, 251), LIT), ((0, 40), ("fb",)), ((120, 320), ("brightness",)), ((5, 300), ("fb", "lit"))]:
            assert_planes_equal(r.relight(planes, rows=rows), rows_of(exp, sc.params, rows, planes), planes,
                                f"relight() rows {rows} planes {planes}")
        # a host frame of some rows: relit rows inside them
        r.set_lights(lights_a)
        r.set_light_model(par.LIGHTS_UNBOUNDED)
        r.set_light_tints(None)
        assert_planes_equal(r.render(ALL, rows=(40, 200)), rows_of(exp_a, sc.params, (40, 200), ALL), ALL, "rows 40-200")
        set_state(par, T, r, lights, radii, TINTS[:4])
        for rows in ((40, 200), (81, 159)):
            assert_planes_equal(r.relight(LIT, rows=rows), rows_of(exp, sc.params, rows, LIT), LIT, f"relit rows {rows}")
        assert status(par, r.relight, rows=(0, 200)) == ERR_NOT_READY
        assert_planes_equal(r.render(ALL), exp, ALL, "a full render after the relit frames")
        r.stats()
