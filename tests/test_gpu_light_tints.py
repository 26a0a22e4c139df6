"""GPU parity of tinted lights (par_set_light_tints): every plane byte for byte against the frame composed from the
pinned oracle by light_tints.compose_tinted (the composers of test_gpu_lights and light_range extended by the contract
beside par_set_light_tints; tests/test_light_tints_cpu.py pins that composer without a GPU), the ray count, and what the
tints must not touch.

Conditions on the inputs, asserted on the host before anything is rendered (LT.conditions): the expected frame shows
covered pixels with red != green and with green != blue, pixels with one channel's factor clamped at 1 and another below
1, pixels where at least two non-black lights add a positive term, and covered pixels with the black light's lit bit.
A frame of one light cannot have two lights adding, and the frames of one and two lights here have no black light: each
case names the conditions it must meet (NEED), all of them for the frames of four and eight lights."""
import numpy as np
import pytest

import light_tints as LT
from test_gpu_light_range import Scene, lights_with, scene
from test_gpu_lights_edges import MANY_BINS_LIGHTS, MIXED_STAGE_LIGHTS, many_bins_scene, mixed_stage_scene
from test_gpu_lights_graph import Planes, replay
from test_gpu_parity import ALL, assert_planes_equal

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_NOT_READY = 1, 5, 8

# a zero component, fractions, components above 1, one black light (index 3)
TINTS = [(1, .25, 0), (0, .5, 1.5), (2, 2, 2), (0, 0, 0), (.5, 1, .25), (1.5, 0, .75), (.125, .125, 1), (3, .5, 0)]
BLACK = 3
COLOUR = ("r!=g", "g!=b")
EVERY = COLOUR + ("clamped in some, not all", "two adding", "black lit")

# name: (scene, lights of the scene's pool, radii (None: PAR_LIGHTS_UNBOUNDED), conditions the frame must meet)
CASES = {
    "graybox n=1": ("graybox", [0], None, COLOUR),
    "graybox n=2": ("graybox", [0, 3], None, COLOUR + ("clamped in some, not all", "two adding")),
    "graybox n=4": ("graybox", [0, 3, 6, 7], None, EVERY),
    "graybox n=4 a sun beside torches": ("graybox", [0, 3, 6, 7], [0, 200, 300, 150], EVERY),
    "graybox n=8 ranged": ("graybox", [0, 3, 6, 7, 1, 2, 4, 5], [0, 200, 300, 150, 300, 90, 60, 0], EVERY),
    "graybox n=8": ("graybox", [0, 3, 6, 7, 1, 2, 4, 5], None, EVERY),
    "random0 n=2 ranged": ("random0", [0, 1], [250, 200], COLOUR + ("two adding",)),
    "random0 n=4": ("random0", [0, 1, 2, 6], None, EVERY),
    "random7 n=1 ranged": ("random7", [0], [300], COLOUR),
    "random7 n=4 a sun beside torches": ("random7", [0, 1, 2, 6], [0, 200, 300, 150], EVERY),
    "random7 n=8 ranged": ("random7", [0, 1, 2, 6, 3, 4, 5, 7], [0, 200, 300, 150, 60, 300, 90, 0], EVERY),
    "syn1024 n=2": ("syn1024", [0, 1], None, COLOUR + ("two adding",)),
    "syn1024 n=4 a sun beside torches": ("syn1024", [3, 0, 1, 2], [0, 900, 700, 900], EVERY),
}


def model_of(par, radii):
    return par.LIGHTS_UNBOUNDED if radii is None else par.LIGHTS_RANGED


def expected(T, sc, which, radii, tints, need, tag):
    """(lights, expected planes, composer's info) of a case, its conditions asserted."""
    lights, outs = sc.pick(T, which, radii or [10] * len(which))
    exp, info = LT.compose_tinted(sc.params, outs, lights, tints, ranged=radii is not None)
    black = BLACK if len(which) > BLACK and all(v == 0 for v in info["tints"][BLACK]) else None
    cond = LT.conditions(exp, info, lights, black)
    print(f"{tag}: {cond}")
    for k in need:
        assert cond[k] > 0, f"{tag}: the expected frame must show '{k}', has {cond}"
    return lights, exp, info


def rows_of(planes, params, rows, keys):
    r0, r1 = rows or (0, params.height)
    W = params.width
    return {k: planes[k][r0 * W:r1 * W] for k in keys}


# ---- 1. white tints: the untinted frame ------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_white_tints_give_the_untinted_frame(par, oracle, T, n):
    sc = scene("graybox", par, oracle, T)
    which = [0, 3, 6, 7, 1, 2, 4, 5][:n]
    for radii in (None, [0, 200, 300, 150, 300, 90, 60, 0][:n]):
        lights, _ = sc.pick(T, which, radii or [10] * n)
        with sc.renderer(par, model_of(par, radii)) as r:
            r.set_lights(lights)  # (n = 1, unbounded: the one-light production path, no hook; tinted, the light kernel)
            plain = r.render(ALL, flags=par.RENDER_COUNT_RAYS)
            rays = r.stats().shadow_rays
            for tints in ([LT.WHITE] * n, [LT.WHITE], [LT.WHITE] * 8):
                r.set_light_tints(T.make_tints(tints))
                for k in range(3):
                    got = r.render(ALL, flags=par.RENDER_COUNT_RAYS)
                    assert_planes_equal(got, plain, ALL, f"n={n} radii {radii}: white tints {len(tints)}, render {k}")
                    if n > 1 or radii:  # (the one-light production path counts its rays in its own way)
                        assert r.stats().shadow_rays == rays
            r.set_light_tints(None)
            assert_planes_equal(r.render(ALL), plain, ALL, f"n={n} radii {radii}: untinted again")


# ---- 2. tinted frames against the composed oracle --------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_tinted_frame(par, oracle, T, name):
    sname, which, radii, need = CASES[name]
    sc = scene(sname, par, oracle, T)
    tints = TINTS[:len(which)]
    lights, exp, info = expected(T, sc, which, radii, tints, need, name)
    with sc.renderer(par, model_of(par, radii)) as r:
        r.set_lights(lights)
        r.set_light_tints(T.make_tints(tints))
        for k in range(3):  # (the atomics' order decides the walk area's layout)
            assert_planes_equal(r.render(ALL, flags=par.RENDER_COUNT_RAYS if k else 0), exp, ALL, f"{name}, render {k}")
            if k:
                assert r.stats().shadow_rays == info["rays"], f"{name}: shadow_rays"
        r.stats()


def test_fewer_tints_than_lights_and_tints_before_lights(par, oracle, T):
    """Tints go by light index and do not depend on the light count: two tints for four lights leave lights 2 and 3
    white, and tints set before the lights hold for them."""
    sc = scene("graybox", par, oracle, T)
    which, radii = [0, 3, 6, 7], [0, 200, 300, 150]
    lights, exp, _ = expected(T, sc, which, radii, TINTS[:2], COLOUR, "two tints, four lights")
    _, exp8, _ = expected(T, sc, which, radii, TINTS, COLOUR, "eight tints, four lights")
    with sc.renderer(par, par.LIGHTS_RANGED) as r:
        r.set_light_tints(T.make_tints(TINTS[:2]))
        r.set_lights(lights)
        assert_planes_equal(r.render(ALL), exp, ALL, "two tints, four lights")
        r.set_light_tints(T.make_tints(TINTS))
        assert_planes_equal(r.render(ALL), exp8, ALL, "eight tints, four lights")
        r.set_lights(lights[:2])
        _, exp2, _ = expected(T, sc, which[:2], radii[:2], TINTS[:2], COLOUR, "two lights of them")
        assert_planes_equal(r.render(ALL), exp2, ALL, "eight tints, two lights")
        r.stats()


# ---- 3. what tints must not touch ------------------------------------------------------------------------------

@pytest.mark.parametrize("radii", [None, [0, 200, 300, 150]])
def test_tints_do_not_touch_lit_gbuf_palidx_rays_and_walks(par, oracle, T, radii):
    sc = scene("random7", par, oracle, T)
    lights, _ = sc.pick(T, [0, 1, 2, 6], radii or [10] * 4)
    keep = ("lit", "gbuf", "palidx")
    bgf = par.RENDER_COUNT_RAYS | par.RENDER_TRACE_BACKGROUND
    with sc.renderer(par, model_of(par, radii)) as r:
        r.set_lights(lights)
        plain = r.render(ALL, flags=bgf)
        rays, walks = r.stats().shadow_rays, r.light_walks()
        r.set_light_tints(T.make_tints(TINTS[:4]))
        got = r.render(ALL, flags=bgf)
        assert_planes_equal(got, plain, keep, "tinted against untinted")
        assert r.stats().shadow_rays == rays and r.light_walks() == walks
        assert not np.array_equal(got["fb"], plain["fb"]), "the tints should show"
        assert (got["lit"][got["palidx"] != 0xFF] >> BLACK & 1).any(), "the black light sets its bit"
        bg = got["palidx"] == 0xFF
        assert np.array_equal(got["fb"][bg], plain["fb"][bg]) and np.array_equal(got["brightness"][bg], plain["brightness"][bg])
    if radii:
        assert walks[1] > 0, "some pairs should be culled"


# ---- 4. host paths ---------------------------------------------------------------------------------------------

def test_host_paths_of_a_tinted_frame(par, oracle, T):
    import torch
    sc = scene("graybox", par, oracle, T)
    which, radii = [0, 3, 6, 7], [0, 200, 300, 150]
    lights, exp, _ = expected(T, sc, which, radii, TINTS[:4], EVERY, "host paths")
    with sc.renderer(par, par.LIGHTS_RANGED) as r:
        r.set_lights(lights)
        r.set_light_tints(T.make_tints(TINTS[:4]))
        for rows, planes in [((37, 251), ALL), ((0, 40), ("fb",)), (None, ("fb",)), (None, ("brightness",)),
                             ((120, 320), ("brightness",)), ((5, 300), ("fb", "lit")), ((40, 80), ("gbuf", "palidx"))]:
            for k in range(2):
                got = r.render(planes, rows=rows)
                assert_planes_equal(got, rows_of(exp, sc.params, rows, planes), planes, f"rows {rows} planes {planes}, render {k}")
        # par_render_device: the whole frame and a row range into device planes
        stream = torch.cuda.Stream()
        for rows in (None, (80, 240)):
            out = Planes(sc.params, ALL, rows)
            for k in range(3):
                r.render_device(out.ptrs, rows=rows, stream=stream.cuda_stream)
                stream.synchronize()
                assert_planes_equal(out.host(T), rows_of(exp, sc.params, rows, ALL), ALL, f"render_device rows {rows}, frame {k}")
        r.stats()


# ---- 5. the limit scenes of the light kernel (the lane-walk fallbacks) -----------------------------------------

def limit_frame(par, oracle, T, params, aabbs, pos, radii, tints, tag):
    sc = Scene(par, oracle, T, params, aabbs, pos)
    lights, exp, _ = expected(T, sc, list(range(len(pos))), radii, tints, COLOUR, tag)
    with sc.renderer(par, model_of(par, radii)) as r:
        r.set_lights(lights)
        r.set_light_tints(T.make_tints(tints))
        for k in range(3):
            assert_planes_equal(r.render(ALL), exp, ALL, f"{tag}, render {k}")
        r.stats()


@pytest.mark.parametrize("radii", [None, [500, 0, 300, 250]])
def test_limit_mixed_stage(par, oracle, T, radii):
    params, aabbs = mixed_stage_scene(T)
    limit_frame(par, oracle, T, params, aabbs, MIXED_STAGE_LIGHTS[:4], radii, TINTS[:4], f"mixed stage {radii}")


@pytest.mark.parametrize("radii", [None, [900, 0, 1500, 600]])
def test_limit_more_than_64_occupied_bins(par, oracle, T, radii):
    params, aabbs = many_bins_scene(T)
    limit_frame(par, oracle, T, params, aabbs, MANY_BINS_LIGHTS[:4], radii, TINTS[:4], f"many bins {radii}")


# ---- 6. graphs -------------------------------------------------------------------------------------------------

def status(par, fn, *args, **kw):
    with pytest.raises(par.ParError) as e:
        fn(*args, **kw)
    return e.value.status


@pytest.mark.parametrize("radii", [None, [0, 200, 300, 150]])
def test_graph_replays_follow_tint_values_and_moving_lights(par, oracle, T, radii):
    """par_graph_capture_lights on a tinted context: over several launches the tints' values change and the lights move;
    each replay equals par_render_device of a second context in the same state, and the first the composed oracle."""
    import torch
    sc = scene("random7", par, oracle, T)
    which = [0, 1, 2, 6]
    lights, exp, _ = expected(T, sc, which, radii, TINTS[:4], EVERY, f"graph {radii}")
    stream, stream2 = torch.cuda.Stream(), torch.cuda.Stream()
    out, ref = Planes(sc.params, ALL), Planes(sc.params, ALL)
    rng = np.random.default_rng(11)
    with sc.renderer(par, model_of(par, radii)) as r, sc.renderer(par, model_of(par, radii)) as check:
        tints = T.make_tints(TINTS[:4])
        for c in (r, check):
            c.set_lights(lights)
            c.set_light_tints(tints)
        r.graph_capture_lights(out.ptrs, stream=stream.cuda_stream)
        for k in range(2):  # (both grid sets' graphs)
            assert_planes_equal(replay(r, out, stream, T), exp, ALL, f"tinted graph, replay {k}")
        cur, shown = lights.copy(), set()
        for f in range(8):
            if f % 3 != 2:  # new values, the same state: the graph stays
                tints = T.make_tints(np.roll(np.array(TINTS[:8], dtype=np.float32), f + 1, axis=0)[:2 + f % 3 * 2])
                for c in (r, check):
                    c.set_light_tints(tints)
            if f % 2 or f % 3 == 2:
                cur = cur.copy()
                for ax in "xyz":
                    cur[ax] += rng.choice([-5, 5], size=len(cur)).astype(np.int16)
                r.graph_stage(lights=cur)
                check.set_lights(cur)
            if f == 5:  # fewer lights under the same graph
                r.graph_stage(lights=cur[:2])
                check.set_lights(cur[:2])
            got = replay(r, out, stream, T)
            check.render_device(ref.ptrs, stream=stream2.cuda_stream)
            stream2.synchronize()
            want = ref.host(T)
            assert_planes_equal(got, want, ALL, f"frame {f}: graph replay vs par_render_device")
            shown.add(want["fb"].tobytes())
        assert len(shown) == 8, "every change should show in the frame"
        r.stats()
        check.stats()


def test_graph_refusals_and_state_changes(par, oracle, T):
    import torch
    sc = scene("random7", par, oracle, T)
    which, radii = [0, 1, 2, 6], None
    lights, exp, _ = expected(T, sc, which, radii, TINTS[:4], EVERY, "graph refusals")
    stream = torch.cuda.Stream()
    out = Planes(sc.params, ALL)
    tints = T.make_tints(TINTS[:4])
    with sc.renderer(par) as r:
        r.set_lights(lights)
        r.set_light_tints(tints)
        # the one-light capture refuses a tinted context, with one light too
        assert status(par, r.graph_capture, out.ptrs, stream=stream.cuda_stream) == ERR_UNSUPPORTED
        r.set_lights(lights[:1])
        assert status(par, r.graph_capture, out.ptrs, stream=stream.cuda_stream) == ERR_UNSUPPORTED
        assert "tinted" in par.lib().par_last_error(r._ctx).decode()
        r.set_lights(lights)
        r.graph_capture_lights(out.ptrs, stream=stream.cuda_stream)
        assert_planes_equal(replay(r, out, stream, T), exp, ALL, "tinted graph")
        r.set_light_tints(tints)  # (the same state again: the graph stays)
        assert_planes_equal(replay(r, out, stream, T), exp, ALL, "tinted graph, same tints again")
        # tinted -> untinted drops the graphs
        r.set_light_tints(None)
        assert status(par, r.graph_launch, stream.cuda_stream) == ERR_NOT_READY
        assert status(par, r.graph_stage, lights=lights) == ERR_NOT_READY
        # an untinted light-path graph; untinted again is no change; tinted drops it
        r.graph_capture_lights(out.ptrs, stream=stream.cuda_stream)
        plain = r.render(ALL)
        assert_planes_equal(replay(r, out, stream, T), plain, ALL, "untinted graph")
        r.set_light_tints(None)
        assert_planes_equal(replay(r, out, stream, T), plain, ALL, "untinted graph, untinted again")
        r.set_light_tints(tints)
        assert status(par, r.graph_launch, stream.cuda_stream) == ERR_NOT_READY
        assert status(par, r.graph_stage, lights=lights) == ERR_NOT_READY
        assert_planes_equal(r.render(ALL), exp, ALL, "direct frame after the graphs went")
        r.stats()
    # a one-light graph goes when the context becomes tinted, and a tinted context cannot launch one
    with sc.renderer(par) as r:
        r.set_lights(lights[:1])
        r.graph_capture(out.ptrs, stream=stream.cuda_stream)
        assert_planes_equal(replay(r, out, stream, T), sc.outs[0], ALL, "one-light graph")
        r.set_light_tints(None)  # (no change: the graph stays)
        assert_planes_equal(replay(r, out, stream, T), sc.outs[0], ALL, "one-light graph, still untinted")
        r.set_light_tints(tints)
        assert status(par, r.graph_launch, stream.cuda_stream) == ERR_NOT_READY
        r.stats()


# ---- 7. argument checks with a live context --------------------------------------------------------------------

def test_rejected_calls_change_nothing(par, oracle, T):
    sc = scene("graybox", par, oracle, T)
    which, radii = [0, 3, 6, 7], None
    lights, exp, _ = expected(T, sc, which, radii, TINTS[:4], EVERY, "argument checks")
    L = par.lib()
    good = T.make_tints(TINTS[:4])
    nine = T.make_tints([LT.WHITE] * 9)
    with sc.renderer(par) as r:
        r.set_lights(lights)
        plain = r.render(ALL)
        bad = [(nine, 9), (good, 0), (None, 2), (good, -1)]
        for v in (float("nan"), float("inf"), -float("inf"), -0.5):
            for l, c in ((0, "r"), (1, "g"), (3, "b")):
                t = good.copy()
                t[l][c] = v
                bad.append((t, 4))
        for state, want in (("untinted", plain), ("tinted", exp)):
            if state == "tinted":
                r.set_light_tints(good)
                assert_planes_equal(r.render(ALL), exp, ALL, "tinted frame")
            for t, n in bad:
                assert L.par_set_light_tints(r._ctx, T.ptr(t), n) == ERR_INVALID_ARG, (state, n)
                assert "light tints" in L.par_last_error(r._ctx).decode()
            assert_planes_equal(r.render(ALL), want, ALL, f"{state}: the frame after the rejected calls")
        with pytest.raises(par.ParError):
            r.set_light_tints(nine)
        r.set_light_tints(None)
        assert_planes_equal(r.render(ALL), plain, ALL, "set_light_tints(None) restores the untinted frame")
        r.stats()
