"""GPU tests of the light path's captured graphs (par_graph_capture_lights, par_graph_stage_lights): replays against the
pinned oracle with one light, against a second renderer's direct render with several, while the scene and the lights
move and the light count changes under one graph, and the refusals."""
import os

import numpy as np
import pytest

from helpers import graybox, random_stage_scene
from test_gpu_lights import compose, lights_of, oracle_planes
from test_gpu_parity import ALL, assert_planes_equal

pytestmark = pytest.mark.gpu

NTHREADS = min(os.cpu_count() or 8, 16)
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_NOT_READY = 1, 5, 8
BYTES = {"fb": 4, "gbuf": 28, "palidx": 1, "brightness": 4, "lit": 1}


@pytest.fixture(scope="module")
def sprite(par):
    return par.tile_floor()


class Planes:
    """Device output planes of rows [r0, r1) and their host copies."""

    def __init__(self, params, planes, rows=None):
        import torch
        self.r0, self.r1 = rows or (0, params.height)
        n = (self.r1 - self.r0) * params.width
        self.planes = planes
        self.bufs = {k: torch.zeros(n * BYTES[k], dtype=torch.uint8, device="cuda") for k in planes}
        self.ptrs = {k: b.data_ptr() for k, b in self.bufs.items()}
        # (the fills ran on the current stream; the tests render on streams of their own, which do not wait for it)
        torch.cuda.current_stream().synchronize()

    def host(self, T):
        dt = {"fb": T.COLOR, "gbuf": T.PIXEL, "palidx": np.uint8, "brightness": np.float32, "lit": np.uint8}
        return {k: self.bufs[k].cpu().numpy().view(dt[k]) for k in self.planes}


def replay(r, out, stream, T):
    r.graph_launch(stream.cuda_stream)
    stream.synchronize()
    return out.host(T)


def direct(par, params, sprite, aabbs, lights, planes, rows=None, flags=0):
    with par.Renderer(params) as c:
        c.set_sprites(sprite)
        c.set_entities(aabbs)
        c.set_lights(lights)
        return c.render(planes, rows=rows, flags=flags)


# ---- 1. one light against the pinned oracle -------------------------------------------------------------------

def test_light_graph_one_light_against_the_oracle(par, oracle, golden_frames, sprite, T):
    import torch
    params = T.default_params()
    # (every golden frame with primitives: a graph's AABB upload is a copy of at least one)
    scenes = [(f"golden {name}", aabbs, light) for name, (_, aabbs, light) in golden_frames.items() if len(aabbs)]
    scenes += [(f"random {seed}", *random_stage_scene(seed)) for seed in (0, 2, 5, 9)]
    stream = torch.cuda.Stream()
    for tag, aabbs, light in scenes:
        exp = oracle.render(params, aabbs, sprite, light, nthreads=NTHREADS)
        out = Planes(params, ALL)
        with par.Renderer(params) as r:
            r.set_scene(aabbs, sprite, light)
            r.graph_capture_lights(out.ptrs, stream=stream.cuda_stream)
            for k in range(2):  # (both grid sets' graphs)
                assert_planes_equal(replay(r, out, stream, T), exp, ALL, f"{tag}, replay {k}")
            r.stats()


# ---- 2. the animation of config 5 with several moving lights, frames in flight ---------------------------------

def test_light_graph_animation_frames_in_flight(par, oracle, sprite, T):
    import torch
    w = h = l = 1024
    n, frames = 512, 48
    params = T.default_params(w, h, l)
    aabbs, _ = par.scene_synthetic(n, w, h, l, 41)
    lights = lights_of(T, [(640, 512, 256), (100, 900, 40), (1000, 30, 900)])
    rng = np.random.default_rng(23)
    vel = rng.choice([-5, 0, 5], size=(n, 3)).astype(np.int16)
    lvel = rng.choice([-5, 5], size=(len(lights), 3)).astype(np.int32)
    planes = ("fb", "palidx", "brightness", "lit")
    out = Planes(params, planes)
    ring = {k: torch.zeros(frames, w * h * BYTES[k], dtype=torch.uint8, device="cuda") for k in planes}
    stream = torch.cuda.Stream()
    scenes = []
    with par.Renderer(params) as r:
        r.set_sprites(sprite)
        r.set_entities(aabbs)
        r.set_lights(lights)
        r.graph_capture_lights(out.ptrs, stream=stream.cuda_stream)
        cur = lights.copy()  # what the context holds
        for f in range(frames):
            if f:
                aabbs["px"] += vel[:, 0]
                aabbs["py"] += vel[:, 1]
                aabbs["pz"] += vel[:, 2]
                moved = cur.copy()
                for c, ax in enumerate("xyz"):
                    moved[ax] += lvel[:, c]
                if f % 9 == 0:  # the lights alone, outside the stage call
                    r.graph_stage(aabbs, 0)
                    r.set_lights(moved)
                    cur = moved
                elif f % 11 == 0:  # lights[0] through par_graph_stage: the count is kept
                    r.graph_stage(aabbs, 0, light=moved[0:1])
                    cur[0] = moved[0]
                else:
                    r.graph_stage(aabbs, 0, lights=moved)
                    cur = moved
            r.graph_launch(stream.cuda_stream)
            with torch.cuda.stream(stream):
                for k in planes:
                    ring[k][f].copy_(out.bufs[k], non_blocking=True)
            scenes.append((aabbs.copy(), cur.copy()))
        stream.synchronize()
        r.stats()  # raises on PAR_ERR_DEVICE
    got = {k: v.cpu().numpy() for k, v in ring.items()}
    dt = {"fb": T.COLOR, "palidx": np.uint8, "brightness": np.float32, "lit": np.uint8}
    with par.Renderer(params) as check:
        check.set_sprites(sprite)
        check.set_entities(aabbs)
        for f, (a, ls) in enumerate(scenes):
            check.update_aabbs(a, 0)
            check.set_lights(ls)
            exp = check.render(planes)
            frame = {k: got[k][f].view(dt[k]) for k in planes}
            assert_planes_equal(frame, exp, planes, f"frame {f}: graph replay vs direct render")
            if f % 10 == 0 or f == frames - 1:
                ora, _ = compose(params, oracle_planes(oracle, params, a, sprite, ls), ls)
                assert_planes_equal(frame, ora, planes, f"frame {f}: graph replay vs composed oracle")


# ---- 3. the light count changes under one graph ----------------------------------------------------------------

def test_light_graph_light_count_changes(par, sprite, T):
    import torch
    params = T.default_params()
    aabbs, light = random_stage_scene(7)
    pool = [(480, 160, 80), (250, 150, 90), (255, 152, 88), (240, 100, 150), (-50, 120, -30), (400, 80, 200),
            (60, 140, 20), (20, 300, 10)]
    stream = torch.cuda.Stream()
    out = Planes(params, ALL)
    with par.Renderer(params) as r:
        r.set_scene(aabbs, sprite, light)
        r.graph_capture_lights(out.ptrs, stream=stream.cuda_stream)
        for i, count in enumerate((2, 8, 1, 5)):
            ls = lights_of(T, pool[i:] + pool[:i])[:count]
            r.graph_stage(lights=ls)
            got = replay(r, out, stream, T)
            assert_planes_equal(got, direct(par, params, sprite, aabbs, ls, ALL), ALL, f"{count} lights")
        r.stats()


# ---- 4. background rays and row blocks -------------------------------------------------------------------------

def test_light_graph_background_rays_and_row_blocks(par, sprite, T):
    import torch
    params = T.default_params()
    aabbs = graybox(par)
    ls = lights_of(T, [(480, 160, 80), (100, 50, 200), (240, 300, 20)])
    stream = torch.cuda.Stream()
    bg = par.RENDER_TRACE_BACKGROUND
    for rows, flags, planes in [(None, bg, ALL), ((37, 251), 0, ALL), ((37, 251), bg, ("fb", "lit")),
                                ((5, 300), bg, ("fb", "brightness"))]:
        tag = f"rows {rows} flags {flags} planes {planes}"
        out = Planes(params, planes, rows)
        with par.Renderer(params) as r:
            r.set_sprites(sprite)
            r.set_entities(aabbs)
            r.set_lights(ls)
            if flags and "lit" not in planes:
                # without a lit plane, graph mode needs one direct render with the flag first (its scratch plane)
                with pytest.raises(par.ParError) as e:
                    r.graph_capture_lights(out.ptrs, rows=rows, flags=flags, stream=stream.cuda_stream)
                assert e.value.status == ERR_NOT_READY
                r.render(planes, rows=rows, flags=flags)
            r.graph_capture_lights(out.ptrs, rows=rows, flags=flags, stream=stream.cuda_stream)
            exp = direct(par, params, sprite, aabbs, ls, planes, rows=rows, flags=flags)
            for k in range(2):
                assert_planes_equal(replay(r, out, stream, T), exp, planes, f"{tag}, replay {k}")
            moved = ls.copy()
            moved["x"] -= 30
            moved["z"] += 25
            r.graph_stage(lights=moved)
            exp = direct(par, params, sprite, aabbs, moved, planes, rows=rows, flags=flags)
            assert_planes_equal(replay(r, out, stream, T), exp, planes, f"{tag}, moved lights")
            r.stats()


# ---- 5. refusals and state -------------------------------------------------------------------------------------

def test_light_graph_refusals_and_state(par, sprite, T):
    import torch
    params = T.default_params()
    aabbs, light = random_stage_scene(3)
    stream = torch.cuda.Stream()
    planes = ("fb", "palidx", "brightness", "lit")
    two = lights_of(T, [(480, 160, 80), (100, 50, 200)])

    def status(fn, *args, **kw):
        with pytest.raises(par.ParError) as e:
            fn(*args, **kw)
        return e.value.status

    # a one-light graph refuses several lights and keeps the scene staged before
    out = Planes(params, planes)
    with par.Renderer(params) as r:
        r.set_scene(aabbs, sprite, light)
        assert status(r.graph_stage, lights=two) == ERR_NOT_READY  # (no graph yet)
        r.graph_capture(out.ptrs, stream=stream.cuda_stream)
        staged = aabbs.copy()
        staged["px"] += 5
        r.graph_stage(staged, 0)
        moved = aabbs.copy()
        moved["pz"] -= 5
        assert status(r.graph_stage, moved, 0, lights=two) == ERR_UNSUPPORTED
        got = replay(r, out, stream, T)
        assert_planes_equal(got, direct(par, params, sprite, staged, light, planes), planes, "one-light graph")
        r.stats()

    out = Planes(params, planes)
    with par.Renderer(params) as r:
        r.set_sprites(sprite)
        r.set_entities(aabbs)
        r.set_lights(two)
        r.graph_capture_lights(out.ptrs, stream=stream.cuda_stream)
        L = par.lib()
        ctx = r._ctx
        ls = lights_of(T, [(300, 100, 100)] * 9)
        assert L.par_graph_stage_lights(ctx, None, 0, 0, T.ptr(ls), 0) == ERR_INVALID_ARG
        assert L.par_graph_stage_lights(ctx, None, 0, 0, T.ptr(ls), 9) == ERR_INVALID_ARG
        assert L.par_graph_stage_lights(ctx, None, 0, 0, None, 2) == ERR_INVALID_ARG
        assert L.par_graph_stage_lights(ctx, None, 0, 0, T.ptr(ls), -1) == ERR_INVALID_ARG
        assert status(r.graph_stage, lights=ls) == ERR_INVALID_ARG
        moved = aabbs.copy()
        moved["px"] += 5
        assert L.par_graph_stage_lights(ctx, T.ptr(moved), 0, len(moved), T.ptr(ls), 9) == ERR_INVALID_ARG
        # the rejected calls changed nothing: the next launch renders the captured scene and lights
        got = replay(r, out, stream, T)
        assert_planes_equal(got, direct(par, params, sprite, aabbs, two, planes), planes, "after refusals")
        r.stats()
        r.set_sprites(sprite)
        assert status(r.graph_launch, stream.cuda_stream) == ERR_NOT_READY
        assert status(r.graph_stage, lights=two) == ERR_NOT_READY

    # a staged scene beyond the captured bound: captured with every primitive off screen (no bin insertions), staged
    # with all of them on screen, each into at least eight bins
    crowd, _ = par.scene_synthetic(2000, params.width, params.height, params.length, 4)
    crowd["ex"], crowd["ey"], crowd["ez"] = 20, 20, 20
    hidden = crowd.copy()
    hidden["px"] = -100
    crowd["px"] = 30 + 40 * (np.arange(len(crowd)) % 10)
    crowd["py"], crowd["pz"] = 30, 30
    out = Planes(params, planes)
    with par.Renderer(params) as r:
        r.set_sprites(sprite)
        r.set_entities(hidden)
        r.set_lights(two)
        r.graph_capture_lights(out.ptrs, stream=stream.cuda_stream)
        three = lights_of(T, [(300, 100, 100), (10, 10, 10), (470, 300, 300)])
        assert status(r.graph_stage, crowd, 0, lights=three) == ERR_UNSUPPORTED
        got = replay(r, out, stream, T)
        assert_planes_equal(got, direct(par, params, sprite, hidden, two, planes), planes, "after the bound refusal")
        r.stats()
