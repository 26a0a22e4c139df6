"""GPU tests of shading with generated sprite normals (tests/sprites.py), byte for byte on every plane.

Every other frame of the suite has the tile floor's normals, (0, 1, 0) and (0, 0, -1), with which the diffuse dot product
n.x * t.x + n.y * t.y + n.z * t.z is exact however it is summed. Here the normals are random unit vectors, components in
[-1.5, 1.5], and special values (+-inf, NaNs with payloads, +-0, denormals, +-3e38): tests/test_sprite_normals_cpu.py
holds, without a GPU, that a contracted dot product would change at least 2 % of the lit covered pixels of every scene
used here with every finite table, and holds the oracle and the numpy light composers to the reference's own loop.

The dot product is written twice in csrc/par_kernels.hip: in diffuse(), which render_chunk and the light kernel call,
and in render_tile_item. Where the kernels compiled from them are reached, and what says that they were:
- render_tile_item (the whole-tile items of render_tiles_kernel and of render_both_kernel): every view of
  test_one_light_frames_on_every_render_path is dense, so its columns that are whole tiles are visited as such
  (test_sprite_normals_cpu.py: test_scenes_are_what_the_gpu_tests_need). View dense has a launch of its own for them
  (render_merged == 0, ms_launch[3] > 0); main, odd and crowd take the merged launch (render_merged == 1).
- render_chunk, entry items (render_items_kernel, render_both_kernel): the same frames; every view has occupied columns
  that are no whole tiles (the same CPU test), and ms_launch[2] > 0.
- render_chunk, columns straight from the hash (render_overflow_kernel, the overflow share of render_both_kernel): the same
  test under set_test_hooks(force_generic=True), when no other render kernel is launched (a timed frame has the overflow
  launch and is not merged: ms_launch[4] > 0, render_merged == 0; overflow_columns counts the columns that overflowed
  their record, not these) and, without a hook, view crowd (overflow_columns > 0).
- the light kernel (render_lights_kernel, every form: plain, ranged, tinted, relit, graph):
  test_the_light_kernel_with_one_light_equals_the_oracle (a timed frame is the light kernel's: ms_launch[2] > 0 and no other
  render launch), test_light_states, test_relit_frames, test_graph_replay. The relit form reads its normals from the
  G-buffer; it has no statistic of its own, the call is what selects it.
PAR_RENDER_PIPELINED changes how many wavefronts share a column's walks; no statistic tells such a frame apart.

As measured with libraries built for the purpose: with the sum of diffuse() alone contracted to fma(nz, tz, fma(ny, ty,
nx * tx)) 41 of these 44 tests fail (all but the outlines), with render_tile_item's alone 29 (all that render a one-light
frame), with both 42; test_gpu_parity.py's frames of the tile floor pass with both."""
import functools

import numpy as np
import pytest

import light_range as LR
import light_tints as LT
import outline as OL
import sprites as SP
from test_gpu_lights import NTHREADS, compose
from test_gpu_lights_graph import Planes, replay
from test_gpu_outline import run_and_check
from test_gpu_parity import ALL, assert_planes_equal
from test_sprite_normals_cpu import frame

pytestmark = pytest.mark.gpu

FAST = ("fb", "palidx", "brightness", "gbuf")  # without a lit plane the background's shadow rays are skipped
LIT = ("fb", "brightness", "lit")              # what a relit frame writes
KEPT = ("gbuf", "palidx")                      # what it leaves alone
MERGED = {"main": True, "odd": True, "crowd": True, "dense": False}

POOL = SP.LIGHT_POOL  # light positions of the main view, the view's own light first
# by light index: a zero channel on the light that reaches most pixels (inf * 0 with `special`), black, components above 1
TINTS = [(0, 1, 2.5), (1, .25, 0), (0, 0, 0), (2, 2, 2), (.5, 1, .25), (1.5, 0, .75), (.125, .125, 1), (1, 1, 1)]
RADII5 = [0, 250, 400, 200, 0]
# tag, lights out of POOL, radii (None: PAR_LIGHTS_UNBOUNDED), tints (None: untinted)
STATES = [("n=2", [0, 3], None, None),
          ("n=5", [0, 1, 2, 3, 4], None, None),
          ("n=8", list(range(8)), None, None),
          ("n=5 ranged beside unbounded", [0, 1, 2, 3, 5], RADII5, None),
          ("n=8 tinted", list(range(8)), None, TINTS),
          ("n=5 ranged and tinted", [0, 1, 2, 3, 5], RADII5, TINTS[:5])]
RELIT_STATES = [("one light", [0], None, None), STATES[3], STATES[4], STATES[5]]


def lights_of(T, positions, radii=None):
    a = np.zeros(len(positions), dtype=T.LIGHT)
    for i, (x, y, z) in enumerate(positions):
        a[i]["x"], a[i]["y"], a[i]["z"], a[i]["radius"] = x, y, z, 10 if radii is None else radii[i]
    return a


@functools.lru_cache(maxsize=None)
def lit_plane(view, name, at):
    """The oracle's lit plane of one light (computed once, left unchanged)."""
    from oracle.oracle import Oracle
    params, aabbs, sprites, ids, light, out = frame(view, name)
    if at == tuple(int(light[0][k]) for k in "xyz"):
        return out["lit"]
    return Oracle().render(params, aabbs, sprites, SP.T.make_light(*at), ids, nthreads=NTHREADS, planes=("lit",))["lit"]


def oracle_planes(view, name, positions):
    """The per-light planes the composers take: every plane with the first light, the lit plane with the others."""
    out = frame(view, name)[5]
    return [dict(out, lit=lit_plane(view, name, positions[0]))] + [{"lit": lit_plane(view, name, at)} for at in positions[1:]]


@functools.lru_cache(maxsize=None)
def _expected(view, name, which, radii, tints):
    T = SP.T
    params = frame(view, name)[0]
    positions = [POOL[i] for i in which]
    lights = lights_of(T, positions, radii)
    outs = oracle_planes(view, name, positions)
    info = {}
    if tints is not None:
        exp, info = LT.compose_tinted(params, outs, lights, tints, ranged=radii is not None)
    elif radii is not None:
        exp, per_light, _, _ = LR.compose_ranged(params, outs, lights)
        info = {"per_light": per_light}
    else:
        exp, _ = compose(params, outs, lights)
    return lights, exp, info


def expected(view, name, which, radii, tints):
    """(lights, expected planes, what the composer says about them) of a light state, by the composer of its kind (each
    held to the oracle on these very frames by test_sprite_normals_cpu.py). Computed once, left unchanged."""
    return _expected(view, name, tuple(which), None if radii is None else tuple(radii),
                     None if tints is None else tuple(tints))


def set_state(par, T, r, lights, radii, tints):
    r.set_light_model(par.LIGHTS_UNBOUNDED if radii is None else par.LIGHTS_RANGED)
    r.set_light_tints(None if tints is None else T.make_tints(tints))
    r.set_lights(lights)


def timed(par, T, r, params, stream):
    """A frame timed as a production frame launches it: (par_frame_stats, its planes)."""
    out = Planes(params, ALL)
    st = r.render_device(out.ptrs, stream=stream.cuda_stream, timed=True, flags=par.RENDER_TIMED_AS_LAUNCHED)
    stream.synchronize()
    return st, out.host(T)


# ---- 1. one-light frames on every render path ------------------------------------------------------------------------

@pytest.mark.parametrize("view", list(SP.VIEWS))
@pytest.mark.parametrize("name", SP.TABLES)
def test_one_light_frames_on_every_render_path(par, T, view, name):
    import torch
    params, aabbs, sprites, ids, light, exp = frame(view, name)
    tag = f"{view} {name}"
    stream = torch.cuda.Stream()
    with par.Renderer(params) as r:
        r.set_sprites(sprites)
        r.set_entities(aabbs, ids)
        r.set_light(light)
        # the default path
        assert_planes_equal(r.render(ALL), exp, ALL, tag)
        st = r.stats()
        assert st.occupied_columns > 0
        if view == "crowd":  # columns rendered straight from the hash, without a hook
            assert st.overflow_columns > 0, tag
        elif MERGED[view]:
            assert st.overflow_columns == 0, f"{tag}: overflow_columns {st.overflow_columns}"
        assert_planes_equal(r.render(FAST), exp, FAST, f"{tag}, fast planes")
        st, got = timed(par, T, r, params, stream)
        launches = (list(st.ms_launch), st.render_merged)
        print(f"{tag}: launches {launches}, columns {st.occupied_columns}, overflowed {st.overflow_columns}")
        assert_planes_equal(got, exp, ALL, f"{tag}, timed as launched")
        assert st.ms_launch[2] > 0, launches
        if MERGED[view]:  # entry items, tile items and overflowed columns in one launch
            assert st.render_merged == 1 and st.ms_launch[3] == 0 and st.ms_launch[4] == 0, launches
        else:             # a launch for the entry items, one for the whole-tile items
            assert st.render_merged == 0 and st.ms_launch[3] > 0, launches
        # one wavefront per column for the walks
        assert_planes_equal(r.render(ALL, flags=par.RENDER_PIPELINED), exp, ALL, f"{tag}, pipelined")
        assert_planes_equal(r.render(FAST, flags=par.RENDER_PIPELINED), exp, FAST, f"{tag}, pipelined, fast planes")
        # every column straight from the hash
        r.set_test_hooks(force_generic=True)
        assert_planes_equal(r.render(ALL), exp, ALL, f"{tag}, every column through the overflow kernel")
        assert_planes_equal(r.render(FAST), exp, FAST, f"{tag}, every column through the overflow kernel, fast planes")
        st, got = timed(par, T, r, params, stream)
        launches = (list(st.ms_launch), st.render_merged)
        assert_planes_equal(got, exp, ALL, f"{tag}, every column through the overflow kernel, timed as launched")
        assert st.render_merged == 0 and st.ms_launch[4] > 0, launches
        r.set_test_hooks()
        assert_planes_equal(r.render(ALL), exp, ALL, f"{tag}, after the hook")
        r.stats()  # raises on PAR_ERR_DEVICE


@pytest.mark.parametrize("name", SP.TABLES)
def test_ref_layout_passes_the_normal_bytes_through(par, T, name):
    """One sprite per entity, as the reference has them (par_set_entities_ref_layout); the G-buffer's normal words are the
    table's, NaN payloads and -0 included."""
    params, aabbs, sprites, ids, light, exp = frame("main", name)
    per_entity = sprites[ids] if ids is not None else np.repeat(sprites, len(aabbs))
    with par.Renderer(params) as r:
        r.set_entities_ref_layout(aabbs, per_entity)
        r.set_light(light)
        got = r.render(ALL)
        assert_planes_equal(got, exp, ALL, f"ref layout, {name}")
        assert_planes_equal(r.render(FAST), exp, FAST, f"ref layout, {name}, fast planes")
    if name == "special":
        words = got["gbuf"]["normal"][got["palidx"] != 0xFF].view(np.uint32)
        assert set(words.reshape(-1).tolist()) == set(SP.SPECIAL_WORDS.tolist())


# ---- 2. the light kernel with one light ------------------------------------------------------------------------------

@pytest.mark.parametrize("view", ["main", "odd"])
@pytest.mark.parametrize("name", SP.TABLES)
def test_the_light_kernel_with_one_light_equals_the_oracle(par, T, view, name):
    """By the header's identities a ranged context whose one light has a radius <= 0, and a tinted one whose tints are
    all white, take the light kernel and equal the unbounded, untinted frame."""
    import torch
    params, aabbs, sprites, ids, light, exp = frame(view, name)
    stream = torch.cuda.Stream()

    def is_the_light_kernels(tag):
        st, got = timed(par, T, r, params, stream)
        launches = (list(st.ms_launch), st.render_merged)
        assert_planes_equal(got, exp, ALL, f"{tag}, timed as launched")
        assert st.ms_launch[2] > 0 and st.ms_launch[3] == 0 and st.ms_launch[4] == 0 and st.render_merged == 0, launches

    with par.Renderer(params) as r:
        r.set_sprites(sprites)
        r.set_entities(aabbs, ids)
        r.set_light_model(par.LIGHTS_RANGED)
        for radius in (0, -3):
            tag = f"{view} {name}: ranged, radius {radius}"
            one = light.copy()
            one["radius"] = radius
            r.set_lights(one)
            assert_planes_equal(r.render(ALL), exp, ALL, tag)
            assert_planes_equal(r.render(FAST), exp, FAST, f"{tag}, fast planes")
        is_the_light_kernels(tag)
        r.set_light_tints(T.make_tints([(1, 1, 1)]))
        assert_planes_equal(r.render(ALL), exp, ALL, f"{view} {name}: ranged and white")
        r.set_light_model(par.LIGHTS_UNBOUNDED)
        tag = f"{view} {name}: white"
        assert_planes_equal(r.render(ALL), exp, ALL, tag)
        assert_planes_equal(r.render(FAST), exp, FAST, f"{tag}, fast planes")
        is_the_light_kernels(tag)
        r.set_light_tints(None)
        r.set_test_hooks(lights_path=True)
        tag = f"{view} {name}: the plain light kernel"
        assert_planes_equal(r.render(ALL), exp, ALL, tag)
        is_the_light_kernels(tag)
        r.stats()


# ---- 3. light states against the composers ---------------------------------------------------------------------------

def inf_times_zero(info, tints):
    """Covered pixels at which a light with a zero tint channel adds an infinite term: inf * 0 = NaN in that channel."""
    n = 0
    for l, t in enumerate(tints):
        if any(v == 0 for v in t):
            n += int(np.isinf(info["added"][l]).sum())
    return n


@pytest.mark.parametrize("name", ["unit", "wide", "special"])
def test_light_states(par, T, name):
    params, aabbs, sprites, ids, _, _ = frame("main", name)
    with par.Renderer(params) as r:
        r.set_sprites(sprites)
        r.set_entities(aabbs, ids)
        for tag, which, radii, tints in STATES:
            tag = f"{name} {tag}"
            lights, exp, info = expected("main", name, which, radii, tints)
            for l, (in_range, lit) in enumerate(info.get("per_light", [])):
                if radii[l] > 0:  # a ranged light leaves covered pixels out, and reaches lit and shadowed ones
                    assert (~in_range).any() and (in_range & lit).any() and (in_range & ~lit).any(), f"{tag}: light {l}"
            if tints is not None and name == "special":
                n = inf_times_zero(info, tints)
                print(f"{tag}: {n} terms of inf * 0")
                assert n > 100, f"{tag}: the frame should hold tinted terms of inf * 0"
            set_state(par, T, r, lights, radii, tints)
            assert_planes_equal(r.render(ALL), exp, ALL, tag)
            assert_planes_equal(r.render(FAST), exp, FAST, f"{tag}, fast planes")
        r.stats()


# ---- 4. relit frames -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["wide", "special"])
def test_relit_frames(par, T, name):
    """A frame is rendered, the lights move: par_relight_rows and par_relight_device equal a fresh render of the new
    state, which equals the composed frame."""
    import torch
    params, aabbs, sprites, ids, _, _ = frame("main", name)
    lights_a, exp_a, _ = expected("main", name, [5], None, None)
    stream = torch.cuda.Stream()
    out = Planes(params, ALL)
    with par.Renderer(params) as r:
        r.set_sprites(sprites)
        r.set_entities(aabbs, ids)
        # the host form: each state relit from the frame of the state before it
        r.set_lights(lights_a)
        assert_planes_equal(r.render(ALL), exp_a, ALL, f"{name}: the retained frame")
        for tag, which, radii, tints in RELIT_STATES:
            tag = f"{name} {tag}"
            lights, exp, _ = expected("main", name, which, radii, tints)
            assert exp["fb"].tobytes() != exp_a["fb"].tobytes(), f"{tag}: the new lights should show"
            set_state(par, T, r, lights, radii, tints)
            assert_planes_equal(r.relight(LIT), exp, LIT, f"{tag}, relit rows")
            assert_planes_equal(r.relight(LIT, rows=(37, 203)), {k: exp[k][37 * params.width:203 * params.width] for k in LIT},
                                LIT, f"{tag}, relit rows 37-203")
            assert_planes_equal(r.render(ALL), exp, ALL, f"{tag}, a fresh render")
        # the device form: each state relit over the planes of the one-light frame
        set_state(par, T, r, lights_a, None, None)
        r.render_device(out.ptrs, stream=stream.cuda_stream)
        stream.synchronize()
        assert_planes_equal(out.host(T), exp_a, ALL, f"{name}: the retained device frame")
        for tag, which, radii, tints in RELIT_STATES:
            tag = f"{name} {tag}"
            lights, exp, _ = expected("main", name, which, radii, tints)
            set_state(par, T, r, lights, radii, tints)
            for k in range(2):
                r.relight_device(out.ptrs["gbuf"], {p: out.ptrs[p] for p in LIT}, stream=stream.cuda_stream)
                stream.synchronize()
                got = out.host(T)
                assert_planes_equal(got, exp, LIT, f"{tag}, relit on the device, frame {k}")
                assert_planes_equal(got, exp_a, KEPT, f"{tag}, relit on the device, frame {k}: gbuf and palidx stay")
        r.stats()


# ---- 5. graph replay -------------------------------------------------------------------------------------------------

def test_graph_replay(par, T):
    import torch
    params, aabbs, sprites, ids, light, exp = frame("main", "unit")
    stream = torch.cuda.Stream()
    with par.Renderer(params) as r:
        r.set_sprites(sprites)
        r.set_entities(aabbs, ids)
        r.set_light(light)
        blocking = r.render(ALL)
        assert_planes_equal(blocking, exp, ALL, "one light, the blocking render")
        out = Planes(params, ALL)
        r.graph_capture(out.ptrs, stream=stream.cuda_stream)
        for k in range(2):  # (both grid sets' graphs)
            assert_planes_equal(replay(r, out, stream, T), blocking, ALL, f"par_graph_capture, replay {k}")
        tag, which, radii, tints = STATES[1]
        lights, exp, _ = expected("main", "unit", which, radii, tints)
        r.set_lights(lights)
        blocking = r.render(ALL)
        assert_planes_equal(blocking, exp, ALL, f"{tag}, the blocking render")
        out = Planes(params, ALL)
        r.graph_capture_lights(out.ptrs, stream=stream.cuda_stream)
        for k in range(2):
            assert_planes_equal(replay(r, out, stream, T), blocking, ALL, f"par_graph_capture_lights {tag}, replay {k}")
        r.stats()


# ---- 6. outlines -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["special", "unit", "zeros"])
def test_outlines_of_a_rendered_frame(par, T, name):
    """par_outline_device on the G-buffer of a rendered frame whose normals differ at almost every texel boundary: the
    crease test compares the normals' words, so NaNs equal themselves and -0 differs from +0."""
    params, aabbs, sprites, ids, light, exp = frame("main", name)
    with par.Renderer(params) as r:
        r.set_sprites(sprites)
        r.set_entities(aabbs, ids)
        r.set_light(light)
        got = r.render(("fb", "gbuf"))
    assert_planes_equal(got, exp, ("fb", "gbuf"), f"{name}: the frame")
    rows = (0, params.height)
    style = (2, 128, 320)
    _, edge, _ = run_and_check(par, T, params, style, got["gbuf"], rows, got["fb"], rows, f"outlines, {name}")
    covered = OL.covered(params, got["gbuf"])
    creases = int((edge == 1).sum())
    print(f"{name}: {creases} creases and {int((edge == 2).sum())} silhouette pixels of {int(covered.sum())} covered")
    assert creases > covered.sum() // 2, "creases at almost every texel boundary"
    if name == "zeros":  # top faces of (+-0, 1, +-0): the sign of a zero decides classes of this frame
        same_zero = got["gbuf"].copy()
        words = same_zero.view(np.uint32).reshape(-1, 7)
        words[:, :3][words[:, :3] == 0x80000000] = 0
        differ = int((OL.classes(params, style, same_zero, rows, rows) != edge).sum())
        print(f"{differ} pixels whose class depends on the sign of a zero")
        assert differ > 1000
    if name == "special":
        W = params.width
        run_and_check(par, T, params, style, got["gbuf"][40 * W:203 * W], (40, 203), got["fb"][41 * W:200 * W], (41, 200),
                      "outlines, special, a row block")
