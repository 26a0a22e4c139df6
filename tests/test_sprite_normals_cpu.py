"""Shading with generated sprite normals, without a GPU (tests/sprites.py has the generator and the scenes).

With the tile floor's normals, (0, 1, 0) and (0, 0, -1), the diffuse dot product is exact however it is summed, so no
frame of the tile floor tells a contracted, reordered or widened sum from the contract's. These tests hold, on the
scenes tests/test_gpu_sprite_normals.py renders:
- that the generated tables do tell them apart (test_a_contracted_dot_product_would_show), as a condition;
- the oracle to the reference's own shading loop on G-buffers with generated normals, special values included: live
  where oracle/_ref is built, and everywhere through the hashes tests/golden/make_golden.py recorded from it;
- the numpy light composers (test_gpu_lights.compose, light_range.compose_ranged, light_tints.compose_tinted and their
  one-pixel forms) to the oracle with one unbounded white light, so that a NaN dot product gives 0 and a NaN sum 1 as
  std::max(0.f, dot) and std::min(1.f, s + ambient) do.

contracted_share as measured (view: unit, wide, rough, two tables):
  main   0.0775, 0.0778, 0.0792, 0.0755; with the other lights of sprites.LIGHT_POOL 0.0518 .. 0.0861
  odd    0.0811, 0.0692, 0.0831, 0.0817
  dense  0.0718, 0.0713, 0.0722, 0.0710
  crowd  0.0749, 0.0766, 0.0767, 0.0747
and 0.0 with the tile floor in every view."""
import functools
import json
import os

import numpy as np
import pytest

import light_range as LR
import light_tints as LT
import sequences as SQ
import sprites as SP
from helpers import sha
from test_gpu_lights import compose

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIT = ("fb", "brightness", "lit")
NTHREADS = min(os.cpu_count() or 8, 16)


@pytest.fixture(scope="module")
def ref_checks():
    with open(os.path.join(GOLDEN, "ref_checks.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _frame(view, name, light_pos):
    """The oracle's frame of a table in a view (computed once, left unchanged): (params, aabbs, sprites, ids, light,
    planes)."""
    from oracle.oracle import Oracle
    oracle = Oracle()
    params, aabbs, light = SP.scene(view)
    if light_pos is not None:
        light = SP.T.make_light(*light_pos)
    if name == "floor":
        sprites, ids = oracle.tile_floor(), None
    else:
        sprites, ids = SP.table(oracle.tile_floor(), name, SP.SPRITE_SEED, len(aabbs), params.palette_size)
    return params, aabbs, sprites, ids, light, oracle.render(params, aabbs, sprites, light, ids, nthreads=NTHREADS)


def frame(view, name, light_pos=None):
    return _frame(view, name, light_pos)


def oracle_grid(view):
    from oracle.oracle import Oracle
    params, aabbs, _ = SP.scene(view)
    return Oracle().bin(params, aabbs)


# ---- the generator -----------------------------------------------------------------------------------------------

def test_generator_is_seeded_and_keeps_the_layout(oracle, T):
    base = oracle.tile_floor()
    for kind in SP.KINDS:
        a, b = SP.sprite(base, kind, 7), SP.sprite(base, kind, 7)
        assert a.tobytes() == b.tobytes() and a.tobytes() != SP.sprite(base, kind, 8).tobytes(), kind
        assert a.dtype == T.SPRITE and a.shape == (1,)
        assert 0 <= a["color"].min() and a["color"].max() == 3 and len(np.unique(a["color"])) == 4, kind
        jitter = a["depth"][0] - base["depth"][0]
        if kind == "rough":
            assert set(np.unique(jitter)) == {0, 1, 2, 3}
            assert a["normal"].tobytes() == SP.sprite(base, "unit", 7)["normal"].tobytes()
        else:
            assert not jitter.any(), kind
    n = SP.sprite(base, "unit", 7)["normal"][0]
    l2 = np.sqrt(n["x"].astype(np.float64) ** 2 + n["y"].astype(np.float64) ** 2 + n["z"].astype(np.float64) ** 2)
    assert np.abs(l2 - 1).max() < 1e-6
    w = SP.sprite(base, "wide", 7)["normal"][0]
    for k in "xyz":
        assert w[k].min() < -1.4 and w[k].max() > 1.4 and np.abs(w[k]).max() <= 1.5
    words = SP.sprite(base, "special", 7)["normal"].view(np.uint32)
    assert set(words.reshape(-1).tolist()) == set(SP.SPECIAL_WORDS.tolist())
    two = SP.two_tables(base, 7)
    assert two.shape == (2,) and two[0].tobytes() == SP.sprite(base, "unit", 7)[0].tobytes()
    assert two[1].tobytes() == SP.sprite(base, "wide", 8)[0].tobytes()
    assert SP.sprite_ids(5).tolist() == [0, 1, 0, 1, 0] and SP.sprite_ids(5).dtype == np.int32


def test_scenes_are_what_the_gpu_tests_need():
    for view in SP.VIEWS:
        params, aabbs, _, _, _, out = frame(view, "unit")
        covered = out["palidx"] != 0xFF
        lit = (out["lit"][covered] != 0).mean()
        print(f"{view}: {len(aabbs)} entities, covered {covered.mean():.3f}, lit of the covered {lit:.3f}")
        assert covered.mean() > 0.5 and 0.3 < lit < 0.85, view
        assert (aabbs["ex"] <= 20).all() and (aabbs["ey"] + aabbs["ez"] <= 40).all()
        # what decides the frame's launches (csrc/par_book.h, par_launch_render_both): dense frames have whole-tile
        # items; fewer than 2 048 columns take the one merged launch
        _, tileable, dense = SQ.column_histograms(params, aabbs)
        occupied, records, _ = SQ.grid_sizes(params, oracle_grid(view))
        gx, gy, _ = params.grid_dims()
        print(f"{view}: {gx * gy} columns, {int(occupied.sum())} occupied, {tileable} whole tiles, most records {records}")
        assert dense, view
        assert tileable >= 40 and occupied.sum() >= tileable + 10  # whole-tile items, and entry items beside them
        if view == "dense":  # too large for the merged launch
            assert tileable >= 2048 and occupied.sum() >= tileable + 100
        else:
            assert gx * gy < 2048
        assert (records > SQ.COL_ENT) == (view == "crowd")  # more slot records than a column record holds
    assert 200 <= len(frame("main", "unit")[1]) <= 300
    for x, y, z in SP.REFERENCE_LIGHTS:
        assert 0 <= x <= 480 and 0 <= z < 320 and 1 <= y + z <= 320
    assert tuple(SP.VIEWS["main"][-1]) == SP.REFERENCE_LIGHTS[0] == SP.LIGHT_POOL[0] and len(SP.LIGHT_POOL) == 8


# ---- teeth -------------------------------------------------------------------------------------------------------

TEETH = [(view, None) for view in SP.VIEWS] + [("main", at) for at in SP.LIGHT_POOL[1:]]


@pytest.mark.parametrize("view,light_pos", TEETH)
def test_a_contracted_dot_product_would_show(view, light_pos):
    """On every scene of the GPU tests: a contracted dot product changes the brightness of at least 2 % of the lit
    covered pixels with every finite table, and of none with the tile floor (the gap these tests close)."""
    for name in SP.FINITE + ("two",):
        params, _, _, _, light, out = frame(view, name, light_pos)
        share = SP.contracted_share(params, out["gbuf"], out["lit"], light)
        print(f"{view} {light_pos} {name}: contracted_share {share:.4f}")
        assert share >= 0.02, (view, name, share)
    params, _, _, _, light, out = frame(view, "floor", light_pos)
    assert (out["lit"][out["palidx"] != 0xFF] != 0).any()
    assert SP.contracted_share(params, out["gbuf"], out["lit"], light) == 0.0


def test_both_clamps_act_with_wide_normals():
    params, _, _, _, _, out = frame("main", "wide")
    b = out["brightness"][(out["palidx"] != 0xFF) & (out["lit"] != 0)]
    assert (b == np.float32(1)).sum() > 100 and (b == np.float32(params.ambient)).sum() > 100
    assert ((b > np.float32(params.ambient)) & (b < np.float32(1))).sum() > 100


# ---- normal bytes in the oracle's G-buffer -----------------------------------------------------------------------

def test_normal_bytes_reach_the_oracles_gbuffer():
    """Every covered texel's normal words are a row of the sprite's table; NaN payloads, -0 and denormals included."""
    for view in SP.VIEWS:
        _, _, sprites, _, _, out = frame(view, "special")
        covered = out["palidx"] != 0xFF
        got = out["gbuf"]["normal"][covered].view(np.uint32).reshape(-1, 3)
        rows = {r.tobytes() for r in sprites["normal"].view(np.uint32).reshape(-1, 3)}
        assert {r.tobytes() for r in np.unique(got, axis=0)} <= rows
        seen = set(got.reshape(-1).tolist())
        assert seen == set(SP.SPECIAL_WORDS.tolist()), view


# ---- the oracle against the reference ----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", SP.KINDS)
def test_oracle_equals_the_reference_on_generated_gbuffers(oracle, reference, ref_checks, kind):
    """oracle.render at the reference's view for three lights inside its arrays: the planes equal the hashes of the
    reference's own shading loop on the oracle's G-buffer and grid (make_golden.py), and that loop itself where it runs."""
    from oracle.oracle import GridArrays
    for at in SP.REFERENCE_LIGHTS:
        params, aabbs, sprites, ids, light, out = frame("main", kind, at)
        assert (params.width, params.height, params.length, params.bin_size) == (480, 320, 320, 40)
        exp = ref_checks["sprite_normals"][kind]["%d,%d,%d" % at]
        for k in ("gbuf", "fb", "brightness", "lit"):
            assert sha(out[k]) == exp[k], (kind, at, k)
        if reference is None:
            continue
        grid = oracle.bin(params, aabbs, GridArrays(params))
        fb, br, lit = reference.shade(grid, out["gbuf"], light)
        own = reference.shade_own(grid, out["gbuf"], light)
        assert own.tobytes() == out["fb"].tobytes(), (kind, at)
        assert fb.tobytes() == out["fb"].tobytes(), (kind, at)
        assert br.tobytes() == out["brightness"].tobytes(), (kind, at)
        assert lit.tobytes() == out["lit"].tobytes(), (kind, at)


# ---- the numpy light composers against the oracle ----------------------------------------------------------------

def planes_equal(got, exp, tag):
    for k in LIT:
        g, e = got[k], exp[k]
        if g.tobytes() != e.tobytes():
            diff = np.nonzero(g.view(np.uint8).reshape(len(g), -1) != e.view(np.uint8).reshape(len(e), -1))[0]
            p = int(diff[0])
            raise AssertionError(f"{tag}: plane {k} differs at {len(np.unique(diff))} pixels; first flat index {p}: "
                                 f"composer {g[p]}, oracle {e[p]}, texel {exp['gbuf'][p]}")


@pytest.mark.parametrize("view", list(SP.VIEWS))
@pytest.mark.parametrize("name", SP.TABLES)
def test_composers_restate_the_oracle_with_one_white_unbounded_light(T, view, name):
    params, _, _, _, light, out = frame(view, name)
    outs = [out]
    white = T.make_tints([(1, 1, 1)])
    for radius in (0, -7):  # (a radius <= 0 leaves a ranged light unbounded)
        lights = light.copy()
        lights["radius"] = radius
        planes_equal(compose(params, outs, lights)[0], out, f"{view} {name}: compose")
        planes_equal(LR.compose_ranged(params, outs, lights)[0], out, f"{view} {name}: compose_ranged, radius {radius}")
        for ranged in (False, True):
            planes_equal(LT.compose_tinted(params, outs, lights, white, ranged)[0], out,
                         f"{view} {name}: compose_tinted, ranged {ranged}, radius {radius}")


def test_one_pixel_forms_restate_the_oracle_on_special_normals(T):
    params, _, _, _, light, out = frame("main", "special")
    lights = light.copy()
    lights["radius"] = 0
    idx = np.nonzero(out["palidx"] != 0xFF)[0]
    nan_dot = 0
    for p in np.random.default_rng(5).choice(idx, 400, replace=False):
        p = int(p)
        b, bits = LR.scalar_pixel(params, [out], lights, p)
        assert bits == int(out["lit"][p])
        assert np.float32(b).tobytes() == out["brightness"][p].tobytes(), (p, out["gbuf"][p])
        f, m, bits = LT.scalar_pixel(params, [out], lights, [(1, 1, 1)], True, p)
        assert bits == int(out["lit"][p]) and np.float32(m).tobytes() == out["brightness"][p].tobytes(), p
        assert all(np.float32(v).tobytes() == out["brightness"][p].tobytes() for v in f), p
        n = out["gbuf"]["normal"][p]
        nan_dot += bool(bits and np.isnan([n["x"], n["y"], n["z"]]).any())
    assert nan_dot > 20, "the sample should hold lit pixels whose dot product is NaN"


def test_an_infinite_term_times_a_zero_tint_gives_one(T):
    """The contract's std::min(1.f, s + ambient) is (s + ambient < 1) ? s + ambient : 1: a NaN sum (inf * 0) gives 1."""
    params, _, _, _, light, out = frame("main", "special")
    tints = [(0, 1, 2.5)]
    exp, info = LT.compose_tinted(params, [out], light, tints, ranged=False)
    inf_term = info["on"][0] & np.isinf(info["added"][0])
    assert inf_term.sum() > 100
    idx = info["idx"][inf_term]
    assert (info["factors"][0][inf_term] == np.float32(1)).all()  # inf * 0 = NaN -> 1
    assert (exp["fb"]["red"][idx] == out["gbuf"]["color"]["red"][idx]).all()
    assert (exp["brightness"][idx] == np.float32(1)).all()
    for p in idx[:50]:
        f, m, _ = LT.scalar_pixel(params, [out], light, tints, False, int(p))
        assert f[0] == np.float32(1) and m == np.float32(1)
