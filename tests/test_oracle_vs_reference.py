"""The CPU oracle against the reference's OWN functions (oracle/_ref, compiled from the reference where it lies).
What those functions answered is committed (tests/golden/ref_checks.*, made by tests/golden/make_golden.py), so the
oracle is held to it on every machine; where oracle/_ref is built, the reference also runs live and must agree."""
import json
import os

import numpy as np
import pytest

from helpers import DEBUG_LINE_MICE, random_stage_scene, sha, shadow_walk_cases
from oracle.oracle import GridArrays

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref_checks():
    with open(os.path.join(GOLDEN, "ref_checks.json")) as f:
        checks = json.load(f)
    checks["shadow"] = np.load(os.path.join(GOLDEN, "ref_checks.npz"))["shadow"]
    return checks


def test_constants_and_sprite(oracle, reference, ref_checks, T):
    consts = {"bin": 40, "width": 480, "height": 320, "length": 320, "gx": 12, "gy": 8, "gz": 8, "slots": 8}
    assert ref_checks["consts"] == consts
    p = T.default_params()
    assert (p.width, p.height, p.length, p.bin_size) == (480, 320, 320, 40) and tuple(p.grid_dims()) == (12, 8, 8)
    assert T.SLOTS == 8
    assert sha(oracle.tile_floor()) == ref_checks["tile_sprite"]
    pal = np.array([(p.palette[i].red, p.palette[i].green, p.palette[i].blue, p.palette[i].alpha) for i in range(4)],
                   dtype=np.uint8)
    assert sha(pal) == ref_checks["palette"]
    if reference is not None:
        assert reference.consts == consts
        assert oracle.tile_floor().tobytes() == reference.tile_sprite().tobytes()
        assert pal.tobytes() == reference.palette().tobytes()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_scenes_all_stages(oracle, reference, ref_checks, T, seed):
    aabbs, light = random_stage_scene(seed)
    params = T.default_params()
    g_or = oracle.bin(params, aabbs)
    gb_or, _ = oracle.primary(params, g_or, oracle.tile_floor())
    fb_or, br_or, lit_or = oracle.shade(params, g_or, gb_or, light)
    exp = ref_checks["stages"][str(seed)]
    assert sha(np.frombuffer(g_or.dump(), dtype=np.uint8)) == exp["grid"]
    assert sha(gb_or) == exp["gbuf"]
    assert sha(fb_or) == exp["fb"]  # the reference's own loop, alt:702-760
    assert sha(br_or) == exp["brightness"]
    assert sha(lit_or) == exp["lit"]
    if reference is None:
        return
    h = reference.scene(aabbs)
    g_ref = GridArrays(params)
    reference.bin(h, g_ref)
    assert g_ref.dump() == g_or.dump()
    gb_ref = reference.primary(h, g_ref)
    assert gb_ref.tobytes() == gb_or.tobytes()
    fb_ref, br_ref, lit_ref = reference.shade(g_ref, gb_ref, light)
    fb_own = reference.shade_own(g_ref, gb_ref, light)
    reference.scene_free(h)
    assert fb_own.tobytes() == fb_or.tobytes()
    assert fb_own.tobytes() == fb_ref.tobytes()
    assert fb_ref.tobytes() == fb_or.tobytes()
    assert br_ref.tobytes() == br_or.tobytes()
    assert lit_ref.tobytes() == lit_or.tobytes()


def test_shadow_walk_direct(oracle, reference, ref_checks, T):
    aabbs, walks = shadow_walk_cases()
    params = T.default_params()
    g = oracle.bin(params, aabbs)
    assert sha(np.frombuffer(g.dump(), dtype=np.uint8)) == ref_checks["shadow_walk_grid"]
    exp = ref_checks["shadow"]
    assert len(exp) == len(walks) == 3000 and 0 < int(exp.sum()) < len(exp)
    for i, (s, e, ent, ray) in enumerate(walks):
        got = oracle.shadow(g, s, e, ent, ray)
        assert got == int(exp[i]), i
        if reference is not None:
            assert got == reference.shadow(g, s, e, ent, ray), i


def test_reference_own_shading_loop_on_the_golden_frames(oracle, reference, ref_checks, golden_frames, T):
    """alt:702-760 and alt:763-772 compiled from where they lie (ref_shade_own / ref_debug_line_own): the oracle's
    RGBA frame of every golden case equals the committed hash of the reference's own loop (make_golden.py), and the
    debug lines drawn into it one after another equal the reference's own; live, the reference's loop equals the
    committed hash, the harness replay's frame and the oracle's."""
    params = T.default_params()
    sprite = oracle.tile_floor()
    for name, (m, aabbs, light) in golden_frames.items():
        out = oracle.render(params, aabbs, sprite, light, planes=("fb", "gbuf"))
        gbuf = out["gbuf"]
        assert sha(gbuf) == m["gbuf"], name
        assert sha(out["fb"]) == m["fb"], name
        b = out["fb"].copy()
        for (mx, my), exp in zip(DEBUG_LINE_MICE, ref_checks["debug_lines"][name]):
            oracle.debug_line(params, gbuf, light, mx, my, b)
            assert sha(b) == exp, (name, mx, my)
        if reference is None:
            continue
        h = reference.scene(aabbs)
        g = GridArrays(params)
        reference.bin(h, g)
        gbuf = reference.primary(h, g)
        own = reference.shade_own(g, gbuf, light)
        replay, _, _ = reference.shade(g, gbuf, light)
        reference.scene_free(h)
        assert sha(own) == m["fb"], name
        assert own.tobytes() == replay.tobytes(), name
        assert own.tobytes() == out["fb"].tobytes(), name
        a, b = own.copy(), own.copy()
        for mx, my in DEBUG_LINE_MICE:
            pick = gbuf[my * 480 + mx:my * 480 + mx + 1]
            reference.debug_line_own(pick, mx, my, light, a)
            oracle.debug_line(params, gbuf, light, mx, my, b)
            assert a.tobytes() == b.tobytes(), (name, mx, my)
