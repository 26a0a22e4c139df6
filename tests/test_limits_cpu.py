"""What the scenes of tests/limits.py reach, held on the CPU with the oracle alone, so that test_gpu_limits.py compares
frames that really lie at the limits: covered pixels in bin column, bin row and z bin 1023 (or the last of the axis), lit
and shadowed ones among them, boxes whose sums leave int16 on screen, culled boxes nowhere, a wrapped slot counter and a
column over its record. And the two helpers the GPU tests lean on, held to the oracle's whole-frame entries: the row-block
oracle and the shadow rays of the covered pixels alone."""
import numpy as np
import pytest

import limits as LM
import sequences as SQ
import sprites as SP

T = LM.T


# ---- the helpers against the oracle's whole-frame entries ------------------------------------------------------------

@pytest.mark.parametrize("rows", [(0, 17), (33, 90), (101, 120)])
def test_the_block_oracle_equals_the_whole_frame(oracle, rows):
    params, aabbs, light = SP.scene("odd")  # 200 x 120, bin 16: no multiple of its bin
    sprites, ids = SP.table(oracle.tile_floor(), "two", SP.SPRITE_SEED, len(aabbs))
    whole = oracle.render(params, aabbs, sprites, light, ids)
    assert (whole["lit"] == 0).any() and (whole["lit"] == 1).any()
    W = params.width
    for nthreads in (1, 3):
        got = LM.render_block(params, oracle.bin(params, aabbs), sprites, ids, light, rows, nthreads=nthreads)
        for k in LM.ALL:
            exp = whole[k][rows[0] * W:rows[1] * W]
            assert len(got[k]) == len(exp) and got[k].tobytes() == exp.tobytes(), f"plane {k}, rows {rows}"
    covered = whole["palidx"][rows[0] * W:rows[1] * W] != T.PALIDX_BACKGROUND
    assert covered.any() and not covered.all()
    # the shading alone, over the block's G-buffer
    again = LM.render_block(params, oracle.bin(params, aabbs), sprites, ids, light, rows, ("fb", "brightness", "lit"),
                            gbuf=got["gbuf"])
    for k in ("fb", "brightness", "lit"):
        assert again[k].tobytes() == got[k].tobytes(), k


@pytest.mark.parametrize("view,end", [("int16 deep", "x-"), ("int16 deep", "z+"), ("int16 deep", "y-")])
def test_the_shadow_rays_of_covered_pixels_restate_the_oracle(view, end):
    at = LM.end_lights(view)[end]
    for rows, planes in LM.lit_frame(view, at).items():
        m = LM.covered(planes)
        got = LM.covered_lit(view, at)[rows]
        assert np.array_equal(got[m], planes["lit"][m]) and not got[~m].any()
        assert (got[m] == 1).any() and (got[m] == 0).any(), "lit and shadowed pixels"


# ---- the scenes ------------------------------------------------------------------------------------------------------

def test_the_views_have_the_grids_of_their_names():
    for view, (W, H, L, B, axes, blocks) in LM.VIEWS.items():
        dims = LM.params_of(view).grid_dims()
        assert dims == LM.GRIDS[view]
        for axis, d in zip("xyz", dims):
            assert (d == 1024) == (axis in axes), view
    assert LM.VIEWS["int16 wide"][0] == LM.VIEWS["int16 tall"][1] == LM.VIEWS["int16 deep"][2] == 32767
    assert 32767 - 1023 * 32 == 31  # the last bin column of the int16 wide view is 31 pixels wide


def last_bin_masks(view, rows, planes):
    gx, gy, gz = LM.GRIDS[view]
    _, _, bx, by, bz = LM.where(view, rows, planes)
    c = LM.covered(planes)
    return {"bin column": c & (bx == gx - 1), "bin row": c & (by == gy - 1), "z bin": c & (bz == gz - 1)}


@pytest.mark.parametrize("view", list(LM.VIEWS))
def test_scenes_reach_their_situations(view):
    params, aabbs, sprites, ids, info = LM.scene(view)
    gx, gy, gz = LM.GRIDS[view]
    B = params.bin_size
    assert 200 <= len(aabbs) <= 400
    e = np.stack([aabbs[k] for k in ("ex", "ey", "ez")], axis=1)
    assert e[:, 0].min() == 1 and e.max() == 20 and e[:, 1:].min() == 0 and (e[:, 1] + e[:, 2]).max() == 40
    frame = LM.lit_frame(view, LM.default_light(view))
    # covered pixels in the last bin of every axis, lit and shadowed
    counts = {k: 0 for k in ("bin column", "bin row", "z bin")}
    lit = {k: set() for k in counts}
    for rows, planes in frame.items():
        for k, m in last_bin_masks(view, rows, planes).items():
            counts[k] += int(m.sum())
            lit[k] |= set(np.unique(planes["lit"][m]).tolist())
    print(view, counts)
    for k in counts:
        assert counts[k] >= 200, f"{view}: {counts[k]} covered pixels in the last {k}"
        assert lit[k] == {0, 1}, f"{view}: lit values {lit[k]} in the last {k}"
    # the culled boxes leave no pixel and no hash entry
    grid = LM.grid(view)
    live = (np.arange(T.SLOTS)[None, :] < grid.count[:, None]).reshape(-1)
    hashed = set(np.unique(grid.map[live]).tolist())
    seen = set()
    for planes in frame.values():
        seen |= set(np.unique(planes["gbuf"]["entity_index"][LM.covered(planes)]).tolist())
    assert len(info["culled"]) == 8 and not hashed & set(info["culled"]) and not seen & set(info["culled"])
    _, nx, _, ny, nz = SQ.footprints(params, aabbs)
    assert not (nx * ny * nz)[info["culled"]].any()
    # the stack: its bin's counter wrapped, its column over the record
    bx, by, bz = info["stack_bin"]
    assert bx == gx - 1
    x0, _, y0, _, _ = SQ.footprints(params, aabbs)
    z0 = np.maximum(0, aabbs["pz"].astype(np.int64) // B)
    inside = (x0 <= bx) & (bx < x0 + nx) & (y0 <= by) & (by < y0 + ny) & (z0 <= bz) & (bz < z0 + nz)
    assert inside[info["stack"]].all() and len(info["stack"]) == LM.STACK
    inserted, count = int(inside.sum()), int(grid.count[(bx * gy + by) * gz + bz])
    assert inserted > T.SLOTS and count == inserted % T.SLOTS and count != inserted, (inserted, count)  # count wrapped
    assert SQ.column_histograms(params, aabbs)[0] >= 1, "a column over its record"
    # the device's record of a column takes COL_ENT slot records and COL_NB occupied bins; a wrapped counter leaves at most
    # SLOTS - 1 records in a bin, so only the view with many z bins can fill it, and there the stacked column does
    _, most_records, most_bins = SQ.grid_sizes(params, grid)
    assert info["deep_stack"] == (view == "int16 deep")
    if info["deep_stack"]:
        assert int((grid.count.reshape(gx, gy, gz)[bx, by] != 0).sum()) > SQ.COL_NB
    else:
        assert gz * (T.SLOTS - 1) <= SQ.COL_ENT and most_records <= SQ.COL_ENT and most_bins <= SQ.COL_NB
    if view == "wide and tall":
        blocks = LM.blocks_of(view)
        for rows in blocks:
            m = last_bin_masks(view, rows, frame[rows])
            assert m["bin column"].any(), rows
        assert last_bin_masks(view, blocks[-1], frame[blocks[-1]])["bin row"].any()
        assert not last_bin_masks(view, blocks[0], frame[blocks[0]])["bin row"].any()


@pytest.mark.parametrize("view", LM.INT16_VIEWS)
def test_int16_boxes(view):
    """The boxes whose sums leave int16 are in the scene of every int16 view, and on screen in the view of their axis."""
    params, aabbs, _, _, info = LM.scene(view)
    W, H, L, B = LM.VIEWS[view][:4]
    a = {k: aabbs[k].astype(np.int64) for k in ("px", "py", "pz", "ex", "ey", "ez")}
    own = np.zeros(len(aabbs), dtype=bool)
    own[info["int16"]] = True
    assert set(LM.INT16_PX) <= set(a["px"][own].tolist())
    beyond_x = own & (a["px"] + a["ex"] > 32767)
    beyond_rows = own & (a["py"] + a["ey"] + a["pz"] + a["ez"] > 32767) & (a["py"] >= 32700)
    deep = own & (a["py"] == -32768) & (a["pz"] == 32767)
    assert beyond_x.any() and beyond_rows.any() and deep.any()
    frame = LM.lit_frame(view, LM.default_light(view))[(0, H)]
    c = LM.covered(frame)
    seen = set(np.unique(frame["gbuf"]["entity_index"][c]).tolist())
    x, _, _, _, bz = LM.where(view, (0, H), frame)
    if view == "int16 wide":
        assert seen & set(np.nonzero(beyond_x)[0].tolist()), "a box with px + ex > 32767 on screen"
        assert seen & set(np.nonzero(own & (a["px"] == -19))[0].tolist()) and c[x == W - 1].any() and c[x == 0].any()
        lx = LM.end_lights(view)["x-"][0]
        assert (np.abs(lx - x[c]) >= 65000).any(), "|lx - x| >= 65 000 at a covered pixel"
    if view == "int16 tall":
        assert seen & set(np.nonzero(beyond_rows)[0].tolist()), "a box with py + ey + pz + ez > 32767 on screen"
    if view == "int16 deep":
        ents = frame["gbuf"]["entity_index"][c & (bz == 1023)]
        assert set(ents.tolist()) & set(np.nonzero(deep)[0].tolist()), "py = -32768, pz = 32767 in z bin 1023"
