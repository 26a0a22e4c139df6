"""The ranged, tinted and relit forms of the light kernel over the 64 scenes of test_gpu_lights_edges.sweep_cases: bin
sizes 8 .. 64, views that are no multiple of the bin or narrower than one, 1 .. 8 lights inside and outside the view,
and three sprite tables. Every expected frame comes from the pinned oracle's per-light planes through the composers
the suite already has (test_gpu_lights.compose, light_range.compose_ranged, light_tints.compose_tinted); the pair
counts of the range cull from light_range.pair_counts over the oracle's hash and the table's depth range. Every
comparison is byte for byte on all planes.

A sweep case is extended in case order from np.random.default_rng(20261017): per light one random(), below 0.25 the
radius is 0 (unbounded), else one integers(max(8, B), (W + H + L) // 2 + 1); then one integers(0, 8, n_lights) into
PALETTE. The sprite table goes by case % 4: 0 and 3 tile_floor alone; 1 tile_floor and a sprite with the colours
shifted and the depths reversed, on the even entities; 2 tile_floor and a sprite with depths 95 / -70 (covered pixels
start in bins without primitives and outside the grid), on every third entity.

test_the_sweep_does_not_pass_vacuously states, without a GPU, what the cases must contain for the GPU tests to mean
something; as measured:
- cases in which a ranged light of index 0 .. 7 has covered pixels out of range / in range and lit / in range and
  shadowed: [46, 23, 21], [47, 27, 23], [40, 24, 20], [29, 21, 18], [22, 12, 8], [13, 7, 4], [7, 5, 4], [5, 4, 3];
- pairs that the slot records cull and the bin alone does not, per bin size: 8: 190 in 5 cases, 16: 12 in 3, 20: 109 in
  6, 24: 143 in 5, 32: 11 in 3, 40: 257 in 16, 48: 21 in 1, 64: 83 in 9; in total 826 of 110 747 culled pairs (of
  203 664 pairs), in 48 cases;
- every pair culled and no shadow ray: cases 12, 26, 39, 45, 58, 61; no pair culled: cases 3, 29, 33, 46, 56;
- table 2: with tile_floor's depth range in place of the table's the culled pairs differ in 12 of the 16 cases (case 2:
  3 404 against 3 488; case 10: 21 938 against 21 999), and all 16 have covered pixels with z outside [0, length);
- at most 20 occupied bins in a column (the light kernel records 64: the pair counts are deterministic);
- covered pixels with unequal fb channels in 50 of the 64 cases.
"""
import functools

import numpy as np
import pytest

import light_range as LR
import light_tints as LT
from test_gpu_light_range import lights_with
from test_gpu_lights import compose, oracle_planes
from test_gpu_lights_edges import SWEEP_CASES, sweep_cases
from test_gpu_lights_graph import Planes, replay
from test_gpu_parity import ALL, assert_planes_equal

STATE_SEED = 20261017
PALETTE = [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2.5, .5, 0), (0, 0, 0), (.25, .75, 1.5), (1, 1, 0)]
BLOCKS = 8
LIT = ("fb", "brightness", "lit")  # what a relit frame writes
BIN_SIZES = (8, 16, 20, 24, 32, 40, 48, 64)
LIGHT_NB = 64  # PAR_LIGHT_NB: the occupied bins of a column whose walks the light kernel records


def sprite_table(par, case, n):
    """(sprites, sprite ids or None) of a case with n entities."""
    s0 = par.tile_floor()
    if case % 4 == 1:
        s1 = s0.copy()
        s1["color"][0] = (s1["color"][0] + 1) % 4
        s1["depth"][0] = s1["depth"][0][::-1]
        return np.concatenate([s0, s1]), (np.arange(n) % 2 == 0).astype(np.int32)
    if case % 4 == 2:
        s2 = s0.copy()
        s2["depth"][0][:400] = 95
        s2["depth"][0][400:] = -70
        return np.concatenate([s0, s2]), (np.arange(n) % 3 == 0).astype(np.int32)
    return s0, None


def bin_culled(params, count, lights, rows=None):
    """How many (start bin, light) pairs of LR.pair_counts the bin's slab alone culls, without the slot records."""
    gx, gy, gz = params.grid_dims()
    B, H = params.bin_size, params.height
    r0, r1 = rows or (0, H)
    c = np.asarray(count).reshape(gx, gy, gz)
    ranged = [((int(L["x"]), int(L["y"]), int(L["z"])), int(L["radius"])) for L in lights if int(L["radius"]) > 0]
    culled = 0
    for bx in range(gx):
        for by in range(r0 // B, (r1 - 1) // B + 1):
            for bz in np.nonzero(c[bx, by])[0]:
                for at, radius in ranged:  # (an unbounded light is never culled)
                    culled += bool(LR.pair_culled(B, H, bx, by, int(bz), at, radius))
    return culled


class Case:
    """One case of the sweep in its full state, and what the oracle and the composers say about it (each computed once,
    on first use, and left unchanged)."""

    def __init__(self, par, T, oracle, case, params, aabbs, pos, rows, radii, tint_ids):
        self.T, self.oracle = T, oracle
        self.case, self.params, self.aabbs, self.pos, self.rows = case, params, aabbs, pos, rows
        self.radii, self.tint_ids = radii, tint_ids
        self.sprites, self.ids = sprite_table(par, case, len(aabbs))
        self.depths = LR.depth_range(self.sprites)
        self.lights = lights_with(T, pos, radii)
        self.tints = [PALETTE[i] for i in tint_ids]
        self.tag = (f"case {case}: {params.width}x{params.height}x{params.length} bin {params.bin_size}, {len(aabbs)} "
                    f"primitives, table {case % 4}, lights {pos} radii {radii} tints {tint_ids}")

    @functools.cached_property
    def outs(self):
        return oracle_planes(self.oracle, self.params, self.aabbs, self.sprites, self.lights, self.ids)

    @functools.cached_property
    def grid(self):
        return self.oracle.bin(self.params, self.aabbs)

    @functools.cached_property
    def full(self):
        """(expected planes, the composer's info) of the ranged and tinted frame."""
        return LT.compose_tinted(self.params, self.outs, self.lights, self.tints, ranged=True)

    @functools.cached_property
    def ranged(self):
        """(expected planes, per light (in range, lit) over the covered pixels, their indices, rays), untinted."""
        return LR.compose_ranged(self.params, self.outs, self.lights)

    @functools.cached_property
    def tinted(self):
        return LT.compose_tinted(self.params, self.outs, self.lights, self.tints, ranged=False)[0]

    @functools.cached_property
    def plain(self):
        return compose(self.params, self.outs, self.lights)[0]

    @functools.cached_property
    def pairs(self):
        return LR.pair_counts(self.params, self.grid.count, self.grid.bins, self.lights, self.depths)

    @functools.cached_property
    def pairs_of_rows(self):
        return LR.pair_counts(self.params, self.grid.count, self.grid.bins, self.lights, self.depths, self.rows)

    @functools.cached_property
    def rays_of_rows(self):
        """The (covered pixel, light) pairs in range or unbounded, of the case's rows alone."""
        _, per_light, idx, _ = self.ranged
        W = self.params.width
        in_rows = (idx >= self.rows[0] * W) & (idx < self.rows[1] * W)
        return sum(int((in_range & in_rows).sum()) for in_range, _ in per_light)

    @functools.cached_property
    def staged(self):
        """(lights, expected planes) of the state a graph is staged to: the lights reversed, the radii rotated by one."""
        n = len(self.pos)
        lights = lights_with(self.T, self.pos[::-1], self.radii[1:] + self.radii[:1])
        order = list(range(n))[::-1]
        outs = [dict(self.outs[0], lit=self.outs[i]["lit"]) if k == 0 else self.outs[i] for k, i in enumerate(order)]
        return lights, LT.compose_tinted(self.params, outs, lights, self.tints, ranged=True)[0]


_cases = []


def cases(par, T, oracle):
    """The cases of the sweep in their full state, shared by every test of this module."""
    if not _cases:
        rng2 = np.random.default_rng(STATE_SEED)
        for case, params, aabbs, pos, rows in sweep_cases(par, T):
            reach = (params.width + params.height + params.length) // 2 + 1
            radii = []
            for _ in pos:
                radii.append(0 if rng2.random() < 0.25 else int(rng2.integers(max(8, params.bin_size), reach)))
            tint_ids = [int(i) for i in rng2.integers(0, 8, len(pos))]
            _cases.append(Case(par, T, oracle, case, params, aabbs, pos, rows, radii, tint_ids))
        assert len(_cases) == SWEEP_CASES and SWEEP_CASES % BLOCKS == 0
    return _cases


def rows_of(planes, params, rows, keys):
    W = params.width
    return {k: planes[k][rows[0] * W:rows[1] * W] for k in keys}


# ---- the GPU tests -----------------------------------------------------------------------------------------------

def set_full_state(par, T, r, c, lights=None):
    r.set_light_model(par.LIGHTS_RANGED)
    r.set_light_tints(T.make_tints(c.tints))
    r.set_lights(c.lights if lights is None else lights)


def check_counts(r, c, rays, pairs, tag):
    pairs, culled = pairs
    assert r.stats().shadow_rays == rays, f"{tag}: shadow_rays {r.stats().shadow_rays}, the composer says {rays}"
    walked, cut = r.light_walks()
    print(f"{tag}: {rays} shadow rays, pairs walked {walked}, culled {cut} of {pairs}")
    assert walked + cut == pairs, f"{tag}: walked {walked} + culled {cut} != {pairs} pairs"
    assert cut == culled, f"{tag}: culled {cut}, the host restatement says {culled}"


def check_case(par, T, r, c):
    params, tag, count_rays = c.params, c.tag, par.RENDER_COUNT_RAYS
    full, info = c.full
    r.set_sprites(c.sprites)
    r.set_entities(c.aabbs, c.ids)
    # 1. ranged and tinted: the full state
    set_full_state(par, T, r, c)
    assert_planes_equal(r.render(ALL, flags=count_rays), full, ALL, f"{tag}, ranged and tinted")
    check_counts(r, c, info["rays"], c.pairs, f"{tag}, ranged and tinted")
    count, _, bins = r.read_grid()
    assert LR.pair_counts(params, count, bins, c.lights, c.depths) == c.pairs, f"{tag}: pair counts of the device's hash"
    got = r.render(ALL, rows=c.rows, flags=count_rays)
    assert_planes_equal(got, rows_of(full, params, c.rows, ALL), ALL, f"{tag}, ranged and tinted, rows {c.rows}")
    check_counts(r, c, c.rays_of_rows, c.pairs_of_rows, f"{tag}, ranged and tinted, rows {c.rows}")
    # 2. the other states in the same context: ranged untinted, unbounded tinted, unbounded untinted
    r.set_light_tints(None)
    assert_planes_equal(r.render(ALL), c.ranged[0], ALL, f"{tag}, ranged, untinted")
    r.set_light_model(par.LIGHTS_UNBOUNDED)
    r.set_light_tints(T.make_tints(c.tints))
    assert_planes_equal(r.render(ALL), c.tinted, ALL, f"{tag}, unbounded, tinted")
    r.set_light_tints(None)
    assert_planes_equal(r.render(ALL), c.plain, ALL, f"{tag}, unbounded, untinted")
    # 3. that frame relit in the full state
    set_full_state(par, T, r, c)
    assert_planes_equal(r.relight(LIT), full, LIT, f"{tag}, relit")
    assert_planes_equal(r.relight(LIT, rows=c.rows), rows_of(full, params, c.rows, LIT), LIT, f"{tag}, relit rows {c.rows}")
    assert_planes_equal(r.relight(LIT, flags=count_rays), full, LIT, f"{tag}, relit, counted")
    check_counts(r, c, info["rays"], c.pairs, f"{tag}, relit")
    # 4. graph replay
    if c.case % 4 == 1:
        import torch
        stream = torch.cuda.Stream()
        out = Planes(params, ALL)
        r.graph_capture_lights(out.ptrs, stream=stream.cuda_stream)
        for k in range(2):  # (both grid sets' graphs)
            assert_planes_equal(replay(r, out, stream, T), full, ALL, f"{tag}, replay {k}")
        lights, staged = c.staged
        r.graph_stage(lights=lights)
        for k in range(2):
            assert_planes_equal(replay(r, out, stream, T), staged, ALL, f"{tag}, lights reversed and staged, replay {k}")
    r.stats()  # raises on PAR_ERR_DEVICE


@pytest.mark.gpu
@pytest.mark.parametrize("block", range(BLOCKS))
def test_light_states_over_the_sweep(par, oracle, T, block):
    refused = []
    n = SWEEP_CASES // BLOCKS
    for c in cases(par, T, oracle)[block * n:(block + 1) * n]:
        try:
            r = par.Renderer(c.params)
        except par.ParError as e:
            refused.append((c.tag, str(e)))
            continue
        with r:
            check_case(par, T, r, c)
    assert not refused, f"par_create refused {len(refused)} cases: {refused[:3]}"


# ---- what keeps the sweep from passing vacuously (no GPU) --------------------------------------------------------

def test_the_sweep_does_not_pass_vacuously(par, oracle, T):
    all_cases = cases(par, T, oracle)
    classes = np.zeros((8, 3), dtype=int)  # cases in which light index l, ranged, has: out of range / lit / shadowed
    by_records = {b: [0, 0] for b in BIN_SIZES}  # bin size: [pairs only the records cull, cases with such pairs]
    pairs_total = culled_total = 0
    all_culled, none_culled, depth_range_shows, outside_grid, coloured = [], [], [], [], []
    most_occupied = 0
    for c in all_cases:
        params = c.params
        one, _ = compose(params, c.outs[:1], c.lights[:1])
        assert_planes_equal(one, c.outs[0], LIT, f"{c.tag}: the composer restates the oracle's one-light frame")
        full, info = c.full
        _, per_light, idx, rays = c.ranged
        assert rays == info["rays"]
        for l, (in_range, lit) in enumerate(per_light):
            if c.radii[l] > 0:
                classes[l] += [(~in_range).any(), (in_range & lit).any(), (in_range & ~lit).any()]
        pairs, culled = c.pairs
        only_records = culled - bin_culled(params, c.grid.count, c.lights)
        assert only_records >= 0
        by_records[params.bin_size][0] += only_records
        by_records[params.bin_size][1] += only_records > 0
        pairs_total += pairs
        culled_total += culled
        if pairs and culled == pairs and rays == 0:
            all_culled.append(c.case)
        if pairs and culled == 0:
            none_culled.append(c.case)
        z = c.outs[0]["gbuf"]["z"][idx].astype(np.int64)
        if c.case % 4 == 2:
            floor_depths = LR.depth_range(c.sprites[:1])
            assert floor_depths != c.depths
            other = LR.pair_counts(params, c.grid.count, c.grid.bins, c.lights, floor_depths)
            if other != c.pairs:
                depth_range_shows.append((c.case, c.pairs[1], other[1]))
            if ((z < 0) | (z >= params.length)).any():
                outside_grid.append(c.case)
        count3 = np.asarray(c.grid.count).reshape(params.grid_dims())
        most_occupied = max(most_occupied, int((count3 != 0).sum(axis=2).max()))
        fb = full["fb"][idx]
        if ((fb["red"] != fb["green"]) | (fb["green"] != fb["blue"])).any():
            coloured.append(c.case)
    only_total = sum(v[0] for v in by_records.values())
    print(f"cases per light index with covered pixels out of range / in range and lit / in range and shadowed: "
          f"{classes.tolist()}; fewest {int(classes.min())}")
    print(f"pairs only the records cull, per bin size [pairs, cases]: {by_records}; in total {only_total} of "
          f"{culled_total} culled pairs ({pairs_total} pairs), in {sum(v[1] for v in by_records.values())} cases")
    print(f"every pair culled and no ray: cases {all_culled}; no pair culled: cases {none_culled}")
    print(f"table 2, culled pairs with the table's depth range / with tile_floor's: {depth_range_shows}")
    print(f"table 2, covered pixels with z outside the grid: cases {outside_grid}")
    print(f"most occupied bins in a column: {most_occupied}")
    print(f"covered pixels with unequal fb channels in {len(coloured)} of {len(all_cases)} cases")
    assert (classes > 0).all(), f"every ranged light index needs each class of covered pixels in some case: {classes.tolist()}"
    for b, (n, _) in by_records.items():
        assert n > 0, f"bin size {b}: no case in which the records cull a pair that the bin alone does not"
    assert all_culled and none_culled
    assert depth_range_shows, "no table-2 case tells the table's depth range from tile_floor's"
    assert outside_grid, "no table-2 case has covered pixels that start outside the grid"
    assert most_occupied <= LIGHT_NB, "the pair counts are deterministic only while every occupied bin is recorded"
    assert 2 * len(coloured) >= len(all_cases)
