"""GPU parity of frames with several lights at the light kernel's limits and on the host paths of such a frame. Every
expected frame is test_gpu_lights.expected(): one oracle.render per light, composed in numpy float32 by the contract of
par_raytracer.h, after the composer has reproduced the oracle's own one-light planes on the same scene; every
comparison is byte for byte. The capacity scenes first prove on the host, from the oracle's bin counts and the pinned
bin sequence of the shadow walk (helpers.walk_probes, test_lights_walk_cpu.py), that they reach the limit they are
named after, in a column that shows covered pixels."""
import numpy as np
import pytest

from helpers import graybox, light_bin, random_stage_scene, walk_record_bounds
from test_gpu_lights import (PLACEMENTS, assert_lit_and_shadowed, covered_pixel_light, expected, lights_of,
                             render_lights)
from test_gpu_lights_graph import Planes, replay
from test_gpu_parity import ALL, assert_planes_equal

pytestmark = pytest.mark.gpu

# The light kernel's LDS budgets: PAR_BIN_WALK (par_internal.h: records of one walk's stage), PAR_LIGHT_NB and
# PAR_LIGHT_WALK (par_kernels.hip: start bins of a column with recorded walks, records of all walks of a column),
# and PAR_MAX_GRID_DIM (par_internal.h: bins per axis).
BIN_WALK, LIGHT_NB, LIGHT_WALK, MAX_GRID_DIM = 64, 64, 1024, 1024
LIGHT_GRID = 65536  # the most workgroups of a light kernel launch (par_launch_render_lights); they stride beyond it


@pytest.fixture(scope="module")
def sprite(par):
    return par.tile_floor()


def floor(nx, nz, skip=()):
    return [(i * 20, 0, j * 20, 20, 20, 20) for i in range(nx) for j in range(nz) if i not in skip]


# ---- what the expected frame and the oracle's bins say about a column ------------------------------------------

class Columns:
    """The oracle's bin counts of a scene and, from the expected G-buffer, the start bins of its covered pixels. A
    covered pixel of screen row r shows world y + z = H - r, so its shadow rays start in bin
    (x / B, r / B, z / B) (alt:724-727): the tile of column (bx, by) is the B x B pixels at (bx * B, by * B)."""

    def __init__(self, params, oracle, aabbs, exp):
        self.params, self.B = params, params.bin_size
        self.gx, self.gy, self.gz = params.grid_dims()
        self.count = oracle.bin(params, aabbs).count
        self.count3 = self.count.reshape(self.gx, self.gy, self.gz)
        idx = np.nonzero(exp["palidx"] != 0xFF)[0]
        z = exp["gbuf"]["z"][idx].astype(np.int64)
        keep = z >= 0
        self.idx = idx[keep]
        self.bx = (self.idx % params.width) // self.B
        self.by = (self.idx // params.width) // self.B
        self.bz = z[keep] // self.B

    def occupied(self, bx, by):
        return np.nonzero(self.count3[bx, by])[0]

    def in_tile(self, bx, by):
        return (self.bx == bx) & (self.by == by)

    def pixels_starting_in(self, bx, by, bz):
        return int((self.in_tile(bx, by) & (self.bz == bz)).sum())

    def shown_columns(self):
        """(bx, by) of every column whose tile shows covered pixels."""
        return sorted({(int(x), int(y)) for x, y in zip(self.bx, self.by)})

    def bounds(self, bx, by, bz, light_pos):
        return walk_record_bounds(self.count, (bx, by, bz), light_bin(self.params, light_pos), self.gy, self.gz)


def mixed_stage_places(cols, positions):
    """(column, start bin, lights whose walk surely fits a stage, lights whose walk surely does not, pixels) of every
    occupied start bin with covered pixels whose walks take both paths."""
    out = []
    for bx, by in cols.shown_columns():
        for bz in cols.occupied(bx, by):
            n_px = cols.pixels_starting_in(bx, by, bz)
            if n_px == 0:
                continue
            b = [cols.bounds(bx, by, int(bz), p) for p in positions]
            fits = [l for l, (lo, hi) in enumerate(b) if hi <= BIN_WALK]
            too_long = [l for l, (lo, hi) in enumerate(b) if lo > BIN_WALK]
            if fits and too_long:
                out.append(((bx, by), int(bz), fits, too_long, n_px))
    return out


def walk_area_demand(cols, bx, by, positions):
    """(occupied bins, sum of the lower bounds of the records of the (bin, light) walks that surely fit a stage)."""
    occ = cols.occupied(bx, by)
    total = 0
    for bz in occ:
        for p in positions:
            lo, hi = cols.bounds(bx, by, int(bz), p)
            if hi <= BIN_WALK:
                total += lo
    return len(occ), total


def covered_occupied_start_bins(cols, bx, by):
    """The distinct occupied bins of column (bx, by) in which covered pixels of its tile start."""
    bz = np.unique(cols.bz[cols.in_tile(bx, by)])
    bz = bz[bz < cols.gz]
    return bz[cols.count3[bx, by, bz] != 0]


def render_three_times(par, params, aabbs, sprite, lights, exp, tag):
    """Which (bin, light) walks get recorded depends on the order of the wavefronts: three renders in one context."""
    with par.Renderer(params) as r:
        r.set_sprites(sprite)
        r.set_entities(aabbs)
        r.set_lights(lights)
        for k in range(3):
            assert_planes_equal(r.render(ALL), exp, ALL, f"{tag}, render {k}")
        r.stats()


# ---- 1. capacity edges with several lights -----------------------------------------------------------------------

def mixed_stage_scene(T):
    """The long-walk scene of test_light_kernel_crowded_columns_and_long_walks: seven boxes in each of the twelve bins
    of one row, on a floor."""
    params = T.default_params(480, 320, 320)
    rows = [(40 * bx + 2 * k, 100, 100, 20, 20, 20) for bx in range(12) for k in range(7)]
    return params, T.make_aabbs(rows + floor(24, 16))


MIXED_STAGE_LIGHTS = [(470, 110, 110), (5, 110, 110), (240, 300, 20), (240, 100, 150), (20, 300, 10), (400, 80, 200),
                      (100, 200, 300), (300, 20, 60)]


@pytest.mark.parametrize("n", [2, 4, 8])
def test_mixed_stage_fits_within_one_start_bin(par, oracle, sprite, T, n):
    """One pixel takes a recorded walk towards one light and lane_shadow_walk towards another. As written, the scene
    has 8 / 12 / 35 such (column, start bin) places with 2 / 4 / 8 lights: e.g. column (0, 2), start bin 2, 1 280
    covered pixels, where the walk towards (470, 110, 110) surely exceeds a stage and the others surely fit."""
    params, aabbs = mixed_stage_scene(T)
    pos = MIXED_STAGE_LIGHTS[:n]
    lights = lights_of(T, pos)
    exp, per_light = expected(params, oracle, aabbs, sprite, lights, tag=f"mixed stage n={n}")
    cols = Columns(params, oracle, aabbs, exp)
    places = mixed_stage_places(cols, pos)
    print(f"mixed stage n={n}: {len(places)} (column, start bin) places; first "
          f"{[(c, bz, f, t, px) for c, bz, f, t, px in places[:3]]}")
    assert places, (f"mixed stage n={n}: no start bin of any shown column {cols.shown_columns()} has a walk that surely "
                    f"fits a stage towards one light and surely does not towards another")
    assert_lit_and_shadowed(per_light[:2], f"mixed stage n={n}")
    render_three_times(par, params, aabbs, sprite, lights, exp, f"mixed stage n={n}")


def walk_area_scene(T):
    """Bin 8: a stair of 58 boxes through one screen column, over a floor."""
    params = T.default_params(480, 320, 480, 8)
    rows = [(200 + k % 3, 300 - 8 * k, 8 * k + 1, 20, 20, 20) for k in range(58)]
    return params, T.make_aabbs(rows + floor(24, 24))


WALK_AREA_LIGHTS = [(20, 300, 310), (470, 10, 470), (300, 160, 80), (230, 60, 10), (240, 310, 300), (5, 5, 5),
                    (470, 300, 20), (100, 100, 100)]
WALK_AREA_COLUMNS = [(25, 0), (25, 1), (25, 2), (26, 0), (26, 1), (26, 2)]


def walk_area_columns(cols, pos):
    """The candidate columns that show covered pixels, have at most PAR_LIGHT_NB occupied bins, and whose surely
    fitting walks need more records than the walk area holds."""
    found = []
    for bx, by in WALK_AREA_COLUMNS:
        n_occ, demand = walk_area_demand(cols, bx, by, pos)
        n_px = int(cols.in_tile(bx, by).sum())
        if n_occ <= LIGHT_NB and demand > LIGHT_WALK and n_px:
            found.append(((bx, by), n_occ, demand, n_px))
    return found


@pytest.mark.parametrize("n", [2, 4, 8])
def test_walk_area_exhausted_with_at_most_64_occupied_bins(par, oracle, sprite, T, n):
    """Walks that fit a stage are refused by the walk area. As written, the columns (25, 0) .. (26, 2) have 60 occupied
    bins and 64 covered pixels each, and their surely fitting walks need at least 1 042 .. 2 302 records with 2 lights,
    1 751 .. 2 755 with 4 and 3 920 .. 5 280 with 8, against an area of 1 024."""
    params, aabbs = walk_area_scene(T)
    pos = WALK_AREA_LIGHTS[:n]
    lights = lights_of(T, pos)
    exp, per_light = expected(params, oracle, aabbs, sprite, lights, tag=f"walk area n={n}")
    cols = Columns(params, oracle, aabbs, exp)
    found = walk_area_columns(cols, pos)
    print(f"walk area n={n}: (column, occupied bins, records of the surely fitting walks, covered pixels) {found}")
    assert found, (f"walk area n={n}: none of the columns {WALK_AREA_COLUMNS} has <= {LIGHT_NB} occupied bins, covered "
                   f"pixels and surely fitting walks of more than {LIGHT_WALK} records")
    render_three_times(par, params, aabbs, sprite, lights, exp, f"walk area n={n}")


MANY_BINS_COLUMN = (12, 5)
MANY_BINS_LIGHTS = [(300, 200, 640), (60, 100, 100), (210, 160, 1270), (470, 300, 20), (200, 10, 900), (5, 100, 400),
                    (250, 250, 100), (400, 60, 1100)]


def many_bins_scene(T):
    """Bin 16, 80 bins deep: eighty one-pixel-wide boxes, one per z bin, all within the tile of one screen column;
    20-cubes elsewhere in the volume and a floor strip stand between them and the lights."""
    params = T.default_params(480, 320, 1280, 16)
    rows = []
    for k in range(80):
        q, pz = k // 16, 16 * k + 2
        rows.append((192 + k % 16, 317 - (80 + 3 * q) - pz, pz, 1, 1, 2))
    rng = np.random.default_rng(5)
    for _ in range(260):
        x, z = int(rng.integers(0, 460)), int(rng.integers(0, 1260))
        y = int(rng.integers(0, 300))
        if 150 <= x < 250 and 200 <= y + z <= 360:
            continue  # (keep the stair's own screen rows free)
        rows.append((x, y, z, 20, 20, 20))
    rows += [(i * 20, 0, j * 20, 20, 20, 20) for i in range(24) for j in range(0, 64, 3)]
    return params, T.make_aabbs(rows)


@pytest.mark.parametrize("n", [2, 8])
def test_more_than_64_occupied_bins_in_a_column(par, oracle, sprite, T, n):
    """Whichever 64 bins get recorded walks, covered pixels start in others. As written, column (12, 5) has 80 occupied
    bins and its 240 covered pixels start in 79 distinct occupied bins; every light reaches some of them only."""
    params, aabbs = many_bins_scene(T)
    pos = MANY_BINS_LIGHTS[:n]
    lights = lights_of(T, pos)
    exp, per_light = expected(params, oracle, aabbs, sprite, lights, tag=f"many bins n={n}")
    cols = Columns(params, oracle, aabbs, exp)
    bx, by = MANY_BINS_COLUMN
    n_occ = len(cols.occupied(bx, by))
    starts = covered_occupied_start_bins(cols, bx, by)
    print(f"many bins n={n}: column {(bx, by)} has {n_occ} occupied bins; its {int(cols.in_tile(bx, by).sum())} "
          f"covered pixels start in {len(starts)} distinct occupied bins")
    assert n_occ > LIGHT_NB and len(starts) > LIGHT_NB, (
        f"many bins n={n}: column {(bx, by)} has {n_occ} occupied bins and covered pixels starting in {len(starts)} "
        f"distinct occupied bins; both must exceed {LIGHT_NB}")
    in_col = cols.in_tile(bx, by)
    covered = np.nonzero(exp["palidx"] != 0xFF)[0]
    sel = np.isin(covered, cols.idx[in_col])
    assert_lit_and_shadowed([v[sel] for v in per_light], f"many bins n={n}, column {(bx, by)}")
    render_three_times(par, params, aabbs, sprite, lights, exp, f"many bins n={n}")


def test_deepest_grid(par, oracle, sprite, T):
    """gz = PAR_MAX_GRID_DIM: the per-column tables are full length. As written, covered pixels start up to z bin
    1 018."""
    params = T.default_params(64, 48, 8 * MAX_GRID_DIM, 8)
    assert params.grid_dims()[2] == MAX_GRID_DIM
    # sixteen boxes side by side on the screen (row = H - y - z), one every 540 units of depth, the last in z bin 1016
    rows = []
    for k in range(16):
        z = 30 + 540 * k
        rows.append((8 * (k % 8), 4 + 22 * (k // 8) - z, z, 8, 8, 10))
    rows += [(20, -4000, 4010, 20, 20, 20), (40, -6990, 7000, 20, 3, 20)]  # (in front of some of them)
    aabbs = T.make_aabbs(rows)
    pos = [(30, 20, 60), (60, -4000, 4100), (32, -9000, 9500)]  # the last one beyond the far end
    lights = lights_of(T, pos)
    exp, per_light = expected(params, oracle, aabbs, sprite, lights, tag="deepest grid")
    cols = Columns(params, oracle, aabbs, exp)
    assert len(cols.bz) and int(cols.bz.max()) > 1000, "covered pixels must start deeper than z bin 1000"
    print(f"deepest grid: covered pixels start in z bins up to {int(cols.bz.max())}")
    render_three_times(par, params, aabbs, sprite, lights, exp, "deepest grid")


def test_crowded_columns_with_eight_lights(par, oracle, sprite, T):
    """The overflow scene of test_light_kernel_crowded_columns_and_long_walks, taken to eight lights."""
    params = T.default_params(480, 320, 640)
    rng = np.random.default_rng(2)
    rows = [(int(rng.integers(200, 260)), int(rng.integers(0, 40)), int(z), 20, 20, 20) for z in rng.integers(0, 300, 500)]
    rows += floor(24, 16, skip=range(4, 8))
    rows += [(100 + k, 290 - 40 * b, 40 * b + 10, 20, 20, 20) for b in range(16) for k in range(7)]
    aabbs = T.make_aabbs(rows)
    pos = [(300, 160, 80), (230, 60, 10), (20, 300, 600), (470, 20, 630), (240, 310, 320), (5, 5, 5), (470, 300, 20),
           (110, 150, 330)]
    lights = lights_of(T, pos)
    exp, per_light = expected(params, oracle, aabbs, sprite, lights, tag="crowded")
    assert_lit_and_shadowed(per_light, "crowded")
    render_three_times(par, params, aabbs, sprite, lights, exp, "crowded n=8")


def strided_columns_scene(par, T):
    """Bin 8, 270 x 270 screen columns, nearly all of them occupied: 108 x 54 cubes tile the screen (a cube shows on 40
    rows), each at a depth of its own, so that the columns a workgroup takes one after the other occupy different z
    bins. Every other cube has a sprite whose depths lie far outside the box: its pixels start in bins that hold no
    primitive in their own column."""
    params = T.default_params(2160, 2160, 160, 8)
    rng = np.random.default_rng(12)
    rows = []
    for i in range(108):
        for j in range(54):
            z = int(rng.integers(0, 140))
            rows.append((20 * i, 40 * j - z, z, 20, 20, 20))
    s0 = par.tile_floor()
    s1 = s0.copy()
    s1["depth"][0][:400] = 63
    s1["depth"][0][400:] = -45
    aabbs = T.make_aabbs(rows)
    return params, aabbs, np.concatenate([s0, s1]), (np.arange(len(aabbs)) % 2).astype(np.int32)


def test_more_occupied_columns_than_workgroups(par, oracle, T):
    """A launch has at most 65536 workgroups; with more occupied columns a workgroup takes several, one after the other
    in the same LDS: what the previous column left there (zslot, wcnt, woff, the walk area) must not be read."""
    params, aabbs, sprites, ids = strided_columns_scene(par, T)
    pos = [(1100, 900, 70), (300, 2000, 150), (2100, 100, 10)]
    lights = lights_of(T, pos)
    exp, per_light = expected(params, oracle, aabbs, sprites, lights, ids, tag="strided columns")
    cols = Columns(params, oracle, aabbs, exp)
    n_cols = int((cols.count3.sum(axis=2) > 0).sum())
    inside = cols.bz < cols.gz
    empty_start = cols.count3[cols.bx[inside], cols.by[inside], cols.bz[inside]] == 0
    print(f"strided columns: {n_cols} occupied columns; {int(empty_start.sum())} of {len(cols.idx)} covered pixels start "
          f"in a bin without primitives")
    assert n_cols > LIGHT_GRID, f"strided columns: {n_cols} occupied columns, a workgroup takes one at the most"
    assert empty_start.any() and not empty_start.all()
    assert_lit_and_shadowed(per_light, "strided columns")
    with par.Renderer(params) as r:
        r.set_sprites(sprites)
        r.set_entities(aabbs, ids)
        r.set_lights(lights)
        for k in range(2):
            assert_planes_equal(r.render(ALL), exp, ALL, f"strided columns, render {k}")
        r.stats()


# ---- 2. the host paths of a several-light frame (direct renders) -------------------------------------------------

PLANE_SETS = [ALL, ("fb", "palidx"), ("fb",), ("lit",), ("brightness", "gbuf")]


def host_path_scene(par, oracle, sprite, T, world, n):
    """The world and n lights: PLACEMENTS, the light on a covered pixel and, in the graybox world, one light below and
    in front of the floor. The background ray of a screen column starts at (x, 0, 0), inside the graybox floor, which
    blocks it towards every light of PLACEMENTS but (240, 100, 150) at x = 240: without a light the floor does not
    hide, that world shows one non-zero background byte at most."""
    params = T.default_params()
    if world == "graybox":
        aabbs, first, other = graybox(par), T.make_light(480, 160, 80), (240, -50, -30)
    else:
        (aabbs, first), other = random_stage_scene(7), (20, 300, 10)
    on_pixel = covered_pixel_light(params, oracle, aabbs, sprite, first)
    if n == 3:
        pos = [PLACEMENTS[3], other if world == "graybox" else PLACEMENTS[4], on_pixel]
    else:
        pos = ([(480, 160, 80), other] + PLACEMENTS)[:n - 1] + [on_pixel]
    assert len(pos) == n
    return params, aabbs, pos


def background_bytes(exp):
    return np.unique(exp["lit"][exp["palidx"] == 0xFF])


def rows_of(exp, planes, w, r0, r1):
    return {k: exp[k][r0 * w:r1 * w] for k in planes}


@pytest.mark.parametrize("world,n", [("graybox", 3), ("graybox", 8), ("random 7", 3), ("random 7", 8)])
def test_host_paths_of_a_several_light_frame(par, oracle, sprite, T, world, n):
    params, aabbs, pos = host_path_scene(par, oracle, sprite, T, world, n)
    w, h = params.width, params.height
    lights = lights_of(T, pos)
    exp, per_light = expected(params, oracle, aabbs, sprite, lights, tag=f"{world} n={n}")
    bg = background_bytes(exp)
    print(f"{world} n={n}: background bytes of the expected lit plane {[int(b) for b in bg]}")
    assert len(bg[bg != 0]) >= 2, f"{world} n={n}: a misplaced background bit needs two different non-zero bytes: {bg}"
    row_ranges = [None, (37, 251), (0, 1), (h - 1, h), (125, 131)]  # (the last one inside one bin row)
    assert 125 // params.bin_size == 130 // params.bin_size
    with par.Renderer(params) as r:
        r.set_sprites(sprite)
        r.set_entities(aabbs)
        r.set_lights(lights)
        for rows in row_ranges:
            r0, r1 = rows or (0, h)
            for planes in PLANE_SETS:
                for flags in (0, par.RENDER_TRACE_BACKGROUND):
                    got = r.render(planes, rows=rows, flags=flags)
                    assert_planes_equal(got, rows_of(exp, planes, w, r0, r1), planes,
                                        f"{world} n={n} rows {rows} planes {planes} flags {flags}")
        # PAR_RENDER_COUNT_RAYS: one ray per light and covered pixel of the rows rendered
        for r0, r1 in [(37, 251), (125, 131)]:
            got = r.render(("fb", "palidx"), rows=(r0, r1), flags=par.RENDER_COUNT_RAYS)
            assert_planes_equal(got, rows_of(exp, ("fb", "palidx"), w, r0, r1), ("fb", "palidx"), "counted rays")
            covered = int((exp["palidx"][r0 * w:r1 * w] != 0xFF).sum())
            assert covered and r.stats().shadow_rays == n * covered, f"{world} n={n} rows {r0}-{r1}"
        r.stats()


def test_row_blocks_of_the_headline_view_with_four_lights(par, oracle, sprite, T):
    w = h = l = 4096
    params = T.default_params(w, h, l)
    aabbs, _ = par.scene_synthetic(1024, w, h, l, 12345)
    lights = lights_of(T, [(2560, 2048, 1024), (300, 3000, 200), (4000, 100, 3900), (2048, 1500, 2048)])
    planes = ("fb", "palidx", "brightness", "lit")
    exp, per_light = expected(params, oracle, aabbs, sprite, lights, tag="4096 row blocks")
    assert_lit_and_shadowed(per_light, "4096 row blocks")
    with par.Renderer(params) as r:
        r.set_sprites(sprite)
        r.set_entities(aabbs)
        r.set_lights(lights)
        for rank in range(8):
            r0, r1 = par.row_block(rank, 8, h, 40)
            got = r.render(planes, rows=(r0, r1))
            assert_planes_equal(got, rows_of(exp, planes, w, r0, r1), planes, f"4096 n=4 rows {r0}-{r1}")
        r.stats()


# ---- 3. shapes and inputs of the one-light suite, with several lights --------------------------------------------

def frame_equals_composed(par, oracle, T, params, aabbs, sprite, pos, tag, sprite_ids=None):
    lights = lights_of(T, pos)
    exp, per_light = expected(params, oracle, aabbs, sprite, lights, sprite_ids, tag=tag)
    got = render_lights(par, params, aabbs, sprite, lights, ALL, sprite_ids)
    assert_planes_equal(got, exp, ALL, tag)
    return exp, per_light


def light_pos(light):
    return tuple(int(light[0][a]) for a in "xyz")


@pytest.mark.parametrize("bin_size,view", [(8, (480, 320, 320)), (24, (500, 333, 290)), (160, (640, 480, 480))])
def test_bin_sizes_with_three_lights(par, oracle, sprite, T, bin_size, view):
    params = T.default_params(*view, bin_size)
    aabbs, light = par.scene_synthetic(260, *view, bin_size)
    w, h, l = view
    pos = [light_pos(light), (w // 8, h - 20, l // 16), (w - 10, h // 3, l - 30)]
    _, per_light = frame_equals_composed(par, oracle, T, params, aabbs, sprite, pos, f"bin {bin_size} n=3")
    assert_lit_and_shadowed(per_light, f"bin {bin_size}")


@pytest.mark.parametrize("view,n_prims,seed", [((123, 77, 91), 60, 1), ((37, 29, 33), 25, 2)])
def test_odd_widths_and_a_view_smaller_than_a_bin_with_two_lights(par, oracle, sprite, T, view, n_prims, seed):
    w, h, l = view
    params = T.default_params(w, h, l)
    aabbs, _ = par.scene_synthetic(n_prims, w, h, l, seed)
    pos = [(w // 2, h // 2, l // 4), (w - 3, 5, l - 2)]
    exp, _ = frame_equals_composed(par, oracle, T, params, aabbs, sprite, pos, f"{w}x{h}x{l} n=2")
    assert (exp["palidx"] != 0xFF).any() and (exp["palidx"] == 0xFF).any()
    lights = lights_of(T, pos)
    for rows in [(0, 1), (h // 3, h - 1)]:
        got = render_lights(par, params, aabbs, sprite, lights, ALL, rows=rows)
        assert_planes_equal(got, rows_of(exp, ALL, w, *rows), ALL, f"{w}x{h}x{l} n=2 rows {rows}")


def test_sprite_ids_with_three_lights(par, oracle, T):
    params = T.default_params()
    s0 = par.tile_floor()
    s1 = s0.copy()
    s1["color"][0] = (s1["color"][0] + 1) % 4
    s1["depth"][0] = s1["depth"][0][::-1]
    sprites = np.concatenate([s0, s1])
    aabbs, light = random_stage_scene(3)
    ids = (np.arange(len(aabbs)) % 2).astype(np.int32)
    pos = [light_pos(light), (400, 80, 200), (60, 140, 20)]
    _, per_light = frame_equals_composed(par, oracle, T, params, aabbs, sprites, pos, "sprite ids n=3", sprite_ids=ids)
    assert_lit_and_shadowed(per_light, "sprite ids")


def test_unoccupied_start_bins_with_three_lights(par, oracle, T):
    params = T.default_params(480, 320, 320)
    sprite = par.tile_floor()
    sprite["depth"][0][:400] = 95
    sprite["depth"][0][400:] = -70
    aabbs, light = par.scene_synthetic(250, 480, 320, 320, 13)
    aabbs["pz"][:40] = -20
    pos = [light_pos(light), (400, 80, 200), (60, 250, 20)]
    exp, per_light = frame_equals_composed(par, oracle, T, params, aabbs, sprite, pos, "unoccupied start bins n=3")
    assert_lit_and_shadowed(per_light, "unoccupied start bins")
    # the scene is what its name says: covered pixels start in bins that hold no primitive, or outside the grid
    count3 = oracle.bin(params, aabbs).count.reshape(params.grid_dims())
    idx = np.nonzero(exp["palidx"] != 0xFF)[0]
    z = exp["gbuf"]["z"][idx].astype(np.int64)
    inside = (z >= 0) & (z < 320)
    bx, by, bz = (idx % 480) // 40, (idx // 480) // 40, z // 40
    assert (~inside).any() and (count3[bx[inside], by[inside], bz[inside]] == 0).any()


def test_empty_scene_with_eight_lights(par, oracle, sprite, T):
    params = T.default_params()
    aabbs, _ = par.scene_synthetic(0, 480, 320, 320, 7)
    pos = [(240, 160, 80), (480, 160, 80), (20, 300, 10)] + PLACEMENTS
    exp, _ = frame_equals_composed(par, oracle, T, params, aabbs, sprite, pos, "empty scene n=8")
    assert (exp["palidx"] == 0xFF).all()
    lights = lights_of(T, pos)
    for planes, flags in [(("fb",), par.RENDER_TRACE_BACKGROUND), (("fb", "lit"), 0), (("lit",), par.RENDER_TRACE_BACKGROUND)]:
        got = render_lights(par, params, aabbs, sprite, lights, planes, flags=flags)
        assert_planes_equal(got, exp, planes, f"empty scene n=8 planes {planes} flags {flags}")


def test_lights_with_infinite_and_nan_slabs_beside_an_ordinary_light(par, oracle, sprite, T):
    """The placements of test_edge_views_and_lights and test_light_kernel_axis_parallel_light_and_background_rays, two
    to four at a time with (240, 100, 150). A light on a covered pixel makes a 0 / 0 direction there; the composer's
    np.where(0 < dot, dot, 0) states what std::max<float>(0, NaN) gives."""
    ordinary = (240, 100, 150)
    params = T.default_params()
    rows = floor(24, 16) + [(200, 20, 100, 20, 20, 20), (220, 40, 100, 20, 20, 20), (200, 20, 140, 20, 20, 20)]
    planes_scene = T.make_aabbs(rows)
    # on primitives' planes and in their bins
    for pos in [[ordinary, (210, 40, 110), (200, 20, 100), (240, 20, 100)], [(210, 30, 110), ordinary, (0, 20, 0)]]:
        frame_equals_composed(par, oracle, T, params, planes_scene, sprite, pos, f"lights on planes {pos}")
    # axis-parallel to whole pixel columns (x = 240; z = 0), and in the start bin of a covered pixel (on the pixel)
    gb = graybox(par)
    on_pixel = covered_pixel_light(params, oracle, gb, sprite, T.make_light(480, 160, 80))
    for pos in [[(240, 160, 0), ordinary, (100, 0, 120)], [ordinary, on_pixel, (240, 160, 0), (100, 0, 120)]]:
        frame_equals_composed(par, oracle, T, params, gb, sprite, pos, f"axis-parallel {pos}")
    # far outside the volume in each direction (out-of-range and aliased flat bin indices)
    aabbs, _ = par.scene_synthetic(300, 480, 320, 320, 4)
    for pos in [[(-300, 500, -200), ordinary, (900, -400, 700), (240, 160, 5000)], [(0, 0, 0), (240, 160, 5000), ordinary]]:
        frame_equals_composed(par, oracle, T, params, aabbs, sprite, pos, f"far lights {pos}")
    # the light's bin x equal to the grid width (the reference's default light), and the 481-wide view of that test
    assert light_bin(params, (480, 160, 80))[0] == params.grid_dims()[0]
    frame_equals_composed(par, oracle, T, params, gb, sprite, [(480, 160, 80), ordinary, (480, 20, 300)], "light bin x == gx")
    params = T.default_params(481, 321, 321)
    aabbs, _ = par.scene_synthetic(200, 481, 321, 321, 3)
    frame_equals_composed(par, oracle, T, params, aabbs, sprite, [(481, 160, 80), ordinary], "481 wide, light x 481")


SWEEP_SEED, SWEEP_CASES = 20261016, 64


def sweep_cases(par, T):
    """The cases of the sweep, in the manner of test_gpu_more.test_random_sweep (the same ranges for view, bin size,
    primitives, clumping and extents), with 1..8 lights anywhere from -100 to size + 100 per axis; in every third
    case two lights coincide."""
    rng = np.random.default_rng(SWEEP_SEED)
    for case in range(SWEEP_CASES):
        b = int(rng.choice([8, 16, 20, 24, 32, 40, 40, 40, 48, 64]))
        w = int(rng.integers(5, 90)) * 8 if case % 3 else int(rng.integers(40, 700))
        h = int(rng.integers(40, 500))
        l = int(rng.integers(40, 500))
        n = int(rng.integers(1, 400))
        params = T.default_params(w, h, l, b)
        aabbs, _ = par.scene_synthetic(n, w, h, l, int(rng.integers(1, 1 << 30)))
        if case % 4 == 1:
            aabbs["px"] = (aabbs["px"] % max(2 * b, 40)).astype(aabbs["px"].dtype)
            aabbs["pz"] = (aabbs["pz"] % max(3 * b, 60)).astype(aabbs["pz"].dtype)
        if case % 6 == 3:
            aabbs["ex"] = rng.integers(0, 21, n).astype(aabbs["ex"].dtype)
            aabbs["ey"] = rng.integers(0, 21, n).astype(aabbs["ey"].dtype)
            aabbs["ez"] = (rng.integers(0, 21, n) % (41 - aabbs["ey"])).astype(aabbs["ez"].dtype)
        n_lights = int(rng.integers(1, 9))
        pos = [(int(rng.integers(-100, w + 101)), int(rng.integers(-100, h + 101)), int(rng.integers(-100, l + 101)))
               for _ in range(n_lights)]
        if case % 3 == 2 and n_lights >= 2:
            pos[int(rng.integers(1, n_lights))] = pos[0]
        r0 = int(rng.integers(0, h - 1))
        r1 = int(rng.integers(r0 + 1, h + 1))
        yield case, params, aabbs, pos, (r0, r1)


def lit_bits_seen(exp, set_bits, clear_bits):
    """Which bits of the expected lit plane are set, and which are clear, somewhere among the covered pixels."""
    lit = exp["lit"][exp["palidx"] != 0xFF]
    if len(lit):
        set_bits |= int(np.bitwise_or.reduce(lit))
        clear_bits |= int(np.bitwise_or.reduce(~lit)) & 0xFF
    return set_bits, clear_bits


def test_random_sweep_with_several_lights(par, oracle, sprite, T):
    refused, coincident, counts = [], 0, set()
    set_bits = clear_bits = 0
    for case, params, aabbs, pos, (r0, r1) in sweep_cases(par, T):
        w = params.width
        tag = f"case {case}: {w}x{params.height}x{params.length} bin {params.bin_size}, {len(aabbs)} primitives, lights {pos}"
        lights = lights_of(T, pos)
        exp, per_light = expected(params, oracle, aabbs, sprite, lights, tag=tag)
        # bits at and above the light count stay clear, so only this case's own lights count as "clear somewhere"
        s, c = lit_bits_seen(exp, 0, 0)
        set_bits |= s
        clear_bits |= c & ((1 << len(pos)) - 1)
        counts.add(len(pos))
        coincident += len(set(pos)) < len(pos)
        try:
            r = par.Renderer(params)
        except par.ParError as e:
            refused.append((tag, str(e)))
            continue
        with r:
            r.set_sprites(sprite)
            r.set_entities(aabbs)
            r.set_lights(lights)  # (one light: the production one-light path, no hook)
            assert_planes_equal(r.render(ALL), exp, ALL, tag + " (all planes)")
            part = r.render(ALL, rows=(r0, r1))
            assert_planes_equal(part, rows_of(exp, ALL, w, r0, r1), ALL, tag + f" rows {r0}..{r1}")
            r.stats()
    assert not refused, f"par_create refused {len(refused)} cases: {refused[:3]}"
    assert counts == set(range(1, 9)) and coincident >= SWEEP_CASES // 6
    assert set_bits == 0xFF and clear_bits == 0xFF, (
        f"every light index must be lit and shadowed somewhere in the sweep: set {set_bits:#x}, clear {clear_bits:#x}")


# ---- 4. the graph form on the same edges -------------------------------------------------------------------------

def graph_replays_equal_composed(par, oracle, sprite, T, params, aabbs, pos_a, pos_b, tag, rows=None, flags=0, planes=ALL,
                                 direct_first=False):
    """Capture with the lights pos_a, replay twice (both grid sets' graphs), stage pos_b (another count, other
    positions), replay again: every replay against the composed oracle."""
    import torch
    w, h = params.width, params.height
    r0, r1 = rows or (0, h)
    stream = torch.cuda.Stream()
    out = Planes(params, planes, rows)
    la, lb = lights_of(T, pos_a), lights_of(T, pos_b)
    exp_a, _ = expected(params, oracle, aabbs, sprite, la, tag=tag)
    exp_b, _ = expected(params, oracle, aabbs, sprite, lb, tag=tag)
    with par.Renderer(params) as r:
        r.set_sprites(sprite)
        r.set_entities(aabbs)
        r.set_lights(la)
        if direct_first:  # without a lit plane, a graph of every-ray-traced frames needs the scratch plane of one
            got = r.render(planes, rows=rows, flags=flags)
            assert_planes_equal(got, rows_of(exp_a, planes, w, r0, r1), planes, f"{tag}, direct")
        r.graph_capture_lights(out.ptrs, rows=rows, flags=flags, stream=stream.cuda_stream)
        for k in range(2):
            got = replay(r, out, stream, T)
            assert_planes_equal(got, rows_of(exp_a, planes, w, r0, r1), planes, f"{tag}, {len(pos_a)} lights, replay {k}")
        r.graph_stage(lights=lb)
        for k in range(2):
            got = replay(r, out, stream, T)
            assert_planes_equal(got, rows_of(exp_b, planes, w, r0, r1), planes, f"{tag}, {len(pos_b)} lights staged, "
                                                                               f"replay {k}")
        r.stats()  # raises on PAR_ERR_DEVICE


def test_graph_on_the_walk_area_scene(par, oracle, sprite, T):
    params, aabbs = walk_area_scene(T)
    moved = [(x + 15, y - 10, z + 25) for x, y, z in WALK_AREA_LIGHTS[4:] + WALK_AREA_LIGHTS[:1]]
    for pos in (WALK_AREA_LIGHTS, moved):
        lights = lights_of(T, pos)
        exp, _ = expected(params, oracle, aabbs, sprite, lights, tag="walk area graph")
        found = walk_area_columns(Columns(params, oracle, aabbs, exp), pos)
        assert found, f"walk area graph, lights {pos}: no column of {WALK_AREA_COLUMNS} exhausts the walk area"
    graph_replays_equal_composed(par, oracle, sprite, T, params, aabbs, WALK_AREA_LIGHTS, moved, "walk area graph")


def test_graph_on_the_mixed_stage_scene(par, oracle, sprite, T):
    params, aabbs = mixed_stage_scene(T)
    a, b = MIXED_STAGE_LIGHTS[:3], [(5, 110, 110), (475, 118, 102)] + MIXED_STAGE_LIGHTS[2:8]
    for pos in (a, b):
        exp, _ = expected(params, oracle, aabbs, sprite, lights_of(T, pos), tag="mixed stage graph")
        assert mixed_stage_places(Columns(params, oracle, aabbs, exp), pos), f"mixed stage graph, lights {pos}"
    graph_replays_equal_composed(par, oracle, sprite, T, params, aabbs, a, b, "mixed stage graph")


@pytest.mark.parametrize("planes", [ALL, ("fb", "brightness")])
def test_graph_of_a_row_block_with_every_ray_traced(par, oracle, sprite, T, planes):
    params, aabbs, pos = host_path_scene(par, oracle, sprite, T, "graybox", 3)
    _, _, pos8 = host_path_scene(par, oracle, sprite, T, "graybox", 8)
    graph_replays_equal_composed(par, oracle, sprite, T, params, aabbs, pos, pos8, f"row block graph {planes}",
                                 rows=(37, 251), flags=par.RENDER_TRACE_BACKGROUND, planes=planes,
                                 direct_first="lit" not in planes)
