"""GPU tests at the size limits: grids 1024 bins wide, tall or deep and coordinates at the ends of int16 on every render
path (part A), and the post calls beyond one launch, beyond 4 GiB and at 1024 x 1024 tiles (part B). Everything is
compared byte for byte: frames with the oracle (tests/limits.py: its row-block form where a whole view is too large) or with
test_gpu_lights.compose over the oracle's per-light planes, post calls with their numpy models.

tests/test_limits_cpu.py holds, without a GPU, that the scenes reach what they are named for: covered pixels, lit and
shadowed, in bin column, bin row and z bin 1023 (or the last of the axis), boxes whose sums leave int16 on screen, a wrapped
slot counter, a column with more pairs than the host's bookkeeping takes for sure to fit a record, and none of the culled
boxes anywhere.

overflow_columns: a wrapped counter leaves a bin at most 7 records, so a column of gz z bins holds at most 7 * gz of them,
and a column record takes 64 (and 32 occupied bins): only the int16 deep view (gz = 1024) can have a column that really
overflows its record, and there the stacked column has a box in each of 40 z bins and overflow_columns > 0 is asserted. On
the other five views (gz <= 8) no scene can make it positive; there it is asserted to be 0, and every column goes through
the overflow kernel under set_test_hooks(force_generic=True).

Lights at the ends of int16 are tens of thousands of probes from every pixel, and the oracle traces the background's rays
too: frames under such lights are composed from the lit planes of the covered pixels alone (limits.shadow_rays, held to
par_oracle_shade on the CPU) and compared on every plane but `lit`; the `lit` plane, with every background ray, is compared
on the one-light frames, whose light lies inside the view.

As measured with libraries built for the purpose (none committed), of these 38 tests: with render_item's decode of
par_item.where masked with 0x1FF, 9 fail (the one-light, render_device and relit frames of the views wide and tall, int16
wide and int16 tall); with the output row offset of present_kernel and upscale_kernel cut to 32 bits, 4 (present and the
three scalers of test_output_rows_beyond_4_gib); with first_tile_row taken as 0 in upscale_kernel, 2 (both of
test_upscale_takes_two_launches). tests/test_gpu_parity.py, test_gpu_present.py and test_gpu_upscale.py pass with all
three."""
import numpy as np
import pytest

import finish as F
import limits as LM
import outline as O
import plane_tiles as PT
import present as P
import sequences as SQ
import test_gpu_finish as FINT
import test_gpu_plane_tiles as PTT
import test_gpu_quantize as TQ
import test_gpu_upscale as UPT
import upscale as U
from test_gpu_lights_graph import Planes, replay
from test_gpu_parity import ALL, assert_planes_equal

pytestmark = pytest.mark.gpu

FAST = ("fb", "palidx", "brightness", "gbuf")  # without a lit plane the background's shadow rays are skipped
LIT = ("fb", "brightness", "lit")
VIEWS = list(LM.VIEWS)


def scene_renderer(par, view):
    params, aabbs, sprites, ids, _ = LM.scene(view)
    r = par.Renderer(params)
    r.set_sprites(sprites)
    r.set_entities(aabbs, ids)
    r.set_light(LM.lights_array([LM.default_light(view)]))
    return r


def one_light(view):
    """{rows: the oracle's planes} of a view under its default light."""
    return LM.lit_frame(view, LM.default_light(view))


def columns_in(view, rows):
    """Occupied screen columns of the bin rows a block touches, from the oracle's hash (sequences.grid_sizes)."""
    params = LM.params_of(view)
    per_row = SQ.grid_sizes(params, LM.grid(view))[0]
    return int(per_row[rows[0] // params.bin_size:(rows[1] - 1) // params.bin_size + 1].sum())


# ---- A1. one-light frames on the default path and with every column through the overflow kernel ----------------------

@pytest.mark.parametrize("view", VIEWS)
def test_one_light_frames(par, T, view):
    params, aabbs, _, _, info = LM.scene(view)
    exp = one_light(view)
    blocks = LM.blocks_of(view)
    W, H = params.width, params.height
    with scene_renderer(par, view) as r:
        for hook in (False, True):
            r.set_test_hooks(force_generic=hook)
            for rows in blocks + (blocks[:1] if len(blocks) > 1 else ()):  # (the first block again after the last)
                tag = f"{view} rows {rows}" + (", every column through the overflow kernel" if hook else "")
                assert_planes_equal(r.render(ALL, rows=rows), exp[rows], ALL, tag)
                st = r.stats()  # raises on PAR_ERR_DEVICE
                assert st.bin_insertions == SQ.bounds(params, aabbs)[0], tag
                assert st.occupied_columns == columns_in(view, rows), tag
                if info["deep_stack"]:  # (elsewhere no column can: test_limits_cpu.py)
                    assert st.overflow_columns > 0, f"{tag}: the stacked column should overflow its record"
                else:
                    assert st.overflow_columns == 0, f"{tag}: overflow_columns {st.overflow_columns}"
                assert SQ.grids_equal(r.read_grid(), LM.grid(view)), f"{tag}: read_grid() against oracle.bin"
                assert_planes_equal(r.render(FAST, rows=rows), exp[rows], FAST, f"{tag}, fast planes")
            last = exp[blocks[-1]]["gbuf"][-1:]
            assert r.pick(W - 1, H - 1).tobytes() == last.tobytes(), f"{view}: pick at the last pixel"
            assert r.pick(W - 1, 0).tobytes() == exp[blocks[0]]["gbuf"][W - 1:W].tobytes(), f"{view}: pick at the last column"
        r.stats()


# ---- A2. several lights through the light kernel, lights at the ends of int16 ----------------------------------------

def light_sets(view):
    """A three-light frame with the ends of the view's limited axes, and all eight: two inside, six ends."""
    ends = LM.end_lights(view)
    axes = LM.VIEWS[view][4]
    inside = LM.inside_lights(view)
    first = LM.default_light(view)
    three = [first] + ([ends["x-"], ends["y+"]] if axes == "xy" else [ends[axes + "-"], ends[axes + "+"]])
    other = next(p for p in inside if p != first)
    return [("three lights", three), ("eight lights", [first, other] + list(ends.values()))]


@pytest.mark.parametrize("view", VIEWS)
def test_several_lights_at_the_ends_of_int16(par, T, view):
    with scene_renderer(par, view) as r:
        for tag, positions in light_sets(view):
            exp, lights = LM.composed(view, positions)
            r.set_lights(lights)
            for rows in LM.blocks_of(view):
                assert_planes_equal(r.render(FAST, rows=rows), exp[rows], FAST, f"{view} rows {rows}, {tag}")
        # one light through the light kernel: every ray, and the lit plane
        r.set_lights(LM.lights_array([LM.default_light(view)]))
        r.set_test_hooks(lights_path=True)
        for rows in LM.blocks_of(view):
            assert_planes_equal(r.render(ALL, rows=rows), one_light(view)[rows], ALL, f"{view} rows {rows}, the light kernel")
        r.stats()


# ---- A3. render_device into poisoned planes with guard rows ----------------------------------------------------------

@pytest.mark.parametrize("view", VIEWS)
def test_render_device_into_guarded_planes(par, T, view):
    params = LM.params_of(view)
    mem = SQ.TorchMem()
    stream = mem.stream()
    with scene_renderer(par, view) as r:
        for rows in LM.blocks_of(view):
            out = SQ.Guarded(mem, params.width, ALL, rows)
            out.poison(stream)
            r.render_device(out.ptrs, rows=rows, stream=stream.handle)
            snap = out.snapshot(stream)
            stream.synchronize()
            tag = f"{view} rows {rows}, render_device"
            assert_planes_equal(out.planes_of(snap, tag), one_light(view)[rows], ALL, tag)
        r.stats()


# ---- A4. relit frames after the light moves to an end of int16 -------------------------------------------------------

@pytest.mark.parametrize("view", VIEWS)
def test_relight_after_a_light_moves_to_an_end_of_int16(par, T, view):
    axes = LM.VIEWS[view][4]
    ends = [LM.end_lights(view)[a + s] for a in axes for s in "-+"]
    with scene_renderer(par, view) as r:
        for rows in LM.blocks_of(view):
            tag = f"{view} rows {rows}"
            assert_planes_equal(r.render(ALL, rows=rows), one_light(view)[rows], ALL, f"{tag}: the retained frame")
            for at in ends:
                exp, lights = LM.composed(view, [at])
                r.set_lights(lights)
                assert exp[rows]["fb"].tobytes() != one_light(view)[rows]["fb"].tobytes(), f"{tag}: the new light should show"
                assert_planes_equal(r.relight(("fb", "brightness"), rows=rows), exp[rows], ("fb", "brightness"),
                                    f"{tag}, relit with the light at {at}")
            r.set_light(LM.lights_array([LM.default_light(view)]))
            assert_planes_equal(r.relight(LIT, rows=rows), one_light(view)[rows], LIT, f"{tag}, relit with the light back")
        r.stats()


# ---- A5. a captured graph with a box staged into bin column 1023 -----------------------------------------------------

def test_graph_replay_with_a_box_moved_into_column_1023(par, T):
    import torch
    view = "widest grid"
    params, aabbs, sprites, ids, info = LM.scene(view)
    W, H, B = params.width, params.height, params.bin_size
    rows = (0, H)
    light = LM.lights_array([LM.default_light(view)])
    # an entity on screen in the middle of the view goes to the front of the last bin column
    seen = np.unique(one_light(view)[rows]["gbuf"]["entity_index"][LM.covered(one_light(view)[rows])])
    i = int(next(e for e in seen if W // 4 < aabbs["px"][e] < 3 * W // 4))
    moved = aabbs.copy()
    moved[i] = T.make_aabbs([LM.box(H, W - 6, -3, -10, (20, 20, 20))])[0]
    exp = LM.oracle().render(params, moved, sprites, light, ids, nthreads=LM.NTHREADS)
    there = (exp["gbuf"]["entity_index"] == i) & (exp["palidx"] != T.PALIDX_BACKGROUND)
    assert there.any() and (np.nonzero(there)[0] % W // B == 1023).all(), "the moved box shows in bin column 1023 alone"
    stream = torch.cuda.Stream()
    out = Planes(params, ALL)
    with scene_renderer(par, view) as r:
        r.graph_capture(out.ptrs, stream=stream.cuda_stream)
        for k in range(2):  # (both grid sets' graphs)
            assert_planes_equal(replay(r, out, stream, T), one_light(view)[rows], ALL, f"replay {k}")
        r.graph_stage(moved[i:i + 1], first=i)
        for k in range(2):
            assert_planes_equal(replay(r, out, stream, T), exp, ALL, f"replay {k} with the box in column 1023")
        r.graph_stage(aabbs[i:i + 1], first=i)
        assert_planes_equal(replay(r, out, stream, T), one_light(view)[rows], ALL, "replay with the box back")
        r.stats()


# ======================================================================================================================
# B. the post calls beyond one launch, beyond 4 GiB, and at 1024 x 1024 tiles
# ======================================================================================================================

MAX_TILE_ROWS = 65535        # tile rows a launch takes (the grid's y extent)
UP_TH, FIN_TH = 4, 16        # source rows of a tile of upscale and of finish
GIB = 1 << 30


# ---- B1. two launches by tile rows -----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (2, 4))
def test_upscale_takes_two_launches(par, T, k):
    """A source three wide with more tile rows than one launch takes: the second launch starts at first_tile_row 65 535,
    and the rows beside the cut see each other."""
    w, h, cut = 3, MAX_TILE_ROWS * UP_TH + UP_TH + 3, MAX_TILE_ROWS * UP_TH
    params = T.default_params(w, h)
    fb, index, palette = UPT.three_valued(T, np.random.default_rng(42), w, h)
    UPT.assert_rules_fire(index, w, h, k, f"{w}x{h} k {k}")
    plane = index.reshape(h, w).astype(np.uint32)
    big = U.scaled_elements(plane, k)
    differs = big != np.repeat(np.repeat(plane, k, axis=0), k, axis=1)
    assert differs[k * (cut - 1):k * cut].any() and differs[k * cut:k * (cut + 1)].any(), "rules fire on both sides of the cut"
    assert differs[k * cut:].mean() >= 0.05, "and in the second launch's rows"
    desc = T.make_upscale_desc(k, 4 * w * k + 4, U.BGRA)
    halves = np.concatenate([U.model(params, desc, (0, cut), (cut - 1, cut), index=index[:cut * w])[1],
                             U.model(params, desc, (cut, h), (cut, cut + 1), index=index[cut * w:])[1]])
    assert (halves != big[k * (cut - 1):k * (cut + 1)]).any(), "the rows beside the cut differ from two independent halves'"
    for kw, want in ((dict(fb=fb), ("out",)), (dict(index=index, palette=palette), ("out", "index"))):
        exp = U.model(params, desc, None, None, guard=UPT.GUARD, **kw)
        got = UPT.run(par, T, params, desc, None, None, want=want, **kw)
        UPT.check_both(got, (exp[0], exp[1] if "index" in want else None), f"{w}x{h} k {k} {sorted(kw)}")


def test_finish_takes_two_launches(par, T):
    """A frame two wide with more tile rows than one launch takes, outlined and quantised: against finish.py's composition
    and against the chain of the three device calls; outlines cross the cut."""
    import torch
    w, h, cut = 2, MAX_TILE_ROWS * FIN_TH + FIN_TH + 3, MAX_TILE_ROWS * FIN_TH
    params, gbuf, fb, palette = F.inputs(T, w, h, seed=8)
    rows = (0, h)
    near = lambda a, b: gbuf[a * w:b * w]  # (the classes of a row need the rows next to it alone)
    edge = O.classes(params, F.STYLE, near(cut - 2, cut + 2), (cut - 2, cut + 2), (cut - 1, cut + 1))
    bare = np.concatenate([O.classes(params, F.STYLE, near(cut - 2, cut), (cut - 2, cut), (cut - 1, cut)),
                           O.classes(params, F.STYLE, near(cut, cut + 2), (cut, cut + 2), (cut, cut + 1))])
    assert (edge != bare).any() and (O.classes(params, F.STYLE, near(cut, h), (cut, h), (cut, h)) != 0).any(), \
        "outlines cross the cut, and the second launch has some"
    stage = F.stages("outline+quantise", F.STYLE, gbuf, rows, palette, F.SPREAD)
    desc = T.make_present_desc(1, 1, 4 * w + 4, P.BGRA)
    got = FINT.both(par, T, params, desc, None, fb, stage, "finish, two launches")
    assert len(np.unique(got[1])) > 8
    d_g = torch.from_numpy(gbuf.view(np.uint8).copy()).cuda()
    d_fb = torch.from_numpy(fb.view(np.uint8).copy()).cuda()  # outlined in place by the chain
    d_pal = torch.from_numpy(palette.view(np.uint8).copy()).cuda()
    d_index = torch.full((w * h,), FINT.GUARD, dtype=torch.uint8, device="cuda")
    d_out = torch.full((h * (4 * w + 4),), FINT.GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    par.outline(params, T.make_outline_style(*F.STYLE), d_g.data_ptr(), rows, d_fb.data_ptr(), rows, fb_out=d_fb.data_ptr())
    par.quantize(params, d_pal.data_ptr(), len(palette), d_fb.data_ptr(), rows, index_out=d_index.data_ptr(), spread=F.SPREAD)
    par.present(params, desc, d_out.data_ptr(), rows, index=d_index.data_ptr(), d_palette=d_pal.data_ptr(),
                n_colors=len(palette))
    torch.cuda.synchronize()
    FINT.check(got, (d_out.cpu().numpy().reshape(h, 4 * w + 4), d_index.cpu().numpy()), "finish against the chain")


# ---- B2. output rows that begin beyond 2^32 bytes --------------------------------------------------------------------

def smallest_pitch(row):
    """The smallest pitch, a multiple of 16, with which output row `row` begins beyond 2^32 bytes."""
    p = ((1 << 32) // row + 16) // 16 * 16
    assert p % 16 == 0 and row * p > 1 << 32 >= row * (p - 16) and p < 1 << 31
    return p


def far_rows_case(call):
    """(width, height, rows, output rows, the last row addressed by a product, bytes of a row's picture, pitch) of a call of
    FAR_CALLS. A kernel forms the offset of the first output row of a source row (for Scale4x: of a row of the Scale2x
    plane) as a product with the pitch, and reaches the output rows after it by adding pitches. So the rows are the fewest
    (a pitch stays below 2^31) and the pitch the smallest with which the last such product lies beyond 2^32, which is
    where a product cut to 32 bits would show; the last output row then begins beyond 2^32 too. The scalers give the
    output rows at a clamped edge the same content, so their rows are a block with its halo."""
    w, h, rows, factor_x, factor_y, step = {"present": (37, 4, (0, 4), 2, 1, 1), "finish": (12, 4, (0, 4), 1, 1, 1),
                                            "upscale 2": (21, 5, (1, 4), 2, 2, 2), "upscale 3": (37, 5, (1, 4), 3, 3, 3),
                                            "upscale 4": (21, 6, (2, 4), 4, 4, 2)}[call]
    n = (rows[1] - rows[0]) * factor_y
    return w, h, rows, n, n - step, 4 * w * factor_x, smallest_pitch(n - step)


FAR_CALLS = ("present", "finish", "upscale 2", "upscale 3", "upscale 4")


@pytest.mark.parametrize("call", FAR_CALLS)
def test_output_rows_beyond_4_gib(par, T, call):
    """The surface is a few rows, a pitch of 0.7 to 1.4 GB apart. It is filled with the guard byte, the call runs, and the
    check stays on the device: every row's picture equals the model's row, every other byte is still the guard. A row
    offset cut to 32 bits lands in an earlier row's picture, and every row's content differs from every other's."""
    import torch
    w, h, rows, n, last_product, row_bytes, pitch = far_rows_case(call)
    begins = [r * pitch for r in range(n)]
    assert begins[-1] >= begins[last_product] > 1 << 32 and any(1 << 31 <= b < 1 << 32 for b in begins[:-1])
    assert 8 <= w <= 37 and (begins[last_product] & 0xFFFFFFFF) < row_bytes  # cut to 32 bits it lands in row 0's picture
    total = begins[-1] + row_bytes
    assert total <= 6 * GIB
    if torch.cuda.mem_get_info()[0] < 16 * GIB:
        pytest.skip("less than 16 GiB of device memory free")
    rng = np.random.default_rng(len(call) + n)
    params = T.default_params(w, h)
    d_src = {}

    def up(name, a):
        d_src[name] = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
        return d_src[name].data_ptr()

    if call == "present":
        fb = P.random_colors(T, rng, w * h)
        tight, desc = (T.make_present_desc(2, 1, p, P.BGRA) for p in (row_bytes, pitch))
        exp = P.model(params, tight, rows, fb=fb)
        run = lambda out: par.present(params, desc, out, rows, fb=up("fb", fb))
    elif call == "finish":
        _, gbuf, fb, palette = F.inputs(T, w, h, seed=5)
        tight, desc = (T.make_present_desc(1, 1, p, P.RGBA) for p in (row_bytes, pitch))
        stage = F.stages("outline+quantise", F.STYLE, gbuf, rows, palette, F.SPREAD)
        exp = F.model(params, *stage, tight, fb, rows)[0]
        run = lambda out: par.finish(params, desc, out, rows, up("fb", fb), style=T.make_outline_style(*F.STYLE),
                                     gbuf=up("gbuf", gbuf), d_palette=up("palette", palette), n_colors=len(palette),
                                     spread=F.SPREAD)
    else:
        k = int(call[-1])
        fb, index, palette = UPT.three_valued(T, rng, w, h)
        tight, desc = (T.make_upscale_desc(k, p, U.RGBA) for p in (row_bytes, pitch))
        if k == 3:
            exp = U.model(params, tight, (0, h), rows, fb=fb)[0]
            run = lambda out: par.upscale(params, desc, out, rows, fb=up("fb", fb), src_rows=(0, h))
        else:
            exp = U.model(params, tight, (0, h), rows, index=index, palette=palette)[0]
            run = lambda out: par.upscale(params, desc, out, rows, index=up("index", index), d_palette=up("palette", palette),
                                          n_colors=len(palette), src_rows=(0, h))
    assert exp.shape == (n, row_bytes) and len({r.tobytes() for r in exp}) == n, "every row differs from every other"
    surface = torch.full((total,), UPT.GUARD, dtype=torch.uint8, device="cuda")
    try:
        torch.cuda.synchronize()
        run(surface.data_ptr())
        torch.cuda.synchronize()
        d_exp = torch.from_numpy(exp.copy()).cuda()
        for r, b in enumerate(begins):
            got = surface[b:b + row_bytes]
            if not torch.equal(got, d_exp[r]):
                host = got.cpu().numpy()
                like = [q for q in range(n) if host.tobytes() == exp[q].tobytes()]
                raise AssertionError(f"{call}: output row {r} (at byte {b}) differs from the model's in "
                                     f"{int((host != exp[r]).sum())} bytes; it equals the model's rows {like}")
            gap = surface[b + row_bytes:begins[r + 1]] if r + 1 < n else surface[:0]
            written = int(torch.count_nonzero(gap != UPT.GUARD))
            assert written == 0, f"{call}: {written} bytes between output rows {r} and {r + 1} were written"
    finally:
        del surface
        torch.cuda.empty_cache()


# ---- B3. the tile calls at gx = gy = 1024 ----------------------------------------------------------------------------

TILE_VIEW = (8192, 8192, 8)  # width, height, bin size


def tile_flips(rng, rows, corners):
    """(x, y) of one element in each of the tiles `corners` and of three hundred seeded tiles of the block `rows`."""
    W, H, B = TILE_VIEW
    by = rng.integers(rows[0] // B, (rows[1] + B - 1) // B, 300)
    tiles = list(corners) + list(zip(rng.integers(0, W // B, 300).tolist(), by.tolist()))
    return [(bx * B + int(rng.integers(0, B)), t * B + int(rng.integers(0, B))) for bx, t in tiles]


@pytest.mark.parametrize("e,rows", [(1, (0, 8192)), (4, (0, 24)), (4, (8168, 8192)), (28, (0, 24)), (28, (8168, 8192))])
def test_tile_calls_at_1024_by_1024_tiles(par, T, e, rows):
    import torch
    W, H, B = TILE_VIEW
    params = T.default_params(W, H, B, B)
    gx, gy = PT.grid(params)
    assert (gx, gy) == (1024, 1024)
    r0, r1 = rows
    rng = np.random.default_rng(e + r0)
    corners = [(1023, 1023), (1023, 0), (0, 1023), (512, 512)]
    corners = [(bx, by) for bx, by in corners if r0 <= by * B < r1] + [(1023, r0 // B), (1023, (r1 - 1) // B), (0, (r1 - 1) // B), (512, r0 // B + 1)]
    a = PT.random_plane(rng, (r1 - r0) * W * e)  # the block alone
    cur = a.copy()
    for x, y in tile_flips(rng, rows, corners):
        cur[((y - r0) * W + x) * e + int(rng.integers(0, e))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    exp = PT.changed(params, e, a, cur, rows)
    count = exp[2]
    listed = {(int(t) & 0xFFFF, int(t) >> 16) for t in exp[1]}
    assert set(corners) <= listed and 250 < count <= 308
    if rows == (0, H):
        assert {(1023, 1023), (1023, 0), (0, 1023), (512, 512)} <= listed
    capacity = 512
    d_a, d_b = (torch.from_numpy(p).cuda() for p in (a, cur))
    d_map, d_tiles, d_count = TQ.Carved(4 * gx * gy, 0), TQ.Carved(4 * capacity, 0), TQ.Carved(4, 0)
    d_packed = TQ.Carved(B * B * e * capacity, 0)
    torch.cuda.synchronize()
    par.plane_tiles_changed(params, e, d_a.data_ptr(), d_b.data_ptr(), rows, d_map.ptr, d_tiles.ptr, capacity, d_count.ptr)
    torch.cuda.synchronize()
    assert d_map.guards_intact() and d_tiles.guards_intact() and d_count.guards_intact()
    got = (d_map.host(np.int32), d_tiles.host(np.int32), int(d_count.host(np.int32)[0]))
    PTT.check_changed(got, exp, capacity, f"E {e} rows {rows}")  # the map with its ranks, the list and the count
    # the round trip over that list: the counted pack, the fetch, the host's copy brought up to date
    par.plane_tiles_pack_counted(params, e, d_tiles.ptr, d_count.ptr, capacity, d_b.data_ptr(), rows, d_packed.ptr)
    tiles = np.full(capacity, PTT.GUARD_WORD, dtype=np.uint32).view(np.int32)
    packed = np.full(capacity * B * B * e, TQ.GUARD, dtype=np.uint8)
    n, got_count = par.plane_tiles_fetch(params, e, d_count.ptr, d_tiles.ptr, d_packed.ptr, capacity, tiles, packed)
    assert n == got_count == count and d_packed.guards_intact()
    assert tiles[:n].tobytes() == exp[1].tobytes() and (tiles[n:].view(np.uint32) == PTT.GUARD_WORD).all()
    assert packed.tobytes() == np.concatenate([PT.pack(params, e, exp[1], cur, rows, TQ.GUARD),
                                               np.full((capacity - n) * B * B * e, TQ.GUARD, dtype=np.uint8)]).tobytes()
    frame = a.copy()  # (the whole plane's address, were it there: the call writes the rows `rows` alone)
    par.plane_tiles_apply_host(params, e, tiles, n, packed, rows, frame.ctypes.data - r0 * W * e)
    assert frame.tobytes() == cur.tobytes(), f"E {e} rows {rows}: the host's copy is not the current plane"
    # assemble: the fill where no tile changed, the tiles' contents elsewhere
    fill = bytes(range(7, 7 + e))
    d_frame = TQ.Carved((r1 - r0) * W * e, 0)
    torch.cuda.synchronize()
    par.plane_tiles_assemble(params, e, d_map.ptr, d_packed.ptr, fill, d_frame.ptr - r0 * W * e, rows)
    torch.cuda.synchronize()
    assert d_frame.guards_intact()
    want = np.tile(np.frombuffer(fill, dtype=np.uint8), (r1 - r0) * W).reshape(r1 - r0, W, e)
    src = cur.reshape(r1 - r0, W, e)
    for bx, by in listed:
        lo, hi = max(by * B, r0) - r0, min((by + 1) * B, r1) - r0
        want[lo:hi, bx * B:(bx + 1) * B] = src[lo:hi, bx * B:(bx + 1) * B]
    assert d_frame.host(np.uint8).tobytes() == want.tobytes(), f"E {e} rows {rows}: the assembled block"
    assert d_a.cpu().numpy().tobytes() == a.tobytes() and d_b.cpu().numpy().tobytes() == cur.tobytes(), "an input was written"
