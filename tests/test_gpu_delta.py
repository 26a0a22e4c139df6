"""GPU tests of the changed-tiles calls (par_tiles_changed_device, par_tiles_pack_counted, par_tiles_fetch,
par_tiles_apply_host) and of FrameDelta: maps, lists, counts and slots byte for byte against the contract restated in
numpy (tests/delta.py; tests/test_delta_cpu.py holds it to per-pixel loops without a GPU). Every plane the calls write
lies in a guard-filled tensor whose guard bytes are checked after the call; the inputs are checked unchanged. The frames
(delta.FRAMES) are the smallest at which each mechanism of the kernels can go wrong, each run whole and as a row block;
the planes of a block are rows [r0, r1) of the whole frames, so the rows just outside the block lie right beside the
memory a call may read."""
import importlib

import numpy as np
import pytest

import delta as D
from test_gpu_quantize import GUARD, Carved

pytestmark = pytest.mark.gpu

GUARD_WORD = GUARD * 0x01010101


def params_of(T, w, h, b):
    return T.default_params(w, h, h, b)


class Planes:
    """Two whole frames on the device, each at its own 16-byte phase; `a` and `b` address the block's first row."""

    def __init__(self, params, a_full, b_full, rows, shifts=(0, 0)):
        self.host = (np.asarray(a_full, dtype=np.uint32), np.asarray(b_full, dtype=np.uint32))
        self.dev = [Carved(4 * len(f), s, f) for f, s in zip(self.host, shifts)]
        off = 4 * rows[0] * params.width
        self.a, self.b = self.dev[0].ptr + off, self.dev[1].ptr + off

    def unchanged(self):
        return all(d.host(np.uint32).tobytes() == f.tobytes() and d.guards_intact() for d, f in zip(self.dev, self.host))


def run_changed(par, params, planes, rows, capacity, null_tiles=False, same=False):
    """One par_tiles_changed_device call: (map, the list plane of `capacity` words, count, the device planes)."""
    import torch
    gx, gy = D.grid(params)
    d_map, d_count = Carved(4 * gx * gy, 0), Carved(4, 0)
    d_tiles = None if null_tiles else Carved(4 * capacity, 0)
    torch.cuda.synchronize()
    par.tiles_changed(params, planes.a, planes.a if same else planes.b, rows, d_map.ptr,
                      None if d_tiles is None else d_tiles.ptr, capacity, d_count.ptr)
    torch.cuda.synchronize()
    assert d_map.guards_intact() and d_count.guards_intact() and (d_tiles is None or d_tiles.guards_intact())
    assert planes.unchanged(), "an input was written"
    tiles = np.zeros(0, dtype=np.int32) if d_tiles is None else d_tiles.host(np.int32)
    return d_map.host(np.int32), tiles, int(d_count.host(np.int32)[0]), (d_map, d_tiles, d_count)


def check_changed(got, exp, capacity, tag):
    map_, tiles, count = got[:3]
    e_map, e_tiles, e_count = exp
    assert count == e_count, f"{tag}: count {count}, expected {e_count}"
    bad = np.nonzero(map_ != e_map)[0]
    assert len(bad) == 0, f"{tag}: the map differs at {len(bad)} tiles, first {bad[:4]}"
    m = min(e_count, capacity)
    assert tiles[:m].tobytes() == e_tiles[:m].tobytes(), f"{tag}: the list differs"
    assert (tiles[m:].view(np.uint32) == GUARD_WORD).all(), f"{tag}: list entries from min(count, capacity) on were written"


def both_blocks(h):
    return ((0, h), D.block_rows(h))


# ---- 1. map, list and count against the model -----------------------------------------------------------------------

@pytest.mark.parametrize("w,h,b", D.FRAMES)
def test_flips_against_the_model(par, T, w, h, b):
    params = params_of(T, w, h, b)
    gx, gy = D.grid(params)
    a = D.random_plane(np.random.default_rng(w + h), w * h)
    for rows in both_blocks(h):
        D.check_flips(params, rows)
        inside, outside = D.flips(params, rows)
        cut = slice(rows[0] * w, rows[1] * w)
        cur = D.flipped(params, a, inside + outside)
        exp = D.changed(params, a[cut], cur[cut], rows)
        assert exp[2] == len({(x // b, y // b) for x, y, _, _ in inside})
        check_changed(run_changed(par, params, Planes(params, a, cur, rows), rows, gx * gy), exp, gx * gy, f"rows {rows}")
        if outside:  # a flip in a row just outside the block, in a tile that is in the block, does not flag it
            cur = D.flipped(params, a, outside)
            got = run_changed(par, params, Planes(params, a, cur, rows), rows, gx * gy)
            assert got[2] == 0 and (got[0] == -1).all() and (got[1].view(np.uint32) == GUARD_WORD).all()


# ---- 2. phases ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,b", [D.FRAMES[0], D.FRAMES[1], D.FRAMES[3]])
def test_phases(par, T, w, h, b):
    """`a` and `b` at bytes 0, 4, 8 and 12 past a 16-byte boundary, independently: the same result on either path."""
    params = params_of(T, w, h, b)
    gx, gy = D.grid(params)
    a = D.random_plane(np.random.default_rng(2 * w + h), w * h)
    for rows in both_blocks(h):
        inside, outside = D.flips(params, rows)
        cut = slice(rows[0] * w, rows[1] * w)
        cur = D.flipped(params, a, inside + outside)
        exp = D.changed(params, a[cut], cur[cut], rows)
        for sa in (0, 4, 8, 12):
            for sb in (0, 4, 8, 12):
                got = run_changed(par, params, Planes(params, a, cur, rows, (sa, sb)), rows, gx * gy)
                check_changed(got, exp, gx * gy, f"rows {rows} phases {sa}, {sb}")


# ---- 3. capacity -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,b", [D.FRAMES[3], D.FRAMES[5]])
def test_capacity(par, T, w, h, b):
    params = params_of(T, w, h, b)
    gx, gy = D.grid(params)
    rng = np.random.default_rng(3 * w + h)
    a = D.random_plane(rng, w * h)
    cur = a.copy()
    cur[rng.random(w * h) < 0.02] ^= np.uint32(0x100)
    for rows in both_blocks(h):
        cut = slice(rows[0] * w, rows[1] * w)
        exp = D.changed(params, a[cut], cur[cut], rows)
        count = exp[2]
        assert 2 < count < gx * gy
        planes = Planes(params, a, cur, rows)
        for capacity in (0, 1, count - 1, count, gx * gy):
            check_changed(run_changed(par, params, planes, rows, capacity), exp, capacity, f"rows {rows} capacity {capacity}")
        got = run_changed(par, params, planes, rows, 0, null_tiles=True)
        check_changed(got, exp, 0, f"rows {rows} null list")


# ---- 4. extremes -------------------------------------------------------------------------------------------------------

def test_extremes(par, T):
    w, h, b = D.FRAMES[5]
    params = params_of(T, w, h, b)
    gx, gy = D.grid(params)
    assert gx * gy == 1200
    rng = np.random.default_rng(4)
    a = D.random_plane(rng, w * h)
    everything = a ^ np.uint32(1 << 24)
    flags = rng.random(gx * gy) < 0.5
    half = a.copy().reshape(h, w)
    for i in np.nonzero(flags)[0]:
        bx, by = i % gx, i // gx
        half[by * b + int(rng.integers(0, b)), bx * b + int(rng.integers(0, b))] ^= np.uint32(0x8000)
    half = half.reshape(-1)
    for rows in both_blocks(h):
        cut = slice(rows[0] * w, rows[1] * w)
        in_block = sum(1 for by in range(gy) if D.tile_rows(params, by, rows)[0] < D.tile_rows(params, by, rows)[1]) * gx
        for tag, cur in (("none", a.copy()), ("all", everything), ("half", half)):
            exp = D.changed(params, a[cut], cur[cut], rows)
            if tag == "none":
                assert exp[2] == 0 and (exp[0] == -1).all()
            if tag == "all":
                assert exp[2] == in_block
            if tag == "half":
                assert 0 < exp[2] < in_block and (rows != (0, h) or exp[2] == flags.sum())
            planes = Planes(params, a, cur, rows)
            first = run_changed(par, params, planes, rows, gx * gy)
            check_changed(first, exp, gx * gy, f"rows {rows} {tag}")
            again = run_changed(par, params, planes, rows, gx * gy)
            assert all(first[k].tobytes() == again[k].tobytes() for k in (0, 1)) and first[2] == again[2], \
                f"rows {rows} {tag}: the same call twice differs"
        same = run_changed(par, params, Planes(params, a, everything, rows), rows, gx * gy, same=True)
        assert same[2] == 0 and (same[0] == -1).all() and (same[1].view(np.uint32) == GUARD_WORD).all()


# ---- 5. the counted pack ---------------------------------------------------------------------------------------------

def run_packs(par, params, block_ptr, rows, d_tiles_ptr, d_count_ptr, capacity, m, shift=0):
    """par_tiles_pack_counted and par_tiles_pack with n = m, each into a guard-filled buffer of `capacity` slots."""
    import torch
    slot = 4 * params.bin_size * params.bin_size
    counted, plain = Carved(capacity * slot, shift), Carved(capacity * slot, shift)
    torch.cuda.synchronize()
    par.tiles_pack_counted(params, d_tiles_ptr, d_count_ptr, capacity, block_ptr, rows, counted.ptr)
    par.tiles_pack(params, d_tiles_ptr, m, block_ptr, rows, plain.ptr)
    torch.cuda.synchronize()
    assert counted.guards_intact() and plain.guards_intact()
    return counted.host(np.uint8), plain.host(np.uint8)


@pytest.mark.parametrize("w,h,b", D.FRAMES)
def test_counted_pack(par, T, w, h, b):
    import torch
    params = params_of(T, w, h, b)
    gx, gy = D.grid(params)
    rng = np.random.default_rng(5 * w + h)
    a = D.random_plane(rng, w * h)
    cur = D.random_plane(rng, w * h) if gx * gy <= 64 else a ^ (rng.random(w * h) < 0.01).astype(np.uint32)
    for rows in both_blocks(h):
        cut = slice(rows[0] * w, rows[1] * w)
        e_map, e_tiles, count = D.changed(params, a[cut], cur[cut], rows)
        assert count >= 1
        planes = Planes(params, a, cur, rows)
        for capacity in sorted({gx * gy, count, max(count - 1, 1)}):
            m = min(count, capacity)
            _, tiles, got_count, (d_map, d_tiles, d_count) = run_changed(par, params, planes, rows, capacity)
            assert got_count == count and tiles[:m].tobytes() == e_tiles[:m].tobytes()
            counted, plain = run_packs(par, params, planes.b, rows, d_tiles.ptr, d_count.ptr, capacity, m)
            exp = np.full(len(counted), GUARD, dtype=np.uint8)
            model = D.pack(params, e_tiles[:m], cur[cut], rows, GUARD)
            exp[:len(model)] = model
            assert counted.tobytes() == plain.tobytes(), f"rows {rows} capacity {capacity}: differs from par_tiles_pack"
            assert counted.tobytes() == exp.tobytes(), f"rows {rows} capacity {capacity}: differs from the model"
            assert planes.unchanged() and d_tiles.guards_intact() and d_count.guards_intact()
        if (w, h, b) not in (D.FRAMES[0], D.FRAMES[1]):
            continue
        # both packs at another phase of the slots (the frame's block starts where rows[0] * w puts it)
        capacity = gx * gy
        _, tiles, _, (d_map, d_tiles, d_count) = run_changed(par, params, planes, rows, capacity)
        for shift in (4, 8):
            counted, plain = run_packs(par, params, planes.b, rows, d_tiles.ptr, d_count.ptr, capacity, count, shift)
            assert counted.tobytes() == plain.tobytes(), f"rows {rows} slots at phase {shift}"
        # a garbage negative count packs nothing
        d_count.t[d_count.at:d_count.at + 4] = torch.from_numpy(np.array([-12345], dtype=np.int32).view(np.uint8)).cuda()
        counted, plain = run_packs(par, params, planes.b, rows, d_tiles.ptr, d_count.ptr, capacity, 0)
        assert (counted == GUARD).all() and (plain == GUARD).all()
        # list entries outside the grid are skipped: their slots stay as they were, the others are packed
        listed = tiles[:count].copy()
        listed[0] = gx | (int(listed[0]) >> 16) << 16
        if count > 2:
            listed[count // 2] = (int(listed[count // 2]) & 0xFFFF) | gy << 16
        listed[count - 1] = -1 if count > 1 else listed[count - 1]
        d_list = Carved(4 * count, 0, listed)
        d_n = Carved(4, 0, np.array([count + 7], dtype=np.int32))  # (a count beyond the capacity is clamped to it)
        counted, plain = run_packs(par, params, planes.b, rows, d_list.ptr, d_n.ptr, count, count)
        assert counted.tobytes() == plain.tobytes()
        assert counted.tobytes() == D.pack(params, listed, cur[cut], rows, GUARD).tobytes()
        slot = 4 * b * b
        assert (counted[:slot] == GUARD).all() and (counted[(count - 1) * slot:] == GUARD).all()
        assert d_list.guards_intact() and d_n.guards_intact() and planes.unchanged()


# ---- 6. round trip -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,b", D.FRAMES)
def test_round_trip(par, T, w, h, b):
    import torch
    params = params_of(T, w, h, b)
    gx, gy = D.grid(params)
    rng = np.random.default_rng(6 * w + h)
    a = D.random_plane(rng, w * h)
    for rows in both_blocks(h):
        cut = slice(rows[0] * w, rows[1] * w)
        inside, outside = D.flips(params, rows)
        cur = D.flipped(params, a, inside + outside)
        cur[cut][rng.random(cut.stop - cut.start) < 0.01] ^= np.uint32(0x00FF0000)
        count = D.changed(params, a[cut], cur[cut], rows)[2]
        assert count >= 1 and (count >= 2 or gx * min(gy, 1 + (rows[1] - 1) // b - rows[0] // b) == 1)
        planes = Planes(params, a, cur, rows)
        for capacity in (gx * gy, count, count - 1):
            _, _, _, (d_map, d_tiles, d_count) = run_changed(par, params, planes, rows, capacity)
            d_packed = Carved(4 * b * b * capacity, 0)
            stream = torch.cuda.Stream()
            par.tiles_pack_counted(params, d_tiles.ptr, d_count.ptr, capacity, planes.b, rows, d_packed.ptr)
            torch.cuda.synchronize()
            # the fetch is what waits: the pack above is enqueued again on a stream of its own and not waited for
            par.tiles_pack_counted(params, d_tiles.ptr, d_count.ptr, capacity, planes.b, rows, d_packed.ptr,
                                   stream=stream.cuda_stream)
            tiles = np.full(capacity, GUARD_WORD, dtype=np.uint32).view(np.int32)
            packed = np.full(capacity * b * b, GUARD_WORD, dtype=np.uint32)
            n, got_count = par.tiles_fetch(params, d_count.ptr, d_tiles.ptr, d_packed.ptr, capacity, tiles,
                                           packed.view(T.COLOR), stream=stream.cuda_stream)
            assert got_count == count
            frame = a.copy()
            if capacity < count:
                assert n == 0, "an incomplete list is not fetched"
                assert (tiles.view(np.uint32) == GUARD_WORD).all() and (packed == GUARD_WORD).all(), "something was copied"
                continue
            assert n == count
            assert (tiles[n:].view(np.uint32) == GUARD_WORD).all() and (packed[n * b * b:] == GUARD_WORD).all()
            par.tiles_apply_host(params, tiles, n, packed.view(T.COLOR), rows, frame.view(T.COLOR))
            assert frame[cut].tobytes() == cur[cut].tobytes(), f"rows {rows} capacity {capacity}: the block is not b"
            rest = np.ones(w * h, dtype=bool)
            rest[cut] = False
            assert frame[rest].tobytes() == a[rest].tobytes(), f"rows {rows}: rows outside the block were written"
            assert planes.unchanged() and d_packed.guards_intact()


# ---- 7. the frame loop -------------------------------------------------------------------------------------------------

def test_frame_loop(par, T):
    """A swap chain of two device frames, the graybox scene at 480 x 320: the entity of aabbs[0] moves for six steps,
    then the light moves. FrameDelta keeps a host frame equal to render()'s fb at every step, with no host wait between
    the render and the fetch; the calls leave the context's statistics and a following relit frame as they are without
    them."""
    import torch
    FD = importlib.import_module("pixel-art-raytracer_amd.delta")
    params = T.default_params()
    w, h = params.width, params.height
    assert (w, h) == (480, 320)
    aabbs = par.scene_graybox(w, h)
    light = T.make_light(480, 160, 80)
    sprite = par.tile_floor()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    fb = [torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda") for _ in range(2)]
    gbuf = [torch.zeros(28 * w * h, dtype=torch.uint8, device="cuda") for _ in range(2)]
    relit = [torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()

    steps = [("entity", 5 * (k + 1)) for k in range(6)] + [("light", 40)]
    gx, gy, _ = params.grid_dims()
    with par.Renderer(params, 0) as with_calls, par.Renderer(params, 0) as without, par.Renderer(params, 0) as ref:
        for r in (with_calls, without, ref):
            r.set_scene(aabbs, sprite, light)
        delta = FD.FrameDelta(params)
        tiny = FD.FrameDelta(params, capacity=1)
        assert delta.capacity == max(1, int(gx * gy * FD.DEFAULT_CAPACITY_SHARE)) and len(delta.frame) == w * h
        with_calls.render_device({"fb": fb[0].data_ptr(), "gbuf": gbuf[0].data_ptr()}, stream=s)
        without.render_device({"fb": fb[0].data_ptr(), "gbuf": gbuf[0].data_ptr()}, stream=s)
        delta.first(fb[0].data_ptr(), s)
        tiny.first(fb[0].data_ptr(), s)
        assert delta.frame.tobytes() == ref.render(("fb",))["fb"].tobytes()
        fallbacks = 0
        moved = aabbs[:1].copy()
        for k, (what, amount) in enumerate(steps):
            prev, cur = fb[k % 2], fb[(k + 1) % 2]
            before = moved.copy()
            if what == "entity":
                moved = aabbs[:1].copy()
                moved["px"] += amount
                for r in (with_calls, without, ref):
                    r.update_aabbs(moved, 0)
            else:
                light = T.make_light(480 - amount, 160, 80 + amount)
                for r in (with_calls, without, ref):
                    r.set_light(light)
            expect = ref.render(("fb",))["fb"]
            outs = {"fb": cur.data_ptr(), "gbuf": gbuf[(k + 1) % 2].data_ptr()}
            without.render_device(outs, stream=s)
            stream.synchronize()
            with_calls.render_device(outs, stream=s)
            count, fell_back = delta.update(prev.data_ptr(), cur.data_ptr(), s)  # no host wait before the fetch
            assert count > 0 and fell_back == (count > delta.capacity), (k, count)
            assert what != "entity" or not fell_back, "one moving entity stays within the default capacity"
            assert delta.frame.tobytes() == expect.tobytes(), f"step {k}: the host frame is not the rendered frame"
            assert cur.cpu().numpy().tobytes() == expect.tobytes()
            if what == "entity":
                # geometry alone moved: the changed tiles lie within what the old and the new scene can reach
                scene_before, scene_after = aabbs.copy(), aabbs.copy()
                scene_before[:1], scene_after[:1] = before, moved
                reach = set(par.scene_tiles(params, scene_before).tolist()) | set(par.scene_tiles(params, scene_after).tolist())
                got = delta._d_tiles.cpu().numpy()[:count]
                assert set(got.tolist()) <= reach, f"step {k}"
                assert count < gx * gy
            count_tiny, fell_back = tiny.update(prev.data_ptr(), cur.data_ptr(), s)
            assert count_tiny == count
            fallbacks += int(fell_back)
            assert fell_back == (count > 1) and tiny.frame.tobytes() == expect.tobytes(), f"step {k}: the fallback's frame"
        assert fallbacks >= 1, "the fallback path was never taken"
        # statistics and a following relit frame are as they are without the calls
        counters = ("entities", "bin_insertions", "shadow_rays", "occupied_columns", "overflow_columns", "render_merged")
        st = [r.stats() for r in (with_calls, without)]
        assert [getattr(st[0], c) for c in counters] == [getattr(st[1], c) for c in counters]
        last = len(steps) % 2
        light = T.make_light(300, 200, 120)
        for r, out in ((with_calls, relit[0]), (without, relit[1])):
            r.set_light(light)
            r.relight_device(gbuf[last].data_ptr(), {"fb": out.data_ptr()}, stream=s)
        stream.synchronize()
        assert relit[0].cpu().numpy().tobytes() == relit[1].cpu().numpy().tobytes()
        assert relit[0].cpu().numpy().tobytes() != fb[last].cpu().numpy().tobytes(), "the relit frame should differ"
