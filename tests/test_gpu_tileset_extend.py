"""GPU tests of shared tile sets (par_tileset_extend_device, par_tileset_extend_host, SharedTileSet): tiles, map, count
and first_new byte for byte against the contract restated in numpy (tileset_extend.model; tests/test_tileset_extend_cpu.py
holds it to a per-cell loop with one dict without a GPU), on buffers carved out of guard-filled tensors (Carved of
test_gpu_quantize.py). After every call the guards round the plane, the work block, the tiles, the map, the count and
first_new are checked, the plane and the stored tiles are unchanged and the storage from min(T_out, capacity) tiles on
still holds its poison. The work block is never prepared: it holds the guard byte.

The sizes, by what they cross in the implementation. The cell-layout kernels are test_gpu_tileset.py's (widths 61, 64,
67; plane and tiles phases 0 to 3 for the word and the byte loads and stores). The stored tiles are inserted by a launch
sized by `capacity` whose workgroups take 16 (8 x 8), 8 or 4 (16 x 16) stored tiles and leave when their first tile is at
or beyond S, a device value: S of 0, 1, one less than, exactly and one more than a workgroup's tiles, and 1023 to 1025,
with S == capacity and S < capacity. The table has P >= 2 (N + capacity) slots, of which the hash launch empties the
first 4 N and the entry launch the rest: a capacity far above N (the stored-count tests) and far below it (the big
planes) cross both. The scan levels, the second launch of a tall plane and the limit are test_gpu_tileset.py's shapes
with a stored set."""
import importlib

import numpy as np
import pytest

import tileset as TS
import tileset_extend as TX
from test_gpu_quantize import GUARD, Carved
from test_gpu_tileset import Call, upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext(par):
    return importlib.import_module("pixel-art-raytracer_amd.tileset_extend")


@pytest.fixture(scope="module")
def tileset(par):
    return importlib.import_module("pixel-art-raytracer_amd.tileset")


class Shared:
    """One kept set on carved device buffers (`capacity` tiles of guard bytes, the count, first_new) and the model's
    copy of it: every extend() is one call on a fresh carved plane, map and work block, checked against the model."""

    def __init__(self, ext, T, tile, capacity, tiles_phase=0, with_map=True, with_first=True, model=TX.model):
        self.ext, self.T, self.tile, self.capacity, self.size = ext, T, tile, capacity, tile[0] * tile[1]
        self.tiles = Carved(capacity * self.size, tiles_phase) if capacity else None
        self.count = Carved(4, 0, np.zeros(1, np.uint32))
        self.first = Carved(4, 0) if with_first else None
        self.with_map, self.model = with_map, model
        self.stored, self.t = TX.no_tiles(tile), 0
        self.work = None

    def seed(self, stored, t_in):
        """A caller-made set: `stored` are the min(t_in, capacity) stored tiles."""
        stored = np.ascontiguousarray(stored, dtype=np.uint8).reshape(-1, self.tile[1], self.tile[0])
        assert len(stored) == min(t_in, self.capacity)
        if len(stored):
            self.tiles.t[self.tiles.at:self.tiles.at + stored.size] = _cuda(stored.reshape(-1))
        upload(self.count, np.array([t_in], np.uint32))
        self.stored, self.t = stored.copy(), t_in

    def launch(self, idx, rows, h, w, work, tile_map, pad, flips, stream=None):
        params = self.T.default_params(w, h)
        self.ext.tileset_extend(params, idx.ptr, rows, self.tile, work.ptr, self.tiles.ptr if self.tiles else None, self.capacity,
                                self.count.ptr, map_out=tile_map.ptr if tile_map else None,
                                first_new_out=self.first.ptr if self.first else None, pad=pad, flips=flips, stream=stream)

    def extend(self, plane, w, h, pad, flips, tag, rows=None, phase=0, keep_work=False, exp=None):
        """One call, checked; returns the model's (tiles after, map, T_out, first_new)."""
        import torch
        rows = rows or (0, h)
        n_rows = rows[1] - rows[0]
        gcx, gcy = TS.grid(w, n_rows, self.tile)
        n = gcx * gcy
        idx = Carved(len(plane), phase, plane)
        if not (keep_work and self.work is not None):
            self.work = Carved(self.ext.tileset_extend_work_bytes(n, self.capacity), 0)
        assert self.work.nbytes <= 4104 + 32 * (n + self.capacity) and self.work.ptr % 8 == 0
        tile_map = Carved(4 * n, 0) if self.with_map else None
        torch.cuda.synchronize()
        self.launch(idx, rows, h, w, self.work, tile_map, pad, flips)
        torch.cuda.synchronize()
        if exp is None:
            exp = self.model(self.stored, self.t, plane, w, n_rows, self.tile, pad, flips, self.capacity)
        self.check(idx, plane, tile_map, exp, tag)
        self.stored, self.t = exp[0], exp[2]
        self.last_map = tile_map
        return exp

    def check(self, idx, plane, tile_map, exp, tag):
        e_tiles, e_map, e_count, e_first = exp
        for name, buf in (("plane", idx), ("work", self.work), ("tiles", self.tiles), ("map", tile_map), ("count", self.count),
                          ("first_new", self.first)):
            assert buf is None or buf.guards_intact(), f"{tag}: {name}: bytes outside the buffer were written"
        assert idx.host(np.uint8).tobytes() == np.asarray(plane, np.uint8).tobytes(), f"{tag}: the plane was written"
        count = int(self.count.host(np.uint32)[0])
        assert count == e_count, f"{tag}: the count is {count}, the model's {e_count}"
        if self.first is not None:
            assert int(self.first.host(np.uint32)[0]) == e_first == self.t, f"{tag}: first_new"
        if tile_map is not None:
            got = tile_map.host(np.uint32)
            bad = np.nonzero(got != e_map)[0]
            assert len(bad) == 0, f"{tag}: the map differs at {len(bad)} cells, first {bad[:4]}: {got[bad[:4]]} for {e_map[bad[:4]]}"
        if self.tiles is not None:
            tiles = self.tiles.host(np.uint8)
            kept = min(e_count, self.capacity)
            assert len(e_tiles) == kept
            s = len(self.stored)
            assert tiles[:s * self.size].tobytes() == self.stored.tobytes(), f"{tag}: a stored tile was written"
            assert tiles[:kept * self.size].tobytes() == e_tiles.tobytes(), f"{tag}: the tiles"
            assert (tiles[kept * self.size:] == GUARD).all(), f"{tag}: storage beyond {kept} tiles was written"


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


# ---- 1. sequences: sizes, phases, flips ----------------------------------------------------------------------------------

@pytest.mark.parametrize("w", [61, 64, 67])
@pytest.mark.parametrize("h", [23, 40])
def test_sequences_of_three_calls(ext, T, w, h):
    reused, added = 0, 0
    for tile in TS.TILES:
        frames = TX.frame_sequence(100 * w + h + tile[0] + 2 * tile[1], 3, w, h, tile, kinds=4, step=3)
        n = TS.grid(w, h, tile)[0] * TS.grid(w, h, tile)[1]
        for flips in range(4):
            for phase in range(4):
                shared = Shared(ext, T, tile, 3 * n, tiles_phase=(phase * 3 + flips) & 3)
                for k, plane in enumerate(frames):
                    exp = shared.extend(plane, w, h, 1 + 6 * (phase & 1), flips, f"{w}x{h} {tile} flips {flips} phase {phase} call {k}",
                                        phase=phase)
                    if k:
                        reused += int(((exp[1] & TS.ID_MASK) < exp[3]).any())
                        added += exp[2] > exp[3]
    assert reused > 100 and added > 60, "later frames should both reuse stored tiles and add new ones"


# ---- 2. count 0 against a build ------------------------------------------------------------------------------------------

def test_from_count_0_it_is_a_build(ext, tileset, T):
    import torch
    rng = np.random.default_rng(21)
    for tile, w, h, flips, pad in (((8, 8), 67, 40, 3, 5), ((16, 16), 61, 23, 1, 0), ((8, 16), 64, 40, 2, 9), ((16, 8), 131, 67, 0, 1)):
        plane = TS.mixed_plane(rng, w, h, tile, 9, colours=3)
        n = TS.grid(w, h, tile)[0] * TS.grid(w, h, tile)[1]
        for capacity in (n, 3):
            call = Call(tileset, T, w, h, None, tile, plane, phase=1, capacity=capacity, tiles_phase=2)
            torch.cuda.synchronize()
            call.build(pad, flips)
            torch.cuda.synchronize()
            shared = Shared(ext, T, tile, capacity, tiles_phase=2)
            exp = shared.extend(plane, w, h, pad, flips, f"count 0, {tile}, capacity {capacity}", phase=1)
            assert exp[3] == 0
            assert torch.equal(shared.tiles.t, call.tiles.t), "tiles, guards included"
            assert torch.equal(shared.last_map.t, call.map.t) and torch.equal(shared.count.t, call.count.t)


# ---- 3. stored counts at the edges of the stored launch ---------------------------------------------------------------------

def set_of(rng, tile, count, colours=3):
    """`count` distinct random tiles (distinct: tile i holds i in its first bytes)."""
    tiles = rng.integers(0, colours, (count, tile[1], tile[0]), dtype=np.uint8)
    tiles[:, 0, 0], tiles[:, 0, 1], tiles[:, 0, 2] = np.arange(count) & 255, (np.arange(count) >> 8) & 255, 7
    return tiles


def plane_of_tiles(tiles, gcx, tile):
    n = len(tiles)
    assert n % gcx == 0
    return np.ascontiguousarray(tiles.reshape(n // gcx, gcx, tile[1], tile[0]).transpose(0, 2, 1, 3)).reshape(-1)


@pytest.mark.parametrize("tile,counts", [((8, 8), (0, 1, 15, 16, 17, 1023, 1024, 1025)), ((16, 16), (0, 1, 3, 4, 5, 1023, 1024, 1025))])
def test_stored_counts_at_the_edges_of_a_workgroup(ext, T, tile, counts):
    """A plane of 8 x 6 cells: each stored count S twice, with S == capacity and with S < capacity; the plane holds the
    last stored tiles (where there are any), the first one, and new ones, so a wrong S shows as a tile not found or as
    poison matched."""
    rng = np.random.default_rng(31)
    pool = set_of(rng, tile, 1025 + 48)
    for s in counts:
        picks = np.concatenate([np.arange(max(0, s - 20), s), np.arange(min(s, 1)), 1025 + np.arange(48)])[:48]
        cells = pool[picks[rng.permutation(48)]]
        plane = plane_of_tiles(cells, 8, tile)
        for capacity in (s, s + 37):
            shared = Shared(ext, T, tile, capacity, tiles_phase=s & 3)
            shared.seed(pool[:s], s)
            exp = shared.extend(plane, 8 * tile[0], 6 * tile[1], 0, 0, f"{tile} S {s} capacity {capacity}")
            assert exp[2] == s + len(np.unique(picks[picks >= s])) and ((exp[1] & TS.ID_MASK) < s).sum() == (picks < s).sum()
            assert (picks < s).sum() == (min(s, 20) + 1 if s else 0)


# ---- 4. extreme planes ---------------------------------------------------------------------------------------------------

def test_one_colour_meets_on_a_slot_a_stored_tile_owns(ext, T):
    tile, w, h = (8, 8), 512, 512
    plane = np.full(w * h, 9, np.uint8)
    stored = set_of(np.random.default_rng(41), tile, 40)
    stored[17] = 9
    stored[29] = 9  # a duplicate: the lower number wins
    shared = Shared(ext, T, tile, 64)
    shared.seed(stored, 40)
    exp = shared.extend(plane, w, h, 0, 3, "one colour, stored")
    assert exp[2] == 40 and (exp[1] == 17).all() and len(exp[1]) == 4096
    shared = Shared(ext, T, tile, 64)
    exp = shared.extend(plane, w, h, 0, 3, "one colour, an empty set")
    assert exp[2] == 1 and not exp[1].any()


def test_all_distinct_and_none_stored_then_all_stored(ext, T):
    tile, w, h = (8, 8), 512, 512
    plane = TS.distinct_plane(w, h, tile)
    stored = set_of(np.random.default_rng(42), tile, 100)  # (byte 2 is 7: no cell of distinct_plane has it)
    shared = Shared(ext, T, tile, 100 + 4096)
    shared.seed(stored, 100)
    exp = shared.extend(plane, w, h, 0, 0, "all distinct, none stored")
    assert exp[2] == 4196 and np.array_equal(exp[1], 100 + np.arange(4096, dtype=np.uint32))
    # every cell equal to a different stored tile, in another order: nothing is new and not a tile byte is written
    cells = TS.cells_of(plane, w, h, tile, 0)
    order = np.random.default_rng(43).permutation(4096)
    shared = Shared(ext, T, tile, 4096, tiles_phase=1)
    shared.seed(cells[order], 4096)
    exp = shared.extend(plane, w, h, 0, 0, "every cell a different stored tile")
    assert exp[2] == 4096 and np.array_equal(exp[1], np.argsort(order).astype(np.uint32))


# ---- 5. capacity ---------------------------------------------------------------------------------------------------------

def test_capacity_crossed_then_exceeded_and_capacity_0(ext, T):
    tile, w, h = (8, 8), 67, 40
    frames = TX.frame_sequence(51, 3, w, h, tile, kinds=6, step=5, colours=3)
    full, _ = TX.sequence_model(frames, w, h, tile, 5, 3, 1000)
    t0, t1 = full[0][2], full[1][2]
    assert t0 + 2 < t1
    shared = Shared(ext, T, tile, t0 + 2, tiles_phase=3)
    shared.extend(frames[0], w, h, 5, 3, "below the capacity")
    exp = shared.extend(frames[1], w, h, 5, 3, "T_in < capacity < T_out")
    assert exp[3] < shared.capacity < exp[2]
    exp = shared.extend(frames[2], w, h, 5, 3, "T_in > capacity")
    assert exp[3] > shared.capacity and exp[2] > exp[3], "tiles that were not stored count again"
    again = shared.extend(frames[2], w, h, 5, 3, "T_in > capacity, the same plane again")
    assert again[2] - again[3] == exp[2] - exp[3]
    none = Shared(ext, T, tile, 0)
    counts = [none.extend(f, w, h, 5, 3, f"capacity 0, call {k}")[2] for k, f in enumerate(frames)]
    assert counts == list(np.cumsum([TS.model(f, w, h, tile, 5, 3)[2] for f in frames]))


# ---- 6. caller-made sets -------------------------------------------------------------------------------------------------

def test_caller_made_sets(ext, T):
    tile = (8, 8)
    t = np.zeros((8, 8), np.uint8)
    t[0, 0], t[0, 1], t[1, 0] = 1, 2, 3  # its canonical form under flips 3 is its xy mirror
    other = np.full((8, 8), 4, np.uint8)
    plane = plane_of_tiles(np.stack([t, other, t[::-1, ::-1], other]), 4, tile)
    shared = Shared(ext, T, tile, 8)
    shared.seed(np.stack([other, t, other, t]), 4)  # duplicates, and t is stored as it is: not canonical under flips 3
    exp = shared.extend(plane, 32, 8, 0, 3, "duplicates and a stored tile that is not canonical")
    assert exp[2] == 5 and list(exp[1]) == [4 | (3 << 30), 0, 4, 0], "t's mirror is a new tile, the lowest duplicate wins"
    shared = Shared(ext, T, tile, 8)
    shared.seed(np.stack([other, t, other, t]), 4)
    exp = shared.extend(plane, 32, 8, 0, 0, "the same set without flips")
    assert exp[2] == 5 and list(exp[1]) == [1, 0, 4, 0]


# ---- 7. row blocks, merge, idempotence -------------------------------------------------------------------------------------

def test_row_blocks_in_order_give_the_frames_build(ext, T):
    tile, w, h = (8, 8), 37, 40
    plane = TS.mixed_plane(np.random.default_rng(61), w, h, tile, 9, colours=2)
    whole = TS.model(plane, w, h, tile, 3, 3)
    shared = Shared(ext, T, tile, 40)
    maps = []
    for r0, r1 in ((0, 16), (16, 32), (32, 40)):
        exp = shared.extend(plane[r0 * w:r1 * w], w, h, 3, 3, f"rows {r0}..{r1}", rows=(r0, r1), phase=r0 & 3)
        maps.append(shared.last_map.host(np.uint32))
    assert np.array_equal(np.concatenate(maps), whole[1]) and exp[2] == whole[2]
    assert shared.tiles.host(np.uint8)[:whole[2] * 64].tobytes() == whole[0].tobytes()


def test_merge_of_two_built_sets_and_the_same_plane_twice(ext, T):
    tile, w, h = (16, 8), 131, 67
    a_plane, b_plane = TX.frame_sequence(62, 2, w, h, tile, kinds=7, step=6)
    a, b = TS.model(a_plane, w, h, tile, 0, 3), TS.model(b_plane, w, h, tile, 0, 3)
    shared = Shared(ext, T, tile, a[2] + b[2], tiles_phase=2)
    shared.seed(a[0], a[2])
    # B as an index plane of width tile_w and T_B * tile_h rows
    exp = shared.extend(b[0].reshape(-1), tile[0], b[2] * tile[1], 0, 3, "merge")
    assert not (exp[1] >> 30).any(), "B is canonical under the same flips"
    direct = TX.model(a[0], a[2], b_plane, w, h, tile, 0, 3, a[2] + b[2])
    assert a[2] < exp[2] < a[2] + b[2] and exp[2] == direct[2] and exp[0].tobytes() == direct[0].tobytes()
    assert np.array_equal(exp[1][b[1] & TS.ID_MASK] & TS.ID_MASK, direct[1] & TS.ID_MASK), "map_out is B's renumbering"
    again = shared.extend(b[0].reshape(-1), tile[0], b[2] * tile[1], 0, 3, "the same plane twice")
    assert again[2] == exp[2] and np.array_equal(again[1], exp[1]) and again[0].tobytes() == exp[0].tobytes()


# ---- 8. scan levels, launch cuts, the limit ----------------------------------------------------------------------------

def test_mixed_with_20000_stored_crosses_every_level_of_the_scan(ext, T):
    tile, w, h = (8, 8), 2048, 1032
    rng = np.random.default_rng(71)
    pool = set_of(rng, tile, 24000, colours=4)
    stored = pool[:20000]
    pick = rng.integers(15000, 24000, 33024)
    pick[rng.integers(0, 33024, 12000)] = 19999  # a background: runs, and many cells on one stored tile's slot
    plane = plane_of_tiles(pool[pick], 256, tile)
    shared = Shared(ext, T, tile, 30000)
    shared.seed(stored, 20000)
    exp = shared.extend(plane, w, h, 0, 0, "33 024 cells, 20 000 stored")
    new = exp[2] - exp[3]
    first = np.nonzero(np.diff(np.maximum.accumulate(exp[1] & TS.ID_MASK)) > 0)[0] + 1
    assert 3000 < new <= 4000 and (first >= 32 * 1024).any(), "new tiles up to the last workgroup of the scan"


def test_a_tall_plane_with_a_stored_set_takes_two_launches(ext, T):
    rows = 8 * 65600
    rng = np.random.default_rng(72)
    plane = TS.mixed_plane(rng, 8, rows, (8, 8), 40, colours=2)
    head = TS.model(plane[:8 * 8 * 30000], 8, 8 * 30000, (8, 8), 0, 3)
    shared = Shared(ext, T, (8, 8), 64)
    shared.seed(head[0][::2], (head[2] + 1) // 2)  # every other tile of the plane's set is stored
    exp = shared.extend(plane, 8, rows, 0, 3, "65 600 cell rows")
    tail = exp[1][65535:]
    assert ((tail & TS.ID_MASK) < exp[3]).any() and ((tail & TS.ID_MASK) >= exp[3]).any() and (tail >> 30).any()


def test_the_limit_of_cells_and_capacity(ext, T):
    """N = 2^20 cells that all differ into a set of capacity 2^20 of which 2^20 - 4096 are stored: the largest virtual
    number and the largest table (2^22 slots). The expectation is in closed form, so EVERYTHING is checked, the whole
    map and every tile byte: without flips stored tile i is cell S - 1 - i, so map[c] = S - 1 - c below S, and the cells
    from S on are new tiles c in their order."""
    import torch
    side, tile = 8192, (8, 8)
    n = s = TS.MAX_CELLS
    s -= 4096
    plane = TS.distinct_plane(side, side, tile)
    cells = TS.cells_of(plane, side, side, tile, 0)
    shared = Shared(ext, T, tile, n)
    shared.seed(cells[:s][::-1], s)
    e_map = np.arange(n, dtype=np.uint32)
    e_map[:s] = s - 1 - e_map[:s]
    after = np.concatenate([shared.stored, cells[s:]])
    exp = shared.extend(plane, side, side, 0, 0, "2^20 cells, capacity 2^20", exp=(after, e_map, n, s))
    assert ext.tileset_extend_work_bytes(n, n) == shared.work.nbytes == 4096 + 16 * n + 4 * (1 << 22) + 8
    assert ext.tileset_extend_work_bytes(n + 1, n) == 0 == ext.tileset_extend_work_bytes(n, n + 1)
    torch.cuda.synchronize()


# ---- 9. repeat calls and nulls -------------------------------------------------------------------------------------------

def test_a_second_call_and_the_same_call_twice_on_one_unprepared_work_block(ext, T):
    tile, w, h = (8, 8), 131, 67
    first, second = TX.frame_sequence(81, 2, w, h, tile, kinds=30, step=25, colours=2)
    shared = Shared(ext, T, tile, 400, tiles_phase=1)
    a = shared.extend(first, w, h, 0, 3, "the first call", phase=1)
    b = shared.extend(first, w, h, 0, 3, "the same call again", phase=1, keep_work=True)
    assert b[2] == a[2] and np.array_equal(a[1], b[1])
    c = shared.extend(second, w, h, 0, 3, "another plane on the same work block", phase=2, keep_work=True)
    assert c[2] > b[2]


@pytest.mark.parametrize("with_map,with_first", [(False, True), (True, False), (False, False)])
def test_null_outputs(ext, T, with_map, with_first):
    tile, w, h = (8, 16), 67, 40
    frames = TX.frame_sequence(82, 2, w, h, tile)
    for capacity in (64, 0):
        shared = Shared(ext, T, tile, capacity, with_map=with_map, with_first=with_first)
        for k, plane in enumerate(frames):
            shared.extend(plane, w, h, 2, 3, f"map {with_map} first_new {with_first} capacity {capacity} call {k}")


# ---- 10. capture ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [(8, 8), (16, 16)])
def test_captured_once_every_replay_extends_the_last_ones_set(ext, T, tile):
    """One extend captured with torch.cuda.graph after one eager run, then replayed on three new planes: each replay finds
    the count and the tiles the replay before left. Against the eager sequence on a second set of buffers, whole tensors
    with their guards; one wait a replay."""
    import torch
    w, h = 131, 67
    frames = TX.frame_sequence(91, 4, w, h, tile, kinds=5, step=6)
    n = TS.grid(w, h, tile)[0] * TS.grid(w, h, tile)[1]
    capacity = 2 * n
    stream = torch.cuda.Stream()

    def buffers():
        shared = Shared(ext, T, tile, capacity, tiles_phase=1)
        return (shared, Carved(w * h, 3, frames[0]), Carved(ext.tileset_extend_work_bytes(n, capacity), 0), Carved(4 * n, 0))

    eager, e_idx, e_work, e_map = buffers()
    shared, idx, work, tile_map = buffers()
    torch.cuda.synchronize()
    shared.launch(idx, (0, h), h, w, work, tile_map, 0, 3, stream=stream.cuda_stream)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        shared.launch(idx, (0, h), h, w, work, tile_map, 0, 3, stream=stream.cuda_stream)
    # the capture ran nothing: the set holds frame 0 once
    exp, _ = TX.sequence_model(frames, w, h, tile, 0, 3, capacity)
    eager.launch(e_idx, (0, h), h, w, e_work, e_map, 0, 3)
    torch.cuda.synchronize()
    counts = []
    for k in (1, 2, 3):
        for buf, mine in ((idx, shared), (e_idx, eager)):
            upload(buf, frames[k])
        for buf in (tile_map, e_map, work, e_work):
            buf.t.fill_(GUARD)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            graph.replay()
        stream.synchronize()
        eager.launch(e_idx, (0, h), h, w, e_work, e_map, 0, 3)
        torch.cuda.synchronize()
        for name, a, b in (("tiles", shared.tiles, eager.tiles), ("map", tile_map, e_map), ("count", shared.count, eager.count),
                           ("first_new", shared.first, eager.first)):
            assert torch.equal(a.t, b.t), f"replay {k}: {name} differs from the eager sequence"
        assert work.guards_intact() and idx.guards_intact()
        tiles, t_map, t_out, t_in = exp[k]
        assert int(shared.count.host(np.uint32)[0]) == t_out and int(shared.first.host(np.uint32)[0]) == t_in
        assert tile_map.host(np.uint32).tobytes() == t_map.tobytes()
        got = shared.tiles.host(np.uint8)
        assert got[:tiles.size].tobytes() == tiles.tobytes() and (got[tiles.size:] == GUARD).all()
        counts.append(t_out)
    assert counts[0] < counts[1] < counts[2]


# ---- 11. the host form and the plumbing ------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [None, (16, 23)])
def test_host_form_equals_the_device_path(ext, T, rows):
    w, h = 37, 23
    r0, r1 = rows or (0, h)
    params = T.default_params(w, h)
    for tile, pad, flips in (((8, 8), 0, 3), ((16, 16), 200, 0), ((8, 16), 1, 2)):
        first, second = TX.frame_sequence(101 + tile[0], 2, w, r1 - r0, tile, kinds=3, step=3)
        n = TS.grid(w, r1 - r0, tile)[0] * TS.grid(w, r1 - r0, tile)[1]
        start = TS.model(first, w, r1 - r0, tile, pad, flips)
        for capacity in (2 * n, start[2] + 1, start[2] - 1, 0):  # stored below the capacity, crossed, a count above it
            stored, t_in = start[0][:capacity], start[2]
            shared = Shared(ext, T, tile, capacity)
            shared.seed(stored, t_in)
            exp = shared.extend(second, w, h, pad, flips, f"device, {tile}, capacity {capacity}", rows=rows)
            keep = second.copy()
            got = ext.tileset_extend_host(params, second, tile, stored, t_in, capacity, rows=rows, pad=pad, flips=flips)
            assert second.tobytes() == keep.tobytes() and sorted(got) == ["count", "first_new", "map", "tiles"]
            assert got["count"] == exp[2] and got["first_new"] == exp[3] == t_in
            assert got["map"].tobytes() == exp[1].tobytes() and got["tiles"].tobytes() == exp[0].tobytes()
            assert got["tiles"].shape == (min(exp[2], capacity), tile[1], tile[0])
    # the raw symbol: the caller's bytes from min(T_out, capacity) tiles on stay
    tile, capacity = (8, 8), start[2] + 40
    room = np.full(capacity * 128, 0x5C, np.uint8)
    import ctypes as C
    count, first_new = C.c_int(0), C.c_int(-1)
    tile, first = (8, 16), TX.frame_sequence(101 + 8, 2, w, r1 - r0, (8, 16), kinds=3, step=3)[0]
    e = TX.model(TX.no_tiles(tile), 0, first, w, r1 - r0, tile, 1, 2, capacity)
    rc = ext.lib().par_tileset_extend_host(C.byref(params), -1, T.ptr(first), r0, r1, 8, 16, 1, 2, T.ptr(room), capacity,
                                           C.byref(count), None, C.byref(first_new))
    assert rc == 0 and count.value == e[2] and first_new.value == 0
    assert room[:e[0].size].tobytes() == e[0].tobytes() and (room[e[0].size:] == 0x5C).all()


def test_shared_tile_set_over_a_short_sequence(ext, T):
    import torch
    tile, w, h = (8, 8), 131, 67
    frames = TX.frame_sequence(111, 3, w, h, tile, kinds=6, step=5)
    n = TS.grid(w, h, tile)[0] * TS.grid(w, h, tile)[1]
    params = T.default_params(w, h)
    exp, _ = TX.sequence_model(frames, w, h, tile, 2, 3, 64)
    kept = ext.SharedTileSet(params, tile, 64, n, flips=3, pad=2)
    for lap in range(2):
        for k, plane in enumerate(frames):
            idx, tile_map = Carved(w * h, 1, plane), Carved(4 * n, 0)
            torch.cuda.synchronize()
            kept.add(idx.ptr, map_out=tile_map.ptr)
            count, first_new, added = kept.fetch()
            tiles, t_map, t_out, t_in = exp[k]
            assert (count, first_new) == (t_out, t_in), (lap, k)
            assert added.shape == (min(t_out, 64) - min(t_in, 64), 8, 8) and added.tobytes() == tiles[min(t_in, 64):].tobytes()
            assert tile_map.guards_intact() and tile_map.host(np.uint32).tobytes() == t_map.tobytes()
        assert exp[-1][2] > exp[0][2]
        kept.reset()
    kept.add(idx.ptr, rows=(0, 64))
    assert kept.fetch()[0] == TS.model(frames[2][:64 * w], w, 64, tile, 2, 3)[2]
    with pytest.raises(Exception):
        ext.SharedTileSet(params, tile, 8, 4).add(idx.ptr)


# ---- 12. in a frame loop -------------------------------------------------------------------------------------------------

def test_in_a_frame_loop(par, ext, tileset, oracle, T):
    """The graybox scene with boxes that move, four frames: each is rendered, its palette fitted at 33, quantised by the
    cells call, its index plane added to the shared set and drawn back from the shared set, on one stream with one wait
    a frame. Every frame's plane comes back byte for byte and the counts are the model's."""
    import torch
    import cells as CM
    import palette as P
    from test_gpu_light_range import lights_with, scene
    from test_gpu_lights_graph import Planes as FramePlanes
    from test_gpu_palette import Block, garbage_work
    from test_gpu_parity import ALL

    cells = importlib.import_module("pixel-art-raytracer_amd.cells")
    sc = scene("graybox", par, oracle, T)
    params = sc.params
    W, H = params.width, params.height
    N, TILE, CAP = 33, (8, 8), 1024
    n = TS.grid(W, H, TILE)[0] * TS.grid(W, H, TILE)[1]
    stream = torch.cuda.Stream()
    out = FramePlanes(params, ALL)
    block = Block(T, garbage_work(T, 83))
    d_fitted = Carved(4 * N, 0)
    index, redrawn, tile_map = Carved(W * H, 1), Carved(W * H, 2), Carved(4 * n, 0)
    shared = Shared(ext, T, TILE, CAP)
    work = Carved(ext.tileset_extend_work_bytes(n, CAP), 0)
    torch.cuda.synchronize()
    counts, stored, t = [], TX.no_tiles(TILE), 0
    with sc.renderer(par) as r:
        s = stream.cuda_stream
        r.set_lights(lights_with(T, [sc.positions[3]], [0]))
        for frame in range(4):
            aabbs = sc.aabbs.copy()
            aabbs["px"][:4] += 3 * frame
            r.set_entities(aabbs, sc.sprite_ids)
            r.render_device(out.ptrs, stream=s)
            par.palette_reset(block.ptr, stream=s)
            par.palette_count(params, out.ptrs["fb"], (0, H), block.ptr, stream=s)
            par.palette_cut(block.ptr, N, stream=s)
            par.palette_sum(params, out.ptrs["fb"], (0, H), block.ptr, stream=s)
            par.palette_emit(block.ptr, N, d_fitted.ptr, stream=s)
            cells.quantize_cells(params, d_fitted.ptr, 3, 11, TILE, out.ptrs["fb"], (0, H), index_out=index.ptr, stream=s)
            shared.launch(index, (0, H), H, W, work, tile_map, 0, 3, stream=s)
            tileset.tileset_expand(params, shared.tiles.ptr, CAP, TILE, tile_map.ptr, (0, H), redrawn.ptr, stream=s)
            stream.synchronize()
            plane = index.host(np.uint8)
            exp = TX.model(stored, t, plane, W, H, TILE, 0, 3, CAP)
            stored, t = exp[0], exp[2]
            assert t <= CAP, "the test's capacity holds the animation"
            assert int(shared.count.host(np.uint32)[0]) == exp[2] and int(shared.first.host(np.uint32)[0]) == exp[3], frame
            assert tile_map.host(np.uint32).tobytes() == exp[1].tobytes(), frame
            assert shared.tiles.host(np.uint8)[:stored.size].tobytes() == stored.tobytes(), frame
            assert redrawn.host(np.uint8).tobytes() == plane.tobytes(), f"frame {frame}: the plane from the shared set"
            for buf in (index, redrawn, tile_map, work, shared.tiles, shared.count, shared.first, d_fitted):
                assert buf.guards_intact()
            counts.append((exp[3], exp[2]))
        r.stats()
    print(counts)
    assert counts[0][0] == 0 and all(b > a for a, b in counts) and counts[3][1] - counts[3][0] < counts[0][1]
