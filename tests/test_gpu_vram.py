"""GPU tests of VRAM export (the add-on of addons/include/par_vram.h): the local plane, the encoded and decoded tiles, the
map words and both bad counts byte for byte against the contract restated in numpy (tests/vram.py; tests/test_vram_cpu.py
holds it to a loop over pixels and bits without a GPU), on buffers carved out of guard-filled tensors (Carved of
test_gpu_quantize.py). After every call the guards round every buffer are checked, the inputs are unchanged, and `out`
beyond the n tiles encoded still holds its poison.

The sizes, by what they cross in the implementation. An encode or decode takes a wavefront an 8 x 8 sub-tile and four
wavefronts a workgroup, so a workgroup holds four, two or one tile: 0, 1, 3, 4, 5, 63, 64, 65 and 1025 tiles are nothing, a
part of a workgroup, a whole one, one more, and many with a ragged last one at every tile size. The launch is sized by the
capacity, so a count below it leaves whole workgroups without work. The map takes a thread a cell, 256 a workgroup; the
local plane eight bytes a thread with a bytewise tail."""
import importlib

import numpy as np
import pytest

import tileset as TS
import vram as V
from test_gpu_quantize import GUARD, Carved
from test_gpu_tileset import upload

pytestmark = pytest.mark.gpu

VRAM = importlib.import_module("pixel-art-raytracer_amd.vram")  # (without the add-on's binding nothing here can run)
COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 1025)
POISON = 0x0BADF00D


@pytest.fixture(scope="module")
def vram():
    return VRAM


def layout_struct(vram, L):
    return vram.MapLayout(*(L[f] for f in V.FIELDS))


def random_tiles(rng, n, tile, bpp, dirty):
    """n tiles below 2^bpp; dirty 1 puts one byte too large into one tile's last sub-tile, 2 into every tile."""
    tiles = rng.integers(0, 1 << bpp, (n, tile[1], tile[0]), dtype=np.uint8)
    if dirty == 1 and n:
        tiles[n // 2, tile[1] - 1, tile[0] - 3] |= 1 << bpp
    elif dirty == 2:
        tiles[:, rng.integers(0, tile[1]), rng.integers(0, tile[0])] |= 0x80
    return tiles


def encoded(vram, tiles, tile, fmt, count, phases=(0, 0), with_bad=True, stream=None, tag=""):
    """One par_vram_encode_tiles_device over the set `tiles` with the device count `count` (None: a null count), checked."""
    import torch
    capacity, each = len(tiles), V.tile_bytes(fmt, tile)
    src = Carved(tiles.size, phases[0], tiles.reshape(-1))
    out = Carved(capacity * each, phases[1])
    d_count = Carved(4, 4, np.array([count], np.uint32)) if count is not None else None
    bad = Carved(4, 8, np.array([POISON], np.uint32)) if with_bad else None
    torch.cuda.synchronize()
    vram.encode_tiles(src.ptr, capacity, d_count.ptr if d_count else None, tile, fmt, out.ptr, bad_out=bad.ptr if bad else None,
                      stream=stream)
    torch.cuda.synchronize()
    n = capacity if count is None else min(count, capacity)
    e_data, e_bad = V.encode_tiles(tiles[:n], tile, fmt)
    for name, buf in (("tiles", src), ("out", out), ("count", d_count), ("bad_out", bad)):
        assert buf is None or buf.guards_intact(), f"{tag}: {name}: bytes outside the buffer were written"
    assert src.host(np.uint8).tobytes() == tiles.tobytes(), f"{tag}: the tiles were written"
    assert d_count is None or int(d_count.host(np.uint32)[0]) == count, f"{tag}: the count was written"
    got = out.host(np.uint8)
    wrong = np.nonzero(got[:n * each] != e_data)[0]
    assert len(wrong) == 0, f"{tag}: {len(wrong)} bytes differ, first at {wrong[:4]}: {got[wrong[:4]]} for {e_data[wrong[:4]]}"
    assert (got[n * each:] == GUARD).all(), f"{tag}: out beyond {n} tiles was written"
    if bad is not None:
        assert int(bad.host(np.uint32)[0]) == e_bad, f"{tag}: bad is {int(bad.host(np.uint32)[0])}, the model's {e_bad}"
    return e_bad


def decoded(vram, data, n_tiles, tile, fmt, phases=(0, 0), tag=""):
    import torch
    src = Carved(data.size, phases[0], data)
    out = Carved(n_tiles * tile[0] * tile[1], phases[1])
    torch.cuda.synchronize()
    vram.decode_tiles(src.ptr, n_tiles, tile, fmt, out.ptr)
    torch.cuda.synchronize()
    assert src.guards_intact() and out.guards_intact(), f"{tag}: bytes outside a buffer were written"
    assert src.host(np.uint8).tobytes() == data.tobytes(), f"{tag}: the data was written"
    exp = V.decode_tiles(data, tile, fmt).reshape(-1)
    got = out.host(np.uint8)
    wrong = np.nonzero(got != exp)[0]
    assert len(wrong) == 0, f"{tag}: {len(wrong)} pixels differ, first at {wrong[:4]}: {got[wrong[:4]]} for {exp[wrong[:4]]}"
    return got


# ---- 1. encode ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", V.FORMATS, ids=V.FORMAT_NAMES)
def test_encode_every_tile_size_and_count(vram, fmt):
    """Every count of the list as *count equal to, above and below the capacity, and as a null count; clean sets, one bad
    tile and all bad tiles go round with the cases, and every fourth call has no bad_out."""
    rng = np.random.default_rng(100 + fmt)
    bpp = V.BPP[fmt]
    i, bad_seen = 0, set()
    for tile in TS.TILES:
        for n in COUNTS:
            cases = [(max(n, 1), n), (max(n, 1), n + 5), (n + 2, n)] + ([(n, None)] if n else [])
            for capacity, count in cases:
                if tile != (8, 8) and n == 1025 and count != n:
                    continue  # (the largest set once a tile size, and in every way at 8 x 8)
                tiles = random_tiles(rng, capacity, tile, bpp, i % 3)
                e_bad = encoded(vram, tiles, tile, fmt, count, with_bad=i % 4 != 3, tag=f"{V.FORMAT_NAMES[fmt]} {tile} capacity {capacity} count {count}")
                encoded_tiles = capacity if count is None else min(count, capacity)
                if encoded_tiles >= 2:
                    bad_seen.add({0: "none", 1: "one", encoded_tiles: "all"}.get(e_bad, "some"))
                i += 1
    assert {"none", "one", "all"} <= bad_seen, "clean sets, one bad tile and all tiles bad were all met"


@pytest.mark.parametrize("fmt", V.FORMATS, ids=V.FORMAT_NAMES)
def test_encode_every_byte_phase(vram, fmt):
    rng = np.random.default_rng(200 + fmt)
    for a in range(4):
        for b in range(4):
            tile = TS.TILES[(a + b) % 4]
            tiles = random_tiles(rng, 6, tile, V.BPP[fmt], (a + b) % 3)
            encoded(vram, tiles, tile, fmt, 5, phases=(a, b), tag=f"{V.FORMAT_NAMES[fmt]} {tile} phases {a} {b}")


def test_encode_counts_bad_tiles_not_bytes_or_sub_tiles(vram):
    """A 16 x 16 tile with a byte too large in each of its four sub-tiles is one bad tile; tiles beyond the count are not
    counted; only the low bits are encoded."""
    rng = np.random.default_rng(3)
    tiles = rng.integers(0, 4, (9, 16, 16), dtype=np.uint8)
    tiles[2, ::8, ::8] = 0xFF
    tiles[4, 15, 0] = 4
    tiles[7] = 0xFF  # beyond the count below
    assert encoded(vram, tiles, (16, 16), V.F_2BPP_PLANAR, 6, tag="16 x 16") == 2
    assert encoded(vram, tiles, (16, 16), V.F_2BPP_ROWS, None, tag="16 x 16, all") == 3
    assert encoded(vram, tiles.reshape(-1, 8, 8), (8, 8), V.F_4BPP_ROWS, None, tag="as rows of 64 bytes") == 2 + 4


@pytest.mark.parametrize("fmt", V.FORMATS, ids=V.FORMAT_NAMES)
def test_the_anchors_and_the_sub_tile_order_on_the_device(vram, fmt):
    """The hand-worked tiles of the header through the device, and a 16 x 16 tile whose quadrants differ."""
    from test_vram_cpu import ANCHORS, one_tile
    for name, f, pixels, want in ANCHORS:
        if f != fmt:
            continue
        host = vram.encode_tiles_host(one_tile(*pixels), (8, 8), fmt)
        exp = np.zeros(8 * V.BPP[fmt], dtype=np.uint8)
        for at, byte in want.items():
            exp[at] = byte
        assert host["data"].tolist() == exp.tolist() and host["bad"] == 0, name
    quadrants = np.zeros((1, 16, 16), dtype=np.uint8)
    quadrants[0, :8, 8:], quadrants[0, 8:, :8], quadrants[0, 8:, 8:] = 1, 0, 1
    quadrants[0, 8, 0] = 1
    encoded(vram, quadrants, (16, 16), fmt, None, tag="quadrants")


# ---- 2. decode -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", V.FORMATS, ids=V.FORMAT_NAMES)
def test_decode_every_tile_size_and_count(vram, fmt):
    rng = np.random.default_rng(300 + fmt)
    for tile in TS.TILES:
        for n in COUNTS[1:]:
            data = rng.integers(0, 256, n * V.tile_bytes(fmt, tile), dtype=np.uint8)
            got = decoded(vram, data, n, tile, fmt, tag=f"{V.FORMAT_NAMES[fmt]} {tile} {n} tiles")
            assert got.max() < 1 << V.BPP[fmt]
            if n in (5, 65):
                # encode(decode(d)) == d, on the device both ways
                encoded(vram, got.reshape(n, tile[1], tile[0]), tile, fmt, None, tag="back again")
                assert V.encode_tiles(got, tile, fmt)[0].tobytes() == data.tobytes()


@pytest.mark.parametrize("fmt", V.FORMATS, ids=V.FORMAT_NAMES)
def test_decode_every_byte_phase(vram, fmt):
    rng = np.random.default_rng(400 + fmt)
    for a in range(4):
        for b in range(4):
            tile = TS.TILES[(a + 2 * b) % 4]
            data = rng.integers(0, 256, 5 * V.tile_bytes(fmt, tile), dtype=np.uint8)
            decoded(vram, data, 5, tile, fmt, phases=(a, b), tag=f"{V.FORMAT_NAMES[fmt]} {tile} phases {a} {b}")


# ---- 3. map words --------------------------------------------------------------------------------------------------------

def mapped(vram, L, tile_map, gcx, gcy, cells, ratio, phase=0, with_bad=True, tag=""):
    import torch
    n, wb = gcx * gcy, L["word_bytes"]
    src = Carved(4 * n, 4, tile_map)
    d_cells = Carved(len(cells), 1, cells) if cells is not None else None
    out = Carved(n * wb, phase)
    bad = Carved(4, 4, np.array([POISON], np.uint32)) if with_bad else None
    torch.cuda.synchronize()
    vram.encode_map(layout_struct(vram, L), src.ptr, (gcx, gcy), out.ptr, cells=d_cells.ptr if d_cells else None, ratio=ratio,
                    bad_out=bad.ptr if bad else None)
    torch.cuda.synchronize()
    e_data, e_bad = V.encode_map(L, tile_map, gcx, gcy, cells, ratio)
    for name, buf in (("map", src), ("cells", d_cells), ("out", out), ("bad_out", bad)):
        assert buf is None or buf.guards_intact(), f"{tag}: {name}: bytes outside the buffer were written"
    assert src.host(np.uint32).tobytes() == tile_map.tobytes(), f"{tag}: the map was written"
    assert d_cells is None or d_cells.host(np.uint8).tobytes() == cells.tobytes(), f"{tag}: the cells were written"
    got = out.host(np.uint8)
    wrong = np.nonzero(got != e_data)[0]
    assert len(wrong) == 0, f"{tag}: {len(wrong)} bytes differ, first at {wrong[:4]}: {got[wrong[:4]]} for {e_data[wrong[:4]]}"
    if bad is not None:
        assert int(bad.host(np.uint32)[0]) == e_bad, f"{tag}: bad is {int(bad.host(np.uint32)[0])}, the model's {e_bad}"
    return e_bad


def random_map(rng, n, id_bits, flips=True):
    ids = rng.integers(0, 1 << id_bits, n).astype(np.uint32)
    return ids | (rng.integers(0, 4, n).astype(np.uint32) << 30 if flips else np.uint32(0))


LAYOUTS = [(V.MACHINES[m], V.preset(m)) for m in range(6)] + [
    ("one byte", V.layout_of(word_bytes=1, tile_bits=4, pal_shift=4, pal_bits=2, flip_x_bit=6, flip_y_bit=7, tile_step=3, tile_base=2)),
    ("four bytes, little", V.layout_of(word_bytes=4, tile_bits=20, pal_shift=20, pal_bits=8, flip_x_bit=30, flip_y_bit=31, set_bits=1 << 29)),
    ("four bytes, big", V.layout_of(word_bytes=4, big_endian=1, tile_bits=32, pal_shift=3, pal_bits=0, flip_x_bit=-1, flip_y_bit=31,
                                    tile_step=16, tile_base=65535, set_bits=-(1 << 31))),
    ("two bytes, big, no flips", V.layout_of(big_endian=1, tile_bits=16, pal_bits=0, flip_x_bit=-1, flip_y_bit=-1)),
    ("two bytes, little, set bits", V.layout_of(tile_bits=8, pal_shift=8, pal_bits=4, flip_x_bit=12, flip_y_bit=-1, set_bits=0x8000)),
]


@pytest.mark.parametrize("name,L", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_map_every_layout_grid_and_ratio(vram, name, L):
    """gcx of 1, 7, 8 and 9 under both ratios each way (an odd gcx under ratio 2 has a ragged last colour cell), a null
    `cells`, and every output phase."""
    rng = np.random.default_rng(sum(name.encode()))
    i = 0
    for gcx in (1, 7, 8, 9):
        for ratio in ((1, 1), (2, 2), (2, 1), (1, 2)):
            gcy = (5, 1, 12, 3)[i % 4]
            tile_map = random_map(rng, gcx * gcy, min(30, L["tile_bits"] + (i % 3 == 0)))
            cells = rng.integers(0, min(256, (1 << L["pal_bits"]) + (i % 5 == 0)), V.colour_cells(gcx, gcy, ratio), dtype=np.uint8)
            mapped(vram, L, tile_map, gcx, gcy, cells if i % 4 != 2 else None, ratio, phase=i % 4, with_bad=i % 7 != 6,
                   tag=f"{name} {gcx} x {gcy} ratio {ratio}")
            i += 1


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_map_cell_counts(vram, n):
    rng = np.random.default_rng(n)
    for i, (gcx, gcy) in enumerate(((n, 1), (1, n))):
        L = LAYOUTS[(n + 5 * i) % len(LAYOUTS)][1]
        ratio = ((2, 1), (1, 2))[i]
        cells = rng.integers(0, 1 << min(8, L["pal_bits"] + 1), V.colour_cells(gcx, gcy, ratio), dtype=np.uint8)
        mapped(vram, L, random_map(rng, n, 12), gcx, gcy, cells, ratio, phase=1 + i, tag=f"{gcx} x {gcy}")


def test_map_of_the_largest_grid(vram):
    rng = np.random.default_rng(20)
    tile_map = random_map(rng, 1 << 20, 11)
    cells = rng.integers(0, 9, V.colour_cells(1024, 1024, (2, 2)), dtype=np.uint8)
    bad = mapped(vram, V.preset(V.SNES), tile_map, 1024, 1024, cells, (2, 2), phase=3, tag="1024 x 1024")
    assert 0 < bad < 1 << 20


def test_map_each_bad_condition_alone(vram):
    """A tile number too large, a palette too large and a flip the layout has no bit for, one cell each, then all three
    in one cell: bad_out counts cells."""
    L = V.preset(V.NES)
    clean = np.array([5, 255, 0, 17, 200, 9], dtype=np.uint32)
    cells = np.zeros(6, dtype=np.uint8)
    assert mapped(vram, L, clean, 3, 2, cells, (1, 1), tag="clean") == 0
    for tag, at, entry, pal in (("tile", 1, 256, 0), ("palette", 2, 0, 1), ("x flip", 3, 17 | 1 << 30, 0), ("y flip", 4, 200 | 1 << 31, 0),
                                ("all at once", 5, 300 | 3 << 30, 7)):
        tile_map, chosen = clean.copy(), cells.copy()
        tile_map[at], chosen[at] = entry, pal
        assert mapped(vram, L, tile_map, 3, 2, chosen, (1, 1), tag=tag) == 1, tag
    G = V.preset(V.GBC)
    assert mapped(vram, G, np.array([255 | 3 << 30], np.uint32), 1, 1, np.array([7], np.uint8), (1, 1), tag="gbc, full") == 0
    assert mapped(vram, G, np.array([255], np.uint32), 1, 1, np.array([8], np.uint8), (1, 1), tag="gbc, palette 8") == 1
    # the header's anchors through the device: tile 5, palette 3, x flip
    for machine, want in ((V.SNES, [0x05, 0x4C]), (V.MEGADRIVE, [0x68, 0x05]), (V.GBA, [0x05, 0x34]), (V.NES, [0x05])):
        host = vram.encode_map_host(vram.map_layout_preset(machine), np.array([5 | 1 << 30], np.uint32), (1, 1), cells=np.array([3], np.uint8))
        assert host["data"].tolist() == want and host["bad"] == int(machine == V.NES), V.MACHINES[machine]


# ---- 4. the local plane --------------------------------------------------------------------------------------------------

def localised(vram, plane, sub_size, phases=(0, 0), in_place=False, tag=""):
    import torch
    src = Carved(plane.size, phases[0], plane)
    out = src if in_place else Carved(plane.size, phases[1])
    torch.cuda.synchronize()
    vram.local(src.ptr, plane.size, sub_size, out.ptr)
    torch.cuda.synchronize()
    assert src.guards_intact() and out.guards_intact(), f"{tag}: bytes outside a buffer were written"
    if not in_place:
        assert src.host(np.uint8).tobytes() == plane.tobytes(), f"{tag}: the index plane was written"
    got, exp = out.host(np.uint8), plane % sub_size if sub_size < 256 else plane
    wrong = np.nonzero(got != exp)[0]
    assert len(wrong) == 0, f"{tag}: {len(wrong)} bytes differ, first at {wrong[:4]}: {got[wrong[:4]]} for {exp[wrong[:4]]}"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100003])
def test_local_sizes_sub_sizes_and_phases(vram, n):
    rng = np.random.default_rng(n)
    plane = rng.integers(0, 256, n, dtype=np.uint8)
    i = 0
    for sub_size in (1, 3, 4, 16, 256):
        for a in range(4):
            localised(vram, plane, sub_size, phases=(a, (a + i) % 4), tag=f"{n} bytes, K {sub_size}, phases {a} {(a + i) % 4}")
            localised(vram, plane, sub_size, phases=(a, a), in_place=True, tag=f"{n} bytes, K {sub_size}, in place at phase {a}")
            i += 1


def test_local_every_byte_under_every_sub_size(vram):
    """All 256 byte values under each K of 1 .. 256 (the kernel divides by a multiplication), whole eights and a tail."""
    import torch
    plane = np.concatenate([np.arange(256, dtype=np.uint8), np.arange(255, 252, -1, dtype=np.uint8)])
    src, out = Carved(plane.size, 1, plane), Carved(256 * 264, 3)
    torch.cuda.synchronize()
    for k in range(1, 257):
        vram.local(src.ptr, plane.size, k, out.ptr + (k - 1) * 264)
    torch.cuda.synchronize()
    assert src.guards_intact() and out.guards_intact() and src.host(np.uint8).tobytes() == plane.tobytes()
    got = out.host(np.uint8).reshape(256, 264)
    for k in range(1, 257):
        assert got[k - 1, :259].tobytes() == (plane.astype(np.uint32) % k).astype(np.uint8).tobytes(), f"K {k}"
    assert (got[:, 259:] == GUARD).all()


# ---- 5. the host forms ---------------------------------------------------------------------------------------------------

def test_host_forms(vram):
    rng = np.random.default_rng(50)
    tiles = random_tiles(rng, 7, (16, 8), 4, 1)
    keep = tiles.copy()
    got = vram.encode_tiles_host(tiles, (16, 8), V.F_4BPP_PACKED_HI, count=5)
    e_data, e_bad = V.encode_tiles(tiles[:5], (16, 8), V.F_4BPP_PACKED_HI)
    assert sorted(got) == ["bad", "data"] and got["data"].tobytes() == e_data.tobytes() and got["bad"] == e_bad == 1
    assert tiles.tobytes() == keep.tobytes()
    none = vram.encode_tiles_host(tiles, (16, 8), V.F_4BPP_PACKED_HI, count=0)
    assert none["data"].size == 0 and none["bad"] == 0
    back = vram.decode_tiles_host(got["data"], (16, 8), V.F_4BPP_PACKED_HI)
    assert back.shape == (5, 8, 16) and back.tobytes() == (tiles[:5] & 15).tobytes()
    tile_map = random_map(rng, 7 * 5, 11)
    cells = rng.integers(0, 5, V.colour_cells(7, 5, (2, 2)), dtype=np.uint8)
    for machine in (V.MEGADRIVE, V.GBC):
        got = vram.encode_map_host(vram.map_layout_preset(machine), tile_map, (7, 5), cells=cells, ratio=(2, 2), device=0)
        e_data, e_bad = V.encode_map(V.preset(machine), tile_map, 7, 5, cells, (2, 2))
        assert got["data"].tobytes() == e_data.tobytes() and got["bad"] == e_bad > 0, V.MACHINES[machine]
    got = vram.encode_map_host(vram.map_layout_preset(V.SNES), tile_map & np.uint32(0xC00003FF), (7, 5))
    assert got["data"].tobytes() == V.encode_map(V.preset(V.SNES), tile_map & np.uint32(0xC00003FF), 7, 5)[0].tobytes() and got["bad"] == 0


# ---- 6. captured -----------------------------------------------------------------------------------------------------------

class Chain:
    """The buffers of local -> build -> encode tiles -> encode map over a w x h cells index plane of 8 x 8 tiles, and the
    launches on a stream."""

    def __init__(self, vram, tileset, T, w, h, cell, sub_size, machine, flips, capacity):
        self.vram, self.tileset, self.params = vram, tileset, T.default_params(w, h)
        self.w, self.h, self.cell, self.sub_size, self.machine, self.flips, self.capacity = w, h, cell, sub_size, machine, flips, capacity
        self.gcx, self.gcy = TS.grid(w, h, (8, 8))
        self.n = self.gcx * self.gcy
        self.fmt = V.MACHINE_FORMATS[machine][0]
        self.L = V.preset(machine)
        self.layout = layout_struct(vram, self.L)
        self.ratio = (cell[0] // 8, cell[1] // 8)
        self.index, self.local = Carved(w * h, 1), Carved(w * h, 3)
        self.chosen = Carved(V.colour_cells(self.gcx, self.gcy, self.ratio), 1)
        self.work = Carved(tileset.tileset_work_bytes(self.n), 0)
        self.tiles, self.tile_map, self.count = Carved(capacity * 64, 2), Carved(4 * self.n, 4), Carved(4, 4)
        self.chr = Carved(capacity * V.tile_bytes(self.fmt, (8, 8)), 1)
        self.words = Carved(self.n * self.L["word_bytes"], 3)
        self.bad_tiles, self.bad_cells = Carved(4, 4), Carved(4, 8)
        self.outputs = (self.local, self.work, self.tiles, self.tile_map, self.count, self.chr, self.words, self.bad_tiles, self.bad_cells)

    def launch(self, stream=None):
        v, s = self.vram, stream
        v.local(self.index.ptr, self.w * self.h, self.sub_size, self.local.ptr, stream=s)
        self.tileset.tileset_build(self.params, self.local.ptr, (0, self.h), (8, 8), self.work.ptr, self.count.ptr,
                                   tiles_out=self.tiles.ptr, capacity=self.capacity, map_out=self.tile_map.ptr, flips=self.flips, stream=s)
        v.encode_tiles(self.tiles.ptr, self.capacity, self.count.ptr, (8, 8), self.fmt, self.chr.ptr, bad_out=self.bad_tiles.ptr, stream=s)
        v.encode_map(self.layout, self.tile_map.ptr, (self.gcx, self.gcy), self.words.ptr, cells=self.chosen.ptr, ratio=self.ratio,
                     bad_out=self.bad_cells.ptr, stream=s)

    def check(self, index, chosen, tag):
        exp = V.export(TS, index, chosen, self.sub_size, self.w, self.h, self.cell, self.machine, self.flips)
        for buf in (self.index, self.chosen, *self.outputs):
            assert buf.guards_intact(), f"{tag}: bytes outside a buffer were written"
        assert self.index.host(np.uint8).tobytes() == index.tobytes() and self.chosen.host(np.uint8).tobytes() == chosen.tobytes(), tag
        assert self.local.host(np.uint8).tobytes() == (index % self.sub_size).tobytes(), f"{tag}: the local plane"
        count = int(self.count.host(np.uint32)[0])
        assert count == exp["count"] <= exp["flat"], f"{tag}: T is {count}, the model's {exp['count']}"
        kept = min(count, self.capacity)
        each = V.tile_bytes(self.fmt, (8, 8))
        assert self.tile_map.host(np.uint32).tobytes() == exp["map"].tobytes(), f"{tag}: the tile map"
        got = self.chr.host(np.uint8)
        assert got[:kept * each].tobytes() == exp["chr"][:kept * each].tobytes(), f"{tag}: the encoded tiles"
        assert (got[kept * each:] == GUARD).all(), f"{tag}: tiles beyond the count were encoded"
        assert self.words.host(np.uint8).tobytes() == exp["map_bytes"].tobytes(), f"{tag}: the map words"
        bad = int(self.bad_tiles.host(np.uint32)[0]) + int(self.bad_cells.host(np.uint32)[0])
        assert bad == exp["bad"], f"{tag}: bad is {bad}, the model's {exp['bad']}"
        return exp


def test_captured_and_replayed_on_a_plane_with_another_tile_count(vram, T):
    """local -> build -> encode tiles -> encode map captured with torch.cuda.graph after one eager run, replayed on other
    planes: every output follows the count the stream then finds; one wait a replay."""
    import torch
    from test_vram_cpu import cells_plane
    tileset = importlib.import_module("pixel-art-raytracer_amd.tileset")
    w, h, cell = 131, 67, (16, 16)
    rng = np.random.default_rng(60)
    planes = [cells_plane(rng, w, h, cell, 8, 16, kinds) for kinds in (3, 17, 40)]
    chain = Chain(vram, tileset, T, w, h, cell, 16, V.SNES, 3, 17 * 9)
    stream = torch.cuda.Stream()

    def load(k):
        for buf in chain.outputs:
            buf.t.fill_(GUARD)
        upload(chain.index, planes[k][0])
        upload(chain.chosen, planes[k][1])
        torch.cuda.synchronize()

    load(0)
    chain.launch(stream=stream.cuda_stream)
    stream.synchronize()
    chain.check(*planes[0], "eagerly")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        chain.launch(stream=stream.cuda_stream)
    counts = set()
    for k in (1, 2, 0, 1):
        load(k)
        with torch.cuda.stream(stream):
            graph.replay()
        stream.synchronize()
        counts.add(chain.check(*planes[k], f"replay on plane {k}")["count"])
    assert len(counts) == 3


# ---- 7. in a frame loop --------------------------------------------------------------------------------------------------

def test_in_a_frame_loop(par, vram, oracle, T):
    """The graybox scene under two tinted ranged lights: render_device, the palette fitted at 33, the cells fitted at 8 x 4
    over 8 x 8 cells, the frame quantised under that table, the local plane, its tile set under both mirrors, and the set
    and the map encoded for the SNES, all on the frame's stream with one wait at the end. What comes back gives the cells
    index plane again (the closing identity)."""
    import torch
    import cells as CL
    import cells_fit as CF
    import palette as P
    from test_gpu_light_range import scene
    from test_gpu_light_tints import COLOUR, TINTS, expected
    from test_gpu_lights_graph import Planes as FramePlanes
    from test_gpu_palette import Block, garbage_work
    from test_gpu_parity import ALL, assert_planes_equal
    from test_vram_cpu import GRAYBOX

    cells = importlib.import_module("pixel-art-raytracer_amd.cells")
    fit = importlib.import_module("pixel-art-raytracer_amd.cells_fit")
    tileset = importlib.import_module("pixel-art-raytracer_amd.tileset")
    sc = scene("graybox", par, oracle, T)
    params = sc.params
    W, H = params.width, params.height
    lights, exp, _ = expected(T, sc, [3, 6], [200, 300], TINTS[:2], COLOUR, "graybox, two tinted ranged lights")
    fb = exp["fb"]
    N, CELL, S, K = 33, (8, 8), 8, 4
    master = P.fit(T, fb, N)[0]
    e_table = CF.model(fb, W, H, CELL, master, S, K, 0)[0]
    e_index, _, e_chosen = CL.model(params, e_table, S, K, CELL, fb, None, 0)

    stream = torch.cuda.Stream()
    out = FramePlanes(params, ALL)
    block = Block(T, garbage_work(T, 85))
    d_master, d_table = Carved(4 * N, 0), Carved(4 * S * K, 0)
    fit_work = Carved(fit.cells_fit_work_bytes(W, H, CELL), 0)
    chain = Chain(vram, tileset, T, W, H, CELL, K, V.SNES, 3, 1024)
    torch.cuda.synchronize()
    with sc.renderer(par, par.LIGHTS_RANGED) as r:
        r.set_lights(lights)
        r.set_light_tints(T.make_tints(TINTS[:2]))
        s = stream.cuda_stream
        r.render_device(out.ptrs, flags=par.RENDER_COUNT_RAYS, stream=s)
        par.palette_reset(block.ptr, stream=s)
        par.palette_count(params, out.ptrs["fb"], (0, H), block.ptr, stream=s)
        par.palette_cut(block.ptr, N, stream=s)
        par.palette_sum(params, out.ptrs["fb"], (0, H), block.ptr, stream=s)
        par.palette_emit(block.ptr, N, d_master.ptr, stream=s)
        fit.cells_fit(out.ptrs["fb"], W, H, CELL, d_master.ptr, N, S, K, 0, fit_work.ptr, d_table.ptr, stream=s)
        cells.quantize_cells(params, d_table.ptr, S, K, CELL, out.ptrs["fb"], (0, H), index_out=chain.index.ptr,
                             cell_out=chain.chosen.ptr, stream=s)
        chain.launch(stream=s)
        stream.synchronize()
        assert_planes_equal(out.host(T), exp, ALL, "the frame itself")
        assert d_master.guards_intact() and d_table.guards_intact() and fit_work.guards_intact()
        assert d_table.host(T.COLOR).tobytes() == e_table.tobytes(), "the fitted table"
        got = chain.check(e_index, e_chosen, "the frame loop")
        assert (got["count"], got["flat"]) == GRAYBOX[(8, 3)] and got["bad"] == 0
        # the closing identity on what came back from the device
        back = dict(got, chr=chain.chr.host(np.uint8)[:got["count"] * 32].copy(), map_bytes=chain.words.host(np.uint8).copy())
        assert V.closing_identity(TS, back, e_chosen, K, W, H).tobytes() == e_index.tobytes()
        r.stats()
