"""Shared tile sets without a GPU: the three calls are declared in include/par_tileset_extend.h (and in no other
header), exported and wrapped by the tileset_extend module (tests/test_abi_cpu.py holds the binding's table to the header's
prototypes and compiles the header as pedantic C11 alone, twice and beside the other three in any order); every
PAR_ERR_INVALID_ARG of both calls comes back before any device work and with nothing written, each rule on its own;
par_tileset_extend_work_bytes is the header's formula and keeps its bound; the vectorised model the GPU tests lean on
(tileset_extend.model) equals a per-cell loop with one dict on random sequences and on crafted sets worked out by hand; the
consequences the contract states hold; and the host form's copy arithmetic holds under a sanitiser
(tests/tileset_extend_spans_check.cpp, a stand-alone program)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import headers
import tileset as TS
import tileset_extend as TX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = 1
SYMBOLS = ("par_tileset_extend_work_bytes", "par_tileset_extend_device", "par_tileset_extend_host")
HEADER = "par_tileset_extend.h"


@pytest.fixture(scope="module")
def ext(par):
    return importlib.import_module("pixel-art-raytracer_amd.tileset_extend")


# ---- declared, exported, bound -------------------------------------------------------------------------------------

def test_declared_exported_and_bound(par, ext):
    assert tuple(name for _, name, _ in headers.prototypes(HEADER)) == SYMBOLS
    assert SYMBOLS == tuple(ext.ABI_TILESET_EXTEND) == ext.ABI_TILESET_EXTEND_SYMBOLS
    assert ext.ABI_TILESET_EXTEND is par.ABI_HEADERS[HEADER]
    for other in ("par_raytracer.h", "par_cells.h", "par_tileset.h", "par_types.h"):
        assert "par_tileset_extend" not in headers.text(other)
    wrappers = ("tileset_extend_work_bytes", "tileset_extend", "tileset_extend_host", "SharedTileSet")
    headers.assert_apart(par, HEADER, ext, wrappers)
    tileset = importlib.import_module("pixel-art-raytracer_amd.tileset")
    assert not any(hasattr(tileset, fn) for fn in wrappers)
    # the contract's headings, and what is left out on purpose, are in the header
    text = headers.text(HEADER)
    for word in ("removing tiles", "lossy merging", "persists between calls", "rotations", "torch.distributed", "2^30",
                 "low 30 bits", "Overflow", "Merge"):
        assert word in text, word


def test_the_prototypes_are_the_contracts():
    header = " ".join(headers.without_comments(HEADER).split())
    for proto in (
            "size_t par_tileset_extend_work_bytes(int n_cells, int capacity);",
            "int par_tileset_extend_device(const par_params* params, void* stream, const uint8_t* index, int row_begin, "
            "int row_end, int tile_w, int tile_h, int pad, int flips, void* work, uint8_t* tiles, int capacity, "
            "uint32_t* count, uint32_t* map_out, uint32_t* first_new_out);",
            "int par_tileset_extend_host(const par_params* params, int device, const uint8_t* index, int row_begin, "
            "int row_end, int tile_w, int tile_h, int pad, int flips, uint8_t* tiles, int capacity, int* count, "
            "uint32_t* map_out, int* first_new_out);"):
        assert proto in header, proto


# ---- par_tileset_extend_work_bytes -------------------------------------------------------------------------------------

def test_work_bytes_is_the_headers_formula_and_keeps_its_bound(ext):
    def formula(n, cap):
        p = 1
        while p < 2 * (n + cap):
            p *= 2
        return 4096 + 16 * n + 4 * p + 8

    sizes = (1, 2, 3, 15, 16, 17, 1000, 1023, 1024, 1025, 2400, 33024, (1 << 19) + 1, (1 << 20) - 1, 1 << 20)
    for n in sizes:
        for cap in (0,) + sizes:
            got = ext.tileset_extend_work_bytes(n, cap)
            assert got == formula(n, cap), (n, cap)
            assert got <= 4104 + 32 * (n + cap) and (got - 4104 - 16 * n) // 4 >= 2 * (n + cap), (n, cap)
            assert got % 8 == 0
    assert ext.tileset_extend_work_bytes(1 << 20, 1 << 20) == 4104 + 32 * (1 << 20)
    for n, cap in ((0, 4), (-1, 4), ((1 << 20) + 1, 4), ((1 << 31) - 1, 0), (4, -1), (4, (1 << 20) + 1), (4, (1 << 31) - 1),
                   (-(1 << 31), -(1 << 31))):
        assert ext.tileset_extend_work_bytes(n, cap) == 0, (n, cap)
    assert ext.lib().par_tileset_extend_work_bytes.restype is C.c_size_t


# ---- argument errors: no device needed, nothing written -----------------------------------------------------------

W, H = 24, 40
BAD = [
    ("null params", dict(params=None)),
    ("tile_w 4", dict(tile=(4, 8))),
    ("tile_w 12", dict(tile=(12, 8))),
    ("tile_w 32", dict(tile=(32, 8))),
    ("tile_w 0", dict(tile=(0, 8))),
    ("tile_h 4", dict(tile=(8, 4))),
    ("tile_h 32", dict(tile=(8, 32))),
    ("tile_h 0", dict(tile=(8, 0))),
    ("tile_h negative", dict(tile=(8, -8))),
    ("width 0", dict(width=0)),
    ("width negative", dict(width=-8)),
    ("row_begin negative", dict(rows=(-8, 8))),
    ("row_begin == row_end", dict(rows=(8, 8))),
    ("row_begin > row_end", dict(rows=(16, 8))),
    ("row_end > height", dict(rows=(0, 48))),
    ("tile_h 8: row_begin inside a cell", dict(rows=(4, 16))),
    ("tile_h 8: row_end inside a cell", dict(rows=(8, 12))),
    ("tile_h 16: row_begin inside a cell", dict(rows=(8, 32), tile=(8, 16))),
    ("tile_h 16: row_end inside a cell", dict(rows=(16, 24), tile=(8, 16))),
    ("tile_h 8: row_end inside the last cell", dict(rows=(32, 36), height=37)),
    ("one cell more than 2^20", dict(width=8 * 1025, height=8 * 1024, rows=(0, 8 * 1024))),
    ("far more cells than 2^20", dict(width=(1 << 31) - 1, height=(1 << 31) - 1, rows=(0, (1 << 31) - 1))),
    ("null index", dict(index=None)),
    ("null count", dict(count=None)),
    ("null tiles with capacity 1", dict(tiles=None, capacity=1)),
    ("capacity -1", dict(capacity=-1)),
    ("capacity -1 and null tiles", dict(tiles=None, capacity=-1)),
    ("capacity 2^20 + 1", dict(capacity=(1 << 20) + 1)),
    ("capacity 2^31 - 1", dict(capacity=(1 << 31) - 1)),
    ("pad -1", dict(pad=-1)),
    ("pad 256", dict(pad=256)),
    ("flips -1", dict(flips=-1)),
    ("flips 4", dict(flips=4)),
]
BAD_DEVICE = BAD + [("null work", dict(work=None)), ("work off its 8 bytes", dict(work_shift=4))]
BAD_HOST = BAD + [("*count -1", dict(count_value=-1)), ("*count the lowest int", dict(count_value=-(1 << 31)))]


def raw_call(ext, T, which, over):
    """One call of the raw symbol on host dummies: (status, whether any buffer changed)."""
    L = ext.lib()
    params = T.default_params(W, over.get("height", H))
    params.width = over.get("width", W)
    n = W * H
    bufs = {"index": np.full(n, 0xA5, np.uint8), "tiles": np.full(n, 0xC3, np.uint8), "map": np.full(n, 0x3C3C3C3C, np.uint32),
            "count": np.full(2, 3, np.int32), "first": np.full(2, 0x69696969, np.uint32),
            "work": np.full(4104 + 32 * (n + 4), 0x5A, np.uint8)}
    if "count_value" in over:
        bufs["count"][:] = over["count_value"]
    before = {k: v.copy() for k, v in bufs.items()}
    arg = dict(params=params, tile=(8, 8), rows=(0, params.height), pad=0, flips=3, capacity=4, **bufs)
    arg.update({k: v for k, v in over.items() if k not in ("width", "height", "work_shift", "count_value")})
    p = None if arg["params"] is None else C.byref(arg["params"])
    ptr = T.ptr
    work = ptr(arg["work"])
    if "work_shift" in over:
        work = C.c_void_p(arg["work"].ctypes.data + over["work_shift"])
    (tw, th), (r0, r1) = arg["tile"], arg["rows"]
    if which == "device":
        rc = L.par_tileset_extend_device(p, None, ptr(arg["index"]), r0, r1, tw, th, arg["pad"], arg["flips"], work,
                                         ptr(arg["tiles"]), arg["capacity"], ptr(arg["count"]), ptr(arg["map"]), ptr(arg["first"]))
    else:
        rc = L.par_tileset_extend_host(p, -1, ptr(arg["index"]), r0, r1, tw, th, arg["pad"], arg["flips"], ptr(arg["tiles"]),
                                       arg["capacity"], ptr(arg["count"]), ptr(arg["map"]), ptr(arg["first"]))
    return rc, any(bufs[k].tobytes() != before[k].tobytes() for k in bufs)


@pytest.mark.parametrize("which,bad", [("device", BAD_DEVICE), ("host", BAD_HOST)])
def test_invalid_arguments_need_no_device_and_write_nothing(ext, T, which, bad):
    assert len({tag for tag, _ in bad}) == len(bad)
    for tag, over in bad:
        rc, changed = raw_call(ext, T, which, over)
        assert rc == ERR_INVALID_ARG, f"{which}: {tag}: status {rc}"
        assert not changed, f"{which}: {tag}: something was written"


def test_what_the_rules_admit_is_not_refused(par, ext, T):
    """The host form on the arguments next to the refused ones (the device form would take host dummies for device
    memory): any status but PAR_ERR_INVALID_ARG, which without a GPU is PAR_ERR_NO_DEVICE."""
    want = 0 if par.device_count() > 0 else 2
    for over in (dict(), dict(rows=(8, 16)), dict(rows=(16, 32), tile=(8, 16)), dict(rows=(32, 37), tile=(16, 16), height=37),
                 dict(rows=(32, 37), height=37), dict(pad=255), dict(flips=0), dict(capacity=0), dict(capacity=0, tiles=None),
                 dict(map=None), dict(first=None), dict(map=None, first=None), dict(tile=(16, 8)), dict(count_value=0),
                 dict(count_value=4), dict(count_value=5), dict(capacity=W * H // 64)):
        rc, _ = raw_call(ext, T, "host", over)
        assert rc == want, (over, rc)


def test_binding_raises_and_checks_its_arrays(par, T, ext):
    params = T.default_params(16, 16)
    with pytest.raises(par.ParError) as e:
        ext.tileset_extend(params, 0, (0, 16), (8, 8), 0x1000, 0x2000, 4, 0x3000)
    assert e.value.status == ERR_INVALID_ARG and str(e.value) == "PAR_ERR_INVALID_ARG: par_tileset_extend_device"
    plane = np.zeros(256, np.uint8)
    with pytest.raises(par.ParError) as e:
        ext.tileset_extend_host(params, plane, (8, 12), np.zeros(0, np.uint8), 0, 4)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(par.ParError) as e:
        ext.tileset_extend_host(params, plane, (8, 8), np.zeros(0, np.uint8), -1, 4)
    assert e.value.status == ERR_INVALID_ARG and str(e.value) == "PAR_ERR_INVALID_ARG: par_tileset_extend_host"
    with pytest.raises(ValueError, match="tileset_extend_host: "):
        ext.tileset_extend_host(params, plane[:-1], (8, 8), np.zeros(0, np.uint8), 0, 4)
    for stored, count, capacity in ((np.zeros(64, np.uint8), 2, 4), (np.zeros(65, np.uint8), 1, 4), (np.zeros(3 * 64, np.uint8), 3, 2),
                                    (np.zeros(64, np.uint8), 0, 4)):
        with pytest.raises(ValueError, match="tileset_extend_host: tiles holds"):
            ext.tileset_extend_host(params, plane, (8, 8), stored, count, capacity)
    for bad in ("s", 1.5, np.int64(0x1000)):
        with pytest.raises(TypeError):
            ext.tileset_extend(params, bad, (0, 16), (8, 8), 0x1000, 0x2000, 4, 0x3000)
        with pytest.raises(TypeError):
            ext.tileset_extend(params, 0x1000, (0, 16), (8, 8), 0x1000, 0x2000, 4, 0x3000, stream=bad)


def test_arguments_reach_the_library_in_the_headers_order(par, T, ext, monkeypatch):
    from test_binding_cpu import A, StandIn
    stand_in = StandIn(returns={"par_tileset_extend_work_bytes": 777}, writes={"par_tileset_extend_host": {11: 5, 13: 3}})
    monkeypatch.setattr(par, "lib", lambda: stand_in)
    P = T.default_params(140, 40)
    assert ext.tileset_extend_work_bytes(90, 12) == 777
    assert stand_in.calls.pop() == ("par_tileset_extend_work_bytes", [90, 12])
    ext.tileset_extend(P, 0x1000, (16, 32), (8, 16), 0x2000, 0x4000, 9, 0x3000, map_out=0x5000, first_new_out=0x7000, pad=7,
                       flips=2, stream=0x6000)
    assert stand_in.calls.pop() == ("par_tileset_extend_device", [A(P), 0x6000, 0x1000, 16, 32, 8, 16, 7, 2, 0x2000, 0x4000, 9,
                                                                  0x3000, 0x5000, 0x7000])
    ext.tileset_extend(P, 0x1000, (0, 40), (16, 8), 0x2000, None, 0, 0x3000)
    assert stand_in.calls.pop() == ("par_tileset_extend_device", [A(P), None, 0x1000, 0, 40, 16, 8, 0, 0, 0x2000, None, 0, 0x3000,
                                                                  None, None])
    plane = np.zeros(16 * 140, dtype=np.uint8)
    stored = np.arange(3 * 128, dtype=np.uint8).reshape(3, 16, 8)
    out = ext.tileset_extend_host(P, plane, (8, 16), stored, 3, 9, rows=(16, 32), pad=7, flips=2, device=2)
    assert list(out) == ["tiles", "map", "count", "first_new"] and out["count"] == 5 and out["first_new"] == 3
    assert out["tiles"].shape == (5, 16, 8) and out["map"].shape == (18,) and out["map"].dtype == np.uint32
    assert out["tiles"][:3].tobytes() == stored.tobytes(), "the stored tiles are handed to the library"
    name, args = stand_in.calls.pop()
    assert name == "par_tileset_extend_host"
    assert args[:9] == [A(P), 2, A(plane), 16, 32, 8, 16, 7, 2] and args[9] == A(out["tiles"].base) and args[10] == 9
    assert args[12] == A(out["map"])
    out = ext.tileset_extend_host(P, np.zeros(40 * 140, dtype=np.uint8), (16, 16), np.zeros((0, 16, 16), np.uint8), 0, 0)
    name, args = stand_in.calls.pop()
    assert args[9] is None and args[10] == 0 and args[1] == -1 and args[3:5] == [0, 40] and out["tiles"].shape == (0, 16, 16)
    stand_in.status = 6
    with pytest.raises(par.ParError) as e:
        ext.tileset_extend(P, 0x1000, (0, 40), (16, 8), 0x2000, None, 0, 0x3000)
    assert e.value.status == 6 and str(e.value) == "PAR_ERR_EXTENT: par_tileset_extend_device"


# ---- the model the GPU tests compare with --------------------------------------------------------------------------

def same(a, b, tag):
    for name, x, y in zip(("tiles", "map"), a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"{tag}: {name}"
    assert a[2:] == b[2:], f"{tag}: T_out, first_new"


@pytest.mark.parametrize("tile", TS.TILES)
def test_model_equals_the_loop_on_random_sequences(tile):
    reused = added = mirrored = 0
    for w, h in ((21, 19), (37, 23)):
        frames = TX.frame_sequence(1000 * w + tile[0] + 2 * tile[1], 3, w, h, tile, kinds=3, step=2)
        n = TS.grid(w, h, tile)[0] * TS.grid(w, h, tile)[1]
        for flips in range(4):
            for pad in (0, 255):
                for capacity in (3 * n, n // 2, 1, 0):
                    a, end_a = TX.sequence_model(frames, w, h, tile, pad, flips, capacity)
                    b, end_b = TX.sequence_model(frames, w, h, tile, pad, flips, capacity, fn=TX.model_loop)
                    for k, (x, y) in enumerate(zip(a, b)):
                        same(x, y, f"{w}x{h} {tile} flips {flips} pad {pad} capacity {capacity} call {k}")
                        assert len(x[1]) == n and x[0].shape == (min(x[2], capacity), tile[1], tile[0])
                        assert ((x[1] >> 30) & ~np.uint32(flips) == 0).all(), "only allowed codes"
                        mirrored += int((x[1] >> 30).any())
                        if k and capacity == 3 * n:
                            reused += int(((x[1] & TS.ID_MASK) < x[3]).any())
                            added += x[2] > x[3]
                    assert end_a[1] == end_b[1] and end_a[0].tobytes() == end_b[0].tobytes()
    assert reused >= 12 and added >= 8 and mirrored > 30, (reused, added, mirrored)


def cell_plane(cells, gcx, tile):
    n = len(cells)
    return np.ascontiguousarray(np.asarray(cells, np.uint8).reshape(n // gcx, gcx, tile[1], tile[0]).transpose(0, 2, 1, 3)).reshape(-1)


def entries(*pairs):
    return np.array([i | (f << 30) for i, f in pairs], dtype=np.uint32)


def crafted():
    """name -> (stored, t_in, plane, w, rows, flips, capacity, (tiles after, map, T_out)), tiles of 8 x 8, pad 0, worked
    out by hand. t has 1, 2 right of it and 3 below it in its top left corner: its xy mirror is its smallest image, then
    y, then x, then t (tests/test_tileset_cpu.py). `five` is a tile of one colour."""
    tile = (8, 8)
    t = np.zeros((8, 8), np.uint8)
    t[0, 0], t[0, 1], t[1, 0] = 1, 2, 3
    tx, ty, txy = t[:, ::-1], t[::-1], t[::-1, ::-1]
    five, six = np.full((8, 8), 5, np.uint8), np.full((8, 8), 6, np.uint8)
    out = {}
    # cells: five, txy, six, five. Stored: six, five, six, five: five is tile 1 (not 3), six is tile 0 (not 2), txy is new
    plane = cell_plane([five, txy, six, five], 4, tile)
    out["a stored duplicate"] = (np.stack([six, five, six, five]), 4, plane, 32, 8, 0, 8,
                                 (np.stack([six, five, six, five, txy]), entries((1, 0), (4, 0), (0, 0), (1, 0)), 5))
    # t is stored as it is. Under flips 3 the cell t has the canonical form txy under code 3: the stored t is not matched
    # although the cell equals it bytewise, and a new tile txy is made; the cell five matches tile 1.
    plane = cell_plane([t, five], 2, tile)
    out["a stored non-canonical tile under flips 3"] = (np.stack([t, five]), 2, plane, 16, 8, 3, 8,
                                                        (np.stack([t, five, txy]), entries((2, 3), (1, 0)), 3))
    # the same set without flips: the cell t is the stored tile 0
    out["the same set without flips"] = (np.stack([t, five]), 2, plane, 16, 8, 0, 8,
                                         (np.stack([t, five]), entries((0, 0), (1, 0)), 2))
    # the cell's mirror is stored: txy is stored, the cells t, tx, ty are it under codes 3, 2, 1; with x alone, t and tx
    # have the form tx and ty has txy: tx is new (under codes 1 and 0), ty is tile 0 under code 1
    plane = cell_plane([t, tx, ty], 3, tile)
    out["a cell whose mirror is stored"] = (txy[None], 1, plane, 24, 8, 3, 8, (txy[None], entries((0, 3), (0, 2), (0, 1)), 1))
    out["a cell whose mirror is stored, x alone"] = (txy[None], 1, plane, 24, 8, 1, 8,
                                                     (np.stack([txy, tx]), entries((1, 1), (1, 0), (0, 1)), 2))
    # T_in above the capacity: 2 tiles are stored of a count of 7. five matches tile 1; t and six are new tiles 7 and 8,
    # none is written; the second t is the same new tile within the call
    plane = cell_plane([t, five, six, t], 4, tile)
    out["T_in above capacity"] = (np.stack([six * 0, five]), 7, plane, 32, 8, 0, 2,
                                  (np.stack([six * 0, five]), entries((7, 0), (1, 0), (8, 0), (7, 0)), 9))
    # capacity crossed mid-call: one tile stored of capacity 2: t is new tile 1 and is written, six is new tile 2 and is not
    out["capacity crossed mid-call"] = (five[None], 1, plane, 32, 8, 0, 2,
                                        (np.stack([five, t]), entries((1, 0), (0, 0), (2, 0), (1, 0)), 3))
    # capacity 0: nothing stored, nothing matches: the plane's own T (3) is added to the count
    out["capacity 0"] = (TX.no_tiles(tile), 40, plane, 32, 8, 0, 0, (TX.no_tiles(tile), entries((40, 0), (41, 0), (42, 0), (40, 0)), 43))
    return out


CRAFTED = ["a stored duplicate", "a stored non-canonical tile under flips 3", "the same set without flips",
           "a cell whose mirror is stored", "a cell whose mirror is stored, x alone", "T_in above capacity",
           "capacity crossed mid-call", "capacity 0"]


@pytest.mark.parametrize("name", CRAFTED)
def test_crafted_sets(name):
    cases = crafted()
    assert sorted(cases) == sorted(CRAFTED)
    stored, t_in, plane, w, rows, flips, capacity, (tiles, tile_map, t_out) = cases[name]
    got = TX.model(stored, t_in, plane, w, rows, (8, 8), 0, flips, capacity)
    same(got, TX.model_loop(stored, t_in, plane, w, rows, (8, 8), 0, flips, capacity), name)
    assert got[2] == t_out and got[3] == t_in and np.array_equal(got[1], tile_map), (name, got[1], tile_map)
    assert got[0].tobytes() == np.ascontiguousarray(tiles).tobytes(), name


# ---- the consequences ----------------------------------------------------------------------------------------------

def test_1_from_count_0_it_is_a_build():
    rng = np.random.default_rng(3)
    for tile in TS.TILES:
        plane = TS.mixed_plane(rng, 61, 23, tile, 6, colours=3)
        for flips in range(4):
            for capacity in (100, 3, 0):
                got = TX.model(TX.no_tiles(tile), 0, plane, 61, 23, tile, 4, flips, capacity)
                same(got[:3], TS.model(plane, 61, 23, tile, 4, flips, capacity), f"{tile} flips {flips}")
                same(got[:3], TS.model_loop(plane, 61, 23, tile, 4, flips, capacity), f"{tile} flips {flips}, the loop")


def test_2_3_4_a_sequence_is_one_loop_row_blocks_and_stacked_frames():
    tile, w = (8, 8), 37
    first, second = TX.frame_sequence(4, 2, w, 40, tile, kinds=5, step=4)
    second = second[:23 * w]
    stacked = np.concatenate([first, second])
    whole = TS.model_loop(stacked, w, 63, tile, 2, 3)
    calls, (tiles, count) = TX.sequence_model([first, second], w, [40, 23], tile, 2, 3, 200)
    assert count == whole[2] and tiles.tobytes() == whole[0].tobytes(), "4: the first stacked on the second"
    assert np.array_equal(np.concatenate([c[1] for c in calls]), whole[1])
    # 3: row blocks in ascending order
    frame = TS.model(first, w, 40, tile, 2, 3)
    blocks = [(0, 16), (16, 32), (32, 40)]
    assert all(TS.admits(r0, r1, 40, tile) for r0, r1 in blocks)
    calls, (tiles, count) = TX.sequence_model([first[r0 * w:r1 * w] for r0, r1 in blocks], w, [r1 - r0 for r0, r1 in blocks], tile,
                                              2, 3, 200)
    assert count == frame[2] and tiles.tobytes() == frame[0].tobytes()
    assert np.array_equal(np.concatenate([c[1] for c in calls]), frame[1]), "the concatenated maps are the frame's map"
    assert [c[3] for c in calls] == [0, calls[0][2], calls[1][2]]


def test_5_6_the_same_plane_again_adds_nothing_and_a_set_is_a_plane():
    tile, w, h = (16, 8), 131, 67
    a_plane, b_plane = TX.frame_sequence(6, 2, w, h, tile, kinds=7, step=6)
    for flips in (0, 3):
        a, b = TS.model(a_plane, w, h, tile, 0, flips), TS.model(b_plane, w, h, tile, 0, flips)
        merged = TX.model(a[0], a[2], b[0].reshape(-1), tile[0], b[2] * tile[1], tile, 0, flips, 1000)
        assert not (merged[1] >> 30).any(), "B is canonical under the same flips: every code is 0"
        assert a[2] < merged[2] < a[2] + b[2], "the sets share tiles and B adds some"
        # map_out is B's renumbering: B's map through it is the map of b_plane into the merged set
        direct = TX.model(a[0], a[2], b_plane, w, h, tile, 0, flips, 1000)
        assert np.array_equal(merged[1][b[1] & TS.ID_MASK] & TS.ID_MASK, direct[1] & TS.ID_MASK)
        assert direct[2] == merged[2] and direct[0].tobytes() == merged[0].tobytes()
        again = TX.model(merged[0], merged[2], b[0].reshape(-1), tile[0], b[2] * tile[1], tile, 0, flips, 1000)
        assert again[2] == merged[2] and again[0].tobytes() == merged[0].tobytes() and np.array_equal(again[1], merged[1])


def test_7_8_overflow_counts_again_and_caller_made_sets():
    tile, w, h = (8, 8), 67, 40
    frames = TX.frame_sequence(7, 2, w, h, tile, kinds=8, step=0, colours=3)
    complete, _ = TX.sequence_model([frames[0], frames[0]], w, h, tile, 0, 3, 100)
    assert complete[1][2] == complete[0][2] <= 100
    capacity = complete[0][2] - 3
    short, _ = TX.sequence_model([frames[0], frames[0]], w, h, tile, 0, 3, capacity)
    assert short[0][2] == complete[0][2] > capacity, "the first call's count is exact"
    assert short[1][2] == short[0][2] + 3, "the three tiles that were not stored count again: an upper bound"
    # 8: the crafted cases hold the rest; here, a stored tile that is no cell's canonical form is never matched
    t = np.zeros((8, 8), np.uint8)
    t[0, 0], t[0, 1], t[1, 0] = 1, 2, 3
    got = TX.model(t[None], 1, t.reshape(-1), 8, 8, tile, 0, 3, 4)
    assert got[2] == 2 and got[1][0] == 1 | (3 << 30)


# ---- the host form's copy arithmetic ---------------------------------------------------------------------------------

def test_extend_spans_under_a_sanitiser(tmp_path):
    """tests/tileset_extend_spans_check.cpp with csrc/par_hostcall.h alone (no HIP), address and undefined-behaviour
    sanitisers on, as a child process."""
    exe = tmp_path / "tileset_extend_spans_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "pixel-art-raytracer_amd", "csrc"),
           os.path.join(ROOT, "tests", "tileset_extend_spans_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "warning" not in p.stderr, p.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith(" checks, 0 failures"), out.stdout[-2000:]
    assert int(out.stdout.strip().splitlines()[-1].split()[0]) >= 2000
