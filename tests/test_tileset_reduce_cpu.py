"""Tile budgets without a GPU: the three calls are declared in addons/include/par_tileset_reduce.h, an add-on header that
includes no header of the project, exported by a library of their own and wrapped by the tileset_reduce module, whose
table is none of abi.py's and which the package does not import; the header compiles as pedantic C11 alone, twice and
beside the four core headers; every PAR_ERR_INVALID_ARG of both calls comes back before any device work and with nothing
written, each rule on its own; par_tileset_reduce_work_bytes is the header's formula; the binding hands its arguments over
in the header's order; the vectorised model the GPU tests lean on (tileset_reduce.model) equals a loop in Python integers
on random sets and on crafted sets worked out by hand; the consequences the contract states hold; and the figures of the
graybox frame that README and DESIGN quote are the model's."""
import ctypes as C
import importlib
import inspect
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import headers
import tileset as TS
import tileset_reduce as TR

ROOT = headers.ROOT
ADDON_INCLUDE = os.path.join(ROOT, "addons", "include")
HEADER = os.path.join(ADDON_INCLUDE, "par_tileset_reduce.h")
ERR_INVALID_ARG, ERR_NO_DEVICE = 1, 2
SYMBOLS = ("par_tileset_reduce_work_bytes", "par_tileset_reduce_device", "par_tileset_reduce_host")


RED = importlib.import_module("pixel-art-raytracer_amd.tileset_reduce")  # (without the add-on's binding nothing here can run)


@pytest.fixture(scope="module")
def red():
    return RED


def header_text():
    return open(HEADER).read()


def header_code():
    return re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)


def header_prototypes():
    return re.findall(r"^(%s)\s+(par_[a-z_0-9]+)\(([^;]*?)\);" % "|".join(re.escape(r) for r in headers.RETURNS), header_code(),
                      flags=re.M | re.S)


# ---- declared, exported, bound -------------------------------------------------------------------------------------

def test_the_prototypes_are_the_contracts():
    code = " ".join(header_code().split())
    for proto in (
            "size_t par_tileset_reduce_work_bytes(int n_cells, int capacity);",
            "int par_tileset_reduce_device(void* stream, const uint8_t* tiles, int capacity, const uint32_t* count, int tile_w, "
            "int tile_h, int flips, const uint32_t* map, int n_cells, const uint8_t* palette, int n_colors, int budget, "
            "void* work, uint8_t* tiles_out, uint32_t* map_out, uint32_t* remap_out, uint32_t* count_out, uint64_t* error_out);",
            "int par_tileset_reduce_host(int device, const uint8_t* tiles, int n_tiles, int tile_w, int tile_h, int flips, "
            "const uint32_t* map, int n_cells, const uint8_t* palette, int n_colors, int budget, uint8_t* tiles_out, "
            "uint32_t* map_out, uint32_t* remap_out, int* count_out, uint64_t* error_out);"):
        assert proto in code, proto
    assert tuple(name for _, name, _ in header_prototypes()) == SYMBOLS
    assert re.findall(r"#include\s+([<\"][^>\"]+[>\"])", header_code()) == ["<stddef.h>", "<stdint.h>"]
    for define, value in (("PAR_TILESET_REDUCE_MAX_TILES", "4096"), ("PAR_TILESET_REDUCE_MAX_BUDGET", "1024")):
        assert re.search(r"#define %s %s\b" % (define, value), code), define
    text = " ".join(header_text().replace("\n *", " ").split())  # the comment as running text
    for word in ("k-medoid", "gglomerative", "per sub-palette", "without one map", "otations", "budget + 6 launches",
                 "4096 + 20 * capacity", "lowest number among equals", "compose by XOR"):
        assert word in text, word


def test_the_table_is_the_headers_and_no_core_table(par, red):
    protos = header_prototypes()
    assert SYMBOLS == tuple(red.ABI_TILESET_REDUCE) == red.ABI_TILESET_REDUCE_SYMBOLS
    L = red.lib()
    for proto in protos:
        ret, name, _ = proto
        want_restype, want = headers.want_signature(proto)
        restype, argtypes = headers.signature(red.ABI_TILESET_REDUCE[name])
        assert list(argtypes) == want and restype is want_restype, name
        fn = getattr(L, name)
        assert list(fn.argtypes) == want and fn.restype is want_restype, name
    assert not any(table is red.ABI_TILESET_REDUCE for table in par.ABI_HEADERS.values())
    for name in SYMBOLS:
        assert not any(name in table for table in (*par.ABI_HEADERS.values(), par.ABI_DEBUG_HOOKS)), name
        assert not hasattr(par.lib(), name), f"{name} is exported by the core library"
    for h in os.listdir(headers.INCLUDE):
        assert "par_tileset_reduce_" not in headers.without_comments(h), h
    for fn in ("tileset_reduce_work_bytes", "tileset_reduce", "tileset_reduce_host"):
        # (once imported, the package has the submodule under the name of its wrapper tileset_reduce: a module, no wrapper)
        assert callable(getattr(red, fn)) and (not hasattr(par, fn) or inspect.ismodule(getattr(par, fn))), fn
    # one sentence in each tile-set header: the lossy merge exists, in the add-on
    for h in ("par_tileset.h", "par_tileset_extend.h"):
        assert "par_tileset_reduce.h" in headers.text(h), h


def test_the_add_on_exports_exactly_its_table(red):
    nm = shutil.which("nm")
    assert nm is not None, "no nm to list the library's symbols"
    out = subprocess.run([nm, "-D", "--defined-only", red.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(f[2] for f in (line.split() for line in out.splitlines()) if len(f) == 3 and f[1] == "T" and f[2].startswith("par_"))
    assert exported == sorted(SYMBOLS)


def test_importing_the_package_does_not_load_the_module():
    code = ("import importlib, json, sys\npar = importlib.import_module('pixel-art-raytracer_amd')\npar.lib()\n"
            "print(json.dumps(sorted(m for m in sys.modules if m.startswith('pixel-art-raytracer_amd.'))))\n"
            "red = importlib.import_module('pixel-art-raytracer_amd.tileset_reduce')\n"
            "print(json.dumps([red.tileset_reduce_work_bytes(7, 9), red.lib() is not par.lib()]))")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().splitlines()
    assert json.loads(lines[-2]) == ["pixel-art-raytracer_amd.abi", "pixel-art-raytracer_amd.types"]
    assert json.loads(lines[-1]) == [4096 + 20 * 9, True]


BODY = r"""
#include <stdio.h>
int main(void) {
    unsigned char tiles[128] = {0}, out[64] = {0}, palette[4] = {0};
    uint32_t map[3] = {0, 1, 1}, map_out[3] = {7, 7, 7}, count = 2, count_out = 9;
    uint64_t work[1 + (4096 + 40) / 8];
    int rc = par_tileset_reduce_device(NULL, tiles, 2, &count, 8, 8, 4, map, 3, palette, 1, 1, work, out, map_out, NULL,
                                       &count_out, NULL);
    printf("%d %d %u %lu %lu\n", PAR_TILESET_REDUCE_MAX_TILES + PAR_TILESET_REDUCE_MAX_BUDGET, rc, (unsigned)count_out,
           (unsigned long)par_tileset_reduce_work_bytes(3, 2), (unsigned long)par_tileset_reduce_work_bytes(3, 4097));
    return 0;
}
"""
CORE = ["par_raytracer.h", "par_cells.h", "par_tileset.h", "par_tileset_extend.h"]


@pytest.mark.parametrize("includes", [["par_tileset_reduce.h"], ["par_tileset_reduce.h"] * 2, CORE + ["par_tileset_reduce.h"],
                                      ["par_tileset_reduce.h"] + CORE], ids=["alone", "twice", "behind the core", "before the core"])
def test_header_is_pedantic_c11(tmp_path, includes):
    src, exe = tmp_path / "reduce.c", tmp_path / "reduce"
    src.write_text("".join(f'#include "{h}"\n' for h in includes) + BODY)
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", ADDON_INCLUDE, "-I", headers.INCLUDE,
                        str(src), "-o", str(exe), "-L", headers.LIB_DIR, "-lpar_tileset_reduce", f"-Wl,-rpath,{headers.LIB_DIR}"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["5120", "1", "9", str(4096 + 40), "0"], (out.stdout, out.stderr)


# ---- par_tileset_reduce_work_bytes -------------------------------------------------------------------------------------

def test_work_bytes_is_the_headers_formula_and_keeps_its_bound(red):
    for n in (1, 2, 600, 2400, (1 << 20) - 1, 1 << 20):
        for cap in (1, 2, 31, 32, 33, 519, 4095, 4096):
            got = red.tileset_reduce_work_bytes(n, cap)
            assert got == 4096 + 20 * cap, (n, cap)
            assert got <= 4096 + 20 * (n + cap), "O(n_cells + capacity)"
    assert red.tileset_reduce_work_bytes(1 << 20, 4096) == 4096 + 20 * 4096 < 4096 * 4096, "no T x T matrix"
    for n, cap in ((0, 4), (-1, 4), ((1 << 20) + 1, 4), ((1 << 31) - 1, 1), (4, 0), (4, -1), (4, 4097), (4, (1 << 31) - 1),
                   (-(1 << 31), -(1 << 31))):
        assert red.tileset_reduce_work_bytes(n, cap) == 0, (n, cap)
    assert red.lib().par_tileset_reduce_work_bytes.restype is C.c_size_t


# ---- argument errors: no device needed, nothing written -----------------------------------------------------------

BAD = [
    ("null tiles", dict(tiles=None)),
    ("null map", dict(map=None)),
    ("null palette", dict(palette=None)),
    ("null tiles_out", dict(tiles_out=None)),
    ("null map_out", dict(map_out=None)),
    ("null count_out", dict(count_out=None)),
    ("tiles_out is tiles", dict(overlap=0)),
    ("tiles_out begins inside tiles", dict(overlap=5 * 64 - 1)),
    ("tiles_out ends inside tiles", dict(overlap=-(3 * 64 - 1))),
    ("n_tiles 0", dict(n_tiles=0)),
    ("n_tiles -1", dict(n_tiles=-1)),
    ("n_tiles 4097", dict(n_tiles=4097)),
    ("n_tiles 2^31 - 1", dict(n_tiles=(1 << 31) - 1)),
    ("budget 0", dict(budget=0)),
    ("budget -1", dict(budget=-1)),
    ("budget 1025", dict(budget=1025)),
    ("n_cells 0", dict(n_cells=0)),
    ("n_cells -1", dict(n_cells=-1)),
    ("n_cells 2^20 + 1", dict(n_cells=(1 << 20) + 1)),
    ("n_colors 0", dict(n_colors=0)),
    ("n_colors -1", dict(n_colors=-1)),
    ("n_colors 257", dict(n_colors=257)),
    ("tile_w 4", dict(tile=(4, 8))),
    ("tile_w 12", dict(tile=(12, 8))),
    ("tile_w 32", dict(tile=(32, 8))),
    ("tile_w 0", dict(tile=(0, 8))),
    ("tile_h 4", dict(tile=(8, 4))),
    ("tile_h 32", dict(tile=(8, 32))),
    ("tile_h 0", dict(tile=(8, 0))),
    ("tile_h negative", dict(tile=(8, -8))),
    ("flips -1", dict(flips=-1)),
    ("flips 4", dict(flips=4)),
]
BAD_DEVICE = BAD + [("null count", dict(count=None)), ("null work", dict(work=None)), ("work off its 8 bytes", dict(work_shift=4))]


def raw_call(red, T, which, over):
    """One call of the raw symbol on host dummies: (status, whether any buffer changed). The set has 5 tiles of 8 x 8, the
    map 12 entries, the budget is 3."""
    L = red.lib()
    bufs = {"tiles": np.full(16 * 64, 0xA5, np.uint8), "map": np.full(12, 0x3C3C3C3C, np.uint32), "palette": np.full(4 * 6, 0x77, np.uint8),
            "tiles_out": np.full(16 * 64, 0xC3, np.uint8), "map_out": np.full(12, 0x69696969, np.uint32),
            "remap_out": np.full(16, 0x11111111, np.uint32), "count": np.full(2, 5, np.uint32), "count_out": np.full(2, 0x5A5A5A5A, np.uint32),
            "error_out": np.full(2, 0x4B, np.uint64), "work": np.full((4096 + 20 * 16) // 8 + 2, 0x5A, np.uint64)}
    before = {k: v.copy() for k, v in bufs.items()}
    arg = dict(tile=(8, 8), flips=3, n_tiles=5, n_cells=12, n_colors=6, budget=3, **bufs)
    arg.update({k: v for k, v in over.items() if k not in ("work_shift", "overlap")})
    ptr = T.ptr
    work = ptr(arg["work"])
    if "work_shift" in over:
        work = C.c_void_p(arg["work"].ctypes.data + over["work_shift"])
    tiles_out = ptr(arg["tiles_out"])
    if "overlap" in over:  # tiles holds tiles 8 .. 12 of its buffer, tiles_out three tiles `overlap` bytes past them
        tiles_at = arg["tiles"].ctypes.data + 8 * 64
        tiles, tiles_out = C.c_void_p(tiles_at), C.c_void_p(tiles_at + over["overlap"])
    else:
        tiles = ptr(arg["tiles"])
    (tw, th) = arg["tile"]
    if which == "device":
        rc = L.par_tileset_reduce_device(None, tiles, arg["n_tiles"], ptr(arg["count"]), tw, th, arg["flips"], ptr(arg["map"]),
                                         arg["n_cells"], ptr(arg["palette"]), arg["n_colors"], arg["budget"], work, tiles_out,
                                         ptr(arg["map_out"]), ptr(arg["remap_out"]), ptr(arg["count_out"]), ptr(arg["error_out"]))
    else:
        rc = L.par_tileset_reduce_host(-1, tiles, arg["n_tiles"], tw, th, arg["flips"], ptr(arg["map"]), arg["n_cells"],
                                       ptr(arg["palette"]), arg["n_colors"], arg["budget"], tiles_out, ptr(arg["map_out"]),
                                       ptr(arg["remap_out"]), ptr(arg["count_out"]), ptr(arg["error_out"]))
    return rc, any(bufs[k].tobytes() != before[k].tobytes() for k in bufs)


@pytest.mark.parametrize("which,bad", [("device", BAD_DEVICE), ("host", BAD)])
def test_invalid_arguments_need_no_device_and_write_nothing(red, T, which, bad):
    assert len({tag for tag, _ in bad}) == len(bad)
    for tag, over in bad:
        rc, changed = raw_call(red, T, which, over)
        assert rc == ERR_INVALID_ARG, f"{which}: {tag}: status {rc}"
        assert not changed, f"{which}: {tag}: something was written"


def test_what_the_rules_admit_is_not_refused(par, red, T):
    """The host form on the arguments next to the refused ones (the device form would take host dummies for device
    memory): any status but PAR_ERR_INVALID_ARG, which without a GPU is PAR_ERR_NO_DEVICE."""
    want = 0 if par.device_count() > 0 else ERR_NO_DEVICE
    for over in (dict(), dict(remap_out=None), dict(error_out=None), dict(remap_out=None, error_out=None), dict(flips=0),
                 dict(tile=(16, 8), n_tiles=2), dict(tile=(8, 16), n_tiles=2), dict(tile=(16, 16), n_tiles=4, budget=4),
                 dict(n_tiles=1), dict(n_tiles=16), dict(budget=1), dict(budget=16), dict(n_cells=1), dict(n_colors=1),
                 dict(overlap=5 * 64), dict(overlap=-3 * 64)):
        rc, _ = raw_call(red, T, "host", over)
        assert rc == want, (over, rc)


def test_binding_raises_and_checks_its_arrays(par, red):
    with pytest.raises(par.ParError) as e:
        red.tileset_reduce(0x1000, 4, 0x2000, (8, 8), 0x3000, 9, 0x4000, 3, 2, 0x5000, 0x1000, 0x6000, 0x7000)
    assert e.value.status == ERR_INVALID_ARG and str(e.value) == "PAR_ERR_INVALID_ARG: par_tileset_reduce_device"
    with pytest.raises(par.ParError) as e:
        red.tileset_reduce_host(np.zeros((2, 8, 8), np.uint8), (8, 8), np.zeros(4, np.uint32), np.zeros((2, 4), np.uint8), 0)
    assert e.value.status == ERR_INVALID_ARG and str(e.value) == "PAR_ERR_INVALID_ARG: par_tileset_reduce_host"
    with pytest.raises(ValueError, match="tileset_reduce_host: tiles holds"):
        red.tileset_reduce_host(np.zeros(65, np.uint8), (8, 8), np.zeros(4, np.uint32), np.zeros((2, 4), np.uint8), 1)
    with pytest.raises(ValueError, match="tileset_reduce_host: palette holds"):
        red.tileset_reduce_host(np.zeros(64, np.uint8), (8, 8), np.zeros(4, np.uint32), np.zeros(7, np.uint8), 1)
    for bad in ("s", 1.5, np.int64(0x1000)):
        with pytest.raises(TypeError):
            red.tileset_reduce(bad, 4, 0x2000, (8, 8), 0x3000, 9, 0x4000, 3, 2, 0x5000, 0x8000, 0x6000, 0x7000)
        with pytest.raises(TypeError):
            red.tileset_reduce(0x1000, 4, 0x2000, (8, 8), 0x3000, 9, 0x4000, 3, 2, 0x5000, 0x8000, 0x6000, 0x7000, stream=bad)


def test_arguments_reach_the_library_in_the_headers_order(par, red, monkeypatch):
    from test_binding_cpu import A, StandIn
    stand_in = StandIn(returns={"par_tileset_reduce_work_bytes": 777}, writes={"par_tileset_reduce_host": {14: 2, 15: 99}})
    monkeypatch.setattr(red, "lib", lambda: stand_in)
    assert red.tileset_reduce_work_bytes(90, 12) == 777
    assert stand_in.calls.pop() == ("par_tileset_reduce_work_bytes", [90, 12])
    red.tileset_reduce(0x1000, 40, 0x2000, (8, 16), 0x3000, 77, 0x4000, 33, 25, 0x5000, 0x6000, 0x7000, 0x8000, remap_out=0x9000,
                       error_out=0xA000, flips=2, stream=0xB000)
    assert stand_in.calls.pop() == ("par_tileset_reduce_device", [0xB000, 0x1000, 40, 0x2000, 8, 16, 2, 0x3000, 77, 0x4000, 33, 25,
                                                                  0x5000, 0x6000, 0x7000, 0x9000, 0x8000, 0xA000])
    red.tileset_reduce(0x1000, 40, 0x2000, (16, 8), 0x3000, 77, 0x4000, 33, 25, 0x5000, 0x6000, 0x3000, 0x8000)
    assert stand_in.calls.pop() == ("par_tileset_reduce_device", [None, 0x1000, 40, 0x2000, 16, 8, 0, 0x3000, 77, 0x4000, 33, 25,
                                                                  0x5000, 0x6000, 0x3000, None, 0x8000, None])
    tiles = np.arange(3 * 128, dtype=np.uint8).reshape(3, 16, 8)
    tile_map = np.arange(5, dtype=np.uint32)
    palette = np.arange(28, dtype=np.uint8).reshape(7, 4)
    out = red.tileset_reduce_host(tiles, (8, 16), tile_map, palette, 4, flips=1, device=2)
    assert list(out) == ["tiles", "map", "remap", "count", "error"] and out["count"] == 2 and out["error"] == 99
    assert out["tiles"].shape == (2, 16, 8) and out["map"].shape == (5,) and out["remap"].shape == (3,)
    name, args = stand_in.calls.pop()
    assert name == "par_tileset_reduce_host"
    assert args[:6] == [2, A(tiles), 3, 8, 16, 1] and args[7:11] == [5, A(palette), 7, 4]
    assert args[11] == A(out["tiles"].base) and args[12] == A(out["map"]) and args[13] == A(out["remap"])
    red.tileset_reduce_host(tiles, (8, 16), tile_map, palette, 4)
    assert stand_in.calls.pop()[1][0] == -1
    stand_in.status = 4
    with pytest.raises(par.ParError) as e:
        red.tileset_reduce_host(tiles, (8, 16), tile_map, palette, 4)
    assert e.value.status == 4 and str(e.value) == "PAR_ERR_OOM: par_tileset_reduce_host"


# ---- the model the GPU tests compare with --------------------------------------------------------------------------

@pytest.mark.parametrize("tile", TS.TILES)
def test_model_equals_the_loop_on_random_sets(tile):
    rng = np.random.default_rng(100 + tile[0] + 2 * tile[1])
    mirrored = dropped = 0
    for flips in range(4):
        for t, budget in ((1, 1), (5, 2), (9, 4), (12, 11), (12, 12), (7, 9), (10, 1)):
            tiles, tile_map = TR.random_set(rng, t, tile, 3, 40, kinds=2, spare=2)
            palette = TR.random_palette(rng, 4)
            for count in (t, t + 5):
                a = TR.model(tiles, count, tile_map, palette, budget, flips)
                TR.same(a, TR.model_loop(tiles, count, tile_map, palette, budget, flips), f"{tile} flips {flips} T {t} K {budget}")
                assert ((a[2] >> 30) & ~np.uint32(flips) == 0).all() and ((a[1] >> 30) & ~np.uint32(flips | 3) == 0).all()
                assert a[3] == min(count, t + 2, budget) and len(a[2]) == min(count, t + 2)
                mirrored += int((a[2] >> 30).any())
                dropped += len(a[2]) - a[3]
    assert mirrored >= 6 and dropped > 100, (mirrored, dropped)


@pytest.mark.parametrize("name", TR.CRAFTED)
def test_crafted_sets(name):
    cases = TR.crafted()
    assert sorted(cases) == sorted(TR.CRAFTED)
    (tiles, count, tile_map, budget, flips), want = cases[name]
    got = TR.model(tiles, count, tile_map, TR.CRAFTED_PALETTE, budget, flips)
    TR.same(got, TR.model_loop(tiles, count, tile_map, TR.CRAFTED_PALETTE, budget, flips), name)
    want = (np.ascontiguousarray(want[0]), *want[1:])
    TR.same(got, want, name)


# ---- the consequences ----------------------------------------------------------------------------------------------

def plane_set(rng, w, h, tile, flips, kinds=9, colours=3):
    """A plane of whole cells with a few pixels changed, its set and map."""
    plane = TS.mixed_plane(rng, w, h, tile, kinds, colours=colours)
    at = rng.integers(0, len(plane), len(plane) // 50)
    plane[at] = rng.integers(0, colours, len(at))
    return (plane, *TS.model(plane, w, h, tile, 0, flips))


def test_1_2_a_budget_that_holds_is_the_identity_and_one_keeps_the_most_used():
    rng = np.random.default_rng(41)
    palette = TR.random_palette(rng, 5)
    for tile in TS.TILES:
        for flips in (0, 3):
            plane, tiles, tile_map, t = plane_set(rng, 96, 64, tile, flips)
            wild = tile_map.copy()
            wild[::7] |= np.uint32(0x3FFFFF00)  # ids beyond T read as T - 1
            for budget in (t, t + 1, 1024):
                got = TR.model(tiles, t, wild, palette, budget, flips)
                assert got[3] == t and got[4] == 0 and got[0].tobytes() == tiles.tobytes() and np.array_equal(got[2], np.arange(t))
                assert np.array_equal(got[1] >> 30, wild >> 30), "the map keeps its flips"
                assert np.array_equal(got[1] & TS.ID_MASK, np.minimum(wild & TS.ID_MASK, t - 1)), "and has clamped ids"
            one = TR.model(tiles, t, tile_map, palette, 1, flips)
            u = TR.usage(tile_map, t)
            assert one[3] == 1 and one[0].tobytes() == tiles[int(np.argmax(u))].tobytes() and not (one[1] & TS.ID_MASK).any()


def test_3_4_5_nested_sets_the_error_is_the_pictures_and_a_build_counts_at_most_k():
    rng = np.random.default_rng(42)
    palette = TR.random_palette(rng, 5)
    for tile, flips, w, h in (((8, 8), 3, 96, 64), ((16, 16), 0, 128, 96), ((8, 16), 1, 96, 64), ((16, 8), 2, 96, 64)):
        plane, tiles, tile_map, t = plane_set(rng, w, h, tile, flips, kinds=14)
        original = TR.view(palette, tiles, tile, tile_map, w, h)
        last_error, last_kept = None, None
        for budget in range(1, t + 1, max(1, t // 12)):
            r_tiles, r_map, remap, count, error = TR.model(tiles, t, tile_map, palette, budget, flips)
            # (the tiles of a build differ bytewise: a tile is kept exactly when its new number holds its own bytes)
            kept = {i for i in range(t) if r_tiles[remap[i] & TS.ID_MASK].tobytes() == tiles[i].tobytes() and remap[i] >> 30 == 0}
            assert last_error is None or error <= last_error, "3: the error never rises with K"
            assert last_kept is None or last_kept <= kept, "3: the kept sets are nested"
            last_error, last_kept = error, kept
            reduced = TR.view(palette, r_tiles, tile, r_map, w, h)
            assert int(np.abs(reduced - original).sum()) == error, f"4: {tile} K {budget}"
            drawn = TS.expand_model(r_tiles, tile, r_map, w, h)
            assert TS.model(drawn, w, h, tile, 0, flips)[2] <= budget, "5"
        assert TR.model(tiles, t, tile_map, palette, 1, flips)[4] > 0 == TR.model(tiles, t, tile_map, palette, t, flips)[4], "down to 0 at T"
    # 4 on a ragged frame: the pad pixels of a cell are counted in D and not shown: at most the error
    tile, w, h = (8, 8), 61, 23
    plane = TS.mixed_plane(rng, w, h, tile, 12, colours=3)
    tiles, tile_map, t = TS.model(plane, w, h, tile, 2, 3)
    r_tiles, r_map, _, _, error = TR.model(tiles, t, tile_map, palette, max(1, t // 3), 3)
    seen = int(np.abs(TR.view(palette, r_tiles, tile, r_map, w, h) - TR.view(palette, tiles, tile, tile_map, w, h)).sum())
    assert 0 < seen <= error


def test_6_7_equal_colours_cost_nothing_and_unused_tiles_wait_for_a_tie_at_0():
    rng = np.random.default_rng(43)
    tile, t = (8, 8), 30
    tiles, tile_map = TR.random_set(rng, t, tile, 3, 200)
    fitted = rng.integers(0, 256, (3, 4), dtype=np.uint8)
    # 6: a padded fitted palette (copies of entry 0 behind the fitted entries) changes nothing
    padded = np.concatenate([fitted, np.repeat(fitted[:1], 13, axis=0)])
    for budget in (4, 11):
        TR.same(TR.model(tiles, t, tile_map, padded, budget, 3), TR.model(tiles, t, tile_map, fitted, budget, 3), "a padded palette")
    # 6: every tile once more through the entries 3 .. 5, copies of 0 .. 2: a twin is at D == 0 from its tile, a kept tile's
    # twin has the product 0 and waits, so a budget of half the set leaves no error
    twins = np.concatenate([tiles, tiles + 3])
    doubled = np.concatenate([fitted, fitted])
    both = np.concatenate([tile_map, tile_map + np.uint32(t)])
    got = TR.model(twins, 2 * t, both, doubled, t, 0)
    assert got[3] == t and got[4] == 0
    assert TR.model(twins, 2 * t, both, doubled, 5, 0)[4] > 0
    # 7: the tiles from 20 on are stored and unused. With a budget of the used tiles, every used tile that differs from the
    # kept ones has a product above 0 and goes before any unused tile: no error is left (the crafted sets hold the tie at 0)
    used = tile_map.copy()
    used[(used & TS.ID_MASK) >= 20] = 3
    u = TR.usage(used, t)
    n_used = int((u > 0).sum())
    assert (u[20:] == 0).all() and n_used >= 15
    _, _, _, count, error = TR.model(tiles, t, used, fitted, n_used, 0)
    assert count == n_used and error == 0
    assert TR.model(tiles, t, used, fitted, 3, 0)[4] > 0


# ---- the figures DESIGN and README quote -----------------------------------------------------------------------------

# (tile, flips) -> (T, {K: (the rule's error, the most-used baseline's)})
GRAYBOX = {
    (8, 0): (519, {256: (87741, 316721), 128: (308626, 486546), 64: (633857, 830764)}),
    (8, 3): (402, {256: (26680, 145974), 128: (143915, 361313), 64: (383699, 508084)}),
    (16, 0): (337, {256: (66009, 202409), 128: (643803, 1062049), 64: (1477261, 2080378)}),
    (16, 3): (305, {256: (21082, 77677), 128: (350134, 629264), 64: (868995, 1347320)}),
}


def test_the_graybox_frames_budget_figures(par, oracle, T):
    """The frame of test_tileset_cpu.py::test_the_graybox_frames_tile_counts through its fitted 33-entry palette, reduced
    to 256, 128 and 64 tiles by the rule and by the baseline that keeps the most used tiles: the summed L1 error of the
    reduced picture, recomputed by the model and pinned. The figures at 256 are the ones a scratch model gave when the
    feature was proposed (87 741 / 316 721, 26 680 / 145 974, 66 009 / 202 409, 21 082 / 77 677): the two agree, so the loop
    form had nothing to decide and neither was wrong (the loop holds the model on small sets above). The quantiser itself
    leaves 729 075 on that frame."""
    import palette as P
    import quantize as Q
    from test_gpu_light_range import scene
    from test_gpu_light_tints import COLOUR, TINTS, expected
    sc = scene("graybox", par, oracle, T)
    _, exp, _ = expected(T, sc, [3, 6], [200, 300], TINTS[:2], COLOUR, "graybox, two tinted ranged lights")
    fb = exp["fb"]
    fitted, n_entries, _ = P.fit(T, fb, 33)
    index = Q.model(sc.params, fitted, fb, None, 0)[0]
    palette = np.ascontiguousarray(fitted).view(np.uint8).reshape(-1, 4)
    rgb = palette[:, :3].astype(np.int64)
    shown = np.ascontiguousarray(fb).view(np.uint8).reshape(-1, 4)[:, :3].astype(np.int64)
    assert int(np.abs(shown - rgb[index]).sum()) == 729075
    got = {}
    for (side, flips), (t, by_budget) in GRAYBOX.items():
        tile = (side, side)
        tiles, tile_map, count = TS.model(index, 480, 320, tile, 0, flips)
        assert count == t
        figures = {}
        for budget in by_budget:
            rule = TR.model(tiles, count, tile_map, palette, budget, flips)
            base = TR.most_used(tiles, count, tile_map, palette, budget, flips)
            assert rule[3] == base[3] == budget and rule[4] < base[4]
            for r in (rule, base):
                drawn = TR.view(palette, r[0], tile, r[1], 480, 320)
                assert int(np.abs(drawn - rgb[index]).sum()) == r[4], "the error is the picture's"
            figures[budget] = (rule[4], base[4])
        got[(side, flips)] = (count, figures)
    print(got)
    assert got == GRAYBOX
    tiles, tile_map, count = TS.model(index, 480, 320, (8, 8), 0, 0)
    assert int((TR.usage(tile_map, count) == 1).sum()) == 347, "why keeping the most used tiles is a poor rule here"
