"""The objects add-on without a GPU: the nine calls are declared in addons/include/par_objects.h, an add-on header that
includes no header of the project, exported by a library of their own and wrapped by the objects module, whose table is
none of abi.py's and which the package does not import; the header compiles as pedantic C11 alone, twice and beside the
core and the other add-on headers; the record and the descriptor are the binding's; the enumerations are par_screen.h's
and par_vram.h's; every PAR_ERR_INVALID_ARG comes back before any device work and with nothing written, each rule on its
own; the host arithmetic (work bytes, limits, pack, unpack) is the header's; the vectorised model the GPU tests lean on
(tests/objects.py) equals a loop over objects, pixels and bits in Python integers; crafted tables worked out by hand hold;
and the eight consequences the header states hold on the models, the first over tests/screen.py and tests/vram.py."""
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
import objects as OB
import screen as S
import tileset as TS
import tileset_extend as TX
import vram as V

ROOT = headers.ROOT
ADDON_INCLUDE = os.path.join(ROOT, "addons", "include")
HEADER = os.path.join(ADDON_INCLUDE, "par_objects.h")
ERR_INVALID_ARG, ERR_NO_DEVICE = 1, 2
SYMBOLS = ("par_objects_work_bytes", "par_objects_from_maps_work_bytes", "par_objects_machine_limits", "par_objects_pack",
           "par_objects_unpack", "par_objects_draw_device", "par_objects_from_maps_device", "par_objects_draw_host",
           "par_objects_from_maps_host")

OBJECTS = importlib.import_module("pixel-art-raytracer_amd.objects")  # (without the add-on's binding nothing here can run)
SCREEN = importlib.import_module("pixel-art-raytracer_amd.screen")
VRAM = importlib.import_module("pixel-art-raytracer_amd.vram")


@pytest.fixture(scope="module")
def objects():
    return OBJECTS


def header_text():
    return open(HEADER).read()


def header_code():
    return re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)


def header_prototypes():
    return re.findall(r"^(%s)\s+(par_[a-z_0-9]+)\(([^;]*?)\);" % "|".join(re.escape(r) for r in headers.RETURNS), header_code(),
                      flags=re.M | re.S)


def enum_of(name, text=None):
    body = re.search(r"enum %s \{([^}]*)\}" % name, text or header_code()).group(1)
    return {k: int(v) for k, v in re.findall(r"(PAR_[A-Z0-9_]+) = (\d+)", body)}


def code_of(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ADDON_INCLUDE, header)).read(), flags=re.S)


# ---- declared, exported, bound -------------------------------------------------------------------------------------

def test_the_prototypes_are_the_contracts():
    code = " ".join(header_code().split())
    for proto in (
            "size_t par_objects_work_bytes(int height, int line_limit);",
            "size_t par_objects_from_maps_work_bytes(int n_cells);",
            "int par_objects_machine_limits(int machine, int* line_limit, int* max_objects);",
            "int par_objects_pack(int format, const par_object* objects, int n, uint8_t* out, int* bad);",
            "int par_objects_unpack(int format, const uint8_t* data, int n, par_object* objects_out);",
            "int par_objects_draw_device(void* stream, const par_objects_desc* desc, const uint8_t* chr, const par_object* objects, "
            "const uint32_t* count, const uint8_t* pal_words, const uint8_t* bg_index, void* work, uint8_t* fb_io, uint8_t* index_io, "
            "uint32_t* bad_out, uint32_t* over_out);",
            "int par_objects_from_maps_device(void* stream, const uint32_t* map_bg, const uint8_t* cells_bg, const uint32_t* map, "
            "const uint8_t* cells, int gcx, int gcy, int tile_w, int tile_h, int x0, int y0, int capacity, void* work, "
            "par_object* objects_out, uint32_t* count_out);",
            "int par_objects_draw_host(int device, const par_objects_desc* desc, const uint8_t* chr, const par_object* objects, int count, "
            "const uint8_t* pal_words, const uint8_t* bg_index, uint8_t* fb_io, uint8_t* index_io, int* bad, int* over);",
            "int par_objects_from_maps_host(int device, const uint32_t* map_bg, const uint8_t* cells_bg, const uint32_t* map, "
            "const uint8_t* cells, int gcx, int gcy, int tile_w, int tile_h, int x0, int y0, int capacity, par_object* objects_out, "
            "int* count);"):
        assert proto in code, proto
    assert tuple(name for _, name, _ in header_prototypes()) == SYMBOLS
    assert re.findall(r"#include\s+([<\"][^>\"]+[>\"])", header_code()) == ["<stddef.h>", "<stdint.h>"]
    for define, value in (("PAR_OBJECTS_MAX", "65536"), ("PAR_OBJECTS_MAX_LINE", "128"), ("PAR_OBJECTS_MAX_TILES", r"\(1 << 20\)"),
                          ("PAR_OBJECTS_MAX_CELLS", r"\(1 << 20\)"), ("PAR_OBJECTS_MAX_SIDE", "4096"), ("PAR_OBJECTS_FLIP_X", r"\(1 << 8\)"),
                          ("PAR_OBJECTS_FLIP_Y", r"\(1 << 9\)"), ("PAR_OBJECTS_BEHIND", r"\(1 << 10\)"), ("PAR_OBJECTS_HIDDEN", r"\(1 << 11\)")):
        assert re.search(r"#define %s %s" % (define, value), code), define
    text = " ".join(header_text().replace("\n *", " ").split())  # the comment as running text
    for word in ("Left out on purpose", "high table", "link list", "shape and size bits", "8 x 16 modes", "sprite-zero hit", "the next add-on",
                 "TWO launches", "three launches", "4 * height * (1 + line_limit)", "4 * ceil(n_cells / 1024)", "RESTATED", "MASKS",
                 "NES's and the Game Boy's rule", "closing identity", "31 07 62 64", "2E 1C 09 C5", "56 bytes", "16 bytes", "ascending j",
                 "8 / 64", "10 / 40", "20 / 80", "32 / 128", "128 / 128", "unpack(pack(o)) == o", "no atomic places anything",
                 "q << 3 | q >> 2", "q * 0x55"):
        assert word in text, word


def test_the_enumerations_are_par_screens_and_par_vrams(objects):
    ours, theirs = enum_of("par_objects_tile_format"), enum_of("par_screen_tile_format", code_of("par_screen.h"))
    assert {k.replace("PAR_OBJECTS_", ""): v for k, v in ours.items()} == {k.replace("PAR_SCREEN_", ""): v for k, v in theirs.items()}
    assert list(ours.values()) == list(V.FORMATS) == list(objects.FORMATS) == list(SCREEN.FORMATS) and objects.BPP == V.BPP
    ours, theirs = enum_of("par_objects_palette_format"), enum_of("par_screen_palette_format", code_of("par_screen.h"))
    assert {k.replace("PAR_OBJECTS_", ""): v for k, v in ours.items()} == {k.replace("PAR_SCREEN_", ""): v for k, v in theirs.items()}
    assert (objects.BGR555, objects.BGR333_MD, objects.BGR222, objects.RGBA8) == (SCREEN.BGR555, SCREEN.BGR333_MD, SCREEN.BGR222, SCREEN.RGBA8)
    assert objects.PALETTE_ENTRY_BYTES == SCREEN.PALETTE_ENTRY_BYTES == S.ENTRY_BYTES
    ours, theirs = enum_of("par_objects_machine"), enum_of("par_vram_machine", code_of("par_vram.h"))
    assert {k.replace("PAR_OBJECTS_", ""): v for k, v in ours.items()} == {k.replace("PAR_VRAM_", ""): v for k, v in theirs.items()}
    assert (objects.NES, objects.GBC, objects.SMS, objects.MEGADRIVE, objects.SNES, objects.GBA) == (V.NES, V.GBC, V.SMS, V.MEGADRIVE, V.SNES, V.GBA)
    assert enum_of("par_objects_oam_format") == {"PAR_OBJECTS_OAM_NES": 0, "PAR_OBJECTS_OAM_GB": 1}
    assert (objects.OAM_NES, objects.OAM_GB) == (OB.OAM_NES, OB.OAM_GB) == (0, 1)
    assert (objects.FLIP_X, objects.FLIP_Y, objects.BEHIND, objects.HIDDEN) == (OB.FLIP_X, OB.FLIP_Y, OB.BEHIND, OB.HIDDEN) == (256, 512, 1024, 2048)
    assert (objects.MAX_OBJECTS, objects.MAX_LINE, objects.MAX_TILES, objects.MAX_CELLS, objects.MAX_SIDE) == (
        OB.MAX_OBJECTS, OB.MAX_LINE, OB.MAX_TILES, OB.MAX_CELLS, OB.MAX_SIDE) == (65536, 128, 1 << 20, 1 << 20, 4096)


def test_the_table_is_the_headers_and_no_other_table(par, objects):
    assert SYMBOLS == tuple(objects.ABI_OBJECTS) == objects.ABI_OBJECTS_SYMBOLS
    L = objects.lib()
    assert L is objects.lib() and L is not par.lib()
    for proto in header_prototypes():
        _, name, _ = proto
        want_restype, want = headers.want_signature(proto)
        restype, argtypes = headers.signature(objects.ABI_OBJECTS[name])
        assert list(argtypes) == want and restype is want_restype, name
        fn = getattr(L, name)
        assert list(fn.argtypes) == want and fn.restype is want_restype, name
    assert not any(table is objects.ABI_OBJECTS for table in par.ABI_HEADERS.values())
    others = {name: importlib.import_module("pixel-art-raytracer_amd." + name) for name in ("tileset_reduce", "cells_fit", "vram", "screen", "machine_fit")}
    tables = {"tileset_reduce": "ABI_TILESET_REDUCE", "cells_fit": "ABI_CELLS_FIT", "vram": "ABI_VRAM", "screen": "ABI_SCREEN",
              "machine_fit": "ABI_MACHINE_FIT"}
    for name in SYMBOLS:
        assert not any(name in table for table in (*par.ABI_HEADERS.values(), par.ABI_DEBUG_HOOKS)), name
        assert not hasattr(par.lib(), name), f"{name} is exported by the core library"
        for other, module in others.items():
            assert name not in getattr(module, tables[other]) and not hasattr(module.lib(), name), (name, other)
    for other, module in others.items():
        assert not any(hasattr(L, symbol) for symbol in getattr(module, tables[other])), other
    for h in os.listdir(headers.INCLUDE):
        assert "par_objects_" not in headers.without_comments(h), h
    for h in os.listdir(ADDON_INCLUDE):
        assert h == "par_objects.h" or "par_object" not in code_of(h), h
    for fn in ("work_bytes", "from_maps_work_bytes", "machine_limits", "pack", "unpack", "draw", "from_maps", "draw_host", "from_maps_host", "desc"):
        assert callable(getattr(objects, fn)) and (not hasattr(par, fn) or inspect.ismodule(getattr(par, fn))), fn


def test_the_add_on_exports_exactly_its_table(objects):
    nm = shutil.which("nm")
    assert nm is not None, "no nm to list the library's symbols"
    out = subprocess.run([nm, "-D", "--defined-only", objects.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(f[2] for f in (line.split() for line in out.splitlines()) if len(f) == 3 and f[1] == "T" and f[2].startswith("par_"))
    assert exported == sorted(SYMBOLS)


def test_importing_the_package_does_not_load_the_module():
    code = ("import importlib, json, sys\npar = importlib.import_module('pixel-art-raytracer_amd')\npar.lib()\n"
            "print(json.dumps(sorted(m for m in sys.modules if m.startswith('pixel-art-raytracer_amd.'))))\n"
            "objects = importlib.import_module('pixel-art-raytracer_amd.objects')\n"
            "print(json.dumps([objects.work_bytes(24, 8), objects.lib() is not par.lib()]))")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = p.stdout.strip().splitlines()
    assert json.loads(out[-2]) == ["pixel-art-raytracer_amd.abi", "pixel-art-raytracer_amd.types"]
    assert json.loads(out[-1]) == [4 * 24 * 9, True]


def test_a_missing_library_is_the_loaders_import_error(par, objects, monkeypatch, tmp_path):
    missing = str(tmp_path / "lib" / "libpar_objects.so")
    monkeypatch.setattr(objects, "LIB_PATH", missing)
    monkeypatch.setattr(objects, "_lib", None)
    with pytest.raises(ImportError) as e:
        objects.lib()
    assert str(e.value) == (f"{missing} is missing: build it with `make -C pixel-art-raytracer_amd/csrc` "
                            "(or __graft_entry__.build()). There is no CPU fallback.")
    assert objects._lib is None


def struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header_code(), flags=re.S).group(1)
    return [(kind, n.strip()) for kind, names in re.findall(r"(\w+)\s+([^;]+);", body) for n in names.split(",")]


def test_the_structures_are_the_headers(objects):
    record = struct_fields("par_object")
    assert record == [("int32_t", n) for n in ("x", "y", "tile", "attr")]
    assert objects.OBJECT == OB.OBJECT and objects.OBJECT.itemsize == 16 and objects.OBJECT.names == ("x", "y", "tile", "attr")
    assert [objects.OBJECT.fields[n][1] for n in objects.OBJECT.names] == [0, 4, 8, 12]
    assert all(objects.OBJECT.fields[n][0] == np.dtype(np.int32) for n in objects.OBJECT.names)
    desc = struct_fields("par_objects_desc")
    assert all(kind == "int32_t" for kind, _ in desc)
    assert tuple(n for _, n in desc) == OB.DESC_FIELDS == objects.DESC_FIELDS == tuple(n for n, _ in objects.Desc._fields_)
    assert C.sizeof(objects.Desc) == 4 * 14 == 56 and C.alignment(objects.Desc) == 4
    for i, name in enumerate(OB.DESC_FIELDS):
        field = getattr(objects.Desc, name)
        assert (field.offset, field.size) == (4 * i, 4), name
    d = objects.desc(tile_w=16, line_limit=32)
    assert (d.tile_w, d.line_limit, d.bg_sub_size, d.opaque) == (16, 32, 1, 0)
    with pytest.raises(TypeError, match="no field"):
        objects.desc(tiles=3)


BODY = r"""
#include <stdio.h>
int main(void) {
    unsigned char chr[32] = {0}, fb[4 * 64] = {9, 9}, oam[8] = {0};
    par_object o[2] = {{100, 50, 7, 2 | PAR_OBJECTS_FLIP_X | PAR_OBJECTS_BEHIND}, {20, 30, 9, 5 | PAR_OBJECTS_FLIP_Y | PAR_OBJECTS_BEHIND}};
    par_object back[1];
    par_objects_desc d = {8, 12, PAR_OBJECTS_4BPP_ROWS, 1, 2, 8, PAR_OBJECTS_RGBA8, 1, 1, 0, 1, 0, 8, 8};
    uint32_t work[8 * 9], out[1] = {5};
    int line = 0, most = 0, bad = 7;
    int rc = par_objects_draw_device(NULL, &d, chr, o, NULL, chr, NULL, work, fb, NULL, NULL, NULL);
    int rc_maps = par_objects_from_maps_device(NULL, out, NULL, out, NULL, 1, 1, 8, 8, 0, 0, 0, work, o, out);
    int rc_lim = par_objects_machine_limits(PAR_OBJECTS_SNES, &line, &most);
    int rc_pack = par_objects_pack(PAR_OBJECTS_OAM_NES, o, 1, oam, &bad);
    par_objects_pack(PAR_OBJECTS_OAM_GB, o + 1, 1, oam + 4, &bad);
    par_objects_unpack(PAR_OBJECTS_OAM_GB, oam + 4, 1, back);
    printf("%d %d %d %u %u %d %d %d %d %d %02X%02X%02X%02X %02X%02X%02X%02X %d %d %lu %lu %lu %lu\n",
           PAR_OBJECTS_MAX + PAR_OBJECTS_MAX_LINE + PAR_OBJECTS_MAX_TILES + PAR_OBJECTS_MAX_CELLS + PAR_OBJECTS_MAX_SIDE, rc, rc_maps,
           (unsigned)fb[0], (unsigned)out[0], rc_lim, line, most, rc_pack, bad, oam[0], oam[1], oam[2], oam[3], oam[4], oam[5], oam[6], oam[7],
           (int)back[0].x, (int)back[0].attr, (unsigned long)par_objects_work_bytes(8, 8), (unsigned long)par_objects_from_maps_work_bytes(1025),
           (unsigned long)sizeof(par_object), (unsigned long)sizeof(par_objects_desc));
    return 0;
}
"""
CORE = ["par_raytracer.h", "par_cells.h", "par_tileset.h", "par_tileset_extend.h"]
ADDONS = ["par_tileset_reduce.h", "par_cells_fit.h", "par_vram.h", "par_screen.h", "par_machine_fit.h"]


def test_every_other_add_on_header_is_compiled_beside_it():
    """ADDONS above is every other header of addons/include."""
    assert sorted(os.listdir(ADDON_INCLUDE)) == sorted(ADDONS + ["par_objects.h"])


@pytest.mark.parametrize("includes", [["par_objects.h"], ["par_objects.h"] * 2, CORE + ADDONS + ["par_objects.h"], ["par_objects.h"] + ADDONS + CORE],
                         ids=["alone", "twice", "behind the core and the add-ons", "before them"])
def test_header_is_pedantic_c11(tmp_path, includes):
    src, exe = tmp_path / "objects.c", tmp_path / "objects"
    src.write_text("".join(f'#include "{h}"\n' for h in includes) + BODY)
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", ADDON_INCLUDE, "-I", headers.INCLUDE,
                        str(src), "-o", str(exe), "-L", headers.LIB_DIR, "-lpar_objects", f"-Wl,-rpath,{headers.LIB_DIR}"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    # tile_h 12 and capacity 0 are refused; the anchors of the header; 20 | fy | behind comes back
    assert out.returncode == 0 and out.stdout.split() == [
        str(65536 + 128 + (2 << 20) + 4096), "1", "1", "9", "5", "0", "32", "128", "0", "0", "31076264", "2E1C09C5", "20", str(5 | 512 | 1024),
        str(4 * 8 * 9), "8", "16", "56"], (out.stdout, out.stderr)


def test_the_enumerations_by_static_assert(tmp_path):
    names = ("1BPP", "2BPP_PLANAR", "2BPP_ROWS", "4BPP_ROWS", "4BPP_PACKED_HI", "4BPP_PACKED_LO", "4BPP_ROW_PLANES", "BGR555", "BGR333_MD", "BGR222", "RGBA8")
    asserts = "".join(f'_Static_assert((int)PAR_OBJECTS_{n} == (int)PAR_SCREEN_{n}, "{n}");\n' for n in names)
    asserts += "".join(f'_Static_assert((int)PAR_OBJECTS_{n} == (int)PAR_VRAM_{n}, "{n}");\n' for n in ("NES", "GBC", "SMS", "MEGADRIVE", "SNES", "GBA"))
    src = tmp_path / "all.c"
    src.write_text('#include "par_vram.h"\n#include "par_screen.h"\n#include "par_objects.h"\n'
                   '_Static_assert(sizeof(par_object) == 16 && sizeof(par_objects_desc) == 56, "no padding");\n'
                   '_Static_assert(offsetof(par_object, attr) == 12 && offsetof(par_objects_desc, height) == 52, "offsets");\n'
                   '_Static_assert(PAR_OBJECTS_MAX_TILES == PAR_SCREEN_MAX_TILES && PAR_OBJECTS_MAX_SIDE == PAR_SCREEN_MAX_SIDE, "limits");\n'
                   + asserts + "int main(void) { return 0; }\n")
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", ADDON_INCLUDE, "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


# ---- argument errors: no device needed, nothing written -----------------------------------------------------------

def buffers():
    return {"chr": np.full(12 * 128, 0xA5, np.uint8), "objects": np.full(4 * 16 + 2, 3, np.int32), "count": np.full(2, 5, np.uint32),
            "pal_words": np.full(1024, 0x3C, np.uint8), "bg_index": np.full(32 * 24, 1, np.uint8), "work": np.full(24 * 9 + 2, 7, np.uint32),
            "fb_io": np.full(4 * 32 * 24 + 8, 0x5A, np.uint8), "index_io": np.full(32 * 24 + 8, 0xC3, np.uint8),
            "bad_out": np.full(2, 0x11111111, np.uint32), "over_out": np.full(2, 0x33333333, np.uint32), "bad": np.full(2, 0x22222222, np.int32),
            "over": np.full(2, 0x44444444, np.int32), "map_bg": np.full(14, 1, np.uint32), "map": np.full(14, 2, np.uint32),
            "cells_bg": np.full(12, 0, np.uint8), "cells": np.full(12, 1, np.uint8), "objects_out": np.full(4 * 16 + 2, 9, np.int32),
            "count_out": np.full(2, 0x55555555, np.uint32), "found": np.full(2, 0x66666666, np.int32), "out": np.full(64, 0x77, np.uint8),
            "data": np.full(64, 0x12, np.uint8)}


SCALARS = dict(gcx=4, gcy=3, tile_w=8, tile_h=8, x0=0, y0=0, capacity=12, host_count=16, format=0, n=16, machine=0)


def raw_call(objects, which, over):
    """One call of the raw symbol on host dummies: (status, whether any buffer changed)."""
    L = objects.lib()
    bufs = buffers()
    before = {k: v.copy() for k, v in bufs.items()}
    arg = dict(desc=OB.desc_of(), **SCALARS, **bufs)
    shifts = {k[:-6]: v for k, v in over.items() if k.endswith("_shift")}
    for k, v in over.items():
        if k.endswith("_shift"):
            continue
        if k in OB.DESC_FIELDS:
            arg["desc"][k] = v
        elif k.startswith("m_"):  # a from_maps scalar that shares its name with a descriptor field
            arg[k[2:]] = v
        else:
            arg[k] = v

    def p(name):
        return C.c_void_p(arg[name].ctypes.data + shifts.get(name, 0)) if arg[name] is not None else None

    d = None if arg["desc"] is None else objects.desc(**arg["desc"])
    by_ref = lambda s: None if s is None else C.byref(s)  # noqa: E731
    a = arg
    if which == "draw":
        rc = L.par_objects_draw_device(None, by_ref(d), p("chr"), p("objects"), p("count"), p("pal_words"), p("bg_index"), p("work"), p("fb_io"),
                                       p("index_io"), p("bad_out"), p("over_out"))
    elif which == "draw_host":
        rc = L.par_objects_draw_host(-1, by_ref(d), p("chr"), p("objects"), a["host_count"], p("pal_words"), p("bg_index"), p("fb_io"), p("index_io"),
                                     p("bad"), p("over"))
    elif which == "maps":
        rc = L.par_objects_from_maps_device(None, p("map_bg"), p("cells_bg"), p("map"), p("cells"), a["gcx"], a["gcy"], a["tile_w"], a["tile_h"],
                                            a["x0"], a["y0"], a["capacity"], p("work"), p("objects_out"), p("count_out"))
    elif which == "maps_host":
        rc = L.par_objects_from_maps_host(-1, p("map_bg"), p("cells_bg"), p("map"), p("cells"), a["gcx"], a["gcy"], a["tile_w"], a["tile_h"],
                                          a["x0"], a["y0"], a["capacity"], p("objects_out"), p("found"))
    elif which == "pack":
        rc = L.par_objects_pack(a["format"], p("objects"), a["n"], p("out"), p("bad"))
    elif which == "unpack":
        rc = L.par_objects_unpack(a["format"], p("data"), a["n"], p("objects_out"))
    else:
        rc = L.par_objects_machine_limits(a["machine"], p("bad"), p("over"))
    return rc, any(bufs[k].tobytes() != before[k].tobytes() for k in bufs)


DRAW_RULES = [
    ("null desc", dict(desc=None)), ("null chr", dict(chr=None)), ("null objects", dict(objects=None)),
    ("both planes null", dict(fb_io=None, index_io=None)), ("an fb_io without pal_words", dict(pal_words=None)),
    ("objects off their 4 bytes", dict(objects_shift=2)), ("fb_io off its 4 bytes", dict(fb_io_shift=1)),
    ("tile_w 4", dict(tile_w=4)), ("tile_w 12", dict(tile_w=12)), ("tile_w 32", dict(tile_w=32)), ("tile_h 0", dict(tile_h=0)),
    ("tile_h 24", dict(tile_h=24)), ("tile_h -8", dict(tile_h=-8)), ("format -1", dict(tile_format=-1)), ("format 7", dict(tile_format=7)),
    ("n_tiles 0", dict(n_tiles=0)), ("n_tiles -1", dict(n_tiles=-1)), ("n_tiles 2^20 + 1", dict(n_tiles=(1 << 20) + 1)),
    ("n_objects 0", dict(n_objects=0)), ("n_objects -1", dict(n_objects=-1)), ("n_objects 65537", dict(n_objects=65537)),
    ("line_limit 0", dict(line_limit=0)), ("line_limit -1", dict(line_limit=-1)), ("line_limit 129", dict(line_limit=129)),
    ("pal_format -1", dict(pal_format=-1)), ("pal_format 4", dict(pal_format=4)), ("n_colors 0", dict(n_colors=0)),
    ("n_colors 257", dict(n_colors=257)), ("sub_size 0", dict(sub_size=0)), ("sub_size 257", dict(sub_size=257)), ("sub_size -1", dict(sub_size=-1)),
    ("pal_base -1", dict(pal_base=-1)), ("pal_base 256", dict(pal_base=256)), ("bg_sub_size 0", dict(bg_sub_size=0)),
    ("bg_sub_size 257", dict(bg_sub_size=257)), ("opaque 2", dict(opaque=2)), ("opaque -1", dict(opaque=-1)), ("width 0", dict(width=0)),
    ("width 4097", dict(width=4097)), ("width -1", dict(width=-1)), ("height 0", dict(height=0)), ("height 4097", dict(height=4097))]
MAPS_RULES = [
    ("null map_bg", dict(map_bg=None)), ("null map", dict(map=None)), ("null objects_out", dict(objects_out=None)),
    ("cells without cells_bg", dict(cells_bg=None)), ("cells_bg without cells", dict(cells=None)),
    ("map_bg off its 4 bytes", dict(map_bg_shift=2)), ("map off its 4 bytes", dict(map_shift=1)), ("objects_out off its 4 bytes", dict(objects_out_shift=2)),
    ("gcx 0", dict(gcx=0)), ("gcy 0", dict(gcy=0)), ("gcx -1", dict(gcx=-1)), ("gcy -1", dict(gcy=-1)), ("2^20 + 1 cells", dict(gcx=(1 << 20) + 1, gcy=1)),
    ("a product that wraps 32 bits", dict(gcx=1 << 16, gcy=1 << 16)), ("tile_w 4", dict(m_tile_w=4)), ("tile_w 32", dict(m_tile_w=32)),
    ("tile_h 0", dict(m_tile_h=0)), ("tile_h 12", dict(m_tile_h=12)), ("capacity 0", dict(capacity=0)), ("capacity -1", dict(capacity=-1)),
    ("capacity 65537", dict(capacity=65537)), ("x0 -32769", dict(x0=-32769)), ("y0 -32769", dict(y0=-32769)), ("x0 32768", dict(x0=32768)),
    ("y0 32768", dict(y0=32768)), ("the last column past int16", dict(x0=32767 - 23)), ("the last row past int16", dict(y0=32767 - 15)),
    ("a sum that wraps 32 bits", dict(x0=(1 << 31) - 1))]
BAD = {
    "draw": DRAW_RULES + [("null work", dict(work=None)), ("work off its 4 bytes", dict(work_shift=2)), ("count off its 4 bytes", dict(count_shift=2)),
                          ("bad_out off its 4 bytes", dict(bad_out_shift=2)), ("over_out off its 4 bytes", dict(over_out_shift=1))],
    "draw_host": DRAW_RULES + [("null bad", dict(bad=None)), ("null over", dict(over=None)), ("count -1", dict(host_count=-1))],
    "maps": MAPS_RULES + [("null work", dict(work=None)), ("work off its 4 bytes", dict(work_shift=1)), ("null count_out", dict(count_out=None)),
                          ("count_out off its 4 bytes", dict(count_out_shift=2))],
    "maps_host": MAPS_RULES + [("null count", dict(found=None))],
    "pack": [("format -1", dict(format=-1)), ("format 2", dict(format=2)), ("null objects", dict(objects=None)), ("null out", dict(out=None)),
             ("null bad", dict(bad=None)), ("n 0", dict(n=0)), ("n -1", dict(n=-1)), ("n 65537", dict(n=65537))],
    "unpack": [("format -1", dict(format=-1)), ("format 2", dict(format=2)), ("null data", dict(data=None)), ("null objects_out", dict(objects_out=None)),
               ("n 0", dict(n=0)), ("n -1", dict(n=-1)), ("n 65537", dict(n=65537))],
    "limits": [("machine -1", dict(machine=-1)), ("machine 6", dict(machine=6)), ("null line_limit", dict(bad=None)), ("null max_objects", dict(over=None))]}


@pytest.mark.parametrize("which", list(BAD))
def test_invalid_arguments_need_no_device_and_write_nothing(objects, which):
    bad = BAD[which]
    assert len({tag for tag, _ in bad}) == len(bad)
    for tag, over in bad:
        rc, changed = raw_call(objects, which, over)
        assert rc == ERR_INVALID_ARG, f"{which}: {tag}: status {rc}"
        assert not changed, f"{which}: {tag}: something was written"


def test_what_the_rules_admit_is_not_refused(par, objects):
    """The host forms on the arguments next to the refused ones (the device forms would take host dummies for device
    memory): any status but PAR_ERR_INVALID_ARG, which without a GPU is PAR_ERR_NO_DEVICE."""
    want = 0 if par.device_count() > 0 else ERR_NO_DEVICE
    for which, overs in (
            ("draw_host", [dict(), dict(fb_io=None, pal_words=None), dict(index_io=None), dict(bg_index=None), dict(host_count=0),
                           dict(host_count=1 << 30), dict(tile_w=16, tile_h=16, n_tiles=3), dict(line_limit=1), dict(line_limit=128),
                           dict(n_colors=256, sub_size=256, pal_base=255, bg_sub_size=256), dict(n_colors=1, sub_size=1), dict(opaque=1),
                           dict(width=1, height=1), dict(index_io_shift=3), dict(chr_shift=1, pal_words_shift=3, bg_index_shift=1),
                           *(dict(tile_format=f) for f in V.FORMATS), *(dict(pal_format=f) for f in S.PAL_FORMATS)]),
            ("maps_host", [dict(), dict(cells=None, cells_bg=None), dict(gcx=1, gcy=1), dict(capacity=1), dict(capacity=65536),
                           dict(x0=-32768, y0=-32768), dict(x0=32767 - 24, y0=32767 - 16), dict(m_tile_w=16, m_tile_h=16, x0=-100)])):
        for over in overs:
            rc, _ = raw_call(objects, which, over)
            assert rc == want, (which, over, rc)
    for which in ("pack", "unpack", "limits"):
        assert raw_call(objects, which, dict())[0] == 0, which


def test_binding_raises_and_checks_its_arrays(par, objects):
    d = objects.desc(**OB.desc_of(width=0))
    with pytest.raises(par.ParError) as e:
        objects.draw(d, 0x1000, 0x2000, 0x3000, index_io=0x4000)
    assert e.value.status == ERR_INVALID_ARG and str(e.value) == "PAR_ERR_INVALID_ARG: par_objects_draw_device"
    with pytest.raises(par.ParError) as e:
        objects.from_maps(0x1000, 0x2000, (4, 3), (8, 8), 0, 0x3000, 0x4000, 0x5000)
    assert str(e.value) == "PAR_ERR_INVALID_ARG: par_objects_from_maps_device"
    with pytest.raises(par.ParError) as e:
        objects.machine_limits(6)
    assert str(e.value) == "PAR_ERR_INVALID_ARG: par_objects_machine_limits"
    with pytest.raises(par.ParError) as e:
        objects.pack(2, np.zeros(1, objects.OBJECT))
    assert str(e.value) == "PAR_ERR_INVALID_ARG: par_objects_pack"
    d.width = 32
    chr_data, table, pal = np.zeros(12 * 32, np.uint8), np.zeros(16, objects.OBJECT), np.zeros(64, np.uint8)
    index = np.zeros((24, 32), np.uint8)
    with pytest.raises(ValueError, match="draw_host: chr holds"):
        objects.draw_host(d, chr_data[:-1], table, pal, index=index)
    with pytest.raises(ValueError, match="draw_host: 15 objects"):
        objects.draw_host(d, chr_data, table[:-1], pal, index=index)
    with pytest.raises(ValueError, match="not OBJECT records"):
        objects.draw_host(d, chr_data, np.zeros(64, np.int32), pal, index=index)
    with pytest.raises(ValueError, match="draw_host: the palette holds"):
        objects.draw_host(d, chr_data, table, pal[:-4], index=index)
    with pytest.raises(ValueError, match="draw_host: index holds"):
        objects.draw_host(d, chr_data, table, pal, index=index[:-1])
    with pytest.raises(ValueError, match="draw_host: bg_index names"):
        objects.draw_host(d, chr_data, table, pal, fb=np.zeros((24, 32, 4), np.uint8), bg_index="index")
    with pytest.raises(ValueError, match="from_maps_host: the maps hold"):
        objects.from_maps_host(np.zeros(11, np.uint32), np.zeros(12, np.uint32), (4, 3), (8, 8), 4)
    with pytest.raises(ValueError, match="unpack: the data holds"):
        objects.unpack(0, np.zeros(5, np.uint8))
    for bad in ("s", 1.5, np.int64(0x1000)):
        with pytest.raises(TypeError):
            objects.draw(d, bad, 0x2000, 0x3000, index_io=0x4000)
        with pytest.raises(TypeError):
            objects.draw(d, 0x1000, 0x2000, 0x3000, index_io=0x4000, stream=bad)


def test_arguments_reach_the_library_in_the_headers_order(par, objects, monkeypatch):
    from test_binding_cpu import A, StandIn
    stand_in = StandIn(returns={"par_objects_work_bytes": 777, "par_objects_from_maps_work_bytes": 88})
    monkeypatch.setattr(objects, "lib", lambda: stand_in)
    assert objects.work_bytes(24, 8) == 777 and stand_in.calls.pop() == ("par_objects_work_bytes", [24, 8])
    assert objects.from_maps_work_bytes(99) == 88 and stand_in.calls.pop() == ("par_objects_from_maps_work_bytes", [99])
    d = objects.desc(**OB.desc_of())
    objects.draw(d, 0x1000, 0x2000, 0x3000, pal_words=0x4000, fb_io=0x5000, index_io=0x6000, count=0x7000, bg_index=0x8000, bad_out=0x9000,
                 over_out=0xA000, stream=0xB000)
    assert stand_in.calls.pop() == ("par_objects_draw_device", [0xB000, A(d), 0x1000, 0x2000, 0x7000, 0x4000, 0x8000, 0x3000, 0x5000, 0x6000,
                                                              0x9000, 0xA000])
    objects.draw(d, 0x1000, 0x2000, 0x3000, index_io=0x6000)
    assert stand_in.calls.pop() == ("par_objects_draw_device", [None, A(d), 0x1000, 0x2000, None, None, None, 0x3000, None, 0x6000, None, None])
    objects.from_maps(0x1000, 0x2000, (4, 3), (8, 16), 12, 0x3000, 0x4000, 0x5000, cells_bg=0x6000, cells=0x7000, origin=(-5, 9), stream=0x8000)
    assert stand_in.calls.pop() == ("par_objects_from_maps_device", [0x8000, 0x1000, 0x6000, 0x2000, 0x7000, 4, 3, 8, 16, -5, 9, 12, 0x3000,
                                                                   0x4000, 0x5000])
    stand_in.writes = {"par_objects_draw_host": {9: 3, 10: 4}, "par_objects_from_maps_host": {13: 2}, "par_objects_machine_limits": {1: 8, 2: 64},
                       "par_objects_pack": {4: 1}}
    assert objects.machine_limits(0) == (8, 64)
    chr_data, table, pal = np.zeros(12 * 32, np.uint8), np.zeros(16, objects.OBJECT), np.zeros(64, np.uint8)
    index, fb = np.zeros((24, 32), np.uint8), np.zeros((24, 32, 4), np.uint8)
    out = objects.draw_host(d, chr_data, table, pal, fb=fb, index=index, count=5, bg_index="index", device=1)
    name, args = stand_in.calls.pop()
    assert name == "par_objects_draw_host" and args[:6] == [1, A(d), A(chr_data), A(table), 5, A(pal)]
    assert args[6:9] == [A(out["index"]), A(out["fb"]), A(out["index"])] and (out["bad"], out["over"]) == (3, 4)
    assert out["fb"] is not fb and out["index"] is not index, "the caller's planes are copied"
    out = objects.draw_host(d, chr_data, table, index=index)
    name, args = stand_in.calls.pop()
    assert args[4:8] == [16, None, None, None] and out["fb"] is None
    maps = np.zeros(12, np.uint32)
    got = objects.from_maps_host(maps, maps, (4, 3), (8, 8), 7, origin=(1, 2), device=2)
    name, args = stand_in.calls.pop()
    assert name == "par_objects_from_maps_host" and args[:12] == [2, A(maps), None, A(maps), None, 4, 3, 8, 8, 1, 2, 7]
    assert got["count"] == 2 and len(got["objects"]) == 2
    packed, bad = objects.pack(1, table)
    name, args = stand_in.calls.pop()
    assert name == "par_objects_pack" and args[:3] == [1, A(table), 16] and bad == 1 and packed.shape == (16, 4)
    stand_in.status = 4
    with pytest.raises(par.ParError) as e:
        objects.from_maps_host(maps, maps, (4, 3), (8, 8), 7)
    assert e.value.status == 4 and str(e.value) == "PAR_ERR_OOM: par_objects_from_maps_host"


# ---- host arithmetic ---------------------------------------------------------------------------------------------------

def test_both_work_bytes_formulas(objects):
    for h in (1, 9, 37, 4096):
        for limit in (1, 8, 127, 128):
            assert objects.work_bytes(h, limit) == OB.work_bytes(h, limit) == 4 * h * (1 + limit)
    for h, limit in ((0, 8), (4097, 8), (-1, 8), (24, 0), (24, 129), (24, -1)):
        assert objects.work_bytes(h, limit) == OB.work_bytes(h, limit) == 0
    for n in (1, 1023, 1024, 1025, 2400, 1 << 18, 1 << 20):
        got = objects.from_maps_work_bytes(n)
        assert got == OB.from_maps_work_bytes(n) == 4 * ((n + 1023) // 1024) and 0 < got <= 4 * n + 4096
    for n in (0, -1, (1 << 20) + 1):
        assert objects.from_maps_work_bytes(n) == OB.from_maps_work_bytes(n) == 0
    assert objects.lib().par_objects_work_bytes.restype is C.c_size_t


def test_the_limits_table(objects):
    assert {m: objects.machine_limits(m) for m in range(6)} == OB.LIMITS == {0: (8, 64), 1: (10, 40), 2: (8, 64), 3: (20, 80), 4: (32, 128),
                                                                               5: (128, 128)}


NES_EDGES = dict(x=(0, 255), y=(1, 256), tile=(0, 255), p=(0, 3))
GB_EDGES = dict(x=(-8, 247), y=(-16, 239), tile=(0, 255), p=(0, 7))


def test_the_anchors_of_the_header(objects):
    nes = OB.objects_of([(100, 50, 7, 2 | OB.FLIP_X | OB.BEHIND)])
    gb = OB.objects_of([(20, 30, 9, 5 | OB.FLIP_Y | OB.BEHIND)])
    for fmt, o, want in ((OB.OAM_NES, nes, [0x31, 0x07, 0x62, 0x64]), (OB.OAM_GB, gb, [0x2E, 0x1C, 0x09, 0xC5])):
        for got in (objects.pack(fmt, o), OB.pack(fmt, o), OB.pack_loop(fmt, o)):
            assert got[0].tolist() == [want] and got[1] == 0
        for back in (objects.unpack(fmt, np.array(want, np.uint8)), OB.unpack(fmt, want), OB.unpack_loop(fmt, want)):
            assert back.tobytes() == o.tobytes()


@pytest.mark.parametrize("fmt,edges", [(OB.OAM_NES, NES_EDGES), (OB.OAM_GB, GB_EDGES)], ids=["nes", "gb"])
def test_pack_and_unpack_on_every_field_edge(objects, fmt, edges):
    """Each field at its two ends and one past them, the others in the middle; every flag; hidden. Consequence 8."""
    middle = dict(x=100, y=100, tile=100, p=1)
    records, fit = [], []
    for field, (lo, hi) in edges.items():
        for value, ok in ((lo, True), (hi, True), (lo - 1, field == "p" and False), (hi + 1, False)):
            if field == "p" and value < 0:
                continue
            r = dict(middle, **{field: value})
            records.append((r["x"], r["y"], r["tile"], r["p"]))
            fit.append(ok)
    for flags in range(8):
        records.append((middle["x"], middle["y"], middle["tile"], middle["p"] | flags << 8))
        fit.append(True)
    records.append((70000, -70000, 300, 200 | 1 << 20))
    fit.append(False)
    o = OB.objects_of(records)
    assert OB.fits(fmt, o).tolist() == fit
    got, bad = objects.pack(fmt, o)
    for other in (OB.pack(fmt, o), OB.pack_loop(fmt, o)):
        assert got.tobytes() == other[0].tobytes() and bad == other[1] == fit.count(False)
    back = objects.unpack(fmt, got)
    assert back.tobytes() == OB.unpack(fmt, got).tobytes() == OB.unpack_loop(fmt, got).tobytes()
    keep = np.array(fit)
    assert back[keep].tobytes() == o[keep].tobytes(), "unpack inverts pack on the fitting ones"
    assert not (back["attr"] & OB.HIDDEN).any()
    # hidden: byte 0 alone says so, the other bytes as they are, and never counted
    hidden = o.copy()
    hidden["attr"] |= OB.HIDDEN
    h, h_bad = objects.pack(fmt, hidden)
    assert h_bad == 0 == OB.pack(fmt, hidden)[1] == OB.pack_loop(fmt, hidden)[1] and h.tobytes() == OB.pack(fmt, hidden)[0].tobytes()
    assert (h[:, 0] == (0xFF if fmt == OB.OAM_NES else 0)).all() and h[:, 1:].tobytes() == got[:, 1:].tobytes()
    # random tables round the limits
    rng = np.random.default_rng(80 + fmt)
    r = np.zeros(500, OB.OBJECT)
    r["x"], r["y"], r["tile"] = rng.integers(-40, 300, 500), rng.integers(-40, 300, 500), rng.integers(-5, 270, 500)
    r["attr"] = rng.integers(0, 12, 500) | rng.integers(0, 16, 500) << 8
    got, bad = objects.pack(fmt, r)
    assert got.tobytes() == OB.pack(fmt, r)[0].tobytes() == OB.pack_loop(fmt, r)[0].tobytes() and bad == OB.pack(fmt, r)[1] == OB.pack_loop(fmt, r)[1]
    ok = OB.fits(fmt, r) & ((r["attr"] & OB.HIDDEN) == 0)
    assert 50 < ok.sum() < 450 and objects.unpack(fmt, got)[ok].tobytes() == r[ok].tobytes()


# ---- the model the GPU tests compare with --------------------------------------------------------------------------

def planes_of(rng, d, with_fb=True):
    fb = rng.integers(0, 256, (d["height"], d["width"], 4), dtype=np.uint8) if with_fb else None
    return fb, rng.integers(0, d["n_colors"], (d["height"], d["width"]), dtype=np.uint8)


def both(d, chr_bytes, table, pal=None, bg=None, fb=None, index=None, count=None):
    """The two forms of the model, held to each other: (fb, index, bad, over)."""
    a = OB.draw(d, chr_bytes, table, pal, bg, fb, index, count)
    b = OB.draw_loop(d, chr_bytes, table, pal, bg, fb, index, count)
    assert a[2:] == b[2:]
    for x, y in zip(a[:2], b[:2]):
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes())
    return a


@pytest.mark.parametrize("fmt", V.FORMATS, ids=V.FORMAT_NAMES)
def test_model_equals_the_loop_on_random_tables(fmt):
    rng = np.random.default_rng(200 + fmt)
    seen_over = seen_bad = 0
    for i, tile in enumerate(TS.TILES):
        d = OB.desc_of(tile_w=tile[0], tile_h=tile[1], tile_format=fmt, n_tiles=7, n_objects=40, line_limit=(1, 3, 8, 128)[i],
                       pal_format=S.PAL_FORMATS[i], n_colors=(16, 13, 256, 1)[i], sub_size=(4, 3, 16, 2)[i], pal_base=(0, 5, 200, 0)[i],
                       bg_sub_size=(4, 3, 2, 1)[i], opaque=i % 2, width=(29, 40, 17, 33)[i], height=(21, 9, 33, 16)[i])
        chr_bytes = OB.random_chr(rng, d)
        table = OB.random_table(rng, d, 40, behind_share=0.4)
        pal = rng.integers(0, 256, d["n_colors"] * S.ENTRY_BYTES[d["pal_format"]], dtype=np.uint8)
        fb, index = planes_of(rng, d)
        bg = (None, "index", rng.integers(0, 16, (d["height"], d["width"]), dtype=np.uint8), "index")[i]
        got = both(d, chr_bytes, table, pal, bg, fb, index, count=(None, 40, 33, 99)[i])
        assert got[0].tobytes() != fb.tobytes() and (d["n_colors"] == 1 or got[1].tobytes() != index.tobytes())
        seen_over += got[3]
        seen_bad += got[2]
        only_index = both(d, chr_bytes, table, None, bg, None, index)
        assert only_index[0] is None and (i == 2 or only_index[1].tobytes() == got[1].tobytes())
    assert seen_over > 0 and seen_bad > 0


def test_from_maps_model_equals_the_loop():
    rng = np.random.default_rng(77)
    for grid, tile, share in (((1, 1), (8, 8), 1.0), ((8, 6), (16, 8), 0.3), ((61, 3), (8, 16), 0.5), ((7, 5), (16, 16), 0.0)):
        n = grid[0] * grid[1]
        a = rng.integers(0, 50, n).astype(np.uint32) | rng.integers(0, 4, n).astype(np.uint32) << 30
        b = np.where(rng.random(n) < share, a ^ (rng.integers(1, 4, n).astype(np.uint32) << rng.choice([0, 30], n).astype(np.uint32)), a).astype(np.uint32)
        ca = rng.integers(0, 4, n, dtype=np.uint8)
        cb = np.where(rng.random(n) < share / 2, ca ^ 1, ca).astype(np.uint8)
        for cells in (None, (ca, cb)):
            for capacity in (1, n, 65536):
                kw = dict(origin=(-13, 7)) if cells is None else dict(cells_bg=cells[0], cells=cells[1], origin=(5, -9))
                x, y = OB.from_maps(a, b, grid, tile, capacity, **kw), OB.from_maps_loop(a, b, grid, tile, capacity, **kw)
                assert x[1] == y[1] and x[0].tobytes() == y[0].tobytes() and len(x[0]) == min(x[1], capacity)
    # worked by hand: cells 1 and 5 of a 3 x 2 grid differ, one by its word's flip bit, one by its cell byte
    a = np.array([1, 2, 3, 4, 5, 6], np.uint32)
    b = np.array([1, 2 | 1 << 31, 3, 4, 5, 6], np.uint32)
    got, total = OB.from_maps(a, b, (3, 2), (8, 16), 8, np.zeros(6, np.uint8), np.array([0, 2, 0, 0, 0, 3], np.uint8), origin=(10, 20))
    assert total == 2 and got.tolist() == [(18, 20, 2, 2 | OB.FLIP_Y), (26, 36, 6, 3)]


# ---- crafted tables, worked out by hand ---------------------------------------------------------------------------------

def solid_tiles(values, tile=(8, 8), fmt=V.F_4BPP_ROWS):
    """Tile k filled with values[k]."""
    tiles = np.stack([np.full((tile[1], tile[0]), v, np.uint8) for v in values])
    return tiles, V.encode_tiles(tiles, tile, fmt)[0]


def crafted(table, values, bg=None, index=None, **over):
    d = OB.desc_of(n_tiles=len(values), n_objects=len(table), n_colors=64, sub_size=4, bg_sub_size=4, width=16, height=16, **over)
    index = np.full((16, 16), 63, np.uint8) if index is None else index
    return both(d, solid_tiles(values)[1], OB.objects_of(table), None, bg, None, index)


def test_a_stack_of_three_objects_on_one_pixel():
    """Objects 0, 1 and 2 at (4, 4), (6, 6) and (8, 8): pixel (9, 9) is under all three and shows object 0, (13, 13) under
    1 and 2 shows 1, (15, 15) shows 2; sub-palettes 0, 1, 2 and values 1, 2, 3 give indices 1, 6, 11."""
    _, index, bad, over = crafted([(4, 4, 0, 0), (6, 6, 1, 1), (8, 8, 2, 2)], [1, 2, 3])
    assert (bad, over) == (0, 0)
    assert index[9, 9] == 1 and index[13, 13] == 6 and index[15, 15] == 11 and index[3, 3] == 63 and index[4, 4] == 1 and index[12, 11] == 6
    assert int((index == 1).sum()) == 64 and int((index == 6).sum()) == 64 - 36 and int((index == 11).sum()) == 64 - 36


def test_a_behind_object_masks_a_front_one():
    """Object 0 is behind, object 1 in front, both over all of an 8 x 8 square whose background is opaque (index 5, 5 % 4 !=
    0) on the left half and transparent (index 8) on the right: on the left NOTHING is written, though object 1 alone would
    show; on the right object 0 shows. Without bg_index the behind bit does nothing."""
    bg = np.full((16, 16), 8, np.uint8)
    bg[:, :4] = 5
    table = [(0, 0, 0, 0 | OB.BEHIND), (0, 0, 1, 1)]
    _, index, _, _ = crafted(table, [1, 2], bg=bg, index=bg.copy())
    assert (index[:8, :4] == 5).all() and (index[:8, 4:8] == 1).all() and (index[8:, :] == bg[8:, :]).all()
    _, same, _, _ = crafted(table, [1, 2], bg="index", index=bg.copy())
    assert same.tobytes() == index.tobytes(), "bg_index may be index_io itself"
    _, free, _, _ = crafted(table, [1, 2], bg=None, index=bg.copy())
    assert (free[:8, :8] == 1).all()
    _, front, _, _ = crafted(table[1:], [1, 2], bg=bg, index=bg.copy())
    assert (front[:8, :8] == 6).all(), "object 1 alone shows over any background"


def test_a_transparent_hole_shows_a_lower_object():
    tiles = np.zeros((2, 8, 8), np.uint8)
    tiles[0] = 1
    tiles[0, 2:4, 2:6] = 0  # a hole in object 0's tile
    tiles[1] = 2
    chr_bytes = V.encode_tiles(tiles, (8, 8), V.F_4BPP_ROWS)[0]
    d = OB.desc_of(n_tiles=2, n_objects=2, n_colors=64, width=16, height=16)
    table = OB.objects_of([(4, 4, 0, 0), (4, 4, 1, 1)])
    start = np.full((16, 16), 63, np.uint8)
    index = both(d, chr_bytes, table, None, None, None, start)[1]
    assert (index[6:8, 6:10] == 6).all() and int((index == 6).sum()) == 8 and int((index == 1).sum()) == 56
    index = both(dict(d, opaque=1), chr_bytes, table, None, None, None, start)[1]
    assert (index[6:8, 6:10] == 0).all() and int((index == 6).sum()) == 0, "opaque: the first covering object wins with its 0"
    index = both(dict(d, n_objects=1), chr_bytes, table[:1], None, None, None, start)[1]
    assert (index[6:8, 6:10] == 63).all(), "with no winner the pixel is not written"


def test_objects_straddling_all_four_edges_and_wholly_off_screen():
    table = [(-3, 5, 0, 0), (13, 5, 0, 0), (5, -5, 0, 0), (5, 12, 0, 0), (-8, 0, 0, 0), (16, 0, 0, 0), (0, -8, 0, 0), (0, 16, 0, 0),
             (-32768, -32768, 0, 0), (32767, 32767, 0, 0)]
    _, index, bad, over = crafted(table, [1])
    assert (bad, over) == (0, 0)
    want = np.full((16, 16), 63, np.uint8)
    want[5:13, 0:5] = want[5:13, 13:16] = want[0:3, 5:13] = want[12:16, 5:13] = 1
    assert index.tolist() == want.tolist()


def test_a_line_with_line_limit_plus_one_objects():
    """Nine objects side by side... on two rows of a 16-wide screen they overlap; every one covers lines 0 to 7: the ninth
    is dropped on each of the eight lines (over 8), and the pixels it alone covers keep their bytes."""
    table = [(0, 0, 0, 0)] * 8 + [(8, 0, 1, 0)]
    _, index, bad, over = crafted(table, [1, 2])
    assert (bad, over) == (0, 8) and (index[:8, :8] == 1).all() and (index[:8, 8:] == 63).all()
    _, index, _, over = crafted(table, [1, 2], line_limit=9)
    assert over == 0 and (index[:8, 8:] == 2).all()
    # x does not matter for the line list: eight objects wholly off screen to the left use the line up
    _, index, _, over = crafted([(-8, 0, 0, 0)] * 8 + [(8, 0, 1, 0)], [1, 2])
    assert over == 8 and (index == 63).all()
    # hidden and bad ones do not
    _, index, bad, over = crafted([(0, 0, 0, OB.HIDDEN)] * 4 + [(0, 0, 7, 0)] * 4 + [(8, 0, 1, 0)], [1, 2])
    assert (bad, over) == (4, 0) and (index[:8, 8:] == 2).all() and (index[:8, :8] == 63).all()


# ---- the eight consequences ------------------------------------------------------------------------------------------------

class TwoFrames:
    """Two cells index planes over ONE tile set: frame 0 builds it, frame 1 extends it; the chr bytes, the two maps with
    their cell bytes, and the two screens (tests/screen.py over tests/vram.py's words, RGBA8 entries, backdrop 0)."""

    def __init__(self, seed, w, h, tile, K, n_sub, flips, fmt=V.F_4BPP_ROWS):
        rng = np.random.default_rng(seed)
        self.w, self.h, self.tile, self.K, self.n_sub, self.fmt = w, h, tile, K, n_sub, fmt
        self.grid = TS.grid(w, h, tile)
        n = self.grid[0] * self.grid[1]
        locals_ = TX.frame_sequence(seed, 2, w, h, tile, kinds=5, step=4, colours=min(K, 1 << V.BPP[fmt]))
        self.cells = [rng.integers(0, n_sub, n, dtype=np.uint8)]
        self.cells.append(np.where(rng.random(n) < 0.2, (self.cells[0] + 1) % n_sub, self.cells[0]).astype(np.uint8))
        tiles0, map0, t0 = TS.model(locals_[0], w, h, tile, 0, flips)
        tiles1, map1, t1, _ = TX.model(tiles0, t0, locals_[1], w, h, tile, 0, flips, 4096)
        self.locals, self.maps, self.tiles, self.count = locals_, [map0, map1], tiles1, t1
        self.chr = V.encode_tiles(tiles1, tile, fmt)[0]
        self.table = rng.integers(0, 256, (n_sub * K, 4), dtype=np.uint8)
        self.pal = self.table.reshape(-1)
        L = V.layout_of(word_bytes=4, tile_bits=20, pal_shift=20, pal_bits=8, flip_x_bit=30, flip_y_bit=31)
        self.sd = S.desc_of(L, tile_w=tile[0], tile_h=tile[1], tile_format=fmt, n_tiles=t1, map_w=self.grid[0], map_h=self.grid[1],
                            n_colors=n_sub * K, sub_size=K, width=w, height=h)
        self.words = [V.encode_map(L, m, self.grid[0], self.grid[1], c)[0] for m, c in zip(self.maps, self.cells)]
        self.screens = [S.draw(self.sd, self.chr, wd, self.pal)[:2] for wd in self.words]
        self.objects, self.D = OB.from_maps(self.maps[0], self.maps[1], self.grid, tile, 65536, self.cells[0], self.cells[1])

    def desc(self, **over):
        d = OB.desc_of(tile_w=self.tile[0], tile_h=self.tile[1], tile_format=self.fmt, n_tiles=self.count, n_objects=max(1, self.D),
                       line_limit=128, n_colors=self.n_sub * self.K, sub_size=self.K, bg_sub_size=self.K, opaque=1, width=self.w, height=self.h)
        d.update(over)
        return d


TWO = [(64, 48, (8, 8), 4, 4, 3), (61, 37, (8, 8), 16, 4, 0), (64, 32, (16, 16), 4, 8, 1), (45, 30, (16, 8), 16, 2, 2)]


@pytest.fixture(scope="module")
def two():
    return {case: TwoFrames(300 + i, *case) for i, case in enumerate(TWO)}


@pytest.mark.parametrize("case", TWO, ids=[f"{c[0]}x{c[1]} of {c[2]}" for c in TWO])
def test_consequences_1_and_2_the_closing_identity_and_what_transparency_keeps(two, case):
    f = two[case]
    assert 0 < f.D <= f.grid[0] * f.grid[1]
    shown, _, most = OB.lines(f.desc(), f.objects, f.D)
    assert most <= 128
    fb, index, bad, over = both(f.desc(), f.chr, f.objects, f.pal, None, f.screens[0][0], f.screens[0][1])
    assert (bad, over) == (0, 0)
    assert index.tobytes() == f.screens[1][1].tobytes() and fb.tobytes() == f.screens[1][0].tobytes()
    assert index.tobytes() != f.screens[0][1].tobytes()
    # (2) opaque 0: differs exactly at the pixels of differing cells whose new value is 0, which keep the first screen's bytes
    t_fb, t_index, _, _ = both(f.desc(opaque=0), f.chr, f.objects, f.pal, None, f.screens[0][0], f.screens[0][1])
    differing = np.zeros(f.grid[0] * f.grid[1], dtype=bool)
    differing[(f.maps[0] != f.maps[1]) | (f.cells[0] != f.cells[1])] = True
    per_pixel = np.repeat(np.repeat(differing.reshape(f.grid[1], f.grid[0]), f.tile[1], axis=0), f.tile[0], axis=1)[:f.h, :f.w]
    zero = per_pixel & (f.locals[1].reshape(f.h, f.w) == 0)
    assert zero.any()
    assert (t_index[zero] == f.screens[0][1][zero]).all() and (t_fb[zero] == f.screens[0][0][zero]).all()
    assert (t_index[~zero] == index[~zero]).all() and (t_fb[~zero] == fb[~zero]).all()
    assert ((t_index != index) | (t_fb != fb).any(axis=2))[~zero].sum() == 0


def test_consequence_3_nothing_to_draw_leaves_the_planes(two):
    f = two[TWO[0]]
    d = f.desc()
    fb0, index0 = f.screens[0]
    for tag, table, count in (("a count of 0", f.objects, 0), ("every object hidden", None, None), ("every object bad", None, None)):
        if table is None:
            table = f.objects.copy()
            if "hidden" in tag:
                table["attr"] |= OB.HIDDEN
            else:
                table["tile"] = f.count
        fb, index, bad, over = both(d, f.chr, table, f.pal, None, fb0, index0, count)
        assert fb.tobytes() == fb0.tobytes() and index.tobytes() == index0.tobytes() and over == 0, tag
        assert bad == (f.D if "bad" in tag else 0), tag


def test_consequence_4_the_line_limit(two):
    f = two[TWO[0]]
    shown, _, most = OB.lines(f.desc(), f.objects, f.D)
    assert 2 <= most < 128
    full = OB.draw(f.desc(), f.chr, f.objects, f.pal, None, *f.screens[0])
    for limit in (most, most + 1, 128):
        got = OB.draw(f.desc(line_limit=limit), f.chr, f.objects, f.pal, None, *f.screens[0])
        assert got[0].tobytes() == full[0].tobytes() and got[1].tobytes() == full[1].tobytes() and got[3] == 0, limit
    for limit in (1, most - 1):
        d = f.desc(line_limit=limit)
        got = both(d, f.chr, f.objects, f.pal, None, *f.screens[0])
        kept, over, _ = OB.lines(d, f.objects, f.D)
        assert got[3] == over > 0 and got[1].tobytes() != full[1].tobytes()
        # the table with every dropped (object, line) pair removed, under a limit that drops nothing
        again = OB.draw(f.desc(), f.chr, f.objects, f.pal, None, *f.screens[0], shown=kept)
        assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes(), limit
        assert (kept.sum(axis=0) <= limit).all() and not (kept & ~shown).any()


def test_consequence_5_a_flip_for_a_tile_stored_mirrored(two):
    for case in (TWO[0], TWO[3]):
        f = two[case]
        base = OB.draw(f.desc(opaque=0), f.chr, f.objects, f.pal, None, *f.screens[0])
        for axis, bit in ((2, OB.FLIP_X), (1, OB.FLIP_Y)):
            mirrored = V.encode_tiles(np.ascontiguousarray(np.flip(f.tiles, axis=axis)), f.tile, f.fmt)[0]
            table = f.objects.copy()
            table["attr"] ^= bit
            got = both(f.desc(opaque=0), mirrored, table, f.pal, None, *f.screens[0])
            assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes(), (case, axis)
            assert OB.draw(f.desc(opaque=0), f.chr, table, f.pal, None, *f.screens[0])[1].tobytes() != base[1].tobytes()


def test_consequence_6_colour_words_or_their_rgba(two):
    f = two[TWO[1]]
    for fmt in (S.BGR555, S.BGR333_MD, S.BGR222):
        words = V.palette_words(f.table, fmt)
        rgba = SCREEN.palette_rgba(words, fmt)
        a = both(f.desc(pal_format=fmt), f.chr, f.objects, words, None, *f.screens[0])
        b = OB.draw(f.desc(pal_format=S.RGBA8), f.chr, f.objects, rgba.reshape(-1), None, *f.screens[0])
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), fmt


def test_consequence_7_objects_that_share_no_pixel_may_be_permuted(two):
    """from_maps gives one object a cell: no two share a pixel."""
    rng = np.random.default_rng(7)
    for case in TWO[:2]:
        f = two[case]
        base = OB.draw(f.desc(opaque=0), f.chr, f.objects, f.pal, None, *f.screens[0])
        for _ in range(3):
            table = f.objects[rng.permutation(f.D)]
            got = both(f.desc(opaque=0), f.chr, table, f.pal, None, *f.screens[0])
            assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes()
    # and objects that do share pixels may not
    d = OB.desc_of(n_tiles=2, n_objects=2, n_colors=64, width=16, height=16)
    chr_bytes = solid_tiles([1, 2])[1]
    start = np.full((16, 16), 63, np.uint8)
    a = OB.draw(d, chr_bytes, OB.objects_of([(0, 0, 0, 0), (4, 4, 1, 0)]), None, None, None, start)[1]
    b = OB.draw(d, chr_bytes, OB.objects_of([(4, 4, 1, 0), (0, 0, 0, 0)]), None, None, None, start)[1]
    assert a.tobytes() != b.tobytes()


def test_consequence_8_unpack_inverts_pack_on_fitting_visible_objects(objects):
    rng = np.random.default_rng(8)
    for fmt, edges in ((OB.OAM_NES, NES_EDGES), (OB.OAM_GB, GB_EDGES)):
        o = np.zeros(300, OB.OBJECT)
        for field in ("x", "y", "tile"):
            o[field] = rng.integers(edges[field][0], edges[field][1] + 1, 300)
        o["attr"] = rng.integers(0, edges["p"][1] + 1, 300) | rng.integers(0, 8, 300) << 8
        assert OB.fits(fmt, o).all()
        packed, bad = objects.pack(fmt, o)
        assert bad == 0 and objects.unpack(fmt, packed).tobytes() == o.tobytes() == OB.unpack(fmt, OB.pack(fmt, o)[0]).tobytes()
