"""The machine fit without a GPU: the four calls are declared in addons/include/par_machine_fit.h, an add-on header that
includes no header of the project, exported by a library of their own and wrapped by the machine_fit module, whose table
is none of abi.py's and which the package does not import; the header compiles as pedantic C11 alone, twice and beside the
other headers; the enum is par_screen_palette_format's in value; every PAR_ERR_INVALID_ARG of both calls comes back before
any device work and with nothing written, each rule on its own; par_machine_fit_work_bytes is the header's formula;
par_machine_round is the loop's rounding on every byte at every depth and survives the colour words; the two-candidate move
the device computes is the brute-force move; the vectorised model the GPU tests lean on (machine_fit.model) equals the
loops in Python integers on random frames and on crafted frames worked out by hand; the consequences the contract states
hold on the models; and the figures of the graybox frame that README and DESIGN quote are the model's."""
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

import cells as CL
import cells_fit as CF
import headers
import machine_fit as MF
import quantize as Q
import screen as S
import tileset as TS
import vram as V

ROOT = headers.ROOT
ADDON_INCLUDE = os.path.join(ROOT, "addons", "include")
HEADER = os.path.join(ADDON_INCLUDE, "par_machine_fit.h")
ERR_INVALID_ARG, ERR_NO_DEVICE = 1, 2
SYMBOLS = ("par_machine_round", "par_machine_fit_work_bytes", "par_machine_fit_device", "par_machine_fit_host")


FIT = importlib.import_module("pixel-art-raytracer_amd.machine_fit")  # (without the add-on's binding nothing here can run)


@pytest.fixture(scope="module")
def fit():
    return FIT


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
            "size_t par_machine_round(const uint8_t* palette, int n, int depth, uint8_t* out);",
            "size_t par_machine_fit_work_bytes(int width, int height, int cell_w, int cell_h);",
            "int par_machine_fit_device(void* stream, const uint8_t* fb, int width, int height, int cell_w, int cell_h, "
            "const uint8_t* palette, int n_colors, int n_sub, int sub_size, int rounds, int depth, int backdrop, void* work, "
            "uint8_t* table_out, uint32_t* seeds_out, uint64_t* errors_out);",
            "int par_machine_fit_host(int device, const uint8_t* fb, int width, int height, int cell_w, int cell_h, "
            "const uint8_t* palette, int n_colors, int n_sub, int sub_size, int rounds, int depth, int backdrop, "
            "uint8_t* table_out, uint32_t* seeds_out, uint64_t* errors_out);",
            "enum par_machine_depth { PAR_MACHINE_BGR555 = 0, PAR_MACHINE_BGR333_MD = 1, PAR_MACHINE_BGR222 = 2, PAR_MACHINE_RGBA8 = 3 };"):
        assert proto in code, proto
    assert tuple(name for _, name, _ in header_prototypes()) == SYMBOLS
    assert re.findall(r"#include\s+([<\"][^>\"]+[>\"])", header_code()) == ["<stddef.h>", "<stdint.h>"]
    for define, value in (("PAR_MACHINE_FIT_MAX_CELLS", r"\(1 << 20\)"), ("PAR_MACHINE_FIT_MAX_SUB_SIZE", "16"),
                          ("PAR_MACHINE_FIT_MAX_ROUNDS", "32")):
        assert re.search(r"#define %s %s" % (define, value), code), define
    text = " ".join(header_text().replace("\n *", " ").split())  # the comment as running text
    for word in ("NES's fixed master palette", "caller-chosen backdrop colour", "dither awareness", "budget of distinct colours",
                 "row blocks and several frames", "5 + S + 4 * R launches", "180224 + 25 * cells", "lowest l among equals",
                 "lowest c among equals", "no term in pixels", "0xFFFFFFFF", "never rises", "ONE entry", "l << 3 | l >> 2",
                 "l << 5 | l << 2 | l >> 1", "l * 0x55", "w(l) >> (8 - b) == l"):
        assert word in text, word
    assert (MF.HEAD_BYTES, MF.BYTES_PER_CELL, MF.launches(8, 6, 1)) == (180224, 25, 5 + 8 + 24 + 1 + 1)


def test_the_enum_is_the_screens_palette_format(fit):
    screen_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ADDON_INCLUDE, "par_screen.h")).read(), flags=re.S)
    body = re.search(r"enum par_screen_palette_format\s*\{([^}]*)\}", screen_h).group(1)
    theirs = {name.replace("PAR_SCREEN_PAL_", "").replace("PAR_SCREEN_", ""): int(value) for name, value in re.findall(r"(PAR_\w+)\s*=\s*(\d+)", body)}
    body = re.search(r"enum par_machine_depth\s*\{([^}]*)\}", header_code()).group(1)
    ours = {name.replace("PAR_MACHINE_", ""): int(value) for name, value in re.findall(r"(PAR_\w+)\s*=\s*(\d+)", body)}
    assert ours == {"BGR555": 0, "BGR333_MD": 1, "BGR222": 2, "RGBA8": 3} and sorted(theirs.values()) == [0, 1, 2, 3]
    assert ours == theirs, (ours, theirs)
    D = fit.Depth
    assert (D.BGR555, D.BGR333_MD, D.BGR222, D.RGBA8) == (S.BGR555, S.BGR333_MD, S.BGR222, S.RGBA8) == tuple(MF.DEPTHS)
    assert D.BITS == MF.BITS == (5, 3, 2, 8)


def test_the_table_is_the_headers_and_no_core_table(par, fit):
    protos = header_prototypes()
    assert SYMBOLS == tuple(fit.ABI_MACHINE_FIT) == fit.ABI_MACHINE_FIT_SYMBOLS
    L = fit.lib()
    for proto in protos:
        ret, name, _ = proto
        want_restype, want = headers.want_signature(proto)
        restype, argtypes = headers.signature(fit.ABI_MACHINE_FIT[name])
        assert list(argtypes) == want and restype is want_restype, name
        fn = getattr(L, name)
        assert list(fn.argtypes) == want and fn.restype is want_restype, name
    assert not any(table is fit.ABI_MACHINE_FIT for table in par.ABI_HEADERS.values())
    for name in SYMBOLS:
        assert not any(name in table for table in (*par.ABI_HEADERS.values(), par.ABI_DEBUG_HOOKS)), name
        assert not hasattr(par.lib(), name), f"{name} is exported by the core library"
    for h in os.listdir(headers.INCLUDE):
        assert "par_machine_" not in headers.without_comments(h), h
    for fn in ("machine_round", "machine_fit_work_bytes", "machine_fit", "machine_fit_host"):
        assert callable(getattr(fit, fn)) and (not hasattr(par, fn) or inspect.ismodule(getattr(par, fn))), fn
    assert (fit.MAX_CELLS, fit.MAX_SUB_SIZE, fit.MAX_ROUNDS) == (CF.MAX_CELLS, CF.MAX_SUB_SIZE, CF.MAX_ROUNDS) == (1 << 20, 16, 32)


def exported(path):
    nm = shutil.which("nm")
    assert nm is not None, "no nm to list the library's symbols"
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(f[2] for f in (line.split() for line in out.splitlines()) if len(f) == 3 and f[1] == "T" and f[2].startswith("par_"))


def test_the_add_on_exports_exactly_its_table_and_the_plain_fit_keeps_its_three(fit):
    assert exported(fit.LIB_PATH) == sorted(SYMBOLS)
    plain = importlib.import_module("pixel-art-raytracer_amd.cells_fit")
    assert exported(plain.LIB_PATH) == sorted(["par_cells_fit_work_bytes", "par_cells_fit_device", "par_cells_fit_host"])


def test_importing_the_package_does_not_load_the_module():
    code = ("import importlib, json, sys\npar = importlib.import_module('pixel-art-raytracer_amd')\npar.lib()\n"
            "print(json.dumps(sorted(m for m in sys.modules if m.startswith('pixel-art-raytracer_amd.'))))\n"
            "fit = importlib.import_module('pixel-art-raytracer_amd.machine_fit')\n"
            "print(json.dumps([fit.machine_fit_work_bytes(20, 9, (8, 8)), fit.lib() is not par.lib()]))")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().splitlines()
    assert json.loads(lines[-2]) == ["pixel-art-raytracer_amd.abi", "pixel-art-raytracer_amd.types"]
    assert json.loads(lines[-1]) == [180224 + 25 * 6, True]


def test_a_missing_library_is_an_import_error_in_the_cores_words(par, fit, monkeypatch, tmp_path):
    missing = str(tmp_path / "lib" / "libmachine_fit.so")
    monkeypatch.setattr(fit, "LIB_PATH", missing)
    monkeypatch.setattr(fit, "_lib", None)
    with pytest.raises(ImportError) as e:
        fit.lib()
    assert str(e.value) == (f"{missing} is missing: build it with `make -C pixel-art-raytracer_amd/csrc` "
                            "(or __graft_entry__.build()). There is no CPU fallback.")
    assert fit._lib is None


def test_the_loaded_library_carries_its_table_and_no_other(par, fit):
    L = fit.lib()
    assert L is fit.lib() and L is not par.lib()
    for symbol, sig in fit.ABI_MACHINE_FIT.items():
        restype, argtypes = sig if type(sig) is tuple else (C.c_int, sig)
        fn = getattr(L, symbol)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), symbol
    for other, table in (("tileset_reduce", "ABI_TILESET_REDUCE"), ("cells_fit", "ABI_CELLS_FIT"), ("vram", "ABI_VRAM"), ("screen", "ABI_SCREEN")):
        module = importlib.import_module("pixel-art-raytracer_amd." + other)
        assert not any(hasattr(L, symbol) for symbol in getattr(module, table)), other
        assert not any(hasattr(module.lib(), symbol) for symbol in SYMBOLS), other


BODY = r"""
#include <stdio.h>
int main(void) {
    unsigned char fb[4 * 64] = {0}, palette[8] = {100, 10, 190, 7, 0, 0, 0, 0}, table[8] = {9, 9, 9, 9, 9, 9, 9, 9}, out[8] = {0};
    uint32_t seeds[2] = {7, 7};
    uint64_t errors[1] = {5}, work[1 + (180224 + 25) / 8];
    int rc = par_machine_fit_device(NULL, fb, 8, 8, 8, 8, palette, 2, 2, 1, 33, PAR_MACHINE_BGR555, 0, work, table, seeds, errors);
    unsigned long n = (unsigned long)par_machine_round(palette, 2, PAR_MACHINE_BGR333_MD, out);
    printf("%d %d %u %u %lu %lu %lu %u %u %u %u %d\n", PAR_MACHINE_FIT_MAX_CELLS + PAR_MACHINE_FIT_MAX_SUB_SIZE + PAR_MACHINE_FIT_MAX_ROUNDS, rc,
           (unsigned)table[0], (unsigned)seeds[0], (unsigned long)par_machine_fit_work_bytes(8, 8, 8, 8),
           (unsigned long)par_machine_fit_work_bytes(8, 8, 8, 12), n, (unsigned)out[0], (unsigned)out[1], (unsigned)out[2], (unsigned)out[3],
           (int)PAR_MACHINE_RGBA8);
    return (int)errors[0] - 5;
}
"""
CORE = ["par_raytracer.h", "par_cells.h", "par_tileset.h", "par_tileset_extend.h"]
ADDONS = ["par_tileset_reduce.h", "par_cells_fit.h", "par_vram.h", "par_screen.h"]


@pytest.mark.parametrize("includes", [["par_machine_fit.h"], ["par_machine_fit.h"] * 2, CORE + ADDONS + ["par_machine_fit.h"],
                                      ["par_machine_fit.h"] + ADDONS + CORE], ids=["alone", "twice", "behind the others", "before the others"])
def test_header_is_pedantic_c11(tmp_path, includes):
    src, exe = tmp_path / "fit.c", tmp_path / "fit"
    src.write_text("".join(f'#include "{h}"\n' for h in includes) + BODY)
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", ADDON_INCLUDE, "-I", headers.INCLUDE,
                        str(src), "-o", str(exe), "-L", headers.LIB_DIR, "-lpar_machine_fit", f"-Wl,-rpath,{headers.LIB_DIR}"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == [str((1 << 20) + 48), "1", "9", "7", str(180224 + 25), "0", "8", "109", "0", "182",
                                                          "7", "3"], (out.stdout, out.stderr)


# ---- par_machine_fit_work_bytes ------------------------------------------------------------------------------------------

def test_work_bytes_is_the_headers_formula_and_keeps_its_bound(fit):
    for width, height in ((1, 1), (8, 8), (9, 9), (61, 37), (480, 320), (4096, 4096), (8192, 8192), (1 << 23, 1), (1, 1 << 23)):
        for cell in CL.CELLS:
            cells = -(-width // cell[0]) * -(-height // cell[1])
            got = fit.machine_fit_work_bytes(width, height, cell)
            assert got == MF.work_bytes(width, height, cell) == 180224 + 25 * cells, (width, height, cell)
            assert got - 180224 <= 25 * cells, "at most 25 bytes a cell and a constant"
    assert fit.machine_fit_work_bytes(4096, 4096, (8, 8)) < 4096 * 4096, "no term in pixels: under a byte a pixel at 8 x 8"
    for width, height, cell in ((0, 8, (8, 8)), (8, 0, (8, 8)), (-1, 8, (8, 8)), (8, -1, (8, 8)), (8, 8, (4, 8)), (8, 8, (8, 12)),
                                (8, 8, (32, 8)), (8, 8, (8, 0)), (8, 8, (-8, 8)), (8193, 8192, (8, 8)), (8192, 8193, (8, 8)),
                                ((1 << 31) - 1, (1 << 31) - 1, (16, 16)), ((1 << 23) + 1, 1, (8, 8)), (-(1 << 31), -(1 << 31), (8, 8))):
        assert fit.machine_fit_work_bytes(width, height, cell) == 0 == MF.work_bytes(width, height, cell), (width, height, cell)
    assert fit.lib().par_machine_fit_work_bytes.restype is C.c_size_t


# ---- argument errors: no device needed, nothing written -----------------------------------------------------------

BAD = [
    ("null fb", dict(fb=None)),
    ("null palette", dict(palette=None)),
    ("null table_out", dict(table_out=None)),
    ("width 0", dict(width=0)),
    ("width -1", dict(width=-1)),
    ("height 0", dict(height=0)),
    ("height -1", dict(height=-1)),
    ("2^20 + 1 cells in a row", dict(width=8 * (1 << 20) + 1, height=1)),
    ("2^20 + 1 cells in a column", dict(width=1, height=8 * (1 << 20) + 1)),
    ("2^20 + 2^10 cells", dict(width=8 * 1025, height=8 * 1024)),
    ("2^31 - 1 both ways", dict(width=(1 << 31) - 1, height=(1 << 31) - 1)),
    ("cell_w 4", dict(cell=(4, 8))),
    ("cell_w 12", dict(cell=(12, 8))),
    ("cell_w 32", dict(cell=(32, 8))),
    ("cell_w 0", dict(cell=(0, 8))),
    ("cell_h 4", dict(cell=(8, 4))),
    ("cell_h 32", dict(cell=(8, 32))),
    ("cell_h 0", dict(cell=(8, 0))),
    ("cell_h negative", dict(cell=(8, -8))),
    ("sub_size 0", dict(sub_size=0)),
    ("sub_size -1", dict(sub_size=-1)),
    ("sub_size 17", dict(sub_size=17, n_sub=1, n_colors=17)),
    ("n_colors below sub_size", dict(n_colors=2)),
    ("n_colors 0", dict(n_colors=0, sub_size=1)),
    ("n_colors 257", dict(n_colors=257)),
    ("n_sub 0", dict(n_sub=0)),
    ("n_sub -1", dict(n_sub=-1)),
    ("S * K 257", dict(n_sub=257, sub_size=1)),
    ("S * K 258", dict(n_sub=86)),
    ("S * K wraps 32 bits", dict(n_sub=1 << 30, sub_size=4, n_colors=4)),
    ("rounds -1", dict(rounds=-1)),
    ("rounds 33", dict(rounds=33)),
    ("depth -1", dict(depth=-1)),
    ("depth 4", dict(depth=4)),
    ("depth 5 (bits, not a value)", dict(depth=5)),
    ("depth 2^31 - 1", dict(depth=(1 << 31) - 1)),
    ("backdrop -1", dict(backdrop=-1)),
    ("backdrop 2", dict(backdrop=2)),
    ("backdrop 256", dict(backdrop=256)),
    ("backdrop with sub_size 1", dict(backdrop=1, sub_size=1)),
]
BAD_DEVICE = BAD + [("null work", dict(work=None)), ("work off its 8 bytes", dict(work_shift=4))]


def raw_call(fit, T, which, over):
    """One call of the raw symbol on host dummies: (status, whether any buffer changed). The frame is 16 x 8 under 8 x 8
    cells, the master has 6 entries, the table 2 x 3, there is one round, at BGR555 without the backdrop."""
    L = fit.lib()
    bufs = {"fb": np.full(4 * 128, 0xA5, np.uint8), "palette": np.full(4 * 6, 0x77, np.uint8), "table_out": np.full(4 * 256, 0xC3, np.uint8),
            "seeds_out": np.full(256, 0x11111111, np.uint32), "errors_out": np.full(40, 0x4B, np.uint64),
            "work": np.full((180224 + 25 * 2) // 8 + 2, 0x5A, np.uint64)}
    before = {k: v.copy() for k, v in bufs.items()}
    arg = dict(width=16, height=8, cell=(8, 8), n_colors=6, n_sub=2, sub_size=3, rounds=1, depth=0, backdrop=0, **bufs)
    arg.update({k: v for k, v in over.items() if k != "work_shift"})
    ptr = T.ptr
    work = ptr(arg["work"])
    if "work_shift" in over:
        work = C.c_void_p(arg["work"].ctypes.data + over["work_shift"])
    head = (ptr(arg["fb"]), arg["width"], arg["height"], arg["cell"][0], arg["cell"][1], ptr(arg["palette"]), arg["n_colors"],
            arg["n_sub"], arg["sub_size"], arg["rounds"], arg["depth"], arg["backdrop"])
    tail = (ptr(arg["table_out"]), ptr(arg["seeds_out"]), ptr(arg["errors_out"]))
    if which == "device":
        rc = L.par_machine_fit_device(None, *head, work, *tail)
    else:
        rc = L.par_machine_fit_host(-1, *head, *tail)
    return rc, any(bufs[k].tobytes() != before[k].tobytes() for k in bufs)


@pytest.mark.parametrize("which,bad", [("device", BAD_DEVICE), ("host", BAD)])
def test_invalid_arguments_need_no_device_and_write_nothing(fit, T, which, bad):
    assert len({tag for tag, _ in bad}) == len(bad)
    for tag, over in bad:
        rc, changed = raw_call(fit, T, which, over)
        assert rc == ERR_INVALID_ARG, f"{which}: {tag}: status {rc}"
        assert not changed, f"{which}: {tag}: something was written"


def test_what_the_rules_admit_is_not_refused(par, fit, T):
    """The host form on the arguments next to the refused ones: any status but PAR_ERR_INVALID_ARG, which without a GPU is
    PAR_ERR_NO_DEVICE."""
    want = 0 if par.device_count() > 0 else ERR_NO_DEVICE
    for over in (dict(), dict(seeds_out=None), dict(errors_out=None), dict(cell=(16, 16)), dict(sub_size=1, n_colors=1), dict(sub_size=6),
                 dict(n_sub=1), dict(n_sub=85), dict(n_sub=256, sub_size=1), dict(rounds=0), dict(rounds=32), dict(width=15, height=7),
                 dict(depth=1), dict(depth=2), dict(depth=3), dict(backdrop=1), dict(backdrop=1, sub_size=2), dict(backdrop=1, depth=3)):
        rc, _ = raw_call(fit, T, "host", over)
        assert rc == want, (over, rc)


def test_binding_raises_and_hands_its_arguments_over_in_the_headers_order(par, fit, monkeypatch):
    with pytest.raises(par.ParError) as e:
        fit.machine_fit(0x1000, 16, 8, (8, 8), 0x2000, 6, 2, 3, 1, 4, 0, 0x3000, 0x4000)
    assert e.value.status == ERR_INVALID_ARG and str(e.value) == "PAR_ERR_INVALID_ARG: par_machine_fit_device"
    with pytest.raises(par.ParError) as e:
        fit.machine_fit_host(np.zeros((128, 4), np.uint8), 16, 8, (8, 8), np.zeros((6, 4), np.uint8), 2, 1, backdrop=1)
    assert e.value.status == ERR_INVALID_ARG and str(e.value) == "PAR_ERR_INVALID_ARG: par_machine_fit_host"
    with pytest.raises(ValueError, match="machine_fit_host: fb holds"):
        fit.machine_fit_host(np.zeros((127, 4), np.uint8), 16, 8, (8, 8), np.zeros((6, 4), np.uint8), 2, 3)
    with pytest.raises(ValueError, match="machine_fit_host: palette holds"):
        fit.machine_fit_host(np.zeros((128, 4), np.uint8), 16, 8, (8, 8), np.zeros(7, np.uint8), 2, 3)
    for bad in (dict(palette=np.zeros((0, 4), np.uint8), depth=0), dict(palette=np.zeros((257, 4), np.uint8), depth=0),
                dict(palette=np.zeros((4, 4), np.uint8), depth=4), dict(palette=np.zeros((4, 4), np.uint8), depth=-1)):
        with pytest.raises(ValueError, match="machine_round"):
            fit.machine_round(**bad)
    from test_binding_cpu import A, StandIn
    stand_in = StandIn(returns={"par_machine_fit_work_bytes": 777})
    monkeypatch.setattr(fit, "lib", lambda: stand_in)
    assert fit.machine_fit_work_bytes(90, 12, (8, 16)) == 777
    assert stand_in.calls.pop() == ("par_machine_fit_work_bytes", [90, 12, 8, 16])
    fit.machine_fit(0x1000, 61, 37, (8, 16), 0x2000, 33, 5, 4, 3, 2, 1, 0x3000, 0x4000, seeds_out=0x5000, errors_out=0x6000, stream=0x7000)
    assert stand_in.calls.pop() == ("par_machine_fit_device", [0x7000, 0x1000, 61, 37, 8, 16, 0x2000, 33, 5, 4, 3, 2, 1, 0x3000, 0x4000,
                                                               0x5000, 0x6000])
    fb = np.arange(4 * 20 * 9, dtype=np.uint32).astype(np.uint8).reshape(-1, 4)
    palette = np.arange(28, dtype=np.uint8).reshape(7, 4)
    out = fit.machine_fit_host(fb, 20, 9, (8, 16), palette, 3, 2, rounds=4, depth=1, backdrop=1, device=2)
    name, args = stand_in.calls.pop()
    assert name == "par_machine_fit_host" and list(out) == ["table", "seeds", "errors"]
    assert args[:6] == [2, A(fb), 20, 9, 8, 16] and args[6:13] == [A(palette), 7, 3, 2, 4, 1, 1]
    assert args[13:] == [A(out["table"]), A(out["seeds"]), A(out["errors"])]


# ---- the lattice -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", MF.DEPTHS, ids=S.PAL_NAMES)
def test_round_is_the_loops_on_every_byte_and_survives_the_colour_words(fit, depth):
    vram = importlib.import_module("pixel-art-raytracer_amd.vram")
    screen = importlib.import_module("pixel-art-raytracer_amd.screen")
    loop = MF.round_loop(depth)
    assert MF.round_values(depth).tolist() == loop and sorted(set(loop)) == MF.lattice(depth).tolist()
    for l, w in enumerate(MF.lattice(depth).tolist()):
        assert w >> (8 - MF.BITS[depth]) == l and loop[w] == w, "a level widens to a value that narrows to it, and is its own rounding"
    # every byte in every channel, alpha anything: 256 entries (x, 255 - x, x ^ 0x5A, x + 1)
    x = np.arange(256)
    palette = np.stack([x, 255 - x, x ^ 0x5A, (x + 1) & 255], axis=1).astype(np.uint8)
    got = fit.machine_round(palette, depth)
    want = np.stack([np.array(loop)[palette[:, 0]], np.array(loop)[palette[:, 1]], np.array(loop)[palette[:, 2]], palette[:, 3]], axis=1)
    assert got.tobytes() == want.astype(np.uint8).tobytes()
    assert got.tobytes() == np.ascontiguousarray(MF.round_palette(palette.view(Q_COLOR()).reshape(-1), depth)).tobytes()
    assert fit.machine_round(got, depth).tobytes() == got.tobytes(), "rounding twice is rounding once"
    if depth != MF.RGBA8:
        back = screen.palette_rgba(vram.palette_words(got, depth), depth)
        assert back[:, :3].tobytes() == got[:, :3].tobytes() and (back[:, 3] == 255).all(), "stored without loss"
        assert S.palette_rgba(V.palette_words(got, depth), depth)[:, :3].tobytes() == got[:, :3].tobytes()
    # the ties: half way between two levels goes down
    for a, b in zip(MF.lattice(depth).tolist(), MF.lattice(depth).tolist()[1:]):
        if (a + b) % 2 == 0:
            assert loop[(a + b) // 2] == a
    # in place, one entry, and the refusals of the raw symbol
    one = np.array([200, 100, 50, 9], np.uint8)
    assert fit.lib().par_machine_round(one.ctypes.data, 1, depth, one.ctypes.data) == 4 and one.tolist() == [loop[200], loop[100], loop[50], 9]
    keep = np.full(8, 0x3C, np.uint8)
    for args in ((None, 1, depth, keep.ctypes.data), (one.ctypes.data, 1, depth, None), (one.ctypes.data, 0, depth, keep.ctypes.data),
                 (one.ctypes.data, 257, depth, keep.ctypes.data), (one.ctypes.data, 1, 4, keep.ctypes.data), (one.ctypes.data, 1, -1, keep.ctypes.data)):
        assert fit.lib().par_machine_round(*args) == 0 and (keep == 0x3C).all()


def Q_COLOR():
    return importlib.import_module("pixel-art-raytracer_amd.types").COLOR


# ---- the move --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", MF.DEPTHS, ids=S.PAL_NAMES)
def test_the_two_candidate_move_is_the_brute_force_move(depth):
    rng = np.random.default_rng(40 + depth)
    w = MF.lattice(depth).tolist()

    def same(values, tag):
        values = [int(v) for v in values]
        brute = MF.move_loop(values, depth)
        assert MF.move_two_candidates(values, depth) == brute == MF.move(np.bincount(values, minlength=256), depth), (tag, values[:12])
        return brute

    for trial in range(400):
        n = int(rng.integers(1, 60))
        kind = trial % 4
        if kind == 0:
            values = rng.integers(0, 256, n)
        elif kind == 1:
            values = np.clip(int(rng.integers(0, 256)) + rng.integers(-25, 26, n), 0, 255)
        elif kind == 2:
            values = rng.choice(w, n)  # on the lattice
        else:
            values = np.where(rng.random(n) < 0.5, int(rng.integers(0, 256)), int(rng.integers(0, 256)))  # two values, many ties
        same(values, f"random {trial}")
    for l, a in enumerate(w):
        assert same([a] * 7, "all pixels at one lattice value") == a
        assert same([a], "one pixel") == a
        assert same([a, a, min(255, a + 1)], "a median exactly on a lattice value") == a
        if l + 1 < len(w):
            b = w[l + 1]
            assert same([a, b], "an exact tie between a and b") == a
            assert same([a, a, b, b], "an exact tie between a and b") == a
            assert same([a, b, b], "b wins") == b
            if b - a >= 2:
                mid = (a + b) // 2
                assert same([mid], "one pixel inside") == (a if mid - a <= b - mid else b)
                assert same([a + 1, b - 1], "a tie from inside") == a
    assert same([255] * 5, "a median at 255") == 255 and same([0, 255, 255], "a median at 255") == 255
    assert same([254, 254, 255], "the top interval") == (255 if depth != MF.RGBA8 else 254)
    for x in range(256):
        assert same([x], "one pixel") == MF.round_loop(depth)[x], "one pixel moves to its rounding"


# ---- the model the GPU tests compare with --------------------------------------------------------------------------

@pytest.mark.parametrize("cell", CL.CELLS)
def test_model_equals_the_loop_on_random_frames(T, cell):
    rng = np.random.default_rng(100 + cell[0] + 2 * cell[1])
    moved, turn = 0, 0
    for (width, height), (n_sub, sub_size), n_colors, rounds in (((19, 11), (3, 2), 5, 2), ((17, 18), (4, 3), 9, 1), ((24, 16), (2, 5), 5, 0),
                                                                 ((9, 33), (5, 2), 7, 3)):
        palette = Q.random_colors(T, rng, n_colors)
        for noise in (0, 30):
            for backdrop in (0, 1):
                depth = turn % 4
                turn += 1
                fb = CF.random_frame(T, rng, width, height, colours=palette if noise else None, noise=noise)
                got = MF.model(fb, width, height, cell, palette, n_sub, sub_size, rounds, depth, backdrop)
                CF.same(got, MF.model_loop(fb, width, height, cell, palette, n_sub, sub_size, rounds, depth, backdrop),
                        f"{cell} {width}x{height} S {n_sub} K {sub_size} depth {depth} backdrop {backdrop}")
                assert len(got[0]) == n_sub * sub_size and got[1][0] == CF.NO_SEED and len(got[2]) == rounds + 1
                moved += int(rounds > 0 and got[2][-1] < got[2][0])
    assert moved >= 6


# ---- crafted frames, worked out by hand ----------------------------------------------------------------------------

BLACK, RED, GREEN, BLUE = (0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255)
CRAFTED = ("a backdrop that is not any cell's first wish", "a pooled entry that no pixel takes", "master entries that become equal after rounding",
           "the pooled entry moves to the pooled optimum")


def crafted(T):
    """name -> ((fb, width, height, cell, palette, n_sub, sub_size, rounds, depth, backdrop), (table, seeds, errors)), the
    results by hand. The master's alphas are 200 + index, so a table entry shows where it came from."""
    def master(*rows):
        return CF.colours(T, [(*row, 200 + i) for i, row in enumerate(rows)])

    def result(entries, seeds, errors):
        return CF.colours(T, entries), np.array(seeds, dtype=np.uint32), np.array(errors, dtype=np.uint64)

    out = {}
    # Three cells, RGBA8 so that nothing rounds. Cell 0: 33 red, 31 black. Cell 1: 33 green, 31 black. Cell 2: 33 blue, 31 black.
    # H: black 93, red 33, green 33, blue 33: b0 is black though every cell wants its own colour first. K = 2: W_c is (black,
    # the cell's colour), own 0 everywhere; A_0 is (black, red): best is 0, 33 * 255, 33 * 255: cell 1 is the seed.
    pal = master(BLACK, RED, GREEN, BLUE)
    fb = CF.painted(T, 24, 8, (8, 8), [[RED] * 33 + [BLACK] * 31, [GREEN] * 33 + [BLACK] * 31, [BLUE] * 33 + [BLACK] * 31])
    out[CRAFTED[0]] = ((fb, 24, 8, (8, 8), pal, 2, 2, 0, MF.RGBA8, 1),
                       result([(*BLACK, 200), (*RED, 201), (*BLACK, 200), (*GREEN, 202)], [CF.NO_SEED, 1], [33 * 255]))
    # Two equal cells at RGBA8, S = 2, K = 4. A cell: 12 each of A (60, 0, 0), B (0, 60, 0), C (0, 0, 60), which are 80 from
    # p = (20, 20, 20) and 90 from their own q; 10 of (100, 0, 0) and 9 each of (0, 100, 0), (0, 0, 100), 50 from their q.
    # H: p 72, the qs 20, 18, 18: b0 is p, every list is (p, qA, qB, qC), nothing is gained and cell 0 is the seed. Error
    # 2 * (36 * 80 + 28 * 50). Round 1: both cells take sub-palette 0; p gets A, B, C and moves to the medians (0, 0, 0) (24 of
    # 36 values a channel are 0), the qs move onto their 100s. Error 2 * 36 * 40: A, B, C are 60 from p now and 40 from a q.
    # Round 2: NO pixel takes the pooled entry, at either position: it keeps (0, 0, 0, 255). qA has 12 x 60 and 10 x 100,
    # element 10 of 22 is 60; qB and qC have 12 and 9, element 10 of 21 is 60. Error 2 * 28 * 40. Sub-palette 1 never
    # gets a pixel: its qs keep their master bytes, its position 0 follows the pool.
    pal = master((20, 20, 20), (150, 0, 0), (0, 150, 0), (0, 0, 150))
    one = [(60, 0, 0), (0, 60, 0), (0, 0, 60)] * 12 + [(100, 0, 0)] * 10 + [(0, 100, 0)] * 9 + [(0, 0, 100)] * 9
    fb = CF.painted(T, 16, 8, (8, 8), [one, one])
    out[CRAFTED[1]] = ((fb, 16, 8, (8, 8), pal, 2, 4, 2, MF.RGBA8, 1),
                       result([(0, 0, 0, 255), (60, 0, 0, 255), (0, 60, 0, 255), (0, 0, 60, 255),
                               (0, 0, 0, 255), (150, 0, 0, 201), (0, 150, 0, 202), (0, 0, 150, 203)], [CF.NO_SEED, 0],
                              [2 * (36 * 80 + 28 * 50), 2 * 36 * 40, 2 * 28 * 40]))
    # BGR222: (80, 0, 0) and (90, 0, 0) both round to (85, 0, 0), (250, 0, 0) to (255, 0, 0). One cell of 40 pixels of
    # (88, 0, 0) and 24 of (250, 0, 0): every (88, 0, 0) goes to the LOWER of the equal entries, index 0, so index 1 has no
    # pixel: K = 2 gives (entry 0, entry 2), error 40 * 3 + 24 * 5.
    pal = master((80, 0, 0), (90, 0, 0), (250, 0, 0))
    fb = CF.painted(T, 8, 8, (8, 8), [[(88, 0, 0)] * 40 + [(250, 0, 0)] * 24])
    out[CRAFTED[2]] = ((fb, 8, 8, (8, 8), pal, 1, 2, 0, MF.BGR222, 0), result([(85, 0, 0, 200), (255, 0, 0, 202)], [CF.NO_SEED], [40 * 3 + 24 * 5]))
    # BGR333_MD with the backdrop, two cells: cell 0 is 64 x (40, 0, 0), cell 1 is 64 x (100, 0, 0); the master (36, 0, 0),
    # (109, 0, 0) is on the lattice already. H ties at 64: b0 is entry 0. K = 2, S = 2: every list is (0, 1), the seed is cell
    # 0. Round: both cells take sub-palette 0; cell 0's pixels entry 0 (4 away), cell 1's entry 1 (9 away). The pooled entry
    # has 64 pixels at 40: 36 stays (4 against 33). Entry 1 has 64 at 100: 109 (9) against 73 (27): stays. Error 64 * 13 both.
    pal = master((36, 0, 0), (109, 0, 0))
    fb = CF.painted(T, 16, 8, (8, 8), [[(40, 0, 0)], [(100, 0, 0)]])
    out[CRAFTED[3]] = ((fb, 16, 8, (8, 8), pal, 2, 2, 1, MF.BGR333_MD, 1),
                       result([(36, 0, 0, 255), (109, 0, 0, 255), (36, 0, 0, 255), (109, 0, 0, 201)], [CF.NO_SEED, 0], [64 * 13, 64 * 13]))
    return out


@pytest.mark.parametrize("name", CRAFTED)
def test_crafted_frames(T, name):
    (fb, width, height, cell, palette, n_sub, sub_size, rounds, depth, backdrop), exp = crafted(T)[name]
    assert len(fb) == width * height
    CF.same(MF.model(fb, width, height, cell, palette, n_sub, sub_size, rounds, depth, backdrop), exp, f"{name}: the model")
    CF.same(MF.model_loop(fb, width, height, cell, palette, n_sub, sub_size, rounds, depth, backdrop), exp, f"{name}: the loop")


# ---- the consequences ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def busy(T):
    """A 43 x 29 frame near a hidden table of 6 x 3 colours under 8 x 8 cells, and a master of 24 entries."""
    rng = np.random.default_rng(31)
    hidden = Q.random_colors(T, rng, 18)
    fb, _ = CL.near_sub_palettes(T, rng, CF.frame_params(43, 29), hidden, 6, 3, (8, 8), 10)
    return fb, 43, 29, (8, 8), np.concatenate([hidden, Q.random_colors(T, rng, 6)])


MODES = [(depth, backdrop) for depth in MF.DEPTHS for backdrop in (0, 1)]


@pytest.mark.parametrize("depth,backdrop", MODES)
def test_1_and_2_the_errors_never_rise_and_the_table_is_on_the_lattice(busy, depth, backdrop):
    fb, width, height, cell, master = busy
    fell = 0
    for n_sub, sub_size in ((1, 4), (3, 3), (5, 2), (4, 4)):
        table, _, errors = MF.model(fb, width, height, cell, master, n_sub, sub_size, 5, depth, backdrop)
        errors = errors.astype(np.int64)
        assert (np.diff(errors) <= 0).all(), (n_sub, sub_size, errors)
        assert MF.on_lattice(table, depth)
        if backdrop:
            assert len({table[s * sub_size].tobytes() for s in range(n_sub)}) == 1
        fell += int(errors[-1] < errors[0])
    assert fell >= 3 or depth == MF.BGR222, "the rounds lower something (four levels a channel leave little to move to)"


def test_3_at_rgba8_without_backdrop_it_is_the_plain_fit(busy):
    fb, width, height, cell, master = busy
    for n_sub, sub_size, rounds in ((1, 4, 0), (3, 3, 2), (5, 2, 3), (4, 4, 1)):
        CF.same(MF.model(fb, width, height, cell, master, n_sub, sub_size, rounds, MF.RGBA8, 0),
                CF.model(fb, width, height, cell, master, n_sub, sub_size, rounds), f"S {n_sub} K {sub_size} R {rounds}")


@pytest.mark.parametrize("depth,backdrop", MODES)
def test_4_the_last_error_is_the_difference_quantize_cells_leaves(busy, depth, backdrop):
    fb, width, height, cell, master = busy
    for rounds in (0, 2):
        table, _, errors = MF.model(fb, width, height, cell, master, 4, 3, rounds, depth, backdrop)
        out = CL.model_loop(CF.frame_params(width, height), table, 4, 3, cell, fb, None, 0)[1]
        assert CF.l1_difference(fb, out) == int(errors[rounds]) > 0


@pytest.mark.parametrize("fmt,machine", [(S.BGR555, V.SNES), (S.BGR333_MD, V.MEGADRIVE), (S.BGR222, V.SMS)], ids=["bgr555", "bgr333 md", "bgr222"])
def test_5_the_closing_identity_under_the_machines_own_rules(busy, fmt, machine):
    fb, width, height, cell, master = busy
    n_sub, sub_size = {V.SNES: (4, 3), V.MEGADRIVE: (4, 4), V.SMS: (2, 16)}[machine]
    for backdrop in (0, 1):
        table, _, errors = MF.model(fb, width, height, cell, master, n_sub, sub_size, 2, fmt, backdrop)
        words = V.palette_words(np.ascontiguousarray(table).view(np.uint8).reshape(-1, 4), fmt)
        assert S.palette_rgba(words, fmt)[:, :3].tobytes() == np.ascontiguousarray(table).view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
        for screen_backdrop in ((0, 1) if backdrop else (0,)):
            for flips in (0, 3):
                got, out, bad = MF.shown(TS, fb, width, height, cell, table, n_sub, sub_size, fmt, screen_backdrop, L=V.preset(machine),
                                         tile_format=V.MACHINE_FORMATS[machine][0], flips=flips)
                want = out.copy()
                want["alpha"] = 255
                assert bad == 0 and got.tobytes() == want.tobytes(), (backdrop, screen_backdrop, flips)
                assert CF.l1_difference(fb, got) == int(errors[2]), "the shown frame's error is errors_out[R] and nothing else"
    # and what the identity costs the plain fit: its table does not survive the words
    plain = CF.model(fb, width, height, cell, master, n_sub, sub_size, 2)[0]
    got, out, _ = MF.shown(TS, fb, width, height, cell, plain, n_sub, sub_size, fmt, 0, L=V.preset(machine), tile_format=V.MACHINE_FORMATS[machine][0])
    assert got["red"].tobytes() != out["red"].tobytes() or got["green"].tobytes() != out["green"].tobytes()


def test_6_one_sub_palette_without_rounds_is_the_most_used_rounded_entries(busy):
    fb, width, height, cell, master = busy
    for depth in MF.DEPTHS:
        rounded = MF.round_palette(master, depth)
        index = Q.model(CF.frame_params(width, height), rounded, fb, None, 0)[0]
        used = np.bincount(index, minlength=len(master))
        order = sorted(range(len(master)), key=lambda j: (-used[j], j))[:5]
        table, seeds, _ = MF.model(fb, width, height, cell, master, 1, 5, 0, depth, 0)
        assert table.tobytes() == rounded[order].tobytes() and list(seeds) == [CF.NO_SEED]


def test_7_a_frame_of_one_colour(T):
    fb = np.zeros(20 * 9, dtype=T.COLOR)
    fb[:] = (90, 14, 200, 3)
    master = CF.colours(T, [(0, 0, 0, 9), (100, 10, 190, 8), (255, 255, 255, 7), (100, 10, 190, 6)])
    for depth, distance in ((MF.BGR555, 9 + 6 + 11), (MF.BGR333_MD, 19 + 14 + 18), (MF.BGR222, 5 + 14 + 30), (MF.RGBA8, 24)):
        rounded = MF.round_palette(master, depth)
        for backdrop in (0, 1):
            table, seeds, errors = MF.model(fb, 20, 9, (8, 8), master, 3, 2, 0, depth, backdrop)
            assert table.tobytes() == rounded[[1, 0] * 3].tobytes() and list(seeds) == [CF.NO_SEED, 0, 0]
            assert int(errors[0]) == distance * 180 == CF.l1_difference(fb, Q.model(CF.frame_params(20, 9), rounded, fb, None, 0)[1])


# ---- the graybox frame -----------------------------------------------------------------------------------------------------

# The master fitted at 33 and refined six rounds, 8 x 4 over 8 x 8 cells, R = 6 (the plain fit's own error is 595 951). What
# the machine shows against the RENDERED frame, summed L1: the plain fit's table through the machine's colour words drawn
# with screen backdrop 0 and 1, then the machine fit without and with the backdrop as (errors_out[0], errors_out[6]); the
# fit with the backdrop is shown with screen backdrop 1, and that is its errors_out[6].
GRAYBOX_SHOWN = {
    "snes": (S.BGR555, 1140233, 2552524, (1650447, 1224642), (1648081, 1324859)),
    "megadrive": (S.BGR333_MD, 8388142, 10169386, (4858410, 4854947), (4858410, 4854947)),
    "sms": (S.BGR222, 16876486, 18262234, (12943560, 12943560), (12943560, 12943560)),
}


@pytest.fixture(scope="module")
def graybox(par, oracle, T):
    from test_palette_refine_cpu import graybox_frame
    import palette as P
    import palette_refine as PR
    params, fb = graybox_frame(par, oracle, T)
    assert (params.width, params.height) == (480, 320)
    master = PR.refine(T, params, fb, None, P.fit(T, fb, 33)[0], 6)[0]
    plain = CF.model(fb, 480, 320, (8, 8), master, 8, 4, 6)
    assert int(plain[2][6]) == 595951
    return fb, master, plain[0]


@pytest.mark.parametrize("machine", list(GRAYBOX_SHOWN))
def test_the_graybox_figures(graybox, machine):
    """The figures README and DESIGN quote, and that on this frame the machine fit's shown error is not above the plain
    fit's under the machine's own rules."""
    fb, master, plain = graybox
    fmt, plain_0, plain_1, fit_0, fit_1 = GRAYBOX_SHOWN[machine]
    figures = {}
    for screen_backdrop in (0, 1):
        got, _, bad = MF.shown(TS, fb, 480, 320, (8, 8), plain, 8, 4, fmt, screen_backdrop)
        assert bad == 0
        figures[f"plain, screen backdrop {screen_backdrop}"] = CF.l1_difference(fb, got)
    for backdrop in (0, 1):
        table, _, errors = MF.model(fb, 480, 320, (8, 8), master, 8, 4, 6, fmt, backdrop)
        assert (np.diff(errors.astype(np.int64)) <= 0).all() and MF.on_lattice(table, fmt)
        got, _, bad = MF.shown(TS, fb, 480, 320, (8, 8), table, 8, 4, fmt, backdrop)
        assert bad == 0 and CF.l1_difference(fb, got) == int(errors[6]), "what the machine shows costs errors_out[R]"
        figures[f"machine fit, backdrop {backdrop}"] = (int(errors[0]), int(errors[6]))
    print(machine, figures)
    assert figures == {"plain, screen backdrop 0": plain_0, "plain, screen backdrop 1": plain_1, "machine fit, backdrop 0": fit_0,
                       "machine fit, backdrop 1": fit_1}
    assert fit_1[1] <= plain_1, "under the backdrop rule the machine fit shows no more error than the plain fit"
