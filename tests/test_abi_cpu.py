"""CPU-side checks of the product library: it loads, exports every symbol the four headers of include/ declare and no
other but the debug hooks, the binding's tables (pixel-art-raytracer_amd/abi.py) are the headers' prototypes and are all
set when the library loads, the headers compile as pedantic C11 alone, twice and together in every order, the host-side
scene helpers match the reference's scene, and rendering without a GPU fails loudly (no fallback)."""
import ctypes
import importlib
import itertools
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import headers

ROOT = headers.ROOT
MAIN = "par_raytracer.h"
PROTOTYPES = {MAIN: 75, "par_cells.h": 3, "par_tileset.h": 5, "par_tileset_extend.h": 3}  # par.ABI_HEADERS, counted


def test_exports_every_declared_symbol(par):
    L = par.lib()
    assert list(par.ABI_HEADERS) == list(PROTOTYPES) and par.ABI_HEADERS[MAIN] is par.ABI
    for header, table in par.ABI_HEADERS.items():
        declared = {name for _, name, _ in headers.prototypes(header)}
        assert declared == set(table), (header, declared ^ set(table))
        for name in declared:
            assert getattr(L, name) is not None
    assert par.ABI_SYMBOLS == tuple(par.ABI)


@pytest.mark.parametrize("header", PROTOTYPES)
def test_the_bindings_table_is_the_headers_prototypes(par, header):
    """Every prototype of the header, its parameters in count, order and kind: the table install() walks agrees, and so do
    the argtypes and restypes that the loaded library's functions carry. A parameter type the mapping does not know fails
    here: a new scalar type is to be decided, not defaulted."""
    protos, table = headers.prototypes(header), par.ABI_HEADERS[header]
    assert len(protos) == PROTOTYPES[header] == len(table)
    assert [name for _, name, _ in protos] == list(table)  # the header's order
    L = par.lib()
    for proto in protos:
        ret, name, _ = proto
        want_restype, want = headers.want_signature(proto)
        restype, argtypes = headers.signature(table[name])
        assert list(argtypes) == want, name
        assert restype is want_restype, name
        fn = getattr(L, name)
        assert list(fn.argtypes) == want and fn.restype is want_restype, name
        if ret == "int":
            assert not isinstance(table[name], tuple), f"{name}: the default restype is not written out"
        else:
            assert isinstance(table[name], tuple), f"{name}: (restype, argument types)"


def test_the_debug_hooks_are_apart_and_bound(par):
    assert set(par.ABI_DEBUG_HOOKS) == {"par_debug_read_stamps", "par_debug_set_hooks", "par_debug_read_light_walks",
                                        "par_debug_read_items"}
    for header, table in par.ABI_HEADERS.items():
        assert not set(par.ABI_DEBUG_HOOKS) & set(table)
        plain = headers.without_comments(header)
        for name in par.ABI_DEBUG_HOOKS:
            assert name not in plain
    for name, entry in par.ABI_DEBUG_HOOKS.items():
        restype, argtypes = headers.signature(entry)
        fn = getattr(par.lib(), name)
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype is ctypes.c_int


def test_every_exported_symbol_is_in_exactly_one_table(par):
    """The par_* functions the built library defines are the disjoint union of the four headers' tables and the hooks."""
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm to list the library's symbols")
    out = subprocess.run([nm, "-D", "--defined-only", par.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(f[2] for f in (line.split() for line in out.splitlines())
                      if len(f) == 3 and f[1] == "T" and f[2].startswith("par_"))
    bound = [name for table in (*par.ABI_HEADERS.values(), par.ABI_DEBUG_HOOKS) for name in table]
    assert len(bound) == len(set(bound)), "a symbol is in two tables"
    assert exported == sorted(bound), set(exported) ^ set(bound)


INSTALLED_AT_LOAD = r"""
import ctypes, importlib, json, sys
par = importlib.import_module("pixel-art-raytracer_amd")
loaded = sorted(m for m in sys.modules if m.startswith("pixel-art-raytracer_amd."))
L = par.lib()
wrong, sized = [], []
for table in (*par.ABI_HEADERS.values(), par.ABI_DEBUG_HOOKS):
    for name, sig in table.items():
        restype, argtypes = sig if type(sig) is tuple else (ctypes.c_int, sig)
        fn = getattr(L, name)
        if fn.argtypes is None or list(fn.argtypes) != list(argtypes) or fn.restype is not restype:
            wrong.append(name)
        if fn.restype is ctypes.c_size_t:
            sized.append(name)
print(json.dumps({"loaded": loaded, "wrong": wrong, "size_t": sized}))
"""


def test_every_table_is_installed_at_load(par):
    """A fresh interpreter that imports the package alone and calls lib(): every function of every table carries its
    table's types, the two size_t returns of the side headers among them, with no side module imported."""
    p = subprocess.run([sys.executable, "-c", INSTALLED_AT_LOAD], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["loaded"] == ["pixel-art-raytracer_amd.abi", "pixel-art-raytracer_amd.types"]
    assert got["wrong"] == []
    assert got["size_t"] == ["par_tileset_work_bytes", "par_tileset_extend_work_bytes"]


def test_the_hip_runtime_is_one_handle(par):
    pytest.importorskip("torch")
    hip = par.hip_runtime()
    assert par.hip_runtime() is hip
    assert len(hip.hipMemcpyAsync.argtypes) == 5 and len(hip.hipStreamSynchronize.argtypes) == 1
    assert len(hip.hipGetDevice.argtypes) == 1


def test_constants_are_the_headers(par):
    header = headers.without_comments(MAIN)
    status = re.search(r"typedef enum par_status \{(.*?)\} par_status;", header, flags=re.S).group(1)
    assert {int(v): k for k, v in re.findall(r"(PAR_\w+) = (\d+)", status)} == par.STATUS_NAMES
    assert par.PAR_OK == 0 and par.STATUS_NAMES[0] == "PAR_OK"
    flags = dict(re.findall(r"PAR_(RENDER_\w+) = 1u << (\d+)", header))
    assert len(flags) == 4
    for name, shift in flags.items():
        assert getattr(par, name) == 1 << int(shift), name
    assert par.MAX_LIGHTS == int(re.search(r"#define PAR_MAX_LIGHTS (\d+)", header).group(1))
    models = re.search(r"enum \{ PAR_LIGHTS_UNBOUNDED = (\d+), PAR_LIGHTS_RANGED = (\d+) \};", header)
    assert (par.LIGHTS_UNBOUNDED, par.LIGHTS_RANGED) == (int(models.group(1)), int(models.group(2)))


def test_library_carries_no_tuning_or_test_switches(par):
    """Launch shapes are constants of the library and test switches are per-context hooks (par_debug_set_hooks):
    nothing in the shipped library reads an environment variable that changes how it renders."""
    blob = open(par.LIB_PATH, "rb").read()
    for name in (b"PAR_TUNE_", b"PAR_EXP_", b"PAR_TEST_", b"PAR_FORCE_GENERIC", b"PAR_BUILD_TWO_LAUNCHES"):
        assert name not in blob, name


def test_default_params_and_grid(par, T):
    p = T.Params()
    par.lib().par_default_params(ctypes.byref(p))
    q = T.default_params()
    assert bytes(p) == bytes(q)
    gx, gy, gz = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert par.lib().par_grid_dims(ctypes.byref(p), ctypes.byref(gx), ctypes.byref(gy), ctypes.byref(gz)) == 0
    assert (gx.value, gy.value, gz.value) == (12, 8, 8) == p.grid_dims()  # alt:120-122
    p.width, p.height, p.length = 4096, 4096, 4096
    assert p.grid_dims() == (103, 103, 103)


def test_tile_sprite_matches_oracle_restatement(par, oracle):
    assert par.tile_floor().tobytes() == oracle.tile_floor().tobytes()


def test_graybox_scene(par, appendix_b):
    a = par.scene_graybox(480, 320)
    assert len(a) == appendix_b["stats"]["entities"]
    assert (a["px"].min(), a["px"].max()) == (0, 9580) and (a["pz"].min(), a["pz"].max()) == (-5860, 6380)
    assert tuple(a[0][["px", "py", "pz", "ex", "ey", "ez"]]) == (240, 36, 80, 20, 20, 20)  # player, alt:520-523


def test_synthetic_scene_is_deterministic(par):
    a, l = par.scene_synthetic(1024, 4096, 4096, 4096, 12345)
    b, _ = par.scene_synthetic(1024, 4096, 4096, 4096, 12345)
    assert a.tobytes() == b.tobytes()
    assert tuple(l[0][["x", "y", "z"]]) == (2560, 2048, 1024)
    assert a["px"].min() >= -20 and a["px"].max() < 4096 and a["py"].max() < 200 and a["pz"].max() < 4096

    # splitmix64(12345): first three draws, independent restatement
    def sm(state):
        mask = (1 << 64) - 1
        state = (state + 0x9E3779B97F4A7C15) & mask
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        return state, z ^ (z >> 31)

    s = 12345
    s, r0 = sm(s)
    s, r1 = sm(s)
    s, r2 = sm(s)
    assert (int(a[0]["px"]), int(a[0]["py"]), int(a[0]["pz"])) == (-20 + r0 % 4116, -20 + r1 % 220, -20 + r2 % 4116)


def test_debug_line_matches_oracle(par, oracle, T):
    params = T.default_params()
    light = T.make_light(480, 160, 80)
    gbuf = np.zeros(480 * 320, dtype=T.PIXEL)
    gbuf[0]["y"], gbuf[0]["z"] = 121, 199
    fa = np.zeros(480 * 320, dtype=T.COLOR)
    fb = np.zeros(480 * 320, dtype=T.COLOR)
    oracle.debug_line(params, gbuf, light, 0, 0, fa)
    par.debug_line(params, gbuf[0:1], 0, light, fb)
    assert fa.tobytes() == fb.tobytes() and fa["alpha"].sum() > 0


def test_no_gpu_means_loud_failure(par, T):
    if par.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(par.ParError) as e:
        par.Renderer(T.default_params())
    assert e.value.status == 2  # PAR_ERR_NO_DEVICE: there is no CPU rendering path


# header -> (a C program that calls into it, the first words of what it prints)
PLAIN_C = {
    MAIN: (r'''
#include <stdio.h>
int main(void) {
    par_params p;
    int gx, gy, gz;
    par_default_params(&p);
    if (par_grid_dims(&p, &gx, &gy, &gz) != PAR_OK) return 1;
    par_sprite s;
    par_sprite_tile_floor(&s);
    printf("%d %d %d %d %zu %zu %zu %s\n", gx, gy, gz, s.depth[0], sizeof(par_pixel), sizeof(par_aabb),
           sizeof(par_sprite), par_status_string(PAR_ERR_NO_DEVICE));
    printf("%zu %zu %zu\n", sizeof(par_params), sizeof(par_frame_stats), sizeof(par_outputs));
    return 0;
}
''', ["12", "8", "8", "19", "28", "16", "16000"]),
    "par_cells.h": (r'''
#include <stdio.h>
int main(void) {
    par_color in[3] = {{1, 2, 3, 4}, {5, 6, 7, 8}, {9, 10, 11, 12}}, out[6];
    int n = par_cells_pairs(in, 3, out, 6);
    printf("%d %d %d %d\n", n, out[1].red, out[4].red, out[5].alpha);
    return par_quantize_cells_host(0, -1, in, 1, 3, 8, 8, 0, in, 0, 1, out, 0, 0) == 1 ? 0 : 1;
}
''', ["3", "5", "5", "12"]),
    "par_tileset.h": (r'''
#include <stdio.h>
int main(void) {
    uint8_t plane[64] = {0};
    uint32_t map[1];
    int count = -5;
    printf("%lu %lu %d\n", (unsigned long)par_tileset_work_bytes(3), (unsigned long)par_tileset_work_bytes(0),
           PAR_TILESET_MAX_CELLS);
    return par_tileset_build_host(0, -1, plane, 0, 8, 8, 8, 0, 3, 0, 0, map, &count) == 1 && count == -5 ? 0 : 1;
}
''', [str(4096 + 48 + 32), "0", str(1 << 20)]),
    "par_tileset_extend.h": (r'''
#include <stdio.h>
int main(void) {
    uint8_t plane[64] = {0};
    uint32_t map[1];
    int count = -5, first_new = -7;
    printf("%lu %lu %lu\n", (unsigned long)par_tileset_extend_work_bytes(3, 2), (unsigned long)par_tileset_extend_work_bytes(0, 2),
           (unsigned long)par_tileset_extend_work_bytes(3, -1));
    return par_tileset_extend_host(0, -1, plane, 0, 8, 8, 8, 0, 3, 0, 0, &count, map, &first_new) == 1 && count == -5 &&
                   first_new == -7
               ? 0
               : 1;
}
''', [str(4096 + 48 + 4 * 16 + 8), "0", "0"]),
}


def test_headers_are_plain_c(tmp_path):
    """include/*.h is a C ABI: it must compile as C11 (no C++), and a C program must link against the library."""
    body, first = PLAIN_C[MAIN]
    out = headers.compile_and_run(tmp_path, [MAIN], body)
    assert out.split()[:7] == first
    # the ctypes mirrors of the structures are laid out as the header's
    import ctypes as C
    T = importlib.import_module("pixel-art-raytracer_amd.types")
    assert [int(v) for v in out.splitlines()[1].split()] == [C.sizeof(T.Params), C.sizeof(T.FrameStats),
                                                             C.sizeof(T.Outputs)]


@pytest.mark.parametrize("header", PROTOTYPES)
def test_every_header_is_plain_c_in_any_company(tmp_path, header):
    """The header alone, twice, and the four together in each of their 24 orders, as pedantic C11; the header's program
    links and prints the same every time."""
    assert sorted(PLAIN_C) == sorted(PROTOTYPES) == sorted(h for h in os.listdir(headers.INCLUDE) if h != "par_types.h")
    body, first = PLAIN_C[header]
    orders = {"alone": [header], "twice": [header, header]}
    orders.update((f"order{k}", list(order)) for k, order in enumerate(itertools.permutations(PROTOTYPES)))
    assert len(orders) == 26
    for tag, includes in orders.items():
        words = headers.compile_and_run(tmp_path, includes, body, tag).split()
        # (par_raytracer.h's program goes on with the text of a status and the sizes test_headers_are_plain_c reads)
        assert words[:len(first)] == first and (header == MAIN or len(words) == len(first)), (tag, words)
