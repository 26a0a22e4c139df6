"""CPU-side checks of the product library: it loads, exports every symbol include/par_raytracer.h declares, the
host-side scene helpers match the reference's scene, and rendering without a GPU fails loudly (no fallback)."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_every_declared_symbol(par):
    L = par.lib()
    header = open(os.path.join(ROOT, "include", "par_raytracer.h")).read()
    declared = set(re.findall(r"^(?:const char\*|void|int)\s+(par_[a-z_0-9]+)\(", header, flags=re.M))
    assert declared == set(par.ABI_SYMBOLS), declared ^ set(par.ABI_SYMBOLS)
    for name in declared:
        assert getattr(L, name) is not None


def header_without_comments():
    header = open(os.path.join(ROOT, "include", "par_raytracer.h")).read()
    return re.sub(r"/\*.*?\*/", "", header, flags=re.S)


def signature(entry):
    """(return type, argument types) of an entry of the binding's table: an int return is not written out there."""
    return entry if isinstance(entry, tuple) else (ctypes.c_int, entry)


RETURNS = {"int": ctypes.c_int, "void": None, "const char*": ctypes.c_char_p}
SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "uint64_t": ctypes.c_uint64}


def test_the_bindings_table_is_the_headers_prototypes(par):
    """Every prototype of the header, its parameters in count, order and kind: the table lib() walks agrees, and so do
    the argtypes and restypes that the loaded library's functions carry. A parameter type the mapping does not know fails
    here: a new scalar type is to be decided, not defaulted."""
    protos = re.findall(r"^(const char\*|void|int)\s+(par_[a-z_0-9]+)\(([^;]*?)\);", header_without_comments(),
                        flags=re.M | re.S)
    assert len(protos) == 75 == len(par.ABI)
    assert [name for _, name, _ in protos] == list(par.ABI) == list(par.ABI_SYMBOLS)  # the header's order
    L = par.lib()
    for ret, name, params in protos:
        want = []
        for p in (" ".join(p.split()) for p in params.split(",")):
            if p == "void":
                assert params.strip() == "void"
            elif "*" in p:
                want.append(ctypes.c_void_p)
            else:
                kind, _ = p.rsplit(" ", 1)  # "<type> <name>"
                assert kind in SCALARS, f"{name}: no ctypes type decided for a parameter `{p}`"
                want.append(SCALARS[kind])
        restype, argtypes = signature(par.ABI[name])
        assert list(argtypes) == want, name
        assert restype is RETURNS[ret], name
        fn = getattr(L, name)
        assert list(fn.argtypes) == want and fn.restype is RETURNS[ret], name
        if ret == "int":
            assert not isinstance(par.ABI[name], tuple), f"{name}: the default restype is not written out"


def test_the_debug_hooks_are_apart_and_bound(par):
    assert set(par.ABI_DEBUG_HOOKS) == {"par_debug_read_stamps", "par_debug_set_hooks", "par_debug_read_light_walks"}
    assert not set(par.ABI_DEBUG_HOOKS) & set(par.ABI)
    header = header_without_comments()
    for name, entry in par.ABI_DEBUG_HOOKS.items():
        assert name not in header
        restype, argtypes = signature(entry)
        fn = getattr(par.lib(), name)
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype is ctypes.c_int


def test_constants_are_the_headers(par):
    header = header_without_comments()
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


def test_headers_are_plain_c(tmp_path):
    """include/*.h is a C ABI: it must compile as C11 (no C++), and a C program must link against the library."""
    import subprocess
    src = tmp_path / "abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "par_raytracer.h"
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
''')
    exe = tmp_path / "abi"
    lib_dir = os.path.join(ROOT, "pixel-art-raytracer_amd", "lib")
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe), "-L", lib_dir, "-lpar_raytracer", f"-Wl,-rpath,{lib_dir}"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0
    assert out.stdout.split()[:7] == ["12", "8", "8", "19", "28", "16", "16000"]
    # the ctypes mirrors of the structures are laid out as the header's
    import ctypes as C
    T = importlib.import_module("pixel-art-raytracer_amd.types")
    assert [int(v) for v in out.stdout.splitlines()[1].split()] == [C.sizeof(T.Params), C.sizeof(T.FrameStats),
                                                                   C.sizeof(T.Outputs)]
