"""Machine fit: the table of per-cell sub-palettes of cells_fit fitted under a tile machine's colour depth and backdrop rule
(addons/include/par_machine_fit.h). An add-on: the four calls live in a library of their own, lib/libpar_machine_fit.so,
which this module loads itself at the first call; their signatures are ABI_MACHINE_FIT below, a table that is NOT one of
abi.py's (the core library exports none of them), and the package does not import this module. The calls raise the
package's ParError with the symbol's name; a device pointer or a stream is an int or None.

    fit = importlib.import_module("pixel-art-raytracer_amd.machine_fit")
"""
import ctypes as C
import os
import sys

import numpy as np

from .types import ptr

_par = sys.modules[__package__]  # the package module: its ParError, _ok and _dp, and the HIP runtime it shares with torch

_p, _i = C.c_void_p, C.c_int
# addons/include/par_machine_fit.h, in its order
ABI_MACHINE_FIT = {
    "par_machine_round": (C.c_size_t, [_p, _i, _i, _p]),
    "par_machine_fit_work_bytes": (C.c_size_t, [_i, _i, _i, _i]),
    "par_machine_fit_device": [_p, _p, _i, _i, _i, _i, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p],
    "par_machine_fit_host": [_i, _p, _i, _i, _i, _i, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p],
}
ABI_MACHINE_FIT_SYMBOLS = tuple(ABI_MACHINE_FIT)
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libpar_machine_fit.so")
MAX_CELLS, MAX_SUB_SIZE, MAX_ROUNDS = 1 << 20, 16, 32


class Depth:
    """par_machine_depth: equal in value to the screen add-on's palette formats; 5, 3, 2 and 8 bits a channel."""
    BGR555, BGR333_MD, BGR222, RGBA8 = range(4)
    BITS = (5, 3, 2, 8)


_lib = None


def lib():
    """libpar_machine_fit.so with the table set on its functions, loaded at the first call (the package's loader). No
    fallback."""
    global _lib
    if _lib is None:
        _lib = _par._load(LIB_PATH, ABI_MACHINE_FIT)
    return _lib


def machine_round(palette, depth):
    """Host arithmetic (par_machine_round): the (n, 4) uint8 entries of `palette`, a COLOR array or uint8, rounded to the
    lattice of `depth`, alpha kept. Raises ValueError where the call refuses (no entries, over 256, an unknown depth)."""
    palette = np.ascontiguousarray(palette).view(np.uint8).reshape(-1)
    if len(palette) % 4:
        raise ValueError(f"machine_round: palette holds {len(palette)} bytes, no whole number of entries of 4")
    out = np.zeros(max(4, len(palette)), dtype=np.uint8)
    n = lib().par_machine_round(ptr(palette), len(palette) // 4, depth, ptr(out))
    if n != len(palette) or n == 0:
        raise ValueError(f"machine_round: {len(palette) // 4} entries at depth {depth} were refused")
    return out[:n].reshape(-1, 4)


def machine_fit_work_bytes(width, height, cell):
    """The bytes of the work block of a machine_fit over a width x height frame under cells of cell[0] x cell[1] pixels
    (par_machine_fit_work_bytes); 0 outside the limits."""
    return lib().par_machine_fit_work_bytes(width, height, cell[0], cell[1])


def machine_fit(fb, width, height, cell, palette, n_colors, n_sub, sub_size, rounds, depth, backdrop, work, table_out,
                seeds_out=None, errors_out=None, stream=None):
    """Device pointers (ints): cells_fit's table under the colour depth `depth` (a Depth value) and, with backdrop 1, one
    shared entry 0 (par_machine_fit_device): the n_sub * sub_size four-byte entries go to table_out, the n_sub seed cells
    (uint32) to seeds_out and the rounds + 1 errors (uint64) to errors_out when given. `work` holds
    machine_fit_work_bytes(width, height, cell) bytes and needs no preparation. Asynchronous on `stream`."""
    dp = _par._dp
    _par._ok(lib().par_machine_fit_device, dp(stream), dp(fb), width, height, cell[0], cell[1], dp(palette), n_colors, n_sub,
             sub_size, rounds, depth, backdrop, dp(work), dp(table_out), dp(seeds_out), dp(errors_out))


def machine_fit_host(fb, width, height, cell, palette, n_sub, sub_size, rounds=0, depth=Depth.RGBA8, backdrop=0, device=-1):
    """The same on host arrays (par_machine_fit_host): `fb` is a COLOR array (or uint8, four bytes a pixel) of
    width * height pixels, `palette` likewise the master's entries. Returns {"table": uint8 array (n_sub * sub_size, 4),
    "seeds": uint32 array of n_sub, "errors": uint64 array of rounds + 1}."""
    who = "machine_fit_host"
    fb = np.ascontiguousarray(fb).view(np.uint8).reshape(-1)
    palette = np.ascontiguousarray(palette).view(np.uint8).reshape(-1)
    if len(palette) % 4:
        raise ValueError(f"{who}: palette holds {len(palette)} bytes, no whole number of entries of 4")
    if len(fb) != 4 * max(0, int(width)) * max(0, int(height)):
        raise ValueError(f"{who}: fb holds {len(fb)} bytes, a {width} x {height} frame {4 * max(0, width) * max(0, height)}")
    table = np.zeros((max(1, min(256, max(0, n_sub) * max(0, sub_size))), 4), dtype=np.uint8)
    seeds = np.zeros(max(1, n_sub), dtype=np.uint32)
    errors = np.zeros(max(1, min(MAX_ROUNDS, rounds) + 1), dtype=np.uint64)
    _par._ok(lib().par_machine_fit_host, device, ptr(fb), width, height, cell[0], cell[1], ptr(palette), len(palette) // 4,
             n_sub, sub_size, rounds, depth, backdrop, ptr(table), ptr(seeds), ptr(errors))
    return {"table": table, "seeds": seeds, "errors": errors}
