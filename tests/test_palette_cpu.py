"""Fitted palettes without a GPU: the six calls are declared, exported and bound; every PAR_ERR_INVALID_ARG comes back
before any device work and with nothing written; the mirror of par_palette_work has the header's layout; the model the
GPU tests compare with (palette.py) equals a plain per-cell loop (cut) and Python big integers (emit); the two
consequences the contract states hold; and on the tinted graybox frame a fitted palette of the ramp's size is closer to
the frame than the ramp, in sum and at the worst pixel."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import headers
import palette as P
import quantize as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = 1

DECLARATIONS = {
    "par_palette_reset_device": "void* stream, par_palette_work* work",
    "par_palette_count_device": "const par_params* params, void* stream, const par_color* fb, int row_begin, int row_end, "
                                "par_palette_work* work",
    "par_palette_cut_device": "void* stream, par_palette_work* work, int n_colors",
    "par_palette_sum_device": "const par_params* params, void* stream, const par_color* fb, int row_begin, int row_end, "
                              "par_palette_work* work",
    "par_palette_emit_device": "void* stream, const par_palette_work* work, int n_colors, par_color* d_palette",
    "par_palette_fit_host": "const par_params* params, int device, const par_color* fb, int row_begin, int row_end, "
                            "int n_colors, par_color* palette_out, int* n_entries_out",
}


def test_declared_exported_and_bound(par):
    headers.assert_declared(par, "par_raytracer.h", DECLARATIONS, ("palette_reset", "palette_count", "palette_cut", "palette_sum", "palette_emit", "palette_fit_host"))


def test_the_mirror_has_the_headers_layout(T, tmp_path):
    W = T.PALETTE_WORK
    assert W.itemsize == 172048 == C.sizeof(T.PaletteWork) and T.PALETTE_CELLS == 32768
    offsets = {"hist": 0, "sums": 131072, "lut": 139264, "n_entries": 172032, "reserved": 172036}
    for name, at in offsets.items():
        assert W.fields[name][1] == at == getattr(T.PaletteWork, name).offset, name
    assert W["hist"].shape == (32768,) and W["sums"].shape == (256, 4) and W["lut"].shape == (32768,)
    # and the header says the same to a C compiler
    import subprocess
    src = tmp_path / "work.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "par_types.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(par_palette_work), offsetof(par_palette_work, hist),\n'
                   '           offsetof(par_palette_work, sums), offsetof(par_palette_work, lut),\n'
                   '           offsetof(par_palette_work, n_entries), offsetof(par_palette_work, reserved));\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "work"
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert [int(v) for v in out.stdout.split()] == [172048, 0, 131072, 139264, 172032, 172036]
    # the cell of a colour
    c = np.array([(255, 0, 8, 9), (7, 8, 255, 0)], dtype=T.COLOR)
    assert T.palette_cell(c).tolist() == [31 | 1 << 10, 1 << 5 | 31 << 10] == P.cells(c).tolist()


# ---- argument errors: no device needed, nothing written -----------------------------------------------------------

def _bad_calls(call):
    """(tag, overrides) — one case per condition of the contract that the call can meet."""
    plane = [("null params", dict(params=None)), ("null fb", dict(fb=None)), ("width 0", dict(width=0)),
             ("width negative", dict(width=-8)), ("row_begin negative", dict(rows=(-1, 4))),
             ("row_begin == row_end", dict(rows=(3, 3))), ("row_begin > row_end", dict(rows=(5, 2))),
             ("row_end > height", dict(rows=(0, 7)))]
    colors = [("n_colors 0", dict(n_colors=0)), ("n_colors 257", dict(n_colors=257)), ("n_colors -1", dict(n_colors=-1))]
    work = [("null work", dict(work=None)), ("work 4 bytes past an 8-byte boundary", dict(work_shift=4)),
            ("work 1 byte past an 8-byte boundary", dict(work_shift=1))]
    return {"reset": work, "count": plane + work, "sum": plane + work, "cut": colors + work,
            "emit": colors + work + [("null palette", dict(palette=None))],
            "fit": plane + colors + [("null palette_out", dict(palette=None)),
                                     ("null n_entries_out", dict(n_entries=None))]}[call]


@pytest.mark.parametrize("call", ["reset", "count", "cut", "sum", "emit", "fit"])
def test_invalid_arguments_need_no_device_and_write_nothing(par, T, call):
    L = par.lib()
    cases = _bad_calls(call)
    assert len(cases) >= 3
    for tag, over in cases:
        params = T.default_params(8, 6)
        params.width = over.get("width", 8)
        # host dummies: never dereferenced
        fb = np.full(8 * 6 * 4, 0xA5, dtype=np.uint8).view(T.COLOR)
        palette = np.full(256 * 4, 0x5A, dtype=np.uint8).view(T.COLOR)
        block = np.full(T.PALETTE_WORK.itemsize + 16, 0xC3, dtype=np.uint8)
        at = (-block.ctypes.data) % 8 + over.get("work_shift", 0)
        n_entries = C.c_int(-77)
        arg = dict(params=params, fb=fb, palette=palette, work=block.ctypes.data + at, n_colors=4, rows=(0, 6),
                   n_entries=n_entries)
        arg.update({k: v for k, v in over.items() if k not in ("width", "work_shift")})
        p = None if arg["params"] is None else C.byref(arg["params"])
        work = C.c_void_p(arg["work"])
        n_out = None if arg["n_entries"] is None else C.byref(arg["n_entries"])
        stream = C.c_void_p(0)
        r0, r1 = arg["rows"]
        rc = {"reset": lambda: L.par_palette_reset_device(stream, work),
              "count": lambda: L.par_palette_count_device(p, stream, T.ptr(arg["fb"]), r0, r1, work),
              "cut": lambda: L.par_palette_cut_device(stream, work, arg["n_colors"]),
              "sum": lambda: L.par_palette_sum_device(p, stream, T.ptr(arg["fb"]), r0, r1, work),
              "emit": lambda: L.par_palette_emit_device(stream, work, arg["n_colors"], T.ptr(arg["palette"])),
              "fit": lambda: L.par_palette_fit_host(p, -1, T.ptr(arg["fb"]), r0, r1, arg["n_colors"], T.ptr(arg["palette"]),
                                                    n_out)}[call]()
        assert rc == ERR_INVALID_ARG, f"{call}: {tag}: status {rc}"
        assert (fb.view(np.uint8) == 0xA5).all() and (palette.view(np.uint8) == 0x5A).all() and (block == 0xC3).all() \
            and n_entries.value == -77, f"{call}: {tag}: something was written"


def test_binding_raises_invalid_arg(par, T):
    params = T.default_params(8, 6)
    for call in (lambda: par.palette_reset(0), lambda: par.palette_count(params, 0, (0, 6), 8),
                 lambda: par.palette_cut(8, 0), lambda: par.palette_sum(params, 8, (0, 6), 12),
                 lambda: par.palette_emit(8, 300, 8),
                 lambda: par.palette_fit_host(params, np.zeros(48, dtype=T.COLOR), 0)):
        with pytest.raises(par.ParError) as e:
            call()
        assert e.value.status == ERR_INVALID_ARG


# ---- the model the GPU tests compare with: the cut ------------------------------------------------------------------

def cut_loop(hist, n_colors):
    """The cut of the contract one cell at a time in Python integers: (lut as a list of 32 768 entries, n_entries)."""
    occupied = [(c & 31, (c >> 5) & 31, c >> 10, int(h)) for c, h in enumerate(hist) if h]
    if not occupied:
        return [0] * 32768, 0
    regions = [{"lo": [0, 0, 0], "hi": [31, 31, 31], "cells": occupied}]

    def stats(r):
        n = sum(cell[3] for cell in r["cells"])
        lo = [min(cell[a] for cell in r["cells"]) for a in range(3)]
        hi = [max(cell[a] for cell in r["cells"]) for a in range(3)]
        return n, lo, hi, max(h - l for l, h in zip(lo, hi))

    while len(regions) < n_colors:
        best, key = None, None
        for k, r in enumerate(regions):
            n, _, _, e = stats(r)
            if e >= 1 and (key is None or e > key[0] or (e == key[0] and n > key[1])):
                best, key = k, (e, n)
        if best is None:
            break
        r = regions[best]
        n, lo, hi, e = stats(r)
        axis = 0 if hi[0] - lo[0] == e else (1 if hi[1] - lo[1] == e else 2)
        s = hi[axis] - 1
        for v in range(lo[axis], hi[axis]):
            if 2 * sum(cell[3] for cell in r["cells"] if cell[axis] <= v) >= n:
                s = v
                break
        left = {"lo": list(r["lo"]), "hi": list(r["hi"]), "cells": [c for c in r["cells"] if c[axis] <= s]}
        right = {"lo": list(r["lo"]), "hi": list(r["hi"]), "cells": [c for c in r["cells"] if c[axis] > s]}
        left["hi"][axis], right["lo"][axis] = s, s + 1
        assert left["cells"] and right["cells"]
        regions[best] = left
        regions.append(right)
    lut = [None] * 32768
    for k, r in enumerate(regions):
        for b in range(r["lo"][2], r["hi"][2] + 1):
            for g in range(r["lo"][1], r["hi"][1] + 1):
                for red in range(r["lo"][0], r["hi"][0] + 1):
                    assert lut[red | g << 5 | b << 10] is None, "the regions overlap"
                    lut[red | g << 5 | b << 10] = k
    assert None not in lut, "the regions do not cover the cube"
    return lut, len(regions)


def cell(r, g, b):
    return r | g << 5 | b << 10


def crafted_histograms():
    """name -> (hist, n_colors list): the situations the GPU cut cases are named for, shared with test_gpu_palette.py."""
    rng = np.random.default_rng(21)
    out = {}
    out["all zero"] = (np.zeros(32768, dtype=np.uint32), [1, 5, 256])
    h = np.zeros(32768, dtype=np.uint32)
    h[cell(3, 30, 17)] = 9
    out["one cell"] = (h, [1, 2, 256])
    h = np.zeros(32768, dtype=np.uint32)
    h[rng.choice(32768, 300, replace=False)] = rng.integers(1, 1000, 300)
    out["300 cells"] = (h, [1, 2, 255, 256])
    h = np.zeros(32768, dtype=np.uint32)
    h[rng.choice(32768, 40, replace=False)] = rng.integers(1, 1000, 40)
    out["fewer cells than n_colors"] = (h, [41, 64, 256])
    h = np.zeros(32768, dtype=np.uint32)
    for c in (cell(2, 5, 9), cell(12, 15, 9), cell(7, 9, 9), cell(2, 15, 9)):
        h[c] = 5
    out["equal extents on red and green"] = (h, [2, 3, 4])
    h = np.zeros(32768, dtype=np.uint32)
    for c in (cell(1, 2, 3), cell(21, 22, 23), cell(11, 2, 23), cell(1, 22, 13)):
        h[c] = 7
    out["equal extents on three axes"] = (h, [2, 3, 4])
    h = np.zeros(32768, dtype=np.uint32)
    for c in (cell(0, 0, 0), cell(4, 0, 0), cell(20, 0, 0), cell(24, 0, 0), cell(10, 3, 0), cell(30, 3, 0)):
        h[c] = 10
    out["two regions of equal extent and population"] = (h, [2, 3, 4, 5])
    h = np.zeros(32768, dtype=np.uint32)
    for v, n in ((4, 10), (6, 15), (9, 5), (20, 30)):
        h[cell(v, 0, 0)] = n
    out["a median exactly on 2 cum = n"] = (h, [2, 3])
    h = np.zeros(32768, dtype=np.uint32)
    for v, n in ((4, 1), (6, 2), (9, 3), (20, 100)):
        h[cell(0, v, 7)] = n
    out["a last bin that outweighs the rest"] = (h, [2, 3, 4])
    h = np.zeros(32768, dtype=np.uint32)
    h[rng.choice(32768, 9000, replace=False)] = 0xFFFFFFFF
    h[rng.choice(32768, 500, replace=False)] = rng.integers(0, 1 << 32, 500, dtype=np.uint64).astype(np.uint32)
    out["populations above 32 bits"] = (h, [16, 256])
    out["full random"] = (rng.integers(1, 1 << 20, 32768, dtype=np.uint64).astype(np.uint32), [256])
    return out


def first_split(hist):
    """(axis, s) of the cut's first step: region 0 keeps [0, s] on the axis, and s <= 30."""
    _, hi = P.cut_regions(hist, 2)[0]
    axis = [a for a in range(3) if hi[a] != 31][0]
    return axis, hi[axis]


def test_crafted_histograms_reach_their_situations():
    H = crafted_histograms()
    assert P.cut_regions(H["all zero"][0], 256) == []
    assert P.cut_regions(H["one cell"][0], 256) == [((0, 0, 0), (31, 31, 31))]
    # equal extents: the first axis of red, green, blue wins
    assert first_split(H["equal extents on red and green"][0])[0] == 0
    assert first_split(H["equal extents on three axes"][0])[0] == 0
    # a median on 2 cum = n: 10 + 15 + 5 = 30 of 60 at v = 9, and 25 of 60 at v = 6 is not enough
    assert first_split(H["a median exactly on 2 cum = n"][0]) == (0, 9)
    # no v below hi reaches half: s = hi - 1 = 19 on green
    assert first_split(H["a last bin that outweighs the rest"][0]) == (1, 19)
    # after the first split ({0, 4, 10} | {20, 24, 30} on red) the two regions have extent 10 and 30 pixels each: the
    # lower index is split first
    r2 = P.cut_regions(H["two regions of equal extent and population"][0], 2)
    assert r2 == [((0, 0, 0), (10, 31, 31)), ((11, 0, 0), (31, 31, 31))], r2
    r3 = P.cut_regions(H["two regions of equal extent and population"][0], 3)
    assert r3 == [((0, 0, 0), (4, 31, 31)), ((11, 0, 0), (31, 31, 31)), ((5, 0, 0), (10, 31, 31))], r3
    assert int(H["populations above 32 bits"][0].astype(np.uint64).sum()) > 1 << 44


@pytest.mark.parametrize("name", ["all zero", "one cell", "300 cells", "fewer cells than n_colors",
                                  "equal extents on red and green", "equal extents on three axes",
                                  "two regions of equal extent and population", "a median exactly on 2 cum = n",
                                  "a last bin that outweighs the rest", "populations above 32 bits"])
def test_cut_equals_the_per_cell_loop(T, name):
    hist, n_colors_list = crafted_histograms()[name]
    occupied = int((hist != 0).sum())
    for n_colors in n_colors_list:
        if name == "populations above 32 bits" and n_colors > 16:
            continue  # (the loop is quadratic in the occupied cells; 16 regions of 9000 cells show the 64-bit sums)
        work = P.new_work(T)
        work["hist"][0] = hist
        work["sums"][0] = 0xABCDEF0123456789
        work["reserved"][0] = (1, 2, 3)
        P.cut(work, n_colors)
        lut, n_entries = cut_loop(hist.tolist(), n_colors)
        assert int(work["n_entries"][0]) == n_entries == min(n_colors, occupied), (name, n_colors)
        assert work["lut"][0].tolist() == lut, (name, n_colors)
        assert not work["sums"][0].any() and work["reserved"][0].tolist() == [1, 2, 3]
        assert np.array_equal(work["hist"][0], hist)


def test_cut_of_random_sparse_histograms_equals_the_loop(T):
    rng = np.random.default_rng(22)
    for trial in range(6):
        hist = np.zeros(32768, dtype=np.uint32)
        k = int(rng.integers(2, 200))
        hist[rng.choice(32768, k, replace=False)] = rng.integers(1, 50, k)
        n_colors = int(rng.integers(1, 257))
        work = P.new_work(T)
        work["hist"][0] = hist
        P.cut(work, n_colors)
        lut, n_entries = cut_loop(hist.tolist(), n_colors)
        assert int(work["n_entries"][0]) == n_entries == min(n_colors, k)
        assert work["lut"][0].tolist() == lut, trial


# ---- emit -----------------------------------------------------------------------------------------------------------

def crafted_sums(T):
    """A work block whose sums hold rows of count 0, means exactly on a half, and sums above 2^32."""
    rng = np.random.default_rng(23)
    work = P.new_work(T)
    s = work["sums"][0]
    n = rng.integers(1, 1 << 20, 256).astype(np.uint64)
    for c in range(3):
        s[:, c] = (rng.integers(0, 256, 256).astype(np.uint64) * n) + rng.integers(0, 2, 256).astype(np.uint64) * (n // 2)
    s[:, 3] = n
    s[5] = (7, 9, 11, 0)  # a count of 0 with sums that are not
    s[9] = (0, 0, 0, 0)
    s[0] = (3, 5, 250 * 2 + 1, 2)  # 1.5, 2.5, 250.5: on a half, rounded up
    s[1] = (200 << 34,(17 << 34) + (1 << 33), 255 << 34, 1 << 34)  # above 2^32; green is 17.5
    return work


def test_emit_equals_big_integers(T):
    work = crafted_sums(T)
    s = work["sums"][0]
    assert s[1, 0] > 1 << 32 and (s[:, 3] == 0).sum() == 2
    for n_entries, n_colors in ((0, 7), (12, 33), (256, 256), (256, 33), (33, 33), (1, 256), (-3, 4)):
        work["n_entries"][0] = n_entries
        got = P.emit(T, work, n_colors)
        assert len(got) == n_colors
        m = min(n_entries, n_colors)
        for k in range(n_colors):
            row = [int(v) for v in s[k if k < m else 0]] if m > 0 else [0, 0, 0, 0]
            if row[3] == 0:
                exp = (0, 0, 0, 0)
            else:  # the mean rounded to the nearest integer, a half upwards
                exp = tuple(int(Fraction(row[c], row[3]) + Fraction(1, 2)) for c in range(3)) + (255,)
            assert tuple(int(v) for v in got[k]) == exp, (n_entries, n_colors, k)
    work["n_entries"][0] = 256
    got = P.emit(T, work, 256)
    assert tuple(int(v) for v in got[0]) == (2, 3, 251, 255) and tuple(int(v) for v in got[1]) == (200, 18, 255, 255)
    assert tuple(int(v) for v in got[5]) == (0, 0, 0, 0)


# ---- the two consequences the contract states -----------------------------------------------------------------------

def one_colour_per_cell(T, rng, n, size):
    """A frame of `size` pixels over n colours that lie in n different cells, every colour used."""
    at = rng.choice(32768, n, replace=False)
    colours = np.zeros(n, dtype=T.COLOR)
    colours["red"] = ((at & 31) << 3) + rng.integers(0, 8, n)
    colours["green"] = (((at >> 5) & 31) << 3) + rng.integers(0, 8, n)
    colours["blue"] = ((at >> 10) << 3) + rng.integers(0, 8, n)
    fb = colours[np.concatenate([np.arange(n), rng.integers(0, n, size - n)])]
    fb["alpha"] = rng.integers(0, 256, size)
    return colours, fb


@pytest.mark.parametrize("occupied,n_colors", [(1, 1), (5, 3), (40, 40), (40, 256), (256, 256), (300, 256), (300, 17)])
def test_n_entries_is_the_smaller_of_n_colors_and_the_occupied_cells(T, occupied, n_colors):
    rng = np.random.default_rng(24)
    _, fb = one_colour_per_cell(T, rng, occupied, 37 * 23)
    palette, n_entries, work = P.fit(T, fb, n_colors)
    assert int((work["hist"][0] != 0).sum()) == occupied and n_entries == min(n_colors, occupied)
    assert int(work["hist"][0].astype(np.uint64).sum()) == len(fb) == int(work["sums"][0][:, 3].sum())


@pytest.mark.parametrize("n,n_colors", [(1, 1), (7, 7), (33, 64), (256, 256)])
def test_one_colour_per_cell_comes_back_exactly(T, n, n_colors):
    rng = np.random.default_rng(25)
    params = T.default_params(37, 23)
    colours, fb = one_colour_per_cell(T, rng, n, 37 * 23)
    palette, n_entries, _ = P.fit(T, fb, n_colors)
    assert n_entries == n
    rgb = lambda a: sorted((a.view(np.uint32) & 0xFFFFFF).tolist())
    assert rgb(palette[:n]) == rgb(colours) and (palette[:n]["alpha"] == 255).all()
    assert palette[n:].tobytes() == palette[:1].tobytes() * (n_colors - n), "padded with copies of entry 0"
    index, out = Q.model(params, palette, fb, None, 0)
    assert out.tobytes() == fb.tobytes() and index.max() < n, "a padded entry never shows"


# ---- the gap this closes: the tinted graybox frame ------------------------------------------------------------------

def test_a_fitted_palette_is_closer_to_the_tinted_graybox_frame_than_the_ramp(par, oracle, T):
    """The frame of test_gpu_quantize.py::test_in_a_frame_loop, composed by the oracle. A scratch run of the model gave
    a summed L1 error of 729 075 against the ramp's 2 291 764 and a largest of 38 against 185."""
    from test_gpu_light_range import scene
    from test_gpu_light_tints import COLOUR, TINTS, expected
    sc = scene("graybox", par, oracle, T)
    params = sc.params
    _, exp, _ = expected(T, sc, [3, 6], [200, 300], TINTS[:2], COLOUR, "graybox, two tinted ranged lights")
    fb = exp["fb"]
    assert len(fb) == 153600
    ramp = par.palette_ramp(params, 8)
    fitted, n_entries, work = P.fit(T, fb, 33)
    assert len(ramp) == 33 == n_entries
    occupied = int((work["hist"][0] != 0).sum())
    assert P.fit(T, fb, 256)[1] == occupied < 256

    def errors(palette):
        d = Q.distances(params, palette, fb, None, 0).min(axis=1).astype(np.int64)
        return int(d.sum()), int(d.max())

    ramp_sum, ramp_max = errors(ramp)
    fit_sum, fit_max = errors(fitted)
    print(f"occupied cells {occupied}; ramp: sum {ramp_sum} max {ramp_max}; fitted 33: sum {fit_sum} max {fit_max}")
    assert fit_sum < ramp_sum and fit_max < ramp_max
