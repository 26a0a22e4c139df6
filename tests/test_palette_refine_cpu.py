"""Refined palettes without a GPU: the two calls are declared, exported and bound; the mirror of
par_palette_refine_work has the header's layout; every PAR_ERR_INVALID_ARG and the PAR_ERR_UNSUPPORTED come back before
any device work and with nothing written; the model the GPU tests compare with (palette_refine.py) equals a per-pixel
restatement through the two-nibble selection, on random and on crafted clusters; and the consequences the contract
states hold: the summed L1 error never rises from round to round, a fixed point stays fixed, one colour per cell comes
back exactly, and on the tinted graybox frame the error falls as the contract's authors measured it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import headers
import palette as P
import palette_refine as R
import quantize as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_UNSUPPORTED = 1, 5

DECLARATIONS = {
    "par_palette_refine_device": "const par_params* params, void* stream, const par_color* fb, int row_begin, int row_end, "
                                 "par_color* d_palette, int n_colors, int iterations, uint8_t* d_index, "
                                 "par_palette_refine_work* work, int32_t* d_changed",
    "par_palette_refine_host": "const par_params* params, int device, const par_color* fb, int row_begin, int row_end, "
                               "par_color* palette, int n_colors, int iterations, int* changed_out",
}


def test_declared_exported_and_bound(par):
    headers.assert_declared(par, "par_raytracer.h", DECLARATIONS, ("palette_refine_device", "palette_refine_host"))


def test_the_mirror_has_the_headers_layout(T, tmp_path):
    W = T.PALETTE_REFINE_WORK
    assert W.itemsize == 54272 == C.sizeof(T.PaletteRefineWork) and W.itemsize % 8 == 0
    offsets = {"bins": 0, "rank": 49152, "high": 53248}
    for name, at in offsets.items():
        assert W.fields[name][1] == at == getattr(T.PaletteRefineWork, name).offset, name
    assert W["bins"].shape == (256, 3, 16) and W["rank"].shape == (256, 4) and W["high"].shape == (256,)
    # and the header says the same to a C compiler
    src = tmp_path / "work.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "par_types.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu\\n", sizeof(par_palette_refine_work),\n'
                   '           offsetof(par_palette_refine_work, bins), offsetof(par_palette_refine_work, rank),\n'
                   '           offsetof(par_palette_refine_work, high), _Alignof(par_palette_refine_work));\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "work"
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert [int(v) for v in out.stdout.split()] == [54272, 0, 49152, 53248, 4]


# ---- argument errors: no device needed, nothing written -----------------------------------------------------------

BAD = [("null params", dict(params=None)), ("null fb", dict(fb=None)), ("null palette", dict(palette=None)),
       ("null index", dict(index=None)), ("null work", dict(work=None)),
       ("n_colors 0", dict(n_colors=0)), ("n_colors 257", dict(n_colors=257)), ("n_colors -1", dict(n_colors=-1)),
       ("iterations 0", dict(iterations=0)), ("iterations 17", dict(iterations=17)), ("iterations -2", dict(iterations=-2)),
       ("width 0", dict(width=0)), ("width negative", dict(width=-8)), ("row_begin negative", dict(rows=(-1, 4))),
       ("row_begin == row_end", dict(rows=(3, 3))), ("row_begin > row_end", dict(rows=(5, 2))),
       ("row_end > height", dict(rows=(0, 7))), ("work 4 bytes past an 8-byte boundary", dict(work_shift=4)),
       ("work 1 byte past an 8-byte boundary", dict(work_shift=1))]
DEVICE_ONLY = {"index", "work", "work_shift"}


@pytest.mark.parametrize("form", ["device", "host"])
def test_invalid_arguments_need_no_device_and_write_nothing(par, T, form):
    L = par.lib()
    cases = [(tag, over) for tag, over in BAD if form == "device" or not (set(over) & DEVICE_ONLY)]
    # 2^32 pixels and one more row: the tallies are 32-bit
    cases += [("2^32 pixels", dict(width=65536, height=65536, rows=(0, 65536), status=ERR_UNSUPPORTED)),
              ("more than 2^32 pixels", dict(width=1 << 20, height=1 << 13, rows=(1, 4098), status=ERR_UNSUPPORTED)),
              ("2^32 pixels and a null palette", dict(width=65536, height=65536, rows=(0, 65536), palette=None))]
    assert len(cases) >= 15
    for tag, over in cases:
        params = T.default_params(8, over.get("height", 6))
        params.width = over.get("width", 8)
        # host dummies: never dereferenced
        fb = np.full(8 * 6 * 4, 0xA5, dtype=np.uint8).view(T.COLOR)
        palette = np.full(256 * 4, 0x5A, dtype=np.uint8).view(T.COLOR)
        index = np.full(8 * 6, 0x3C, dtype=np.uint8)
        block = np.full(T.PALETTE_REFINE_WORK.itemsize + 16, 0xC3, dtype=np.uint8)
        at = (-block.ctypes.data) % 8 + over.get("work_shift", 0)
        changed = C.c_int32(-77)
        arg = dict(params=params, fb=fb, palette=palette, index=index, work=block.ctypes.data + at, n_colors=4,
                   iterations=2, rows=(0, 6))
        arg.update({k: v for k, v in over.items() if k in arg})
        p = None if arg["params"] is None else C.byref(arg["params"])
        r0, r1 = arg["rows"]
        if form == "device":
            rc = L.par_palette_refine_device(p, C.c_void_p(0), T.ptr(arg["fb"]), r0, r1, T.ptr(arg["palette"]),
                                             arg["n_colors"], arg["iterations"], T.ptr(arg["index"]),
                                             C.c_void_p(arg["work"]), C.byref(changed))
        else:
            rc = L.par_palette_refine_host(p, -1, T.ptr(arg["fb"]), r0, r1, T.ptr(arg["palette"]), arg["n_colors"],
                                           arg["iterations"], C.byref(changed))
        assert rc == over.get("status", ERR_INVALID_ARG), f"{form}: {tag}: status {rc}"
        assert (fb.view(np.uint8) == 0xA5).all() and (palette.view(np.uint8) == 0x5A).all() and (index == 0x3C).all() \
            and (block == 0xC3).all() and changed.value == -77, f"{form}: {tag}: something was written"


def test_binding_raises(par, T):
    params = T.default_params(8, 6)
    fb = np.zeros(48, dtype=T.COLOR)
    for call, status in ((lambda: par.palette_refine_device(params, 8, (0, 6), 8, 4, 0, 8, 8), ERR_INVALID_ARG),
                         (lambda: par.palette_refine_device(params, 8, (0, 6), 8, 4, 1, 8, 12), ERR_INVALID_ARG),
                         (lambda: par.palette_refine_device(params, 8, (0, 6), 8, 4, 1, None, 8), ERR_INVALID_ARG),
                         (lambda: par.palette_refine_host(params, fb, np.zeros(0, dtype=T.COLOR), 1), ERR_INVALID_ARG),
                         (lambda: par.palette_refine_host(params, fb, np.zeros(4, dtype=T.COLOR), 17), ERR_INVALID_ARG)):
        with pytest.raises(par.ParError) as e:
            call()
        assert e.value.status == status
    with pytest.raises(ValueError):
        par.palette_refine_host(params, fb[:40], np.zeros(4, dtype=T.COLOR), 1)


# ---- the model the GPU tests compare with: the update ---------------------------------------------------------------

ANCHORS = ((0, 0), (255, 0), (0, 255), (255, 255))  # of the two channels a cluster does not vary


def clusters_frame(T, clusters, free):
    """A one-row frame and a palette: cluster j holds the listed values in channel `free` and ANCHORS[j] in the other two,
    and entry j is {128 in `free`, ANCHORS[j], alpha j}: whatever the value, the pixel is nearest to its cluster's entry
    (at most 128 away against at least 255). Entry 4 lies in the middle of the cube and gets no pixel, entry 5 is a
    copy of entry 0 with another alpha. Returns (params, fb, palette, {entry: its lower median})."""
    assert 1 <= len(clusters) <= 4
    others = [c for c in range(3) if c != free]
    palette = np.zeros(6, dtype=T.COLOR)
    rows = []
    for j in range(4):
        e = [0, 0, 0]
        e[free], e[others[0]], e[others[1]] = 128, ANCHORS[j][0], ANCHORS[j][1]
        palette[j] = (e[0], e[1], e[2], j)
        for v in (clusters[j] if j < len(clusters) else []):
            px = list(e)
            px[free] = v
            rows.append((px[0], px[1], px[2], (v * 7 + j) & 0xFF))
    palette[4] = (128, 128, 128, 7)
    palette[5] = palette[0]
    palette[5]["alpha"] = 9
    fb = np.array(rows, dtype=T.COLOR)
    medians = {j: sorted(c)[(len(c) - 1) // 2] for j, c in enumerate(clusters)}
    return T.default_params(len(fb), 1), fb, palette, medians


def crafted_clusters(T):
    """name -> (params, fb, palette, medians): the situations of the selection, shared with test_gpu_palette_refine.py."""
    out = {}
    out["n = 1, 2, 3, 4"] = clusters_frame(T, [[7], [200, 9], [5, 1, 3], [40, 10, 30, 20]], 0)
    out["values 0 and 255"] = clusters_frame(T, [[0, 255, 0], [255, 0, 255], [0, 255], [255] * 3 + [0] * 2], 1)
    out["0x0F against 0x10"] = clusters_frame(T, [[0x0F, 0x10, 0x0F], [0x10, 0x0F, 0x10], [0x10, 0x0F], [0x0F, 0x10, 0x0F, 0x10]], 2)
    out["every pixel in one high nibble"] = clusters_frame(T, [[0x53, 0x5A, 0x51, 0x5F, 0x58], [0xF0, 0xFF, 0xF7, 0xF7]], 0)
    out["a rank inside a nibble with pixels below it"] = clusters_frame(
        T, [[0x70, 0x35, 0x11, 0x39, 0x31], [0x12, 0x11, 0x39, 0x35, 0x31, 0x70], [0x05, 0x06, 0x41, 0x42, 0x43, 0x44, 0x45]], 1)
    out["three empty entries"] = clusters_frame(T, [[17, 99, 3]], 2)
    return out


EXPECTED_MEDIANS = {"n = 1, 2, 3, 4": [7, 9, 3, 20], "values 0 and 255": [0, 255, 0, 255],
                    "0x0F against 0x10": [0x0F, 0x10, 0x0F, 0x0F], "every pixel in one high nibble": [0x58, 0xF7],
                    "a rank inside a nibble with pixels below it": [0x35, 0x31, 0x42], "three empty entries": [17]}


@pytest.mark.parametrize("name", sorted(EXPECTED_MEDIANS))
def test_crafted_clusters(T, name):
    params, fb, palette, medians = crafted_clusters(T)[name]
    assert [medians[j] for j in sorted(medians)] == EXPECTED_MEDIANS[name]
    free = {"n = 1, 2, 3, 4": "red", "values 0 and 255": "green", "0x0F against 0x10": "blue",
            "every pixel in one high nibble": "red", "a rank inside a nibble with pixels below it": "green",
            "three empty entries": "blue"}[name]
    index = R.assign(params, palette, fb, None)
    assert set(index.tolist()) == set(medians), "every cluster goes to its own entry; the copy of entry 0 gets nothing"
    got, changed = R.update(palette, fb, index)
    loop, changed_loop = R.update_loop(palette, fb, index)
    assert got.tobytes() == loop.tobytes() and changed == changed_loop == len(medians)
    for j in range(6):
        if j in medians:
            exp = palette[j].copy()
            exp[free], exp["alpha"] = medians[j], 255
            assert got[j] == exp, (name, j, got[j], exp)
        else:
            assert got[j] == palette[j], f"{name}: entry {j} has no pixel and keeps its four bytes"
    # the whole call: the index plane is the last round's assignment
    full, last, _ = R.refine(T, params, fb, None, palette, 1)
    assert full.tobytes() == got.tobytes() and np.array_equal(last, index)


def test_update_equals_the_per_pixel_loop_on_random_clusters(T):
    rng = np.random.default_rng(31)
    for trial, n_colors in enumerate((1, 2, 7, 40, 256)):
        fb = Q.random_colors(T, rng, 37 * 23)
        if trial % 2:
            for ch in Q.CHANNELS:  # few values a channel: many equal ones around the rank
                fb[ch] &= 0x33
        palette = Q.random_colors(T, rng, n_colors)
        index = R.assign(T.default_params(37, 23), palette, fb, None)
        got, changed = R.update(palette, fb, index)
        loop, changed_loop = R.update_loop(palette, fb, index)
        assert got.tobytes() == loop.tobytes() and changed == changed_loop, n_colors
        # an arbitrary index plane too: the update does not ask where the assignment came from
        index = rng.integers(0, n_colors, len(fb)).astype(np.uint8)
        assert R.update(palette, fb, index)[0].tobytes() == R.update_loop(palette, fb, index)[0].tobytes()


def test_duplicate_entries_the_lower_index_takes_all(T):
    rng = np.random.default_rng(32)
    params = T.default_params(37, 23)
    fb = Q.random_colors(T, rng, 37 * 23)
    palette = Q.random_colors(T, rng, 7)
    palette[5] = palette[2]
    palette[5]["alpha"] ^= 0xFF
    index = R.assign(params, palette, fb, None)
    assert (index == 2).sum() > 20 and not (index == 5).any()
    got, _ = R.update(palette, fb, index)
    assert got[5] == palette[5] and got.tobytes() == R.update_loop(palette, fb, index)[0].tobytes()


# ---- the consequences the contract states -------------------------------------------------------------------------------

def gradient_frame(T, W=37, H=23):
    """A smooth gradient: neighbouring pixels differ by a few units, so that a cell holds many colours."""
    i = np.arange(W * H)
    x, y = i % W, i // W
    fb = np.zeros(W * H, dtype=T.COLOR)
    fb["red"] = 96 + x
    fb["green"] = 64 + y
    fb["blue"] = 200 - (x + y) // 4
    fb["alpha"] = i & 0xFF
    return fb


def rounds_of(T, params, fb, palette, rounds):
    """[(palette, summed error, largest error, changed)] before the first round and after each."""
    out = [(palette, *R.error(params, palette, fb), None)]
    for _ in range(rounds):
        palette, _, changed = R.refine(T, params, fb, None, palette, 1)
        out.append((palette, *R.error(params, palette, fb), changed))
    return out


@pytest.mark.parametrize("frame", ["random", "gradient"])
@pytest.mark.parametrize("n_colors", [1, 2, 7, 256])
def test_the_summed_error_never_rises(T, frame, n_colors):
    rng = np.random.default_rng(33 + n_colors)
    params = T.default_params(37, 23)
    fb = Q.random_colors(T, rng, 37 * 23) if frame == "random" else gradient_frame(T)
    if frame == "gradient":
        assert len(np.unique(fb.view(np.uint32) & 0xFFFFFF)) > 4 * len(np.unique(P.cells(fb)))
    palette = Q.random_colors(T, rng, n_colors)
    steps = rounds_of(T, params, fb, palette, 4)
    sums = [s[1] for s in steps]
    print(f"{frame} frame, {n_colors} entries: summed L1 error {sums}, largest {[s[2] for s in steps]}")
    for before, after in zip(sums, sums[1:]):
        assert after <= before, sums
    assert sums[1] < sums[0], "the first round should gain something on a random palette"
    # four rounds in one call are the four rounds one by one
    whole, _, changed = R.refine(T, params, fb, None, palette, 4)
    assert whole.tobytes() == steps[4][0].tobytes() and changed == steps[4][3]


def test_a_fixed_point_stays_fixed(T):
    rng = np.random.default_rng(34)
    params = T.default_params(37, 23)
    # a frame whose colours are all palette entries
    palette = Q.random_colors(T, rng, 7, alpha=(255, 255))
    fb = palette[rng.integers(0, 7, 37 * 23)]
    fb["alpha"] = rng.integers(0, 256, len(fb))
    got, index, changed = R.refine(T, params, fb, None, palette, 3)
    assert got.tobytes() == palette.tobytes() and changed == 0
    assert R.error(params, got, fb) == (0, 0)
    # and one reached by rounds: further rounds leave it alone
    fb = gradient_frame(T)
    palette = Q.random_colors(T, rng, 7)
    for rounds in range(1, 17):
        palette, _, changed = R.refine(T, params, fb, None, palette, 1)
        if changed == 0:
            break
    assert changed == 0, "no fixed point in 16 rounds"
    again, _, changed = R.refine(T, params, fb, None, palette, 2)
    assert again.tobytes() == palette.tobytes() and changed == 0


@pytest.mark.parametrize("n,n_colors", [(1, 1), (7, 7), (33, 64), (256, 256)])
def test_one_colour_per_cell_comes_back_exactly(T, n, n_colors):
    from test_palette_cpu import one_colour_per_cell
    rng = np.random.default_rng(35)
    params = T.default_params(37, 23)
    colours, fb = one_colour_per_cell(T, rng, n, 37 * 23)
    fitted, n_entries, _ = P.fit(T, fb, n_colors)
    assert n_entries == n
    got, index, changed = R.refine(T, params, fb, None, fitted, 2)
    assert got.tobytes() == fitted.tobytes() and changed == 0
    assert index.max() < n, "the padded copies of entry 0 get no pixel"
    assert Q.model(params, got, fb, None, 0)[1].tobytes() == fb.tobytes()


# ---- the gap this closes: the tinted graybox frame ------------------------------------------------------------------

def graybox_frame(par, oracle, T):
    """The frame of test_palette_cpu.py's last test, composed by the oracle: (params, fb)."""
    from test_gpu_light_range import scene
    from test_gpu_light_tints import COLOUR, TINTS, expected
    sc = scene("graybox", par, oracle, T)
    _, exp, _ = expected(T, sc, [3, 6], [200, 300], TINTS[:2], COLOUR, "graybox, two tinted ranged lights")
    return sc.params, exp["fb"]


def test_refining_the_fitted_palette_of_the_tinted_graybox_frame(par, oracle, T):
    """The figures of the model on this frame at 33 entries: 729 075 as fitted, 558 150 after one round, 543 232 after
    six, with nothing left to change."""
    params, fb = graybox_frame(par, oracle, T)
    assert len(fb) == 153600
    fitted, n_entries, _ = P.fit(T, fb, 33)
    assert n_entries == 33
    steps = [(fitted, *R.error(params, fitted, fb), None)]
    palette = fitted
    for _ in range(7):
        palette, _, changed = R.refine(T, params, fb, None, palette, 1)
        steps.append((palette, *R.error(params, palette, fb), changed))
    print("summed L1 error by round:", [s[1] for s in steps], "largest:", [s[2] for s in steps],
          "changed:", [s[3] for s in steps])
    assert steps[0][1] == 729075 and steps[1][1] == 558150 and steps[6][1] == 543232
    assert steps[7][3] == 0 and steps[7][0].tobytes() == steps[6][0].tobytes(), "after six rounds nothing is left to change"
    for before, after in zip(steps, steps[1:]):
        assert after[1] <= before[1]
