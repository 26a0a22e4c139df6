"""Microseconds per par_quantize_cells_device call (index plane and cell plane, spread 0) at (S, K) = (4, 4), (120, 2)
and (16, 16) with cells of 8 x 8 and of 16 x 16 pixels, on two rendered frames in device buffers: the 4096 x 4096 headline
frame and the 480 x 320 graybox frame, each under two tinted lights. Beside each figure, on the same buffers and in the
same run, par_quantize_device (index plane only, spread 0) at n_colors = S * K over the same table: it does the same
S * K distance evaluations a pixel, so `ratio` = T_cells / T_quantize is what the S reductions, the choice and the second
K-entry search cost, and what one pixel a lane costs against quantise's four. After a warm-up of every call, batches of
back-to-back launches between two events on one stream; the median batch over its launch count, the fastest and the
slowest (`spread` is (slowest - fastest) / median: what a difference has to exceed). A batch is sized to last a few
milliseconds at least. The tables: the frame's fitted palette of 16 entries as four sub-palettes of four, its 120 pairs
(par_cells_pairs), and its fitted palette of 256 entries as sixteen of sixteen. Prints one JSON line and writes it to
--out (default profiles/cells.json).
   python tools/cells.py [--batches N] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from measure_palette_fit import FRAMES, TINTS  # noqa: E402
from pattern import timed  # noqa: E402

SHAPES = ((4, 4), (120, 2), (16, 16))
CELLS = ((8, 8), (16, 16))


def measure(name, batches):
    import numpy as np
    import torch
    par = importlib.import_module("pixel-art-raytracer_amd")
    cells = importlib.import_module("pixel-art-raytracer_amd.cells")
    T = importlib.import_module("pixel-art-raytracer_amd.types")
    (W, H, L), kind, positions, radii = FRAMES[name]
    params = T.default_params(W, H, L)
    aabbs = par.scene_graybox(W, L) if kind == "graybox" else par.scene_synthetic(1024, W, H, L, 12345)[0]
    lights = np.zeros(len(positions), dtype=T.LIGHT)
    for i, ((x, y, z), r) in enumerate(zip(positions, radii)):
        lights[i]["x"], lights[i]["y"], lights[i]["z"], lights[i]["radius"] = x, y, z, r
    n = W * H
    fb = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    work = torch.zeros(T.PALETTE_WORK.itemsize, dtype=torch.uint8, device="cuda")
    palette = torch.zeros(256 * 4, dtype=torch.uint8, device="cuda")
    index = torch.zeros(n, dtype=torch.uint8, device="cuda")
    chosen = torch.zeros(-(-W // 8) * -(-H // 8), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    torch.cuda.synchronize()
    with par.Renderer(params) as r:
        r.set_sprites(par.tile_floor())
        r.set_entities(aabbs)
        r.set_light_model(par.LIGHTS_RANGED)
        r.set_lights(lights)
        r.set_light_tints(T.make_tints(TINTS))
        r.render_device({"fb": fb.data_ptr()}, stream=s)
        stream.synchronize()
    f, w, p, rows = fb.data_ptr(), work.data_ptr(), palette.data_ptr(), (0, H)
    out = {"frame": name, "pixels": n}
    big = n > 1 << 20
    for n_sub, sub_size in SHAPES:
        fit = 16 if sub_size == 2 else n_sub * sub_size
        par.palette_reset(w, stream=s)
        par.palette_count(params, f, rows, w, stream=s)
        par.palette_cut(w, fit, stream=s)
        par.palette_sum(params, f, rows, w, stream=s)
        par.palette_emit(w, fit, p, stream=s)
        stream.synchronize()
        if sub_size == 2:
            table = cells.cells_pairs(palette[:4 * fit].cpu().numpy().view(T.COLOR))
            assert len(table) == n_sub * sub_size
            palette[:4 * len(table)] = torch.from_numpy(table.view(np.uint8).copy()).cuda()
            torch.cuda.synchronize()
        n_colors = n_sub * sub_size
        per = 20 if big else 200  # a batch of a few milliseconds at least
        key = f"{n_sub}x{sub_size}"
        q = timed(stream, lambda: par.quantize(params, p, n_colors, f, rows, index_out=index.data_ptr(), stream=s), batches, per)
        out[f"quantize_{key}"] = q
        for cell in CELLS:
            t = timed(stream, lambda: cells.quantize_cells(params, p, n_sub, sub_size, cell, f, rows, index_out=index.data_ptr(),
                                                           cell_out=chosen.data_ptr(), stream=s), batches, per)
            t["ratio"] = round(t["us"] / q["us"], 3)
            out[f"cells_{key}_{cell[0]}x{cell[1]}"] = t
            if cell == (8, 8):
                stream.synchronize()
                t["sub_palettes_that_win"] = int(len(torch.unique(chosen)))
        # quantise once more behind the cells calls: how far the yardstick itself moves within the run
        out[f"quantize_{key}_again"] = timed(stream, lambda: par.quantize(params, p, n_colors, f, rows, index_out=index.data_ptr(),
                                                                          stream=s), batches, per)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cells.json"))
    a = ap.parse_args()
    result = {"tool": "cells", "batches": a.batches, "shapes": [list(x) for x in SHAPES], "cells": [list(c) for c in CELLS],
              "frames": [measure(name, a.batches) for name in FRAMES]}
    line = json.dumps(result)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
