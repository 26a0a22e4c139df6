"""Microseconds per par_tileset_build_device call (tiles for every cell, map and count) and per par_tileset_expand_device
call at 4096 x 4096 and 480 x 320, tiles of 8 x 8 and 16 x 16, flips 0 and 3, on three index planes in device buffers: one
colour (every cell meets on one slot of the table), all cells distinct (every cell claims a slot of its own, T = N), and
the size's rendered frame (the 4096 x 4096 headline frame, the 480 x 320 graybox frame, each under two tinted lights)
through its fitted palette of 16 entries and par_quantize_cells_device at four sub-palettes of four with cells of the
tile's size. Beside each figure, in the same run: a device-to-device copy of the plane on the same stream, the traffic
floor (`x_copy` = T_build / T_copy), and once per plane the numpy model of tests/tileset.py on the host, which is what a
user without the call pays after the copy back. After a warm-up of every call, batches of back-to-back launches between
two events on one stream; the median batch over its launch count, the fastest and the slowest (`spread` is (slowest -
fastest) / median: what a difference has to exceed). Prints one JSON line and writes it to --out (default
profiles/tileset.json).
   python tools/tileset.py [--batches N] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from measure_palette_fit import FRAMES, TINTS  # noqa: E402
from pattern import timed  # noqa: E402

TILES = ((8, 8), (16, 16))
FLIPS = (0, 3)


def numpy_model():
    """tests/tileset.py, the contract in numpy (by its path: this tool has its name)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("tileset_model", os.path.join(ROOT, "tests", "tileset.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def rendered(par, T, name):
    """The size's frame in a device buffer."""
    import numpy as np
    import torch
    (W, H, L), kind, positions, radii = FRAMES[name]
    params = T.default_params(W, H, L)
    aabbs = par.scene_graybox(W, L) if kind == "graybox" else par.scene_synthetic(1024, W, H, L, 12345)[0]
    lights = np.zeros(len(positions), dtype=T.LIGHT)
    for i, ((x, y, z), r) in enumerate(zip(positions, radii)):
        lights[i]["x"], lights[i]["y"], lights[i]["z"], lights[i]["radius"] = x, y, z, r
    fb = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with par.Renderer(params) as r:
        r.set_sprites(par.tile_floor())
        r.set_entities(aabbs)
        r.set_light_model(par.LIGHTS_RANGED)
        r.set_lights(lights)
        r.set_light_tints(T.make_tints(TINTS))
        r.render_device({"fb": fb.data_ptr()})
        torch.cuda.synchronize()
    return params, fb


def measure(name, batches):
    import numpy as np
    import torch
    TS = numpy_model()
    par = importlib.import_module("pixel-art-raytracer_amd")
    cells = importlib.import_module("pixel-art-raytracer_amd.cells")
    ts = importlib.import_module("pixel-art-raytracer_amd.tileset")
    T = importlib.import_module("pixel-art-raytracer_amd.types")
    params, fb = rendered(par, T, name)
    W, H = params.width, params.height
    n = W * H
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    big = n > 1 << 20
    per = 20 if big else 200
    palette = torch.zeros(16 * 4, dtype=torch.uint8, device="cuda")
    fit_work = torch.zeros(T.PALETTE_WORK.itemsize, dtype=torch.uint8, device="cuda")
    w, p, rows = fit_work.data_ptr(), palette.data_ptr(), (0, H)
    par.palette_reset(w, stream=s)
    par.palette_count(params, fb.data_ptr(), rows, w, stream=s)
    par.palette_cut(w, 16, stream=s)
    par.palette_sum(params, fb.data_ptr(), rows, w, stream=s)
    par.palette_emit(w, 16, p, stream=s)
    stream.synchronize()
    plane = torch.zeros(n, dtype=torch.uint8, device="cuda")
    redrawn = torch.zeros(n, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = {"frame": name, "pixels": n}

    def copy():
        with torch.cuda.stream(stream):
            redrawn.copy_(plane, non_blocking=True)

    for tile in TILES:
        gcx, gcy = TS.grid(W, H, tile)
        cells_n = gcx * gcy
        work = torch.zeros(ts.tileset_work_bytes(cells_n), dtype=torch.uint8, device="cuda")
        tiles = torch.zeros(cells_n * tile[0] * tile[1], dtype=torch.uint8, device="cuda")
        tile_map = torch.zeros(cells_n, dtype=torch.int32, device="cuda")
        for kind in ("one colour", "all distinct", "frame"):
            if kind == "one colour":
                plane.fill_(9)
            elif kind == "all distinct":
                plane.copy_(torch.from_numpy(TS.distinct_plane(W, H, tile)))
            else:
                cells.quantize_cells(params, p, 4, 4, tile, fb.data_ptr(), rows, index_out=plane.data_ptr(), stream=s)
            torch.cuda.synchronize()
            host_plane = plane.cpu().numpy()
            key = f"{kind} {tile[0]}x{tile[1]}"
            c = timed(stream, copy, batches, per)
            out[f"copy, {key}"] = c
            for flips in FLIPS:
                t0 = time.perf_counter()
                e_tiles, e_map, e_count = TS.model(host_plane, W, H, tile, 0, flips)
                host_ms = 1e3 * (time.perf_counter() - t0)
                b = timed(stream, lambda: ts.tileset_build(params, plane.data_ptr(), rows, tile, work.data_ptr(), count.data_ptr(),
                                                           tiles_out=tiles.data_ptr(), capacity=cells_n,
                                                           map_out=tile_map.data_ptr(), flips=flips, stream=s), batches, per)
                stream.synchronize()
                got = int(count.cpu().numpy().view(np.uint32)[0])
                assert got == e_count and tile_map.cpu().numpy().view(np.uint32).tobytes() == e_map.tobytes(), (key, flips)
                b.update(tiles=got, cells=cells_n, x_copy=round(b["us"] / c["us"], 2), numpy_model_ms=round(host_ms, 1))
                out[f"build, {key}, flips {flips}"] = b
                e = timed(stream, lambda: ts.tileset_expand(params, tiles.data_ptr(), cells_n, tile, tile_map.data_ptr(), rows,
                                                            redrawn.data_ptr(), stream=s), batches, per)
                stream.synchronize()
                assert torch.equal(redrawn, plane), (key, flips)
                e["x_copy"] = round(e["us"] / c["us"], 2)
                out[f"expand, {key}, flips {flips}"] = e
            # the copy once more behind the calls: how far the yardstick itself moves within the run
            out[f"copy again, {key}"] = timed(stream, copy, batches, per)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tileset.json"))
    a = ap.parse_args()
    result = {"tool": "tileset", "batches": a.batches, "tiles": [list(t) for t in TILES], "flips": list(FLIPS),
              "gpus": 1, "frames": [measure(name, a.batches) for name in FRAMES]}
    line = json.dumps(result)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
