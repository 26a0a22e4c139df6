"""Microseconds per fitted-palette call (par_palette_count / cut / sum / emit _device, and the chain reset, count, cut,
sum, emit) on two rendered frames in device buffers: the 4096 x 4096 headline frame and the 480 x 320 graybox frame,
each under two tinted lights. As a yardstick, par_quantize_device at 256 entries (index plane only, spread 0) over the
fitted palette on the same frame. After a warm-up of every call, batches of back-to-back launches between two events on
one stream; the median batch over its launch count, and the fastest. A batch is sized to last a few milliseconds at
least. The frame stays resident (one buffer), as it is directly after the render that made it. Prints one JSON line and
writes it to --out (default profiles/palette_fit.json).
   python tools/measure_palette_fit.py [--batches N] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TINTS = [(1, .25, 0), (0, .5, 1.5)]
FRAMES = {
    # name: (view size, scene, light positions, radii (0: unbounded))
    "headline 4096x4096": ((4096, 4096, 4096), "synthetic", [(2560, 2048, 1024), (300, 3000, 200)], [0, 0]),
    "graybox 480x320": ((480, 320, 320), "graybox", [(250, 150, 90), (400, 80, 200)], [200, 300]),
}


def timed(stream, call, batches, per_batch):
    import torch
    for _ in range(3):
        call()
    stream.synchronize()
    spans = []
    for _ in range(batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(per_batch):
            call()
        e1.record(stream)
        e1.synchronize()
        spans.append(1000.0 * e0.elapsed_time(e1) / per_batch)
    return {"us": round(statistics.median(spans), 2), "us_min": round(min(spans), 2), "per_batch": per_batch}


def measure(name, batches):
    import numpy as np
    import torch
    par = importlib.import_module("pixel-art-raytracer_amd")
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
    host = fb.cpu().numpy().view(np.uint32) & 0xFFFFFF
    f, w, p, rows = fb.data_ptr(), work.data_ptr(), palette.data_ptr(), (0, H)

    def chain(n_colors):
        par.palette_reset(w, stream=s)
        par.palette_count(params, f, rows, w, stream=s)
        par.palette_cut(w, n_colors, stream=s)
        par.palette_sum(params, f, rows, w, stream=s)
        par.palette_emit(w, n_colors, p, stream=s)

    chain(256)
    stream.synchronize()
    block = work.cpu().numpy().view(T.PALETTE_WORK)
    out = {"frame": name, "pixels": n, "colours": int(len(np.unique(host))),
           "occupied_cells": int((block["hist"][0] != 0).sum()), "n_entries_at_256": int(block["n_entries"][0])}
    # a batch of a few milliseconds at least: many launches of the small frame's short calls
    per = 20 if n > 1 << 20 else 400
    out["count"] = timed(stream, lambda: par.palette_count(params, f, rows, w, stream=s), batches, per)
    # (count has added to the histogram: put the frame's own back before the cuts are timed)
    par.palette_reset(w, stream=s)
    par.palette_count(params, f, rows, w, stream=s)
    for n_colors in (33, 256):
        out[f"cut_{n_colors}"] = timed(stream, lambda: par.palette_cut(w, n_colors, stream=s), batches, 100)
    out["sum"] = timed(stream, lambda: par.palette_sum(params, f, rows, w, stream=s), batches, per)
    out["emit_256"] = timed(stream, lambda: par.palette_emit(w, 256, p, stream=s), batches, 400)
    for n_colors in (33, 256):
        out[f"chain_{n_colors}"] = timed(stream, lambda: chain(n_colors), batches, max(4, per // 4))
    chain(256)
    out["quantize_256"] = timed(stream, lambda: par.quantize(params, p, 256, f, rows, index_out=index.data_ptr(), stream=s),
                                batches, per)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "palette_fit.json"))
    a = ap.parse_args()
    result = {"tool": "measure_palette_fit", "batches": a.batches, "frames": [measure(name, a.batches) for name in FRAMES]}
    line = json.dumps(result)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
