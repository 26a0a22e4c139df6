"""Microseconds per par_quantize_pattern_device call at depths 1, 4, 8 and 16 (strength 256, index plane only), at 33 and
at 256 entries, on two rendered frames in device buffers: the 4096 x 4096 headline frame and the 480 x 320 graybox frame,
each under two tinted lights. Beside it, on the same buffers and in the same run, par_quantize_device (index plane only,
spread 0, the same palette): pattern at depth N does N of quantise's searches plus the error update and the sort, so the
figure it is held against is N times quantise, and `ratio_N` is T_pattern(N) / (N * T_quantize). After a warm-up of every
call, batches of back-to-back launches between two events on one stream; the median batch over its launch count, the
fastest and the slowest (`spread` is (slowest - fastest) / median: what a difference has to exceed). A batch is sized to
last a few milliseconds at least. The palette is the frame's fitted palette, refined two rounds. Prints one JSON line and
writes it to --out (default profiles/pattern_dither.json).
   python tools/pattern.py [--batches N] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from measure_palette_fit import FRAMES, TINTS  # noqa: E402

DEPTHS = (1, 4, 8, 16)


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
    us = statistics.median(spans)
    return {"us": round(us, 2), "us_min": round(min(spans), 2), "us_max": round(max(spans), 2),
            "spread": round((max(spans) - min(spans)) / us, 3), "per_batch": per_batch}


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
    refine_work = torch.zeros(T.PALETTE_REFINE_WORK.itemsize, dtype=torch.uint8, device="cuda")
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
    f, w, p, rows = fb.data_ptr(), work.data_ptr(), palette.data_ptr(), (0, H)
    out = {"frame": name, "pixels": n}
    big = n > 1 << 20
    for n_colors in (33, 256):
        par.palette_reset(w, stream=s)
        par.palette_count(params, f, rows, w, stream=s)
        par.palette_cut(w, n_colors, stream=s)
        par.palette_sum(params, f, rows, w, stream=s)
        par.palette_emit(w, n_colors, p, stream=s)
        par.palette_refine_device(params, f, rows, p, n_colors, 2, index.data_ptr(), refine_work.data_ptr(), None, stream=s)
        stream.synchronize()
        q = timed(stream, lambda: par.quantize(params, p, n_colors, f, rows, index_out=index.data_ptr(), stream=s), batches,
                  20 if big else 200)
        out[f"quantize_{n_colors}"] = q
        for depth in DEPTHS:
            # a batch of a few milliseconds at least, and of a few hundred at most
            per = max(2, (20 if big else 200) // depth)
            t = timed(stream, lambda: par.quantize_pattern(params, p, n_colors, f, rows, depth, 256,
                                                           index_out=index.data_ptr(), stream=s), batches, per)
            t["ratio"] = round(t["us"] / (depth * q["us"]), 3)
            out[f"pattern_{n_colors}_{depth}"] = t
        # quantise once more behind the pattern calls: how far the yardstick itself moves within the run
        again = timed(stream, lambda: par.quantize(params, p, n_colors, f, rows, index_out=index.data_ptr(), stream=s),
                      batches, 20 if big else 200)
        out[f"quantize_{n_colors}_again"] = again
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pattern_dither.json"))
    a = ap.parse_args()
    result = {"tool": "pattern", "batches": a.batches, "depths": list(DEPTHS), "strength": 256,
              "frames": [measure(name, a.batches) for name in FRAMES]}
    line = json.dumps(result)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
