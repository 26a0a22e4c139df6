"""Microseconds per round of par_palette_refine_device at 33 and at 256 entries on two rendered frames in device
buffers: the 4096 x 4096 headline frame and the 480 x 320 graybox frame, each under two tinted lights. Beside it, on the
same buffers and in the same run, par_quantize_device (index plane only, spread 0, the same palette) and
par_palette_sum_device: a round is one quantise and two passes shaped like sum plus two small launches, so the
expectation it is held against is 1.25 * (quantize + 2 * sum). After a warm-up of every call, batches of back-to-back
launches between two events on one stream; the median batch over its launch count, and the fastest. A batch is sized to
last a few milliseconds at least. The frame stays resident (one buffer), as it is directly after the render that made
it. `refine_N_1` is a call of one round (it includes the call's one zeroing of the tallies), `refine_N_4` a call of four
rounds over four. The palette is the frame's fitted palette before the first launch and moves towards its fixed point
under the timed launches; the work per round does not depend on it beyond which tallies the adds meet. Prints one JSON
line and writes it to --out (default profiles/palette_refine.json).
   python tools/measure_palette_refine.py [--batches N] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from measure_palette_fit import FRAMES, TINTS, timed  # noqa: E402


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
    changed = torch.zeros(1, dtype=torch.int32, device="cuda")
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

    def fit(n_colors):
        par.palette_reset(w, stream=s)
        par.palette_count(params, f, rows, w, stream=s)
        par.palette_cut(w, n_colors, stream=s)
        par.palette_sum(params, f, rows, w, stream=s)
        par.palette_emit(w, n_colors, p, stream=s)

    def refine(n_colors, rounds):
        par.palette_refine_device(params, f, rows, p, n_colors, rounds, index.data_ptr(), refine_work.data_ptr(),
                                  changed.data_ptr(), stream=s)

    out = {"frame": name, "pixels": n}
    # a batch of a few milliseconds at least: many launches of the small frame's short calls
    per = 20 if n > 1 << 20 else 200
    for n_colors in (33, 256):
        fit(n_colors)
        out[f"quantize_{n_colors}"] = timed(
            stream, lambda: par.quantize(params, p, n_colors, f, rows, index_out=index.data_ptr(), stream=s), batches, per)
        out[f"sum_{n_colors}"] = timed(stream, lambda: par.palette_sum(params, f, rows, w, stream=s), batches, per)
        fit(n_colors)
        out[f"refine_{n_colors}_1"] = timed(stream, lambda: refine(n_colors, 1), batches, per)
        fit(n_colors)
        four = timed(stream, lambda: refine(n_colors, 4), batches, max(4, per // 4))
        out[f"refine_{n_colors}_4"] = {"us": round(four["us"] / 4, 2), "us_min": round(four["us_min"] / 4, 2),
                                       "per_batch": four["per_batch"], "rounds": 4}
        stream.synchronize()
        out[f"changed_after_{n_colors}"] = int(changed.cpu()[0])
        expect = 1.25 * (out[f"quantize_{n_colors}"]["us"] + 2 * out[f"sum_{n_colors}"]["us"])
        out[f"expected_{n_colors}"] = round(expect, 2)
        out[f"round_over_expected_{n_colors}"] = round(out[f"refine_{n_colors}_4"]["us"] / expect, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "palette_refine.json"))
    a = ap.parse_args()
    result = {"tool": "measure_palette_refine", "batches": a.batches, "frames": [measure(name, a.batches) for name in FRAMES]}
    line = json.dumps(result)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
