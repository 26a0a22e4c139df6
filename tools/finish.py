"""Microseconds per par_finish_device call against the chain of the three calls it replaces, in device buffers: the
stage sets {outline + quantise, outline only, quantise only} x the scales (1,1), (3,3), (4,4), on a 480 x 320 and on a
4096 x 4096 frame (the G-buffer and frame of the rendered 1024-primitive benchmark scene, as tools/outline.py makes
them). The 33-entry ramp, spread 32, style (4, 128, 320), tight pitch, RGBA order. After a warm-up, 20 batches of 12
back-to-back calls between two events on one stream, the batches of the two alternating in the same visit; the median
batch over its call count.
  fused: one par_finish_device, no index plane asked for.
  chain: par_outline_device in place, par_quantize_device to an index plane, par_present_device from the index plane
         (outline only: outline in place, present from fb; quantise only: quantize, present). In place the frame darkens
         from call to call, which no kernel's time depends on.
Beside each pair their ratio, the chain's min and max over its batches, and the traffic bound of the fused call: the bytes
it must move (28 B a texel times the halo's amplification of the tile, 66 * 18 / (64 * 16), where outlined; 4 B of fb;
4 * sx * sy B of surface) at 5.7 TB/s (DESIGN section 5's fill). Prints one JSON line.
   python tools/finish.py [--batches N] [--sizes 480x320,4096x4096]

Each size is measured in a child process of its own under a time limit; the first child that fails or runs out of time
ends the run (nothing is tried again)."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALES = ((1, 1), (3, 3), (4, 4))
STAGE_SETS = ("outline+quantise", "outline", "quantise")
STEP_SECONDS = 240
HBM_BYTES_PER_US = 5.7e6  # 5.7 TB/s
HALO = (64 + 2) * (16 + 2) / (64 * 16)  # texels fetched per pixel by the kernel's tile
PER_BATCH = 12
STYLE = (4, 128, 320)  # depth step, silhouette scale, crease scale
SPREAD = 32


def bound_us(pixels, sx, sy, outlined):
    return round(pixels * ((28 * HALO if outlined else 0) + 4 + 4 * sx * sy) / HBM_BYTES_PER_US, 2)


def batch_us(stream, call):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(PER_BATCH):
        call()
    e1.record(stream)
    e1.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / PER_BATCH


def measure(w, h, batches):
    import numpy as np
    import torch
    par = importlib.import_module("pixel-art-raytracer_amd")
    T = importlib.import_module("pixel-art-raytracer_amd.types")
    params = T.default_params(w, h, h)
    n = w * h
    style = T.make_outline_style(*STYLE)
    aabbs, light = par.scene_synthetic(1024, w, h, h, 12345)
    gbuf = torch.zeros(n * 28, dtype=torch.uint8, device="cuda")
    fb = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    index = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = torch.zeros(4 * n * max(sx * sy for sx, sy in SCALES), dtype=torch.uint8, device="cuda")
    palette = par.palette_ramp(T.default_params(), 8)
    d_palette = torch.from_numpy(palette.view(np.uint8).copy()).cuda()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    torch.cuda.synchronize()
    with par.Renderer(params, 0) as r:
        r.set_scene(aabbs, par.tile_floor(), light)
        r.render_device({"gbuf": gbuf.data_ptr(), "fb": fb.data_ptr()}, stream=s)
        stream.synchronize()
    rows = []
    for stages in STAGE_SETS:
        outlined, quantised = "outline" in stages, "quantise" in stages
        for sx, sy in SCALES:
            desc = T.make_present_desc(sx, sy, width=w)

            def fused():
                par.finish(params, desc, out.data_ptr(), (0, h), fb.data_ptr(), style=style if outlined else None,
                           gbuf=gbuf.data_ptr() if outlined else None,
                           d_palette=d_palette.data_ptr() if quantised else None,
                           n_colors=len(palette) if quantised else 0, spread=SPREAD if quantised else 0, stream=s)

            def chain():
                if outlined:
                    par.outline(params, style, gbuf.data_ptr(), (0, h), fb.data_ptr(), (0, h), fb_out=fb.data_ptr(), stream=s)
                if quantised:
                    par.quantize(params, d_palette.data_ptr(), len(palette), fb.data_ptr(), (0, h),
                                 index_out=index.data_ptr(), spread=SPREAD, stream=s)
                    par.present(params, desc, out.data_ptr(), (0, h), index=index.data_ptr(),
                                d_palette=d_palette.data_ptr(), n_colors=len(palette), stream=s)
                else:
                    par.present(params, desc, out.data_ptr(), (0, h), fb=fb.data_ptr(), stream=s)

            for _ in range(PER_BATCH):
                fused()
                chain()
            stream.synchronize()
            a, b = [], []
            for _ in range(batches):
                a.append(batch_us(stream, fused))
                b.append(batch_us(stream, chain))
            fused_us, chain_us = statistics.median(a), statistics.median(b)
            rows.append({"size": f"{w}x{h}", "stages": stages, "scale": [sx, sy], "fused_us": round(fused_us, 2),
                         "chain_us": round(chain_us, 2), "ratio": round(fused_us / chain_us, 3),
                         "fused_min_max_us": [round(min(a), 2), round(max(a), 2)],
                         "chain_min_max_us": [round(min(b), 2), round(max(b), 2)],
                         "bound_traffic_us": bound_us(n, sx, sy, outlined)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--sizes", default="480x320,4096x4096")
    ap.add_argument("--one", default="", help="(internal) measure this size in this process")
    a = ap.parse_args()
    if a.one:
        w, h = (int(v) for v in a.one.split("x"))
        print(json.dumps(measure(w, h, a.batches)))
        return 0
    table = []
    for size in a.sizes.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", size, "--batches", str(a.batches)],
                               capture_output=True, text=True, timeout=STEP_SECONDS)
        except subprocess.TimeoutExpired as e:
            sys.stderr.write(f"{size}: no result within {STEP_SECONDS} s\n")
            for part in (e.stdout, e.stderr):
                if part:
                    sys.stderr.write(part if isinstance(part, str) else part.decode(errors="replace"))
            print(json.dumps({"tool": "finish", "failed_at_size": size, "status": "timeout", "rows": table}))
            return 1
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            print(json.dumps({"tool": "finish", "failed_at_size": size, "status": p.returncode, "rows": table}))
            return 1
        table += json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps({"tool": "finish", "batches": a.batches, "per_batch": PER_BATCH, "halo": round(HALO, 3), "rows": table}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
