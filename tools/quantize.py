"""Microseconds per par_quantize_device call on a 4096 x 4096 frame in device buffers: n_colors in {4, 33, 256} x
spread in {0, 32} x {index only, index + fb_out}. After a warm-up, batches of back-to-back launches between two events
on one stream; the median batch over its launch count. The launches go round a ring of --ring buffer sets (source,
fb_out and index: 144 MiB a set), so that with the default of 4 no launch finds its frame in the 256 MiB Infinity
Cache, as a frame loop with frames in flight would not; --ring 1 quantises one resident frame over and over. Beside each
figure the two bounds DESIGN "Palette output" derives: the bytes the call must move at 5.7 TB/s (DESIGN section 5's
fill) and the search loop's vector instructions at four cycles each. Prints one JSON line.
   python tools/quantize.py [--batches N] [--size W] [--ring N]

Each palette size is measured in a child process of its own under a time limit; the first child that fails or runs out
of time ends the run (nothing is tried again)."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_COLORS = (4, 33, 256)
SPREADS = (0, 32)
STEP_SECONDS = 240
HBM_BYTES_PER_US = 5.7e6      # 5.7 TB/s
VALU_PER_PIXEL_ENTRY = 1.75   # the search loop's listing: 32 v_sad_hi_u8 + 16 v_min3_u32 + 8 v_mov_b32 per 4 pixels x 8 entries
SIMDS, CLOCK_MHZ = 1024, 2400.0


def bounds_us(pixels, n_colors, both):
    traffic = pixels * (4 + 1 + (4 if both else 0)) / HBM_BYTES_PER_US
    valu = VALU_PER_PIXEL_ENTRY * n_colors * pixels / 64 * 4 / (SIMDS * CLOCK_MHZ)
    return round(traffic, 1), round(valu, 1)


def measure(n_colors, size, batches, ring, per_batch=12):
    import numpy as np
    import torch
    par = importlib.import_module("pixel-art-raytracer_amd")
    T = importlib.import_module("pixel-art-raytracer_amd.types")
    params = T.default_params(size, size, size)
    n = size * size
    gen = torch.Generator(device="cuda").manual_seed(1)
    sets = [(torch.randint(0, 256, (n * 4,), dtype=torch.uint8, device="cuda", generator=gen),
             torch.zeros(n * 4, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"))
            for _ in range(ring)]
    turn = [0]
    if n_colors == 33:
        palette = par.palette_ramp(T.default_params(), 8)
    else:
        palette = np.random.default_rng(n_colors).integers(0, 256, n_colors * 4, dtype=np.uint8).view(T.COLOR)
    d_palette = torch.from_numpy(palette.view(np.uint8).copy()).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    rows = []
    for spread in SPREADS:
        for both in (False, True):
            def call():
                fb, fb_out, index = sets[turn[0] % ring]
                turn[0] += 1
                par.quantize(params, d_palette.data_ptr(), n_colors, fb.data_ptr(), (0, size),
                             fb_out=fb_out.data_ptr() if both else None, index_out=index.data_ptr(), spread=spread,
                             stream=stream.cuda_stream)
            for _ in range(2 * ring):
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
            traffic, valu = bounds_us(n, n_colors, both)
            rows.append({"n_colors": n_colors, "spread": spread, "planes": "index+fb_out" if both else "index",
                         "us": round(statistics.median(spans), 1), "us_min": round(min(spans), 1),
                         "bound_traffic_us": traffic, "bound_valu_us": valu})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--one", type=int, default=0, help="(internal) measure this palette size in this process")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(measure(a.one, a.size, a.batches, max(1, a.ring))))
        return 0
    table = []
    for n_colors in N_COLORS:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n_colors), "--size", str(a.size),
                            "--batches", str(a.batches), "--ring", str(a.ring)], capture_output=True, text=True,
                           timeout=STEP_SECONDS)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            print(json.dumps({"tool": "quantize", "failed_at_n_colors": n_colors, "status": p.returncode, "rows": table}))
            return 1
        table += json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps({"tool": "quantize", "size": a.size, "batches": a.batches, "ring": a.ring, "rows": table}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
