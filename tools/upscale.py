"""Microseconds per par_upscale_device call in device buffers: fb and index sources x Scale2x, Scale3x and Scale4x, on a
480 x 320 frame and on a 4096 x 4096 frame (whose Scale4x output is 1 GiB). The method is tools/present.py's: after a
warm-up, 20 batches of 12 back-to-back launches between two events on one stream; the median batch over its launch count.
Tight pitch, RGBA order, a 33-entry palette, the surface only (no index_out). The planes are drawn from three values, so
that the rules have edges to act on. Beside each figure the two yardsticks of DESIGN "Upscale": par_present_device at
(k, k) from the same source, which writes the same bytes, measured in the same visit in batches that alternate with the
upscale's; and the bytes the call must move (written plus read) at 5.7 TB/s (DESIGN section 5's fill). Prints one JSON line.
   python tools/upscale.py [--batches N] [--sizes 480x320,4096x4096]

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

FACTORS = (2, 3, 4)
STEP_SECONDS = 240
HBM_BYTES_PER_US = 5.7e6  # 5.7 TB/s
PER_BATCH = 12


def bound_us(w, h, k, source):
    return round((4 * w * k * h * k + w * h * (4 if source == "fb" else 1)) / HBM_BYTES_PER_US, 2)


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
    gen = torch.Generator(device="cuda").manual_seed(1)
    pick = torch.randint(0, 3, (n,), dtype=torch.uint8, device="cuda", generator=gen)
    index = pick * 7
    colours = torch.tensor([[200, 40, 30, 0], [30, 180, 90, 0], [20, 60, 220, 255]], dtype=torch.uint8, device="cuda")
    fb = colours[pick.long()].reshape(-1).contiguous()
    palette = par.palette_ramp(T.default_params(), 8)
    d_palette = torch.from_numpy(palette.view(np.uint8).copy()).cuda()
    out = torch.zeros(4 * n * max(FACTORS) ** 2, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    rows = []
    for source in ("fb", "index"):
        for k in FACTORS:
            up, pr = T.make_upscale_desc(k, width=w), T.make_present_desc(k, k, width=w)
            if source == "fb":
                def upscale():
                    par.upscale(params, up, out.data_ptr(), (0, h), fb=fb.data_ptr(), stream=stream.cuda_stream)

                def present():
                    par.present(params, pr, out.data_ptr(), (0, h), fb=fb.data_ptr(), stream=stream.cuda_stream)
            else:
                def upscale():
                    par.upscale(params, up, out.data_ptr(), (0, h), index=index.data_ptr(), d_palette=d_palette.data_ptr(),
                                n_colors=len(palette), stream=stream.cuda_stream)

                def present():
                    par.present(params, pr, out.data_ptr(), (0, h), index=index.data_ptr(), d_palette=d_palette.data_ptr(),
                                n_colors=len(palette), stream=stream.cuda_stream)
            for _ in range(PER_BATCH):
                upscale()
                present()
            stream.synchronize()
            ours, theirs = [], []
            for _ in range(batches):
                ours.append(batch_us(stream, upscale))
                theirs.append(batch_us(stream, present))
            us, present_us, bound = statistics.median(ours), statistics.median(theirs), bound_us(w, h, k, source)
            rows.append({"size": f"{w}x{h}", "source": source, "k": k, "us": round(us, 2), "us_min": round(min(ours), 2),
                         "present_us": round(present_us, 2), "bound_traffic_us": bound,
                         "over_present": round(us / present_us, 2), "over_bound": round(us / bound, 2)})
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
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", size, "--batches", str(a.batches)],
                           capture_output=True, text=True, timeout=STEP_SECONDS)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            print(json.dumps({"tool": "upscale", "failed_at_size": size, "status": p.returncode, "rows": table}))
            return 1
        table += json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps({"tool": "upscale", "batches": a.batches, "per_batch": PER_BATCH, "rows": table}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
