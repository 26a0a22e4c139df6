"""Microseconds per par_present_device call in device buffers: fb and index sources x the scales (1,1), (2,2), (3,3),
(4,4), on a 480 x 320 frame (there (16,16) too) and on a 4096 x 4096 frame (which stops at (4,4): that output is 1 GiB
already). After a warm-up, 20 batches of 12 back-to-back launches between two events on one stream; the median batch
over its launch count. Tight pitch, RGBA order, a 33-entry palette. Beside each figure the two yardsticks of DESIGN
"Present": the bytes the call must move (written plus read) at 5.7 TB/s (DESIGN section 5's fill), and, for scale (1,1)
with an fb source, a device-to-device hipMemcpyAsync of the same bytes, measured in the same visit in batches that
alternate with the kernel's. Prints one JSON line.
   python tools/present.py [--batches N] [--sizes 480x320,4096x4096]

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

SCALES = ((1, 1), (2, 2), (3, 3), (4, 4))
STEP_SECONDS = 240
HBM_BYTES_PER_US = 5.7e6  # 5.7 TB/s
PER_BATCH = 12


def bound_us(w, h, sx, sy, source):
    return round((4 * w * sx * h * sy + w * h * (4 if source == "fb" else 1)) / HBM_BYTES_PER_US, 2)


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
    scales = SCALES + (((16, 16),) if n <= 480 * 320 else ())
    gen = torch.Generator(device="cuda").manual_seed(1)
    fb = torch.randint(0, 256, (n * 4,), dtype=torch.uint8, device="cuda", generator=gen)
    index = torch.randint(0, 33, (n,), dtype=torch.uint8, device="cuda", generator=gen)
    palette = par.palette_ramp(T.default_params(), 8)
    d_palette = torch.from_numpy(palette.view(np.uint8).copy()).cuda()
    out = torch.zeros(4 * n * max(sx * sy for sx, sy in scales), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    copy_to = torch.empty_like(fb)
    hip = par.hip_runtime()
    device_to_device = 3  # hipMemcpyDeviceToDevice
    torch.cuda.synchronize()
    rows = []
    for source in ("fb", "index"):
        for sx, sy in scales:
            desc = T.make_present_desc(sx, sy, width=w)
            if source == "fb":
                def call():
                    par.present(params, desc, out.data_ptr(), (0, h), fb=fb.data_ptr(), stream=stream.cuda_stream)
            else:
                def call():
                    par.present(params, desc, out.data_ptr(), (0, h), index=index.data_ptr(),
                                d_palette=d_palette.data_ptr(), n_colors=len(palette), stream=stream.cuda_stream)
            copy = None
            if source == "fb" and (sx, sy) == (1, 1):
                def copy():
                    rc = hip.hipMemcpyAsync(copy_to.data_ptr(), fb.data_ptr(), 4 * n, device_to_device, stream.cuda_stream)
                    assert rc == 0, rc
            for _ in range(PER_BATCH):
                call()
                if copy:
                    copy()
            stream.synchronize()
            spans, copies = [], []
            for _ in range(batches):
                spans.append(batch_us(stream, call))
                if copy:
                    copies.append(batch_us(stream, copy))
            row = {"size": f"{w}x{h}", "source": source, "scale": [sx, sy], "us": round(statistics.median(spans), 2),
                   "us_min": round(min(spans), 2), "bound_traffic_us": bound_us(w, h, sx, sy, source)}
            if copy:
                row["copy_us"] = round(statistics.median(copies), 2)
            rows.append(row)
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
            print(json.dumps({"tool": "present", "failed_at_size": size, "status": p.returncode, "rows": table}))
            return 1
        table += json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps({"tool": "present", "batches": a.batches, "per_batch": PER_BATCH, "rows": table}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
