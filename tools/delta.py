"""What the changed-tiles path costs, on the device and end to end, against the strongest way to get a frame into host
memory without it: one hipMemcpyAsync of the fb plane into pinned memory and a synchronise, measured in the same visit.
Sizes 480 x 320 (the graybox scene, aabbs[0] moving) and 4096 x 4096 (the 1024-primitive benchmark scene, entity 0
moving); bin size 40. After a warm-up, 20 batches of 12 back-to-back calls, the alternatives' batches alternating; the
median batch over its call count, with the min and max over the batches beside it.
  device:  par_tiles_changed_device + par_tiles_pack_counted between two events on one stream, for the rendered pair of
           frames and for synthetic flips of 1 %, 10 %, 50 % and 100 % of the tiles (one pixel a tile); beside it the
           traffic bound of two plane reads at 6 TB/s, and the same calls after a 512 MiB fill on the same stream has
           pushed both planes out of the Infinity Cache (the fill's own time, measured alone, is subtracted).
  host:    wall clock of FrameDelta.update (changed -> pack_counted -> fetch -> apply, capacity = the whole grid) against
           the full pinned copy, same scenes and flips. `wins` says whether the delta path's median lies below the copy's
           median by more than the copy's own spread (max - min over its batches).
--elem-bytes 1 or 28 measures the same on the palidx plane or the G-buffer through the par_plane_tiles_* calls (the
plane is the rendered one, a flip changes one byte of one element, the copy it is held against is that plane's), and
--elem-bytes 4 --plane-calls sends the fb plane through them, to be read beside the rows of the 4-byte calls. Every row
names its element size and its calls.
Prints one JSON line and writes it to profiles/delta.json (or --out).
   python tools/delta.py [--batches N] [--sizes 480x320,4096x4096] [--fractions 0.01,0.1,0.5,1.0] [--out delta.json]
                         [--elem-bytes 1|4|28] [--plane-calls]

Each size is measured in a child process of its own under a time limit; the first child that fails or runs out of time
ends the run (nothing is tried again)."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_SECONDS = 300
PER_BATCH = 12
HBM_BYTES_PER_US = 6.0e6  # 6 TB/s streaming reads
FRACTIONS = (0.01, 0.1, 0.5, 1.0)
EVICT_BYTES = 512 << 20


def stats(v):
    return {"us": round(statistics.median(v), 2), "min_max_us": [round(min(v), 2), round(max(v), 2)]}


PLANES = {1: "palidx", 4: "fb", 28: "gbuf"}


def measure(w, h, batches, fractions, e=4, plane_calls=False):
    import numpy as np
    import torch
    par = importlib.import_module("pixel-art-raytracer_amd")
    T = importlib.import_module("pixel-art-raytracer_amd.types")
    FD = importlib.import_module("pixel-art-raytracer_amd.delta")
    params = T.default_params(w, h, h)
    gx, gy, _ = params.grid_dims()
    grid, b = gx * gy, params.bin_size
    n = w * h
    if (w, h) == (480, 320):
        aabbs, light, scene = par.scene_graybox(w, h), T.make_light(480, 160, 80), "graybox, aabbs[0] moving"
    else:
        aabbs, light = par.scene_synthetic(1024, w, h, h, 12345)
        scene = "1024 primitives, entity 0 moving"
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    plane = PLANES[e]
    plane_calls = plane_calls or e != 4
    prev = torch.zeros(e * n, dtype=torch.uint8, device="cuda")
    cur = torch.zeros(e * n, dtype=torch.uint8, device="cuda")
    evict = torch.zeros(EVICT_BYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with par.Renderer(params, 0) as r:
        r.set_scene(aabbs, par.tile_floor(), light)
        r.render_device({plane: prev.data_ptr()}, stream=s)
        moved = aabbs[:1].copy()
        moved["px"] += 5
        stream.synchronize()
        r.update_aabbs(moved, 0)
        r.render_device({plane: cur.data_ptr()}, stream=s)
        stream.synchronize()
    rendered = cur.clone()
    base = prev.cpu().numpy()
    delta = FD.FrameDelta(params, capacity=grid, elem_bytes=e)
    if plane_calls and e == 4:  # the fb plane through the plane calls, FrameDelta's four calls with it
        delta._changed, delta._pack_counted, delta._fetch, delta._apply = (
            FD._sized(f, 4) for f in (par.plane_tiles_changed, par.plane_tiles_pack_counted, par.plane_tiles_fetch,
                                      par.plane_tiles_apply_host))
    full = torch.zeros(e * n, dtype=torch.uint8).pin_memory()

    def device_calls():
        if plane_calls:
            par.plane_tiles_changed(params, e, prev.data_ptr(), cur.data_ptr(), (0, h), delta._d_map.data_ptr(),
                                    delta._d_tiles.data_ptr(), grid, delta._d_count.data_ptr(), s)
            par.plane_tiles_pack_counted(params, e, delta._d_tiles.data_ptr(), delta._d_count.data_ptr(), grid,
                                         cur.data_ptr(), (0, h), delta._d_packed.data_ptr(), s)
            return
        par.tiles_changed(params, prev.data_ptr(), cur.data_ptr(), (0, h), delta._d_map.data_ptr(),
                          delta._d_tiles.data_ptr(), grid, delta._d_count.data_ptr(), s)
        par.tiles_pack_counted(params, delta._d_tiles.data_ptr(), delta._d_count.data_ptr(), grid, cur.data_ptr(), (0, h),
                               delta._d_packed.data_ptr(), s)

    def fill():
        with torch.cuda.stream(stream):
            evict.fill_(1)

    def events(call, per_batch=PER_BATCH):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(per_batch):
            call()
        e1.record(stream)
        e1.synchronize()
        return 1000.0 * e0.elapsed_time(e1) / per_batch

    def wall(call):
        stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(PER_BATCH):
            call()
        return 1e6 * (time.perf_counter() - t0) / PER_BATCH

    def full_copy():
        FD._copy_to_host(full.data_ptr(), cur.data_ptr(), e * n, s)

    def update():
        return delta.update(prev.data_ptr(), cur.data_ptr(), s)

    def filled_then_calls():
        fill()
        device_calls()

    cases = [(scene, None)] + [(f"flips in {round(100 * f, 1):g} % of the tiles", f) for f in fractions]
    rows = []
    rng = np.random.default_rng(1)
    for name, fraction in cases:
        if fraction is None:
            cur.copy_(rendered)
        else:
            picked = rng.permutation(grid)[:max(1, int(round(fraction * grid)))]
            frame = base.copy().reshape(h, w, e)
            frame[(picked // gx) * b, (picked % gx) * b, min(2, e - 1)] ^= np.uint8(1)  # one byte of one element a tile
            cur.copy_(torch.from_numpy(frame.reshape(-1)).cuda())
        torch.cuda.synchronize()
        for _ in range(PER_BATCH):
            device_calls()
            full_copy()
        count, fell_back = update()
        assert not fell_back
        dev, cold, fill_only, copy_us, delta_us = [], [], [], [], []
        for _ in range(batches):
            dev.append(events(device_calls))
            cold.append(events(filled_then_calls, 4))
            fill_only.append(events(fill, 4))
            copy_us.append(wall(full_copy))
            delta_us.append(wall(update))
        c, d = stats(copy_us), stats(delta_us)
        spread = c["min_max_us"][1] - c["min_max_us"][0]
        rows.append({"size": f"{w}x{h}", "elem_bytes": e, "plane": plane,
                     "calls": "par_plane_tiles_*" if plane_calls else "par_tiles_*", "case": name, "tiles": grid,
                     "changed": count,
                     "changed_share": round(count / grid, 4), "device": stats(dev),
                     "device_after_512MiB_fill_us": round(statistics.median(cold) - statistics.median(fill_only), 2),
                     "fill_us": round(statistics.median(fill_only), 2),
                     "bound_two_reads_us": round(2 * e * n / HBM_BYTES_PER_US, 2),
                     "full_pinned_copy": c, "delta_path": d, "copy_spread_us": round(spread, 2),
                     "wins": bool(d["us"] < c["us"] - spread)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--sizes", default="480x320,4096x4096")
    ap.add_argument("--fractions", default=",".join(str(f) for f in FRACTIONS))
    ap.add_argument("--out", default="delta.json", help="file name under profiles/")
    ap.add_argument("--elem-bytes", type=int, default=4, choices=sorted(PLANES),
                    help="1: the palidx plane, 28: the G-buffer (the plane calls); 4: the fb plane")
    ap.add_argument("--plane-calls", action="store_true", help="with --elem-bytes 4: the fb plane through the plane calls")
    ap.add_argument("--one", default="", help="(internal) measure this size in this process")
    a = ap.parse_args()
    if a.one:
        w, h = (int(v) for v in a.one.split("x"))
        print(json.dumps(measure(w, h, a.batches, [float(f) for f in a.fractions.split(",")], a.elem_bytes,
                                 a.plane_calls)))
        return 0
    table = []
    for size in a.sizes.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", size, "--batches", str(a.batches),
                                "--fractions", a.fractions, "--elem-bytes", str(a.elem_bytes)] +
                               (["--plane-calls"] if a.plane_calls else []),
                               capture_output=True, text=True, timeout=STEP_SECONDS)
        except subprocess.TimeoutExpired as e:
            sys.stderr.write(f"{size}: no result within {STEP_SECONDS} s\n")
            for part in (e.stdout, e.stderr):
                if part:
                    sys.stderr.write(part if isinstance(part, str) else part.decode(errors="replace"))
            print(json.dumps({"tool": "delta", "failed_at_size": size, "status": "timeout", "rows": table}))
            return 1
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            print(json.dumps({"tool": "delta", "failed_at_size": size, "status": p.returncode, "rows": table}))
            return 1
        table += json.loads(p.stdout.strip().splitlines()[-1])
    line = json.dumps({"tool": "delta", "batches": a.batches, "per_batch": PER_BATCH, "elem_bytes": a.elem_bytes,
                       "rows": table})
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", os.path.basename(a.out)), "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
