"""Microseconds per frame with N = 1, 2, 4, 8 lights (par_set_lights) on the graybox world at 480x320 and on the 4096^2
view with 1024 primitives: one frame alone (par_render_device_timed, the span of its launches, median) and four frames
in flight (par_render_device_slots, wall time per frame). Also N = 1 forced through the light kernel (test hook
lights_path) and through the overflow kernel on every column (force_generic), the two paths whose walks it replaces.
Prints one JSON line.   python tools/lights.py [frames]

With --radius F every light is ranged (PAR_LIGHTS_RANGED, par_set_light_model) with radius F x the view's width; with
--torches F light 0 stays a sun (radius 0) and the other N - 1 are such torches. Then N = 2, 4, 8 are timed, in the
same table, each with the (start bin, light) pairs the light kernel walked and culled in one frame.
With --tints every light has a colour (par_set_light_tints, the eight non-white tints below), alone or beside --radius /
--torches: the same table through the tinted light kernels (N = 1 takes the light kernel too; the two N = 1 hook rows
are left out).
With --relight (alone or beside --radius / --torches / --tints) full frames and relit frames (par_relight_device) of
the same lights are timed in turn, full, relit, full, relit, for N = 1, 2, 4, 8: "alone" is the span of the frame's
launches between two events on its stream (the full frame's also as par_render_device_timed gives it, as in the other
tables), "inflight4" is wall time per frame with four contexts, each with its retained frame, on four streams, relit
round robin. Full frames write fb and palidx, relit frames fb; the G-buffer they read is written once, before.
   python tools/lights.py [frames] [--radius F | --torches F] [--tints] [--relight]
                          [--scene graybox_480x320 | synthetic_4096_1024]"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

par = importlib.import_module("pixel-art-raytracer_amd")
T = importlib.import_module("pixel-art-raytracer_amd.types")
pipeline = importlib.import_module("pixel-art-raytracer_amd.pipeline")

FRACTIONS = [(5 / 8, 1 / 2, 1 / 4), (1 / 8, 3 / 4, 1 / 16), (15 / 16, 1 / 16, 7 / 8), (1 / 2, 3 / 8, 1 / 2),
             (1 / 4, 1 / 4, 3 / 4), (3 / 4, 5 / 8, 1 / 8), (1 / 16, 1 / 8, 1 / 2), (7 / 8, 7 / 8, 15 / 16)]
# --tints: a warm torch, a cold moon, components above 1, a zero component; none white, none black
TINTS = [(1, .5, .125), (.25, .5, 1.5), (2, 1.5, 1), (0, 1, .5), (.5, 1, .25), (1.5, 0, .75), (.125, .125, 1), (3, .5, 0)]
TINTED = False  # (main sets it)


def lights_for(params, n, radius=None, sun=False):
    """`radius` (a fraction of the view's width): ranged lights; `sun`: light 0 keeps radius 0."""
    a = np.zeros(n, dtype=T.LIGHT)
    for i, (fx, fy, fz) in enumerate(FRACTIONS[:n]):
        a[i]["x"], a[i]["y"], a[i]["z"] = int(params.width * fx), int(params.height * fy), int(params.length * fz)
        a[i]["radius"] = 10 if radius is None else (0 if sun and i == 0 else min(32767, max(1, int(params.width * radius))))
    return a


def configure(r, lights, mode):
    r.set_light_model(par.LIGHTS_RANGED if mode == "ranged" else par.LIGHTS_UNBOUNDED)
    r.set_lights(lights)
    r.set_light_tints(T.make_tints(TINTS[:len(lights)]) if TINTED else None)
    r.set_test_hooks(lights_path=(mode == "kernel"), force_generic=(mode == "generic"))


def pair_counts(params, aabbs, sprite, lights):
    """(walked, culled) pairs of one ranged frame."""
    with par.Renderer(params, 0) as r:
        r.set_scene(aabbs, sprite, lights[0:1])
        configure(r, lights, "ranged")
        r.render(("fb",), flags=par.RENDER_COUNT_RAYS)
        return r.light_walks()


def alone_us(params, aabbs, sprite, lights, mode, frames):
    with par.Renderer(params, 0) as r:
        r.set_scene(aabbs, sprite, lights[0:1])
        configure(r, lights, mode)
        fb = torch.zeros(params.width * params.height * 4, dtype=torch.uint8, device="cuda")
        pal = torch.zeros(params.width * params.height, dtype=torch.uint8, device="cuda")
        ptrs = {"fb": fb.data_ptr(), "palidx": pal.data_ptr()}
        spans = []
        for i in range(frames + 3):
            st = r.render_device(ptrs, timed=True, flags=par.RENDER_TIMED_AS_LAUNCHED)
            if i >= 3:
                spans.append(1000.0 * sum(v for v in st.ms_launch if v > 0))
        return round(statistics.median(spans), 1)


def inflight_us(params, aabbs, sprite, lights, mode, frames):
    pipe = pipeline.FramePipeline(params, aabbs, sprite, lights[0:1], depth=4)
    try:
        for s in pipe.slots:
            configure(s.renderer, lights, mode)
        pipe.submit_many(0, 8)
        pipe.synchronize()
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            pipe.submit_many(0, frames)
            pipe.synchronize()
            us = (time.perf_counter() - t0) * 1e6 / frames
            best = us if best is None else min(best, us)
        for s in pipe.slots:
            s.renderer.stats()  # PAR_ERR_DEVICE raises
        return round(best, 1)
    finally:
        pipe.close()


def bracket_us(stream, frames, enqueue):
    """Median span of `enqueue()`'s launches on `stream`, one frame at a time, between two events."""
    spans = []
    for i in range(frames + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        enqueue()
        e1.record(stream)
        e1.synchronize()
        if i >= 3:
            spans.append(1000.0 * e0.elapsed_time(e1))
    return round(statistics.median(spans), 1)


def relight_call(r, stream, gbuf, fb):
    """par_relight_device of the whole view into `fb`, its arguments built once."""
    out = T.Outputs(fb.data_ptr(), None, None, None, None)
    args = (r._ctx, ctypes.c_void_p(stream.cuda_stream), 0, r.height, ctypes.c_void_p(gbuf.data_ptr()), ctypes.byref(out), 0)
    fn = par.lib().par_relight_device

    def call():
        rc = fn(*args)
        if rc != 0:
            raise par.ParError(rc, par.lib().par_last_error(r._ctx).decode())
    call.keep = out
    return call


def relight_alone(params, aabbs, sprite, lights, mode, frames, rounds=2):
    n_px = params.width * params.height
    with par.Renderer(params, 0) as r:
        r.set_scene(aabbs, sprite, lights[0:1])
        configure(r, lights, mode)
        stream = torch.cuda.Stream()
        fb = torch.zeros(n_px * 4, dtype=torch.uint8, device="cuda")
        pal = torch.zeros(n_px, dtype=torch.uint8, device="cuda")
        gbuf = torch.zeros(n_px * 28, dtype=torch.uint8, device="cuda")
        ptrs = {"fb": fb.data_ptr(), "palidx": pal.data_ptr()}
        r.render_device(dict(ptrs, gbuf=gbuf.data_ptr()), stream=stream.cuda_stream)
        stream.synchronize()
        relit = relight_call(r, stream, gbuf, fb)
        res = {"full_timed": [], "full": [], "relit": []}
        for _ in range(rounds):
            spans = []
            for i in range(frames + 3):
                st = r.render_device(ptrs, timed=True, flags=par.RENDER_TIMED_AS_LAUNCHED, stream=stream.cuda_stream)
                if i >= 3:
                    spans.append(1000.0 * sum(v for v in st.ms_launch if v > 0))
            res["full_timed"].append(round(statistics.median(spans), 1))
            res["full"].append(bracket_us(stream, frames, lambda: r.render_device(ptrs, stream=stream.cuda_stream)))
            res["relit"].append(bracket_us(stream, frames, relit))
        r.stats()  # PAR_ERR_DEVICE raises
        return res


def relight_inflight(params, aabbs, sprite, lights, mode, frames, rounds=2):
    n_px = params.width * params.height
    pipe = pipeline.FramePipeline(params, aabbs, sprite, lights[0:1], depth=4)
    try:
        calls = []
        for s in pipe.slots:
            configure(s.renderer, lights, mode)
            gbuf = torch.zeros(n_px * 28, dtype=torch.uint8, device="cuda")
            s.renderer.render_device(dict(s.ptrs, gbuf=gbuf.data_ptr()), stream=s.stream.cuda_stream)
            calls.append(relight_call(s.renderer, s.stream, gbuf, s.buffers["fb"]))
        pipe.synchronize()

        def full(n):
            pipe.submit_many(0, n)

        def relit(n):
            for f in range(n):
                calls[f % 4]()

        res = {"full": [], "relit": []}
        for _ in range(rounds):
            for name, submit in (("full", full), ("relit", relit)):
                submit(8)
                pipe.synchronize()
                best = None
                for _ in range(3):
                    t0 = time.perf_counter()
                    submit(frames)
                    pipe.synchronize()
                    us = (time.perf_counter() - t0) * 1e6 / frames
                    best = us if best is None else min(best, us)
                res[name].append(round(best, 1))
        for s in pipe.slots:
            s.renderer.stats()  # PAR_ERR_DEVICE raises
        return res
    finally:
        pipe.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("frames", nargs="?", type=int, default=40)
    ap.add_argument("--radius", type=float, help="every light ranged, radius = this fraction of the view's width")
    ap.add_argument("--torches", type=float, help="one sun and N - 1 torches of that radius")
    ap.add_argument("--tints", action="store_true", help="every light tinted (par_set_light_tints)")
    ap.add_argument("--relight", action="store_true", help="full frames against relit frames (par_relight_device)")
    ap.add_argument("--scene", help="one scene only")
    args = ap.parse_args()
    global TINTED
    TINTED = args.tints
    frames = args.frames
    radius = args.radius if args.radius is not None else args.torches
    sprite = par.tile_floor()
    scenes = {}
    p = T.default_params()
    scenes["graybox_480x320"] = (p, par.scene_graybox(480, 320))
    p = T.default_params(4096, 4096, 4096)
    scenes["synthetic_4096_1024"] = (p, par.scene_synthetic(1024, 4096, 4096, 4096, 12345)[0])
    out = {"tool": "lights", "frames": frames, "us_per_frame": {}}
    if args.tints:
        out["tints"] = True
    if args.relight:
        out["relight"] = True
    if radius is not None:
        out["radius" if args.radius is not None else "torches"] = radius
    for name, (params, aabbs) in scenes.items():
        if args.scene and name != args.scene:
            continue
        res = {}
        if args.relight:
            for n in (1, 2, 4, 8):
                lights = lights_for(params, n, radius, sun=radius is not None and args.radius is None)
                mode = "ranged" if radius is not None else "auto"
                res[f"n{n}"] = {"alone": relight_alone(params, aabbs, sprite, lights, mode, frames),
                                "inflight4": relight_inflight(params, aabbs, sprite, lights, mode, frames)}
            out["us_per_frame"][name] = res
            continue
        if radius is not None:
            for n in (2, 4, 8):
                lights = lights_for(params, n, radius, sun=args.radius is None)
                walked, culled = pair_counts(params, aabbs, sprite, lights)
                res[f"n{n}"] = {"alone": alone_us(params, aabbs, sprite, lights, "ranged", frames),
                                "inflight4": inflight_us(params, aabbs, sprite, lights, "ranged", frames),
                                "pairs_walked": walked, "pairs_culled": culled}
            out["us_per_frame"][name] = res
            continue
        for n in (1, 2, 4, 8):
            lights = lights_for(params, n)
            res[f"n{n}"] = {"alone": alone_us(params, aabbs, sprite, lights, "auto", frames),
                            "inflight4": inflight_us(params, aabbs, sprite, lights, "auto", frames)}
        lights = lights_for(params, 1)
        for mode in () if args.tints else ("kernel", "generic"):
            res[f"n1_{mode}"] = {"alone": alone_us(params, aabbs, sprite, lights, mode, frames),
                                 "inflight4": inflight_us(params, aabbs, sprite, lights, mode, frames)}
        out["us_per_frame"][name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
