"""Microseconds per par_objects_draw_device and par_objects_from_maps_device (addons/include/par_objects.h), eagerly and as
graph replays, in one run on one stream:
  - the draw on the 480 x 320 screen with 40, 128 and 2400 objects (2400: one a cell), and on the 4096 x 4096 screen with
    an empty table (a device count of 0), with 128 objects and with 65536 objects of 8 x 8 on a grid, each beside
    par_screen_draw_device of the same screen (a map over the same tiles) and beside a device-to-device copy of the two
    planes, their batches alternating;
  - from_maps at 2400 and 2^18 cells with a third of the cells differing, beside par_tileset_extend_device's steady state
    over a plane of as many cells (every tile already stored).
Every draw is checked against the numpy model of tests/objects.py (its first CHECK_ROWS rows: a row depends on nothing but
its own number) before it is timed, and every table against the model's. Calls are made back to back on one stream, as a
frame loop makes them: after a warm-up, batches between two events; the median batch over its call count, the fastest and
the slowest (`spread` is (slowest - fastest) / median: what a difference has to exceed). A replay is a captured graph of
one batch's calls.
Prints one JSON line and writes it to --out (default profiles/objects.json).
   python tools/objects.py [--batches N] [--out FILE]"""
import argparse
import importlib
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pattern import timed  # noqa: E402

CHECK_ROWS = 64


def numpy_models():
    """tests/tileset.py, tests/vram.py, tests/screen.py and tests/objects.py, the contracts in numpy (by their paths: tools
    of those names exist; the later ones import the earlier ones by their plain names)."""
    out = {}
    for name in ("tileset", "vram", "screen", "objects"):
        spec = importlib.util.spec_from_file_location("tests_" + name, os.path.join(ROOT, "tests", name + ".py"))
        module = importlib.util.module_from_spec(spec)
        saved = {k: sys.modules.get(k) for k in out}
        sys.modules.update(out)
        spec.loader.exec_module(module)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        out[name] = module
    return out["tileset"], out["vram"], out["screen"], out["objects"]


class Bench:
    def __init__(self, batches):
        import torch
        self.torch, self.batches = torch, batches
        self.TS, self.V, self.S, self.OB = numpy_models()
        self.par = importlib.import_module("pixel-art-raytracer_amd")
        self.T = importlib.import_module("pixel-art-raytracer_amd.types")
        self.screen = importlib.import_module("pixel-art-raytracer_amd.screen")
        self.objects = importlib.import_module("pixel-art-raytracer_amd.objects")
        self.extend = importlib.import_module("pixel-art-raytracer_amd.tileset_extend")
        self.stream = torch.cuda.Stream()

    def zeros(self, n):
        return self.torch.zeros(max(1, n), dtype=self.torch.uint8, device="cuda")

    def up(self, array):
        import numpy as np
        return self.torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).cuda()

    def both_ways(self, call, per):
        """`call` eagerly and as replays of a graph of `per` calls."""
        torch = self.torch
        r = timed(self.stream, call, self.batches, per)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self.stream):
            for _ in range(per):
                call()

        def replay():
            with torch.cuda.stream(self.stream):
                graph.replay()

        g = timed(self.stream, replay, self.batches, 1)
        r.update(replay_us=round(g["us"] / per, 2), replay_us_min=round(g["us_min"] / per, 2), replay_us_max=round(g["us_max"] / per, 2),
                 replay_spread=g["spread"])
        return r

    def drawn(self, size, table, count, limit, per):
        """The draw of `table` (with a device count) over random planes of `size`, 4bpp rows, 64 colours in sub-palettes
        of 16: checked, timed eagerly and replayed, beside the screen's draw and a copy of the planes."""
        import numpy as np
        OB, S, V, s = self.OB, self.S, self.V, self.stream.cuda_stream
        w, h = size
        rng = np.random.default_rng(w + len(table))
        n_tiles = 256
        d = OB.desc_of(n_tiles=n_tiles, n_objects=len(table), line_limit=limit, n_colors=64, sub_size=16, bg_sub_size=16, width=w, height=h)
        chr_bytes = OB.random_chr(rng, d)
        pal = rng.integers(0, 256, 4 * 64, dtype=np.uint8)
        fb, index = rng.integers(0, 256, (h, w, 4), dtype=np.uint8), rng.integers(0, 64, (h, w), dtype=np.uint8)
        t_chr, t_table, t_pal, t_count = self.up(chr_bytes), self.up(table), self.up(pal), self.up(np.array([count], np.uint32))
        t_fb, t_index, t_work = self.up(fb), self.up(index), self.zeros(self.objects.work_bytes(h, limit))
        t_counts = self.zeros(8)
        desc = self.objects.desc(**d)

        def draw():
            self.objects.draw(desc, t_chr.data_ptr(), t_table.data_ptr(), t_work.data_ptr(), pal_words=t_pal.data_ptr(), fb_io=t_fb.data_ptr(),
                              index_io=t_index.data_ptr(), count=t_count.data_ptr(), bad_out=t_counts.data_ptr(),
                              over_out=t_counts.data_ptr() + 4, stream=s)

        draw()
        self.stream.synchronize()
        rows = min(h, CHECK_ROWS)
        e = OB.draw(dict(d, height=rows), chr_bytes, table, pal, None, fb[:rows], index[:rows], count)
        assert t_fb[:4 * w * rows].cpu().numpy().tobytes() == e[0].tobytes(), "fb_io is not the model's"
        assert t_index[:w * rows].cpu().numpy().tobytes() == e[1].tobytes(), "index_io is not the model's"
        bad, over = (int(v) for v in t_counts.cpu().numpy().view(np.uint32))
        assert bad == e[2] and (rows < h or over == e[3]), "the counts are not the model's"
        r = self.both_ways(draw, per)
        r.update(objects=min(count, len(table)), line_limit=limit, bad=bad, dropped=over, launches=2, fills=2)

        # the screen of the same size over the same tiles, and a copy of the two planes
        L = V.preset(V.SNES)
        gcx, gcy = -(-w // 8), -(-h // 8)
        tile_map = rng.integers(0, n_tiles, gcx * gcy).astype(np.uint32)
        words, _ = V.encode_map(L, tile_map, gcx, gcy, rng.integers(0, 4, gcx * gcy, dtype=np.uint8))
        sd = self.screen.desc(L, tile_w=8, tile_h=8, tile_format=V.F_4BPP_ROWS, n_tiles=n_tiles, map_w=gcx, map_h=gcy, pal_format=S.RGBA8,
                              n_colors=64, sub_size=16, width=w, height=h)
        t_words, s_fb, s_index = self.up(words), self.zeros(4 * w * h), self.zeros(w * h)

        def screen():
            self.screen.draw(sd, t_chr.data_ptr(), t_words.data_ptr(), t_pal.data_ptr(), fb_out=s_fb.data_ptr(), index_out=s_index.data_ptr(),
                             bad_out=t_counts.data_ptr(), stream=s)

        hip = self.par.hip_runtime()

        def copy():
            assert hip.hipMemcpyAsync(s_fb.data_ptr(), t_fb.data_ptr(), 4 * w * h, 3, s) == 0
            assert hip.hipMemcpyAsync(s_index.data_ptr(), t_index.data_ptr(), w * h, 3, s) == 0

        sc, cp = timed(self.stream, screen, self.batches, per), timed(self.stream, copy, self.batches, per)
        again = timed(self.stream, draw, self.batches, per)
        r.update(us_again=again["us"], screen_us=sc["us"], screen_spread=sc["spread"], copy_us=cp["us"], copy_spread=cp["spread"],
                 plane_bytes=5 * w * h, x_screen=round(r["us"] / sc["us"], 2), x_copy=round(r["us"] / cp["us"], 2))
        return r

    def draws(self):
        import numpy as np
        OB = self.OB
        rng = np.random.default_rng(1)

        def scattered(n, w, h):
            t = np.zeros(n, OB.OBJECT)
            t["x"], t["y"], t["tile"] = rng.integers(-4, w - 4, n), rng.integers(-4, h - 4, n), rng.integers(0, 256, n)
            t["attr"] = rng.integers(0, 4, n) | rng.integers(0, 4, n) << 8
            return t

        def on_grid(gx, gy):
            c = np.arange(gx * gy)
            t = np.zeros(gx * gy, OB.OBJECT)
            t["x"], t["y"], t["tile"], t["attr"] = (c % gx) * 8, (c // gx) * 8, c % 256, c % 4
            return t

        small, big = (480, 320), (4096, 4096)
        return {
            "480 x 320": {"40 objects": self.drawn(small, scattered(40, *small), 40, 128, 50),
                          "128 objects": self.drawn(small, scattered(128, *small), 128, 128, 50),
                          "2400 objects, one a cell": self.drawn(small, on_grid(60, 40), 2400, 128, 50),
                          "2400 objects, 8 a line": self.drawn(small, on_grid(60, 40), 2400, 8, 50)},
            "4096 x 4096": {"an empty table": self.drawn(big, scattered(128, *big), 0, 128, 20),
                            "128 objects": self.drawn(big, scattered(128, *big), 128, 128, 20),
                            "65536 objects on a grid": self.drawn(big, on_grid(256, 256), 65536, 128, 5)}}

    def from_maps(self, w, h, per):
        import numpy as np
        OB, TS, s = self.OB, self.TS, self.stream.cuda_stream
        gcx, gcy = w // 8, h // 8
        n = gcx * gcy
        rng = np.random.default_rng(n)
        a = rng.integers(0, 1024, n).astype(np.uint32) | rng.integers(0, 4, n).astype(np.uint32) << 30
        b = np.where(rng.random(n) < 1 / 3, a ^ np.uint32(1), a).astype(np.uint32)
        ca = rng.integers(0, 8, n, dtype=np.uint8)
        capacity = min(n, 65536)
        t_a, t_b, t_ca, t_cb = self.up(a), self.up(b), self.up(ca), self.up(ca)
        t_out, t_count, t_work = self.zeros(16 * capacity), self.zeros(4), self.zeros(self.objects.from_maps_work_bytes(n))

        def call():
            self.objects.from_maps(t_a.data_ptr(), t_b.data_ptr(), (gcx, gcy), (8, 8), capacity, t_work.data_ptr(), t_out.data_ptr(),
                                   t_count.data_ptr(), cells_bg=t_ca.data_ptr(), cells=t_cb.data_ptr(), stream=s)

        call()
        self.stream.synchronize()
        e, total = OB.from_maps(a, b, (gcx, gcy), (8, 8), capacity, ca, ca)
        assert int(t_count.cpu().numpy().view(np.uint32)[0]) == total and t_out[:16 * len(e)].cpu().numpy().tobytes() == e.tobytes()
        r = self.both_ways(call, per)
        r.update(cells=n, differing=total, capacity=capacity, launches=3, fills=0)

        # par_tileset_extend_device's steady state: a plane of as many cells whose tiles are all stored
        params = self.T.default_params(w, h)
        plane = TS.mixed_plane(rng, w, h, (8, 8), 200, 4)
        cap = 1024
        t_plane, t_tiles, t_set_count, t_map = self.up(plane), self.zeros(64 * cap), self.zeros(4), self.zeros(4 * n)
        t_xwork = self.zeros(self.extend.tileset_extend_work_bytes(n, cap))

        def extend():
            self.extend.tileset_extend(params, t_plane.data_ptr(), (0, h), (8, 8), t_xwork.data_ptr(), t_tiles.data_ptr(), cap,
                                       t_set_count.data_ptr(), map_out=t_map.data_ptr(), flips=3, stream=s)

        extend()
        self.stream.synchronize()
        stored = int(t_set_count.cpu().numpy().view(np.uint32)[0])
        x = timed(self.stream, extend, self.batches, per)
        assert int(t_set_count.cpu().numpy().view(np.uint32)[0]) == stored, "the steady state adds no tile"
        r.update(extend_us=x["us"], extend_spread=x["spread"], extend_tiles=stored, x_extend=round(r["us"] / x["us"], 2))
        return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects.json"))
    a = ap.parse_args()
    bench = Bench(a.batches)
    result = {"tool": "objects", "batches": a.batches, "gpus": 1,
              "cases": {"draw": bench.draws(), "from_maps": {"2400 cells": bench.from_maps(480, 320, 50), "2^18 cells": bench.from_maps(4096, 4096, 20)}}}
    line = json.dumps(result)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
