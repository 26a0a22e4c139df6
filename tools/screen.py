"""Microseconds per par_screen_draw_device (addons/include/par_screen.h), each beside a device-to-device copy of the
bytes it writes, their batches alternating in the same run on the same stream:
  - the 480 x 320 graybox frame (palette fitted at 33, cells fitted at 8 x 4 over 8 x 8 cells, 8 x 8 tiles under both
    mirrors) exported for each machine and drawn on a screen the size of the frame, with the error of what the machine
    shows: the summed L1 over red, green and blue against the cells frame, without and with the backdrop rule, as
    this run's own draw gives it, and beside it what par_demo --vram MACHINE --vram-show [backdrop] prints for its own first
    frame under the same flags;
  - a 4096 x 4096 screen over a 512 x 512-cell map of 1024 tiles, the shape of the 4096 x 4096 plane's export, for the SNES
    and the Mega Drive (planar and packed), at scroll 0, at an odd scroll phase, with per-line scroll, and the index plane
    alone;
  - a 256 x 240 screen over a 32 x 30 map, the NES's own size, through an attribute grid.
Beside the draw, where the composition can express the same picture (scroll 0, one sub-palette, RGBA8 entries): the three
calls par_vram_decode_tiles_device, par_tileset_expand_device and par_present_device, which write the decoded tiles and the
index plane on the way.
Every output is checked against the numpy model of tests/screen.py in the run before it is timed. Calls are made eagerly,
back to back on one stream, as a frame loop makes them: after a warm-up, batches between two events; the median batch over
its call count, the fastest and the slowest (`spread` is (slowest - fastest) / median: what a difference has to exceed).
Prints one JSON line and writes it to --out (default profiles/screen.json).
   python tools/screen.py [--batches N] [--out FILE]"""
import argparse
import importlib
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pattern import timed  # noqa: E402
from tileset import rendered  # noqa: E402  (tools/tileset.py)

CHECK_ROWS = 512
DEMO_FLAGS = ["--frames", "1", "--palette-fit", "33", "--cells", "8,8", "--cells-fit", "8,4", "--tileset", "8,8,3"]


def numpy_models():
    """tests/tileset.py, tests/vram.py and tests/screen.py, the contracts in numpy (by their paths: tools of those names
    exist; tests/screen.py imports tests/vram.py as `vram`)."""
    out = {}
    for name in ("tileset", "vram", "screen"):
        spec = importlib.util.spec_from_file_location("tests_" + name, os.path.join(ROOT, "tests", name + ".py"))
        module = importlib.util.module_from_spec(spec)
        if name == "screen":
            sys.modules["vram"] = out["vram"]
        spec.loader.exec_module(module)
        out[name] = module
    sys.modules.pop("vram", None)
    return out["tileset"], out["vram"], out["screen"]


class Bench:
    def __init__(self, batches):
        import torch
        self.torch, self.batches = torch, batches
        self.TS, self.V, self.S = numpy_models()
        self.par = importlib.import_module("pixel-art-raytracer_amd")
        self.cells = importlib.import_module("pixel-art-raytracer_amd.cells")
        self.fit = importlib.import_module("pixel-art-raytracer_amd.cells_fit")
        self.tileset = importlib.import_module("pixel-art-raytracer_amd.tileset")
        self.vram = importlib.import_module("pixel-art-raytracer_amd.vram")
        self.screen = importlib.import_module("pixel-art-raytracer_amd.screen")
        self.T = importlib.import_module("pixel-art-raytracer_amd.types")
        self.stream = torch.cuda.Stream()

    def zeros(self, n, dtype=None):
        return self.torch.zeros(n, dtype=dtype or self.torch.uint8, device="cuda")

    def up(self, array):
        import numpy as np
        return self.torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).cuda()

    def beside_a_copy(self, call, nbytes, per):
        """`call` and a device-to-device copy of nbytes bytes, batch after batch in turn."""
        src, dst = self.zeros(nbytes), self.zeros(nbytes)
        hip, s = self.par.hip_runtime(), self.stream.cuda_stream
        device_to_device = 3  # hipMemcpyDeviceToDevice

        def copy():
            rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, device_to_device, s)
            assert rc == 0, rc

        r = timed(self.stream, call, self.batches, per)
        c = timed(self.stream, copy, self.batches, per)
        r2 = timed(self.stream, call, self.batches, per)
        r.update(us_again=r2["us"], copy_bytes=nbytes, copy_us=c["us"], copy_spread=c["spread"], x_copy=round(r["us"] / c["us"], 2))
        return r

    def drawn(self, d, chr_bytes, words, pal, attr=None, lines=None, fb=True, index=False, per=50):
        """The draw of descriptor dict `d` over host VRAM: checked against the model (its first CHECK_ROWS rows: a row
        depends on nothing but its own number, and the model takes a gigabyte at 4096 x 4096), then timed beside a copy of
        its output bytes. Returns (the timing, the model's fb of those rows, the device's fb_out)."""
        import numpy as np
        S, s = self.S, self.stream.cuda_stream
        w, h = d["width"], d["height"]
        desc = self.screen.desc(d["layout"], **{f: d[f] for f in S.DESC_FIELDS})
        bufs = [self.up(chr_bytes), self.up(words), self.up(pal), None if attr is None else self.up(attr),
                None if lines is None else self.up(np.asarray(lines, np.int32))]
        p = [None if b is None else b.data_ptr() for b in bufs]
        fb_out, index_out, bad = self.zeros(4 * w * h) if fb else None, self.zeros(w * h) if index else None, self.zeros(1, self.torch.int32)

        def draw():
            self.screen.draw(desc, p[0], p[1], p[2], fb_out=fb_out.data_ptr() if fb else None, index_out=index_out.data_ptr() if index else None,
                             attr=p[3], line_scroll=p[4], bad_out=bad.data_ptr(), stream=s)

        draw()
        self.stream.synchronize()
        rows = min(h, CHECK_ROWS)
        e_fb, e_index, e_bad = S.draw(dict(d, height=rows), chr_bytes, words, pal, attr, None if lines is None else lines[:2 * rows])
        assert not fb or fb_out[:4 * w * rows].cpu().numpy().tobytes() == e_fb.tobytes(), "fb_out is not the model's"
        assert not index or index_out[:w * rows].cpu().numpy().tobytes() == e_index.tobytes(), "index_out is not the model's"
        assert int(bad.cpu().numpy().view(np.uint32)[0]) == e_bad, "bad_out is not the model's"
        r = self.beside_a_copy(draw, (4 * w * h if fb else 0) + (w * h if index else 0), per)
        r.update(bad=e_bad, launches=1, fills=1)
        return r, e_fb, fb_out

    def composed(self, d, chr_bytes, words_map, pal, shown, per):
        """par_vram_decode_tiles_device, par_tileset_expand_device and par_present_device for the picture of `d` (scroll 0,
        palette 0 in every word, RGBA8 entries): checked against the draw's fb_out `shown` (but for its alpha), then
        timed."""
        par, T, s = self.par, self.T, self.stream.cuda_stream
        w, h, tile = d["width"], d["height"], (d["tile_w"], d["tile_h"])
        params = T.default_params(w, h)
        data, tile_map, colours = self.up(chr_bytes), self.up(words_map), self.up(pal)
        tiles, plane, out = self.zeros(d["n_tiles"] * tile[0] * tile[1]), self.zeros(w * h), self.zeros(4 * w * h)
        desc = T.make_present_desc(1, width=w)

        def chain():
            self.vram.decode_tiles(data.data_ptr(), d["n_tiles"], tile, d["tile_format"], tiles.data_ptr(), stream=s)
            self.tileset.tileset_expand(params, tiles.data_ptr(), d["n_tiles"], tile, tile_map.data_ptr(), (0, h), plane.data_ptr(), stream=s)
            par.present(params, desc, out.data_ptr(), (0, h), index=plane.data_ptr(), d_palette=colours.data_ptr(), n_colors=d["n_colors"],
                        stream=s)

        chain()
        self.stream.synchronize()
        assert bool((out.view(-1, 4)[:, :3] == shown.view(-1, 4)[:, :3]).all()), "the composition shows another picture"
        r = timed(self.stream, chain, self.batches, per)
        r.update(launches=3, bytes_written=d["n_tiles"] * tile[0] * tile[1] + 5 * w * h)
        return r

    def demo_errors(self, machine):
        """`screen frame 0` of par_demo on the graybox frame for `machine`: {backdrop: (bad, error)}, and its vram line."""
        exe = os.path.join(os.path.dirname(self.par.LIB_PATH), "par_demo")
        out = {}
        with tempfile.TemporaryDirectory() as tmp:
            for backdrop in (0, 1):
                p = subprocess.run([exe, *DEMO_FLAGS, "--gif", os.path.join(tmp, "a.gif"), "--vram", machine, "--vram-show",
                                    *(["backdrop"] if backdrop else [])], capture_output=True, text=True, timeout=300)
                assert p.returncode == 0, p.stderr
                m = re.search(r"^screen frame 0: bad (\d+), error (\d+)$", p.stdout, flags=re.M)
                v = re.search(r"^vram frame 0: (\d+) tiles \((\d+) flat\), (\d+) tile bytes, (\d+) map bytes, bad (\d+)$", p.stdout, flags=re.M)
                out["backdrop" if backdrop else "no backdrop"] = {"bad": int(m.group(1)), "error": int(m.group(2))}
                out["export"] = {"tiles": int(v.group(1)), "bad": int(v.group(5))}
        return out

    def graybox(self):
        import numpy as np
        par, T, V, TS, S, s = self.par, self.T, self.V, self.TS, self.S, self.stream.cuda_stream
        params, fb = rendered(par, T, "graybox 480x320")
        W, H = params.width, params.height
        N, CELL, SUBS, K, FLIPS = 33, (8, 8), 8, 4, 3
        gcx, gcy = TS.grid(W, H, (8, 8))
        master, table = self.zeros(4 * N), self.zeros(4 * SUBS * K)
        block = self.zeros(T.PALETTE_WORK.itemsize)
        fit_work = self.zeros(self.fit.cells_fit_work_bytes(W, H, CELL))
        index, chosen = self.zeros(W * H), self.zeros(gcx * gcy)
        w, rows = block.data_ptr(), (0, H)
        par.palette_reset(w, stream=s)
        par.palette_count(params, fb.data_ptr(), rows, w, stream=s)
        par.palette_cut(w, N, stream=s)
        par.palette_sum(params, fb.data_ptr(), rows, w, stream=s)
        par.palette_emit(w, N, master.data_ptr(), stream=s)
        self.fit.cells_fit(fb.data_ptr(), W, H, CELL, master.data_ptr(), N, SUBS, K, 0, fit_work.data_ptr(), table.data_ptr(), stream=s)
        self.cells.quantize_cells(params, table.data_ptr(), SUBS, K, CELL, fb.data_ptr(), rows, index_out=index.data_ptr(),
                                  cell_out=chosen.data_ptr(), stream=s)
        self.stream.synchronize()
        h_index, h_chosen, h_table = index.cpu().numpy(), chosen.cpu().numpy(), table.cpu().numpy().reshape(-1, 4)
        meant = h_table[h_index.astype(np.int64)][:, :3].astype(np.int64).reshape(H, W, 3)
        out = {"frame": "graybox 480x320, palette fitted at 33, cells fitted at 8 x 4 over 8 x 8, tiles 8 x 8 under both mirrors",
               "pixels": W * H, "cells": gcx * gcy, "error_is": "summed L1 over red, green and blue against the cells frame",
               "error_of_one_step_a_channel_everywhere": W * H * 3}
        for m, name in enumerate(V.MACHINES):
            exp = V.export(TS, h_index, h_chosen, K, W, H, CELL, m, FLIPS)
            fmt, colours = V.MACHINE_FORMATS[m]
            d = S.desc_of(exp["layout"], tile_format=fmt, n_tiles=exp["count"], map_w=gcx, map_h=gcy, n_colors=SUBS * K, sub_size=K, width=W,
                          height=H, pal_format=S.RGBA8 if colours is None else colours)
            pal = h_table.reshape(-1) if colours is None else V.palette_words(h_table, colours)
            attr = h_chosen if colours is None else None
            case = {"tiles": exp["count"], "export_bad": exp["bad"], "tile_bytes": len(exp["chr"]), "map_bytes": len(exp["map_bytes"])}
            for backdrop in (0, 1):
                r, e_fb, _ = self.drawn(dict(d, backdrop=backdrop), exp["chr"], exp["map_bytes"], pal, attr=attr)
                r["error"] = int(np.abs(e_fb[:, :, :3].astype(np.int64) - meant).sum())
                case["backdrop" if backdrop else "no backdrop"] = r
            case["par_demo, its own first frame"] = self.demo_errors(name)
            if colours is not None:
                # the closing identity: RGBA8 entries, no backdrop, and the picture is the cells frame
                exact = S.draw(dict(d, pal_format=S.RGBA8), exp["chr"], exp["map_bytes"], h_table.reshape(-1))
                case["error through rgba8 entries, no backdrop"] = int(np.abs(exact[0][:, :, :3].astype(np.int64) - meant).sum())
            out[name] = case
        return out

    def synthetic(self, L, fmt, tile, grid, n_tiles, size, seed, one_palette):
        import numpy as np
        V = self.V
        rng = np.random.default_rng(seed)
        tiles = rng.integers(0, 1 << V.BPP[fmt], (n_tiles, tile[1], tile[0]), dtype=np.uint8)
        n = grid[0] * grid[1]
        flips = (1 if L["flip_x_bit"] >= 0 else 0) | (2 if L["flip_y_bit"] >= 0 else 0)
        tile_map = rng.integers(0, n_tiles, n).astype(np.uint32) | ((rng.integers(0, 4, n).astype(np.uint32) & np.uint32(flips)) << 30)
        cells = np.zeros(n, np.uint8) if one_palette else rng.integers(0, 1 << min(3, L["pal_bits"]), n, dtype=np.uint8)
        words, bad = V.encode_map(L, tile_map, grid[0], grid[1], cells)
        assert bad == 0
        return V.encode_tiles(tiles, tile, fmt)[0], words, tile_map

    def big_screen(self):
        import numpy as np
        V, S = self.V, self.S
        W = H = 4096
        grid, n_tiles, K = (512, 512), 1024, 16
        rng = np.random.default_rng(3)
        pal = rng.integers(0, 256, 4 * 8 * K, dtype=np.uint8)
        out = {"screen": "4096x4096", "map": "512 x 512 cells of 8 x 8", "tiles": n_tiles, "fb_bytes": 4 * W * H}
        for machine, fmt in ((V.SNES, V.F_4BPP_ROWS), (V.MEGADRIVE, V.F_4BPP_PACKED_HI)):
            L = V.preset(machine)
            subs = min(8, 1 << L["pal_bits"])
            chr_bytes, words, _ = self.synthetic(L, fmt, (8, 8), grid, n_tiles, (W, H), 4 + machine, False)
            d = S.desc_of(L, tile_format=fmt, n_tiles=n_tiles, map_w=grid[0], map_h=grid[1], n_colors=subs * K, sub_size=K, width=W, height=H)
            lines = np.stack([(np.arange(H) * 3) % 64 - 32, np.zeros(H, np.int64)], axis=1).astype(np.int32).reshape(-1)
            case = {"scroll 0": self.drawn(d, chr_bytes, words, pal, per=10)[0],
                    "scroll (3, 5)": self.drawn(dict(d, scroll_x=3, scroll_y=5), chr_bytes, words, pal, per=10)[0],
                    "per-line scroll": self.drawn(d, chr_bytes, words, pal, lines=lines, per=10)[0],
                    "backdrop": self.drawn(dict(d, backdrop=1), chr_bytes, words, pal, per=10)[0],
                    "index plane alone": self.drawn(d, chr_bytes, words, pal, fb=False, index=True, per=10)[0],
                    "colour words": self.drawn(dict(d, pal_format=V.MACHINE_FORMATS[machine][1]), chr_bytes, words,
                                               V.palette_words(pal.reshape(-1, 4), V.MACHINE_FORMATS[machine][1]), per=10)[0]}
            # one sub-palette, so that decode, expand and present can show the same picture
            chr_bytes, words, tile_map = self.synthetic(L, fmt, (8, 8), grid, n_tiles, (W, H), 14 + machine, True)
            one = dict(d, n_colors=K)
            r, _, shown = self.drawn(one, chr_bytes, words, pal[:4 * K], per=10)
            case["one sub-palette, draw"] = r
            case["one sub-palette, decode + expand + present"] = self.composed(one, chr_bytes, tile_map, pal[:4 * K], shown, 10)
            out[V.MACHINES[machine]] = case
        return out

    def nes_screen(self):
        import numpy as np
        V, S = self.V, self.S
        L = V.preset(V.NES)
        rng = np.random.default_rng(5)
        chr_bytes, words, tile_map = self.synthetic(L, V.F_2BPP_PLANAR, (8, 8), (32, 30), 256, (256, 240), 6, True)
        pal = rng.integers(0, 256, 4 * 16, dtype=np.uint8)
        d = S.desc_of(L, tile_format=V.F_2BPP_PLANAR, n_tiles=256, map_w=32, map_h=30, ratio_x=2, ratio_y=2, n_colors=16, sub_size=4,
                      width=256, height=240, scroll_x=5, scroll_y=-3, backdrop=1)
        attr = rng.integers(0, 4, S.attr_cells(d), dtype=np.uint8)
        out = {"screen": "256x240", "map": "32 x 30 cells of 8 x 8", "fb_bytes": 4 * 256 * 240,
               "attribute grid, backdrop, scroll (5, -3)": self.drawn(d, chr_bytes, words, pal, attr=attr)[0]}
        one = dict(d, scroll_x=0, scroll_y=0, backdrop=0, n_colors=4)
        r, _, shown = self.drawn(one, chr_bytes, words, pal[:16])
        out["one sub-palette, draw"] = r
        out["one sub-palette, decode + expand + present"] = self.composed(one, chr_bytes, tile_map, pal[:16], shown, 50)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "screen.json"))
    a = ap.parse_args()
    bench = Bench(a.batches)
    result = {"tool": "screen", "batches": a.batches, "gpus": 1,
              "cases": {"graybox": bench.graybox(), "4096 x 4096": bench.big_screen(), "256 x 240": bench.nes_screen()}}
    line = json.dumps(result)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
