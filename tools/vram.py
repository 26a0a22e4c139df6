"""Microseconds per call of the VRAM-export add-on (addons/include/par_vram.h), each beside a device-to-device copy of the
bytes the call reads, their batches alternating in the same run on the same stream:
  - the 480 x 320 graybox frame's chain: palette fitted at 33, cells fitted at 8 x 4 over 8 x 8 cells, the cells quantise,
    then par_vram_local_device, par_tileset_build_device under both mirrors, par_vram_encode_tiles_device and
    par_vram_encode_map_device as the SNES loads them; each call alone, the four eagerly back to back, and the four replayed
    from one captured graph;
  - 4096 tiles of 16 x 16 through par_vram_encode_tiles_device and par_vram_decode_tiles_device in every format;
  - the 4096 x 4096 plane: par_vram_local_device over its 16 MiB and par_vram_encode_map_device over its 2^18 cells of 8 x 8
    under every preset.
Every output is checked against the numpy model of tests/vram.py in the run before it is timed. Calls are made eagerly,
back to back on one stream, as a frame loop makes them: after a warm-up, batches between two events; the median batch over
its call count, the fastest and the slowest (`spread` is (slowest - fastest) / median: what a difference has to exceed).
Every call is one launch, behind one four-byte fill where it counts into a bad_out. Prints one JSON line and writes it to
--out (default profiles/vram.json).
   python tools/vram.py [--batches N] [--out FILE]"""
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
from tileset import rendered  # noqa: E402  (tools/tileset.py)


def numpy_models():
    """tests/tileset.py and tests/vram.py, the contracts in numpy (by their paths: tools of those names exist)."""
    out = []
    for name in ("tileset", "vram"):
        spec = importlib.util.spec_from_file_location("tests_" + name, os.path.join(ROOT, "tests", name + ".py"))
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        out.append(module)
    return out


class Bench:
    def __init__(self, batches):
        import torch
        self.torch, self.batches = torch, batches
        self.TS, self.V = numpy_models()
        self.par = importlib.import_module("pixel-art-raytracer_amd")
        self.cells = importlib.import_module("pixel-art-raytracer_amd.cells")
        self.fit = importlib.import_module("pixel-art-raytracer_amd.cells_fit")
        self.tileset = importlib.import_module("pixel-art-raytracer_amd.tileset")
        self.vram = importlib.import_module("pixel-art-raytracer_amd.vram")
        self.T = importlib.import_module("pixel-art-raytracer_amd.types")
        self.stream = torch.cuda.Stream()

    def zeros(self, n, dtype=None):
        return self.torch.zeros(n, dtype=dtype or self.torch.uint8, device="cuda")

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

    def layout(self, machine):
        return self.vram.map_layout_preset(machine)

    def graybox(self):
        import numpy as np
        torch, par, T, V, TS, vram, s = self.torch, self.par, self.T, self.V, self.TS, self.vram, self.stream.cuda_stream
        params, fb = rendered(par, T, "graybox 480x320")
        W, H = params.width, params.height
        N, CELL, S, K, CAP, FLIPS = 33, (8, 8), 8, 4, 1024, 3
        gcx, gcy = TS.grid(W, H, (8, 8))
        n = gcx * gcy
        master, table = self.zeros(4 * N), self.zeros(4 * S * K)
        block = self.zeros(T.PALETTE_WORK.itemsize)
        fit_work = self.zeros(self.fit.cells_fit_work_bytes(W, H, CELL))
        index, local, chosen = self.zeros(W * H), self.zeros(W * H), self.zeros(n)
        work = self.zeros(self.tileset.tileset_work_bytes(n))
        tiles, tile_map, count = self.zeros(CAP * 64), self.zeros(n, torch.int32), self.zeros(1, torch.int32)
        chr_out, words, bad = self.zeros(CAP * 32), self.zeros(2 * n), self.zeros(2, torch.int32)
        layout = self.layout(vram.SNES)
        w, rows = block.data_ptr(), (0, H)
        par.palette_reset(w, stream=s)
        par.palette_count(params, fb.data_ptr(), rows, w, stream=s)
        par.palette_cut(w, N, stream=s)
        par.palette_sum(params, fb.data_ptr(), rows, w, stream=s)
        par.palette_emit(w, N, master.data_ptr(), stream=s)
        self.fit.cells_fit(fb.data_ptr(), W, H, CELL, master.data_ptr(), N, S, K, 0, fit_work.data_ptr(), table.data_ptr(), stream=s)
        self.cells.quantize_cells(params, table.data_ptr(), S, K, CELL, fb.data_ptr(), rows, index_out=index.data_ptr(),
                                  cell_out=chosen.data_ptr(), stream=s)

        def do_local():
            vram.local(index.data_ptr(), W * H, K, local.data_ptr(), stream=s)

        def do_build():
            self.tileset.tileset_build(params, local.data_ptr(), rows, (8, 8), work.data_ptr(), count.data_ptr(),
                                       tiles_out=tiles.data_ptr(), capacity=CAP, map_out=tile_map.data_ptr(), flips=FLIPS, stream=s)

        def do_tiles():
            vram.encode_tiles(tiles.data_ptr(), CAP, count.data_ptr(), (8, 8), vram.FORMAT_4BPP_ROWS, chr_out.data_ptr(),
                              bad_out=bad.data_ptr(), stream=s)

        def do_map():
            vram.encode_map(layout, tile_map.data_ptr(), (gcx, gcy), words.data_ptr(), cells=chosen.data_ptr(),
                            bad_out=bad.data_ptr() + 4, stream=s)

        def chain():
            do_local()
            do_build()
            do_tiles()
            do_map()

        chain()
        self.stream.synchronize()
        h_index, h_chosen = index.cpu().numpy(), chosen.cpu().numpy()
        exp = V.export(TS, h_index, h_chosen, K, W, H, CELL, V.SNES, FLIPS)
        t = int(count.cpu().numpy().view(np.uint32)[0])
        assert t == exp["count"] <= exp["flat"], (t, exp["count"], exp["flat"])
        assert chr_out.cpu().numpy()[:32 * t].tobytes() == exp["chr"].tobytes(), "the encoded tiles"
        assert words.cpu().numpy().tobytes() == exp["map_bytes"].tobytes(), "the map words"
        assert int(bad.cpu().numpy().sum()) == exp["bad"] == 0
        assert V.closing_identity(TS, exp, h_chosen, K, W, H).tobytes() == h_index.tobytes(), "the closing identity"
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self.stream):
            chain()

        def replay():
            with torch.cuda.stream(self.stream):
                graph.replay()

        per = 50
        return {"frame": "graybox 480x320, palette fitted at 33, cells fitted at 8 x 4 over 8 x 8, SNES", "pixels": W * H, "cells": n,
                "tiles": t, "tiles_flat": exp["flat"], "tile_bytes": 32 * t, "map_bytes": 2 * n, "bad": exp["bad"],
                "local": self.beside_a_copy(do_local, W * H, per), "build": timed(self.stream, do_build, self.batches, per),
                "encode_tiles": self.beside_a_copy(do_tiles, 64 * t, per), "encode_map": self.beside_a_copy(do_map, 4 * n, per),
                "chain of four, eager": timed(self.stream, chain, self.batches, per),
                "chain of four, graph": timed(self.stream, replay, self.batches, per),
                "launches": {"local": 1, "encode_tiles": 1, "encode_map": 1, "fills": {"encode_tiles": 1, "encode_map": 1}}}

    def big_tiles(self):
        import numpy as np
        torch, V, vram, s = self.torch, self.V, self.vram, self.stream.cuda_stream
        n, tile = 4096, (16, 16)
        rng = np.random.default_rng(1)
        out = {"tiles": n, "tile": list(tile), "pixel_bytes": n * 256}
        for fmt in V.FORMATS:
            host = rng.integers(0, 1 << V.BPP[fmt], (n, 16, 16), dtype=np.uint8)
            each = V.tile_bytes(fmt, tile)
            tiles = torch.from_numpy(host.reshape(-1)).cuda()
            data, back, bad = self.zeros(n * each), self.zeros(n * 256), self.zeros(1, torch.int32)

            def encode():
                vram.encode_tiles(tiles.data_ptr(), n, None, tile, fmt, data.data_ptr(), bad_out=bad.data_ptr(), stream=s)

            def decode():
                vram.decode_tiles(data.data_ptr(), n, tile, fmt, back.data_ptr(), stream=s)

            encode()
            decode()
            self.stream.synchronize()
            assert data.cpu().numpy().tobytes() == V.encode_tiles(host, tile, fmt)[0].tobytes(), (fmt, "encode")
            assert back.cpu().numpy().tobytes() == host.tobytes() and int(bad.item()) == 0, (fmt, "decode")
            out[V.FORMAT_NAMES[fmt]] = {"encoded_bytes": n * each, "encode": self.beside_a_copy(encode, n * 256, 50),
                                        "decode": self.beside_a_copy(decode, n * each, 50)}
        return out

    def big_plane(self):
        import numpy as np
        torch, V, vram, s = self.torch, self.V, self.vram, self.stream.cuda_stream
        W = H = 4096
        gcx = gcy = 512
        n = gcx * gcy
        rng = np.random.default_rng(2)
        h_plane = rng.integers(0, 128, W * H, dtype=np.uint8)
        plane, local = torch.from_numpy(h_plane).cuda(), self.zeros(W * H)

        def do_local():
            vram.local(plane.data_ptr(), W * H, 16, local.data_ptr(), stream=s)

        do_local()
        self.stream.synchronize()
        assert local.cpu().numpy().tobytes() == (h_plane % 16).tobytes(), "the local plane"
        out = {"plane": "4096x4096", "cells": n, "local": self.beside_a_copy(do_local, W * H, 10)}
        h_map = (rng.integers(0, 1024, n).astype(np.uint32) | (rng.integers(0, 4, n).astype(np.uint32) << 30))
        h_cells = rng.integers(0, 8, n, dtype=np.uint8)
        tile_map, chosen = torch.from_numpy(h_map.view(np.int32)).cuda(), torch.from_numpy(h_cells).cuda()
        bad = self.zeros(1, torch.int32)
        for machine, name in enumerate(V.MACHINES):
            layout, L = self.layout(machine), V.preset(machine)
            words = self.zeros(n * L["word_bytes"])

            def do_map():
                vram.encode_map(layout, tile_map.data_ptr(), (gcx, gcy), words.data_ptr(), cells=chosen.data_ptr(),
                                bad_out=bad.data_ptr(), stream=s)

            do_map()
            self.stream.synchronize()
            e_words, e_bad = V.encode_map(L, h_map, gcx, gcy, h_cells)
            assert words.cpu().numpy().tobytes() == e_words.tobytes() and int(bad.item()) == e_bad, name
            out[f"encode_map, {name}"] = dict(self.beside_a_copy(do_map, 4 * n, 50), map_bytes=n * L["word_bytes"], bad=e_bad)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vram.json"))
    a = ap.parse_args()
    bench = Bench(a.batches)
    result = {"tool": "vram", "batches": a.batches, "gpus": 1,
              "cases": {"graybox": bench.graybox(), "4096 tiles of 16 x 16": bench.big_tiles(), "4096 x 4096": bench.big_plane()}}
    line = json.dumps(result)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
