"""Microseconds per par_cells_fit_device call (the add-on of addons/include/par_cells_fit.h: the table, the seeds and the
errors), on two planes and at the three machine shapes par_cells.h names, without rounds and with six:
  - the 480 x 320 graybox frame under two tinted ranged lights and the 4096 x 4096 headline frame, each with its master
    fitted at 64 entries and refined six rounds on the device;
  - NES (4 sub-palettes of 4, 16 x 16 cells), Game Boy Color (8 of 4, 8 x 8), Mega Drive (4 of 16, 8 x 8).
Beside every shape, in the same run and on the same stream: one par_quantize_cells_device call at S = 1 with the table's
first K entries, index plane out (what a seed step computes a pixel), and one par_palette_refine_device round at S * K
entries (what a round computes). On the graybox plane every fit is checked against the numpy model of tests/cells_fit.py
first; on the headline plane, where the model would take minutes, errors_out[R] is checked against the summed difference
par_quantize_cells_device leaves under table_out. `launches` is what a call enqueues, 4 + S + 4 R + 1, `passes` those
of them that read the frame, S + 1 + 2 R + 1. Calls are made eagerly, back to back on one stream, as a frame loop makes
them: after a warm-up, batches between two events; the median batch over its call count, the fastest and the slowest
(`spread` is (slowest - fastest) / median: what a difference has to exceed). `graph_us` is the same call replayed from a
captured graph. Prints one JSON line and writes it to --out (default profiles/cells_fit.json).
   python tools/cells_fit.py [--batches N] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pattern import timed  # noqa: E402
from tileset import rendered  # noqa: E402  (tools/tileset.py)

SHAPES = (("NES", 4, 4, (16, 16)), ("GBC", 8, 4, (8, 8)), ("MD", 4, 16, (8, 8)))
ROUNDS = (0, 6)
N = 64


def numpy_model():
    """tests/cells_fit.py, the contract in numpy, with the tests' modules it imports (by their paths: tools of those
    names exist)."""
    import importlib.util
    names = ("quantize", "cells", "palette_refine", "cells_fit")
    kept = {name: sys.modules.get(name) for name in names}
    for name in names:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    model = sys.modules["cells_fit"]
    for name, module in kept.items():
        if module is None:
            del sys.modules[name]
        else:
            sys.modules[name] = module
    return model


class Bench:
    def __init__(self, batches):
        import torch
        self.torch, self.batches = torch, batches
        self.CF = numpy_model()
        self.par = importlib.import_module("pixel-art-raytracer_amd")
        self.cells = importlib.import_module("pixel-art-raytracer_amd.cells")
        self.fit = importlib.import_module("pixel-art-raytracer_amd.cells_fit")
        self.T = importlib.import_module("pixel-art-raytracer_amd.types")
        self.stream = torch.cuda.Stream()

    def master(self, params, fb, n):
        """The frame's palette of n entries, fitted and refined six rounds, in a device buffer."""
        torch, par, T, s = self.torch, self.par, self.T, self.stream.cuda_stream
        H = params.height
        palette = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
        fit_work = torch.zeros(T.PALETTE_WORK.itemsize, dtype=torch.uint8, device="cuda")
        refine_work = torch.zeros(T.PALETTE_REFINE_WORK.itemsize, dtype=torch.uint8, device="cuda")
        scratch = torch.zeros(params.width * H, dtype=torch.uint8, device="cuda")
        w, p, rows = fit_work.data_ptr(), palette.data_ptr(), (0, H)
        par.palette_reset(w, stream=s)
        par.palette_count(params, fb.data_ptr(), rows, w, stream=s)
        par.palette_cut(w, n, stream=s)
        par.palette_sum(params, fb.data_ptr(), rows, w, stream=s)
        par.palette_emit(w, n, p, stream=s)
        par.palette_refine_device(params, fb.data_ptr(), rows, p, n, 6, scratch.data_ptr(), refine_work.data_ptr(), None, stream=s)
        self.stream.synchronize()
        return palette

    def plane(self, name, label, with_model):
        import numpy as np
        torch, par, T, fit, cells, s = self.torch, self.par, self.T, self.fit, self.cells, self.stream.cuda_stream
        params, fb = rendered(par, T, name)
        W, H = params.width, params.height
        palette = self.master(params, fb, N)
        fb_host = fb.cpu().numpy().view(T.COLOR) if with_model else None
        palette_host = palette.cpu().numpy().view(T.COLOR)
        index = torch.zeros(W * H, dtype=torch.uint8, device="cuda")
        shown = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
        refine_work = torch.zeros(T.PALETTE_REFINE_WORK.itemsize, dtype=torch.uint8, device="cuda")
        per = 20 if W * H <= 1 << 20 else 3
        out = {"frame": label, "pixels": W * H, "master": N}
        for machine, S, K, cell in SHAPES:
            work = torch.zeros(fit.cells_fit_work_bytes(W, H, cell), dtype=torch.uint8, device="cuda")
            table = torch.zeros(S * K * 4, dtype=torch.uint8, device="cuda")
            seeds = torch.zeros(S, dtype=torch.int32, device="cuda")
            case = {"cells": self.CF.n_cells(W, H, cell), "work_bytes": int(work.numel())}
            for R in ROUNDS:
                errors = torch.zeros(R + 1, dtype=torch.int64, device="cuda")

                def call():
                    fit.cells_fit(fb.data_ptr(), W, H, cell, palette.data_ptr(), N, S, K, R, work.data_ptr(), table.data_ptr(),
                                  seeds_out=seeds.data_ptr(), errors_out=errors.data_ptr(), stream=s)

                call()
                cells.quantize_cells(params, table.data_ptr(), S, K, cell, fb.data_ptr(), (0, H), fb_out=shown.data_ptr(), stream=s)
                self.stream.synchronize()
                got = errors.cpu().numpy().view(np.uint64)
                a = fb.view(-1, 4)[:, :3].to(torch.int32)
                left = int((a - shown.view(-1, 4)[:, :3].to(torch.int32)).abs().sum(dtype=torch.int64).item())
                assert left == int(got[R]), (machine, R, "the last error is the difference quantize_cells leaves", left, got)
                assert (np.diff(got.astype(np.int64)) <= 0).all(), (machine, R, got)
                if with_model:
                    e = self.CF.model(fb_host, W, H, cell, palette_host, S, K, R)
                    assert table.cpu().numpy().tobytes() == e[0].tobytes(), (machine, R, "the table")
                    assert seeds.cpu().numpy().view(np.uint32).tobytes() == e[1].tobytes(), (machine, R, "the seeds")
                    assert got.tobytes() == e[2].tobytes(), (machine, R, "the errors")
                r = timed(self.stream, call, self.batches, per)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=self.stream):
                    call()

                def replay():
                    with torch.cuda.stream(self.stream):
                        graph.replay()

                g = timed(self.stream, replay, self.batches, per)
                passes = S + 1 + 2 * R + 1
                r.update(errors=[int(got[0]), int(got[R])], launches=4 + S + 4 * R + 1, passes=passes,
                         us_per_pass=round(r["us"] / passes, 2), graph_us=g["us"], graph_spread=g["spread"],
                         checked="the numpy model" if with_model else "the difference quantize_cells leaves")
                case[f"fit, {R} rounds"] = r

            def one_step():
                cells.quantize_cells(params, table.data_ptr(), 1, K, cell, fb.data_ptr(), (0, H), index_out=index.data_ptr(), stream=s)

            flat = table.clone()

            def one_round():
                par.palette_refine_device(params, fb.data_ptr(), (0, H), flat.data_ptr(), S * K, 1, index.data_ptr(),
                                          refine_work.data_ptr(), None, stream=s)

            case["quantize_cells, S = 1"] = timed(self.stream, one_step, self.batches, per)
            case["palette_refine, one round"] = timed(self.stream, one_round, self.batches, per)
            r0, r6 = case["fit, 0 rounds"]["us"], case["fit, 6 rounds"]["us"]
            case["us_per_step"] = round(r0 / (S + 1), 2)
            case["us_per_round"] = round((r6 - r0) / 6, 2)
            case["x_quantize_cells_per_step"] = round(case["us_per_step"] / case["quantize_cells, S = 1"]["us"], 2)
            case["x_palette_refine_per_round"] = round(case["us_per_round"] / case["palette_refine, one round"]["us"], 2)
            out[f"{machine}: {S} x {K}, {cell[0]} x {cell[1]}"] = case
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cells_fit.json"))
    a = ap.parse_args()
    bench = Bench(a.batches)
    result = {"tool": "cells_fit", "batches": a.batches, "gpus": 1,
              "cases": [bench.plane("graybox 480x320", "graybox 480x320, master fitted at 64 and refined 6 rounds", True),
                        bench.plane("headline 4096x4096", "headline 4096x4096, master fitted at 64 and refined 6 rounds", False)]}
    line = json.dumps(result)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
