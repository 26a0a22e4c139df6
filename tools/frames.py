#!/usr/bin/env python3
"""Render N frames of one workload (for rocprofv3 --kernel-trace --stats / --pmc runs on the GPU box).
usage: frames.py [--kept] [--move=K] [synthetic|floor|graybox|small|trace_bg] [frames] [extra render flags, e.g. 2 = count rays]
--kept: every frame carries RENDER_KEPT_OUTPUTS (the buffers are this context's own: kept frames from the second on)
--move=K: before every frame but the first, entities [0, K) step 4 pixels to and fro in x, by update_aabbs of that
          sub-range on the frame's stream (a static level with a few movers; without it nothing changes between frames)"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
par = importlib.import_module("pixel-art-raytracer_amd")
T = par.types
kept = "--kept" in sys.argv
move = max([int(v.split("=")[1]) for v in sys.argv if v.startswith("--move=")] + [0])
sys.argv = [v for v in sys.argv if v != "--kept" and not v.startswith("--move=")]
what = sys.argv[1] if len(sys.argv) > 1 else "synthetic"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 100
flags = 0
extra = (int(sys.argv[3], 0) if len(sys.argv) > 3 else 0) | (par.RENDER_KEPT_OUTPUTS if kept else 0)
if what in ("synthetic", "trace_bg"):
    W = H = L = 4096
    p = T.default_params(W, H, L)
    a, l = par.scene_synthetic(1024, W, H, L, 12345)
    flags = par.RENDER_TRACE_BACKGROUND if what == "trace_bg" else 0
elif what == "floor":
    W = H = L = 4096
    p = T.default_params(W, H, L)
    a = T.make_aabbs([(i * 20, 0, j * 20, 20, 20, 20) for i in range(W // 20) for j in range(L // 20)])
    l = T.make_light(2560, 2048, 1024)
elif what == "small":  # BASELINE config 2
    W = H = L = 512
    p = T.default_params(W, H, L)
    a, l = par.scene_synthetic(64, W, H, L, 12345)
else:
    W, H = 480, 320
    p = T.default_params()
    a, l = par.scene_graybox(), T.make_light(480, 160, 80)
r = par.Renderer(p, 0)
r.set_scene(a, par.tile_floor(), l)
fb = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
pal = torch.zeros(W * H, dtype=torch.uint8, device="cuda")
ptrs = {"fb": fb.data_ptr(), "palidx": pal.data_ptr()}
s = torch.cuda.current_stream().cuda_stream
movers = [a[:move].copy(), a[:move].copy()]
movers[1]["px"] += 4
for f in range(n):
    if move and f:
        r.update_aabbs(movers[f % 2], first=0, stream=s)
    r.render_device(ptrs, stream=s, flags=flags | extra)
torch.cuda.synchronize()
print("done", what, n, "frames; occupied columns", r.stats().occupied_columns)
