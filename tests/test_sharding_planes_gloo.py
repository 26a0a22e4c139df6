"""The N > 1 path for planes other than fb, on CPU: world_size 2 and 3 over gloo. Row blocks of the palidx plane (and,
in one case, of the G-buffer) made independently and assembled on rank 0 by TileGather(elem_bytes=..., fill=...) from the
tiles that can show a primitive must be byte-identical to the whole frame's plane, with the root's block packed like every
other ("tiles") and produced in place ("tiles_in_place")."""
import os
import subprocess
import sys

import pytest

from test_sharding_gloo import ROOT, free_port


@pytest.mark.parametrize("world,height,mode,plane", [(2, 320, "tiles", "palidx"), (3, 200, "tiles", "palidx"),
                                                     (2, 320, "tiles_in_place", "palidx"),
                                                     (3, 200, "tiles_in_place", "palidx"),
                                                     (3, 200, "tiles_in_place", "gbuf")])
def test_tile_gather_assembles_the_plane(tmp_path, world, height, mode, plane):
    out = tmp_path / "result.txt"
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "_gloo_planes_worker.py"), str(height), "240", str(out), mode, plane]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert out.read_text() == "ok"
