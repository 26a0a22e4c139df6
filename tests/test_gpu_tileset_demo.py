"""The host demo's tile count (par_demo --gif F ... --tileset TW,TH[,FLIPS]): the T it prints for every frame is
tileset.model's on the index plane decoded from the GIF itself, the GIF is byte for byte the one of the run without the
flag, and the flag's usage errors."""
import os
import re
import subprocess

import pytest

import tileset as TS
from test_gpu_quantize_demo import index_planes

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^tileset frame (\d+): (\d+) tiles of (\d+) cells$", flags=re.M)


def run(par, gif, *flags, frames=3):
    exe = os.path.join(os.path.dirname(par.LIB_PATH), "par_demo")
    assert os.path.exists(exe), "build with make -C pixel-art-raytracer_amd/csrc"
    p = subprocess.run([exe, "--frames", str(frames), "--gif", str(gif), *flags], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p.stdout


@pytest.mark.parametrize("flags,tile,flips", [
    (["--palette-fit", "16", "--cells", "8,8", "--tileset", "8,8,3"], (8, 8), 3),
    (["--palette-levels", "8", "--dither", "24", "--tileset", "16,8"], (16, 8), 0),
])
def test_demo_prints_the_models_tile_count_and_leaves_the_gif_alone(par, T, tmp_path, flags, tile, flips):
    params = T.default_params()
    w, h = params.width, params.height
    with_flag, without = tmp_path / "with.gif", tmp_path / "without.gif"
    out = run(par, with_flag, *flags)
    plain = run(par, without, *flags[:flags.index("--tileset")])
    assert not LINE.search(plain), "without the flag nothing is printed"
    data = with_flag.read_bytes()
    assert data == without.read_bytes(), "the flag changes no byte of the GIF"
    planes = index_planes(data)
    lines = [tuple(int(x) for x in m) for m in LINE.findall(out)]
    assert len(planes) == 3 and [f for f, _, _ in lines] == [0, 1, 2]
    gcx, gcy = TS.grid(w, h, tile)
    counts = []
    for f, count, cells in lines:
        assert cells == gcx * gcy
        assert count == TS.model(planes[f], w, h, tile, 0, flips)[2], f"frame {f}"
        counts.append(count)
    assert all(1 < c < gcx * gcy for c in counts), counts


def test_demo_refuses_tileset_without_an_index_plane(par, tmp_path):
    exe = os.path.join(os.path.dirname(par.LIB_PATH), "par_demo")
    gif = str(tmp_path / "a.gif")
    for flags in (["--gif", gif, "--tileset", "8,8"],
                  ["--palette-levels", "8", "--tileset", "8,8"],
                  ["--gif", gif, "--palette-levels", "8", "--tileset", "8"],
                  ["--gif", gif, "--palette-levels", "8", "--tileset", "8,12"],
                  ["--gif", gif, "--palette-levels", "8", "--tileset", "32,8"],
                  ["--gif", gif, "--palette-levels", "8", "--tileset", "8,8,4"],
                  ["--gif", gif, "--palette-levels", "8", "--tileset", "8,8,-1"],
                  ["--gif", gif, "--palette-levels", "8", "--tileset", "8,8x"],
                  ["--gif", gif, "--palette-levels", "8", "--tileset", "8,8,3x"]):
        p = subprocess.run([exe, "--frames", "1", *flags], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2, (flags, p.returncode, p.stderr)
        assert "--tileset" in p.stderr, (flags, p.stderr)
    assert not os.path.exists(gif), "a refused run writes nothing"
