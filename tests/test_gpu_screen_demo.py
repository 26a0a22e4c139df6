"""The host demo's screen (par_demo ... --vram MACHINE,DIR --vram-show [backdrop]): every `screen frame` line and the
frame_<i>.ppm of every frame are the model's (tests/screen.py) run over the .chr, .map and .pal files the demo itself wrote,
against the cells frame decoded from the GIF it wrote; without --vram-show the demo prints and writes what it does with the
flag less the `screen frame` lines and the PPMs, so its existing lines (which test_gpu_vram_demo.py holds to the model) are
unchanged; and the flag's usage error."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import screen as S
import tileset as TS
import vram as V
from test_gpu_quantize_demo import colour_tables, index_planes

pytestmark = pytest.mark.gpu

importlib.import_module("pixel-art-raytracer_amd.screen")  # (without the add-on's binding nothing here can run)

LINE = re.compile(r"^screen frame (\d+): bad (\d+), error (\d+)$", flags=re.M)
VRAM_LINE = re.compile(r"^vram frame (\d+): (\d+) tiles \((\d+) flat\), (\d+) tile bytes, (\d+) map bytes, bad (\d+)$", flags=re.M)
FRAMES = 2


def run(par, gif, *flags):
    exe = os.path.join(os.path.dirname(par.LIB_PATH), "par_demo")
    assert os.path.exists(exe), "build with make -C pixel-art-raytracer_amd/csrc"
    p = subprocess.run([exe, "--frames", str(FRAMES), "--gif", str(gif), *flags], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return re.sub(r"\d+\.\d+ms", "ms", p.stdout)  # (the frame line's render time is the one thing that differs run to run)


@pytest.mark.parametrize("machine,flags,cell,shape,backdrop", [
    ("snes", ["--palette-fit", "33", "--cells", "8,8", "--cells-fit", "8,4", "--tileset", "8,8,3"], (8, 8), (8, 4), 0),
    ("megadrive", ["--palette-fit", "64", "--cells", "16,16", "--cells-fit", "4,16,1", "--tileset", "8,8,1"], (16, 16), (4, 16), 1),
    ("nes", ["--palette-fit", "8", "--cells", "16,8", "--tileset", "8,8"], (16, 8), (28, 2), 1),
])
def test_demo_shows_what_the_model_shows(par, T, tmp_path, machine, flags, cell, shape, backdrop):
    params = T.default_params()
    w, h = params.width, params.height
    n_sub, sub_size = shape
    out, plain_out = tmp_path / "shown", tmp_path / "plain"
    out.mkdir()
    plain_out.mkdir()
    with_flag, without = tmp_path / "with.gif", tmp_path / "without.gif"
    text = run(par, with_flag, *flags, "--vram", f"{machine},{out}", "--vram-show", *(["backdrop"] if backdrop else []))
    plain = run(par, without, *flags, "--vram", f"{machine},{plain_out}")
    # without --vram-show: the same lines less the screen's, the same files less the PPMs, the same GIF
    assert not LINE.search(plain) and [row for row in text.splitlines() if not row.startswith("screen frame ")] == plain.splitlines()
    assert with_flag.read_bytes() == without.read_bytes()
    assert sorted(p.name for p in out.iterdir() if not p.name.endswith(".ppm")) == sorted(p.name for p in plain_out.iterdir())
    for p in plain_out.iterdir():
        assert (out / p.name).read_bytes() == p.read_bytes(), p.name
    # each screen line comes right after its frame's vram line
    rows = text.splitlines()
    for f in range(FRAMES):
        at = [i for i, row in enumerate(rows) if row.startswith(f"vram frame {f}:")]
        assert len(at) == 1 and rows[at[0] + 1].startswith(f"screen frame {f}: bad "), f
    lines = [tuple(int(x) for x in m) for m in LINE.findall(text)]
    vram_lines = [tuple(int(x) for x in m) for m in VRAM_LINE.findall(text)]
    assert [l[0] for l in lines] == list(range(FRAMES))
    data = with_flag.read_bytes()
    planes, tables = index_planes(data), colour_tables(data)
    m = V.MACHINES.index(machine)
    fmt, pal_format = V.MACHINE_FORMATS[m]
    gcx, gcy = TS.grid(w, h, (8, 8))
    for f in range(FRAMES):
        index = planes[f].reshape(-1)
        table = np.concatenate([tables[f][:n_sub * sub_size], np.zeros((n_sub * sub_size, 1), np.uint8)], axis=1)
        chr_bytes = np.frombuffer((out / f"frame_{f:03d}.chr").read_bytes(), dtype=np.uint8)
        words = np.frombuffer((out / f"frame_{f:03d}.map").read_bytes(), dtype=np.uint8)
        n_tiles = vram_lines[f][1]
        assert len(chr_bytes) == n_tiles * V.tile_bytes(fmt, (8, 8)) and len(words) == gcx * gcy * V.preset(m)["word_bytes"]
        d = S.desc_of(V.preset(m), tile_format=fmt, n_tiles=n_tiles, map_w=gcx, map_h=gcy, ratio_x=cell[0] // 8, ratio_y=cell[1] // 8,
                      n_colors=min(256, n_sub * sub_size), sub_size=sub_size, backdrop=backdrop, width=w, height=h)
        if machine == "nes":  # no colour words, and the palette in the attribute grid: the cells' cell_out
            chosen = np.ascontiguousarray((index // sub_size).reshape(h, w)[::cell[1], ::cell[0]]).reshape(-1)
            fb, _, bad = S.draw(d, chr_bytes, words, table.reshape(-1), attr=chosen)
        else:
            pal = np.frombuffer((out / f"frame_{f:03d}.pal").read_bytes(), dtype=np.uint8)
            fb, _, bad = S.draw(dict(d, pal_format=pal_format), chr_bytes, words, pal)
        meant = table[index.astype(np.int64)][:, :3].astype(np.int64).reshape(h, w, 3)
        error = int(np.abs(fb[:, :, :3].astype(np.int64) - meant).sum())
        print(f"{machine} frame {f}: bad {bad}, error {error}, {error / (w * h * 3):.3f} a channel")
        assert lines[f] == (f, bad, error), f"frame {f}"
        assert (out / f"frame_{f:03d}.ppm").read_bytes() == b"P6\n%d %d\n255\n" % (w, h) + fb[:, :, :3].tobytes(), f"frame {f}: the PPM"
        # the truncated colours and the backdrop cost something; RGBA8 entries without a backdrop would cost nothing
        assert error > 0
        assert bad == 0, "every word names a tile of the export (on the nes, past 256 tiles, not the one that was meant)"


def test_demo_refuses_a_screen_without_an_export(par, tmp_path):
    exe = os.path.join(os.path.dirname(par.LIB_PATH), "par_demo")
    gif = str(tmp_path / "a.gif")
    p = subprocess.run([exe, "--frames", "1", "--gif", gif, "--palette-fit", "16", "--cells", "8,8", "--tileset", "8,8", "--vram-show"],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--vram-show wants --vram" in p.stderr, (p.returncode, p.stderr)
    assert not os.path.exists(gif), "a refused run writes nothing"
