"""The host demo's shared tile set (par_demo --gif F ... --tileset TW,TH[,FLIPS] --tileset-shared CAP): the `tileset
frame` lines and the GIF are those of the run without the new flag, the `tileset shared frame` lines are
tileset_extend.sequence_model's over the index planes decoded from the GIF itself, with a capacity that holds the
animation and with one small enough to overflow, and the flag's usage errors."""
import os
import re
import subprocess

import pytest

import tileset as TS
import tileset_extend as TX
from test_gpu_quantize_demo import index_planes
from test_gpu_tileset_demo import LINE, run

pytestmark = pytest.mark.gpu

SHARED = re.compile(r"^tileset shared frame (\d+): (\d+) new, (\d+) tiles, capacity (\d+)$", flags=re.M)


def test_demo_prints_the_models_shared_counts_and_leaves_the_rest_alone(par, T, tmp_path):
    params = T.default_params()
    w, h, tile, flips = params.width, params.height, (8, 8), 3
    flags = ["--palette-fit", "33", "--tileset", "8,8,3"]
    with_flag, without, small = tmp_path / "with.gif", tmp_path / "without.gif", tmp_path / "small.gif"
    out = run(par, with_flag, *flags, "--tileset-shared", "1024", frames=4)
    plain = run(par, without, *flags, frames=4)
    assert not SHARED.search(plain), "without the flag nothing of it is printed"
    assert LINE.findall(out) == LINE.findall(plain) and len(LINE.findall(out)) == 4, "the tileset frame lines are unchanged"
    assert [l for l in out.splitlines() if l.startswith("tileset frame")] == [l for l in plain.splitlines() if l.startswith("tileset frame")]
    lines = out.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("tileset frame")]
    assert all(lines[i + 1].startswith(f"tileset shared frame {k}: ") for k, i in enumerate(at)), "after each frame's line"
    data = with_flag.read_bytes()
    assert data == without.read_bytes(), "the flag changes no byte of the GIF"
    planes = index_planes(data)
    assert len(planes) == 4
    exp, _ = TX.sequence_model(planes, w, h, tile, 0, flips, 1024)
    got = [tuple(int(x) for x in m) for m in SHARED.findall(out)]
    assert got == [(k, e[2] - e[3], e[2], 1024) for k, e in enumerate(exp)], (got, [(e[3], e[2]) for e in exp])
    assert exp[0][2] == TS.model(planes[0], w, h, tile, 0, flips)[2] and all(e[2] > e[3] for e in exp[1:])
    # a capacity small enough to overflow: from then on tiles that were not stored count again
    capacity = exp[0][2] // 2
    out = run(par, small, *flags, "--tileset-shared", str(capacity), frames=4)
    assert small.read_bytes() == data
    exp, _ = TX.sequence_model(planes, w, h, tile, 0, flips, capacity)
    got = [tuple(int(x) for x in m) for m in SHARED.findall(out)]
    assert got == [(k, e[2] - e[3], e[2], capacity) for k, e in enumerate(exp)], (got, [(e[3], e[2]) for e in exp])
    assert exp[0][2] > capacity and exp[3][2] >= exp[0][2] + 3 * (exp[0][2] - capacity) // 2, "unstored tiles count again"


def test_demo_refuses_tileset_shared_without_tileset(par, tmp_path):
    exe = os.path.join(os.path.dirname(par.LIB_PATH), "par_demo")
    gif = str(tmp_path / "a.gif")
    for flags in (["--gif", gif, "--palette-fit", "33", "--tileset-shared", "256"],
                  ["--tileset-shared", "256"],
                  ["--gif", gif, "--palette-fit", "33", "--tileset", "8,8", "--tileset-shared", "-1"],
                  ["--gif", gif, "--palette-fit", "33", "--tileset", "8,8", "--tileset-shared", "1048577"],
                  ["--gif", gif, "--palette-fit", "33", "--tileset", "8,8", "--tileset-shared", "256x"],
                  ["--gif", gif, "--palette-fit", "33", "--tileset", "8,8", "--tileset-shared", "x"]):
        p = subprocess.run([exe, "--frames", "1", *flags], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2, (flags, p.returncode, p.stderr)
        assert "--tileset-shared" in p.stderr, (flags, p.stderr)
    # (--tileset's own conditions still hold with the new flag beside it)
    p = subprocess.run([exe, "--frames", "1", "--gif", gif, "--tileset", "8,8", "--tileset-shared", "256"], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 2 and "--tileset wants" in p.stderr
    assert not os.path.exists(gif), "a refused run writes nothing"
