"""The host demo's fitted palettes (par_demo --gif F --palette-fit N [--dither S]): every image's local colour table is
the model's fitted palette (palette.fit) of the frame the demo also writes as PPM, and every index plane is
quantize.model's over that palette; the flag is refused together with --palette-levels and with --finish."""
import os
import subprocess

import numpy as np
import pytest

import palette as P
import quantize as Q
from test_gpu_more import _decode_gif
from test_gpu_quantize_demo import as_colors, colour_tables, demo, index_planes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dither", [0, 32])
def test_demo_writes_each_frame_over_its_fitted_palette(par, T, tmp_path, dither):
    params = T.default_params()
    data, ppm = demo(par, tmp_path, f"fit{dither}", "--palette-fit", "33", "--dither", str(dither))
    tables, frames, indices = colour_tables(data), _decode_gif(data), index_planes(data)
    assert len(tables) == len(frames) == len(indices) == 2
    assert ppm[0].tobytes() != ppm[1].tobytes()
    for f in range(2):
        fb = as_colors(T, ppm[f])
        palette, n_entries, _ = P.fit(T, fb, 33)
        assert 1 < n_entries <= 33
        rgb = np.stack([palette[c] for c in Q.CHANNELS], axis=1)
        assert tables[f].shape == (256, 3)
        assert np.array_equal(tables[f][:33], rgb), f"frame {f}: the colour table starts with the fitted palette"
        assert not tables[f][33:].any()
        index = Q.model(params, palette, fb, None, dither)[0]
        if dither:
            assert (index != Q.model(params, palette, fb, None, 0)[0]).any(), "the dither should show"
        assert np.array_equal(indices[f], index), f"frame {f}: the indices are the model's"
        assert np.array_equal(frames[f], rgb[index]), f"frame {f}: and decode to the fitted colours"


def test_demo_refuses_a_second_palette(par, tmp_path):
    exe = os.path.join(os.path.dirname(par.LIB_PATH), "par_demo")
    gif = str(tmp_path / "a.gif")
    for flags in (["--palette-fit", "33", "--palette-levels", "8"],
                  ["--palette-levels", "8", "--palette-fit", "33"],
                  ["--palette-fit", "33", "--finish", "--out", str(tmp_path), "--outline", "128,320,4"],
                  ["--palette-fit", "0"], ["--palette-fit", "257"], ["--palette-fit", "8x"]):
        p = subprocess.run([exe, "--frames", "1", "--gif", gif, *flags], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2, (flags, p.returncode, p.stderr)
        assert "--palette-fit" in p.stderr
    assert not os.path.exists(gif), "a refused run writes nothing"
