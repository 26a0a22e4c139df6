"""The host demo's colour cells (par_demo --gif F --palette-fit N --cells CW,CH [--palette-refine I] [--dither S]): every
image's local colour table is the flat table of the pairs (cells.pairs) of the model's fitted, refined palette of the
frame the demo also writes as PPM, and every index plane is cells.model's over that table; the flag's usage errors."""
import os
import subprocess

import numpy as np
import pytest

import cells as CM
import palette as P
import palette_refine as R
import quantize as Q
from test_gpu_more import _decode_gif
from test_gpu_quantize_demo import as_colors, colour_tables, demo, index_planes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,cell,refine,dither", [(16, (8, 8), 0, 0), (7, (16, 8), 2, 24)])
def test_demo_writes_each_frame_under_colour_cells(par, T, tmp_path, n, cell, refine, dither):
    params = T.default_params()
    flags = ["--palette-fit", str(n), "--cells", f"{cell[0]},{cell[1]}", "--dither", str(dither)]
    if refine:
        flags += ["--palette-refine", str(refine)]
    data, ppm = demo(par, tmp_path, f"cells{n}", *flags)
    tables, frames, indices = colour_tables(data), _decode_gif(data), index_planes(data)
    assert len(tables) == len(frames) == len(indices) == 2
    assert ppm[0].tobytes() != ppm[1].tobytes()
    n_sub = n * (n - 1) // 2
    for f in range(2):
        fb = as_colors(T, ppm[f])
        palette, n_entries, _ = P.fit(T, fb, n)
        assert 1 < n_entries <= n
        if refine:
            palette = R.refine(T, params, fb, None, palette, refine)[0]
        table = CM.pairs(palette)
        assert len(table) == 2 * n_sub
        rgb = np.stack([table[c] for c in Q.CHANNELS], axis=1)
        assert tables[f].shape == (256, 3)
        assert np.array_equal(tables[f][:2 * n_sub], rgb), f"frame {f}: the colour table starts with the pairs"
        assert not tables[f][2 * n_sub:].any()
        index, _, chosen = CM.model(params, table, n_sub, 2, cell, fb, None, dither)
        assert len(np.unique(chosen)) > 1, "more than one pair wins"
        if dither:
            assert (index != CM.model(params, table, n_sub, 2, cell, fb, None, 0)[0]).any(), "the dither should show"
        assert np.array_equal(indices[f], index), f"frame {f}: the indices are the model's"
        assert np.array_equal(frames[f], rgb[index]), f"frame {f}: and decode to the pairs' colours"


def test_demo_refuses_cells_without_a_small_fitted_palette(par, tmp_path):
    exe = os.path.join(os.path.dirname(par.LIB_PATH), "par_demo")
    gif = str(tmp_path / "a.gif")
    for flags in (["--cells", "8,8"],
                  ["--cells", "8,8", "--palette-levels", "8"],
                  ["--cells", "8,8", "--palette-fit", "17"],
                  ["--palette-fit", "1", "--cells", "8,8"],
                  ["--cells", "8,8", "--palette-fit", "16", "--dither-pattern", "4"],
                  ["--cells", "16,16", "--palette-fit", "16", "--finish", "--out", str(tmp_path), "--outline", "128,320,4"],
                  ["--cells", "8,12", "--palette-fit", "16"], ["--cells", "8", "--palette-fit", "16"],
                  ["--cells", "8,8x", "--palette-fit", "16"], ["--cells", "32,8", "--palette-fit", "16"]):
        p = subprocess.run([exe, "--frames", "1", "--gif", gif, *flags], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2, (flags, p.returncode, p.stderr)
        assert "--cells" in p.stderr or "--palette-fit" in p.stderr, (flags, p.stderr)
    assert not os.path.exists(gif), "a refused run writes nothing"
