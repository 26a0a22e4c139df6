"""The host demo's refined palettes (par_demo --gif F --palette-fit N --palette-refine I): every image's local colour
table is the model's fitted palette of the frame the demo also writes as PPM after I rounds of the model's refinement
(palette.fit, palette_refine.refine), and every index plane is quantize.model's over that palette; without the flag the
GIF is what --palette-fit alone writes; the flag is refused without --palette-fit and outside 1..16."""
import os
import subprocess

import numpy as np
import pytest

import palette as P
import palette_refine as R
import quantize as Q
from test_gpu_more import _decode_gif
from test_gpu_quantize_demo import as_colors, colour_tables, demo, index_planes

pytestmark = pytest.mark.gpu


def test_demo_refines_each_frames_fitted_palette(par, T, tmp_path):
    params = T.default_params()
    data, ppm = demo(par, tmp_path, "refined", "--palette-fit", "33", "--palette-refine", "6")
    plain, ppm_plain = demo(par, tmp_path, "fitted", "--palette-fit", "33")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ppm, ppm_plain)), "the PPM frames stay as they are"
    assert data != plain
    tables, frames, indices = colour_tables(data), _decode_gif(data), index_planes(data)
    plain_tables, plain_indices = colour_tables(plain), index_planes(plain)
    assert len(tables) == len(frames) == len(indices) == 2
    for f in range(2):
        fb = as_colors(T, ppm[f])
        fitted, n_entries, _ = P.fit(T, fb, 33)
        assert 1 < n_entries <= 33
        refined, _, _ = R.refine(T, params, fb, None, fitted, 6)
        before, after = R.error(params, fitted, fb)[0], R.error(params, refined, fb)[0]
        print(f"frame {f}: summed L1 error {before} as fitted, {after} after 6 rounds")
        assert after < before
        rgb = np.stack([refined[c] for c in Q.CHANNELS], axis=1)
        assert tables[f].shape == (256, 3)
        assert np.array_equal(tables[f][:33], rgb), f"frame {f}: the colour table starts with the refined palette"
        assert not tables[f][33:].any()
        index = Q.model(params, refined, fb, None, 0)[0]
        assert np.array_equal(indices[f], index), f"frame {f}: the indices are the model's"
        assert np.array_equal(frames[f], rgb[index]), f"frame {f}: and decode to the refined colours"
        # without the flag: the fitted palette, as before
        assert np.array_equal(plain_tables[f][:33], np.stack([fitted[c] for c in Q.CHANNELS], axis=1))
        assert np.array_equal(plain_indices[f], Q.model(params, fitted, fb, None, 0)[0])


def test_demo_refuses_a_refinement_without_a_fit(par, tmp_path):
    exe = os.path.join(os.path.dirname(par.LIB_PATH), "par_demo")
    gif = str(tmp_path / "a.gif")
    for flags in (["--palette-refine", "6"], ["--palette-levels", "8", "--palette-refine", "6"],
                  ["--palette-fit", "33", "--palette-refine", "0"], ["--palette-fit", "33", "--palette-refine", "17"],
                  ["--palette-fit", "33", "--palette-refine", "2x"]):
        p = subprocess.run([exe, "--frames", "1", "--gif", gif, *flags], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2, (flags, p.returncode, p.stderr)
        assert "--palette-refine wants" in p.stderr
    assert not os.path.exists(gif), "a refused run writes nothing"
