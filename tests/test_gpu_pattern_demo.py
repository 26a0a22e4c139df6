"""The host demo's pattern dither (par_demo --gif F --palette-fit N --palette-refine I --dither-pattern D[,S]): every
image's local colour table is the model's refined palette of the frame the demo also writes as PPM, and every index
plane is pattern.model's over that palette; with --palette-levels the planes are the model's over the ramp; the flag is
refused without a palette, together with --dither or --finish, and outside its ranges."""
import os
import subprocess

import numpy as np
import pytest

import palette as P
import palette_refine as R
import pattern as D
import quantize as Q
from test_gpu_more import _decode_gif
from test_gpu_quantize_demo import as_colors, colour_tables, demo, index_planes

pytestmark = pytest.mark.gpu


def test_demo_dithers_each_frame_towards_its_refined_palette(par, T, tmp_path):
    params = T.default_params()
    data, ppm = demo(par, tmp_path, "pattern", "--palette-fit", "33", "--palette-refine", "2", "--dither-pattern", "8")
    plain, ppm_plain = demo(par, tmp_path, "plain", "--palette-fit", "33", "--palette-refine", "2")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ppm, ppm_plain)), "the PPM frames stay as they are"
    tables, frames, indices = colour_tables(data), _decode_gif(data), index_planes(data)
    plain_indices = index_planes(plain)
    assert len(tables) == len(frames) == len(indices) == 2
    for f in range(2):
        fb = as_colors(T, ppm[f])
        fitted, n_entries, _ = P.fit(T, fb, 33)
        assert 1 < n_entries <= 33
        refined, _, _ = R.refine(T, params, fb, None, fitted, 2)
        rgb = np.stack([refined[c] for c in Q.CHANNELS], axis=1)
        assert tables[f].shape == (256, 3)
        assert np.array_equal(tables[f][:33], rgb), f"frame {f}: the colour table starts with the refined palette"
        assert not tables[f][33:].any()
        index, out = D.model(params, refined, fb, None, 8, 256)
        ordered = Q.model(params, refined, fb, None, 0)
        assert (index != ordered[0]).any(), "the dither should show"
        before, after = D.block_error(params, None, fb, ordered[1]), D.block_error(params, None, fb, out)
        print(f"frame {f}: block error {before} at spread 0, {after} under pattern dither at depth 8")
        assert np.array_equal(indices[f], index), f"frame {f}: the indices are the model's"
        assert np.array_equal(frames[f], rgb[index]), f"frame {f}: and decode to the refined colours"
        assert np.array_equal(plain_indices[f], ordered[0]), f"frame {f}: without the flag, quantise at spread 0"


def test_demo_takes_a_strength_and_a_ramp(par, T, tmp_path):
    params = T.default_params()
    ramp = Q.ramp_array(T, params, 8)
    data, ppm = demo(par, tmp_path, "ramp", "--palette-levels", "8", "--dither-pattern", "5,128")
    indices = index_planes(data)
    for f in range(2):
        fb = as_colors(T, ppm[f])
        assert np.array_equal(indices[f], D.model(params, ramp, fb, None, 5, 128)[0]), f"frame {f}"


def test_demo_refuses_what_does_not_go_together(par, tmp_path):
    exe = os.path.join(os.path.dirname(par.LIB_PATH), "par_demo")
    gif = str(tmp_path / "a.gif")
    fit = ["--palette-fit", "33"]
    for flags in (["--dither-pattern", "8"], ["--palette-refine", "2", "--dither-pattern", "8"],
                  fit + ["--dither-pattern", "8", "--dither", "32"], fit + ["--dither", "0", "--dither-pattern", "8"],
                  ["--palette-levels", "8", "--dither-pattern", "8", "--finish", "--out", str(tmp_path)],
                  fit + ["--dither-pattern", "0"], fit + ["--dither-pattern", "17"], fit + ["--dither-pattern", "8,-1"],
                  fit + ["--dither-pattern", "8,257"], fit + ["--dither-pattern", "8x"], fit + ["--dither-pattern", "8,"],
                  fit + ["--dither-pattern", "8,256,1"]):
        p = subprocess.run([exe, "--frames", "1", "--gif", gif, *flags], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2, (flags, p.returncode, p.stderr)
        assert "--dither-pattern" in p.stderr or "--palette-refine wants" in p.stderr or "--palette-fit cannot" in p.stderr
    assert not os.path.exists(gif), "a refused run writes nothing"
