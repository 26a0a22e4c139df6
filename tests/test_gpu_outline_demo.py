"""The host demo's outlines (par_demo --outline S,C,D): every frame it writes equals the model (outline.model) applied
to the frame it writes without the flag and to that frame's G-buffer, rendered here from the demo's scene; with
--palette-levels the outlined frame is what gets quantised (outline, then quantise); a style of 256,256 changes
no byte of the demo's output."""
import numpy as np
import pytest

import outline as O
import quantize as Q
from test_gpu_quantize_demo import H, W, as_colors, demo, index_planes

pytestmark = pytest.mark.gpu

STYLE = (4, 128, 320)  # depth step, silhouette scale, crease scale: --outline 128,320,4


@pytest.fixture(scope="module")
def demo_gbufs(par, T):
    """The G-buffers of the demo's first two frames: the graybox world, then its key R (entity 0 five to the right)."""
    params = T.default_params()
    aabbs = par.scene_graybox(W, H)
    gbufs = []
    with par.Renderer(params) as r:
        r.set_scene(aabbs, par.tile_floor(), T.make_light(W, H // 2, H // 4))
        for f in range(2):
            if f == 1:
                aabbs[0]["px"] += 5
                r.update_aabbs(aabbs[:1])
            gbufs.append(r.render(("gbuf",))["gbuf"])
    assert gbufs[0].tobytes() != gbufs[1].tobytes()
    return params, gbufs


@pytest.fixture(scope="module")
def plain(par, tmp_path_factory):
    """(GIF bytes, PPM frames) of the demo without the flag."""
    return demo(par, tmp_path_factory.mktemp("demo"), "plain")


def rgb_of(fb):
    return np.stack([fb[c] for c in Q.CHANNELS], axis=1)


def test_demo_outlines_the_frames_it_writes(par, T, tmp_path, demo_gbufs, plain):
    params, gbufs = demo_gbufs
    plain_gif, plain = plain
    _, outlined = demo(par, tmp_path, "outlined", "--outline", "128,320,4")
    for f in range(2):
        edge, exp = O.model(params, STYLE, gbufs[f], (0, H), as_colors(T, plain[f]), (0, H))
        assert (edge == 1).sum() > 100 and (edge == 2).sum() > 100, np.bincount(edge)
        assert (rgb_of(exp) != plain[f]).any(axis=1).sum() > 100, "the lines should show"
        assert np.array_equal(outlined[f], rgb_of(exp)), f"frame {f}"
    # a style that changes no colour: the demo's output without the flag, byte for byte
    gif, frames = demo(par, tmp_path, "neutral", "--outline", "256,256,4")
    assert gif == plain_gif and all(a.tobytes() == b.tobytes() for a, b in zip(frames, plain))


def test_demo_outlines_then_quantises(par, T, tmp_path, demo_gbufs, plain):
    params, gbufs = demo_gbufs
    ramp = Q.ramp_array(T, params, 8)
    _, plain = plain
    data, ppm = demo(par, tmp_path, "both", "--outline", "128,320,4", "--palette-levels", "8", "--dither", "32")
    indices = index_planes(data)
    assert len(indices) == 2
    for f in range(2):
        fb = as_colors(T, plain[f])
        exp = O.model(params, STYLE, gbufs[f], (0, H), fb, (0, H))[1]
        assert np.array_equal(ppm[f], rgb_of(exp)), f"frame {f}: the PPM is the outlined frame, unquantised"
        index = Q.model(params, ramp, exp, None, 32)[0]
        assert (index != Q.model(params, ramp, fb, None, 32)[0]).any(), "the lines should show in the indices"
        assert np.array_equal(indices[f], index), f"frame {f}: the indices are those of the outlined frame"
