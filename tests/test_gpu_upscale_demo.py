"""The host demo's frames through a pixel-art scaler (par_demo --upscale K, with --out): every PPM it writes has the
scaled header and is upscale.model applied to the frame it writes without the flag (par_upscale_host at tight pitch in
RGBA order), after --as-sdl's exchange too; any other K, and the flag together with --scale or --finish, exits with 2 and
writes nothing."""
import os
import subprocess

import numpy as np
import pytest

import upscale as U
from test_gpu_present_demo import H, W, demo

pytestmark = pytest.mark.gpu


def scaled(T, image, k):
    """upscale.model on a (H, W, 3) PPM frame. The demo's frames carry alpha 0 throughout (the graybox sprites' and the
    background's), so equal colours are equal elements."""
    fb = np.zeros(H * W, dtype=T.COLOR)
    fb["red"], fb["green"], fb["blue"] = (image[..., c].reshape(-1) for c in range(3))
    surface = U.model(T.default_params(W, H), T.make_upscale_desc(k, width=W), None, None, fb=fb)[0]
    return surface.reshape(k * H, k * W, 4)[..., :3]


@pytest.mark.parametrize("k", [2, 3, 4])
def test_demo_writes_frames_through_the_scaler(par, T, tmp_path, k):
    _, plain = demo(par, tmp_path / "a")
    assert all(f.shape == (H, W, 3) for f in plain) and plain[0].tobytes() != plain[1].tobytes()
    _, big = demo(par, tmp_path / "b", "--upscale", str(k))
    for f in range(2):
        assert big[f].shape == (k * H, k * W, 3), f"frame {f}: the header is the scaled size"
        assert np.array_equal(big[f], scaled(T, plain[f], k)), f"frame {f}"
        nearest = np.repeat(np.repeat(plain[f], k, axis=0), k, axis=1)
        assert (big[f] != nearest).any(), f"frame {f}: the rules should fire on the scene's diagonals"


def test_demo_scales_the_frame_as_sdl_shows_it(par, T, tmp_path):
    """The scaler acts after --as-sdl's exchange; the exchange shows in the debug line, red in the frame and blue on the
    reference's window."""
    _, sdl = demo(par, tmp_path / "a", "--as-sdl", "--debug-line")
    assert (sdl[0] == (0, 0, 255)).all(axis=2).sum() > 100, "the debug line comes out blue"
    _, big = demo(par, tmp_path / "b", "--upscale", "3", "--as-sdl", "--debug-line")
    for f in range(2):
        assert big[f].shape == (3 * H, 3 * W, 3)
        assert np.array_equal(big[f], scaled(T, sdl[f], 3)), f"frame {f}"


@pytest.mark.parametrize("flags", [("--upscale", "1"), ("--upscale", "5"), ("--upscale", "x"),
                                   ("--upscale", "2", "--scale", "2"),
                                   ("--upscale", "2", "--finish", "--outline", "128,320,4")],
                         ids=["1", "5", "x", "with --scale", "with --finish"])
def test_demo_refuses(par, tmp_path, flags):
    status, _ = demo(par, tmp_path / "bad", *flags, frames=False)
    assert status == 2
    assert not list((tmp_path / "bad").iterdir()), "nothing was written"


def test_demo_wants_out(par, tmp_path):
    exe = os.path.join(os.path.dirname(par.LIB_PATH), "par_demo")
    p = subprocess.run([exe, "--frames", "1", "--upscale", "2"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 2 and "--out" in p.stderr
    assert not list(tmp_path.iterdir()), "nothing was written"
