"""Finish (par_finish_device, par_finish_host) restated on the host: `model` is the composition of outline.model,
quantize.model and present.model and nothing more, as the contract beside the declarations in include/par_raytracer.h is
the composition of the three contracts. tests/test_finish_cpu.py holds it to the three per-pixel loops.

A stage that does not run is passed as None: `style` (with `gbuf`, `grows`) for the outlines, `palette` for the palette."""
import numpy as np

import outline as O
import present as P
import quantize as Q


def model(params, style, gbuf, grows, palette, spread, desc, fb, rows, guard=0):
    """(surface, index): the (rows * sy, pitch) uint8 surface block of rows `rows` (None: the whole frame) of the frame
    block `fb`, its gap bytes holding `guard`, and the index plane of those rows (None without a palette)."""
    rows = rows or (0, params.height)
    assert style is not None or palette is not None, "neither stage: that call is present"
    a = fb if style is None else O.model(params, style, gbuf, grows, fb, rows)[1]
    if palette is None:
        return P.model(params, desc, rows, fb=a, guard=guard), None
    index = Q.model(params, palette, a, rows, spread)[0]
    return P.model(params, desc, rows, index=index, palette=palette, guard=guard), index


STAGE_SETS = ("outline+quantise", "outline", "quantise")


def stages(stage_set, style, gbuf, grows, palette, spread):
    """The (style, gbuf, grows, palette, spread) that `model` takes for one of STAGE_SETS."""
    assert stage_set in STAGE_SETS
    if "outline" not in stage_set:
        style, gbuf, grows = None, None, None
    if "quantise" not in stage_set:
        palette, spread = None, 0
    return style, gbuf, grows, palette, spread


STYLE = (2, 128, 320)  # (depth_step, silhouette_scale, crease_scale): random_texels' keys are a few steps apart
SPREAD = 32


def inputs(T, w, h, n_colors=17, seed=None):
    """(params, gbuf, fb, palette) of a w x h frame: outline.random_texels (every clause of the outline contract is met
    often), random colours, and a random palette of non-zero varied alpha. The seed defaults to 1000 * w + h."""
    rng = np.random.default_rng(1000 * w + h if seed is None else seed)
    params = T.default_params(w, h)
    gbuf = O.random_texels(T, rng, params, w * h)
    fb = O.random_colors(T, rng, w * h)
    palette = P.random_colors(T, rng, n_colors, alpha=(1, 255))
    return params, gbuf, fb, palette


def block_inputs(params, gbuf, fb, rows, grows):
    """The G-buffer rows `grows` and the frame rows `rows` of whole-frame planes."""
    return O.block(gbuf, params.width, grows), O.block(fb, params.width, rows)
