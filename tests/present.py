"""Present (par_present_device, par_present_host) restated on the host: the contract beside the declarations in
include/par_raytracer.h in numpy (`model`: np.repeat on both axes, the clamp, the exchange, the pitch), and the same for
one output pixel at a time in plain Python integers (`slow_model`, which tests/test_present_cpu.py holds `model` to)."""
import numpy as np

RGBA, BGRA = 0, 1


def _desc(desc):
    d = np.asarray(desc).reshape(-1)[0]
    return int(d["scale_x"]), int(d["scale_y"]), int(d["pitch"]), int(d["order"])


def model(params, desc, rows, fb=None, index=None, palette=None, guard=0):
    """The (rows * sy, pitch) uint8 surface block of rows `rows` (None: the whole frame) of the flat COLOR array `fb`, or
    of the flat uint8 array `index` through the COLOR array `palette`; the gap bytes of every row hold `guard`."""
    sx, sy, pitch, order = _desc(desc)
    r0, r1 = rows or (0, params.height)
    W = params.width
    assert (fb is None) != (index is None)
    if index is not None:
        k = np.minimum(np.asarray(index, dtype=np.int64), len(palette) - 1)  # the clamp
        c = np.ascontiguousarray(palette)[k]
    else:
        c = np.ascontiguousarray(fb)
    assert len(c) == (r1 - r0) * W
    px = c.view(np.uint8).reshape(r1 - r0, W, 4)
    if order == BGRA:
        px = px[:, :, [2, 1, 0, 3]]
    big = np.repeat(np.repeat(px, sy, axis=0), sx, axis=1)
    out = np.full(((r1 - r0) * sy, pitch), guard, dtype=np.uint8)
    out[:, :4 * W * sx] = big.reshape((r1 - r0) * sy, 4 * W * sx)
    return out


def slow_model(params, desc, rows, fb=None, index=None, palette=None, guard=0):
    """`model`, one output pixel at a time in Python integers."""
    sx, sy, pitch, order = _desc(desc)
    r0, r1 = rows or (0, params.height)
    W = params.width
    out = np.full(((r1 - r0) * sy, pitch), guard, dtype=np.uint8)
    for Y in range(r0 * sy, r1 * sy):
        for X in range(W * sx):
            s = (Y // sy - r0) * W + X // sx
            if index is not None:
                e = palette[min(int(index[s]), len(palette) - 1)]
            else:
                e = fb[s]
            c = [int(e["red"]), int(e["green"]), int(e["blue"]), int(e["alpha"])]
            if order == BGRA:
                c[0], c[2] = c[2], c[0]
            out[Y - r0 * sy, 4 * X:4 * X + 4] = c
    return out


def random_colors(T, rng, n, alpha=(0, 255)):
    a = np.zeros(n, dtype=T.COLOR)
    for ch in ("red", "green", "blue"):
        a[ch] = rng.integers(0, 256, n, dtype=np.uint8)
    a["alpha"] = rng.integers(alpha[0], alpha[1] + 1, n).astype(np.uint8)
    return a
