"""Palette output (par_quantize_device, par_quantize_host, par_palette_ramp) restated on the host: the contract beside
the declarations in include/par_raytracer.h in numpy int32 (`model`), the same for one pixel at a time in plain Python
integers (`model_loop`, which tests/test_quantize_cpu.py holds `model` to), and the ramp in plain Python integers."""
import numpy as np

BAYER4 = ((0, 8, 2, 10), (12, 4, 14, 6), (3, 11, 1, 9), (15, 7, 13, 5))
CHANNELS = ("red", "green", "blue")


def dithered(params, fb, rows, spread):
    """(n, 3) int32: the channels c' = min(255, max(0, c + off)) of the rows' pixels, and the (n, 3) sums c + off before
    the clamp (what a test needs to show that its inputs clamp)."""
    r0, r1 = rows or (0, params.height)
    W = params.width
    n = (r1 - r0) * W
    assert len(fb) == n
    i = np.arange(n, dtype=np.int64)
    x, y = i % W, r0 + i // W
    t = np.array(BAYER4, dtype=np.int32)[y & 3, x & 3]
    off = np.floor_divide((2 * t - 15) * np.int32(spread), np.int32(32)).astype(np.int32)
    raw = np.stack([fb[c].astype(np.int32) for c in CHANNELS], axis=1) + off[:, None]
    return np.clip(raw, 0, 255).astype(np.int32), raw


def distances(params, palette, fb, rows, spread, with_alpha=False):
    """(n, n_colors) int32 L1 distances d_p of the contract. with_alpha: the alpha bytes counted in (NOT the contract:
    what a test compares with to show that its inputs would tell the difference)."""
    c, _ = dithered(params, fb, rows, spread)
    pal = np.stack([palette[ch].astype(np.int32) for ch in CHANNELS], axis=1)
    d = np.abs(c[:, None, :] - pal[None, :, :]).sum(axis=2, dtype=np.int32)
    if with_alpha:
        d = d + np.abs(fb["alpha"].astype(np.int32)[:, None] - palette["alpha"].astype(np.int32)[None, :])
    return d


def model(params, palette, fb, rows, spread, with_alpha=False):
    """(index, fb_out) of rows `rows` (None: the whole frame) of the frame block `fb` (a flat COLOR array holding those
    rows) against `palette` (a COLOR array)."""
    d = distances(params, palette, fb, rows, spread, with_alpha)
    k = np.argmin(d, axis=1)  # the first minimum: the lowest index among equals
    out = fb.copy()
    for ch in CHANNELS:
        out[ch] = palette[ch][k]
    out["alpha"] = fb["alpha"]  # the pixel's own alpha passes through
    return k.astype(np.uint8), out


def model_loop(params, palette, fb, rows, spread):
    """`model`, one pixel and one palette entry at a time in Python integers."""
    r0, r1 = rows or (0, params.height)
    W = params.width
    index = np.zeros(len(fb), dtype=np.uint8)
    out = fb.copy()
    for i in range((r1 - r0) * W):
        x, y = i % W, r0 + i // W
        off = ((2 * BAYER4[y & 3][x & 3] - 15) * spread) // 32  # Python's // floors
        c = [min(255, max(0, int(fb[ch][i]) + off)) for ch in CHANNELS]
        best, k = None, None
        for p in range(len(palette)):
            d = sum(abs(c[j] - int(palette[ch][p])) for j, ch in enumerate(CHANNELS))
            if best is None or d < best:
                best, k = d, p
        index[i] = k
        for ch in CHANNELS:
            out[ch][i] = palette[ch][k]
    return index, out


def ramp(params, levels):
    """par_palette_ramp as a list of (red, green, blue, alpha) in Python integers (the two float products as the C code
    forms them, in float32)."""
    a = int(np.float32(params.ambient) * np.float32(255))
    rows = []
    for p in range(params.palette_size):
        e = params.palette[p]
        for k in range(levels):
            s = a + ((255 - a) * k) // (levels - 1)
            rows.append(((e.red * s) // 255, (e.green * s) // 255, (e.blue * s) // 255, e.alpha))
    ch = int(np.float32(params.background) * np.float32(params.ambient)) & 0xFF
    rows.append((ch, ch, ch, 0))
    return rows


def ramp_array(T, params, levels):
    rows = ramp(params, levels)
    a = np.zeros(len(rows), dtype=T.COLOR)
    for i, (r, g, b, al) in enumerate(rows):
        a[i]["red"], a[i]["green"], a[i]["blue"], a[i]["alpha"] = r, g, b, al
    return a


def random_colors(T, rng, n, alpha=None):
    """n random COLOR entries; alpha: None = random bytes, else (lo, hi) inclusive."""
    a = np.zeros(n, dtype=T.COLOR)
    for ch in CHANNELS:
        a[ch] = rng.integers(0, 256, n, dtype=np.uint8)
    lo, hi = alpha or (0, 255)
    a["alpha"] = rng.integers(lo, hi + 1, n).astype(np.uint8)
    return a
