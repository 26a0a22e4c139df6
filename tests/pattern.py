"""Pattern dither (par_quantize_pattern_device, par_quantize_pattern_host) restated on the host: the contract beside the
declarations in include/par_raytracer.h in numpy int32 / int64 (`model`), the same for one pixel, one entry and one
candidate at a time in plain Python integers with a plain `sorted` (`model_loop`, which tests/test_pattern_cpu.py holds
`model` to), and the figure the quality comparison uses (`block_error`)."""
import numpy as np

from quantize import BAYER4, CHANNELS

CHUNK = 1 << 14  # pixels of one step of the search: bounds the (pixels, entries) temporaries


def _nearest(t, pal):
    """The index par_quantize_device gives each colour of t (n, 3) at spread 0 against pal (m, 3): L1-nearest, the lowest
    index among equals."""
    k = np.empty(len(t), dtype=np.int64)
    for at in range(0, len(t), CHUNK):
        part = t[at:at + CHUNK]
        d = np.zeros((len(part), len(pal)), dtype=np.int32)
        for ch in range(3):
            d += np.abs(part[:, ch, None] - pal[None, :, ch])
        k[at:at + CHUNK] = np.argmin(d, axis=1)  # the first minimum
    return k


def candidates(palette, fb, depth, strength):
    """(n, depth) int64: the sort keys of every pixel's candidates in the order they are found, and the largest |e| met."""
    c = np.stack([fb[ch].astype(np.int32) for ch in CHANNELS], axis=1)
    pal = np.stack([palette[ch].astype(np.int32) for ch in CHANNELS], axis=1)
    luma = 77 * pal[:, 0].astype(np.int64) + 150 * pal[:, 1] + 29 * pal[:, 2]
    e = np.zeros_like(c, dtype=np.int64)
    keys = np.empty((len(c), depth), dtype=np.int64)
    largest = 0
    for j in range(depth):
        t = np.clip(c + np.floor_divide(e * strength, 256), 0, 255).astype(np.int32)
        k = _nearest(t, pal)
        e += c - pal[k]
        largest = max(largest, int(np.abs(e).max()) if len(e) else 0)
        keys[:, j] = (luma[k] << 8) | k
    return keys, largest


def ranks(params, n, rows, depth):
    r0, r1 = rows or (0, params.height)
    W = params.width
    assert n == (r1 - r0) * W
    i = np.arange(n, dtype=np.int64)
    x, y = i % W, r0 + i // W
    return (np.array(BAYER4, dtype=np.int64)[y & 3, x & 3] * depth) >> 4


def model(params, palette, fb, rows, depth, strength):
    """(index, fb_out) of rows `rows` (None: the whole frame) of the frame block `fb` (a flat COLOR array holding those
    rows) against `palette` (a COLOR array)."""
    keys, _ = candidates(palette, fb, depth, strength)
    keys.sort(axis=1)
    rank = ranks(params, len(fb), rows, depth)
    k = keys[np.arange(len(fb)), rank] & 255
    out = fb.copy()
    for ch in CHANNELS:
        out[ch] = palette[ch][k]
    out["alpha"] = fb["alpha"]  # the pixel's own alpha passes through
    return k.astype(np.uint8), out


def model_loop(params, palette, fb, rows, depth, strength):
    """`model`, one pixel, one entry and one candidate at a time in Python integers."""
    r0, r1 = rows or (0, params.height)
    W = params.width
    assert len(fb) == (r1 - r0) * W
    pal = [tuple(int(palette[ch][p]) for ch in CHANNELS) for p in range(len(palette))]
    px = [tuple(int(fb[ch][i]) for ch in CHANNELS) for i in range(len(fb))]
    index = np.zeros(len(fb), dtype=np.uint8)
    out = fb.copy()
    for i, c in enumerate(px):
        x, y = i % W, r0 + i // W
        e = [0, 0, 0]
        keys = []
        for _ in range(depth):
            t = [min(255, max(0, c[ch] + (e[ch] * strength) // 256)) for ch in range(3)]  # Python's // floors
            best, k = None, None
            for p, entry in enumerate(pal):
                d = abs(t[0] - entry[0]) + abs(t[1] - entry[1]) + abs(t[2] - entry[2])
                if best is None or d < best:
                    best, k = d, p
            for ch in range(3):
                e[ch] += c[ch] - pal[k][ch]
            keys.append(((77 * pal[k][0] + 150 * pal[k][1] + 29 * pal[k][2]) << 8) | k)
        k = sorted(keys)[(BAYER4[y & 3][x & 3] * depth) >> 4] & 255
        index[i] = k
        for ch in range(3):
            out[CHANNELS[ch]][i] = pal[k][ch]
    return index, out


def block_error(params, rows, fb, out):
    """The sum, over red, green and blue and over the aligned 4 x 4 blocks of the rows, of |sum of the block's source
    bytes - sum of its output bytes|: what a viewer at arm's length sees. The rows and the width are multiples of 4."""
    r0, r1 = rows or (0, params.height)
    W, H = params.width, r1 - r0
    assert W % 4 == 0 and H % 4 == 0 and r0 % 4 == 0 and len(fb) == len(out) == W * H
    total = 0
    for ch in CHANNELS:
        d = fb[ch].astype(np.int64) - out[ch].astype(np.int64)
        total += int(np.abs(d.reshape(H // 4, 4, W // 4, 4).sum(axis=(1, 3))).sum())
    return total
