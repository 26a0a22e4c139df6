"""Colour cells (par_quantize_cells_device, par_quantize_cells_host, par_cells_pairs) restated on the host: the contract
beside the declarations in include/par_cells.h in vectorised numpy (`model`), the same for one cell, one pixel and one
entry at a time in plain Python integers (`model_loop`, which tests/test_cells_cpu.py holds `model` to), and the pairs."""
import itertools

import numpy as np

import quantize as Q

CELLS = ((8, 8), (8, 16), (16, 8), (16, 16))
CHUNK = 1 << 14  # pixels whose distances to every entry are held at once


def admits(rows, height, cell):
    """The row cut rule: rows (None: the whole frame) of a frame `height` high are cut at cell rows of `cell`."""
    r0, r1 = rows or (0, height)
    return r0 % cell[1] == 0 and (r1 % cell[1] == 0 or r1 == height)


def grid(params, cell, rows):
    """(gcx, cell rows of the block)."""
    r0, r1 = rows or (0, params.height)
    return -(-params.width // cell[0]), -(-(r1 - r0) // cell[1])


def nearest(params, palette, n_sub, sub_size, fb, rows, spread):
    """((n, S) int32 d(p, s), (n, S) int32 k(p, s)) of the rows' pixels."""
    c, _ = Q.dithered(params, fb, rows, spread)
    pal = np.stack([palette[ch].astype(np.int32) for ch in Q.CHANNELS], axis=1)
    assert len(pal) == n_sub * sub_size
    d_min = np.zeros((len(c), n_sub), dtype=np.int32)
    k_min = np.zeros((len(c), n_sub), dtype=np.int32)
    for a in range(0, len(c), CHUNK):
        part = c[a:a + CHUNK]
        d = np.zeros((len(part), len(pal)), dtype=np.int32)
        for ch in range(3):
            d += np.abs(part[:, ch, None] - pal[None, :, ch])
        d = d.reshape(len(part), n_sub, sub_size)
        k = np.argmin(d, axis=2)  # the first minimum: the lowest k among equals
        k_min[a:a + CHUNK] = k
        d_min[a:a + CHUNK] = np.take_along_axis(d, k[:, :, None], axis=2)[:, :, 0]
    return d_min, k_min


def model(params, palette, n_sub, sub_size, cell, fb, rows, spread):
    """(index, fb_out, cell_plane) of rows `rows` (None: the whole frame) of the frame block `fb` (a flat COLOR array
    holding those rows) under the n_sub sub-palettes of sub_size entries of `palette` (a flat COLOR array) and cells of
    cell[0] x cell[1] pixels; cell_plane is one uint8 a cell of the block's cell rows."""
    r0, r1 = rows or (0, params.height)
    W, (cw, ch) = params.width, cell
    assert admits(rows, params.height, cell) and len(fb) == (r1 - r0) * W
    gcx, gcy = grid(params, cell, rows)
    d_min, k_min = nearest(params, palette, n_sub, sub_size, fb, rows, spread)
    i = np.arange(len(fb), dtype=np.int64)
    of_cell = (i % W) // cw + ((i // W) // ch) * gcx  # (row_begin is a multiple of cell_h: the block's own rows will do)
    E = np.zeros((gcx * gcy, n_sub), dtype=np.int64)
    np.add.at(E, of_cell, d_min)
    assert E.max() <= 256 * 765
    key = (E << 8) | np.arange(n_sub, dtype=np.int64)[None, :]
    chosen = np.argmin(key, axis=1)
    s = chosen[of_cell]
    index = s * sub_size + k_min[i, s]
    assert index.max() < 256
    out = fb.copy()
    for c in Q.CHANNELS:
        out[c] = palette[c][index]
    out["alpha"] = fb["alpha"]  # the pixel's own alpha passes through
    return index.astype(np.uint8), out, chosen.astype(np.uint8)


def model_loop(params, palette, n_sub, sub_size, cell, fb, rows, spread):
    """`model`, one cell, one sub-palette, one pixel and one entry at a time in Python integers."""
    r0, r1 = rows or (0, params.height)
    W, H, (cw, ch) = params.width, params.height, cell
    assert r0 % ch == 0 and (r1 % ch == 0 or r1 == H)
    gcx = (W + cw - 1) // cw
    pal = [[int(palette[c][e]) for c in Q.CHANNELS] for e in range(n_sub * sub_size)]
    index = np.zeros(len(fb), dtype=np.uint8)
    out = fb.copy()
    plane = []
    for cy in range(r0 // ch, (r1 + ch - 1) // ch):
        for cx in range(gcx):
            pixels = []  # (position in the block, dithered channels)
            for y in range(cy * ch, min((cy + 1) * ch, H)):
                for x in range(cx * cw, min((cx + 1) * cw, W)):
                    at = (y - r0) * W + x
                    off = ((2 * Q.BAYER4[y & 3][x & 3] - 15) * spread) // 32  # Python's // floors
                    pixels.append((at, [min(255, max(0, int(fb[c][at]) + off)) for c in Q.CHANNELS]))
            assert pixels and all(0 <= at < len(fb) for at, _ in pixels)
            best = None
            for s in range(n_sub):
                E, ks = 0, []
                for _, c in pixels:
                    d_best, k_best = None, None
                    for k in range(sub_size):
                        d = sum(abs(c[j] - pal[s * sub_size + k][j]) for j in range(3))
                        if d_best is None or d < d_best:
                            d_best, k_best = d, k
                    E += d_best
                    ks.append(k_best)
                if best is None or E < best[0]:
                    best = (E, s, ks)
            _, s, ks = best
            plane.append(s)
            for (at, _), k in zip(pixels, ks):
                index[at] = s * sub_size + k
                for j, c in enumerate(Q.CHANNELS):
                    out[c][at] = pal[s * sub_size + k][j]
    return index, out, np.array(plane, dtype=np.uint8)


def pairs(palette):
    """par_cells_pairs: the flat table of every unordered pair (i, j), i < j, in ascending order."""
    order = [e for pair in itertools.combinations(range(len(palette)), 2) for e in pair]
    return palette[np.array(order, dtype=np.int64)]


def near_sub_palettes(T, rng, params, palette, n_sub, sub_size, cell, noise):
    """A whole frame whose every cell is drawn from one randomly chosen sub-palette's entries plus noise in
    [-noise, noise] a channel; returns (fb, the sub-palette drawn for every cell)."""
    W, H = params.width, params.height
    gcx, gcy = grid(params, cell, None)
    drawn = rng.integers(0, n_sub, gcx * gcy)
    i = np.arange(W * H)
    of_cell = (i % W) // cell[0] + ((i // W) // cell[1]) * gcx
    entry = drawn[of_cell] * sub_size + rng.integers(0, sub_size, W * H)
    fb = np.zeros(W * H, dtype=T.COLOR)
    for c in Q.CHANNELS:
        fb[c] = np.clip(palette[c][entry].astype(np.int32) + rng.integers(-noise, noise + 1, W * H), 0, 255)
    fb["alpha"] = rng.integers(0, 256, W * H)
    return fb, drawn.astype(np.uint8)
