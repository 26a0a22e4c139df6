"""Refined palettes (par_palette_refine_device, par_palette_refine_host) restated on the host: the contract beside the
declarations in include/par_raytracer.h in numpy. `assign` is quantize.model at spread 0, `update` sorts every entry's
pixels per channel, `refine` runs the rounds; `update_loop` is a second restatement, one pixel at a time in Python
integers through the two-nibble selection, which tests/test_palette_refine_cpu.py holds `update` to."""
import numpy as np

import quantize as Q


def assign(params, palette, fb, rows):
    """k(p): the index plane of par_quantize_device at spread 0."""
    return Q.model(params, palette, fb, rows, 0)[0]


def update(palette, fb, index):
    """(palette after the update, entries of which a byte changed): every entry with pixels moves to the lower median of
    each channel over them, element (n - 1) // 2 of the sorted values, and gets alpha 255; one without keeps its bytes."""
    out = palette.copy()
    for k in np.unique(index):
        mine = fb[index == k]
        at = (len(mine) - 1) // 2
        for ch in Q.CHANNELS:
            out[ch][k] = np.sort(mine[ch])[at]
        out["alpha"][k] = 255
    return out, int((out.view(np.uint32) != palette.view(np.uint32)).sum())


def update_loop(palette, fb, index):
    """`update` through the two-stage selection: 16 tallies of the high nibble per (entry, channel), the nibble the rank
    falls into, 16 tallies of the low nibble among the values with that high nibble, and the rank within."""
    n_colors = len(palette)
    hi = [[[0] * 16 for _ in range(3)] for _ in range(n_colors)]
    px = [(int(k), (int(p["red"]), int(p["green"]), int(p["blue"]))) for k, p in zip(index, fb)]
    for k, v in px:
        for c in range(3):
            hi[k][c][v[c] >> 4] += 1
    picked = [[None] * 3 for _ in range(n_colors)]
    for k in range(n_colors):
        for c in range(3):
            n = sum(hi[k][c])
            if n == 0:
                continue
            rank, cum = (n - 1) // 2, 0
            for nib in range(16):
                if cum + hi[k][c][nib] > rank:
                    picked[k][c] = (nib, rank - cum)
                    break
                cum += hi[k][c][nib]
    lo = [[[0] * 16 for _ in range(3)] for _ in range(n_colors)]
    for k, v in px:
        for c in range(3):
            if v[c] >> 4 == picked[k][c][0]:
                lo[k][c][v[c] & 15] += 1
    out = palette.copy()
    for k in range(n_colors):
        if picked[k][0] is None:
            continue
        value = []
        for c in range(3):
            nib, rank = picked[k][c]
            cum = 0
            for low in range(16):
                if cum + lo[k][c][low] > rank:
                    value.append(nib << 4 | low)
                    break
                cum += lo[k][c][low]
        out[k] = (value[0], value[1], value[2], 255)
    return out, int((out.view(np.uint32) != palette.view(np.uint32)).sum())


def refine(T, params, fb, rows, palette, iterations):
    """(palette, index, changed) after `iterations` rounds: the index plane is the last round's assignment, against the
    palette before the last update, and `changed` the entries the last round changed."""
    palette = np.array(palette, dtype=T.COLOR).reshape(-1)
    index, changed = None, 0
    for _ in range(iterations):
        index = assign(params, palette, fb, rows)
        palette, changed = update(palette, fb, index)
    return palette, index, changed


def error(params, palette, fb, rows=None):
    """(summed, largest) L1 error of the rows quantised to the palette at spread 0."""
    d = Q.distances(params, palette, fb, rows, 0).min(axis=1).astype(np.int64)
    return int(d.sum()), int(d.max())
