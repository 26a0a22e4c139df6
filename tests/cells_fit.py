"""Fitted cells (par_cells_fit_device, par_cells_fit_host, the add-on of addons/include/par_cells_fit.h) restated on the
host: the contract beside the declarations in vectorised numpy (`model`), and a second time with the seed one cell, one
pixel and one entry at a time in plain Python integers (`model_loop`, which tests/test_cells_fit_cpu.py holds `model`
to). In both the assign step of a round is tests/cells.py's (its `model` and its `model_loop`) and the medians are
palette_refine.update's. A frame and a palette are flat COLOR arrays; a result is (table as a COLOR array of S * K
entries, seeds as uint32, errors as uint64 of R + 1)."""
import types

import numpy as np

import cells as CL
import palette_refine as PR
import quantize as Q

MAX_CELLS, MAX_SUB_SIZE, MAX_ROUNDS = 1 << 20, 16, 32
HEAD_BYTES, BYTES_PER_CELL = 59392, 25
NO_SEED = 0xFFFFFFFF
CHUNK = 1 << 14


def frame_params(width, height):
    """What tests/cells.py and tests/quantize.py read of a par_params."""
    return types.SimpleNamespace(width=width, height=height)


def n_cells(width, height, cell):
    return -(-width // cell[0]) * -(-height // cell[1])


def work_bytes(width, height, cell):
    """The header's formula, 0 outside the limits."""
    if width < 1 or height < 1 or cell[0] not in (8, 16) or cell[1] not in (8, 16) or n_cells(width, height, cell) > MAX_CELLS:
        return 0
    return HEAD_BYTES + BYTES_PER_CELL * n_cells(width, height, cell)


def launches(n_sub, rounds, with_errors=True):
    return 4 + n_sub + 4 * rounds + (1 if with_errors else 0)


def rgb_of(a):
    return np.stack([a[c].astype(np.int32) for c in Q.CHANNELS], axis=1)


def cell_numbers(width, height, cell):
    i = np.arange(width * height, dtype=np.int64)
    return (i % width) // cell[0] + ((i // width) // cell[1]) * -(-width // cell[0])


def l1_difference(a, b):
    return int(np.abs(rgb_of(a).astype(np.int64) - rgb_of(b)).sum())


def seed(fb, width, height, cell, palette, n_sub, sub_size):
    """(lists A_0 .. A_(S-1) as an (S, K) array of master indices, seeds, W as (cells, K), own, best_S)."""
    K, N, cells = sub_size, len(palette), n_cells(width, height, cell)
    assert 1 <= K <= min(N, MAX_SUB_SIZE) and N <= 256 and n_sub >= 1 and n_sub * K <= 256 and len(fb) == width * height
    px, pal, of_cell = rgb_of(fb), rgb_of(palette), cell_numbers(width, height, cell)
    m = np.zeros(len(px), dtype=np.int64)
    for a in range(0, len(px), CHUNK):
        d = np.abs(px[a:a + CHUNK, None, :] - pal[None, :, :]).sum(axis=2)
        m[a:a + CHUNK] = np.argmin(d, axis=1)  # the first minimum: the lowest index among equals
    h = np.zeros((cells, N), dtype=np.int64)
    np.add.at(h, (of_cell, m), 1)
    H = h.sum(axis=0)
    W = np.argsort(-h, axis=1, kind="stable")[:, :K]  # stable: equal counts in ascending order of j
    A0 = np.argsort(-H, kind="stable")[:K]

    def e_under(lists):
        """e(c, lists[c]) for an (cells, K) array, or e(c, A) for one list."""
        total = np.zeros(cells, dtype=np.int64)
        for a in range(0, len(px), CHUNK):
            part, cs = px[a:a + CHUNK], of_cell[a:a + CHUNK]
            entries = pal[lists[cs]] if lists.ndim == 2 else pal[lists][None, :, :]
            d = np.abs(part[:, None, :] - entries).sum(axis=2).min(axis=1)
            np.add.at(total, cs, d)
        assert total.max() <= 256 * 765
        return total

    own, best = e_under(W), e_under(A0)
    lists, seeds = [A0], [NO_SEED]
    for _ in range(1, n_sub):
        c = int(np.argmax(best - own))  # the first maximum: the lowest c among equals
        lists.append(W[c])
        seeds.append(c)
        best = np.minimum(best, e_under(W[c]))
    return np.array(lists, dtype=np.int64), np.array(seeds, dtype=np.uint32), W, own, best


def rounds_of(assign, fb, width, height, cell, table, n_sub, sub_size, rounds):
    """(table after the rounds, errors): `assign` is cells.model or cells.model_loop."""
    params = frame_params(width, height)
    errors = []
    for _ in range(rounds):
        index, out, _ = assign(params, table, n_sub, sub_size, cell, fb, None, 0)
        errors.append(l1_difference(fb, out))
        table, _ = PR.update(table, fb, index)
    _, out, _ = assign(params, table, n_sub, sub_size, cell, fb, None, 0)
    errors.append(l1_difference(fb, out))
    return table, np.array(errors, dtype=np.uint64)


def model(fb, width, height, cell, palette, n_sub, sub_size, rounds):
    lists, seeds, _, _, _ = seed(fb, width, height, cell, palette, n_sub, sub_size)
    table, errors = rounds_of(CL.model, fb, width, height, cell, palette[lists.reshape(-1)].copy(), n_sub, sub_size, rounds)
    return table, seeds, errors


def seed_loop(fb, width, height, cell, palette, n_sub, sub_size):
    """`seed`'s lists and seeds, in Python integers."""
    K, N, (cw, ch) = sub_size, len(palette), cell
    gcx, gcy = -(-width // cw), -(-height // ch)
    pal = [[int(palette[c][e]) for c in Q.CHANNELS] for e in range(N)]

    def dist(p, j):
        return sum(abs(p[i] - pal[j][i]) for i in range(3))

    def e_of(pixels, A):
        return sum(min(dist(p, j) for j in A) for p in pixels)

    def first_k(counts):
        return sorted(range(N), key=lambda j: (-counts[j], j))[:K]

    H, cells_px, W = [0] * N, [], []
    for cy in range(gcy):
        for cx in range(gcx):
            pixels, h = [], [0] * N
            for y in range(cy * ch, min((cy + 1) * ch, height)):
                for x in range(cx * cw, min((cx + 1) * cw, width)):
                    p = [int(fb[c][y * width + x]) for c in Q.CHANNELS]
                    best = None
                    for j in range(N):
                        d = dist(p, j)
                        if best is None or d < best[0]:
                            best = (d, j)
                    h[best[1]] += 1
                    pixels.append(p)
            for j in range(N):
                H[j] += h[j]
            cells_px.append(pixels)
            W.append(first_k(h))
    own = [e_of(px, W[c]) for c, px in enumerate(cells_px)]
    lists, seeds = [first_k(H)], [NO_SEED]
    best = [e_of(px, lists[0]) for px in cells_px]
    for _ in range(1, n_sub):
        pick = None
        for c in range(len(cells_px)):
            if pick is None or best[c] - own[c] > best[pick] - own[pick]:
                pick = c
        lists.append(W[pick])
        seeds.append(pick)
        best = [min(b, e_of(px, W[pick])) for b, px in zip(best, cells_px)]
    return np.array(lists, dtype=np.int64), np.array(seeds, dtype=np.uint32)


def model_loop(fb, width, height, cell, palette, n_sub, sub_size, rounds):
    lists, seeds = seed_loop(fb, width, height, cell, palette, n_sub, sub_size)
    table, errors = rounds_of(CL.model_loop, fb, width, height, cell, palette[lists.reshape(-1)].copy(), n_sub, sub_size, rounds)
    return table, seeds, errors


def same(got, exp, tag):
    for name, g, e in zip(("table", "seeds", "errors"), got, exp):
        g, e = np.ascontiguousarray(g), np.ascontiguousarray(e)
        assert g.tobytes() == e.tobytes(), f"{tag}: {name}: {g.reshape(-1)[:12]} for {e.reshape(-1)[:12]}"


def random_frame(T, rng, width, height, colours=None, noise=0):
    """A frame of random pixels, or of pixels drawn from the COLOR array `colours` plus noise in [-noise, noise]."""
    n = width * height
    fb = np.zeros(n, dtype=T.COLOR)
    pick = rng.integers(0, len(colours), n) if colours is not None else None
    for c in Q.CHANNELS:
        base = colours[c][pick].astype(np.int32) if colours is not None else rng.integers(0, 256, n)
        fb[c] = np.clip(base + (rng.integers(-noise, noise + 1, n) if noise else 0), 0, 255)
    fb["alpha"] = rng.integers(0, 256, n)
    return fb


def colours(T, rows):
    a = np.zeros(len(rows), dtype=T.COLOR)
    for i, row in enumerate(rows):
        a[i] = tuple(row) if len(row) == 4 else (*row, 255)
    return a


def painted(T, width, height, cell, cell_colours, alpha=7):
    """A frame whose cell c shows the colours cell_colours[c] (a list of (r, g, b)), pixel i of the cell (in row order
    within the cell) the colour i % len."""
    fb = np.zeros(width * height, dtype=T.COLOR)
    gcx = -(-width // cell[0])
    seen = {}
    for y in range(height):
        for x in range(width):
            c = x // cell[0] + (y // cell[1]) * gcx
            i = seen.get(c, 0)
            seen[c] = i + 1
            fb[y * width + x] = (*cell_colours[c][i % len(cell_colours[c])], alpha)
    return fb


def chop(palette, n_sub, sub_size, by_luma=False):
    """The baselines: a flat palette of S * K entries cut into S consecutive groups of K, as it comes or after a stable
    sort by luma (299 red + 587 green + 114 blue)."""
    assert len(palette) == n_sub * sub_size
    if not by_luma:
        return palette.copy()
    luma = 299 * palette["red"].astype(np.int64) + 587 * palette["green"].astype(np.int64) + 114 * palette["blue"].astype(np.int64)
    return palette[np.argsort(luma, kind="stable")].copy()
