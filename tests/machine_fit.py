"""Machine fit (par_machine_round, par_machine_fit_device, par_machine_fit_host, the add-on of
addons/include/par_machine_fit.h) restated on the host, twice: vectorised numpy (`round_palette`, `move`, `model`: what the
GPU tests compare with byte for byte) and as loops in Python integers (`round_loop` over all 256 values of a depth,
`move_loop` by brute force over every level, `seed_loop` with the backdrop, `model_loop`), which
tests/test_machine_fit_cpu.py holds the vectorised forms to. The plain seed is tests/cells_fit.py's, the assign step of a
round tests/cells.py's, the colour words tests/vram.py's and the screen tests/screen.py's; none is restated here. A frame
and a palette are flat COLOR arrays; a result is (table as a COLOR array of S * K entries, seeds as uint32, errors as
uint64 of R + 1)."""
import numpy as np

import cells as CL
import cells_fit as CF
import quantize as Q
import screen as SC
import vram as V

BGR555, BGR333_MD, BGR222, RGBA8 = DEPTHS = range(4)
BITS = (5, 3, 2, 8)
EXTRA_BYTES = 120832  # in front of the plain fit's block
HEAD_BYTES, BYTES_PER_CELL = EXTRA_BYTES + CF.HEAD_BYTES, CF.BYTES_PER_CELL
assert (BGR555, BGR333_MD, BGR222, RGBA8) == (SC.BGR555, SC.BGR333_MD, SC.BGR222, SC.RGBA8)


def work_bytes(width, height, cell):
    """The header's formula, 0 outside the limits."""
    plain = CF.work_bytes(width, height, cell)
    return plain + EXTRA_BYTES if plain else 0


def launches(n_sub, rounds, backdrop, with_errors=True):
    return 5 + n_sub + 4 * rounds + (1 if backdrop else 0) + (1 if with_errors else 0)


def widen(depth, level):
    return level if depth == RGBA8 else SC.widen(level, BITS[depth])


def lattice(depth):
    """w(l) of every level, ascending."""
    return np.array([widen(depth, l) for l in range(1 << BITS[depth])], dtype=np.int64)


def round_values(depth):
    """The rounding of every byte: the nearest w(l), the lowest l among equals (argmin takes the first minimum)."""
    w = lattice(depth)
    return w[np.argmin(np.abs(np.arange(256)[:, None] - w[None, :]), axis=1)].astype(np.uint8)


def round_palette(palette, depth):
    out = palette.copy()
    table = round_values(depth)
    for ch in Q.CHANNELS:
        out[ch] = table[palette[ch]]
    return out


def round_loop(depth):
    """round_values, one value and one level at a time."""
    out = []
    for x in range(256):
        best = None
        for l in range(1 << BITS[depth]):
            if depth == BGR555:
                w = l * 8 + l // 4
            elif depth == BGR333_MD:
                w = l * 32 + l * 4 + l // 2
            elif depth == BGR222:
                w = l * 85
            else:
                w = l
            if best is None or abs(x - w) < best[0]:
                best = (abs(x - w), w)
        out.append(best[1])
    return out


def move(hist, depth):
    """The lattice value that minimises the sum of |x - w(l)| over a channel's pixels, given as a histogram of 256 counts:
    the lowest l among equals."""
    w = lattice(depth)
    cost = np.asarray(hist, dtype=np.int64) @ np.abs(np.arange(256, dtype=np.int64)[:, None] - w[None, :])
    return int(w[int(np.argmin(cost))])


def move_loop(values, depth):
    """The same by brute force over every level, on a list of pixel values."""
    best = None
    for l in range(1 << BITS[depth]):
        w = widen(depth, l)
        cost = sum(abs(int(x) - w) for x in values)
        if best is None or cost < best[0]:
            best = (cost, w)
    return best[1]


def move_two_candidates(values, depth):
    """The device's way, in Python integers: the lattice interval [a, b) of the lower median, the counts either side, the
    count of x == a and the sum of x - a inside, and the sign of g(b) - g(a)."""
    values = sorted(int(x) for x in values)
    n, levels = len(values), [widen(depth, l) for l in range(1 << BITS[depth])]
    median = values[(n - 1) // 2]
    l = max(i for i, w in enumerate(levels) if w <= median)
    a = levels[l]
    if l + 1 == len(levels):
        return a
    b = levels[l + 1]
    below, above = sum(1 for x in values if x < a), sum(1 for x in values if x >= b)
    eq, mid = sum(1 for x in values if x == a), [x for x in values if a < x < b]
    difference = (b - a) * (below + eq - above) + len(mid) * (b - a) - 2 * sum(x - a for x in mid)
    return b if difference < 0 else a


def with_backdrop(order, b0, K):
    """b0 followed by the first K - 1 indices other than b0 of `order`."""
    return [b0] + [int(j) for j in order if j != b0][:K - 1]


def e_under(px, pal, of_cell, cells, lists):
    total = np.zeros(cells, dtype=np.int64)
    for a in range(0, len(px), CF.CHUNK):
        part, cs = px[a:a + CF.CHUNK], of_cell[a:a + CF.CHUNK]
        entries = pal[lists[cs]] if lists.ndim == 2 else pal[lists][None, :, :]
        np.add.at(total, cs, np.abs(part[:, None, :] - entries).sum(axis=2).min(axis=1))
    return total


def seed(fb, width, height, cell, rounded, n_sub, sub_size, backdrop):
    """(lists as an (S, K) array of master indices, seeds) over the ROUNDED master. The plain lists hold K indices, so b0
    and the first K - 1 others of the usual order are b0 and the first K - 1 others of the plain list."""
    lists, seeds, W, _, _ = CF.seed(fb, width, height, cell, rounded, n_sub, sub_size)
    if not backdrop:
        return lists, seeds
    K, cells = sub_size, CF.n_cells(width, height, cell)
    assert K >= 2
    b0 = int(lists[0][0])
    W = np.array([with_backdrop(row, b0, K) for row in W], dtype=np.int64)
    A0 = np.array(with_backdrop(lists[0], b0, K), dtype=np.int64)
    assert A0.tolist() == lists[0].tolist()
    px, pal, of_cell = CF.rgb_of(fb), CF.rgb_of(rounded), CF.cell_numbers(width, height, cell)
    own, best = e_under(px, pal, of_cell, cells, W), e_under(px, pal, of_cell, cells, A0)
    lists, seeds = [A0], [CF.NO_SEED]
    for _ in range(1, n_sub):
        c = int(np.argmax(best - own))
        lists.append(W[c])
        seeds.append(c)
        best = np.minimum(best, e_under(px, pal, of_cell, cells, W[c]))
    return np.array(lists, dtype=np.int64), np.array(seeds, dtype=np.uint32)


def update(table, fb, index, sub_size, depth, backdrop, mover=None):
    """The move of a round: `index` is the assign step's plane of s * K + k."""
    out = table.copy()
    index = np.asarray(index, dtype=np.int64)
    if backdrop:
        index = np.where(index % sub_size == 0, 0, index)
    for k in np.unique(index):
        mine = fb[index == k]
        at = np.arange(0, len(table), sub_size) if backdrop and k == 0 else k
        for ch in Q.CHANNELS:
            out[ch][at] = move(np.bincount(mine[ch], minlength=256), depth) if mover is None else mover(mine[ch].tolist(), depth)
        out["alpha"][at] = 255
    return out


def rounds_of(assign, fb, width, height, cell, table, n_sub, sub_size, rounds, depth, backdrop, mover=None):
    params = CF.frame_params(width, height)
    errors = []
    for _ in range(rounds):
        index, out, _ = assign(params, table, n_sub, sub_size, cell, fb, None, 0)
        errors.append(CF.l1_difference(fb, out))
        table = update(table, fb, index, sub_size, depth, backdrop, mover)
    _, out, _ = assign(params, table, n_sub, sub_size, cell, fb, None, 0)
    errors.append(CF.l1_difference(fb, out))
    return table, np.array(errors, dtype=np.uint64)


def model(fb, width, height, cell, palette, n_sub, sub_size, rounds, depth, backdrop):
    rounded = round_palette(palette, depth)
    lists, seeds = seed(fb, width, height, cell, rounded, n_sub, sub_size, backdrop)
    table, errors = rounds_of(CL.model, fb, width, height, cell, rounded[lists.reshape(-1)].copy(), n_sub, sub_size, rounds, depth, backdrop)
    return table, seeds, errors


def seed_loop(fb, width, height, cell, rounded, n_sub, sub_size, backdrop):
    """`seed`, in Python integers, from the pixels up."""
    K, N, (cw, ch) = sub_size, len(rounded), cell
    gcx, gcy = -(-width // cw), -(-height // ch)
    pal = [[int(rounded[c][e]) for c in Q.CHANNELS] for e in range(N)]

    def dist(p, j):
        return sum(abs(p[i] - pal[j][i]) for i in range(3))

    def e_of(pixels, A):
        return sum(min(dist(p, j) for j in A) for p in pixels)

    H, cells_px, counts = [0] * N, [], []
    for cy in range(gcy):
        for cx in range(gcx):
            pixels, h = [], [0] * N
            for y in range(cy * ch, min((cy + 1) * ch, height)):
                for x in range(cx * cw, min((cx + 1) * cw, width)):
                    p = [int(fb[c][y * width + x]) for c in Q.CHANNELS]
                    h[min(range(N), key=lambda j: (dist(p, j), j))] += 1
                    pixels.append(p)
            for j in range(N):
                H[j] += h[j]
            cells_px.append(pixels)
            counts.append(h)
    order_H = sorted(range(N), key=lambda j: (-H[j], j))
    b0 = order_H[0]

    def first_k(count):
        order = sorted(range(N), key=lambda j: (-count[j], j))
        if not backdrop:
            return order[:K]
        return [b0] + [j for j in order if j != b0][:K - 1]

    W = [first_k(h) for h in counts]
    own = [e_of(px, W[c]) for c, px in enumerate(cells_px)]
    lists, seeds = [first_k(H)], [CF.NO_SEED]
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


def model_loop(fb, width, height, cell, palette, n_sub, sub_size, rounds, depth, backdrop):
    values = round_loop(depth)
    rounded = palette.copy()
    for ch in Q.CHANNELS:
        rounded[ch] = [values[int(x)] for x in palette[ch]]
    lists, seeds = seed_loop(fb, width, height, cell, rounded, n_sub, sub_size, backdrop)
    table, errors = rounds_of(CL.model_loop, fb, width, height, cell, rounded[lists.reshape(-1)].copy(), n_sub, sub_size, rounds, depth,
                              backdrop, mover=move_loop)
    return table, seeds, errors


def on_lattice(table, depth):
    allowed = set(lattice(depth).tolist())
    return all(int(v) in allowed for ch in Q.CHANNELS for v in table[ch])


WIDE = dict(word_bytes=4, big_endian=0, tile_shift=0, tile_bits=20, pal_shift=20, pal_bits=8, flip_x_bit=28, flip_y_bit=29,
            tile_step=1, tile_base=0, set_bits=0)  # a map word that names any tile and any sub-palette


def shown(TS, fb, width, height, cell, table, n_sub, sub_size, fmt, screen_backdrop, L=None, tile_format=V.F_4BPP_ROWS, flips=3):
    """The picture a machine shows of `fb` under `table`: cells, the chain of tests/screen.py's export() under 8 x 8 tiles
    of layout L, the table as colour words of `fmt`, drawn with the screen's backdrop rule. Returns (the shown frame as a
    COLOR array, the cells frame, the bad cells of the chain and of the draw)."""
    params = CF.frame_params(width, height)
    index, out, chosen = CL.model(params, table, n_sub, sub_size, cell, fb, None, 0)
    exp = SC.export(TS, index, chosen, sub_size, width, height, cell, (8, 8), L or WIDE, tile_format, flips)
    words = V.palette_words(np.ascontiguousarray(table).view(np.uint8).reshape(-1, 4), fmt)
    d = dict(exp["desc"], pal_format=fmt, n_colors=n_sub * sub_size, backdrop=screen_backdrop)
    drawn, _, n_bad = SC.draw(d, exp["chr"], exp["map_bytes"], words)
    got = np.ascontiguousarray(drawn.reshape(-1, 4)).view(fb.dtype).reshape(-1)
    return got, out, n_bad + exp["bad"]
