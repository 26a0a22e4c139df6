"""The tile-set contract of include/par_tileset.h restated in numpy: what the GPU tests compare with byte for byte.
model() is vectorised (the canonical forms, then np.unique put into first-appearance order), model_loop() says the same as
a per-cell loop with a dict from bytes to number and the four flips made by slicing, and expand_model() draws a map.
A plane is a flat uint8 array of rows * w bytes; `rows` is the number of rows it holds (a row block's cells start at
its first row, which the contract's cut rule puts on a cell row)."""
import numpy as np

TILES = ((8, 8), (8, 16), (16, 8), (16, 16))
ID_MASK = 0x3FFFFFFF
MAX_CELLS = 1 << 20


def grid(w, rows, tile):
    return -(-w // tile[0]), -(-rows // tile[1])


def admits(row_begin, row_end, height, tile):
    """The contract's rule for a row cut."""
    return row_begin % tile[1] == 0 and (row_end % tile[1] == 0 or row_end == height)


def cells_of(plane, w, rows, tile, pad):
    """(N, th, tw): the call's cells in their numbering, pixels beyond the plane `pad`."""
    tw, th = tile
    gcx, gcy = grid(w, rows, tile)
    full = np.full((gcy * th, gcx * tw), pad, dtype=np.uint8)
    full[:rows, :w] = np.asarray(plane, dtype=np.uint8).reshape(rows, w)
    return np.ascontiguousarray(full.reshape(gcy, th, gcx, tw).transpose(0, 2, 1, 3)).reshape(gcy * gcx, th, tw)


def flipped(cells, f):
    """The images of (N, th, tw) cells under the flip code f: bit 0 mirrors x, bit 1 mirrors y."""
    return cells[:, ::-1 if f & 2 else 1, ::-1 if f & 1 else 1]


def canonical(cells, flips):
    """(the canonical forms (N, th, tw), f* (N,)): the smallest image as a row-major string of unsigned bytes among the
    allowed codes, the lowest code among equals."""
    n = len(cells)
    best, code = cells.copy(), np.zeros(n, dtype=np.uint32)
    at = np.arange(n)
    for f in (1, 2, 3):
        if f & ~flips:
            continue
        image = np.ascontiguousarray(flipped(cells, f))
        a, b = image.reshape(n, -1), best.reshape(n, -1)
        differs = a != b
        first = differs.argmax(axis=1)
        less = differs.any(axis=1) & (a[at, first] < b[at, first])
        best[less] = image[less]
        code[less] = f
    return best, code


def model(plane, w, rows, tile, pad=0, flips=0, capacity=None):
    """(tiles (min(T, capacity), th, tw) uint8, map (N,) uint32, T)."""
    forms, code = canonical(cells_of(plane, w, rows, tile, pad), flips)
    n = len(forms)
    keys = np.ascontiguousarray(forms.reshape(n, -1)).view(np.dtype((np.void, tile[0] * tile[1]))).reshape(n)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")  # the classes by their lowest cell number
    rank = np.empty(len(first), dtype=np.uint32)
    rank[order] = np.arange(len(first), dtype=np.uint32)
    ids = rank[inverse.reshape(n)]
    count = len(first)
    kept = count if capacity is None else min(count, capacity)
    return forms[np.sort(first)[:kept]].copy(), (ids | (code << 30)).astype(np.uint32), count


def model_loop(plane, w, rows, tile, pad=0, flips=0, capacity=None):
    """The same, slowly: a loop over the cells with a dict from bytes to number."""
    tw, th = tile
    gcx, gcy = grid(w, rows, tile)
    img = np.asarray(plane, dtype=np.uint8).reshape(rows, w)
    numbers, tiles, entries = {}, [], []
    for cy in range(gcy):
        for cx in range(gcx):
            cell = np.full((th, tw), pad, dtype=np.uint8)
            part = img[cy * th:(cy + 1) * th, cx * tw:(cx + 1) * tw]
            cell[:part.shape[0], :part.shape[1]] = part
            images = {0: cell, 1: cell[:, ::-1], 2: cell[::-1, :], 3: cell[::-1, ::-1]}
            best, code = None, 0
            for f in range(4):
                if f & ~flips:
                    continue
                s = images[f].tobytes()  # (bytes compare as strings of unsigned bytes)
                if best is None or s < best:
                    best, code = s, f
            if best not in numbers:
                numbers[best] = len(tiles)
                tiles.append(best)
            entries.append(numbers[best] | (code << 30))
    kept = len(tiles) if capacity is None else min(len(tiles), capacity)
    out = np.frombuffer(b"".join(tiles[:kept]), dtype=np.uint8).reshape(kept, th, tw)
    return out, np.array(entries, dtype=np.uint32), len(tiles)


def expand_model(tiles, tile, tile_map, w, rows, before=None):
    """The plane (rows * w,) a map draws: every pixel of the frame takes its byte of tile min(id, n_tiles - 1) under the
    entry's flips. `before` is what the plane held (nothing outside the frame exists in it, so it comes back covered)."""
    tw, th = tile
    gcx, gcy = grid(w, rows, tile)
    tiles = np.asarray(tiles, dtype=np.uint8).reshape(-1, th, tw)
    tile_map = np.asarray(tile_map, dtype=np.uint32)
    assert len(tile_map) == gcx * gcy and len(tiles) >= 1
    ids = np.minimum(tile_map & ID_MASK, len(tiles) - 1)
    drawn = np.empty((len(tile_map), th, tw), dtype=np.uint8)
    for f in range(4):
        sel = (tile_map >> 30) == f
        drawn[sel] = flipped(tiles[ids[sel]], f)
    full = drawn.reshape(gcy, gcx, th, tw).transpose(0, 2, 1, 3).reshape(gcy * th, gcx * tw)
    return np.ascontiguousarray(full[:rows, :w]).reshape(-1)


# ---- planes the tests share ------------------------------------------------------------------------------------------

def distinct_plane(w, rows, tile):
    """A plane whose cell c holds c in its first three bytes (little-endian) and 0 elsewhere: all cells differ, and no
    flip makes two of them equal where a cell's own number is not a palindrome of another's. w and rows are whole cells."""
    tw, th = tile
    gcx, gcy = grid(w, rows, tile)
    assert w == gcx * tw and rows == gcy * th
    img = np.zeros((rows, w), dtype=np.uint8)
    c = np.arange(gcx * gcy, dtype=np.uint32).reshape(gcy, gcx)
    for k in range(3):
        img[0::th, k::tw] = (c >> (8 * k)) & 0xFF
    return img.reshape(-1)


def mixed_plane(rng, w, rows, tile, n_kinds, colours=4):
    """A plane of cells drawn at random from n_kinds random tiles under random mirrors; ragged edges are cut off."""
    tw, th = tile
    gcx, gcy = grid(w, rows, tile)
    kinds = rng.integers(0, colours, (n_kinds, th, tw), dtype=np.uint8)
    pick = rng.integers(0, n_kinds, gcx * gcy)
    flip = rng.integers(0, 4, gcx * gcy)
    cells = kinds[pick]
    for f in range(1, 4):
        cells[flip == f] = flipped(kinds[pick[flip == f]], f)
    full = cells.reshape(gcy, gcx, th, tw).transpose(0, 2, 1, 3).reshape(gcy * th, gcx * tw)
    return np.ascontiguousarray(full[:rows, :w]).reshape(-1)
