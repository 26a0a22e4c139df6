"""The shared-tile-set contract of include/par_tileset_extend.h restated in numpy, on tests/tileset.py's cells_of and
canonical: what the GPU tests compare with byte for byte. model() is vectorised (the stored tiles and the call's
canonical forms in one np.unique, whose first index is a class's lowest virtual position), model_loop() says the same
with one dict seeded with the stored tiles in ascending order (setdefault: the lowest duplicate wins) and a per-cell
loop, and sequence_model() threads a set through several calls. A set is (stored, t_in): `stored` holds the
min(t_in, capacity) stored tiles as (S, th, tw) uint8."""
import numpy as np

import tileset as TS

ID_MASK = TS.ID_MASK


def no_tiles(tile):
    return np.zeros((0, tile[1], tile[0]), dtype=np.uint8)


def _keys(forms, tile):
    n = len(forms)
    return np.ascontiguousarray(forms.reshape(n, tile[0] * tile[1])).view(np.dtype((np.void, tile[0] * tile[1]))).reshape(n)


def model(stored, t_in, plane, w, rows, tile, pad=0, flips=0, capacity=0):
    """(tiles after (min(T_out, capacity), th, tw) uint8, map (N,) uint32, T_out, first_new)."""
    stored = np.asarray(stored, dtype=np.uint8).reshape(-1, tile[1], tile[0])
    s = len(stored)
    assert s == min(t_in, capacity)
    forms, code = canonical(plane, w, rows, tile, pad, flips)
    n = len(forms)
    _, first, inverse = np.unique(np.concatenate([_keys(stored, tile), _keys(forms, tile)]), return_index=True, return_inverse=True)
    owner = first[inverse.reshape(-1)[s:]]  # a cell: the lowest virtual position of its class, stored tiles before cells
    new_firsts = np.sort(first[first >= s])  # the new classes by their lowest cell
    ids = np.where(owner < s, owner, t_in + np.searchsorted(new_firsts, owner)).astype(np.uint64)
    t_out = t_in + len(new_firsts)
    room = max(0, min(t_out, capacity) - s) if t_in <= capacity else 0
    after = np.concatenate([stored, forms[new_firsts[:room] - s]]) if room else stored.copy()
    assert len(after) == min(t_out, capacity)
    return after, ((ids & ID_MASK).astype(np.uint32) | (code << 30)).astype(np.uint32), t_out, t_in


def canonical(plane, w, rows, tile, pad, flips):
    return TS.canonical(TS.cells_of(plane, w, rows, tile, pad), flips)


def model_loop(stored, t_in, plane, w, rows, tile, pad=0, flips=0, capacity=0):
    """The same, slowly: one dict from bytes to number, seeded with the stored tiles, and a loop over the cells."""
    tw, th = tile
    stored = np.asarray(stored, dtype=np.uint8).reshape(-1, th, tw)
    assert len(stored) == min(t_in, capacity)
    numbers = {}
    for i, t in enumerate(stored):
        numbers.setdefault(t.tobytes(), i)
    cells = TS.cells_of(plane, w, rows, tile, pad)
    added, entries = [], []
    for cell in cells:
        images = {0: cell, 1: cell[:, ::-1], 2: cell[::-1, :], 3: cell[::-1, ::-1]}
        best, code = None, 0
        for f in range(4):
            if f & ~flips:
                continue
            s = images[f].tobytes()
            if best is None or s < best:
                best, code = s, f
        if best not in numbers:
            numbers[best] = t_in + len(added)
            added.append(best)
        entries.append((numbers[best] & ID_MASK) | (code << 30))
    t_out = t_in + len(added)
    kept = [a for k, a in enumerate(added) if t_in + k < capacity]
    after = np.concatenate([stored, np.frombuffer(b"".join(kept), dtype=np.uint8).reshape(len(kept), th, tw)])
    return after, np.array(entries, dtype=np.uint32), t_out, t_in


def sequence_model(planes, w, rows, tile, pad=0, flips=0, capacity=0, stored=None, t_in=0, fn=model):
    """The calls one after another on one set: `planes` are flat planes, `rows` the rows each holds (one int for all or
    a list). Returns (the list of each call's (tiles after, map, T_out, first_new), the final (stored, count))."""
    stored = no_tiles(tile) if stored is None else stored
    rows = [rows] * len(planes) if isinstance(rows, int) else rows
    out = []
    for plane, r in zip(planes, rows):
        got = fn(stored, t_in, plane, w, r, tile, pad, flips, capacity)
        out.append(got)
        stored, t_in = got[0], got[2]
    return out, (stored, t_in)


def frame_sequence(seed, n_frames, w, rows, tile, kinds=5, step=3, colours=2):
    """Frames whose later ones both reuse earlier tiles and add new ones: frame k is TS.mixed_plane from the SAME seed
    with kinds + k * step kinds, so its kinds begin with those of the frames before it (the generator fills the kinds in
    order) and end with new ones, and its picks and mirrors differ."""
    return [TS.mixed_plane(np.random.default_rng(seed), w, rows, tile, kinds + k * step, colours) for k in range(n_frames)]
