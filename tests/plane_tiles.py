"""The contract of the plane-tile calls (par_plane_tiles_* in include/par_raytracer.h) restated in numpy, generic over the
element size E, the shared frames of their tests and the flips that make a plane differ. Planes are uint8 arrays of
rows * W * E bytes; tests/test_plane_tiles_cpu.py holds the models to per-element loops without a GPU.
  changed(params, e, a, b, rows)                     -> (map, tiles, count)
  pack(params, e, tiles, block, rows, guard)         -> the slots' bytes, unwritten bytes equal to the guard
  unpack(params, e, tiles, packed, frame)            -> the whole plane (a copy) with the slots' in-view elements in place
  assemble(params, e, map, packed, fill, frame, rows) -> the whole plane (a copy) with the rows written, tile or fill
  apply(params, e, tiles, packed, rows, frame)       -> the whole plane (a copy) with the slots' in-block elements in place
An entry of a list with bx >= gx or by outside [0, gy) is skipped by pack and unpack (apply refuses it in the library)."""
import numpy as np

import delta as D

SIZES = (1, 4, 28)

# (width, height, bin size): the smallest frames at which each mechanism of the kernels can go wrong
FRAMES = list(D.FRAMES) + [
    (120, 45, 40),  # the default bin: 40-byte tile rows at E = 1 divide by 4 and 8, not by 16; last bin row 5 tall
    (140, 20, 10),  # W % 4 == 0 with B % 4 != 0: at E = 1 a dword straddles two tiles
    (45, 20, 9),    # everything odd: slots start on odd bytes
]

block_rows = D.block_rows
grid = D.grid
tile_rows = D.tile_rows


def both_blocks(h):
    return ((0, h), block_rows(h))


def _rows_of(params, e, plane, n_rows):
    return np.asarray(plane, dtype=np.uint8).reshape(n_rows, params.width, e)


def _listed(params, tiles):
    """(i, bx, by) of the entries that lie in the grid."""
    gx, gy = grid(params)
    for i, t in enumerate(np.asarray(tiles, dtype=np.int32)):
        bx, by = int(t) & 0xFFFF, int(t) >> 16
        if bx < gx and 0 <= by < gy:
            yield i, bx, by


def changed(params, e, a, b, rows):
    w, bs = params.width, params.bin_size
    gx, gy = grid(params)
    r0, r1 = rows
    diff = (_rows_of(params, e, a, r1 - r0) != _rows_of(params, e, b, r1 - r0)).any(axis=2)
    full = np.zeros((gy * bs, gx * bs), dtype=bool)  # the whole grid's elements; outside the block nothing differs
    full[r0:r1, :w] = diff
    flags = full.reshape(gy, bs, gx, bs).any(axis=(1, 3)).reshape(-1)
    where = np.nonzero(flags)[0]
    map_ = np.full(gx * gy, -1, dtype=np.int32)
    map_[where] = np.arange(len(where), dtype=np.int32)
    tiles = ((where % gx) | ((where // gx) << 16)).astype(np.int32)
    return map_, tiles, len(where)


def pack(params, e, tiles, block, rows, guard):
    w, bs = params.width, params.bin_size
    r0, r1 = rows
    src = _rows_of(params, e, block, r1 - r0)
    out = np.full((len(tiles), bs, bs, e), guard, dtype=np.uint8)
    for i, bx, by in _listed(params, tiles):
        lo, hi = tile_rows(params, by, rows)
        c0, c1 = bx * bs, min((bx + 1) * bs, w)
        if lo < hi:
            out[i, lo - by * bs:hi - by * bs, :c1 - c0] = src[lo - r0:hi - r0, c0:c1]
    return out.reshape(-1)


def unpack(params, e, tiles, packed, frame):
    w, h, bs = params.width, params.height, params.bin_size
    out = np.array(frame, dtype=np.uint8).reshape(h, w, e)
    slots = np.asarray(packed, dtype=np.uint8).reshape(-1, bs, bs, e)
    for i, bx, by in _listed(params, tiles):
        lo, hi = tile_rows(params, by, (0, h))
        c0, c1 = bx * bs, min((bx + 1) * bs, w)
        out[lo:hi, c0:c1] = slots[i, lo - by * bs:hi - by * bs, :c1 - c0]
    return out.reshape(-1)


def assemble(params, e, map_, packed, fill, frame, rows):
    w, h, bs = params.width, params.height, params.bin_size
    gx, gy = grid(params)
    out = np.array(frame, dtype=np.uint8).reshape(h, w, e)
    slots = np.asarray(packed, dtype=np.uint8).reshape(-1, bs, bs, e)
    out[rows[0]:rows[1]] = np.frombuffer(bytes(fill), dtype=np.uint8)
    for i, slot in enumerate(np.asarray(map_, dtype=np.int32)):
        bx, by = i % gx, i // gx
        lo, hi = tile_rows(params, by, rows)
        c0, c1 = bx * bs, min((bx + 1) * bs, w)
        if slot >= 0 and lo < hi:
            out[lo:hi, c0:c1] = slots[slot, lo - by * bs:hi - by * bs, :c1 - c0]
    return out.reshape(-1)


def apply(params, e, tiles, packed, rows, frame):
    w, h, bs = params.width, params.height, params.bin_size
    out = np.array(frame, dtype=np.uint8).reshape(h, w, e)
    slots = np.asarray(packed, dtype=np.uint8).reshape(-1, bs, bs, e)
    for i, bx, by in _listed(params, tiles):
        lo, hi = tile_rows(params, by, rows)
        c0, c1 = bx * bs, min((bx + 1) * bs, w)
        if lo < hi:
            out[lo:hi, c0:c1] = slots[i, lo - by * bs:hi - by * bs, :c1 - c0]
    return out.reshape(-1)


# ---- the same five, element by element (what test_plane_tiles_cpu.py holds the models to) ---------------------------

def slow_changed(params, e, a, b, rows):
    w, bs = params.width, params.bin_size
    gx, gy = grid(params)
    flags = [0] * (gx * gy)
    for y in range(rows[0], rows[1]):
        for x in range(w):
            at = ((y - rows[0]) * w + x) * e
            if bytes(a[at:at + e]) != bytes(b[at:at + e]):
                flags[x // bs + (y // bs) * gx] = 1
    map_, tiles = [], []
    for i, f in enumerate(flags):
        map_.append(len(tiles) if f else -1)
        if f:
            tiles.append((i % gx) | ((i // gx) << 16))
    return np.array(map_, dtype=np.int32), np.array(tiles, dtype=np.int32), len(tiles)


def _slow_copy(params, e, tiles, rows, slots, plane, plane_row0, to_slots):
    """Every element of every listed slot that lies in the view and in `rows`, one at a time, either way."""
    w, h, bs = params.width, params.height, params.bin_size
    gx, gy = grid(params)
    for i, t in enumerate(tiles):
        bx, by = int(t) & 0xFFFF, int(t) >> 16
        if bx >= gx or by < 0 or by >= gy:
            continue
        for p in range(bs * bs):
            y, x = by * bs + p // bs, bx * bs + p % bs
            if x < w and y < h and rows[0] <= y < rows[1]:
                s, f = (i * bs * bs + p) * e, ((y - plane_row0) * w + x) * e
                if to_slots:
                    slots[s:s + e] = plane[f:f + e]
                else:
                    plane[f:f + e] = slots[s:s + e]


def slow_pack(params, e, tiles, block, rows, guard):
    out = np.full(len(tiles) * params.bin_size ** 2 * e, guard, dtype=np.uint8)
    _slow_copy(params, e, tiles, rows, out, np.asarray(block, dtype=np.uint8), rows[0], True)
    return out


def slow_unpack(params, e, tiles, packed, frame):
    out = np.array(frame, dtype=np.uint8)
    _slow_copy(params, e, tiles, (0, params.height), np.asarray(packed, dtype=np.uint8), out, 0, False)
    return out


def slow_apply(params, e, tiles, packed, rows, frame):
    out = np.array(frame, dtype=np.uint8)
    _slow_copy(params, e, tiles, rows, np.asarray(packed, dtype=np.uint8), out, 0, False)
    return out


def slow_assemble(params, e, map_, packed, fill, frame, rows):
    w, bs = params.width, params.bin_size
    gx, gy = grid(params)
    out = np.array(frame, dtype=np.uint8)
    fill = np.frombuffer(bytes(fill), dtype=np.uint8)
    for y in range(rows[0], rows[1]):
        for x in range(w):
            slot = int(map_[x // bs + (y // bs) * gx])
            f = (y * w + x) * e
            if slot < 0:
                out[f:f + e] = fill
            else:
                s = (slot * bs * bs + (y % bs) * bs + x % bs) * e
                out[f:f + e] = packed[s:s + e]
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------

def random_plane(rng, nbytes):
    return rng.integers(0, 256, nbytes, dtype=np.uint8)


def flips(params, e, rows):
    """The flips of tests/delta.py, each touching ONE byte of one element, on a WHOLE plane, as (x, y, byte of the
    element, xor mask, what it is), y absolute: first those inside the block `rows`, then those in a row just outside it
    (none when the block is the whole frame). The delta.py masks name the byte (0xFF000000 is the last byte of a 4-byte
    element, here the last byte of any element); at E = 28 one tile is flipped in byte 0 only and another in byte 27
    only."""
    inside, outside = D.flips(params, rows)

    def one_byte(k, mask):
        word_byte = [i for i in range(4) if (mask >> (8 * i)) & 0xFF][-1]  # the highest byte the 4-byte flip touches
        byte = {0: 0, 1: min(1, e - 1), 2: e // 2, 3: e - 1}[word_byte]
        if k == 0:
            byte = e - 1   # "alpha byte only; first tile": the element's last byte only
        if k == 1:
            byte = 0       # the right-edge tile: the element's first byte only
        return byte, ((mask >> (8 * word_byte)) & 0xFF) or 1

    ins = [(x, y) + one_byte(k, m) + (what,) for k, (x, y, m, what) in enumerate(inside)]
    outs = [(x, y) + one_byte(len(inside) + k, m) + (what,) for k, (x, y, m, what) in enumerate(outside)]
    return ins, outs


def flipped(params, e, a_full, which):
    b = np.array(a_full, dtype=np.uint8)
    for x, y, byte, mask, _ in which:
        b[(y * params.width + x) * e + byte] ^= np.uint8(mask)
    return b


def check_flips(params, e, rows):
    """What the flip case is named for, asserted from the flips and the model alone (no GPU): returns nothing."""
    w, h, bs = params.width, params.height, params.bin_size
    gx, gy = grid(params)
    r0, r1 = rows
    if (w, h, bs) in D.FRAMES:
        D.check_flips(params, rows)  # the positions are delta.py's, and reach what delta.py names on delta.py's frames
    inside, outside = flips(params, e, rows)
    assert all(r0 <= y < r1 and 0 <= x < w for x, y, _, _, _ in inside)
    assert all((y == r0 - 1 or y == r1) and 0 <= y < h for x, y, _, _, _ in outside) and (rows == (0, h) or outside)
    assert any(x == w - 1 for x, _, _, _, _ in inside) and any(y == r1 - 1 for _, y, _, _, _ in inside)
    assert [(x, y) for x, y, _, _, _ in inside] == [(x, y) for x, y, _, _ in D.flips(params, rows)[0]]
    assert all(0 <= byte < e and 0 < mask < 256 for _, _, byte, mask, _ in inside + outside)
    tile_of = lambda x, y: (x // bs, y // bs)
    assert inside[0][2] == e - 1 and inside[1][2] == 0, "the last byte only in one element, the first only in another"
    if gx > 1:
        assert tile_of(*inside[0][:2]) != tile_of(*inside[1][:2]), "in two tiles"
    a = random_plane(np.random.default_rng(7), w * h * e)
    cut = slice(r0 * w * e, r1 * w * e)
    tiles = {tile_of(x, y) for x, y, _, _, _ in inside}
    _, got, count = changed(params, e, a[cut], flipped(params, e, a, inside + outside)[cut], rows)
    assert count == len(tiles) and sorted(int(t) for t in got) == sorted(bx | by << 16 for bx, by in tiles)
    assert changed(params, e, a[cut], flipped(params, e, a, outside)[cut], rows)[2] == 0
    # each flip alone changes exactly one byte
    for f in inside + outside:
        assert (flipped(params, e, a, [f]) != a).sum() == 1


def background_texel(T):
    """The G-buffer texel of a pixel nothing covers (the definition of par_relight_device), as 28 bytes."""
    texel = np.zeros(1, dtype=T.PIXEL)
    texel["color"]["red"] = texel["color"]["green"] = texel["color"]["blue"] = T.default_params().background
    return texel.tobytes()
