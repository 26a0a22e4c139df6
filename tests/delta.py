"""The contract of the changed-tiles calls (include/par_raytracer.h) restated in numpy, the shared frames of their tests
and the flips that make a frame differ. Planes are uint32 arrays (one word a pixel) of the block's rows; tests/
test_delta_cpu.py holds the three models to per-pixel loops without a GPU.
  changed(params, a, b, rows)               -> (map, tiles, count)
  pack(params, tiles, block, rows, guard)   -> the slots' bytes, unwritten bytes equal to the guard
  apply(params, tiles, packed, rows, frame) -> the frame (a copy) with the slots' in-block pixels in place"""
import numpy as np

# (width, height, bin size): the smallest frames at which each mechanism of the kernels can go wrong
FRAMES = [
    (37, 23, 8),      # edge tile 5 wide and 7 tall; W % 4 != 0
    (64, 16, 8),      # everything on the wide path
    (50, 20, 12),     # B % 4 == 0 with W % 4 == 2; last tile 2 wide
    (130, 35, 10),    # B % 4 != 0: a 16-byte piece straddles two tiles; last bin row 5 tall
    (160, 161, 160),  # largest bin; the last bin row is one pixel row
    (320, 240, 8),    # 1200 tiles: more than one round of the compaction workgroup has threads
]


def block_rows(h):
    """The row block every frame is also run on."""
    return (5, 18) if h >= 18 else (5, 16)


def grid(params):
    b = params.bin_size
    return (params.width + b - 1) // b, (params.height + b - 1) // b


def tile_rows(params, by, rows):
    """Rows of tile row `by` that lie in the block (possibly none)."""
    b = params.bin_size
    return max(by * b, rows[0]), min((by + 1) * b, params.height, rows[1])


def changed(params, a, b, rows):
    w, bs = params.width, params.bin_size
    gx, gy = grid(params)
    r0, r1 = rows
    diff = (np.asarray(a, dtype=np.uint32).reshape(r1 - r0, w) != np.asarray(b, dtype=np.uint32).reshape(r1 - r0, w))
    full = np.zeros((gy * bs, gx * bs), dtype=bool)  # the whole grid's pixels; outside the block nothing differs
    full[r0:r1, :w] = diff
    flags = full.reshape(gy, bs, gx, bs).any(axis=(1, 3)).reshape(-1)
    where = np.nonzero(flags)[0]
    map_ = np.full(gx * gy, -1, dtype=np.int32)
    map_[where] = np.arange(len(where), dtype=np.int32)
    tiles = ((where % gx) | ((where // gx) << 16)).astype(np.int32)
    return map_, tiles, len(where)


def pack(params, tiles, block, rows, guard):
    w, bs = params.width, params.bin_size
    gx, gy = grid(params)
    r0, r1 = rows
    src = np.asarray(block, dtype=np.uint32).reshape(r1 - r0, w)
    word = np.frombuffer(bytes([guard]) * 4, dtype=np.uint32)[0]
    out = np.full((len(tiles), bs, bs), word, dtype=np.uint32)
    for i, t in enumerate(np.asarray(tiles, dtype=np.int32)):
        bx, by = int(t) & 0xFFFF, int(t) >> 16
        if bx >= gx or by < 0 or by >= gy:
            continue
        lo, hi = tile_rows(params, by, rows)
        c0, c1 = bx * bs, min((bx + 1) * bs, w)
        if lo < hi:
            out[i, lo - by * bs:hi - by * bs, :c1 - c0] = src[lo - r0:hi - r0, c0:c1]
    return out.reshape(-1).view(np.uint8)


def apply(params, tiles, packed, rows, frame):
    w, h, bs = params.width, params.height, params.bin_size
    out = np.array(frame, dtype=np.uint32).reshape(h, w)
    slots = np.asarray(packed).view(np.uint32).reshape(-1, bs, bs)
    for i, t in enumerate(np.asarray(tiles, dtype=np.int32)):
        bx, by = int(t) & 0xFFFF, int(t) >> 16
        lo, hi = tile_rows(params, by, rows)
        c0, c1 = bx * bs, min((bx + 1) * bs, w)
        if lo < hi:
            out[lo:hi, c0:c1] = slots[i, lo - by * bs:hi - by * bs, :c1 - c0]
    return out.reshape(-1)


# ---- the same three, pixel by pixel (what test_delta_cpu.py holds the models to) ----------------------------------

def slow_changed(params, a, b, rows):
    w, bs = params.width, params.bin_size
    gx, gy = grid(params)
    flags = [0] * (gx * gy)
    for y in range(rows[0], rows[1]):
        for x in range(w):
            if int(a[(y - rows[0]) * w + x]) != int(b[(y - rows[0]) * w + x]):
                flags[x // bs + (y // bs) * gx] = 1
    map_, tiles = [], []
    for i, f in enumerate(flags):
        map_.append(len(tiles) if f else -1)
        if f:
            tiles.append((i % gx) | ((i // gx) << 16))
    return np.array(map_, dtype=np.int32), np.array(tiles, dtype=np.int32), len(tiles)


def slow_pack(params, tiles, block, rows, guard):
    w, h, bs = params.width, params.height, params.bin_size
    out = np.full(len(tiles) * bs * bs * 4, guard, dtype=np.uint8)
    words = out.view(np.uint32)
    for i, t in enumerate(tiles):
        bx, by = int(t) & 0xFFFF, int(t) >> 16
        for p in range(bs * bs):
            y, x = by * bs + p // bs, bx * bs + p % bs
            if x < w and y < h and rows[0] <= y < rows[1]:
                words[i * bs * bs + p] = block[(y - rows[0]) * w + x]
    return out


def slow_apply(params, tiles, packed, rows, frame):
    w, h, bs = params.width, params.height, params.bin_size
    out = np.array(frame, dtype=np.uint32)
    words = np.asarray(packed).view(np.uint32)
    for i, t in enumerate(tiles):
        bx, by = int(t) & 0xFFFF, int(t) >> 16
        for p in range(bs * bs):
            y, x = by * bs + p // bs, bx * bs + p % bs
            if x < w and y < h and rows[0] <= y < rows[1]:
                out[y * w + x] = words[i * bs * bs + p]
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------

def random_plane(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def flips(params, rows):
    """The single-pixel flips of GPU case 1, on a WHOLE frame, as (x, y, xor mask, what it is), y absolute: first those
    inside the block `rows`, then those in a row just outside it (none when the block is the whole frame). The planes of
    a block are rows [r0, r1) of the whole frames, so an outside flip lies right beside the memory the call may read."""
    w, h, bs = params.width, params.height, params.bin_size
    gx, gy = grid(params)
    r0, r1 = rows
    inside = [
        (0, r0, 0xFF000000, "alpha byte only; first tile"),
        (w - 1, r0, 0x00000100, "last column of a right-edge tile"),
        (w - 1, r1 - 1, 0x00010000, "last tile, its last pixel: last row of a bottom-edge tile"),
    ]
    if gx > 1:
        inside.append((bs, r1 - 1, 0x00000001, "last row of a bottom-edge tile that is no right-edge tile"))
    if gx > 3:
        inside.append((2 * bs + bs // 2, r0 + 1, 0x80, "a tile with exactly one changed pixel"))
    outside = []
    if r0 > 0:
        outside.append((w // 2, r0 - 1, 0x00FFFF00, "the row before the block"))
    if r1 < h:
        outside.append((w // 2, r1, 0x00FFFF00, "the row after the block"))
    return inside, outside


def flipped(params, a_full, which):
    b = np.array(a_full, dtype=np.uint32)
    for x, y, mask, _ in which:
        b[y * params.width + x] ^= np.uint32(mask)
    return b


def check_flips(params, rows):
    """What case 1 is named for, asserted from the flips and the model alone (no GPU): returns nothing."""
    w, h, bs = params.width, params.height, params.bin_size
    gx, gy = grid(params)
    r0, r1 = rows
    inside, outside = flips(params, rows)
    tile_of = lambda x, y: (x // bs, y // bs)
    by_lo, by_hi = r0 // bs, (r1 - 1) // bs
    assert any(m == 0xFF000000 for _, _, m, _ in inside), "a flip in the alpha byte only"
    assert any(x == w - 1 and tile_of(x, y)[0] == gx - 1 for x, y, _, _ in inside), "last column of a right-edge tile"
    assert any(y == min((by_hi + 1) * bs, h, r1) - 1 and tile_of(x, y)[1] == by_hi for x, y, _, _ in inside)
    if rows == (0, h):
        assert any(y == h - 1 for _, y, _, _ in inside), "the last row of a bottom-edge tile"
        assert tile_of(*inside[0][:2]) == (0, 0) and tile_of(*inside[2][:2]) == (gx - 1, gy - 1), "first and last tile"
    assert tile_of(*inside[0][:2]) == (0, by_lo) and tile_of(*inside[2][:2]) == (gx - 1, by_hi)
    tiles = [tile_of(x, y) for x, y, _, _ in inside]
    assert len(set((x, y) for x, y, _, _ in inside)) == len(inside), "no pixel is flipped twice"
    if gx > 1 or by_hi > by_lo:  # (one tile in the block: it takes every flip)
        assert any(tiles.count(t) == 1 for t in tiles), "a tile with exactly one changed pixel"
    assert all(r0 <= y < r1 and 0 <= x < w for x, y, _, _ in inside)
    if rows != (0, h):
        assert outside, "a block has a row outside it"
    for x, y, _, _ in outside:
        assert (y == r0 - 1 or y == r1) and 0 <= y < h
        assert by_lo <= y // bs <= by_hi, "the outside flip's tile is in the block"
    # the model sees the inside flips' tiles, and nothing of the outside ones
    a = random_plane(np.random.default_rng(7), w * h)
    cut = slice(r0 * w, r1 * w)
    _, got, count = changed(params, a[cut], flipped(params, a, inside + outside)[cut], rows)
    assert count == len(set(tiles)) and sorted(int(t) for t in got) == sorted(bx | by << 16 for bx, by in set(tiles))
    assert changed(params, a[cut], flipped(params, a, outside)[cut], rows)[2] == 0
