"""The tile-budget contract of addons/include/par_tileset_reduce.h restated in numpy: what the GPU tests compare with byte
for byte. model() is vectorised: a tile is a one-hot vector over (pixel, distinct colour), so the distances of every tile
to the images of one new centre are one matrix product a step, exact in float32 (sums of integers below 2^24);
model_loop() says the same slowly: per tile, per kept tile, per flip, per pixel, in Python integers; most_used() is the
baseline the figures are set beside: keep the K most used tiles. A set is a uint8 array (capacity, th, tw), a palette a
uint8 array (n_colors, 4); both models return (tiles_out, map_out, remap, count, error)."""
import numpy as np

import tileset as TS

ID_MASK = TS.ID_MASK
MAX_TILES, MAX_BUDGET = 4096, 1024


def allowed(flips):
    return [f for f in range(4) if not f & ~flips]


def usage(tile_map, t):
    return np.bincount(np.minimum(np.asarray(tile_map, np.uint32) & ID_MASK, t - 1), minlength=t).astype(np.int64)


def finish(tiles, t, tile_map, u, kept, d, a, g):
    """The outputs from the kept marks and (d, a, g) of every tile."""
    new = np.cumsum(kept) - kept
    remap = np.where(kept, new, new[a] | (g << 30)).astype(np.uint32)
    m = np.asarray(tile_map, np.uint32)
    r = remap[np.minimum(m & ID_MASK, t - 1)]
    map_out = ((r & ID_MASK) | (((m >> 30) ^ (r >> 30)) << 30)).astype(np.uint32)
    error = int((u[~kept] * d[~kept]).sum())
    return tiles[:t][kept].copy(), map_out, remap, int(kept.sum()), error


def nothing(tiles, tile_map):
    return tiles[:0].copy(), np.asarray(tile_map, np.uint32).copy(), np.zeros(0, np.uint32), 0, 0


def classes_of(palette):
    """(class of every palette entry, the L1 table of the classes): entries of equal red, green and blue are one class."""
    rgb = np.asarray(palette, np.uint8).reshape(-1, 4)[:, :3].astype(np.int64)
    distinct, inverse = np.unique(rgb, axis=0, return_inverse=True)
    table = np.abs(distinct[:, None, :] - distinct[None, :, :]).sum(axis=2)
    return inverse.reshape(-1), table


def model(tiles, count, tile_map, palette, budget, flips=0):
    tiles = np.asarray(tiles, np.uint8)
    capacity, th, tw = tiles.shape
    t = min(int(count), capacity)
    if t == 0:
        return nothing(tiles, tile_map)
    u = usage(tile_map, t)
    if t <= budget:
        every = np.arange(t)
        return finish(tiles, t, tile_map, u, np.ones(t, bool), np.zeros(t, np.int64), every, np.zeros(t, np.int64))
    cls, table = classes_of(palette)
    used, seen = np.unique(cls[np.minimum(tiles[:t], len(cls) - 1)], return_inverse=True)  # the classes the tiles show
    table, seen = table[np.ix_(used, used)], seen.reshape(t, th, tw)
    n_cls = len(table)
    px = th * tw
    onehot = np.zeros((t, px * n_cls), np.float32)
    onehot[np.arange(t)[:, None], np.arange(px)[None, :] * n_cls + seen.reshape(t, px)] = 1
    codes = allowed(flips)
    kept = np.zeros(t, bool)
    d = np.full(t, 1 << 40, np.int64)
    a = np.zeros(t, np.int64)
    g = np.zeros(t, np.int64)
    c = int(np.argmax(u))  # (argmax takes the first of equals: the lowest number)
    for step in range(budget):
        kept[c] = True
        images = np.stack([TS.flipped(seen[c:c + 1], f).reshape(px) for f in codes])  # (F, px)
        # cost[pixel * n_cls + class, image] = |class - the image's class at the pixel|
        cost = np.ascontiguousarray(table[:, images].transpose(2, 0, 1)).reshape(px * n_cls, len(codes)).astype(np.float32)
        dist = np.rint(onehot @ cost).astype(np.int64)  # (t, F)
        best = dist.argmin(axis=1)  # (the first of equals: the lowest code)
        D = dist[np.arange(t), best]
        better = (D < d) | ((D == d) & (c < a))
        d[better], a[better], g[better] = D[better], c, np.asarray(codes)[best[better]]
        score = np.where(kept, -1, u * d)
        c = int(np.argmax(score))
    return finish(tiles, t, tile_map, u, kept, d, a, g)


def distance_loop(palette, x, y, f):
    """D of the contract in Python integers: tile x against the image of tile y under f."""
    th, tw = len(x), len(x[0])
    n = len(palette)
    total = 0
    for r in range(th):
        for q in range(tw):
            p = palette[min(x[r][q], n - 1)]
            o = palette[min(y[th - 1 - r if f & 2 else r][tw - 1 - q if f & 1 else q], n - 1)]
            total += abs(p[0] - o[0]) + abs(p[1] - o[1]) + abs(p[2] - o[2])
    return total


def model_loop(tiles, count, tile_map, palette, budget, flips=0):
    tiles = np.asarray(tiles, np.uint8)
    t = min(int(count), len(tiles))
    if t == 0:
        return nothing(tiles, tile_map)
    rows = tiles.tolist()
    pal = np.asarray(palette, np.uint8).reshape(-1, 4).tolist()
    u = [0] * t
    for word in np.asarray(tile_map, np.uint32).tolist():
        u[min(word & ID_MASK, t - 1)] += 1
    codes = allowed(flips)
    memo = {}

    def nearest(i, centres):
        """(d, a, g) of tile i over the kept tiles `centres`: the least D, then the lowest k, then the lowest f."""
        best = None
        for k in sorted(centres):
            for f in codes:
                if (i, k, f) not in memo:
                    memo[(i, k, f)] = distance_loop(pal, rows[i], rows[k], f)
                if best is None or memo[(i, k, f)] < best[0]:
                    best = (memo[(i, k, f)], k, f)
        return best

    if t <= budget:
        centres = list(range(t))
    else:
        centres = [max(range(t), key=lambda i: (u[i], -i))]
        while len(centres) < budget:
            outside = [i for i in range(t) if i not in centres]
            centres.append(max(outside, key=lambda i: (u[i] * nearest(i, centres)[0], -i)))
    kept = np.zeros(t, bool)
    kept[centres] = True
    near = [nearest(i, centres) for i in range(t)]
    d, a, g = (np.array([n[k] for n in near], np.int64) for k in range(3))
    return finish(tiles, t, tile_map, np.array(u, np.int64), kept, d, a, g)


def most_used(tiles, count, tile_map, palette, budget, flips=0):
    """The baseline: keep the `budget` most used tiles (the lowest number among equals), the rest to the nearest kept."""
    tiles = np.asarray(tiles, np.uint8)
    t = min(int(count), len(tiles))
    u = usage(tile_map, t)
    kept = np.zeros(t, bool)
    kept[np.argsort(-u, kind="stable")[:budget]] = True
    rgb = np.asarray(palette, np.uint8).reshape(-1, 4)[:, :3].astype(np.int32)
    colour = rgb[np.minimum(tiles[:t], len(rgb) - 1)]  # (t, th, tw, 3)
    d = np.full(t, 1 << 40, np.int64)
    a, g = np.zeros(t, np.int64), np.zeros(t, np.int64)
    for k in np.flatnonzero(kept):
        for f in allowed(flips):
            image = colour[k, ::-1 if f & 2 else 1, ::-1 if f & 1 else 1]
            D = np.abs(colour - image[None]).sum(axis=(1, 2, 3)).astype(np.int64)
            better = D < d  # (k and f ascend: the first of equals stays)
            d[better], a[better], g[better] = D[better], k, f
    return finish(tiles, t, tile_map, u, kept, d, a, g)


def view(palette, tiles, tile, tile_map, w, rows):
    """The expanded plane seen through the palette: (rows * w, 3) int64."""
    rgb = np.asarray(palette, np.uint8).reshape(-1, 4)[:, :3].astype(np.int64)
    return rgb[np.minimum(TS.expand_model(tiles, tile, tile_map, w, rows), len(rgb) - 1)]


def random_set(rng, n_tiles, tile, colours, n_cells, kinds=None, spare=0):
    """(tiles (n_tiles + spare, th, tw), map (n_cells,)): tiles that are few-pixel variations of `kinds` base tiles, so
    that distances tie and differ, some of them mirrored, and a map that uses some tiles often, some once and some never, under random codes."""
    tw, th = tile
    kinds = kinds or max(1, n_tiles // 6)
    base = rng.integers(0, colours, (kinds, th, tw), dtype=np.uint8)
    tiles = base[rng.integers(0, kinds, n_tiles + spare)].copy()
    for f in range(1, 4):  # mirrors of the base tiles too, so that a dropped tile's nearest image is often a mirror
        at = rng.integers(0, n_tiles + spare, (n_tiles + spare) // 4)
        tiles[at] = TS.flipped(tiles[at], f)
    for k in range(3):
        at = rng.integers(0, n_tiles + spare, (n_tiles + spare) // 2)
        tiles[at, rng.integers(0, th, len(at)), rng.integers(0, tw, len(at))] = rng.integers(0, colours, len(at), dtype=np.uint8)
    ids = np.minimum(rng.integers(0, n_tiles, n_cells), rng.integers(0, n_tiles, n_cells)).astype(np.uint32)
    ids[rng.integers(0, n_cells, max(1, n_cells // 8))] = rng.integers(0, max(1, n_tiles // 4))
    return tiles, (ids | (rng.integers(0, 4, n_cells).astype(np.uint32) << 30)).astype(np.uint32)


def random_palette(rng, n_colors, duplicates=True):
    pal = rng.integers(0, 256, (n_colors, 4), dtype=np.uint8)
    if duplicates and n_colors > 2:
        pal[n_colors // 2, :3] = pal[0, :3]  # equal colours under different alphas
        pal[-1, :3] = pal[1, :3]
    return pal


# ---- sets worked out by hand -----------------------------------------------------------------------------------------

CRAFTED_PALETTE = np.array([[0, 0, 0, 255], [10, 0, 0, 255], [0, 30, 0, 255], [10, 0, 0, 7], [1, 1, 1, 0]], np.uint8)


def dotted(*dots):
    """An 8 x 8 tile of zeros with byte b at row y, column x for every (y, x, b)."""
    t = np.zeros((8, 8), np.uint8)
    for y, x, b in dots:
        t[y, x] = b
    return t


def entries(*pairs):
    return np.array([i | (f << 30) for i, f in pairs], dtype=np.uint32)


def crafted():
    """name -> ((tiles, count, map, budget, flips), (tiles_out, map_out, remap, count, error)): tiles of 8 x 8 over
    CRAFTED_PALETTE, where the colours 0, 1 and 2 are 10, 30 and 40 apart (0-1, 0-2, 1-2) and entry 3 has entry 1's colour
    under another alpha. z is the tile of zeros, A has a 1 in its corner, B a 2: D(z, A) = 10, D(z, B) = 30, D(A, B) = 40."""
    z, A, B = dotted(), dotted((0, 0, 1)), dotted((0, 0, 2))
    out = {}
    # every tile is used once: S_1 is tile 0; at K = 2 the products are 10 and 30, B is kept, A goes to z (10 < 40)
    m = entries((0, 0), (1, 0), (2, 0))
    out["equal usages, K 1"] = ((np.stack([z, A, B]), 3, m, 1, 0), (z[None], entries((0, 0), (0, 0), (0, 0)), entries((0, 0), (0, 0), (0, 0)), 1, 40))
    out["equal usages, K 2"] = ((np.stack([z, A, B]), 3, m, 2, 0), (np.stack([z, B]), entries((0, 0), (0, 0), (1, 0)), entries((0, 0), (0, 0), (1, 0)), 2, 10))
    # z five times, A three times (3 * 10), C once (1 * 30): equal products, the lower number A is kept; C goes to z (30 < 40)
    C = dotted((7, 7, 2))
    m = entries(*[(0, 0)] * 5, *[(1, 0)] * 3, (2, 0))
    out["equal products"] = ((np.stack([z, A, C]), 3, m, 2, 0),
                             (np.stack([z, A]), entries(*[(0, 0)] * 5, *[(1, 0)] * 3, (0, 0)), entries((0, 0), (1, 0), (0, 0)), 2, 30))
    # a centre that equals its mirrors: every image of z is z, the lowest code 0 is taken
    m = entries((0, 0), (0, 0), (1, 3))
    out["a centre that equals its own mirror"] = ((np.stack([z, A]), 2, m, 1, 3), (z[None], entries((0, 0), (0, 0), (0, 3)), entries((0, 0), (0, 0)), 1, 10))
    # X equals its x mirror; Y is its y mirror: codes 2 and 3 both give D = 0, the lower, 2, is taken
    X, Y = dotted((0, 0, 1), (0, 7, 1)), dotted((7, 0, 1), (7, 7, 1))
    m = entries((0, 0), (0, 0), (1, 0), (1, 2))
    out["a centre that equals its x mirror"] = ((np.stack([X, Y]), 2, m, 1, 3), (X[None], entries((0, 0), (0, 0), (0, 2), (0, 0)), entries((0, 0), (0, 2)), 1, 0))
    # A2 has its 1 beside A's: D(A, A2) = 20. A2 is used most and is S_1, then A (3 * 20 = 60 against z's 10); z is 10 from
    # both: the lower number, A, takes it although A2 was kept first
    A2 = dotted((0, 1, 1))
    m = entries(*[(1, 0)] * 4, *[(0, 0)] * 3, (2, 0))
    out["two kept tiles at equal distance"] = ((np.stack([A, A2, z]), 3, m, 2, 0),
                                               (np.stack([A, A2]), entries(*[(1, 0)] * 4, *[(0, 0)] * 4), entries((0, 0), (1, 0), (0, 0)), 2, 10))
    # A3 shows palette entry 3 where A shows entry 1: the same colour, D = 0; its product 2 * 0 loses against z's 1 * 10
    A3 = dotted((0, 0, 3))
    m = entries((0, 0), (0, 0), (1, 0), (1, 0), (2, 0))
    out["duplicate colours"] = ((np.stack([A, A3, z]), 3, m, 2, 0),
                                (np.stack([A, z]), entries((0, 0), (0, 0), (0, 0), (0, 0), (1, 0)), entries((0, 0), (0, 0), (1, 0)), 2, 0))
    # U is stored and unused: its product is 0 * 30, A's 1 * 10: A is kept, U goes to z (30 < 40) at no error
    U = dotted((3, 3, 2))
    m = entries((0, 0), (0, 0), (0, 0), (1, 0))
    out["an unused tile"] = ((np.stack([z, A, U]), 3, m, 2, 0), (np.stack([z, A]), m.copy(), entries((0, 0), (1, 0), (0, 0)), 2, 0))
    # the unused U (0 * 40) and A3 (1 * 0) tie at 0: the lower number, U, is kept
    m = entries((0, 0), (0, 0), (2, 0))
    out["an unused tile kept on a tie at 0"] = ((np.stack([A, U, A3]), 3, m, 2, 0),
                                                (np.stack([A, U]), entries((0, 0), (0, 0), (0, 0)), entries((0, 0), (1, 0), (0, 0)), 2, 0))
    # a count of 2 in a capacity of 3: the ids 5 and 2 read as 1, the third stored tile is not a tile. A is used three
    # times and kept; z is 10 from A and from A's x mirror: code 0
    junk = np.full((8, 8), 0xEE, np.uint8)
    m = entries((0, 0), (5, 1), (2, 0), (1, 0))
    e = (A[None], entries((0, 0), (0, 1), (0, 0), (0, 0)), entries((0, 0), (0, 0)), 1, 10)
    out["ids beyond T"] = ((np.stack([z, A, junk]), 2, m, 1, 1), e)
    out["a count above the capacity"] = ((np.stack([z, A]), 9, m, 1, 1), e)
    # Q is P's x mirror with one more dot: D(Q, P) is 10 under code 1 and 90 under the others. Q's cells carry codes of
    # their own: 1 ^ 1 = 0 and 2 ^ 1 = 3
    P, Q = dotted((0, 0, 1), (0, 1, 2)), dotted((0, 7, 1), (0, 6, 2), (5, 5, 1))
    m = entries((0, 0), (0, 0), (0, 3), (1, 1), (1, 2))
    out["composed flips on a mirrored cell"] = ((np.stack([P, Q]), 2, m, 1, 3),
                                                (P[None], entries((0, 0), (0, 0), (0, 3), (0, 0), (0, 3)), entries((0, 0), (0, 1)), 1, 20))
    return out


CRAFTED = ["equal usages, K 1", "equal usages, K 2", "equal products", "a centre that equals its own mirror",
           "a centre that equals its x mirror", "two kept tiles at equal distance", "duplicate colours", "an unused tile",
           "an unused tile kept on a tie at 0", "ids beyond T", "a count above the capacity", "composed flips on a mirrored cell"]


def same(got, want, tag):
    """Two results (tiles_out, map_out, remap, count, error) are equal, dtypes and shapes included."""
    for name, x, y in zip(("tiles", "map", "remap"), got, want):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"{tag}: {name}: {x} for {y}"
    assert tuple(got[3:]) == tuple(want[3:]), f"{tag}: count, error: {got[3:]} for {want[3:]}"
