"""Upscale (par_upscale_device, par_upscale_host) restated on the host: the contract beside the declarations in
include/par_raytracer.h in numpy (`model`: whole-plane comparisons of edge-padded shifts, Scale4x as Scale2x of the
Scale2x plane), and the same for one output pixel at a time in plain Python integers (`slow_model`, which
tests/test_upscale_cpu.py holds `model` to; its Scale4x is two applications of its own per-pixel Scale2x)."""
import numpy as np

RGBA, BGRA = 0, 1


def _desc(desc):
    d = np.asarray(desc).reshape(-1)[0]
    return int(d["scaler"]), int(d["pitch"]), int(d["order"])


def _elements(params, src_rows, rows, fb, index):
    """The source as a (s1 - s0, width) plane of integers whose equality is the contract's, with the row ranges."""
    r0, r1 = rows or (0, params.height)
    s0, s1 = src_rows or (r0, r1)
    assert (fb is None) != (index is None) and 0 <= s0 <= r0 < r1 <= s1 <= params.height
    if index is not None:
        e = np.ascontiguousarray(index, dtype=np.uint8).astype(np.uint32)
    else:
        e = np.ascontiguousarray(fb).view(np.uint32)
    return e.reshape(s1 - s0, params.width), (s0, s1, r0, r1)


def _neighbours(e):
    """A B C / D E F / G H I of every element of the plane, the clamp at its four edges applied."""
    p = np.pad(e, 1, mode="edge")
    h, w = e.shape
    return [p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def scale2x(e):
    _, B, _, D, E, F, _, H, _ = _neighbours(e)
    g = (B != H) & (D != F)
    out = np.empty((2 * e.shape[0], 2 * e.shape[1]), dtype=e.dtype)
    out[0::2, 0::2] = np.where(g & (D == B), D, E)
    out[0::2, 1::2] = np.where(g & (B == F), F, E)
    out[1::2, 0::2] = np.where(g & (D == H), D, E)
    out[1::2, 1::2] = np.where(g & (H == F), F, E)
    return out


def scale3x(e):
    A, B, C, D, E, F, G, H, I = _neighbours(e)
    g = (B != H) & (D != F)
    out = np.empty((3 * e.shape[0], 3 * e.shape[1]), dtype=e.dtype)
    out[0::3, 0::3] = np.where(g & (D == B), D, E)
    out[0::3, 1::3] = np.where(g & (((D == B) & (E != C)) | ((B == F) & (E != A))), B, E)
    out[0::3, 2::3] = np.where(g & (B == F), F, E)
    out[1::3, 0::3] = np.where(g & (((D == B) & (E != G)) | ((D == H) & (E != A))), D, E)
    out[1::3, 1::3] = E
    out[1::3, 2::3] = np.where(g & (((B == F) & (E != I)) | ((H == F) & (E != C))), F, E)
    out[2::3, 0::3] = np.where(g & (D == H), D, E)
    out[2::3, 1::3] = np.where(g & (((D == H) & (E != I)) | ((H == F) & (E != G))), H, E)
    out[2::3, 2::3] = np.where(g & (H == F), F, E)
    return out


def scaled_elements(e, k):
    """The plane `e` through the scaler of factor k: a (k * rows, k * columns) plane of `e`'s elements."""
    if k == 2:
        return scale2x(e)
    if k == 3:
        return scale3x(e)
    assert k == 4
    return scale2x(scale2x(e))


def _surface(elements, pitch, order, fb_source, palette, guard):
    """The elements as colours on a surface of that pitch: (rows, pitch) bytes, `guard` in the gaps."""
    if fb_source:
        c = np.ascontiguousarray(elements, dtype=np.uint32)
    else:
        c = np.ascontiguousarray(palette).view(np.uint32)[np.minimum(elements, len(palette) - 1)]  # the clamp
    px = np.ascontiguousarray(c).view(np.uint8).reshape(c.shape[0], c.shape[1], 4)
    if order == BGRA:
        px = px[:, :, [2, 1, 0, 3]]
    out = np.full((c.shape[0], pitch), guard, dtype=np.uint8)
    out[:, :4 * c.shape[1]] = px.reshape(c.shape[0], 4 * c.shape[1])
    return out


def model(params, desc, src_rows, rows, fb=None, index=None, palette=None, guard=0):
    """(surface, index plane) of output rows `rows` (None: the whole frame) from the flat COLOR array `fb` or the flat
    uint8 array `index`, either holding rows `src_rows` (None: `rows`). The surface is (rows * k, pitch) uint8 with
    `guard` in the gap bytes of every row, None for an index source without a palette; the index plane is
    (rows * k, width * k) uint8, None for an fb source."""
    k, pitch, order = _desc(desc)
    e, (s0, s1, r0, r1) = _elements(params, src_rows, rows, fb, index)
    big = scaled_elements(e, k)[k * (r0 - s0):k * (r1 - s0)]
    plane = big.astype(np.uint8) if index is not None else None
    if index is not None and palette is None:
        return None, plane
    return _surface(big, pitch, order, fb is not None, palette, guard), plane


# ---- one output pixel at a time -----------------------------------------------------------------------------------------

def _scale2x_pixel(get, x, y, sx, sy):
    """Sub-element (sx, sy) of the Scale2x block of the element (x, y) of the plane that `get` reads (with its clamps)."""
    B, D, E, F, H = get(x, y - 1), get(x - 1, y), get(x, y), get(x + 1, y), get(x, y + 1)
    g = B != H and D != F
    if (sx, sy) == (0, 0):
        return D if g and D == B else E
    if (sx, sy) == (1, 0):
        return F if g and B == F else E
    if (sx, sy) == (0, 1):
        return D if g and D == H else E
    return F if g and H == F else E


def _scale3x_pixel(get, x, y, sx, sy):
    A, B, C = get(x - 1, y - 1), get(x, y - 1), get(x + 1, y - 1)
    D, E, F = get(x - 1, y), get(x, y), get(x + 1, y)
    G, H, I = get(x - 1, y + 1), get(x, y + 1), get(x + 1, y + 1)
    g = B != H and D != F
    n = 3 * sy + sx
    if n == 0:
        return D if g and D == B else E
    if n == 1:
        return B if g and ((D == B and E != C) or (B == F and E != A)) else E
    if n == 2:
        return F if g and B == F else E
    if n == 3:
        return D if g and ((D == B and E != G) or (D == H and E != A)) else E
    if n == 4:
        return E
    if n == 5:
        return F if g and ((B == F and E != I) or (H == F and E != C)) else E
    if n == 6:
        return D if g and D == H else E
    if n == 7:
        return H if g and ((D == H and E != I) or (H == F and E != G)) else E
    return F if g and H == F else E


def slow_model(params, desc, src_rows, rows, fb=None, index=None, palette=None, guard=0):
    """`model`, one output pixel at a time in Python integers."""
    k, pitch, order = _desc(desc)
    r0, r1 = rows or (0, params.height)
    s0, s1 = src_rows or (r0, r1)
    W = params.width
    if index is not None:
        flat = [int(v) for v in np.asarray(index, dtype=np.uint8)]
    else:
        flat = [int(c["red"]) | int(c["green"]) << 8 | int(c["blue"]) << 16 | int(c["alpha"]) << 24 for c in fb]
    assert len(flat) == (s1 - s0) * W

    def source(x, y):  # absolute row y; the contract's clamps
        x, y = min(max(x, 0), W - 1), min(max(y, s0), s1 - 1)
        return flat[(y - s0) * W + x]

    def doubled(X, Y):  # T of Scale4x: absolute row Y of the 2x plane; T's own clamps
        X, Y = min(max(X, 0), 2 * W - 1), min(max(Y, 2 * s0), 2 * s1 - 1)
        return _scale2x_pixel(source, X // 2, Y // 2, X % 2, Y % 2)

    want_surface = index is None or palette is not None
    out = np.full(((r1 - r0) * k, pitch), guard, dtype=np.uint8) if want_surface else None
    plane = np.zeros(((r1 - r0) * k, W * k), dtype=np.uint8) if index is not None else None
    for Y in range(k * r0, k * r1):
        for X in range(k * W):
            if k == 2:
                e = _scale2x_pixel(source, X // 2, Y // 2, X % 2, Y % 2)
            elif k == 3:
                e = _scale3x_pixel(source, X // 3, Y // 3, X % 3, Y % 3)
            else:
                e = _scale2x_pixel(doubled, X // 2, Y // 2, X % 2, Y % 2)
            if plane is not None:
                plane[Y - k * r0, X] = e
            if out is None:
                continue
            if index is not None:
                p = palette[min(e, len(palette) - 1)]
                c = [int(p["red"]), int(p["green"]), int(p["blue"]), int(p["alpha"])]
            else:
                c = [e & 0xFF, (e >> 8) & 0xFF, (e >> 16) & 0xFF, e >> 24]
            if order == BGRA:
                c[0], c[2] = c[2], c[0]
            out[Y - k * r0, 4 * X:4 * X + 4] = c
    return out, plane


def halo(k):
    """Source rows on each side with which a row block's output is those rows of the whole frame's."""
    return 2 if k == 4 else 1


def with_halo(rows, height, k):
    return max(0, rows[0] - halo(k)), min(height, rows[1] + halo(k))


def three_colors(T, rng):
    """Three colours of which the first two differ in alpha only: a 24-bit compare takes them for one."""
    c = np.zeros(3, dtype=T.COLOR)
    for ch in ("red", "green", "blue", "alpha"):
        c[ch] = rng.integers(0, 256, 3, dtype=np.uint8)
    c[1] = c[0]
    c["alpha"][1] = c["alpha"][0] ^ 0x80
    c["red"][2] = c["red"][0] ^ 0x55  # the third differs in colour
    return c
