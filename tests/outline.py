"""Outlines (par_outline_device, par_outline_host) restated on the host: the contract beside the declarations in
include/par_raytracer.h in numpy on uint32 words (`model`), the same for one pixel at a time in plain Python integers
(`model_loop`, which tests/test_outline_cpu.py holds `model` to), and the carved device planes with guard bytes that the
GPU tests run the call on.

A G-buffer block is a flat PIXEL array holding rows `grows` = (g0, g1); the frame block `fb` is a flat COLOR array
holding rows `rows` = (r0, r1); a style is (depth_step, silhouette_scale, crease_scale) or an OUTLINE_STYLE array."""
import numpy as np

CHANNELS = ("red", "green", "blue")
M32 = 0xFFFFFFFF
# neighbour order of the contract: left, right, up, down as (dx, dy)
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1))


def style_ints(style):
    """(depth_step, silhouette_scale, crease_scale) as Python integers."""
    if isinstance(style, np.ndarray):
        s = style.reshape(-1)[0]
        return int(s["depth_step"]), int(s["silhouette_scale"]), int(s["crease_scale"])
    d, s, c = style
    return int(d), int(s), int(c)


def background_word(params):
    bg = int(params.background)
    return bg | bg << 8 | bg << 16


def words(gbuf, width):
    """(rows, width, 7) uint32 view of a G-buffer block."""
    return np.ascontiguousarray(gbuf).view(np.uint32).reshape(-1, width, 7)


def covered(params, gbuf):
    """Flat bool array: the texel differs from the background texel."""
    w = np.ascontiguousarray(gbuf).view(np.uint32).reshape(-1, 7).copy()
    w[:, 3] ^= np.uint32(background_word(params))
    return w.any(axis=1)


def _shift(a, dx, dy):
    """a[y + dy, x + dx] at [y, x] (np.roll: what wraps round is masked by `present`)."""
    return np.roll(np.roll(a, -dy, axis=0), -dx, axis=1)


def classes(params, style, gbuf, grows, rows):
    """Flat uint8 array of the classes of rows `rows`: 2 silhouette, 1 crease, 0 neither."""
    step, _, _ = style_ints(style)
    W = params.width
    g0, g1 = grows
    r0, r1 = rows
    assert 0 <= g0 <= r0 < r1 <= g1 <= params.height and len(gbuf) == (g1 - g0) * W
    w = words(gbuf, W)
    cov = (w[..., 0] | w[..., 1] | w[..., 2] | (w[..., 3] ^ np.uint32(background_word(params))) | w[..., 4] | w[..., 5]
           | w[..., 6]) != 0
    key = w[..., 4] - w[..., 5]  # uint32: wraps
    ent = w[..., 6]
    ys, xs = np.meshgrid(np.arange(g0, g1), np.arange(W), indexing="ij")

    def against(dx, dy):
        """(present, the pixel meets the silhouette condition against that neighbour, the neighbour meets it against the
        pixel, the neighbour is covered, its normal words differ)."""
        present = (xs + dx >= 0) & (xs + dx < W) & (ys + dy >= max(0, g0)) & (ys + dy < min(params.height, g1))
        n_cov, n_key, n_ent = _shift(cov, dx, dy), _shift(key, dx, dy), _shift(ent, dx, dy)
        other = n_ent != ent
        mine = ~n_cov | (other & ((key - n_key).view(np.int32) >= step))
        theirs = other & ((n_key - key).view(np.int32) >= step)
        differ = np.zeros_like(cov)
        for k in range(3):
            differ |= _shift(w[..., k], dx, dy) != w[..., k]
        return present, mine, theirs, n_cov, differ

    sil = np.zeros_like(cov)
    crease = np.zeros_like(cov)
    for dx, dy in NEIGHBOURS:
        present, mine, theirs, n_cov, differ = against(dx, dy)
        sil |= present & mine
        if (dx, dy) in ((1, 0), (0, 1)):
            crease |= present & n_cov & ~theirs & differ
    sil &= cov
    crease &= cov & ~sil
    cls = np.where(sil, 2, np.where(crease, 1, 0)).astype(np.uint8)
    return cls[r0 - g0:r1 - g0].reshape(-1)


def apply_scale(style, cls, fb):
    """fb_out: each of red, green, blue min(255, (c * s) >> 8) with s by class; alpha passes through."""
    _, s_sil, s_crease = style_ints(style)
    s = np.where(cls == 2, s_sil, np.where(cls == 1, s_crease, 256)).astype(np.int64)
    out = fb.copy()
    for ch in CHANNELS:
        out[ch] = np.minimum(255, (fb[ch].astype(np.int64) * s) >> 8).astype(np.uint8)
    return out


def model(params, style, gbuf, grows, fb, rows):
    """(edge, fb_out) of rows `rows`; fb None gives fb_out None."""
    cls = classes(params, style, gbuf, grows, rows)
    assert fb is None or len(fb) == len(cls)
    return cls, (None if fb is None else apply_scale(style, cls, fb))


def model_loop(params, style, gbuf, grows, fb, rows):
    """`model`, one pixel and one neighbour at a time in Python integers."""
    step, s_sil, s_crease = style_ints(style)
    W, H = params.width, params.height
    g0, g1 = grows
    r0, r1 = rows
    w = [[int(v) for v in t] for t in np.ascontiguousarray(gbuf).view(np.uint32).reshape(-1, 7)]
    bgw = background_word(params)
    background = [0, 0, 0, bgw, 0, 0, 0]

    def texel(x, y):
        return w[(y - g0) * W + x]

    def cov(t):
        return t != background

    def d(t, n):
        v = ((t[4] - t[5]) - (n[4] - n[5])) & M32
        return v - (1 << 32) if v >= 1 << 31 else v

    def meets(t, n):
        """t meets the silhouette condition against its present neighbour n"""
        return (not cov(n)) or (n[6] != t[6] and d(t, n) >= step)

    edge = np.zeros((r1 - r0) * W, dtype=np.uint8)
    out = None if fb is None else fb.copy()
    for y in range(r0, r1):
        for x in range(W):
            t = texel(x, y)
            present = []
            for dx, dy in NEIGHBOURS:
                nx, ny = x + dx, y + dy
                ok = 0 <= nx < W and max(0, g0) <= ny < min(H, g1)
                present.append(texel(nx, ny) if ok else None)
            c = 0
            if cov(t):
                if any(n is not None and meets(t, n) for n in present):
                    c = 2
                else:
                    for n in (present[1], present[3]):  # right, down
                        if n is not None and cov(n) and not meets(n, t) and n[:3] != t[:3]:
                            c = 1
            i = (y - r0) * W + x
            edge[i] = c
            if out is not None:
                s = s_sil if c == 2 else (s_crease if c == 1 else 256)
                for ch in CHANNELS:
                    out[ch][i] = min(255, (int(fb[ch][i]) * s) >> 8)
    return edge, out


def block(plane, width, rows, of=None):
    """Rows `rows` of a flat plane that holds rows `of` (default: from row 0)."""
    base = 0 if of is None else of[0]
    return plane[(rows[0] - base) * width:(rows[1] - base) * width]


def halo(rows, height):
    """The G-buffer rows a caller that shades rows `rows` passes: one more on each side that exists."""
    return max(0, rows[0] - 1), min(height, rows[1] + 1)


def random_colors(T, rng, n):
    return rng.integers(0, 256, 4 * n, dtype=np.uint8).view(T.COLOR)


def random_texels(T, rng, params, n):
    """Texels in which every clause of the contract is met often: a tenth background, two entities, keys a few steps
    apart, normals out of a small set that holds -0.0 and +0.0."""
    g = np.zeros(n, dtype=T.PIXEL)
    w = g.view(np.uint32).reshape(n, 7)
    normals = np.array([0x00000000, 0x80000000, 0x3F800000, 0xBF800000], dtype=np.uint32)
    for k in range(3):
        w[:, k] = normals[rng.integers(0, 4, n)]
    w[:, 3] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    w[:, 4] = rng.integers(0, 4, n).astype(np.uint32)
    w[:, 5] = rng.integers(0, 4, n).astype(np.uint32)
    w[:, 6] = rng.integers(0, 2, n).astype(np.uint32)
    bg = rng.integers(0, 10, n) == 0
    w[bg] = np.array([0, 0, 0, background_word(params), 0, 0, 0], dtype=np.uint32)
    return g


# ---- carved device planes (GPU tests) --------------------------------------------------------------------------------

GUARD = 0xEE
PAD = 256  # guard bytes before and after every carved plane


class Carved:
    """A device plane of `nbytes` bytes that starts `shift` bytes past a 16-byte boundary, inside a guard-filled tensor."""

    def __init__(self, nbytes, shift, content=None):
        import torch
        self.t = torch.full((nbytes + 2 * PAD + 16,), GUARD, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.at, self.nbytes = PAD + shift, nbytes
        self.ptr = self.t.data_ptr() + self.at
        assert self.ptr % 16 == shift % 16
        if content is not None:
            self.t[self.at:self.at + nbytes] = torch.from_numpy(np.ascontiguousarray(content).view(np.uint8).copy()).cuda()

    def host(self, dtype):
        return self.t[self.at:self.at + self.nbytes].cpu().numpy().view(dtype)

    def guards_intact(self):
        h = self.t.cpu().numpy()
        return bool((h[:self.at] == GUARD).all() and (h[self.at + self.nbytes:] == GUARD).all())


def run(par, T, params, style, gbuf, grows, fb, rows, want=("edge", "fb"), in_place=False, shifts=(0, 0, 0, 0)):
    """One par_outline_device call on carved device planes: {"edge": ..., "fb": ...} for the planes asked for, the
    source frame and the G-buffer as they are afterwards under "src" and "gbuf", with every guard byte checked.
    shifts: BYTES past a 16-byte boundary of gbuf, fb, fb_out and edge_out."""
    import torch
    n = (rows[1] - rows[0]) * params.width
    assert fb is None or len(fb) == n
    g = Carved(28 * len(gbuf), shifts[0], gbuf)
    src = Carved(4 * n, shifts[1], fb) if fb is not None else None
    dst = src if in_place else (Carved(4 * n, shifts[2]) if "fb" in want else None)
    edge = Carved(n, shifts[3]) if "edge" in want else None
    torch.cuda.synchronize()
    par.outline(params, style, g.ptr, grows, src.ptr if src else None, rows, fb_out=dst.ptr if dst else None,
                edge_out=edge.ptr if edge else None)
    torch.cuda.synchronize()
    for name, plane in (("gbuf", g), ("fb", src), ("fb_out", dst), ("edge_out", edge)):
        assert plane is None or plane.guards_intact(), f"{name}: bytes outside the plane were written"
    out = {"gbuf": g.host(T.PIXEL)}
    if src is not None:
        out["src"] = src.host(T.COLOR)
    if dst is not None:
        out["fb"] = dst.host(T.COLOR)
    if edge is not None:
        out["edge"] = edge.host(np.uint8)
    return out


def check(got, gbuf, fb, exp_edge, exp_fb, tag, in_place=False):
    if "edge" in got:
        bad = np.nonzero(got["edge"] != exp_edge)[0]
        assert len(bad) == 0, f"{tag}: edge_out differs at {len(bad)} pixels, first {bad[:4]}: {got['edge'][bad[:4]]} for {exp_edge[bad[:4]]}"
    if "fb" in got:
        bad = np.nonzero(got["fb"].view(np.uint32) != exp_fb.view(np.uint32))[0]
        assert len(bad) == 0, f"{tag}: fb_out differs at {len(bad)} pixels, first {bad[:4]}"
    assert got["gbuf"].tobytes() == gbuf.tobytes(), f"{tag}: the G-buffer was written"
    if not in_place and "src" in got:
        assert got["src"].tobytes() == fb.tobytes(), f"{tag}: the source was written"
