"""Fitted palettes (par_palette_*_device, par_palette_fit_host) restated on the host: the contract beside the
declarations in include/par_raytracer.h in numpy and Python integers. Every function works from and to a work block, a
1-element array of types.PALETTE_WORK (`new_work`), and changes exactly the fields the device call changes.
tests/test_palette_cpu.py holds `cut` to a per-cell loop and `emit` to Python big integers without a GPU."""
import numpy as np

AXES = 3  # red, green, blue: a cell is red | green << 5 | blue << 10, so hist.reshape(32, 32, 32) is [blue][green][red]
MASK64 = (1 << 64) - 1


def new_work(T):
    return np.zeros(1, dtype=T.PALETTE_WORK)


def cells(fb):
    return ((fb["red"].astype(np.int64) >> 3) | ((fb["green"].astype(np.int64) >> 3) << 5) |
            ((fb["blue"].astype(np.int64) >> 3) << 10))


def count(work, fb):
    """hist[cell(p)] += 1 for every pixel of `fb`, modulo 2^32."""
    add = np.bincount(cells(fb), minlength=32768).astype(np.uint64)
    work["hist"][0] = ((work["hist"][0].astype(np.uint64) + add) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


class _Region:
    """A box of cells (inclusive ranges lo, hi in the order red, green, blue), its population and its tight bounds."""

    def __init__(self, hist3, lo, hi):
        self.lo, self.hi = list(lo), list(hi)
        sub = hist3[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]  # [blue][green][red]
        self.n = int(sub.sum(dtype=np.uint64))
        self.tlo, self.thi = [0] * AXES, [0] * AXES
        # the population per coordinate on each axis, as Python integers
        self.marginal = []
        for axis in range(AXES):
            m = sub.sum(axis=tuple(a for a in range(3) if a != 2 - axis), dtype=np.uint64)
            at = np.nonzero(sub.max(axis=tuple(a for a in range(3) if a != 2 - axis)))[0]
            self.tlo[axis], self.thi[axis] = lo[axis] + int(at[0]), lo[axis] + int(at[-1])
            self.marginal.append({lo[axis] + v: int(c) for v, c in enumerate(m)})
        self.extent = max(h - l for l, h in zip(self.tlo, self.thi))


def cut_regions(hist, n_colors):
    """The regions of the cut as a list of (lo, hi), in index order; [] when every count is 0."""
    hist3 = np.asarray(hist, dtype=np.uint32).reshape(32, 32, 32)
    if not hist3.any():
        return []
    regions = [_Region(hist3, (0, 0, 0), (31, 31, 31))]
    while len(regions) < n_colors:
        best = None
        for k, r in enumerate(regions):  # the largest extent >= 1, then the larger population, then the lower index
            if r.extent >= 1 and (best is None or (r.extent, r.n) > (regions[best].extent, regions[best].n)):
                best = k
        if best is None:
            break
        r = regions[best]
        axis = [h - l for l, h in zip(r.tlo, r.thi)].index(r.extent)
        lo, hi = r.tlo[axis], r.thi[axis]
        s, cum = hi - 1, 0
        for v in range(lo, hi):
            cum += r.marginal[axis][v]
            if 2 * cum >= r.n:
                s = v
                break
        left_hi, right_lo = list(r.hi), list(r.lo)
        left_hi[axis], right_lo[axis] = s, s + 1
        regions[best] = _Region(hist3, r.lo, left_hi)
        regions.append(_Region(hist3, right_lo, r.hi))
    return [(tuple(r.lo), tuple(r.hi)) for r in regions]


def cut(work, n_colors):
    """Writes all of lut and n_entries and zeroes sums; hist and reserved stay."""
    regions = cut_regions(work["hist"][0], n_colors)
    lut3 = np.zeros((32, 32, 32), dtype=np.uint8)
    for k, (lo, hi) in enumerate(regions):
        lut3[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = k
    work["lut"][0] = lut3.reshape(-1)
    work["n_entries"][0] = len(regions)
    work["sums"][0] = 0


def sums(work, fb):
    """sums[lut[cell(p)]] += {red, green, blue, 1} for every pixel of `fb`, modulo 2^64."""
    entry = work["lut"][0][cells(fb)].astype(np.int64)
    add = np.zeros((256, 4), dtype=np.uint64)
    assert len(fb) < 1 << 40  # (the weighted bincount sums in float64: exact below 2^53)
    for j, ch in enumerate(("red", "green", "blue")):
        add[:, j] = np.bincount(entry, weights=fb[ch].astype(np.float64), minlength=256).astype(np.uint64)
    add[:, 3] = np.bincount(entry, minlength=256).astype(np.uint64)
    work["sums"][0] = work["sums"][0] + add  # uint64 arithmetic wraps


def emit(T, work, n_colors):
    """The n_colors entries par_palette_emit_device writes, as a COLOR array."""
    out = np.zeros(n_colors, dtype=T.COLOR)
    m = min(int(work["n_entries"][0]), n_colors)
    s = work["sums"][0]
    for k in range(n_colors):
        if m <= 0:
            continue
        row = s[k if k < m else 0]
        n = int(row[3])
        if n > 0:
            assert n < 1 << 63  # (2 * n_k is formed in uint64)
            ch = [(((2 * int(row[c]) + n) & MASK64) // (2 * n)) & 0xFF for c in range(3)]
            out[k] = (ch[0], ch[1], ch[2], 255)
    return out


def fit(T, fb, n_colors):
    """reset, count, cut, sums, emit of one frame: (palette, n_entries, work)."""
    work = new_work(T)
    count(work, fb)
    cut(work, n_colors)
    sums(work, fb)
    return emit(T, work, n_colors), int(work["n_entries"][0]), work
