"""Ranged lights (PAR_LIGHTS_RANGED, par_set_light_model) restated on the host: the slab of csrc/par_lightbox.h that the
light kernel culls (start bin, light) pairs by, the pair counts of a frame, and the expected frame composed from the
pinned oracle (test_gpu_lights.compose extended by the contract beside par_set_light_model)."""
import numpy as np

LIGHT_NB = 64  # PAR_LIGHT_NB: occupied bins of a column whose walks the light kernel records


def light_slab(B, H, bx, by, bz):
    """(x0, x1, s0, s1, z0, z1), inclusive, s = y + z: where a pixel of screen column (bx, by) that starts in depth bin
    bz can lie."""
    z0 = -(B - 1) if bz == 0 else bz * B  # (C division truncates: bin 0 also holds -B < z < 0)
    return bx * B, bx * B + B - 1, H - by * B - B + 1, H - by * B, z0, bz * B + B - 1


def gap(v, lo, hi):
    return lo - v if v < lo else (v - hi if v > hi else 0)


def slab_l1(slab, lx, ly, lz):
    """The L1 distance in (x, y, z) from the light to the slab's nearest integer point."""
    x0, x1, s0, s1, z0, z1 = slab
    w = min(max(0, z0 - lz), z1 - lz)  # the z offset nearest to 0
    return gap(lx, x0, x1) + abs(w) + gap(w, s0 - ly - lz, s1 - ly - lz)


def slab_clip(slab, e, dmin, dmax):
    """The part of the slab that slot record e = (px, py, pz, ex, ey, ez) can show with sprite depths in [dmin, dmax],
    or None."""
    px, py, pz, ex, ey, ez = e
    x0, x1, s0, s1, z0, z1 = slab
    c = (max(px, x0), min(px + ex - 1, x1), max(py + pz + 1, s0), min(py + ey + pz + ez, s1), max(pz + dmin, z0),
         min(pz + dmax, z1))
    return c if c[0] <= c[1] and c[2] <= c[3] and c[4] <= c[5] else None


def pair_culled(B, H, bx, by, bz, light, radius, records=None, depths=(0, 0)):
    """The light kernel's range cull of pair ((bx, by, bz), light): by the bin alone, then (`records`: the slot records
    of the column's bins, or None when the column has more occupied bins than the kernel lists) by what they can show."""
    if radius <= 0:
        return False
    slab = light_slab(B, H, bx, by, bz)
    if slab_l1(slab, *light) >= radius:
        return True
    if records is None:
        return False
    pieces = (slab_clip(slab, e, *depths) for e in records)
    return all(c is None or slab_l1(c, *light) >= radius for c in pieces)


def depth_range(sprites):
    return int(sprites["depth"].min()), int(sprites["depth"].max())


def pair_counts(params, count, bins, lights, depths, rows=None):
    """(pairs, culled) of a frame: (start bin, light) pairs of the recorded occupied bins of the columns the frame
    renders, and how many of them the kernel culls. `count`, `bins`: the hash in the reference's layout (bin counts in
    flat (x, y, z) order, eight slots per bin); `depths`: depth_range of the sprite table."""
    gx, gy, gz = params.grid_dims()
    B, H = params.bin_size, params.height
    r0, r1 = rows or (0, H)
    c = np.asarray(count).reshape(gx, gy, gz)
    slots = np.asarray(bins).reshape(gx, gy, gz, -1)
    pairs = culled = 0
    for bx in range(gx):
        for by in range(r0 // B, (r1 - 1) // B + 1):
            occ = np.nonzero(c[bx, by])[0]
            assert len(occ) <= LIGHT_NB, "the pair counts are deterministic only while every occupied bin is recorded"
            records = [tuple(int(slots[bx, by, z, k][f]) for f in ("px", "py", "pz", "ex", "ey", "ez"))
                       for z in occ for k in range(int(c[bx, by, z]))]
            for bz in occ:
                for L in lights:
                    pairs += 1
                    culled += bool(pair_culled(B, H, bx, by, int(bz), (int(L["x"]), int(L["y"]), int(L["z"])),
                                               int(L["radius"]), records, depths))
    return pairs, culled


def l1_length(L, x, y, z):
    """len of the contract in float32: (|dx| + |dy|) + |dz| of the fp32 differences."""
    f32 = np.float32
    dx = (int(L["x"]) - x).astype(f32)
    dy = (int(L["y"]) - y).astype(f32)
    dz = (int(L["z"]) - z).astype(f32)
    return (np.abs(dx) + np.abs(dy)) + np.abs(dz)


def compose_ranged(params, outs, lights):
    """The contract of PAR_LIGHTS_RANGED in numpy float32 from the oracle's per-light planes (as test_gpu_lights.compose
    takes them). Returns the expected planes and, per light, (in range, lit) over the covered pixels, the covered
    pixels' indices, and the (covered pixel, light) pairs that are in range or unbounded."""
    from test_gpu_lights import compose
    exp, _ = compose(params, outs, lights)  # the planes the lights do not touch, and the background's fb / brightness
    base = outs[0]
    W = params.width
    gbuf = base["gbuf"]
    covered = base["palidx"] != 0xFF
    idx = np.nonzero(covered)[0]
    x = (idx % W).astype(np.int64)
    y = gbuf["y"][idx].astype(np.int64)
    z = gbuf["z"][idx].astype(np.int64)
    n = gbuf["normal"][idx]
    f32 = np.float32
    s = np.zeros(len(idx), dtype=f32)
    lit = np.zeros(len(gbuf), dtype=np.uint8)
    bg = np.nonzero(~covered)[0]
    bgx = (bg % W).astype(np.int64)
    zero = np.zeros(len(bg), dtype=np.int64)
    per_light, rays = [], 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):  # (normals may be anything: inf, NaN, 3e38)
        for l, L in enumerate(lights):
            r = int(L["radius"])
            dx = (int(L["x"]) - x).astype(f32)
            dy = (int(L["y"]) - y).astype(f32)
            dz = (int(L["z"]) - z).astype(f32)
            length = (np.abs(dx) + np.abs(dy)) + np.abs(dz)
            tx, ty, tz = dx / length, dy / length, dz / length
            dot = (n["x"] * tx + n["y"] * ty) + n["z"] * tz
            d = np.where(f32(0) < dot, dot, f32(0))
            lit_l = outs[l]["lit"] != 0
            if r > 0:
                in_range = length < f32(r)
                w = f32(1) - length / f32(r)
                term = d * w                                   # rounded, then added
                bg_in = l1_length(L, bgx, zero, zero) < f32(r)
            else:
                in_range = np.ones(len(idx), dtype=bool)
                term = d
                bg_in = np.ones(len(bg), dtype=bool)
            on = in_range & lit_l[idx]
            s = np.where(on, s + term, s)
            bits = np.zeros(len(gbuf), dtype=bool)
            bits[idx] = on
            bits[bg] = bg_in & lit_l[bg]
            lit |= (bits.astype(np.uint8) << l)
            per_light.append((in_range, lit_l[idx]))
            rays += int(in_range.sum())
        b = s + f32(params.ambient)
        bright = np.where(b < f32(1), b, f32(1))
    fb = exp["fb"].copy()
    col = gbuf["color"][idx]
    for ch in ("red", "green", "blue"):
        fb[ch][idx] = (col[ch].astype(f32) * bright).astype(np.uint8)
    brightness = exp["brightness"].copy()
    brightness[idx] = bright
    out = dict(exp, fb=fb, brightness=brightness, lit=lit)
    return out, per_light, idx, rays


def scalar_pixel(params, outs, lights, p):
    """One pixel of the same contract without numpy arrays: (brightness as float32, lit bits)."""
    f32 = np.float32
    g = outs[0]["gbuf"][p]
    x = p % params.width
    if outs[0]["palidx"][p] == 0xFF:
        bits = 0
        for l, L in enumerate(lights):
            r = int(L["radius"])
            ln = f32(f32(abs(f32(int(L["x"]) - x)) + abs(f32(int(L["y"])))) + abs(f32(int(L["z"]))))
            if (r <= 0 or ln < f32(r)) and outs[l]["lit"][p] != 0:
                bits |= 1 << l
        return None, bits
    y, z = int(g["y"]), int(g["z"])
    nx, ny, nz = (f32(g["normal"][k]) for k in ("x", "y", "z"))
    s, bits = f32(0), 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for l, L in enumerate(lights):
            r = int(L["radius"])
            dx, dy, dz = f32(int(L["x"]) - x), f32(int(L["y"]) - y), f32(int(L["z"]) - z)
            ln = f32(f32(abs(dx) + abs(dy)) + abs(dz))
            if r > 0 and not ln < f32(r):
                continue
            if outs[l]["lit"][p] == 0:
                continue
            dot = f32(f32(f32(nx * f32(dx / ln)) + f32(ny * f32(dy / ln))) + f32(nz * f32(dz / ln)))
            d = dot if f32(0) < dot else f32(0)
            if r > 0:
                d = f32(d * f32(f32(1) - f32(ln / f32(r))))
            s = f32(s + d)
            bits |= 1 << l
        b = f32(s + f32(params.ambient))
    return (b if b < f32(1) else f32(1)), bits
