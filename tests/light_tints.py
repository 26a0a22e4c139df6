"""Tinted lights (par_set_light_tints) restated on the host: the expected frame composed in numpy float32 from the pinned
oracle's per-light planes, built on test_gpu_lights.compose (unbounded lights) and light_range.compose_ranged (ranged
ones), which give every plane the tints do not touch and the lights that add to a pixel; and the same contract for one
pixel without arrays."""
import numpy as np

WHITE = (1.0, 1.0, 1.0)
CHANNELS = ("red", "green", "blue")


def tint_rows(tints, n):
    """The tints of lights 0 .. n-1 as float32 triples: `tints` (a LIGHT_TINT array or rows of (r, g, b)) goes by light
    index, the lights it does not name are white."""
    f32 = np.float32
    rows = []
    for t in tints:
        names = getattr(getattr(t, "dtype", None), "names", None)
        rows.append(tuple(f32(t[k]) for k in "rgb") if names else tuple(f32(v) for v in t))
    rows += [tuple(f32(v) for v in WHITE)] * max(0, n - len(rows))
    return rows[:n]


def light_terms(params, outs, lights, ranged):
    """Per light, over the covered pixels: the term the untinted sum would add (d_l, or d_l * w_l rounded for a ranged
    light) and whether it is added (lit, and in range or unbounded). The lit plane and the covered pixels' indices come
    from the composers this builds on."""
    from light_range import compose_ranged
    from test_gpu_lights import compose
    if ranged:
        exp, per_light, idx, rays = compose_ranged(params, outs, lights)
        on = [in_range & lit for in_range, lit in per_light]
    else:
        exp, per_light = compose(params, outs, lights)
        idx = np.nonzero(outs[0]["palidx"] != 0xFF)[0]
        on = list(per_light)
        rays = len(lights) * len(idx)
    W = params.width
    gbuf = outs[0]["gbuf"]
    x = (idx % W).astype(np.int64)
    y = gbuf["y"][idx].astype(np.int64)
    z = gbuf["z"][idx].astype(np.int64)
    n = gbuf["normal"][idx]
    f32 = np.float32
    terms = []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):  # (normals may be anything: inf, NaN, 3e38)
        for L in lights:
            dx = (int(L["x"]) - x).astype(f32)
            dy = (int(L["y"]) - y).astype(f32)
            dz = (int(L["z"]) - z).astype(f32)
            length = (np.abs(dx) + np.abs(dy)) + np.abs(dz)
            dot = (n["x"] * (dx / length) + n["y"] * (dy / length)) + n["z"] * (dz / length)
            d = np.where(f32(0) < dot, dot, f32(0))
            r = int(L["radius"])
            if ranged and r > 0:
                d = d * (f32(1) - length / f32(r))  # (the weight, then the product, each rounded)
            terms.append(d.astype(f32))
    return exp, idx, terms, on, rays


def compose_tinted(params, outs, lights, tints, ranged):
    """The contract of par_set_light_tints in numpy float32. Returns the expected planes and what a test's conditions on
    its inputs need: the covered pixels' indices, their three factors, each light's added term (0 where it adds
    nothing) and the (covered pixel, light) pairs that count as shadow rays."""
    exp, idx, terms, on, rays = light_terms(params, outs, lights, ranged)
    f32 = np.float32
    rows = tint_rows(tints, len(lights))
    sums = [np.zeros(len(idx), dtype=f32) for _ in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(len(lights)):
            for c in range(3):
                sums[c] = np.where(on[l], sums[c] + terms[l] * rows[l][c], sums[c])  # product rounded, then added
        factors = []
        for c in range(3):
            b = sums[c] + f32(params.ambient)
            factors.append(np.where(b < f32(1), b, f32(1)))  # std::min<float>(1, s_c + ambient)
    col = outs[0]["gbuf"]["color"][idx]
    fb = exp["fb"].copy()
    for c, ch in enumerate(CHANNELS):
        fb[ch][idx] = (col[ch].astype(f32) * factors[c]).astype(np.uint8)  # Color::operator*, truncating, per channel
    fb["alpha"][idx] = col["alpha"]
    m = np.where(factors[0] < factors[1], factors[1], factors[0])  # std::max(std::max(b_r, b_g), b_b)
    m = np.where(m < factors[2], factors[2], m)
    brightness = exp["brightness"].copy()
    brightness[idx] = m
    out = dict(exp, fb=fb, brightness=brightness)
    info = {"idx": idx, "factors": factors, "rays": rays, "tints": rows,
            "added": [np.where(on[l], terms[l], f32(0)) for l in range(len(lights))], "on": on}
    return out, info


def scalar_pixel(params, outs, lights, tints, ranged, p):
    """One covered pixel of the same contract without numpy arrays: ((b_r, b_g, b_b), brightness, lit bits), float32."""
    f32 = np.float32
    assert outs[0]["palidx"][p] != 0xFF
    g = outs[0]["gbuf"][p]
    x, y, z = p % params.width, int(g["y"]), int(g["z"])
    nx, ny, nz = (f32(g["normal"][k]) for k in ("x", "y", "z"))
    rows = tint_rows(tints, len(lights))
    s = [f32(0), f32(0), f32(0)]
    bits = 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for l, L in enumerate(lights):
            r = int(L["radius"]) if ranged else 0
            dx, dy, dz = f32(int(L["x"]) - x), f32(int(L["y"]) - y), f32(int(L["z"]) - z)
            ln = f32(f32(abs(dx) + abs(dy)) + abs(dz))
            if r > 0 and not ln < f32(r):
                continue
            if outs[l]["lit"][p] == 0:
                continue
            dot = f32(f32(f32(nx * f32(dx / ln)) + f32(ny * f32(dy / ln))) + f32(nz * f32(dz / ln)))
            t = dot if f32(0) < dot else f32(0)
            if r > 0:
                t = f32(t * f32(f32(1) - f32(ln / f32(r))))
            for c in range(3):
                s[c] = f32(s[c] + f32(t * rows[l][c]))
            bits |= 1 << l
        b = []
        for c in range(3):
            v = f32(s[c] + f32(params.ambient))
            b.append(v if v < f32(1) else f32(1))
    m = b[1] if b[0] < b[1] else b[0]
    m = b[2] if m < b[2] else m
    return tuple(b), m, bits


def conditions(exp, info, lights, black=None):
    """What a tinted frame must show for its test to mean something (counts; the caller asserts them positive):
    covered pixels with red != green and with green != blue, pixels with one channel's factor clamped at 1 and another
    below 1, pixels where at least two non-black lights add a positive term, and covered pixels with the lit bit of the
    black light `black` set."""
    idx = info["idx"]
    fb = exp["fb"][idx]
    fr, fg, fb_ = info["factors"]
    one = np.float32(1)
    clamped = (fr == one).astype(int) + (fg == one) + (fb_ == one)
    adding = np.zeros(len(idx), dtype=int)
    for l in range(len(lights)):
        if any(v > 0 for v in info["tints"][l]):
            adding += info["added"][l] > 0
    out = {"r!=g": int((fb["red"] != fb["green"]).sum()), "g!=b": int((fb["green"] != fb["blue"]).sum()),
           "clamped in some, not all": int(((clamped > 0) & (clamped < 3)).sum()), "two adding": int((adding >= 2).sum())}
    if black is not None:
        assert all(v == 0 for v in info["tints"][black])
        out["black lit"] = int(((exp["lit"][idx] >> black) & 1).sum())
    return out
