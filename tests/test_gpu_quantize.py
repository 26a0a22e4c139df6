"""GPU tests of palette output (par_quantize_device, par_quantize_host): every index plane and every quantised frame byte
for byte against the contract restated in numpy (quantize.model; tests/test_quantize_cpu.py holds it to a per-pixel loop
without a GPU). The shapes are the smallest at which each mechanism of the kernel can go wrong, not the workload's.

Each case first asserts on the host, from the model, that its inputs reach the situation it is named for.

Shapes of case 1: a frame of 64 x 16 has no rows (5, 18), so that shape is run both ways round: 64 wide and 16 high with
the whole frame and rows (5, 16), 16 wide and 64 high with the whole frame and rows (5, 18); 37 x 23 as it stands."""
import numpy as np
import pytest

import quantize as Q

pytestmark = pytest.mark.gpu

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


def run(par, T, params, palette, fb, rows, spread, want=("index", "fb"), in_place=False, shifts=(0, 0, 0)):
    """One par_quantize_device call on carved device planes: ({"index": ..., "fb": ...} for the planes asked for, and the
    source as it is afterwards under "src"), with every guard byte checked. shifts: elements past a 16-byte boundary of
    the source, fb_out and index_out."""
    import torch
    r0, r1 = rows or (0, params.height)
    n = (r1 - r0) * params.width
    assert len(fb) == n
    d_pal = torch.from_numpy(palette.view(np.uint8).copy()).cuda()
    src = Carved(4 * n, 4 * shifts[0], fb)
    dst = src if in_place else (Carved(4 * n, 4 * shifts[1]) if "fb" in want else None)
    idx = Carved(n, shifts[2]) if "index" in want else None
    torch.cuda.synchronize()
    par.quantize(params, d_pal.data_ptr(), len(palette), src.ptr, (r0, r1), fb_out=dst.ptr if dst else None,
                 index_out=idx.ptr if idx else None, spread=spread)
    torch.cuda.synchronize()
    out = {"src": src.host(T.COLOR)}
    for name, plane in (("source", src), ("fb_out", dst), ("index_out", idx)):
        assert plane is None or plane.guards_intact(), f"{name}: bytes outside the plane were written"
    if dst is not None:
        out["fb"] = dst.host(T.COLOR)
    if idx is not None:
        out["index"] = idx.host(np.uint8)
    return out


def check(got, fb, exp_index, exp_fb, tag, in_place=False):
    if "index" in got:
        bad = np.nonzero(got["index"] != exp_index)[0]
        assert len(bad) == 0, f"{tag}: index differs at {len(bad)} pixels, first {bad[:4]}"
    if "fb" in got:
        bad = np.nonzero(got["fb"].view(np.uint32) != exp_fb.view(np.uint32))[0]
        assert len(bad) == 0, f"{tag}: fb_out differs at {len(bad)} pixels, first {bad[:4]}"
    if not in_place:
        assert got["src"].tobytes() == fb.tobytes(), f"{tag}: the source was written"


# ---- 1. shapes and palette sizes ----------------------------------------------------------------------------------

N_COLORS = [1, 2, 15, 16, 17, 255, 256]
SPREADS = [0, 1, 37, 255]
OUTPUTS = [(("index", "fb"), False), (("index",), False), (("fb",), False), (("fb",), True)]
# (width, height, rows)
SHAPES = [(37, 23, None), (37, 23, (5, 18)), (64, 16, None), (64, 16, (5, 16)), (16, 64, None), (16, 64, (5, 18))]


def case1_inputs(T, w, h, rows, n_colors):
    rng = np.random.default_rng(1000 * w + n_colors)
    params = T.default_params(w, h)
    r0, r1 = rows or (0, h)
    return params, Q.random_colors(T, rng, n_colors), Q.random_colors(T, rng, (r1 - r0) * w)


@pytest.mark.parametrize("w,h,rows", SHAPES)
def test_shapes_and_palette_sizes(par, T, w, h, rows):
    assert (37 * 23) % 4 != 0
    for n_colors in N_COLORS:
        params, palette, fb = case1_inputs(T, w, h, rows, n_colors)
        for spread in SPREADS:
            exp_index, exp_fb = Q.model(params, palette, fb, rows, spread)
            if n_colors > 1:
                assert len(np.unique(exp_index)) > 1, "the inputs should use more than one entry"
            for want, in_place in OUTPUTS:
                tag = f"{w}x{h} rows {rows} n_colors {n_colors} spread {spread} {want} in place {in_place}"
                check(run(par, T, params, palette, fb, rows, spread, want, in_place), fb, exp_index, exp_fb, tag, in_place)
    # the odd first row shows in the dither: the same block taken for rows (4, ...) would come out differently
    if rows is not None:
        params, palette, fb = case1_inputs(T, w, h, rows, 17)
        other = Q.model(params, palette, fb, (rows[0] - 1, rows[1] - 1), 37)[0]
        assert (other != Q.model(params, palette, fb, rows, 37)[0]).any()


# ---- 2. alignment and bounds ----------------------------------------------------------------------------------------

def test_alignment_and_bounds(par, T):
    """The three planes at every 16-byte phase, independently: exact results whichever path the kernel takes, and no
    byte outside a plane written (run checks the guards round all of them)."""
    rng = np.random.default_rng(2)
    params = T.default_params(37, 23)
    palette, fb = Q.random_colors(T, rng, 17), Q.random_colors(T, rng, 37 * 23)
    exp_index, exp_fb = Q.model(params, palette, fb, None, 37)
    exp_index0, exp_fb0 = Q.model(params, palette, fb, None, 0)
    for s in range(4):
        for f in range(4):
            for i in range(4):
                got = run(par, T, params, palette, fb, None, 37, shifts=(s, f, i))
                check(got, fb, exp_index, exp_fb, f"source +{s}, fb_out +{f}, index_out +{i}")
        for i in range(4):
            got = run(par, T, params, palette, fb, None, 0, want=("index",), shifts=(s, 0, i))
            check(got, fb, exp_index0, exp_fb0, f"source +{s}, index_out +{i}, index only")
            got = run(par, T, params, palette, fb, None, 37, want=("index", "fb"), in_place=True, shifts=(s, s, i))
            check(got, fb, exp_index, exp_fb, f"source +{s} in place, index_out +{i}", in_place=True)
    # a block of rows: the planes of rows (5, 18) at odd phases
    blk = fb[5 * 37:18 * 37]
    e_index, e_fb = Q.model(params, palette, blk, (5, 18), 37)
    for shifts in ((1, 1, 3), (3, 2, 1), (2, 2, 2)):
        check(run(par, T, params, palette, blk, (5, 18), 37, shifts=shifts), blk, e_index, e_fb, f"rows (5, 18) at {shifts}")


# ---- 3. ties ---------------------------------------------------------------------------------------------------------

def tie_counts(params, palette, fb, spread):
    """Pixels whose smallest distance is reached by (two entries of the same colour, two entries of different colours)."""
    d = Q.distances(params, palette, fb, None, spread)
    best = d.min(axis=1)
    rgb = (palette.view(np.uint32) & 0xFFFFFF).astype(np.int64)
    same = different = 0
    for row, b in zip(d, best):
        at = np.nonzero(row == b)[0]
        if len(at) > 1:
            colours = len(set(rgb[at].tolist()))
            same += colours < len(at)
            different += colours > 1
    return same, different


def colors(T, rows):
    return np.array([tuple(r) for r in rows], dtype=T.COLOR)


TIES = {
    # palette, crafted pixels, the index each crafted pixel must get
    "duplicated entries": ([(200, 0, 0, 1), (90, 90, 90, 2), (0, 200, 0, 3), (90, 90, 90, 4), (90, 90, 90, 5)],
                           [(90, 90, 90, 0), (95, 88, 90, 9), (80, 99, 91, 255)], [1, 1, 1]),
    "along one channel": ([(200, 200, 200, 0), (10, 10, 10, 0), (12, 10, 10, 0)], [(11, 10, 10, 0)], [1]),
    "along one channel, the other way round": ([(200, 200, 200, 0), (12, 10, 10, 0), (10, 10, 10, 0)], [(11, 10, 10, 0)], [1]),
    "across channels": ([(200, 200, 200, 0), (11, 10, 10, 0), (10, 11, 10, 0)], [(10, 10, 10, 0)], [1]),
    "across channels, the other way round": ([(10, 11, 10, 0), (200, 200, 200, 0), (11, 10, 10, 0)], [(10, 10, 10, 0)], [0]),
}


@pytest.mark.parametrize("kind", list(TIES))
def test_ties_go_to_the_lowest_index(par, T, kind):
    entries, crafted, winners = TIES[kind]
    rng = np.random.default_rng(3)
    params = T.default_params(37, 23)
    palette = colors(T, entries)
    fb = Q.random_colors(T, rng, 37 * 23)
    crafted = colors(T, crafted)
    at = rng.choice(len(fb), size=40 * len(crafted), replace=False).reshape(len(crafted), 40)
    for c, where in zip(crafted, at):
        fb[where] = c
    exp_index, exp_fb = Q.model(params, palette, fb, None, 0)
    for where, k in zip(at, winners):
        assert (exp_index[where] == k).all()
    same, different = tie_counts(params, palette, fb, 0)
    if kind == "duplicated entries":
        assert same >= 120, f"{kind}: the model counts {same} tie pixels between equal entries"
    else:
        assert different >= 40, f"{kind}: the model counts {different} tie pixels between different entries"
    check(run(par, T, params, palette, fb, None, 0), fb, exp_index, exp_fb, kind)
    # under the dither the crafted pixels move, and ties fall where they fall: the model says where
    exp_index, exp_fb = Q.model(params, palette, fb, None, 37)
    check(run(par, T, params, palette, fb, None, 37), fb, exp_index, exp_fb, f"{kind}, spread 37")


def test_ties_among_random_entries_of_a_full_palette(par, T):
    rng = np.random.default_rng(33)
    params = T.default_params(37, 23)
    palette = Q.random_colors(T, rng, 256)
    palette[rng.choice(256, 64, replace=False)] = palette[:64]  # 64 duplicates somewhere
    for ch in Q.CHANNELS:
        palette[ch] &= 0xF8  # a coarse lattice: many equidistant pairs
    fb = Q.random_colors(T, rng, 37 * 23)
    same, different = tie_counts(params, palette, fb, 37)
    assert same > 0 and different > 0, (same, different)
    exp_index, exp_fb = Q.model(params, palette, fb, None, 37)
    check(run(par, T, params, palette, fb, None, 37), fb, exp_index, exp_fb, "ties in a full palette")


# ---- 4. key packing --------------------------------------------------------------------------------------------------

def test_key_packing_largest_distance_and_largest_index(par, T):
    """The largest distance (765) beside the largest index (255): d = 764 at index 255 must win over d = 765 at index 0,
    and with every entry black d = 765 at index 0 must win over d = 765 at index 255."""
    rng = np.random.default_rng(4)
    params = T.default_params(37, 23)
    fb = Q.random_colors(T, rng, 37 * 23)
    white = rng.choice(len(fb), 100, replace=False)
    fb[white] = np.array((255, 255, 255, 7), dtype=T.COLOR)
    black = np.zeros(256, dtype=T.COLOR)
    near = black.copy()
    near[255] = np.array((1, 0, 0, 0), dtype=T.COLOR)
    for palette, winner, dist in ((near, 255, 764), (black, 0, 765)):
        d = Q.distances(params, palette, fb, None, 0)
        exp_index, exp_fb = Q.model(params, palette, fb, None, 0)
        assert (exp_index[white] == winner).all() and (d[white].min(axis=1) == dist).all()
        check(run(par, T, params, palette, fb, None, 0), fb, exp_index, exp_fb, f"white pixels to entry {winner}")


# ---- 5. alpha ----------------------------------------------------------------------------------------------------------

def test_alpha_takes_no_part_and_passes_through(par, T):
    rng = np.random.default_rng(5)
    params = T.default_params(37, 23)
    palette = Q.random_colors(T, rng, 16, alpha=(1, 255))
    fb = Q.random_colors(T, rng, 37 * 23)
    assert len(np.unique(fb["alpha"])) > 100 and (palette["alpha"] != 0).all()
    for spread in (0, 37):
        exp_index, exp_fb = Q.model(params, palette, fb, None, spread)
        counted = Q.model(params, palette, fb, None, spread, with_alpha=True)[0]
        assert (counted != exp_index).any(), "alpha counted in the distance should change some pixel"
        assert np.array_equal(exp_fb["alpha"], fb["alpha"])
        got = run(par, T, params, palette, fb, None, spread)
        check(got, fb, exp_index, exp_fb, f"alpha, spread {spread}")
        assert np.array_equal(got["fb"]["alpha"], fb["alpha"])
        got = run(par, T, params, palette, fb, None, spread, want=("fb",), in_place=True)
        check(got, fb, exp_index, exp_fb, f"alpha in place, spread {spread}", in_place=True)


# ---- 6. clamping ---------------------------------------------------------------------------------------------------------

def test_clamping_at_both_ends(par, T):
    rng = np.random.default_rng(6)
    params = T.default_params(37, 23)
    n = 37 * 23
    fb = Q.random_colors(T, rng, n)
    for ch in Q.CHANNELS:  # every channel at 0..3 or 252..255
        fb[ch] = np.where(rng.integers(0, 2, n) == 1, 252, 0) + rng.integers(0, 4, n)
    palette = Q.random_colors(T, rng, 16)
    palette[:6] = colors(T, [(0, 0, 0, 0), (255, 255, 255, 0), (120, 120, 120, 0), (135, 135, 135, 0), (255, 0, 136, 0),
                             (3, 250, 119, 0)])
    _, raw = Q.dithered(params, fb, None, 255)
    assert (raw < 0).sum() > 100 and (raw > 255).sum() > 100, "the inputs should clamp at both ends"
    assert raw.min() == -120 and raw.max() == 255 + 119
    exp_index, exp_fb = Q.model(params, palette, fb, None, 255)
    wrapped = fb.copy()  # what a byte that wraps round instead of clamping would give
    for j, ch in enumerate(Q.CHANNELS):
        wrapped[ch] = (raw[:, j] & 0xFF).astype(np.uint8)
    assert (Q.model(params, palette, wrapped, None, 0)[0] != exp_index).any(), "a missing clamp should show"
    check(run(par, T, params, palette, fb, None, 255), fb, exp_index, exp_fb, "clamping")


# ---- 7. more than one workgroup ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spread", [0, 32])
def test_more_than_one_workgroup(par, T, spread):
    rng = np.random.default_rng(7)
    params = T.default_params(1000, 70)
    palette = par.palette_ramp(T.default_params(), 8)
    assert len(palette) == 33 and 1000 * 70 > 4 * 256 * 8
    fb = Q.random_colors(T, rng, 1000 * 70)
    exp_index, exp_fb = Q.model(params, palette, fb, None, spread)
    assert len(np.unique(exp_index)) > 20
    check(run(par, T, params, palette, fb, None, spread), fb, exp_index, exp_fb, f"1000x70 spread {spread}")
    check(run(par, T, params, palette, fb, None, spread, shifts=(1, 1, 3)), fb, exp_index, exp_fb,
          f"1000x70 spread {spread}, planes one pixel past a 16-byte boundary")


# ---- 8. in a frame loop ----------------------------------------------------------------------------------------------------

def test_in_a_frame_loop(par, oracle, T):
    """The graybox scene under two tinted ranged lights: render_device and quantize on one stream with no host wait
    between; the frame has more than 256 colours (why the call exists); row blocks dither as the whole frame; the
    renderer's retained frame and statistics are as without the quantise calls."""
    import torch
    from test_gpu_light_range import scene
    from test_gpu_light_tints import COLOUR, TINTS, expected
    from test_gpu_lights_graph import Planes
    from test_gpu_parity import ALL, assert_planes_equal
    from test_gpu_relight import LIT, KEPT, expect, relight_in_place, set_state

    sc = scene("graybox", par, oracle, T)
    params = sc.params
    W, H = params.width, params.height
    assert (W, H) == (480, 320)
    which, radii, tints = [3, 6], [200, 300], TINTS[:2]
    lights, exp, _ = expected(T, sc, which, radii, tints, COLOUR, "graybox, two tinted ranged lights")
    fb = exp["fb"]
    n_colours = len(np.unique(fb.view(np.uint32) & 0xFFFFFF))
    assert n_colours > 256, f"the frame should hold more than 256 colours, has {n_colours}"

    ramp = par.palette_ramp(params, 8)
    assert ramp.tobytes() == Q.ramp_array(T, params, 8).tobytes() and len(ramp) == 33
    background = exp["palidx"] == 0xFF
    assert background.sum() > 1000
    d0 = Q.distances(params, ramp, fb, None, 0)
    index0, fb0 = Q.model(params, ramp, fb, None, 0)
    assert (index0[background] == 32).all() and (d0[background, 32] == 0).all(), "background -> the ramp's last entry"
    index32, fb32 = Q.model(params, ramp, fb, None, 32)
    assert (index32 != index0).any()

    d_ramp = torch.from_numpy(ramp.view(np.uint8).copy()).cuda()
    n = W * H
    planes = {k: torch.full((n * b,), GUARD, dtype=torch.uint8, device="cuda")
              for k, b in (("i0", 1), ("f0", 4), ("i32", 1), ("i32_blocks", 1), ("f32_blocks", 4))}
    ptr = {k: v.data_ptr() for k, v in planes.items()}
    stream = torch.cuda.Stream()
    out = Planes(params, ALL)
    torch.cuda.synchronize()
    with sc.renderer(par, par.LIGHTS_RANGED) as r, sc.renderer(par, par.LIGHTS_RANGED) as plain:
        for c in (r, plain):
            c.set_lights(lights)
            c.set_light_tints(T.make_tints(tints))
        s = stream.cuda_stream
        r.render_device(out.ptrs, flags=par.RENDER_COUNT_RAYS, stream=s)
        # (no host wait: the quantise calls are ordered behind the frame by the stream alone)
        par.quantize(params, d_ramp.data_ptr(), 33, out.ptrs["fb"], (0, H), fb_out=ptr["f0"], index_out=ptr["i0"], stream=s)
        par.quantize(params, d_ramp.data_ptr(), 33, out.ptrs["fb"], (0, H), index_out=ptr["i32"], spread=32, stream=s)
        for r0, r1 in ((0, 120), (120, 320)):  # two row blocks; 120 is a bin row
            par.quantize(params, d_ramp.data_ptr(), 33, out.ptrs["fb"] + 4 * r0 * W, (r0, r1),
                         fb_out=ptr["f32_blocks"] + 4 * r0 * W, index_out=ptr["i32_blocks"] + r0 * W, spread=32, stream=s)
        stream.synchronize()
        assert_planes_equal(out.host(T), exp, ALL, "the frame itself")
        host = {k: v.cpu().numpy() for k, v in planes.items()}
        assert np.array_equal(host["i0"], index0), "index plane, spread 0"
        assert (host["i0"][background] == 32).all()
        assert host["f0"].tobytes() == fb0.tobytes(), "quantised frame, spread 0"
        assert np.array_equal(host["i32"], index32), "index plane, spread 32"
        assert np.array_equal(host["i32_blocks"], host["i32"]), "two row blocks against the whole frame"
        assert host["f32_blocks"].tobytes() == fb32.tobytes(), "quantised frame of two row blocks, spread 32"

        # the renderer: statistics and the retained frame as without the quantise calls
        plain_out = Planes(params, ALL)
        plain.render_device(plain_out.ptrs, flags=par.RENDER_COUNT_RAYS, stream=s)
        stream.synchronize()
        a, b = r.stats(), plain.stats()
        for field in ("entities", "bin_insertions", "shadow_rays", "occupied_columns", "overflow_columns"):
            assert getattr(a, field) == getattr(b, field), field
        assert a.shadow_rays > 0
        which_b, radii_b, tints_b = [0, 7, 2], [0, 150, 250], TINTS[2:5]
        lights_b, exp_b, _ = expect(T, sc, which_b, radii_b, tints_b, "graybox relit", COLOUR)
        assert exp_b["fb"].tobytes() != exp["fb"].tobytes()
        set_state(par, T, r, lights_b, radii_b, tints_b)
        got = relight_in_place(r, out, stream, T)
        assert_planes_equal(got, exp_b, LIT, "relit after the quantise calls")
        assert_planes_equal(got, exp, KEPT, "relit after the quantise calls: gbuf and palidx stay")
        # and the relit frame quantised in place, on its stream
        par.quantize(params, d_ramp.data_ptr(), 33, out.ptrs["fb"], (0, H), fb_out=out.ptrs["fb"], spread=32, stream=s)
        stream.synchronize()
        assert out.host(T)["fb"].tobytes() == Q.model(params, ramp, exp_b["fb"], None, 32)[1].tobytes()
        r.stats()


# ---- 9. host form --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [None, (5, 18)])
def test_host_form_equals_the_device_path(par, T, rows):
    for n_colors, spread in ((17, 37), (256, 0), (1, 255)):
        params, palette, fb = case1_inputs(T, 37, 23, rows, n_colors)
        exp_index, exp_fb = Q.model(params, palette, fb, rows, spread)
        dev = run(par, T, params, palette, fb, rows, spread)
        keep = fb.copy()
        got = par.quantize_host(params, palette, fb, rows=rows, spread=spread, planes=("index", "fb"))
        assert fb.tobytes() == keep.tobytes()
        assert got["index"].tobytes() == dev["index"].tobytes() == exp_index.tobytes()
        assert got["fb"].tobytes() == dev["fb"].tobytes() == exp_fb.tobytes()
        only = par.quantize_host(params, palette, fb, rows=rows, spread=spread)
        assert set(only) == {"index"} and only["index"].tobytes() == exp_index.tobytes()
        only = par.quantize_host(params, palette, fb, rows=rows, spread=spread, planes=("fb",), device=0)
        assert set(only) == {"fb"} and only["fb"].tobytes() == exp_fb.tobytes()
