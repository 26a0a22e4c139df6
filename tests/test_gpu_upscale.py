"""GPU tests of upscale (par_upscale_device, par_upscale_host): every surface byte and every index byte against the
contract restated in numpy (upscale.model; tests/test_upscale_cpu.py holds it to a per-pixel loop without a GPU), the gap
bytes of every row and the guard bytes round every plane included. The shapes are the smallest at which each mechanism of
the kernel can go wrong, not the workload's: a workgroup's tile is 128 x 4 source elements, a lane's group 4 output pixels.

Each case first asserts on the host that its inputs reach the situation it is named for: above all that the rules fire.

Shapes of case 1: a frame of 64 x 16 has no rows (5, 18), so its block is rows (5, 16); 16 x 64 and 37 x 23 take rows
(5, 18). Every frame is scaled whole as well: a block with its halo is compared with those output rows of the whole
frame's."""
import ctypes as C

import numpy as np
import pytest

import present as P
import upscale as U
from test_gpu_quantize import GUARD, Carved

pytestmark = pytest.mark.gpu

KS = (2, 3, 4)


def run(par, T, params, desc, src_rows, rows, fb=None, index=None, palette=None, want=("out", "index"), shifts=(0, 0, 0)):
    """One par_upscale_device call on carved device planes: (the (rows * k, pitch) surface block as it is afterwards, gap
    bytes included (they were filled with the guard), or None; the (rows * k, width * k) index plane, or None), with the
    guard bytes round the source and both outputs checked and the source and the palette unchanged. want: the outputs
    asked for ("index" counts with an index source only). shifts: BYTES past a 16-byte boundary of the source, of `out`
    and of index_out."""
    import torch
    r0, r1 = rows or (0, params.height)
    s0, s1 = src_rows or (r0, r1)
    k, pitch, _ = U._desc(desc)
    n = (s1 - s0) * params.width
    source = fb if index is None else index
    assert len(source) == n
    src = Carved(source.itemsize * n, shifts[0], source)
    out = Carved((r1 - r0) * k * pitch, shifts[1]) if "out" in want else None
    idx = Carved((r1 - r0) * k * k * params.width, shifts[2]) if "index" in want and index is not None else None
    d_pal = torch.from_numpy(palette.view(np.uint8).copy()).cuda() if palette is not None and out is not None else None
    torch.cuda.synchronize()
    par.upscale(params, desc, out.ptr if out else None, (r0, r1), fb=None if index is not None else src.ptr,
                index=src.ptr if index is not None else None, d_palette=d_pal.data_ptr() if d_pal is not None else None,
                n_colors=len(palette) if d_pal is not None else 0, src_rows=(s0, s1), index_out=idx.ptr if idx else None)
    torch.cuda.synchronize()
    assert src.guards_intact(), "bytes outside the source were written"
    assert out is None or out.guards_intact(), "bytes outside the surface were written"
    assert idx is None or idx.guards_intact(), "bytes outside the index plane were written"
    assert src.host(np.uint8).tobytes() == source.tobytes(), "the source was written"
    assert d_pal is None or d_pal.cpu().numpy().tobytes() == palette.tobytes(), "the palette was written"
    return (out.host(np.uint8).reshape((r1 - r0) * k, pitch) if out else None,
            idx.host(np.uint8).reshape((r1 - r0) * k, k * params.width) if idx else None)


def check(got, exp, tag):
    """Byte for byte, the gaps (guard bytes in `exp`) included."""
    assert got.shape == exp.shape, tag
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, f"{tag}: {len(bad)} bytes differ, first (row, byte) {bad[:4].tolist()}"


def check_both(got, exp, tag):
    for g, e, what in zip(got, exp, ("surface", "index plane")):
        assert (g is None) == (e is None), f"{tag}: {what}"
        if g is not None:
            check(g, e, f"{tag}: {what}")


def three_valued(T, rng, w, h, values=(0, 1, 2)):
    """A frame drawn from three colours (two of them differ in alpha only) and an index plane drawn from three values, by
    the same draw, with a palette that the values stay inside unless `values` says otherwise."""
    pick = rng.integers(0, 3, w * h)
    colours = U.three_colors(T, rng)
    assert (colours[0].tobytes()[:3] == colours[1].tobytes()[:3]) and colours["alpha"][0] != colours["alpha"][1]
    assert len(np.unique(colours.view(np.uint32))) == 3 and (colours["red"] != colours["blue"]).any()
    return colours[pick], np.array(values, dtype=np.uint8)[pick], P.random_colors(T, rng, 17, alpha=(1, 255))


def assert_rules_fire(index, w, h, k, tag):
    """On the model: at least 5 % of the output elements differ from nearest neighbour, and every sub-position of the
    block but the centre (the inner 2 x 2 for k = 4, which must still differ somewhere) differs in at least 20 pixels."""
    plane = index.reshape(h, w).astype(np.uint32)
    big = U.scaled_elements(plane, k)
    differs = big != np.repeat(np.repeat(plane, k, axis=0), k, axis=1)
    assert differs.mean() >= 0.05, f"{tag}: {differs.mean():.3f} of the output differs from nearest neighbour"
    centre = {2: (), 3: ((1, 1),), 4: ((1, 1), (1, 2), (2, 1), (2, 2))}[k]
    for sy in range(k):
        for sx in range(k):
            count = int(differs[sy::k, sx::k].sum())
            if (sx, sy) not in centre:
                assert count >= 20, f"{tag}: sub-position ({sx}, {sy}) differs in {count} pixels"
            elif k == 4:
                assert count > 0, f"{tag}: sub-position ({sx}, {sy}) never differs"


def kwargs(source, fb, index, palette, w, src_rows=None):
    a, b = (src_rows[0] * w, src_rows[1] * w) if src_rows else (0, None)
    return dict(fb=fb[a:b]) if source == "fb" else dict(index=index[a:b], palette=palette)


# ---- 1. shapes ----------------------------------------------------------------------------------------------------------

FRAMES = [(37, 23, (5, 18)), (64, 16, (5, 16)), (16, 64, (5, 18))]
GAPS = [0, 4, 16, 52]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("w,h,rows", FRAMES)
def test_shapes(par, T, w, h, rows, k):
    rng = np.random.default_rng(1000 * w + h)
    params = T.default_params(w, h)
    fb, index, palette = three_valued(T, rng, w, h)
    assert_rules_fire(index, w, h, k, f"{w}x{h} k {k}")
    # what the shapes are chosen for: a row tail for the narrow path (37 * 3 is no multiple of 4), groups at every phase
    # of a source pixel, pitches on and off the 16-byte phase, index rows on and off the 4-byte phase
    assert (37 * 3) % 4 != 0 and {(4 * g) % 3 for g in range(12)} == {0, 1, 2}
    assert {(4 * w * kk + gap) % 16 == 0 for kk in KS for gap in GAPS} == {True, False}
    src_rows = U.with_halo(rows, h, k)
    assert src_rows[0] == rows[0] - U.halo(k) and (src_rows[1] == rows[1] + U.halo(k) or rows[1] == h)
    # the index plane alone: no palette, and the pitch and the order are not read
    desc = T.make_upscale_desc(k, 2, 7)
    whole = run(par, T, params, desc, None, None, index=index, want=("index",))
    check_both(whole, U.model(params, desc, None, None, index=index), f"{w}x{h} k {k} index_out alone")
    part = run(par, T, params, desc, src_rows, rows, index=index[src_rows[0] * w:src_rows[1] * w], want=("index",))
    assert part[0] is None and np.array_equal(part[1], whole[1][k * rows[0]:k * rows[1]]), "index_out alone: a row block"
    for gap in GAPS:
        for order in (U.RGBA, U.BGRA):
            desc = T.make_upscale_desc(k, 4 * w * k + gap, order)
            for source, want in (("fb", ("out",)), ("index", ("out",)), ("index", ("out", "index"))):
                tag = f"{w}x{h} k {k} gap {gap} order {order} {source} {want}"
                kw = kwargs(source, fb, index, palette, w)
                exp = U.model(params, desc, None, None, guard=GUARD, **kw)
                exp = (exp[0], exp[1] if "index" in want else None)
                whole = run(par, T, params, desc, None, None, want=want, **kw)
                check_both(whole, exp, tag)
                blk = kwargs(source, fb, index, palette, w, src_rows)
                part = run(par, T, params, desc, src_rows, rows, want=want, **blk)
                exp = U.model(params, desc, src_rows, rows, guard=GUARD, **blk)
                check_both(part, (exp[0], exp[1] if "index" in want else None), f"{tag} rows {rows} of {src_rows}")
                for p, f in zip(part, whole):
                    assert p is None or np.array_equal(p, f[k * rows[0]:k * rows[1]]), f"{tag}: rows {rows} of the whole frame's"


# ---- 2. edges and clamps ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_edges_and_clamps(par, T, k):
    rng = np.random.default_rng(20 + k)
    for w, h in ((1, 23), (37, 1), (1, 1), (2, 2)):
        params = T.default_params(w, h)
        fb, index, palette = three_valued(T, rng, w, h)
        desc = T.make_upscale_desc(k, 4 * w * k + 4, U.BGRA)
        for source in ("fb", "index"):
            kw = kwargs(source, fb, index, palette, w)
            check_both(run(par, T, params, desc, None, None, **kw), U.model(params, desc, None, None, guard=GUARD, **kw),
                       f"{w}x{h} k {k} {source}")
    w, h = 37, 23
    params = T.default_params(w, h)
    fb, index, palette = three_valued(T, rng, w, h)
    desc = T.make_upscale_desc(k, 4 * w * k, U.RGBA)
    whole = U.model(params, desc, None, None, index=index, palette=palette, guard=GUARD)
    # a block without a halo in the middle of the frame clamps at its own edges: the model, not the whole frame's rows
    bare = (9, 14)
    kw = kwargs("index", fb, index, palette, w, bare)
    exp = U.model(params, desc, bare, bare, guard=GUARD, **kw)
    assert not np.array_equal(exp[1], whole[1][k * 9:k * 14]), "the clamp at the block's edge should show"
    check_both(run(par, T, params, desc, bare, bare, **kw), exp, f"k {k} rows {bare} without a halo")
    # a halo on one side only, and one row of it where Scale4x wants two
    for src_rows, rows in (((8, 14), (9, 14)), ((9, 15), (9, 14)), ((8, 15), (9, 14))):
        kw = kwargs("fb", fb, index, palette, w, src_rows)
        check_both(run(par, T, params, desc, src_rows, rows, **kw), U.model(params, desc, src_rows, rows, guard=GUARD, **kw),
                   f"k {k} rows {rows} of {src_rows}")
    # a block at each end of the frame, with its halo: those rows of the whole frame's
    for rows in ((0, 3), (h - 3, h), (0, 1), (h - 1, h)):
        src_rows = U.with_halo(rows, h, k)
        kw = kwargs("index", fb, index, palette, w, src_rows)
        got = run(par, T, params, desc, src_rows, rows, **kw)
        check_both(got, U.model(params, desc, src_rows, rows, guard=GUARD, **kw), f"k {k} rows {rows} of {src_rows}")
        for g, f in zip(got, whole):
            assert np.array_equal(g, f[k * rows[0]:k * rows[1]]), f"k {k} rows {rows}: the whole frame's"


# ---- 3. alignment and bounds --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("source", ["fb", "index"])
def test_alignment_and_bounds(par, T, source):
    """The source, `out`, index_out and the pitch at every phase, independently: exact bytes whichever path the kernel
    takes, and no byte outside a plane or inside a gap written (run checks the guards, check the gaps)."""
    rng = np.random.default_rng(3)
    w, h, k = 37, 23, 3
    params = T.default_params(w, h)
    fb, index, palette = three_valued(T, rng, w, h)
    assert_rules_fire(index, w, h, k, "alignment")
    kw = kwargs(source, fb, index, palette, w)
    pitches = [4 * w * k + gap for gap in range(0, 64, 4)]
    assert sorted(p % 16 for p in pitches) == sorted([0, 4, 8, 12] * 4) and {p % 16 for p in pitches[:4]} == {0, 4, 8, 12}
    source_shifts = (0, 4, 8, 12) if source == "fb" else (0, 1, 2, 3)
    for pitch in pitches[:4]:  # every residue mod 16
        for order in (U.RGBA, U.BGRA):
            desc = T.make_upscale_desc(k, pitch, order)
            exp = U.model(params, desc, None, None, guard=GUARD, **kw)
            for s in source_shifts:
                for o in (0, 4, 8, 12):
                    check_both(run(par, T, params, desc, None, None, shifts=(s, o, o // 4), **kw), exp,
                               f"{source} +{s}, out +{o}, index_out +{o // 4}, pitch {pitch}, order {order}")
    # the index plane's word stores: a scaled width that is a multiple of 4, index_out on and off the 4-byte phase
    if source == "index":
        params4 = T.default_params(36, 5)
        _, index4, _ = three_valued(T, rng, 36, 5)
        for kk in KS:
            desc = T.make_upscale_desc(kk, 0, 0)
            exp = U.model(params4, desc, None, None, index=index4)
            assert (36 * kk) % 4 == 0
            for i in (0, 1, 2, 3):
                check_both(run(par, T, params4, desc, None, None, index=index4, want=("index",), shifts=(i, 0, i)), exp,
                           f"36x5 k {kk} index_out +{i}")
    # a block of rows at odd phases
    desc = T.make_upscale_desc(k, pitches[1], U.RGBA)
    blk = kwargs(source, fb, index, palette, w, (4, 19))
    exp = U.model(params, desc, (4, 19), (5, 18), guard=GUARD, **blk)
    for shifts in ((source_shifts[1], 12, 3), (source_shifts[3], 4, 1), (source_shifts[2], 0, 2)):
        check_both(run(par, T, params, desc, (4, 19), (5, 18), shifts=shifts, **blk), exp, f"{source} rows (5, 18) at {shifts}")


# ---- 4. palette ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_colors", [1, 2, 17, 256])
def test_palette_clamps_after_the_comparison(par, T, n_colors):
    rng = np.random.default_rng(40 + n_colors)
    w, h = 37, 23
    params = T.default_params(w, h)
    palette = P.random_colors(T, rng, n_colors, alpha=(1, 255))
    assert (palette["alpha"] != 0).all()
    # three values of which two overrun every palette but the full one, the background's index among them
    values = (0, 200, T.PALIDX_BACKGROUND)
    _, index, _ = three_valued(T, rng, w, h, values)
    beyond = index >= n_colors
    assert (beyond.sum() >= 300 and (index == 255).sum() >= 100) if n_colors < 256 else not beyond.any()
    for k in KS:
        assert_rules_fire(index, w, h, k, f"n_colors {n_colors} k {k}")
        # 200 next to 255 is an edge for the rules: the plane with both set to 255 scales differently
        merged = np.where(index == 200, 255, index).astype(np.uint8)
        desc = T.make_upscale_desc(k, 4 * w * k + 12, U.RGBA)
        exp = U.model(params, desc, None, None, index=index, palette=palette, guard=GUARD)
        exp_merged = U.model(params, desc, None, None, index=merged, palette=palette, guard=GUARD)
        assert not np.array_equal(np.where(exp[1] == 200, 255, exp[1]), exp_merged[1])
        if 2 <= n_colors <= 200:
            assert not np.array_equal(exp[0], exp_merged[0]), "and it shows on the surface, where both are one colour"
        got = run(par, T, params, desc, None, None, index=index, palette=palette)
        check_both(got, exp, f"n_colors {n_colors} k {k}")
        assert set(np.unique(got[1])) <= set(values), "index_out holds raw bytes"
        px = got[0][:, :4 * w * k].reshape(h * k, w * k, 4)
        over = got[1] >= n_colors
        assert (px[over] == palette[-1:].view(np.uint8)).all(), "beyond the palette: its last entry, alpha included"
        check_both(run(par, T, params, T.make_upscale_desc(k, 4 * w * k, U.BGRA), None, None, index=index, palette=palette),
                   U.model(params, T.make_upscale_desc(k, 4 * w * k, U.BGRA), None, None, index=index, palette=palette,
                           guard=GUARD), f"n_colors {n_colors} k {k} BGRA")


@pytest.mark.parametrize("k", KS)
def test_palette_cycling_at_the_scaled_size(par, T, k):
    """par_present_device at (1, 1) on index_out with a rotated palette and a par_params of the scaled width equals the
    upscale call made with that palette."""
    import torch
    rng = np.random.default_rng(44)
    w, h = 37, 23
    params = T.default_params(w, h)
    _, index, palette = three_valued(T, rng, w, h, (2, 9, 16))
    assert len(np.unique(palette.view(np.uint32))) == 17
    desc = T.make_upscale_desc(k, 4 * w * k, U.BGRA)
    first = run(par, T, params, desc, None, None, index=index, palette=palette)
    check_both(first, U.model(params, desc, None, None, index=index, palette=palette, guard=GUARD), "cycle 0")
    big = T.default_params(w * k, h * k)
    d_index = torch.from_numpy(first[1].copy()).cuda()
    before = first[0]
    for turn in range(1, 4):
        rotated = np.roll(palette, turn)
        again = run(par, T, params, desc, None, None, index=index, palette=rotated, want=("out",))[0]
        d_pal = torch.from_numpy(rotated.view(np.uint8).copy()).cuda()
        shown = torch.full((h * k * 4 * w * k,), GUARD, dtype=torch.uint8, device="cuda")
        par.present(big, T.make_present_desc(1, 1, 4 * w * k, P.BGRA), shown.data_ptr(), (0, h * k), index=d_index.data_ptr(),
                    d_palette=d_pal.data_ptr(), n_colors=17)
        torch.cuda.synchronize()
        check(shown.cpu().numpy().reshape(again.shape), again, f"cycle {turn}")
        assert (again != before).any(), f"cycle {turn} should differ from the one before"
        before = again


# ---- 5. against present -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_distinct_neighbours_give_presents_surface(par, T, k):
    """Where no two of a pixel's four neighbours are equal no rule fires: the surface is par_present_device's at (k, k),
    both computed on the GPU."""
    import torch
    rng = np.random.default_rng(5)
    w, h = 37, 23
    params = T.default_params(w, h)
    index = ((np.arange(w)[None, :] + 2 * np.arange(h)[:, None]) % 5).astype(np.uint8).reshape(-1)
    grid = index.reshape(h, w).astype(np.int32)
    assert (grid[:, :-2] != grid[:, 2:]).all() and (grid[:-2] != grid[2:]).all()  # left-right, up-down
    assert (grid[:-1, :-1] != grid[1:, 1:]).all() and (grid[:-1, 1:] != grid[1:, :-1]).all()  # up-left, ..., down-right
    palette = P.random_colors(T, rng, 5, alpha=(1, 255))
    fb = palette[index]
    for source in ("fb", "index"):
        for order in (U.RGBA, U.BGRA):
            pitch = 4 * w * k + 8
            kw = kwargs(source, fb, index, palette, w)
            got = run(par, T, params, T.make_upscale_desc(k, pitch, order), None, None, want=("out",), **kw)[0]
            src = torch.from_numpy(np.ascontiguousarray(kw.get("fb", kw.get("index"))).view(np.uint8).copy()).cuda()
            d_pal = torch.from_numpy(palette.view(np.uint8).copy()).cuda()
            shown = torch.full((h * k * pitch,), GUARD, dtype=torch.uint8, device="cuda")
            if source == "fb":
                par.present(params, T.make_present_desc(k, k, pitch, order), shown.data_ptr(), (0, h), fb=src.data_ptr())
            else:
                par.present(params, T.make_present_desc(k, k, pitch, order), shown.data_ptr(), (0, h), index=src.data_ptr(),
                            d_palette=d_pal.data_ptr(), n_colors=5)
            torch.cuda.synchronize()
            check(got, shown.cpu().numpy().reshape(got.shape), f"k {k} {source} order {order}")


# ---- 6. several workgroups and tile seams -------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,k", [(1000, 70, 2), (1000, 70, 4), (300, 40, 3)])
def test_several_workgroups_and_tile_seams(par, T, w, h, k):
    rng = np.random.default_rng(6)
    params = T.default_params(w, h)
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    # long diagonal edges both ways, so that rules fire across every seam of the 128 x 4 tiles
    index = (((x + y) // 7 + (x - y + h) // 5) % 3).astype(np.uint8).reshape(-1)
    colours = U.three_colors(T, rng)
    fb = colours[index]
    palette = P.random_colors(T, rng, 33, alpha=(1, 255))
    assert w > 2 * 128 and h > 8 * 4, "several tiles each way"
    plane = index.reshape(h, w).astype(np.uint32)
    differs = U.scaled_elements(plane, k) != np.repeat(np.repeat(plane, k, axis=0), k, axis=1)
    per_source = differs.reshape(h, k, w, k).any(axis=(1, 3))
    for seam in range(128, w, 128):  # a rule fires in the columns on both sides of every seam
        assert per_source[:, seam - 1].any() and per_source[:, seam].any(), seam
    for seam in range(4, h, 4):
        assert per_source[seam - 1].any() and per_source[seam].any(), seam
    desc = T.make_upscale_desc(k, 4 * w * k, U.BGRA)
    assert int(desc["pitch"][0]) % 16 == 0
    for source in ("fb", "index"):
        kw = kwargs(source, fb, index, palette, w)
        exp = U.model(params, desc, None, None, guard=GUARD, **kw)
        check_both(run(par, T, params, desc, None, None, **kw), exp, f"{w}x{h} k {k} {source}")
        check_both(run(par, T, params, desc, None, None, shifts=(0, 4, 1), **kw), exp,
                   f"{w}x{h} k {k} {source}, out one word past a 16-byte boundary")


# ---- 7. in a frame loop -------------------------------------------------------------------------------------------------

def test_in_a_frame_loop(par, oracle, T):
    """The graybox scene under two tinted ranged lights: render_device, outline in place, quantize and the upscale calls on
    one stream with no host wait between; the surfaces equal the model applied to the models of the earlier stages; two
    row blocks with their halo written into one surface equal the whole frame's; the renderer's statistics and a
    following relit frame are as they are without the calls."""
    import torch
    import outline as O
    import quantize as Q
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
    style_values = (4, 128, 320)
    style = T.make_outline_style(*style_values)
    edge, outlined = O.model(params, style_values, exp["gbuf"], (0, H), exp["fb"], (0, H))
    assert (outlined.view(np.uint32) != exp["fb"].view(np.uint32)).sum() > 100, "the lines should show"
    ramp = par.palette_ramp(params, 8)
    assert len(ramp) == 33
    index = Q.model(params, ramp, outlined, None, 32)[0]
    assert len(np.unique(index)) > 8
    desc_i = T.make_upscale_desc(3, order=U.BGRA, width=W)
    desc_f = T.make_upscale_desc(2, order=U.RGBA, width=W)
    exp_i, exp_plane = U.model(params, desc_i, None, None, index=index, palette=ramp)
    exp_f, _ = U.model(params, desc_f, None, None, fb=outlined)
    assert exp_i.shape == (3 * H, 12 * W) and exp_f.shape == (2 * H, 8 * W) and exp_plane.shape == (3 * H, 3 * W)
    assert (exp_i != P.model(params, T.make_present_desc(3, 3, 12 * W, P.BGRA), None, index=index, palette=ramp)).any()
    assert (exp_f != P.model(params, T.make_present_desc(2, 2, 8 * W, P.RGBA), None, fb=outlined)).any(), "rules fire"
    cut = 120  # a bin row: where a sharded frame is cut

    d_ramp = torch.from_numpy(ramp.view(np.uint8).copy()).cuda()
    planes = {k: torch.full((n,), GUARD, dtype=torch.uint8, device="cuda")
              for k, n in (("index", W * H), ("from_index", exp_i.size), ("from_fb", exp_f.size), ("plane", exp_plane.size),
                           ("from_index_blocks", exp_i.size), ("from_fb_blocks", exp_f.size))}
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
        # (no host wait: every later call is ordered behind the frame by the stream alone)
        par.outline(params, style, out.ptrs["gbuf"], (0, H), out.ptrs["fb"], (0, H), fb_out=out.ptrs["fb"], stream=s)
        par.quantize(params, d_ramp.data_ptr(), len(ramp), out.ptrs["fb"], (0, H), index_out=ptr["index"], spread=32, stream=s)
        par.upscale(params, desc_i, ptr["from_index"], (0, H), index=ptr["index"], d_palette=d_ramp.data_ptr(),
                    n_colors=len(ramp), index_out=ptr["plane"], stream=s)
        par.upscale(params, desc_f, ptr["from_fb"], (0, H), fb=out.ptrs["fb"], stream=s)
        for r0, r1 in ((0, cut), (cut, H)):  # two row blocks, each with a halo of one row, into one surface
            s0, s1 = max(0, r0 - 1), min(H, r1 + 1)
            par.upscale(params, desc_i, ptr["from_index_blocks"] + r0 * 3 * 12 * W, (r0, r1), index=ptr["index"] + s0 * W,
                        d_palette=d_ramp.data_ptr(), n_colors=len(ramp), src_rows=(s0, s1), stream=s)
            par.upscale(params, desc_f, ptr["from_fb_blocks"] + r0 * 2 * 8 * W, (r0, r1), fb=out.ptrs["fb"] + 4 * s0 * W,
                        src_rows=(s0, s1), stream=s)
        stream.synchronize()
        frame = out.host(T)
        assert_planes_equal(frame, exp, [k for k in ALL if k != "fb"], "the frame itself")
        assert frame["fb"].tobytes() == outlined.tobytes(), "outlined in place"
        host = {k: v.cpu().numpy() for k, v in planes.items()}
        assert np.array_equal(host["index"], index), "index plane of the outlined frame"
        check(host["from_index"].reshape(exp_i.shape), exp_i, "Scale3x from the index plane, BGRA")
        check(host["plane"].reshape(exp_plane.shape), exp_plane, "Scale3x of the index plane")
        check(host["from_fb"].reshape(exp_f.shape), exp_f, "Scale2x from fb")
        check(host["from_index_blocks"].reshape(exp_i.shape), exp_i, "two row blocks from the index plane")
        check(host["from_fb_blocks"].reshape(exp_f.shape), exp_f, "two row blocks from fb")

        # the renderer: statistics and the retained frame as without the calls
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
        assert_planes_equal(got, exp_b, LIT, "relit after the upscale calls")
        assert_planes_equal(got, exp, KEPT, "relit after the upscale calls: gbuf and palidx stay")
        r.stats()


# ---- 8. host form -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("source", ["fb", "index"])
def test_host_form_equals_the_device_path(par, T, source, k):
    rng = np.random.default_rng(8)
    w, h = 37, 23
    params = T.default_params(w, h)
    fb, index, palette = three_valued(T, rng, w, h, (1, 200, 255))  # two beyond the palette
    for rows in (None, (5, 18)):
        r0, r1 = rows or (0, h)
        src_rows = U.with_halo((r0, r1), h, k)
        kw = kwargs(source, fb, index, palette, w, src_rows)
        keep = {key: v.copy() for key, v in kw.items()}
        for gap in (0, 12):
            desc = T.make_upscale_desc(k, 4 * w * k + gap, U.BGRA)
            exp = U.model(params, desc, src_rows, (r0, r1), guard=GUARD, **kw)
            dev = run(par, T, params, desc, src_rows, (r0, r1), **kw)
            check_both(dev, exp, f"device path, gap {gap}")
            got = par.upscale_host(params, desc, rows=(r0, r1), src_rows=src_rows, want_index=source == "index", **kw)
            surface, plane = got if source == "index" else (got, None)
            assert surface.shape == ((r1 - r0) * k, 4 * w * k + gap) and surface.dtype == np.uint8
            assert np.array_equal(surface[:, :4 * w * k], dev[0][:, :4 * w * k]), f"host form against the device path, gap {gap}"
            assert (surface[:, 4 * w * k:] == 0).all(), "the binding's zeros in the gap"
            assert plane is None or np.array_equal(plane, dev[1])
            # the C call on arrays of the caller's: the gap bytes stay as they are
            mine = np.full(exp[0].shape, GUARD, dtype=np.uint8)
            mine_plane = np.full(((r1 - r0) * k, w * k), GUARD, dtype=np.uint8) if source == "index" else None
            rc = par.lib().par_upscale_host(C.byref(params), 0, T.ptr(desc), T.ptr(kw.get("fb")), T.ptr(kw.get("index")),
                                            T.ptr(kw.get("palette")), len(palette) if source == "index" else 0,
                                            src_rows[0], src_rows[1], r0, r1, T.ptr(mine), T.ptr(mine_plane))
            assert rc == 0
            check_both((mine, mine_plane), exp, f"host form, gap {gap}: the model, the gap bytes untouched")
            for key, v in kw.items():
                assert v.tobytes() == keep[key].tobytes(), f"{key} was written"
    if source == "index":  # the index plane alone
        desc = T.make_upscale_desc(k, 0, 0)
        got = par.upscale_host(params, desc, index=index, want_index=True)
        assert got[0] is None and np.array_equal(got[1], U.model(params, desc, None, None, index=index)[1])
