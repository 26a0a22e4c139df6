"""GPU tests of fitted palettes (par_palette_reset / count / cut / sum / emit _device, par_palette_fit_host): the work
block byte for byte against the contract restated in numpy (palette.py; tests/test_palette_cpu.py holds it to a per-cell
loop and to big integers without a GPU). The shapes are the smallest at which each mechanism of the kernels can go wrong.

The work block and every plane are carved out of guard-filled tensors (Carved of test_gpu_quantize.py); the work block
sits 8 bytes past a 16-byte boundary; the guards are checked after every call. Each case first asserts on the host that
its inputs reach the situation it is named for.

The count and the sum kernel's constants (par_palette.hip): a workgroup takes PX_PER_ROUND = PALETTE_PX_PER_ROUND pixels
in one round while that gives at most TARGET_WGS = PALETTE_TARGET_WGS workgroups, and more rounds beyond. The two large
frames here are sized by them: 515 x 257 is 33 workgroups of one round that add into the same cells, and 1025 x 1025, a
little over PX_PER_ROUND * TARGET_WGS pixels (about a million), is the smallest kind of plane that takes two rounds."""
import numpy as np
import pytest

import palette as P
import quantize as Q
from test_gpu_quantize import Carved
from test_palette_cpu import crafted_histograms, crafted_sums

pytestmark = pytest.mark.gpu

PX_PER_ROUND = 4096
TARGET_WGS = 256
BIG = (515, 257)  # width, height: 132 355 pixels, one round
HUGE = (1025, 1025)  # 1 050 625 pixels, two rounds


class Block:
    """A par_palette_work on the device, 8 bytes past a 16-byte boundary, uploaded from a host block."""

    def __init__(self, T, work):
        self.T = T
        self.c = Carved(T.PALETTE_WORK.itemsize, 8, work.view(np.uint8))
        assert self.c.ptr % 16 == 8
        self.ptr = self.c.ptr

    def host(self):
        return self.c.host(np.uint8).copy().view(self.T.PALETTE_WORK)

    def check(self, exp, tag, fields=("hist", "sums", "lut", "n_entries", "reserved")):
        import torch
        torch.cuda.synchronize()
        assert self.c.guards_intact(), f"{tag}: bytes outside the work block were written"
        got = self.host()
        for f in fields:
            bad = np.nonzero((got[f][0] != exp[f][0]).reshape(-1))[0]
            assert len(bad) == 0, f"{tag}: {f} differs at {len(bad)} places, first {bad[:4]}: " \
                                  f"{got[f][0].reshape(-1)[bad[:4]]} for {exp[f][0].reshape(-1)[bad[:4]]}"
        return got


def garbage_work(T, seed):
    """A block of random bytes: what a call must leave alone shows."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, T.PALETTE_WORK.itemsize, dtype=np.uint8).view(T.PALETTE_WORK).copy()


def source(T, fb, shift):
    """The frame block on the device, `shift` pixels past a 16-byte boundary."""
    return Carved(4 * len(fb), 4 * shift, fb)


def pass_over(par, which, params, src, rows, block):
    (par.palette_count if which == "count" else par.palette_sum)(params, src.ptr, rows, block.ptr)


def model_pass(which, work, fb):
    (P.count if which == "count" else P.sums)(work, fb)


# ---- reset ----------------------------------------------------------------------------------------------------------

def test_reset_zeroes_the_whole_block(par, T):
    block = Block(T, garbage_work(T, 1))
    par.palette_reset(block.ptr)
    block.check(P.new_work(T), "reset")


# ---- count and sum: shapes, phases, accumulation --------------------------------------------------------------------

def frames_37x23(T):
    rng = np.random.default_rng(2)
    fb = Q.random_colors(T, rng, 37 * 23)
    for ch in Q.CHANNELS:  # a coarse lattice, so that cells hold several pixels
        fb[ch] &= 0xC7
    return T.default_params(37, 23), fb


@pytest.mark.parametrize("which", ["count", "sum"])
@pytest.mark.parametrize("rows", [None, (5, 18)])
def test_shapes_and_phases(par, T, which, rows):
    """37 x 23 whole and rows (5, 18), the source at each of the four 16-byte phases; the fields the call does not own
    are random bytes before and the same bytes after, and the ones it owns are added to."""
    params, fb = frames_37x23(T)
    assert (37 * 23) % 4 != 0 and (13 * 37) % 4 != 0
    r0, r1 = rows or (0, 23)
    blk = fb[r0 * 37:r1 * 37]
    for shift in range(4):
        work = garbage_work(T, 10 + shift)
        assert len(np.unique(work["lut"][0])) == 256, "the table should use all 256 byte values"
        exp = work.copy()
        model_pass(which, exp, blk)
        changed = "hist" if which == "count" else "sums"
        assert (exp[changed][0] != work[changed][0]).sum() > (50 if which == "count" else 150)
        block, src = Block(T, work), source(T, blk, shift)
        pass_over(par, which, params, src, (r0, r1), block)
        block.check(exp, f"{which} rows {rows} source +{shift}")
        assert src.guards_intact() and src.host(T.COLOR).tobytes() == blk.tobytes()


@pytest.mark.parametrize("which", ["count", "sum"])
def test_a_frame_of_one_colour(par, T, which):
    """64 x 16 pixels of one colour (alpha varies): whole wavefronts hold one cell, the case that adds once."""
    params = T.default_params(64, 16)
    fb = np.zeros(1024, dtype=T.COLOR)
    fb["red"], fb["green"], fb["blue"] = 31, 127, 200
    fb["alpha"] = np.arange(1024) & 0xFF
    cell = 31 >> 3 | (127 >> 3) << 5 | (200 >> 3) << 10
    assert (P.cells(fb) == cell).all()
    for shift in (0, 1):  # whole wavefronts of whole groups, and the same one pixel off
        work = P.new_work(T)
        work["lut"][0] = np.arange(32768) % 251
        entry = cell % 251
        exp = work.copy()
        model_pass(which, exp, fb)
        if which == "count":
            assert exp["hist"][0][cell] == 1024 and int(exp["hist"][0].astype(np.uint64).sum()) == 1024
        else:
            assert exp["sums"][0][entry].tolist() == [31 * 1024, 127 * 1024, 200 * 1024, 1024]
            assert int((exp["sums"][0] != 0).sum()) == 4
        block, src = Block(T, work), source(T, fb, shift)
        pass_over(par, which, params, src, (0, 16), block)
        block.check(exp, f"{which} one colour source +{shift}")
    if which == "sum":
        # one entry, several colours in its cell: a wavefront of one entry that is not of one colour
        fb["red"] = 24 + (np.arange(1024) % 8)
        fb["blue"] = 200 + (np.arange(1024) // 8) % 8
        assert (P.cells(fb) == cell).all() and len(np.unique(fb.view(np.uint32) & 0xFFFFFF)) == 64
        work = P.new_work(T)
        work["lut"][0] = np.arange(32768) % 251
        exp = work.copy()
        model_pass(which, exp, fb)
        block, src = Block(T, work), source(T, fb, 0)
        pass_over(par, which, params, src, (0, 16), block)
        block.check(exp, "sum one entry, 64 colours")


@pytest.mark.parametrize("size", [BIG, HUGE], ids=["one round", "two rounds"])
@pytest.mark.parametrize("which", ["count", "sum"])
def test_many_workgroups_add_into_the_same_cells(par, T, which, size):
    W, H = size
    n = W * H
    if size == BIG:
        assert 32 * PX_PER_ROUND < n < 33 * PX_PER_ROUND
    else:
        assert PX_PER_ROUND * TARGET_WGS < n < PX_PER_ROUND * TARGET_WGS + PX_PER_ROUND and n < 1.01 * (1 << 20)
    rng = np.random.default_rng(3)
    params = T.default_params(W, H)
    fb = Q.random_colors(T, rng, n)
    for ch in Q.CHANNELS:
        fb[ch] &= 0xC7  # 64 cells, eight values of a channel in each
    fb[1000:1000 + 300] = fb[1000]  # and a run of one colour across a wavefront's end
    cells = P.cells(fb)
    slice_px = PX_PER_ROUND * (1 if size == BIG else 2)
    for at in range(0, n - slice_px, slice_px):
        assert len(np.unique(cells[at:at + slice_px])) == 64, "every workgroup's slice should hold every cell"
    for shift in (0, 3):
        work = garbage_work(T, 30 + shift)
        exp = work.copy()
        model_pass(which, exp, fb)
        block, src = Block(T, work), source(T, fb, shift)
        pass_over(par, which, params, src, (0, H), block)
        block.check(exp, f"{which} {W}x{H} source +{shift}")


def test_count_adds_to_what_it_finds_and_wraps(par, T):
    params, fb = frames_37x23(T)
    cells = P.cells(fb)
    work = P.new_work(T)
    rng = np.random.default_rng(4)
    work["hist"][0] = rng.integers(0, 1 << 32, 32768, dtype=np.uint64).astype(np.uint32)
    wrapped = int(cells[0])
    work["hist"][0][wrapped] = 0xFFFFFFFF
    exp = work.copy()
    P.count(exp, fb)
    assert exp["hist"][0][wrapped] == int((cells == wrapped).sum()) - 1, "the preset cell should wrap"
    block, src = Block(T, work), source(T, fb, 0)
    par.palette_count(params, src.ptr, (0, 23), block.ptr)
    block.check(exp, "count onto preset counts")


def test_sum_adds_to_sums_above_32_bits(par, T):
    params, fb = frames_37x23(T)
    rng = np.random.default_rng(5)
    work = garbage_work(T, 6)
    work["sums"][0] = rng.integers(1 << 32, 1 << 62, (256, 4), dtype=np.uint64)
    work["sums"][0][3] = 0xFFFFFFFFFFFFFFFF  # (a row that wraps if a pixel maps to entry 3)
    exp = work.copy()
    P.sums(exp, fb)
    assert (exp["sums"][0] >> np.uint64(32) != 0).sum() > 900
    block, src = Block(T, work), source(T, fb, 2)
    par.palette_sum(params, src.ptr, (0, 23), block.ptr)
    block.check(exp, "sum onto preset sums")


@pytest.mark.parametrize("which", ["count", "sum"])
def test_row_blocks_and_frames_in_turn(par, T, which):
    """Two row blocks counted in turn equal the whole frame; two different frames in turn equal their concatenation."""
    params, fb = frames_37x23(T)
    other = np.roll(fb, 101)
    other["red"] ^= 0x80
    start = P.new_work(T)
    start["lut"][0] = garbage_work(T, 7)["lut"][0]
    whole = start.copy()
    model_pass(which, whole, fb)
    block = Block(T, start)
    srcs = [source(T, fb[:5 * 37], 1), source(T, fb[5 * 37:], 2)]
    pass_over(par, which, params, srcs[0], (0, 5), block)
    pass_over(par, which, params, srcs[1], (5, 23), block)
    block.check(whole, f"{which}: two row blocks")
    both = whole.copy()
    model_pass(which, both, other)
    concat = start.copy()
    model_pass(which, concat, np.concatenate([fb, other]))
    assert both.tobytes() == concat.tobytes() != whole.tobytes()
    src = source(T, other, 0)
    pass_over(par, which, params, src, (0, 23), block)
    block.check(both, f"{which}: a second frame")
    assert all(s.guards_intact() for s in srcs + [src])


# ---- cut ----------------------------------------------------------------------------------------------------------------

CUTS = [(name, n) for name, (_, ns) in crafted_histograms().items() for n in ns]


@pytest.fixture(scope="module")
def histograms():
    return crafted_histograms()


@pytest.mark.parametrize("name,n_colors", CUTS, ids=[f"{name}-{n}" for name, n in CUTS])
def test_cut(par, T, histograms, name, n_colors):
    """The histogram uploaded straight into the block; lut, n_entries and sums hold random bytes before. (That each
    histogram reaches its situation is asserted in test_palette_cpu.py, from the same model.)"""
    hist = histograms[name][0]
    work = garbage_work(T, 40)
    work["hist"][0] = hist
    exp = work.copy()
    P.cut(exp, n_colors)
    occupied = int((hist != 0).sum())
    assert int(exp["n_entries"][0]) == min(n_colors, occupied) and not exp["sums"][0].any()
    assert exp["reserved"].tobytes() == work["reserved"].tobytes() and work["sums"][0].all()
    if occupied:
        assert len(np.unique(exp["lut"][0])) == min(n_colors, occupied)
    block = Block(T, work)
    par.palette_cut(block.ptr, n_colors)
    got = block.check(exp, f"cut {name} at {n_colors}")
    assert np.array_equal(got["hist"][0], hist)


def test_the_cut_names_cover_the_situations():
    names = {name for name, _ in CUTS}
    assert {"all zero", "one cell", "fewer cells than n_colors", "equal extents on red and green",
            "equal extents on three axes", "two regions of equal extent and population", "a median exactly on 2 cum = n",
            "a last bin that outweighs the rest", "populations above 32 bits", "full random"} <= names
    assert {n for name, n in CUTS if name == "300 cells"} == {1, 2, 255, 256}


# ---- emit ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_entries,n_colors", [(0, 7), (12, 33), (256, 256), (256, 33), (33, 33), (1, 256), (200, 1)])
def test_emit(par, T, n_entries, n_colors):
    work = crafted_sums(T)
    s = work["sums"][0]
    assert (s[:, 3] == 0).sum() == 2 and s[1, 0] > 1 << 32 and (2 * int(s[0, 0])) % (2 * int(s[0, 3])) == int(s[0, 3])
    work["n_entries"][0] = n_entries
    work["lut"][0] = garbage_work(T, 50)["lut"][0]
    exp = P.emit(T, work, n_colors)
    block = Block(T, work)
    out = Carved(4 * n_colors, 4)
    par.palette_emit(block.ptr, n_colors, out.ptr)
    block.check(work, f"emit {n_entries} of {n_colors}")  # the block is only read
    assert out.guards_intact(), "more than n_colors entries were written"
    got = out.host(T.COLOR)
    assert got.tobytes() == exp.tobytes(), (got[:8], exp[:8])
    m = min(n_entries, n_colors)
    if 0 < m < n_colors:
        assert got[m:].tobytes() == got[:1].tobytes() * (n_colors - m)
    if m == 0:
        assert not got.view(np.uint8).any()


# ---- in a frame loop ----------------------------------------------------------------------------------------------------

def test_in_a_frame_loop(par, oracle, T):
    """The graybox scene under two tinted ranged lights: render_device, then reset, count, cut, sum, emit and quantize
    on one stream with no host wait between. The palette, n_entries and the index plane are the model's; the renderer's
    statistics and retained frame are as they are without the calls."""
    import torch
    from test_gpu_light_range import scene
    from test_gpu_light_tints import COLOUR, TINTS, expected
    from test_gpu_lights_graph import Planes
    from test_gpu_parity import ALL, assert_planes_equal
    from test_gpu_relight import LIT, KEPT, expect, relight_in_place, set_state

    sc = scene("graybox", par, oracle, T)
    params = sc.params
    W, H = params.width, params.height
    which, radii, tints = [3, 6], [200, 300], TINTS[:2]
    lights, exp, _ = expected(T, sc, which, radii, tints, COLOUR, "graybox, two tinted ranged lights")
    fb = exp["fb"]
    models = {n: P.fit(T, fb, n) for n in (33, 256)}
    assert models[33][1] == 33 and models[256][1] == 122 == int((models[256][2]["hist"][0] != 0).sum())

    stream = torch.cuda.Stream()
    out = Planes(params, ALL)
    blocks = {n: Block(T, garbage_work(T, 60 + n)) for n in models}
    palettes = {n: Carved(4 * n, 0) for n in models}
    indices = {n: Carved(W * H, 0) for n in models}
    torch.cuda.synchronize()
    with sc.renderer(par, par.LIGHTS_RANGED) as r, sc.renderer(par, par.LIGHTS_RANGED) as plain:
        for c in (r, plain):
            c.set_lights(lights)
            c.set_light_tints(T.make_tints(tints))
        s = stream.cuda_stream
        r.render_device(out.ptrs, flags=par.RENDER_COUNT_RAYS, stream=s)
        # (no host wait: the calls are ordered behind the frame and behind one another by the stream alone)
        for n in models:
            b = blocks[n].ptr
            par.palette_reset(b, stream=s)
            par.palette_count(params, out.ptrs["fb"], (0, H), b, stream=s)
            par.palette_cut(b, n, stream=s)
            par.palette_sum(params, out.ptrs["fb"], (0, H), b, stream=s)
            par.palette_emit(b, n, palettes[n].ptr, stream=s)
            par.quantize(params, palettes[n].ptr, n, out.ptrs["fb"], (0, H), index_out=indices[n].ptr, stream=s)
        stream.synchronize()
        assert_planes_equal(out.host(T), exp, ALL, "the frame itself")
        for n, (palette, n_entries, work) in models.items():
            got = blocks[n].check(work, f"the block at {n}")
            assert int(got["n_entries"][0]) == n_entries
            assert palettes[n].guards_intact() and indices[n].guards_intact()
            assert palettes[n].host(T.COLOR).tobytes() == palette.tobytes(), f"palette at {n}"
            index = Q.model(params, palette, fb, None, 0)[0]
            assert index.max() < n_entries, "a padded entry never shows"
            assert np.array_equal(indices[n].host(np.uint8), index), f"index plane at {n}"

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
        set_state(par, T, r, lights_b, radii_b, tints_b)
        got = relight_in_place(r, out, stream, T)
        assert_planes_equal(got, exp_b, LIT, "relit after the palette calls")
        assert_planes_equal(got, exp, KEPT, "relit after the palette calls: gbuf and palidx stay")


# ---- host form ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [None, (5, 18)])
def test_host_form_equals_the_device_path(par, T, rows):
    params, fb = frames_37x23(T)
    r0, r1 = rows or (0, 23)
    blk = fb[r0 * 37:r1 * 37]
    for n_colors in (1, 17, 256):
        palette, n_entries, work = P.fit(T, blk, n_colors)
        block, src, out = Block(T, garbage_work(T, 70)), source(T, blk, 1), Carved(4 * n_colors, 0)
        par.palette_reset(block.ptr)
        par.palette_count(params, src.ptr, (r0, r1), block.ptr)
        par.palette_cut(block.ptr, n_colors)
        par.palette_sum(params, src.ptr, (r0, r1), block.ptr)
        par.palette_emit(block.ptr, n_colors, out.ptr)
        block.check(work, f"device path rows {rows} at {n_colors}")
        assert out.guards_intact() and src.guards_intact()
        keep = blk.copy()
        got, got_entries = par.palette_fit_host(params, blk, n_colors, rows=rows)
        assert blk.tobytes() == keep.tobytes()
        assert got.tobytes() == out.host(T.COLOR).tobytes() == palette.tobytes(), n_colors
        assert got_entries == n_entries == min(n_colors, int((work["hist"][0] != 0).sum()))
    got, got_entries = par.palette_fit_host(params, blk, 17, rows=rows, device=0)
    assert got.tobytes() == P.fit(T, blk, 17)[0].tobytes()
