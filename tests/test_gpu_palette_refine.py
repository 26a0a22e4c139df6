"""GPU tests of refined palettes (par_palette_refine_device, par_palette_refine_host): the palette, the index plane and
the changed count byte for byte against the contract restated in numpy (palette_refine.py;
tests/test_palette_refine_cpu.py holds it to a per-pixel loop without a GPU). The shapes are the smallest at which each
mechanism of the kernels can go wrong.

Every buffer is carved out of a guard-filled tensor (Carved of test_gpu_quantize.py) and the guards are checked after
every call: the source at a chosen 16-byte phase, the palette and the changed count 4 bytes past a 16-byte boundary, the
work block 8 bytes past one and filled with random bytes, d_index on an odd byte. With d_index one byte past a 16-byte
boundary the index bytes of a group share a dword only when the source is one pixel past a boundary: the four phases of
the source take both forms of the index load.

The two large frames are those of test_gpu_palette.py, sized by the count and sum kernels' constants, which the tally
kernel shares: 515 x 257 is 33 workgroups of one round that add into the same tallies, 1025 x 1025 the smallest kind of
plane that takes two rounds."""
import numpy as np
import pytest

import palette as P
import palette_refine as R
import quantize as Q
from test_gpu_palette import BIG, HUGE, PX_PER_ROUND, TARGET_WGS
from test_gpu_quantize import Carved
from test_palette_refine_cpu import EXPECTED_MEDIANS, crafted_clusters

pytestmark = pytest.mark.gpu

UNTOUCHED = -77  # what the changed count holds before a call


class Call:
    """The buffers of one refinement on the device."""

    def __init__(self, T, fb, palette, shift=0, index_shift=1, seed=0):
        rng = np.random.default_rng(1000 + seed)
        self.T, self.fb, self.n_colors = T, fb, len(palette)
        self.src = Carved(4 * len(fb), 4 * shift, fb)
        self.palette = Carved(4 * len(palette), 4, palette)
        self.index = Carved(len(fb), index_shift, np.full(len(fb), 0xAB, dtype=np.uint8))
        self.work = Carved(T.PALETTE_REFINE_WORK.itemsize, 8,
                           rng.integers(0, 256, T.PALETTE_REFINE_WORK.itemsize, dtype=np.uint8))
        self.changed = Carved(4, 4, np.array([UNTOUCHED], dtype=np.int32))
        assert self.work.ptr % 16 == 8 and self.index.ptr % 16 == index_shift and self.src.ptr % 16 == 4 * shift

    def run(self, par, params, rows, iterations, with_changed=True, stream=0):
        par.palette_refine_device(params, self.src.ptr, rows, self.palette.ptr, self.n_colors, iterations, self.index.ptr,
                                  self.work.ptr, self.changed.ptr if with_changed else None, stream=stream)

    def results(self, tag):
        """(palette, index, changed) after a wait, every guard checked and the source as it was."""
        import torch
        torch.cuda.synchronize()
        for name in ("src", "palette", "index", "work", "changed"):
            assert getattr(self, name).guards_intact(), f"{tag}: bytes outside {name} were written"
        assert self.src.host(self.T.COLOR).tobytes() == self.fb.tobytes(), f"{tag}: the source was written"
        return self.palette.host(self.T.COLOR), self.index.host(np.uint8), int(self.changed.host(np.int32)[0])

    def check(self, exp, tag):
        palette, index, changed = self.results(tag)
        assert palette.tobytes() == exp[0].tobytes(), f"{tag}: palette {palette[:8]} for {exp[0][:8]}"
        bad = np.nonzero(index != exp[1])[0]
        assert len(bad) == 0, f"{tag}: index differs at {len(bad)} places, first {bad[:4]}: {index[bad[:4]]} for {exp[1][bad[:4]]}"
        assert changed == exp[2], f"{tag}: changed {changed} for {exp[2]}"


def lattice_frame(T, rng, n):
    fb = Q.random_colors(T, rng, n)
    for ch in Q.CHANNELS:  # a coarse lattice: 512 colours, so that equal neighbours and equal values around a rank occur
        fb[ch] &= 0xC7
    return fb


# ---- shapes, phases, rounds -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("rows", [None, (5, 18)])
def test_shapes_and_phases(par, T, rows, iterations):
    rng = np.random.default_rng(41)
    params = T.default_params(37, 23)
    fb = lattice_frame(T, rng, 37 * 23)
    assert (37 * 23) % 4 != 0 and (13 * 37) % 4 != 0
    r0, r1 = rows or (0, 23)
    blk = fb[r0 * 37:r1 * 37]
    palette = Q.random_colors(T, rng, 7)
    exp = R.refine(T, params, blk, (r0, r1), palette, iterations)
    assert exp[2] > 0 and exp[0].tobytes() != palette.tobytes() and len(np.unique(exp[1])) > 3
    words = []
    for shift in range(4):
        call = Call(T, blk, palette, shift, seed=shift)
        lead = shift  # pixels that do not exist before pixel 0: a whole group starts at pixel 4 g - lead
        words.append((call.index.ptr - lead) % 4 == 0)
        call.run(par, params, (r0, r1), iterations)
        call.check(exp, f"rows {rows}, {iterations} rounds, source +{shift}")
    assert sorted(words) == [False, False, False, True], "both forms of the index load should be taken"


def test_a_frame_of_one_colour(par, T):
    """64 x 16 pixels of one colour (alpha varies): whole wavefronts hold one index and one colour, the case that adds
    once. One pixel off, no wavefront does."""
    params = T.default_params(64, 16)
    fb = np.zeros(1024, dtype=T.COLOR)
    fb["red"], fb["green"], fb["blue"] = 31, 127, 200
    fb["alpha"] = np.arange(1024) & 0xFF
    palette = np.array([(200, 10, 10, 1), (40, 120, 190, 2), (41, 120, 190, 3)], dtype=T.COLOR)
    exp = R.refine(T, params, fb, None, palette, 2)
    assert (exp[1] == 1).all() and exp[2] == 0
    assert exp[0].tolist() == [(200, 10, 10, 1), (31, 127, 200, 255), (41, 120, 190, 3)]
    for shift, index_shift in ((0, 1), (1, 1), (0, 0), (3, 3)):
        call = Call(T, fb, palette, shift, index_shift)
        call.run(par, params, (0, 16), 2)
        call.check(exp, f"one colour, source +{shift}, index +{index_shift}")
        call = Call(T, fb, palette, shift, index_shift)
        call.run(par, params, (0, 16), 1)
        call.check(R.refine(T, params, fb, None, palette, 1), f"one colour, one round, source +{shift}")
    # two colours of one entry in runs of 128 and of 3: wavefronts of one index that are not of one colour, and lanes
    # whose four pixels merge in part
    for run in (128, 3):
        fb["red"] = np.where((np.arange(1024) // run) % 2, 31, 33)
        exp = R.refine(T, params, fb, None, palette, 1)
        assert (exp[1] == 1).all()
        call = Call(T, fb, palette, 0, 0)
        call.run(par, params, (0, 16), 1)
        call.check(exp, f"two colours in runs of {run}")


@pytest.mark.parametrize("name", sorted(EXPECTED_MEDIANS))
def test_crafted_clusters(par, T, name):
    """The situations of the selection as tiny frames (that each reaches its situation is asserted in
    test_palette_refine_cpu.py, from the same frames)."""
    params, fb, palette, medians = crafted_clusters(T)[name]
    exp = R.refine(T, params, fb, None, palette, 1)
    assert exp[2] == len(medians)
    for shift in (0, 2):
        call = Call(T, fb, palette, shift)
        call.run(par, params, (0, 1), 1)
        call.check(exp, f"{name}, source +{shift}")


# ---- many workgroups ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [BIG, HUGE], ids=["one round", "two rounds"])
def test_many_workgroups_add_into_the_same_tallies(par, T, size):
    W, H = size
    n = W * H
    if size == BIG:
        assert 32 * PX_PER_ROUND < n < 33 * PX_PER_ROUND
    else:
        assert PX_PER_ROUND * TARGET_WGS < n < PX_PER_ROUND * TARGET_WGS + PX_PER_ROUND
    rng = np.random.default_rng(42)
    params = T.default_params(W, H)
    fb = lattice_frame(T, rng, n)
    fb[1000:1000 + 300] = fb[1000]  # a run of one colour across a wavefront's end
    palette = Q.random_colors(T, rng, 7)
    exp = R.refine(T, params, fb, None, palette, 2)
    slice_px = PX_PER_ROUND * (1 if size == BIG else 2)
    for at in range(0, n - slice_px, slice_px):
        assert len(np.unique(exp[1][at:at + slice_px])) == 7, "every workgroup's slice should hold every entry"
    for shift in (0, 3):
        call = Call(T, fb, palette, shift, seed=shift)
        call.run(par, params, (0, H), 2)
        call.check(exp, f"{W}x{H} source +{shift}")


# ---- the ends of the argument ranges, and what is optional ----------------------------------------------------------------

@pytest.mark.parametrize("n_colors", [1, 256])
def test_one_entry_and_256_entries(par, T, n_colors):
    rng = np.random.default_rng(43)
    params = T.default_params(37, 23)
    fb = lattice_frame(T, rng, 37 * 23)
    palette = Q.random_colors(T, rng, n_colors)
    for iterations in (1, 16):
        exp = R.refine(T, params, fb, None, palette, iterations)
        if n_colors == 256:
            assert len(np.unique(exp[1])) > 60 and exp[1].max() > 250
        call = Call(T, fb, palette, 1)
        call.run(par, params, (0, 23), iterations)
        call.check(exp, f"{n_colors} entries, {iterations} rounds")


def test_a_null_changed_count_and_a_count_of_zero(par, T):
    rng = np.random.default_rng(44)
    params = T.default_params(37, 23)
    fb = lattice_frame(T, rng, 37 * 23)
    palette = Q.random_colors(T, rng, 7)
    exp = R.refine(T, params, fb, None, palette, 2)
    call = Call(T, fb, palette, 2)
    call.run(par, params, (0, 23), 2, with_changed=False)
    got = call.results("no changed count")
    assert got[0].tobytes() == exp[0].tobytes() and np.array_equal(got[1], exp[1]) and got[2] == UNTOUCHED
    # a frame whose colours are all palette entries is a fixed point: a count of 0, over the -77 that was there
    palette = Q.random_colors(T, rng, 7, alpha=(255, 255))
    fb = palette[rng.integers(0, 7, 37 * 23)]
    fb["alpha"] = rng.integers(0, 256, len(fb))
    exp = R.refine(T, params, fb, None, palette, 3)
    assert exp[2] == 0 and exp[0].tobytes() == palette.tobytes()
    call = Call(T, fb, palette, 0)
    call.run(par, params, (0, 23), 3)
    call.check(exp, "a fixed point")


def test_a_second_call_goes_on_where_the_first_ended(par, T):
    rng = np.random.default_rng(45)
    params = T.default_params(37, 23)
    fb = lattice_frame(T, rng, 37 * 23)
    palette = Q.random_colors(T, rng, 40)
    two, four = R.refine(T, params, fb, None, palette, 2), R.refine(T, params, fb, None, palette, 4)
    assert two[0].tobytes() != four[0].tobytes()
    call = Call(T, fb, palette, 3)
    call.run(par, params, (0, 23), 2)
    call.check(two, "the first two rounds")
    call.run(par, params, (0, 23), 2)  # on the work block as the first call left it
    call.check(four, "two rounds more")


def test_padded_copies_of_entry_0(par, T):
    """A fitted palette padded by emit: the copies get no pixel in the first round and keep the OLD entry 0."""
    from test_palette_cpu import one_colour_per_cell
    rng = np.random.default_rng(46)
    params = T.default_params(37, 23)
    _, fb = one_colour_per_cell(T, rng, 5, 37 * 23)
    for ch in Q.CHANNELS:
        fb[ch] ^= rng.integers(0, 8, len(fb)).astype(np.uint8)  # several colours a cell: the means are not the medians
    fitted, n_entries, _ = P.fit(T, fb, 9)
    assert n_entries == 5 and fitted[5:].tobytes() == fitted[:1].tobytes() * 4
    exp = R.refine(T, params, fb, None, fitted, 1)
    assert exp[1].max() < 5 and exp[0][5:].tobytes() == fitted[5:].tobytes() and exp[2] > 0
    call = Call(T, fb, fitted, 0)
    call.run(par, params, (0, 23), 1)
    call.check(exp, "a padded palette")


# ---- in a frame loop ----------------------------------------------------------------------------------------------------

def test_in_a_frame_loop(par, oracle, T):
    """The graybox scene under two tinted ranged lights: render_device, then reset, count, cut, sum, emit at 33, six rounds
    of refine and quantize on one stream with no host wait between. The palette and both index planes are the model's;
    the renderer's statistics and retained frame are as they are without the calls."""
    import torch
    from test_gpu_light_range import scene
    from test_gpu_light_tints import COLOUR, TINTS, expected
    from test_gpu_lights_graph import Planes
    from test_gpu_palette import Block, garbage_work
    from test_gpu_parity import ALL, assert_planes_equal
    from test_gpu_relight import LIT, KEPT, expect, relight_in_place, set_state

    sc = scene("graybox", par, oracle, T)
    params = sc.params
    W, H = params.width, params.height
    which, radii, tints = [3, 6], [200, 300], TINTS[:2]
    lights, exp, _ = expected(T, sc, which, radii, tints, COLOUR, "graybox, two tinted ranged lights")
    fb = exp["fb"]
    N, ROUNDS = 33, 6
    fitted, n_entries, _ = P.fit(T, fb, N)
    refined = R.refine(T, params, fb, None, fitted, ROUNDS)
    before, after = R.error(params, fitted, fb)[0], R.error(params, refined[0], fb)[0]
    print(f"summed L1 error: {before} as fitted, {after} after {ROUNDS} rounds; changed in the last: {refined[2]}")
    assert (before, after) == (729075, 543232)

    stream = torch.cuda.Stream()
    out = Planes(params, ALL)
    block = Block(T, garbage_work(T, 80))
    call = Call(T, fb[:1], fitted)  # (its palette, work block and changed count; the source is the rendered frame)
    scratch, final = Carved(W * H, 1), Carved(W * H, 0)
    torch.cuda.synchronize()
    with sc.renderer(par, par.LIGHTS_RANGED) as r, sc.renderer(par, par.LIGHTS_RANGED) as plain:
        for c in (r, plain):
            c.set_lights(lights)
            c.set_light_tints(T.make_tints(tints))
        s = stream.cuda_stream
        r.render_device(out.ptrs, flags=par.RENDER_COUNT_RAYS, stream=s)
        # (no host wait: the calls are ordered behind the frame and behind one another by the stream alone)
        par.palette_reset(block.ptr, stream=s)
        par.palette_count(params, out.ptrs["fb"], (0, H), block.ptr, stream=s)
        par.palette_cut(block.ptr, N, stream=s)
        par.palette_sum(params, out.ptrs["fb"], (0, H), block.ptr, stream=s)
        par.palette_emit(block.ptr, N, call.palette.ptr, stream=s)
        par.palette_refine_device(params, out.ptrs["fb"], (0, H), call.palette.ptr, N, ROUNDS, scratch.ptr, call.work.ptr,
                                  call.changed.ptr, stream=s)
        par.quantize(params, call.palette.ptr, N, out.ptrs["fb"], (0, H), index_out=final.ptr, stream=s)
        stream.synchronize()
        assert_planes_equal(out.host(T), exp, ALL, "the frame itself")
        for plane in (call.palette, call.work, call.changed, scratch, final):
            assert plane.guards_intact()
        assert call.palette.host(T.COLOR).tobytes() == refined[0].tobytes(), "the refined palette"
        assert np.array_equal(scratch.host(np.uint8), refined[1]), "the assignment of the last round"
        assert int(call.changed.host(np.int32)[0]) == refined[2]
        assert np.array_equal(final.host(np.uint8), Q.model(params, refined[0], fb, None, 0)[0]), "the index plane"

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
    rng = np.random.default_rng(47)
    params = T.default_params(37, 23)
    fb = lattice_frame(T, rng, 37 * 23)
    r0, r1 = rows or (0, 23)
    blk = fb[r0 * 37:r1 * 37]
    for n_colors, iterations in ((1, 1), (17, 3), (256, 2)):
        palette = Q.random_colors(T, rng, n_colors)
        exp = R.refine(T, params, blk, (r0, r1), palette, iterations)
        call = Call(T, blk, palette, 1)
        call.run(par, params, (r0, r1), iterations)
        call.check(exp, f"device path rows {rows} at {n_colors}")
        keep_fb, keep_palette = blk.copy(), palette.copy()
        got, changed = par.palette_refine_host(params, blk, palette, iterations, rows=rows)
        assert blk.tobytes() == keep_fb.tobytes() and palette.tobytes() == keep_palette.tobytes()
        assert got.tobytes() == call.palette.host(T.COLOR).tobytes() == exp[0].tobytes(), n_colors
        assert changed == exp[2]
    got, changed = par.palette_refine_host(params, blk, palette, 2, rows=rows, device=0)
    assert got.tobytes() == exp[0].tobytes() and changed == exp[2]
    # a null changed_out is allowed
    import ctypes as C
    out = palette.copy()
    rc = par.lib().par_palette_refine_host(C.byref(params), -1, T.ptr(blk), r0, r1, T.ptr(out), len(out), 2, None)
    assert rc == 0 and out.tobytes() == exp[0].tobytes()
