"""GPU tests of colour cells (par_quantize_cells_device, par_quantize_cells_host): every index plane, every quantised
frame and every cell plane byte for byte against the contract restated in numpy (cells.model; tests/test_cells_cpu.py
holds it to a per-cell, per-pixel, per-entry loop without a GPU). The shapes are the smallest at which each mechanism of
the kernel can go wrong: a lane takes four consecutive pixels of a cell's row, a cell 16, 32 or 64 lanes and a workgroup
the 16, 8 or 4 cells side by side, so 1 x 1 is one live pixel of one lane, 8 x 8 one whole cell, 9 x 9 has edge cells one
pixel wide and one pixel high, 37 x 23 is ragged in both directions (a lane's four pixels hang over the right edge by
three) and is taken whole and in the row blocks its height admits, 37 x 40 has a block in its middle, and 131 x 67 is
more than one workgroup a cell row at every cell size. The (S, K) pairs go round the search's unroll by eight and its
tail, round the pairing of sub-palettes (odd S) and up to S = 256; random frames make the cells of a wavefront choose
different sub-palettes, S = 1 and the 16 x 16 cells make them choose one, which are the two forms of the second search.

Every plane is carved out of a guard-filled tensor (Carved of test_gpu_quantize.py) and the guards are checked after every
call."""
import importlib

import numpy as np
import pytest

import cells as CM
import palette as P
import present as PR
import quantize as Q
from test_gpu_pattern import OUTPUTS
from test_gpu_quantize import Carved, check

pytestmark = pytest.mark.gpu

POISON = 0xEE  # (Carved's guard byte: what a cell plane holds before a call)


@pytest.fixture(scope="module")
def cells(par):
    return importlib.import_module("pixel-art-raytracer_amd.cells")


class Planes:
    """The carved device planes of one call. shifts: elements past a 16-byte boundary of the source and fb_out, bytes past
    one of index_out and cell_out."""

    def __init__(self, T, params, palette, cell, fb, rows, want=("index", "fb"), in_place=False, with_cells=True,
                 shifts=(0, 0, 0, 0)):
        r0, r1 = rows or (0, params.height)
        n = (r1 - r0) * params.width
        assert len(fb) == n
        gcx, gcy = CM.grid(params, cell, rows)
        self.T, self.rows = T, (r0, r1)
        self.pal = Carved(4 * len(palette), 4, palette)
        self.src = Carved(4 * n, 4 * shifts[0], fb)
        self.dst = self.src if in_place else (Carved(4 * n, 4 * shifts[1]) if "fb" in want else None)
        self.idx = Carved(n, shifts[2]) if "index" in want else None
        self.cel = Carved(gcx * gcy, shifts[3]) if with_cells else None
        self.palette = palette

    def call(self, cells, params, n_sub, sub_size, cell, spread, stream=None):
        cells.quantize_cells(params, self.pal.ptr, n_sub, sub_size, cell, self.src.ptr, self.rows,
                             fb_out=self.dst.ptr if self.dst else None, index_out=self.idx.ptr if self.idx else None,
                             cell_out=self.cel.ptr if self.cel else None, spread=spread, stream=stream)

    def results(self):
        out = {"src": self.src.host(self.T.COLOR)}
        for name, plane in (("palette", self.pal), ("source", self.src), ("fb_out", self.dst), ("index_out", self.idx),
                            ("cell_out", self.cel)):
            assert plane is None or plane.guards_intact(), f"{name}: bytes outside the plane were written"
        assert self.pal.host(self.T.COLOR).tobytes() == self.palette.tobytes(), "the palette was written"
        if self.dst is not None:
            out["fb"] = self.dst.host(self.T.COLOR)
        if self.idx is not None:
            out["index"] = self.idx.host(np.uint8)
        if self.cel is not None:
            out["cells"] = self.cel.host(np.uint8)
        return out


def run(cells, T, params, palette, n_sub, sub_size, cell, fb, rows, spread, **kw):
    """One par_quantize_cells_device call on carved device planes, with every guard byte checked."""
    import torch
    planes = Planes(T, params, palette, cell, fb, rows, **kw)
    torch.cuda.synchronize()
    planes.call(cells, params, n_sub, sub_size, cell, spread)
    torch.cuda.synchronize()
    return planes.results()


def check_all(got, fb, exp, tag, in_place=False):
    check(got, fb, exp[0], exp[1], tag, in_place)
    if "cells" in got:
        bad = np.nonzero(got["cells"] != exp[2])[0]
        assert len(bad) == 0, f"{tag}: cell_out differs at {len(bad)} cells, first {bad[:4]}"


def inputs(T, w, h, rows, n_entries, seed=0):
    rng = np.random.default_rng(9000 + 1000 * w + n_entries + seed)
    params = T.default_params(w, h)
    r0, r1 = rows or (0, h)
    return params, Q.random_colors(T, rng, n_entries), Q.random_colors(T, rng, (r1 - r0) * w)


# ---- 1. frames, cells, (S, K), spreads, outputs ----------------------------------------------------------------------

FRAMES = [(1, 1, None), (8, 8, None), (9, 9, None), (37, 23, None), (37, 23, (8, 16)), (37, 23, (16, 23)),
          (37, 40, (16, 32)), (131, 67, None)]
SK = [(1, 1), (1, 256), (256, 1), (2, 2), (4, 4), (8, 4), (7, 9), (16, 16), (65, 3), (120, 2)]
SPREADS = [0, 24]


@pytest.mark.parametrize("w,h,rows", FRAMES)
def test_frames_cells_and_sub_palettes(cells, T, w, h, rows):
    assert 131 > 16 * 8 and all(n * k <= 256 for n, k in SK)
    admitted = [cell for cell in CM.CELLS if CM.admits(rows, h, cell)]
    assert len(admitted) == (2 if rows == (8, 16) else 4)
    several = 0
    for cell in admitted:
        for n_sub, sub_size in SK:
            params, palette, fb = inputs(T, w, h, rows, n_sub * sub_size)
            for spread in SPREADS:
                exp = CM.model(params, palette, n_sub, sub_size, cell, fb, rows, spread)
                several += len(np.unique(exp[2])) > 1
                for want, in_place in (OUTPUTS if spread else OUTPUTS[:1]):
                    tag = f"{w}x{h} rows {rows} cells {cell} S {n_sub} K {sub_size} spread {spread} {want} in place {in_place}"
                    check_all(run(cells, T, params, palette, n_sub, sub_size, cell, fb, rows, spread, want=want,
                                  in_place=in_place), fb, exp, tag, in_place)
                got = run(cells, T, params, palette, n_sub, sub_size, cell, fb, rows, spread, with_cells=False)
                assert "cells" not in got
                check_all(got, fb, exp, f"{w}x{h} rows {rows} cells {cell} S {n_sub} K {sub_size} spread {spread} no cell_out")
    if w > 16:
        assert several > len(admitted) * len(SPREADS) * 4, "the inputs should let more than one sub-palette win"


# ---- 2. alignment and bounds ----------------------------------------------------------------------------------------

def test_alignment_and_bounds(cells, T):
    """The source at every 16-byte phase with the outputs at matching and at mismatched phases: exact results, and no
    byte outside a plane written (run checks the guards round all of them)."""
    params, palette, fb = inputs(T, 37, 23, None, 28, seed=3)
    for cell in ((8, 8), (16, 16)):
        exp = CM.model(params, palette, 7, 4, cell, fb, None, 24)
        for s in range(4):
            for f, i, c in ((s, s, s), ((s + 1) & 3, 3 * s + 1, s + 5), ((s + 2) & 3, 4 * s + 2, 7), (0, 15 - s, 2 * s + 1)):
                got = run(cells, T, params, palette, 7, 4, cell, fb, None, 24, shifts=(s, f, i, c))
                check_all(got, fb, exp, f"cells {cell}: source +{s}, fb_out +{f}, index_out +{i}, cell_out +{c}")
            got = run(cells, T, params, palette, 7, 4, cell, fb, None, 24, want=("index", "fb"), in_place=True,
                      shifts=(s, s, s + 1, 3))
            check_all(got, fb, exp, f"cells {cell}: source +{s} in place", in_place=True)
    blk = fb[16 * 37:23 * 37]
    exp = CM.model(params, palette, 7, 4, (8, 16), blk, (16, 23), 24)
    for shifts in ((1, 1, 3, 1), (3, 2, 1, 2), (2, 2, 2, 3)):
        check_all(run(cells, T, params, palette, 7, 4, (8, 16), blk, (16, 23), 24, shifts=shifts), blk, exp,
                  f"rows (16, 23) at {shifts}")


# ---- 3. the crafted cells of test_cells_cpu.py ----------------------------------------------------------------------

def test_crafted_cells(cells, T):
    from test_cells_cpu import CRAFTED, crafted
    cases = crafted(T)
    for name in CRAFTED:
        params, palette, n_sub, sub_size, cell, fb, spread, (index, plane) = cases[name]
        exp = CM.model(params, palette, n_sub, sub_size, cell, fb, None, spread)
        assert np.array_equal(exp[0], index) and np.array_equal(exp[2], plane)
        check_all(run(cells, T, params, palette, n_sub, sub_size, cell, fb, None, spread), fb, exp, name)


# ---- 4. the consequences -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", CM.CELLS)
def test_one_sub_palette_is_quantise_on_the_same_buffers(par, cells, T, cell):
    import torch
    for K, spread in ((9, 0), (17, 24), (256, 24), (1, 0)):
        params, palette, fb = inputs(T, 37, 23, None, K, seed=4)
        a = Planes(T, params, palette, cell, fb, None, shifts=(1, 1, 3, 0))
        torch.cuda.synchronize()
        par.quantize(params, a.pal.ptr, K, a.src.ptr, (0, 23), fb_out=a.dst.ptr, index_out=a.idx.ptr, spread=spread)
        torch.cuda.synchronize()
        plain = a.results()
        assert plain["index"].tobytes() == Q.model(params, palette, fb, None, spread)[0].tobytes()
        a.idx.t.fill_(0xEE)
        a.dst.t.fill_(0xEE)
        torch.cuda.synchronize()
        a.call(cells, params, 1, K, cell, spread)
        torch.cuda.synchronize()
        got = a.results()
        assert got["index"].tobytes() == plain["index"].tobytes() and got["fb"].tobytes() == plain["fb"].tobytes(), (K, spread)
        assert not got["cells"].any()


def test_duplicated_sub_palettes_never_win(cells, T):
    rng = np.random.default_rng(91)
    params = T.default_params(37, 23)
    a, b = Q.random_colors(T, rng, 4), Q.random_colors(T, rng, 4)
    for cell in ((8, 8), (16, 8)):
        fb, drawn = CM.near_sub_palettes(T, rng, params, np.concatenate([a, b]), 2, 4, cell, 6)
        assert len(np.unique(drawn)) == 2
        single = run(cells, T, params, np.concatenate([a, b]), 2, 4, cell, fb, None, 24)
        assert len(np.unique(single["cells"])) == 2
        doubled = run(cells, T, params, np.concatenate([a, b, a, b]), 4, 4, cell, fb, None, 24)
        for k in ("index", "fb", "cells"):
            assert doubled[k].tobytes() == single[k].tobytes(), (cell, k)
        check_all(doubled, fb, CM.model(params, np.concatenate([a, b, a, b]), 4, 4, cell, fb, None, 24), f"doubled, {cell}")


def test_cells_of_a_sub_palettes_entries_and_drawn_near_them(cells, T):
    rng = np.random.default_rng(92)
    params = T.default_params(93, 75)
    for cell in CM.CELLS:
        palette = Q.random_colors(T, rng, 8 * 4)
        fb, drawn = CM.near_sub_palettes(T, rng, params, palette, 8, 4, cell, 0)
        got = run(cells, T, params, palette, 8, 4, cell, fb, None, 0)
        assert np.array_equal(got["cells"], drawn) and got["fb"].tobytes() == fb.tobytes()
        fb, drawn = CM.near_sub_palettes(T, rng, params, palette, 8, 4, cell, 6)
        exp = CM.model(params, palette, 8, 4, cell, fb, None, 0)
        assert len(np.unique(exp[2])) > 4
        check_all(run(cells, T, params, palette, 8, 4, cell, fb, None, 0), fb, exp, f"near sub-palettes, {cell}")


def test_a_row_block_equals_the_whole_frames_rows(cells, T):
    params, palette, fb = inputs(T, 37, 43, None, 32, seed=5)
    for cell in CM.CELLS:
        whole = run(cells, T, params, palette, 8, 4, cell, fb, None, 24)
        gcx = -(-37 // cell[0])
        for r0, r1 in ((0, 16), (16, 32), (32, 43)):
            part = run(cells, T, params, palette, 8, 4, cell, fb[r0 * 37:r1 * 37], (r0, r1), 24, shifts=(r0 & 3, 1, r1 & 3, 1))
            assert np.array_equal(part["index"], whole["index"][r0 * 37:r1 * 37]), (cell, r0, r1)
            assert part["fb"].tobytes() == whole["fb"][r0 * 37:r1 * 37].tobytes(), (cell, r0, r1)
            assert np.array_equal(part["cells"], whole["cells"][r0 // cell[1] * gcx:-(-r1 // cell[1]) * gcx]), (cell, r0, r1)


def test_alpha_takes_no_part_and_passes_through(cells, T):
    rng = np.random.default_rng(93)
    params = T.default_params(37, 23)
    palette = Q.random_colors(T, rng, 16, alpha=(1, 255))
    fb = Q.random_colors(T, rng, 37 * 23)
    exp = CM.model(params, palette, 4, 4, (8, 8), fb, None, 24)
    got = run(cells, T, params, palette, 4, 4, (8, 8), fb, None, 24)
    check_all(got, fb, exp, "alpha")
    assert np.array_equal(got["fb"]["alpha"], fb["alpha"]) and len(np.unique(fb["alpha"])) > 100
    other = fb.copy()
    other["alpha"] = 255 - fb["alpha"]
    flipped = run(cells, T, params, palette, 4, 4, (8, 8), other, None, 24)
    assert np.array_equal(flipped["index"], exp[0]) and np.array_equal(flipped["fb"]["alpha"], other["alpha"])


# ---- 5. a second call, and the call under stream capture -----------------------------------------------------------------

def test_a_second_call_on_the_same_buffers(cells, T):
    import torch
    params, palette, fb = inputs(T, 131, 67, None, 64, seed=6)
    other = inputs(T, 131, 67, None, 64, seed=7)[2]
    for cell in ((8, 8), (16, 16)):
        p = Planes(T, params, palette, cell, fb, None)
        torch.cuda.synchronize()
        p.call(cells, params, 16, 4, cell, 24)
        torch.cuda.synchronize()
        check_all(p.results(), fb, CM.model(params, palette, 16, 4, cell, fb, None, 24), f"first call, {cell}")
        p.src.t[p.src.at:p.src.at + p.src.nbytes] = torch.from_numpy(other.view(np.uint8).copy()).cuda()
        p.call(cells, params, 8, 8, cell, 0)
        torch.cuda.synchronize()
        check_all(p.results(), other, CM.model(params, palette, 8, 8, cell, other, None, 0), f"second call, {cell}")


@pytest.mark.parametrize("cell", [(8, 8), (16, 16)])
def test_captured_and_replayed_on_new_inputs(cells, T, cell):
    """The call captured with torch.cuda.graph in its default, global capture-error mode after one eager run, replayed on
    new frames and new palettes with the outputs poisoned before every replay."""
    import torch
    sets = [inputs(T, 131, 67, None, 240, seed=10 + k) for k in range(3)]
    params = sets[0][0]
    stream = torch.cuda.Stream()
    p = Planes(T, params, sets[0][1], cell, sets[0][2], None)
    torch.cuda.synchronize()

    def load(k):
        for plane, content in ((p.pal, sets[k][1]), (p.src, sets[k][2])):
            plane.t[plane.at:plane.at + plane.nbytes] = torch.from_numpy(content.view(np.uint8).copy()).cuda()
        for plane in (p.dst, p.idx, p.cel):
            plane.t.fill_(POISON)
        p.palette = sets[k][1]
        torch.cuda.synchronize()

    def verify(k, tag):
        stream.synchronize()
        check_all(p.results(), sets[k][2], CM.model(params, sets[k][1], 120, 2, cell, sets[k][2], None, 24), tag)

    load(0)
    p.call(cells, params, 120, 2, cell, 24, stream=stream.cuda_stream)
    verify(0, "eagerly")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        p.call(cells, params, 120, 2, cell, 24, stream=stream.cuda_stream)
    planes = set()
    for k in (1, 2, 0, 1):
        load(k)
        with torch.cuda.stream(stream):
            graph.replay()
        verify(k, f"replay on input set {k}")
        planes.add(p.idx.host(np.uint8).tobytes())
    assert len(planes) == 3


# ---- 6. host form ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [None, (16, 23)])
def test_host_form_equals_the_device_path(cells, T, rows):
    for (n_sub, sub_size), cell, spread in (((7, 9), (8, 8), 24), ((120, 2), (16, 16), 0), ((1, 1), (8, 16), 0)):
        params, palette, fb = inputs(T, 37, 23, rows, n_sub * sub_size, seed=8)
        exp = CM.model(params, palette, n_sub, sub_size, cell, fb, rows, spread)
        dev = run(cells, T, params, palette, n_sub, sub_size, cell, fb, rows, spread)
        keep = fb.copy()
        got = cells.quantize_cells_host(params, palette, n_sub, sub_size, cell, fb, rows=rows, spread=spread,
                                        planes=("index", "fb", "cells"))
        assert fb.tobytes() == keep.tobytes()
        assert got["index"].tobytes() == dev["index"].tobytes() == exp[0].tobytes()
        assert got["fb"].tobytes() == dev["fb"].tobytes() == exp[1].tobytes()
        assert got["cells"].tobytes() == dev["cells"].tobytes() == exp[2].tobytes()
        only = cells.quantize_cells_host(params, palette, n_sub, sub_size, cell, fb, rows=rows, spread=spread)
        assert set(only) == {"index"} and only["index"].tobytes() == exp[0].tobytes()
        only = cells.quantize_cells_host(params, palette, n_sub, sub_size, cell, fb, rows=rows, spread=spread,
                                         planes=("fb",), device=0)
        assert set(only) == {"fb"} and only["fb"].tobytes() == exp[1].tobytes()


# ---- 7. in a frame loop ----------------------------------------------------------------------------------------------------

def test_in_a_frame_loop(par, cells, oracle, T):
    """The graybox scene under two tinted ranged lights: render_device, then reset, count, cut, sum, emit at 16, the
    palette read back once for par_cells_pairs (host arithmetic: 120 pairs), then the cells quantise at 8 x 8 and present
    on the frame's stream. Each plane is the composed models'."""
    import torch
    from test_gpu_light_range import scene
    from test_gpu_light_tints import COLOUR, TINTS, expected
    from test_gpu_lights_graph import Planes as FramePlanes
    from test_gpu_palette import Block, garbage_work
    from test_gpu_parity import ALL, assert_planes_equal

    sc = scene("graybox", par, oracle, T)
    params = sc.params
    W, H = params.width, params.height
    lights, exp, _ = expected(T, sc, [3, 6], [200, 300], TINTS[:2], COLOUR, "graybox, two tinted ranged lights")
    fb = exp["fb"]
    N, CELL = 16, (8, 8)
    fitted, n_entries, _ = P.fit(T, fb, N)
    table = CM.pairs(fitted)
    assert len(table) == 240
    e_index, e_fb, e_cells = CM.model(params, table, 120, 2, CELL, fb, None, 0)
    assert len(np.unique(e_cells)) > 1, "more than one sub-palette wins"
    print(f"fitted entries {n_entries}, sub-palettes that win {len(np.unique(e_cells))} of 120")
    desc = T.make_present_desc(2, 2, order=T.PRESENT_BGRA, width=W)
    e_surface = PR.model(params, desc, None, index=e_index, palette=table)
    gcx, gcy = CM.grid(params, CELL, None)

    stream = torch.cuda.Stream()
    out = FramePlanes(params, ALL)
    block = Block(T, garbage_work(T, 82))
    d_fitted, d_table = Carved(4 * N, 0), Carved(4 * 240, 4)
    index, quantised, chosen = Carved(W * H, 0), Carved(4 * W * H, 0), Carved(gcx * gcy, 1)
    surface = Carved(e_surface.size, 0)
    torch.cuda.synchronize()
    with sc.renderer(par, par.LIGHTS_RANGED) as r:
        r.set_lights(lights)
        r.set_light_tints(T.make_tints(TINTS[:2]))
        s = stream.cuda_stream
        r.render_device(out.ptrs, flags=par.RENDER_COUNT_RAYS, stream=s)
        par.palette_reset(block.ptr, stream=s)
        par.palette_count(params, out.ptrs["fb"], (0, H), block.ptr, stream=s)
        par.palette_cut(block.ptr, N, stream=s)
        par.palette_sum(params, out.ptrs["fb"], (0, H), block.ptr, stream=s)
        par.palette_emit(block.ptr, N, d_fitted.ptr, stream=s)
        stream.synchronize()  # (the one host wait: the pairs are host arithmetic on the 16 fitted entries)
        got_fitted = d_fitted.host(T.COLOR)
        assert got_fitted.tobytes() == fitted.tobytes(), "the fitted palette"
        got_table = cells.cells_pairs(got_fitted)
        assert got_table.tobytes() == table.tobytes()
        d_table.t[d_table.at:d_table.at + d_table.nbytes] = torch.from_numpy(got_table.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        cells.quantize_cells(params, d_table.ptr, 120, 2, CELL, out.ptrs["fb"], (0, H), fb_out=quantised.ptr,
                             index_out=index.ptr, cell_out=chosen.ptr, stream=s)
        par.present(params, desc, surface.ptr, (0, H), index=index.ptr, d_palette=d_table.ptr, n_colors=240, stream=s)
        stream.synchronize()
        assert_planes_equal(out.host(T), exp, ALL, "the frame itself")
        for plane in (d_fitted, d_table, index, quantised, chosen, surface):
            assert plane.guards_intact()
        assert d_table.host(T.COLOR).tobytes() == table.tobytes(), "the table was written"
        got_index = index.host(np.uint8)
        bad = np.nonzero(got_index != e_index)[0]
        assert len(bad) == 0, f"index differs at {len(bad)} pixels, first {bad[:4]}"
        assert quantised.host(T.COLOR).tobytes() == e_fb.tobytes(), "the quantised frame"
        assert chosen.host(np.uint8).tobytes() == e_cells.tobytes(), "the cell plane"
        assert surface.host(np.uint8).tobytes() == e_surface.tobytes(), "the presented surface"
        r.stats()
